"""Views of frames: a region (x0, y0, w, h) of a frame, reduced by a box mean over s x s blocks, s in {1, 2, 4, 8} (include/rbf.h,
rbf_frame_view_batch, has the normative rule).  View says what a reader wants, view_host is the rule in numpy -- for frames that only
ever exist on the host (an inflated type-1 keyframe, the frame-by-frame route) --, views_device takes the views of frames that lie in
device memory, so that only the views are downloaded.  No filter other than the box mean."""
import ctypes

import numpy as np

SCALES = (1, 2, 4, 8)


def check_region(roi, scale, height, width):
    """(x0, y0, w, h) of a view of (height, width) frames, checked: roi None = the whole frame.  ValueError for a scale outside
    {1, 2, 4, 8}, a region that is no four integers, is empty or leaves the frame."""
    if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, np.integer)) or scale not in SCALES:
        raise ValueError("scale must be one of %r, got %r" % (SCALES, scale))
    if roi is None:
        return 0, 0, int(width), int(height)
    try:
        vals = tuple(roi)
    except TypeError:
        raise ValueError("roi must be (x, y, w, h) or None, got %r" % (roi,)) from None
    if len(vals) != 4 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError("roi must be four integers (x, y, w, h), got %r" % (roi,))
    x0, y0, w, h = (int(v) for v in vals)
    if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > width or y0 + h > height:
        raise ValueError("roi %r: a region of at least one pixel inside a frame of %dx%d" % ((x0, y0, w, h), width, height))
    return x0, y0, w, h


def view_shape(region, scale, frame_shape):
    """The shape of a view of frames of frame_shape ((H, W) or (H, W, C)): (ceil(h/s), ceil(w/s)[, C])."""
    _, _, w, h = region
    return (-(-h // scale), -(-w // scale)) + tuple(frame_shape[2:])


class View:
    """What a reader wants of the frames of a chain or of a decoded keyframe: the region (x0, y0, w, h) -- None: the whole frame, known
    once a frame's shape is (resolve) --, the scale, and for a chain `wanted`: the positions (0-based, ascending) of the frames of the
    run that are viewed at all; None = every frame.  downloads: the byte counts of the frame downloads made under this view (the chain
    blocks' and the decoded keyframes'; list.append is atomic, the lanes share it)."""

    def __init__(self, roi=None, scale=1, wanted=None, downloads=None):
        self.roi, self.scale = roi, scale
        self.wanted = None if wanted is None else [int(p) for p in wanted]
        self.downloads = [] if downloads is None else downloads

    def resolve(self, frame_shape):
        """(x0, y0, w, h) for frames of frame_shape, checked."""
        return check_region(self.roi, self.scale, frame_shape[0], frame_shape[1])

    def shape(self, frame_shape):
        return view_shape(self.resolve(frame_shape), self.scale, frame_shape)

    def at(self, wanted):
        """This view of other positions; the downloads still go to the same list."""
        return View(self.roi, self.scale, wanted, self.downloads)


def view_host(frame, roi=None, scale=1):
    """The view of one (H, W) or (H, W, C) uint8 / uint16 frame in numpy: the twin of the kernels.  Every block's samples are summed in
    64 bits; a block has cnt = bw * bh pixels, and out = (2 * sum + cnt) // (2 * cnt)."""
    a = np.asarray(frame)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3):
        raise ValueError("a view is taken of an (H, W) or (H, W, C) frame of uint8 or uint16, got %r of %s" % (a.shape, a.dtype))
    x0, y0, w, h = check_region(roi, scale, a.shape[0], a.shape[1])
    s = int(scale)
    part = a[y0:y0 + h, x0:x0 + w]
    if s == 1:
        return np.ascontiguousarray(part)
    oh, ow = -(-h // s), -(-w // s)
    rows = np.arange(0, h, s)
    cols = np.arange(0, w, s)
    sums = np.add.reduceat(np.add.reduceat(part.astype(np.int64), rows, axis=0), cols, axis=1)
    bh = np.minimum(s, h - rows).reshape((oh, 1) + (1,) * (a.ndim - 2))
    bw = np.minimum(s, w - cols).reshape((1, ow) + (1,) * (a.ndim - 2))
    cnt = bh * bw
    return ((2 * sums + cnt) // (2 * cnt)).astype(a.dtype)


def views_device(ctx, alloc, frames_ptr, frame_stride, slots, frame_shape, dtype, view):
    """The views of the frames in slots `slots` (ascending) of a device block -- frame i at frames_ptr + i * frame_stride -- as one
    (len(slots),) + view shape array: ONE rbf_frame_view_batch into the block alloc("views", nbytes), one download of exactly the
    views.  The download is recorded in view.downloads."""
    from . import _native as nat
    dtype = np.dtype(dtype)
    H, W = int(frame_shape[0]), int(frame_shape[1])
    C = int(frame_shape[2]) if len(frame_shape) == 3 else 1
    x0, y0, w, h = view.resolve(frame_shape)
    shape = view_shape((x0, y0, w, h), view.scale, frame_shape)
    nbytes = len(slots) * int(np.prod(shape)) * dtype.itemsize
    vb = alloc("views", nbytes)
    idx = (ctypes.c_uint32 * len(slots))(*[int(i) for i in slots])
    nat.check(nat.lib().rbf_frame_view_batch(ctx.handle, frames_ptr, frame_stride, idx, len(slots), W, H, C, dtype.itemsize,
                                             x0, y0, w, h, view.scale, vb.ptr, vb.nbytes))
    view.downloads.append(nbytes)
    return vb.download(nbytes).view(dtype).reshape((len(slots),) + shape)
