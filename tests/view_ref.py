"""The naive reference of a frame view (include/rbf.h, rbf_frame_view_batch): blocks walked in Python loops, one output sample at a time,
Python integers -- a helper of the view tests (CPU and GPU), written from the rule's text and sharing no code with the package.  The
`rounding` and `ragged_div` keywords build the WRONG views a kernel could compute, for the non-vacuity checks."""
import numpy as np

GEOMETRIES = [(1, 1), (5, 3), (15, 1), (16, 1), (1, 15), (9, 9), (37, 9), (67, 33), (1030, 2)]      # (W, H)
CHANNELS = (1, 3, 4)
DTYPES = (np.uint8, np.uint16)
SCALES = (1, 2, 4, 8)


def view_ref(frame, roi=None, scale=1, rounding="half_up", ragged_div="count"):
    """The view of an (H, W) or (H, W, C) frame.  rounding="floor" and ragged_div="full" (a ragged block divided by s^2) are wrong on
    purpose."""
    a = np.asarray(frame)
    H, W = a.shape[:2]
    x0, y0, w, h = (0, 0, W, H) if roi is None else roi
    assert w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= W and y0 + h <= H and scale in SCALES
    s = scale
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    flat = a.reshape(H, W, -1)
    C = flat.shape[2]
    out = np.zeros((oh, ow, C), dtype=a.dtype)
    for Y in range(oh):
        ys = range(y0 + s * Y, min(y0 + s * Y + s, y0 + h))
        for X in range(ow):
            xs = range(x0 + s * X, min(x0 + s * X + s, x0 + w))
            cnt = len(ys) * len(xs)
            div = cnt if ragged_div == "count" else s * s
            for c in range(C):
                total = sum(int(flat[y, x, c]) for y in ys for x in xs)
                out[Y, X, c] = (2 * total + div) // (2 * div) if rounding == "half_up" else total // div
    return out.reshape((oh, ow) + a.shape[2:])


def view_ref_stack(frames, roi=None, scale=1):
    """view_ref of every frame of a stack of same-shape frames at once: the same walk over the blocks, each block summed over its
    pixels for all frames and channels together (int64) -- what the surface tests hold whole clips against (the CPU test holds it
    against view_ref)."""
    a = np.stack([np.asarray(f) for f in frames])
    F, H, W = a.shape[:3]
    x0, y0, w, h = (0, 0, W, H) if roi is None else roi
    assert w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= W and y0 + h <= H and scale in SCALES
    s = scale
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    flat = a.reshape(F, H, W, -1)
    out = np.zeros((F, oh, ow, flat.shape[3]), dtype=a.dtype)
    for Y in range(oh):
        ya, yb = y0 + s * Y, min(y0 + s * Y + s, y0 + h)
        for X in range(ow):
            xa, xb = x0 + s * X, min(x0 + s * X + s, x0 + w)
            cnt = (yb - ya) * (xb - xa)
            total = flat[:, ya:yb, xa:xb, :].astype(np.int64).sum(axis=(1, 2))
            out[:, Y, X, :] = (2 * total + cnt) // (2 * cnt)
    return out.reshape((F, oh, ow) + a.shape[3:])


def regions(W, H, s):
    """The regions a geometry is swept with at scale s: the whole frame, an odd corner with what is left, and -- where the frame has
    the room -- sides that are and are not multiples of s, hung off odd and even corners."""
    out = [(0, 0, W, H)]
    if W > 1 or H > 1:
        out.append((min(1, W - 1), min(1, H - 1), W - min(1, W - 1), H - min(1, H - 1)))
    for x0, y0, w, h in ((3, 1, 2 * s, s), (1, 2, 2 * s + 1, s + 1), (2, 0, 3 * s - 1, 2 * s), (5, 3, s, 3 * s + 1)):
        if x0 + w <= W and y0 + h <= H:
            out.append((x0, y0, w, h))
    return out


def noise_frame(W, H, C, dtype, seed):
    """A frame of independent uniform samples, (H, W) for C == 1."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, np.iinfo(dtype).max + 1, size=(H, W, C), dtype=np.uint32).astype(dtype)
    return a[:, :, 0] if C == 1 else a
