"""The opt-in sample codec (ImprovedVideoCompressor(sample_codec="rice")): every stored sample is predicted, the prediction error is mapped
to an unsigned value and written with a chunked Rice code, encoded and decoded on the GPU by csrc/rbf_kernels_rice.h through the C ABI's
rbf_rice_* entries.  There is no CPU codec (tests/sample_codec_ref.py is the numpy reference the tests compare against).

Format (normative, include/rbf.h has the bit layout):
  stream    '<I' N | '<B' B | 3 zero bytes | k[C] | '<H' words[C] | zero pad to 4 bytes | payload ('<I' words), C = ceil(N / 1024)
  mapping   s = (x - pred) mod 2^B read as a B-bit two's-complement value, u = 2s (s >= 0) or -2s - 1
  code      per chunk of 1024 samples one k in [0, B]: k == B stores u; else q = u >> k < 16 is q one-bits, a zero-bit and the k low bits of
            u, q >= 16 is 16 one-bits and the B bits of u

Records of 'BFV2' containers (next to type 1 = zlib keyframe, 2 = inter-frame):
  3 = keyframe     '<III' height, width, itemsize | '<B' channels (0 = a 2-D frame) | '<B' yuv (1 = decode to YUVFrame) | the stream of the
                   H*W*C samples, predicted from the pixel to the left (column 0: the pixel above; the first pixel: 0), per channel
  4 = inter-frame  type 2's bytes ('<B' itemsize + the "f64" wire record) with the stream of the pair's residuals against frame t-1 at the
                   mask's pixels in the value field; value_count = its sample count
  7 = keyframe     within a bound per channel (bounded_keyframes=True; include/rbf.h has the rule): type 3's head | '<B' version = 1 |
                   '<B' n = max(1, channels) | n x '<H' d_c | zero padding to 4 bytes | the stream of the quantised residuals q
"""
import ctypes
import struct

import numpy as np

from . import _native as nat
from .container import INTER_RICE, KEY_NEAR, KEY_RICE  # noqa: F401  (the record types this module's streams travel in)
from .engine import DeviceFrame, rebuild_chain
from .view import views_device
from .frame_codec import YUVFrame, _PlaneDict, frame_data

CHUNK = 1024
_KEY_HEAD = struct.Struct("<IIIBB")
_PLANES = ("y_plane", "u_plane", "v_plane")
NEAR_VERSION = 1


def nchunks(n):
    return (int(n) + CHUNK - 1) // CHUNK


def header_bytes(n):
    """Header, table and padding of a stream of n samples."""
    return (8 + 3 * nchunks(n) + 3) // 4 * 4


def max_stream_bytes(n, bits):
    """The longest a stream of n samples can be: every chunk stored raw (k = B)."""
    full, tail = divmod(int(n), CHUNK)
    return header_bytes(n) + 4 * (full * (CHUNK * bits // 32) + (tail * bits + 31) // 32)


def stream_info(buf):
    """(N, B, the length its table declares) of a sample stream; ValueError when the table does not fit in buf."""
    buf = memoryview(buf).cast("B")
    if len(buf) < 8:
        raise ValueError("sample stream shorter than its 8-byte header")
    n, bits = struct.unpack_from("<IB", buf, 0)
    c = nchunks(n)
    if header_bytes(n) > len(buf):
        raise ValueError("the table of a sample stream of %d chunks runs past its %d bytes" % (c, len(buf)))
    words = np.frombuffer(buf[8 + c:8 + 3 * c], dtype="<u2")
    return n, bits, header_bytes(n) + 4 * int(words.sum(dtype=np.int64))


def key_format(frame):
    """(channels byte, yuv byte) of the type-3 record that carries `frame`, or None when only a zlib keyframe can: samples other than
    uint8 / uint16, more than 4 channels, or a yuv_info whose planes are not the frame's own channels."""
    arr = frame_data(frame)
    if arr.dtype not in (np.uint8, np.uint16) or arr.ndim not in (2, 3) or 0 in arr.shape:
        return None
    H, W, C, _ = nat.frame_geometry(arr)
    if C > 4 or H > 65535 or H * W * C >= 1 << 32:
        return None
    info = getattr(frame, "yuv_info", None)
    if info is None:
        return (0 if arr.ndim == 2 else C), 0
    if not isinstance(frame, YUVFrame) or arr.ndim != 3 or C < 3 or info.get("format") != "YUV444":
        return None
    stored = {k: v for k, v in info.items() if k != "format"}          # (_PlaneDict: only the planes copied out so far)
    if not isinstance(info, _PlaneDict) and set(stored) != set(_PLANES):
        return None
    for key, plane in stored.items():
        if key not in _PLANES or not np.array_equal(np.asarray(plane), arr[..., _PLANES.index(key)]):
            return None
    return C, 1


def key_record(frame, stream):
    """The type-3 record of `frame` around its stream."""
    arr = frame_data(frame)
    channels, yuv = key_format(frame)
    return _KEY_HEAD.pack(arr.shape[0], arr.shape[1], arr.dtype.itemsize, channels, yuv) + bytes(stream)


def parse_key_record(rec):
    """Fields of a type-3 record (height, width, itemsize, channels, yuv, stream); ValueError when they do not agree with each other."""
    if len(rec) < _KEY_HEAD.size + 8:
        raise ValueError("truncated keyframe record")
    h, w, item, channels, yuv = _KEY_HEAD.unpack_from(rec, 0)
    if item not in (1, 2) or channels > 4 or yuv > 1 or h == 0 or w == 0:
        raise ValueError("keyframe record: itemsize %d, %d channels, yuv %d" % (item, channels, yuv))
    stream = memoryview(rec)[_KEY_HEAD.size:]
    n, bits, size = stream_info(stream)
    if n != h * w * max(1, channels) or bits != 8 * item or size != len(stream):
        raise ValueError("keyframe record: a stream of %d %d-bit samples in %d bytes for a %dx%dx%d frame of %d-byte samples"
                         % (n, bits, len(stream), h, w, max(1, channels), item))
    return {"height": h, "width": w, "itemsize": item, "channels": channels, "yuv": yuv, "stream": stream}


def _near_bounds(bounds, n):
    d = [int(v) for v in bounds]
    if len(d) != n or any(not 0 <= v <= 65535 for v in d):
        raise ValueError("a type-7 record carries %d bounds in 0..65535, got %r" % (n, list(bounds)))
    return d


def near_key_record(frame, bounds, stream):
    """The type-7 record of `frame` -- only its shape, dtype and yuv_info are read -- around the stream rbf_rice_encode_intra_near made of
    it under the per-channel `bounds`."""
    arr = frame_data(frame)
    channels, yuv = key_format(frame)
    n = max(1, channels)
    head = _KEY_HEAD.pack(arr.shape[0], arr.shape[1], arr.dtype.itemsize, channels, yuv) + struct.pack("<BB%dH" % n, NEAR_VERSION, n, *_near_bounds(bounds, n))
    return head + b"\0" * (-len(head) % 4) + bytes(stream)


def parse_near_key_record(rec):
    """Fields of a type-7 record (parse_key_record's, and `bounds`: the n per-channel bounds); ValueError for a version other than 1, an n
    other than max(1, channels), non-zero padding, or a stream whose N or B disagrees with the head."""
    if len(rec) < _KEY_HEAD.size + 2:
        raise ValueError("truncated bounded keyframe record")
    h, w, item, channels, yuv = _KEY_HEAD.unpack_from(rec, 0)
    if item not in (1, 2) or channels > 4 or yuv > 1 or h == 0 or w == 0:
        raise ValueError("bounded keyframe record: itemsize %d, %d channels, yuv %d" % (item, channels, yuv))
    version, n = struct.unpack_from("<BB", rec, _KEY_HEAD.size)
    if version != NEAR_VERSION:
        raise ValueError("bounded keyframe record version %d is unknown (this reader knows %d)" % (version, NEAR_VERSION))
    if n != max(1, channels):
        raise ValueError("bounded keyframe record: %d bounds for %d channel(s)" % (n, max(1, channels)))
    off = _KEY_HEAD.size + 2 + 2 * n
    body = off + (-off % 4)
    if len(rec) < body + 8:
        raise ValueError("truncated bounded keyframe record")
    bounds = list(struct.unpack_from("<%dH" % n, rec, _KEY_HEAD.size + 2))
    if any(bytes(rec[off:body])):
        raise ValueError("bounded keyframe record: padding bytes are not zero")
    stream = memoryview(rec)[body:]
    cnt, bits, size = stream_info(stream)
    if cnt != h * w * n or bits != 8 * item or size != len(stream):
        raise ValueError("bounded keyframe record: a stream of %d %d-bit samples in %d bytes for a %dx%dx%d frame of %d-byte samples"
                         % (cnt, bits, len(stream), h, w, n, item))
    return {"height": h, "width": w, "itemsize": item, "channels": channels, "yuv": yuv, "bounds": bounds, "stream": stream}


def _split(raw, sizes):
    out, off = [], 0
    for s in sizes:
        out.append(raw[off:off + int(s)])
        off += int(s)
    return out


class SampleCoder:
    """The sample codec on one library context: device buffers grown on demand (close() returns them)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.bufs = nat.BufferCache(ctx)
        self._buf = self.bufs.get

    def close(self):
        self.bufs.close()

    def encode_frames(self, frames):
        """Type-3 streams of same-shape frames: one upload per frame, ONE rbf_rice_encode_intra, one exact-size download."""
        arrs = [frame_data(f) for f in frames]
        a = arrs[0]
        H, W, C, _ = nat.frame_geometry(a)
        fb = self._buf("frames", a.nbytes * len(arrs))
        for i, x in enumerate(arrs):
            fb.upload(x, i * a.nbytes)
        cap = len(arrs) * max_stream_bytes(H * W * C, 8 * a.dtype.itemsize)
        ob = self._buf("streams", cap)
        sizes = (ctypes.c_uint64 * len(arrs))()
        nat.check(nat.lib().rbf_rice_encode_intra(self.ctx.handle, fb.ptr, a.nbytes, len(arrs), W, H, C, a.dtype.itemsize, ob.ptr, ob.nbytes, sizes))
        return _split(ob.download(sum(sizes)).tobytes(), sizes)

    def encode_near(self, frames_ptr, frame_stride, nframes, indices, width, height, channels, sample_bytes, bounds):
        """Type-7 streams of the frames `indices` (ascending, each < nframes) of a resident dense block, which become their rebuilt frames
        Y IN PLACE (rbf_rice_encode_intra_near): ONE launch sequence, one exact-size download.  bounds: `channels` per-channel bounds."""
        idx = [int(i) for i in indices]
        if not idx or any(not 0 <= i < nframes for i in idx) or any(b <= a for a, b in zip(idx, idx[1:])):
            raise ValueError("frame indices %r: ascending indices inside the block of %d frames" % (idx, nframes))
        d = [int(v) for v in bounds]
        if len(d) != channels or any(v < 0 or v >> 32 for v in d):
            raise ValueError("bounds %r: one non-negative bound for each of the %d channels" % (list(bounds), channels))
        cap = len(idx) * max_stream_bytes(width * height * channels, 8 * sample_bytes)
        ob = self._buf("streams", cap)
        sizes = (ctypes.c_uint64 * len(idx))()
        nat.check(nat.lib().rbf_rice_encode_intra_near(self.ctx.handle, frames_ptr, frame_stride, (ctypes.c_uint32 * len(idx))(*idx), len(idx), width,
                                                       height, channels, sample_bytes, (ctypes.c_uint32 * channels)(*d), ob.ptr, ob.nbytes, sizes))
        return _split(ob.download(sum(sizes)).tobytes(), sizes)

    def encode_inter(self, frames_ptr, frame_stride, nframes, width, height, channels, sample_bytes, masks_ptr, mask_stride, ones):
        """Type-4 streams of the nframes-1 pairs of resident dense frames under their packed masks (rbf_rice_encode_inter): ONE launch
        sequence, one exact-size download.  ones: the masks' set-bit counts."""
        pairs = nframes - 1
        cap = sum(max_stream_bytes(int(o) * channels, 8 * sample_bytes) for o in ones)
        ob = self._buf("streams", cap)
        sizes = (ctypes.c_uint64 * pairs)()
        cnt = (ctypes.c_uint64 * pairs)(*[int(o) for o in ones])
        nat.check(nat.lib().rbf_rice_encode_inter(self.ctx.handle, frames_ptr, frame_stride, nframes, width, height, channels, sample_bytes,
                                                  masks_ptr, mask_stride, cnt, ob.ptr, ob.nbytes, sizes))
        return _split(ob.download(sum(sizes)).tobytes(), sizes)

    def encode_pair(self, prev, curr, mask_packed, ones):
        """The type-4 stream of one pair (the frame-by-frame route's twin of GopCoder.rice_streams)."""
        a, b = np.ascontiguousarray(frame_data(prev)), np.ascontiguousarray(frame_data(curr))
        H, W, C, sb = nat.frame_geometry(a)
        stride = nat.packed_stride(H * W)
        fb = self._buf("pair", 2 * a.nbytes)
        fb.upload(a, 0)
        fb.upload(b, a.nbytes)
        mb = self._buf("pair_mask", stride).upload(nat.mask_rows([mask_packed], H * W))
        return self.encode_inter(fb.ptr, a.nbytes, 2, W, H, C, sb, mb.ptr, stride, [ones])[0]

    def decode_frame_device(self, stream, height, width, channels, itemsize, bounds=None, on_decoded=None):
        """A type-3 stream (bounds: a type-7 stream and its per-channel bounds) decoded into the coder's frame block, where it stays: a
        DeviceFrame -- (H, W) for channels == 0, else (H, W, channels) -- that is valid until this coder decodes its next frame.  Nothing
        is downloaded.  on_decoded(ptr, frame_bytes, 1), optional: called with the frame's device address (engine.rebuild_chain's hook)."""
        C = max(1, channels)
        nbytes = height * width * C * itemsize
        fb = self._buf("frame", nbytes)
        src = np.frombuffer(stream, dtype=np.uint8)
        if bounds is None:
            nat.check(nat.lib().rbf_rice_decode_intra(self.ctx.handle, src.ctypes.data, src.nbytes, width, height, C, itemsize, fb.ptr))
        else:
            d = (ctypes.c_uint32 * C)(*_near_bounds(bounds, C))
            try:
                nat.check(nat.lib().rbf_rice_decode_intra_near(self.ctx.handle, src.ctypes.data, src.nbytes, width, height, C, itemsize, d, fb.ptr))
            except nat.RbfError as e:
                if e.code != nat.RBF_EINVAL:
                    raise
                raise ValueError("corrupt bounded keyframe record: %s" % e) from None      # (the record's bytes are wrong, not the call)
        if on_decoded is not None:
            on_decoded(fb.ptr, nbytes, 1)
        return DeviceFrame(fb.ptr, (height, width) if channels == 0 else (height, width, C), np.uint8 if itemsize == 1 else np.uint16)

    def fetch(self, frame, view=None):
        """A DeviceFrame of this coder's context on the host: the whole frame, or with view (view.View) its view only
        (rbf_frame_view_batch into a view block, one download of exactly the view)."""
        if view is None:
            out = np.empty(frame.nbytes, dtype=np.uint8)
            nat.check(nat.lib().rbf_memcpy_d2h(self.ctx.handle, out.ctypes.data, frame.ptr, frame.nbytes))
            return out.view(frame.dtype).reshape(frame.shape)
        return views_device(self.ctx, self._buf, frame.ptr, frame.nbytes, [0], frame.shape, frame.dtype, view)[0]

    def decode_frame(self, stream, height, width, channels, itemsize, on_decoded=None, view=None):
        """A type-3 stream back to its frame: (H, W) for channels == 0, else (H, W, channels) (rbf_rice_decode_intra).
        on_decoded(ptr, frame_bytes, 1), optional: called with the frame's device address before its download (engine.rebuild_chain's hook).
        view, optional (view.View): the hook first, then the view on the device, then a download of the view only."""
        return self.fetch(self.decode_frame_device(stream, height, width, channels, itemsize, None, on_decoded), view)

    def decode_near_frame(self, stream, height, width, channels, itemsize, bounds, on_decoded=None, view=None):
        """decode_frame for a type-7 stream: the rebuilt frame Y (rbf_rice_decode_intra_near); bounds: the record's per-channel bounds."""
        return self.fetch(self.decode_frame_device(stream, height, width, channels, itemsize, bounds, on_decoded), view)

    def apply_chain(self, base, masks_packed, streams, chunk_frames=64, chunk_bytes=256 << 20, on_rebuilt=None, before_download=None, view=None):
        """engine.apply_chain for type-4 records: frame t = frame t-1 plus the residuals of stream t at mask t's '1' pixels, rebuilt on the
        device in chunks of frames (one upload of the chunk's masks and streams, ONE rbf_rice_apply_inter, one download).  on_rebuilt,
        before_download, view: rebuild_chain's hooks and view; base may be a DeviceFrame of this coder's context.  Returns the frames as
        views of the downloaded chunk blocks (with view: the views of the wanted frames)."""
        if not isinstance(base, DeviceFrame):
            base = np.ascontiguousarray(base)
        H, W, C, sb = nat.frame_geometry(base)
        stride = nat.packed_stride(H * W)

        def rebuild(c0, cnt, fb, mb):
            part = [bytes(s) for s in streams[c0:c0 + cnt]]
            blob = np.frombuffer(b"".join(part), dtype=np.uint8)
            sizes = (ctypes.c_uint64 * cnt)(*[len(s) for s in part])
            nat.check(nat.lib().rbf_rice_apply_inter(self.ctx.handle, blob.ctypes.data, sizes, cnt, W, H, C, sb, mb.ptr, stride, fb.ptr))
        return rebuild_chain(self._buf, base, masks_packed, chunk_frames, chunk_bytes, rebuild, on_rebuilt, before_download, view)
