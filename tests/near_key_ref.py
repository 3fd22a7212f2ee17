"""Numpy twin of the bounded-error keyframe rule (record type 7; include/rbf.h states it, csrc/rbf_kernels_keyquant.h runs it).  A test
helper: not collected, not part of the package.  quantise() walks the loop as the rule states it -- serially along a row, vectorised over
the rows -- which is what the kernels, who run the rule's closed form (closed_form() here), are held against; the decoder is two cumulative
sums."""
import struct

import numpy as np

import sample_codec_ref as ref

HEAD = struct.Struct("<IIIBB")
VERSION = 1


def as_bounds(bounds, channels):
    """`channels` bounds from one number or a sequence."""
    d = [int(bounds)] * channels if np.ndim(bounds) == 0 else [int(v) for v in bounds]
    assert len(d) == channels and all(0 <= v <= 65535 for v in d), (bounds, channels)
    return d


def _step(x, p, d, bits, trace=None):
    """One step of every row's chain: samples x with predictions p (int64 arrays) -> (q, S)."""
    if d == 0:
        return (x - p) & ((1 << bits) - 1), x.copy()
    t = 2 * d + 1
    e = x - p
    n = np.abs(e) + d
    if trace is not None:
        trace["residues"].setdefault(t, set()).update(int(v) for v in np.unique(n % t))
    q = np.sign(e) * (n // t)
    return q, p + q * t


def quantise(frame, bounds, trace=None):
    """(Y, u, S) of a frame (H, W) or (H, W, C) of uint8 / uint16 under per-channel bounds: the rebuilt frame (the frame's shape and
    dtype), the stream's u values (raster order, channels interleaved) and the integer states (H, W, C).  trace: a dict that receives what
    the inputs exercised (`residues`: per step t the residues of |e| + d mod t that occurred)."""
    a = np.asarray(frame)
    bits = 8 * a.dtype.itemsize
    x = a.astype(np.int64).reshape(a.shape[0], a.shape[1], -1)
    H, W, C = x.shape
    d = as_bounds(bounds, C)
    if trace is not None:
        trace.setdefault("residues", {})
    S = np.zeros_like(x)
    q = np.zeros_like(x)
    for c in range(C):
        p = np.zeros(1, dtype=np.int64)
        for y in range(H):                       # column 0: a chain down the frame
            q[y:y + 1, 0, c], S[y:y + 1, 0, c] = _step(x[y:y + 1, 0, c], p, d[c], bits, trace)
            p = S[y:y + 1, 0, c]
        for i in range(1, W):                    # every row: a chain from its column 0, all rows at once
            q[:, i, c], S[:, i, c] = _step(x[:, i, c], S[:, i - 1, c], d[c], bits, trace)
    top = (1 << bits) - 1
    Y = np.where(np.array(d)[None, None, :] > 0, np.clip(S, 0, top), S & top)
    exact = [c for c in range(C) if d[c] == 0]
    qs = q.copy()
    for c in exact:                              # B-bit two's complement -> signed, for the mapping below
        qs[:, :, c] = np.where(q[:, :, c] >= 1 << (bits - 1), q[:, :, c] - (1 << bits), q[:, :, c])
    u = np.where(qs >= 0, 2 * qs, -2 * qs - 1).reshape(-1)
    assert int(u.max(initial=0)) <= top
    return Y.astype(a.dtype).reshape(a.shape), u, S


def closed_form(frame, bounds):
    """(Y, S) without the loop: the chain starts at 0 and moves in multiples of t, so S = t * floor((X + d) / t)."""
    a = np.asarray(frame)
    x = a.astype(np.int64).reshape(a.shape[0], a.shape[1], -1)
    d = np.array(as_bounds(bounds, x.shape[2]), dtype=np.int64)[None, None, :]
    t = 2 * d + 1
    S = (x + d) // t * t
    return np.minimum(S, np.iinfo(a.dtype).max).astype(a.dtype).reshape(a.shape), S


def stream(frame, bounds, ks=None):
    """(Y, the frame's sample stream)."""
    a = np.asarray(frame)
    Y, u, _ = quantise(a, bounds)
    return Y, ref.encode(u, 8 * a.dtype.itemsize, ks)


def rebuild(u, shape, dtype, bounds):
    """Y from a stream's u values: q = the signed residual, prefix sums of q t down column 0 and along every row, clamp or mask."""
    bits = 8 * np.dtype(dtype).itemsize
    H, W = shape[:2]
    s = ref.from_u(u, bits).reshape(H, W, -1)
    C = s.shape[2]
    d = as_bounds(bounds, C)
    q = np.where(s >= 1 << (bits - 1), s - (1 << bits), s)
    v = q * (2 * np.array(d, dtype=np.int64) + 1)[None, None, :]
    v[:, 0] = np.cumsum(v[:, 0], axis=0)
    S = np.cumsum(v, axis=1)
    top = (1 << bits) - 1
    Y = np.where(np.array(d)[None, None, :] > 0, np.clip(S, 0, top), S & top)
    return Y.astype(dtype).reshape(shape)


def decode(buf, shape, dtype, bounds):
    """Y from a sample stream (the bit-walking reference decoder: short streams)."""
    u, bits = ref.decode(buf)
    assert bits == 8 * np.dtype(dtype).itemsize
    return rebuild(u, shape, dtype, bounds)


def record(frame, bounds, yuv=0, ks=None):
    """(Y, the type-7 record of `frame`)."""
    a = np.asarray(frame)
    channels = 0 if a.ndim == 2 else a.shape[2]
    n = max(1, channels)
    d = as_bounds(bounds, n)
    Y, s = stream(a, d, ks)
    head = HEAD.pack(a.shape[0], a.shape[1], a.dtype.itemsize, channels, yuv) + struct.pack("<BB", VERSION, n) + struct.pack("<%dH" % n, *d)
    head += b"\0" * (-len(head) % 4)
    return Y, head + s


def parse(rec):
    """(height, width, itemsize, channels, yuv, bounds, stream) of a type-7 record; ValueError as the product's parser."""
    rec = bytes(rec)
    if len(rec) < HEAD.size + 2:
        raise ValueError("truncated")
    h, w, item, channels, yuv = HEAD.unpack_from(rec, 0)
    version, n = struct.unpack_from("<BB", rec, HEAD.size)
    if version != VERSION or n != max(1, channels) or channels > 4 or item not in (1, 2) or yuv > 1:
        raise ValueError("bad head")
    off = HEAD.size + 2 + 2 * n
    if len(rec) < off:
        raise ValueError("truncated")
    d = list(struct.unpack_from("<%dH" % n, rec, HEAD.size + 2))
    pad = -off % 4
    if any(rec[off:off + pad]) or len(rec) < off + pad + 8:
        raise ValueError("padding")
    s = rec[off + pad:]
    cnt, bits = struct.unpack_from("<IB", s, 0)
    if cnt != h * w * n or bits != 8 * item:
        raise ValueError("stream does not fit the head")
    c = -(-cnt // ref.CHUNK)
    table = (8 + 3 * c + 3) // 4 * 4
    if len(s) < table or table + 4 * int(np.frombuffer(s, dtype="<u2", count=c, offset=8 + c).sum()) != len(s):
        raise ValueError("the stream's table does not match its length")
    return h, w, item, channels, yuv, d, s


def reciprocal(t):
    """(m, sh) of the kernels' division by an odd step t >= 3: floor(n / t) = (n * m >> 32) >> sh for n < 2^18."""
    L = t.bit_length() - 1
    K = 31 + L
    return ((1 << K) + t - 1) // t, L - 1
