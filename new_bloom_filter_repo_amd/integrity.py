"""Frame digests: the opt-in check that lets a container prove, without the originals, that the decoder rebuilt exactly the frames the
encoder coded (ImprovedVideoCompressor(frame_digests=True); FLAC's MD5 and FFV1's slice CRCs play the same role).

FD1 (normative: include/rbf.h) is defined over bytes; a frame's bytes are its dense C-order (H, W, C) samples, little-endian.  Three
implementations agree bit for bit: the kernel (csrc/rbf_kernels_digest.h, through rbf_frame_digest_batch: digests_device below), the host
twin in C (csrc/rbf_digest.h: frame_digest_host) and the numpy twin (frame_digest), which is what the tests compare the other two against.

The digests travel in the container's last record (type 5, container.DIGESTS):
  '<B' version = 1 | '<B' algo = 1 (FD1) | '<H' 0 | '<I' count | count x '<Q' digest | '<Q' FD1 of all the bytes in front of it
(build_trailer / parse_trailer; container.split_trailer checks where the record stands and how many frames it covers)."""
import struct

import numpy as np

P1, P2, P3, P4, P5 = (np.uint64(0x9E3779B185EBCA87), np.uint64(0xC2B2AE3D27D4EB4F), np.uint64(0x165667B19E3779F9),
                      np.uint64(0x85EBCA77C2B2AE63), np.uint64(0x27D4EB2F165667C5))
BLOCK = 4096
TRAILER_VERSION, ALGO_FD1 = 1, 1
_HEAD = struct.Struct("<BBHI")
_M64 = (1 << 64) - 1


class IntegrityError(ValueError):
    """A decoded frame does not have the digest its container stores.  frame: its index in the stream; expected: the stored digest;
    got: the digest of what the decoder rebuilt; key_record: the record index of the keyframe its run hangs off."""

    def __init__(self, frame, expected, got, key_record=None):
        self.frame, self.expected, self.got, self.key_record = int(frame), int(expected), int(got), key_record
        super().__init__("frame %d decodes to digest 0x%016X, the container stores 0x%016X (its run hangs off the keyframe in record %s)"
                         % (self.frame, self.got, self.expected, key_record))


def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _round(acc, x):
    return _rotl(acc + x * P2, 31) * P1


def _merge(a, b):
    return (a ^ _round(np.uint64(0), b)) * P1 + P4


def _aval(h):
    h = h ^ (h >> np.uint64(33))
    h = h * P2
    h = h ^ (h >> np.uint64(29))
    h = h * P3
    return h ^ (h >> np.uint64(32))


def _blocks(words, seeds):
    """The hashes of blocks: words uint64 (nb, 512), seeds uint64 (nb,) -> uint64 (nb,)."""
    w = words.reshape(-1, 4, 64, 2)                              # [block, row, lane, half] = w[128 r + 2 l + h]
    with np.errstate(over="ignore"):
        acc = seeds[:, None] + P5 + np.arange(64, dtype=np.uint64)[None, :] * P1
        for r in range(4):
            for h in range(2):
                acc = _round(acc, w[:, r, :, h])
        d = 1
        while d < 64:
            acc = _merge(acc[:, 0::2], acc[:, 1::2])             # the lanes that are multiples of 2d, each with its neighbour d lanes up
            d *= 2
        return _aval(acc[:, 0])


def _as_bytes(data):
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data)
        if a.dtype.byteorder == ">":
            a = a.astype(a.dtype.newbyteorder("<"))
        return a.reshape(-1).view(np.uint8)
    d = getattr(data, "data", None)                              # a YUVFrame
    if isinstance(d, np.ndarray):
        return _as_bytes(d)
    return np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)


def frame_digest(data):
    """FD1 of a frame (its dense C-order samples, little-endian) or of a bytes-like object: the numpy twin, vectorised over blocks and
    lanes.  Returns a Python int."""
    b = _as_bytes(data)
    L = b.size
    while b.size > BLOCK:
        nb = (b.size + BLOCK - 1) // BLOCK
        padded = np.zeros(nb * BLOCK, dtype=np.uint8)
        padded[:b.size] = b
        b = _blocks(padded.view("<u8").reshape(nb, 512), np.arange(nb, dtype=np.uint64)).astype("<u8").view(np.uint8)
    padded = np.zeros(BLOCK, dtype=np.uint8)
    padded[:b.size] = b
    return int(_blocks(padded.view("<u8").reshape(1, 512), np.array([L], dtype=np.uint64))[0])


def frame_digest_host(data):
    """FD1 by the library's host twin (rbf_frame_digest_host: plain C++, no GPU, no context; ctypes drops the GIL, so it runs in host
    thread pools).  Returns a Python int."""
    from . import _native as nat
    b = _as_bytes(data)
    return int(nat.lib().rbf_frame_digest_host(b.ctypes.data if b.size else None, b.size))


def digests_device(ctx, ptr, stride, nframes, frame_bytes, out=None):
    """FD1 of nframes byte ranges [ptr + f*stride, +frame_bytes) of device memory (rbf_frame_digest_batch on ctx's stream) and ONE download
    of 8*nframes bytes: uint64[nframes].  out: a device block (anything with a .ptr) of at least 8*nframes bytes to use (default: a
    temporary one)."""
    from . import _native as nat
    nframes = int(nframes)
    if nframes == 0:
        return np.zeros(0, dtype=np.uint64)
    buf = out if out is not None else ctx.alloc(8 * nframes)
    try:
        nat.check(nat.lib().rbf_frame_digest_batch(ctx.handle, ptr, int(stride), nframes, int(frame_bytes), buf.ptr))
        res = np.empty(nframes, dtype=np.uint64)
        nat.check(nat.lib().rbf_memcpy_d2h(ctx.handle, res.ctypes.data, buf.ptr, 8 * nframes))     # (waits for the stream)
        return res
    finally:
        if out is None:
            buf.free()


# ------------------------------------------------------------------ the trailer record (type 5)
def build_trailer(digests):
    """The body of the DIGESTS record for the frames' digests, in stream order."""
    body = _HEAD.pack(TRAILER_VERSION, ALGO_FD1, 0, len(digests)) + b"".join(struct.pack("<Q", int(d) & _M64) for d in digests)
    return body + struct.pack("<Q", frame_digest(body))


def parse_trailer(body):
    """The digests of a DIGESTS record body; a plain ValueError for anything that is not a whole, undamaged version-1 trailer."""
    body = bytes(body)
    if len(body) < _HEAD.size + 8:
        raise ValueError("unknown record type 5: its %d bytes are shorter than a digest trailer's header and checksum" % len(body))
    version, algo, zero, count = _HEAD.unpack_from(body, 0)
    if version != TRAILER_VERSION:
        raise ValueError("digest trailer version %d is unknown (this reader knows %d)" % (version, TRAILER_VERSION))
    if algo != ALGO_FD1 or zero != 0:
        raise ValueError("digest trailer: algorithm %d, reserved field %d (expected %d and 0)" % (algo, zero, ALGO_FD1))
    if len(body) != _HEAD.size + 8 * count + 8:
        raise ValueError("digest trailer of %d bytes does not hold the %d digests it declares" % (len(body), count))
    (stored,) = struct.unpack_from("<Q", body, len(body) - 8)
    if stored != frame_digest(body[:-8]):
        raise ValueError("digest trailer is damaged: its own checksum does not match")
    return list(struct.unpack_from("<%dQ" % count, body, _HEAD.size))
