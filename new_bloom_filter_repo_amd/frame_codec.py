"""Frame-level codecs around the GPU Bloom path.

* FixedVideoCompressor -- the zlib keyframe codec and the YUV frame wrapper the product surface
  uses (fixed_video_compressor.py:15-334).  Plain host Python: keyframes are not on the hot path.
* VideoFrameCompressor -- the inter-frame residual codec (improved_video_compressor.py:768-1027):
  luma residual mask (A1), changed-value gather (A2), Bloom+witness coding of the mask (A3-A5),
  the wire record (A7) and the inverse (A6, A8).  In the reference these methods read
  `self.bloom_compressor`, which nothing ever assigns; here the constructor wires it.

Deliberate, documented divergences from the reference record format:
  - k travels as float64 ('<d'), not float32: with float32 the decoder's activation threshold
    differs from the encoder's and roughly 1 in 130 1080p frames would desynchronise the witness.
    `wire_format="reference"` reproduces the reference bytes exactly (tests pin it to fixture G7).
  - changed values keep the frame dtype (the reference hard-codes uint8, which truncates 16-bit video).
"""
import struct
import zlib

import numpy as np

from . import _native as nat
from .bloom_compressor import BloomFilterCompressor
from .engine import BloomEngine, adaptive_threshold, gather_values, scatter_values


# ----------------------------------------------------------------------------- YUV wrapper
class _PlaneDict(dict):
    """yuv_info of a YUVFrame: 'format' is there from the start, a plane ('y_plane', 'u_plane', 'v_plane') is copied out of the
    interleaved frame the first time it is asked for (the reference copies all three when it wraps a frame,
    fixed_video_compressor.py:292-296; only the keyframe record ever reads them, :64-75 -- three strided 2 MB copies per 1080p frame were
    most of what compress_video / decompress_video cost on the host: round 5's end-to-end profile, git history)."""
    _CHANNEL = {"y_plane": 0, "u_plane": 1, "v_plane": 2}

    def __init__(self, frame):
        super().__init__(format="YUV444")
        self._frame = frame

    def __missing__(self, key):
        if key not in self._CHANNEL:
            raise KeyError(key)
        plane = self[key] = self._frame[:, :, self._CHANNEL[key]].copy()
        return plane

    def __contains__(self, key):
        return key in self._CHANNEL or super().__contains__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default


class YUVFrame:
    """ndarray-like wrapper carrying contiguous copies of the three planes
    (FixedVideoCompressor.add_yuv_info_to_frame, fixed_video_compressor.py:287-334); the copies are made on first use (_PlaneDict)."""

    def __init__(self, frame):
        frame = np.asarray(frame)
        self.data = frame
        self.yuv_info = _PlaneDict(frame)
        self.shape, self.dtype, self.nbytes = frame.shape, frame.dtype, frame.nbytes

    def __array__(self, dtype=None, copy=None):
        return self.data if dtype is None else self.data.astype(dtype)

    def copy(self):
        return YUVFrame(self.data.copy())

    def __getitem__(self, key):
        return self.data[key]

    def __setitem__(self, key, value):
        self.data[key] = value

    def tobytes(self):
        return self.data.tobytes()

    def astype(self, dtype):
        return self.data.astype(dtype)

    def flatten(self):
        return self.data.flatten()

    def reshape(self, *a, **k):
        return self.data.reshape(*a, **k)

    @property
    def size(self):
        return self.data.size

    @property
    def T(self):
        return self.data.T


def frame_data(frame):
    """The ndarray behind a frame (YUVFrame or ndarray)."""
    return frame.data if isinstance(frame, YUVFrame) else np.asarray(frame)


# ----------------------------------------------------------------------------- keyframes
class FixedVideoCompressor:
    """Per-frame zlib-9 codec, byte-compatible with the reference's keyframe record:
    '<III' height width itemsize | '<I' len | zlib(frame) | '<B' has_yuv [| planes ...]."""

    def __init__(self, verbose=True):
        self.verbose = verbose

    def compress_frame(self, frame):
        return self.compress_frame_jobs(frame)()

    def compress_frame_jobs(self, frame, submit=None):
        """The keyframe record as up to four independent zlib-9 jobs -- the interleaved frame and its three planes -- handed to
        `submit(fn) -> future` (default: run inline); returns a callable that waits for them and joins the record.  One code path for the
        byte layout (fixed_video_compressor.py:38-106), whether the jobs run one after the other (compress_frame) or on a pool's threads
        (ImprovedVideoCompressor: a 1080p keyframe is ~0.4 s of zlib-9 in ONE job, the longest thing a 300-frame clip waits for)."""
        if submit is None:
            class _Now:
                def __init__(self, fn):
                    self.value = fn()

                def result(self):
                    return self.value
            submit = _Now
        arr = frame_data(frame)
        head = struct.pack("<III", arr.shape[0], arr.shape[1], arr.dtype.itemsize)
        body = submit(lambda: zlib.compress(arr.tobytes(), level=9))
        has_info = hasattr(frame, "yuv_info")
        planes = []
        if has_info:
            fmt = frame.yuv_info.get("format", "YUV444").encode("utf-8")

            def plane_job(key):
                plane = frame.yuv_info[key]          # (copied out of the interleaved frame on first use, on the job's thread)
                return zlib.compress(plane.tobytes(), level=9), plane.shape
            planes = [submit(lambda key=key: plane_job(key)) for key in ("y_plane", "u_plane", "v_plane")]

        def finish():
            b = body.result()
            out = [head, struct.pack("<I", len(b)), b, struct.pack("<B", 1 if has_info else 0)]
            if has_info:
                out += [struct.pack("<H", len(fmt)), fmt]
                for job in planes:
                    z, shape = job.result()
                    out += [struct.pack("<I", len(z)), z, struct.pack("<II", *shape)]
            return b"".join(out)
        return finish

    def decompress_frame(self, blob):
        """The frame of a keyframe record.  A plain ValueError for a record that is cut short or whose bytes do not inflate to the frame
        its head declares."""
        try:
            return self._decompress_frame(blob)
        except (struct.error, zlib.error, IndexError, UnicodeDecodeError, ZeroDivisionError, MemoryError) as e:
            raise ValueError("damaged keyframe record: %s" % e) from None

    def _decompress_frame(self, blob):
        h, w, item = struct.unpack_from("<III", blob, 0)
        (size,) = struct.unpack_from("<I", blob, 12)
        raw = zlib.decompress(blob[16:16 + size])
        dtype = {1: np.uint8, 2: np.uint16}.get(item, np.float32)
        gray = h * w * item
        if len(raw) > gray and len(raw) % gray == 0:
            # at most four samples per pixel, as in a type-3 record: a damaged itemsize re-reads the same bytes as more samples of
            # fewer bytes, which the frame digest -- taken over bytes -- cannot see
            if len(raw) // gray > 4:
                raise ValueError("keyframe record: %d samples per pixel" % (len(raw) // gray))
            frame = np.frombuffer(raw, dtype=dtype).reshape(h, w, len(raw) // gray)
        else:
            frame = np.frombuffer(raw, dtype=dtype).reshape(h, w)
        # trailer: '<B' has_yuv_info [| '<H' len, format | 3 x ('<I' len, zlib(plane), '<II' shape)]
        # (fixed_video_compressor.py:108-184: a frame written with yuv_info comes back as the wrapper)
        off = 16 + size
        if off >= len(blob) or blob[off] not in (0, 1):
            raise ValueError("keyframe record: its has_yuv byte is %s" % ("missing" if off >= len(blob) else blob[off]))
        if blob[off] == 0 and off + 1 != len(blob):
            raise ValueError("keyframe record: %d bytes behind a frame without planes" % (len(blob) - off - 1))
        if blob[off] == 1:
            off += 1
            (flen,) = struct.unpack_from("<H", blob, off)
            fmt = bytes(blob[off + 2:off + 2 + flen]).decode("utf-8")
            off += 2 + flen
            planes = []
            for _ in range(3):
                (zlen,) = struct.unpack_from("<I", blob, off)
                z = blob[off + 4:off + 4 + zlen]
                ph, pw = struct.unpack_from("<II", blob, off + 4 + zlen)
                off += 12 + zlen
                pdata = zlib.decompress(z)
                # the reference reads the planes as uint8 (fixed_video_compressor.py:155,163,171); planes of 16-bit frames keep the frame dtype
                pdt = np.uint8 if len(pdata) == ph * pw else dtype
                planes.append(np.frombuffer(pdata, dtype=pdt).reshape(ph, pw))
            if off != len(blob):
                raise ValueError("keyframe record: %d bytes behind its third plane" % (len(blob) - off))
            # the STORED planes come back in yuv_info, whatever their shape (a reference record may carry subsampled planes)
            out = YUVFrame.__new__(YUVFrame)
            out.data = frame
            out.shape, out.dtype, out.nbytes = frame.shape, frame.dtype, frame.nbytes
            out.yuv_info = {"format": fmt, "y_plane": planes[0], "u_plane": planes[1], "v_plane": planes[2]}
            return out
        return frame

    def compress_video(self, frames):
        if self.verbose:
            print(f"Compressing {len(frames)} frames")
        return [self.compress_frame(f) for f in frames]

    def decompress_video(self, blobs):
        if self.verbose:
            print(f"Decompressing {len(blobs)} frames")
        return [self.decompress_frame(b) for b in blobs]

    def verify_lossless(self, original_frames, decompressed_frames):
        from .verify import verify_lossless
        res = verify_lossless(original_frames, decompressed_frames)
        if self.verbose and "exact_frame_matches" in res:
            print(f"Lossless verification: {'SUCCESS' if res['lossless'] else 'FAILED'}")
            print(f"Exact frame matches: {res['exact_frame_matches']}/{res['total_frames']}")
        return res

    def add_yuv_info_to_frame(self, yuv_frame):
        return YUVFrame(yuv_frame)


# ----------------------------------------------------------------------------- wire record (A7)
def build_record(wire_format, p, n, k, bitmap_bits, bitmap_packed, witness_bits, witness_packed, value_count, values_z):
    """The inter-frame wire record of improved_video_compressor.py:933-959 from already packed parts
    (bitmap_packed / witness_packed: numpy.packbits bytes; values_z: zlib-9 of the value bytes).
    wire_format "reference": k as float32, the reference's bytes; "f64": k as float64 (module docstring)."""
    bm, wb = bytes(bitmap_packed), bytes(witness_packed)
    return b"".join([
        struct.pack("<f", p), struct.pack("<I", n),
        struct.pack("<f" if wire_format == "reference" else "<d", k),
        struct.pack("<I", bitmap_bits), struct.pack("<I", witness_bits),
        struct.pack("<I", len(bm)), bm, struct.pack("<I", len(wb)), wb,
        struct.pack("<I", len(values_z)), struct.pack("<I", value_count), values_z])


def parse_record(wire_format, compressed_data):
    """Fields of a wire record without decoding anything (:983-1012): dict with p, n, k, bitmap_bits,
    witness_bits, bitmap (packed bytes), witness (packed bytes), values_z, value_count.  A plain ValueError for a record that is cut
    short anywhere, whose bitmap or witness byte count is not ceil(bits / 8), or that is longer than its fields say."""
    mv = memoryview(compressed_data)
    off = 0

    def take(fmt, what):
        nonlocal off
        if off + struct.calcsize(fmt) > len(mv):
            raise ValueError("truncated inter-frame record: its %d bytes end in front of or inside %s" % (len(mv), what))
        v = struct.unpack_from(fmt, mv, off)[0]
        off += struct.calcsize(fmt)
        return v

    def take_bytes(what, bits):
        nonlocal off
        size = take("<I", "the size of " + what)
        if size != (bits + 7) // 8:
            raise ValueError("inter-frame record: %d bytes of %s for %d bits" % (size, what, bits))
        if off + size > len(mv):
            raise ValueError("truncated inter-frame record: its %d bytes end inside %s" % (len(mv), what))
        part = np.frombuffer(mv[off:off + size], dtype=np.uint8)
        off += size
        return part
    out = {"p": take("<f", "p"), "n": take("<I", "n"), "k": take("<f" if wire_format == "reference" else "<d", "k"),
           "bitmap_bits": take("<I", "bitmap_bits"), "witness_bits": take("<I", "witness_bits")}
    out["bitmap"] = take_bytes("the bitmap", out["bitmap_bits"])
    out["witness"] = take_bytes("the witness", out["witness_bits"])
    vsize = take("<I", "the size of the values")
    out["value_count"] = take("<I", "the value count")
    if off + vsize != len(mv):
        raise ValueError("inter-frame record: %d bytes of values declared, %d are there" % (vsize, len(mv) - off))
    out["values_z"] = bytes(mv[off:off + vsize])
    return out


# ----------------------------------------------------------------------------- inter-frames
class VideoFrameCompressor:
    def __init__(self, noise_tolerance=10.0, keyframe_interval=30, min_diff_threshold=3.0,
                 max_diff_threshold=30.0, bloom_threshold_modifier=1.0, num_threads=None,
                 use_direct_yuv=False, verbose=False, wire_format="f64", ctx=None, mask_channels="luma"):
        """mask_channels: "luma" (default) -- the reference's residual mask on the luma plane; "all" -- a pixel's bit is 1 when ANY of its
        samples changed (rbf_residual_mask_batch_ex), so that the (mask, all channels) record is lossless even where only chroma moved.
        "all" is lossless only: _calculate_frame_diff takes threshold 0 and nothing else."""
        if mask_channels not in ("luma", "all"):
            raise ValueError("mask_channels must be 'luma' or 'all', got %r" % (mask_channels,))
        self.mask_channels = mask_channels
        self.noise_tolerance = noise_tolerance
        self.keyframe_interval = keyframe_interval
        self.min_diff_threshold = min_diff_threshold
        self.max_diff_threshold = max_diff_threshold
        self.bloom_threshold_modifier = bloom_threshold_modifier
        self.use_direct_yuv = use_direct_yuv
        self.verbose = verbose
        self.num_threads = max(1, num_threads or 1)            # kept for signature parity; the GPU does the work
        if wire_format not in ("f64", "reference"):
            raise ValueError("wire_format must be 'f64' or 'reference'")
        self.wire_format = wire_format
        self._ctx = ctx or nat.default_context()
        self.bloom_compressor = BloomFilterCompressor(verbose=False, ctx=self._ctx)
        self._engine = BloomEngine(self._ctx)

    def close(self):
        """Return the device scratch of this codec (also happens when the object is dropped)."""
        self._engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- A1 + A2
    def _luma_pair(self, prev_frame, curr_frame):
        a, b = frame_data(prev_frame), frame_data(curr_frame)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError("frames must have the same shape and dtype")
        if a.dtype not in (np.uint8, np.uint16):
            raise ValueError("8- or 16-bit unsigned samples expected")
        is_color = a.ndim > 2 and a.shape[2] > 1
        if is_color and a.shape[2] < 3:
            raise ValueError("color frames need at least 3 channels")          # cv2.cvtColor would raise as well
        return a, b, is_color

    def _luma_planes(self, a, b, is_color):
        """(prev_gray, curr_gray) of improved_video_compressor.py:787-798."""
        if not is_color:
            return a, b
        if self.use_direct_yuv:
            return a[:, :, 0], b[:, :, 0]
        gray = self._engine.bgr_to_gray(np.stack([a, b]))                     # cv2.COLOR_BGR2GRAY on the GPU
        return gray[0], gray[1]

    # ---- A1, adaptive threshold
    def _estimate_noise_level(self, frame):
        """np.std of luma - medianBlur5(luma) as np.float32 -- improved_video_compressor.py:727-744.
        `frame` is a 2-D luma plane (what _calculate_frame_diff passes, :805)."""
        luma = frame_data(frame)
        if luma.ndim != 2:
            raise ValueError("a 2-D luma plane is expected")
        return self._engine.noise_levels(luma[None])[0]

    def _adaptive_diff_threshold(self, frame):
        """max(min, min(max, noise_level * noise_tolerance)) -- improved_video_compressor.py:746-766."""
        return adaptive_threshold(self._estimate_noise_level(frame), self.noise_tolerance,
                                  self.min_diff_threshold, self.max_diff_threshold)

    def _calculate_frame_diff(self, prev_frame, curr_frame, threshold=None):
        """(binary_diff HxW uint8, changed_values, density) -- improved_video_compressor.py:768-847.
        threshold=None: noise-adaptive threshold of the current luma plane (:804-805).
        mask_channels="all": the all-channel mask of the full frames at threshold 0 (anything else raises ValueError)."""
        if self.mask_channels == "all" and (threshold is None or np.ndim(threshold) != 0 or float(threshold) != 0.0):
            raise ValueError("mask_channels='all' is lossless only: threshold must be 0, got %r" % (threshold,))
        a, b, is_color = self._luma_pair(prev_frame, curr_frame)
        if self.mask_channels == "all" and is_color:
            masks, ones = self._engine.residual_masks(np.stack([a, b]), 0, luma_only=False)
            h, w = a.shape[:2]
            n = h * w
            packed = masks[0][:(n + 7) // 8]
            values = gather_values(self._ctx, b, packed)
            binary_diff = np.unpackbits(packed)[:n].reshape(h, w)
            return binary_diff, values, np.uint64(ones[0]) / binary_diff.size
        ya, yb = self._luma_planes(a, b, is_color)
        if threshold is None:
            threshold = self._adaptive_diff_threshold(yb)
        masks, ones = self._engine.residual_masks(np.stack([ya, yb]), threshold)
        h, w = a.shape[:2]
        n = h * w
        packed = masks[0][:(n + 7) // 8]
        values = gather_values(self._ctx, b, packed)
        binary_diff = np.unpackbits(packed)[:n].reshape(h, w)
        density = np.uint64(ones[0]) / binary_diff.size
        return binary_diff, values, density

    # ---- A8
    def _apply_frame_diff(self, base_frame, diff_mask, changed_values):
        """improved_video_compressor.py:849-909 (color frames are left untouched when the value
        count does not match, exactly as the reference's `if len(changed_values) == expected_values`)."""
        base = frame_data(base_frame)
        mask = np.asarray(diff_mask, dtype=np.uint8)
        ch = base.shape[2] if base.ndim == 3 else 1
        count = int(mask.sum())
        if len(changed_values) != count * ch:
            if base.ndim == 3 and ch > 1:
                out = base.copy()
                return YUVFrame(out) if isinstance(base_frame, YUVFrame) else out
            raise ValueError("changed_values does not match the mask")
        out = scatter_values(self._ctx, base, np.packbits(mask.reshape(-1)), np.asarray(changed_values).astype(base.dtype))
        return YUVFrame(out) if isinstance(base_frame, YUVFrame) else out

    # ---- A3-A5 + A7
    def _build_record(self, p, n, k, bitmap_bits, bitmap_packed, witness_bits, witness_packed, value_count, values_z):
        return build_record(self.wire_format, p, n, k, bitmap_bits, bitmap_packed, witness_bits, witness_packed, value_count, values_z)

    def _compress_frame_differences(self, binary_diff, changed_values):
        """(record bytes, ratio) -- improved_video_compressor.py:911-967."""
        flat = np.asarray(binary_diff).flatten()
        bitmap, witness, p, n, _ = self.bloom_compressor.compress(flat)
        k, _l = self.bloom_compressor._calculate_optimal_params(n, p)
        vals = np.asarray(changed_values)
        rec = self._build_record(p, n, k, len(bitmap), np.packbits(bitmap).tobytes(), len(witness),
                                 np.packbits(np.array(witness, dtype=np.uint8)).tobytes(), len(vals),
                                 zlib.compress(vals.tobytes(), level=9))
        ratio = (len(rec) * 8) / (n + len(vals) * 8)
        return rec, ratio

    def _parse_record(self, compressed_data):
        return parse_record(self.wire_format, compressed_data)

    def _decompress_frame_differences(self, compressed_data, frame_shape, dtype=np.uint8):
        """(binary_diff, changed_values) -- improved_video_compressor.py:969-1027."""
        mv = memoryview(compressed_data)
        off = 0

        def take(fmt):
            nonlocal off
            v = struct.unpack_from(fmt, mv, off)[0]
            off += struct.calcsize(fmt)
            return v
        _p = take("<f")
        n = take("<I")
        k = take("<f" if self.wire_format == "reference" else "<d")
        bitmap_len = take("<I")
        witness_len = take("<I")
        size = take("<I")
        bitmap = np.unpackbits(np.frombuffer(mv[off:off + size], dtype=np.uint8))[:bitmap_len]
        off += size
        size = take("<I")
        witness = np.unpackbits(np.frombuffer(mv[off:off + size], dtype=np.uint8))[:witness_len].tolist()
        off += size
        vsize = take("<I")
        vcount = take("<I")
        values = np.frombuffer(zlib.decompress(mv[off:off + vsize]), dtype=dtype)[:vcount]
        flat = self.bloom_compressor.decompress(bitmap, witness, n, k) if witness_len > 0 else bitmap
        if len(frame_shape) == 3 and frame_shape[2] > 1:
            shape = (frame_shape[0], frame_shape[1])
        else:
            shape = tuple(frame_shape)
        return np.asarray(flat).reshape(shape), values
