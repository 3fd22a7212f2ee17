"""Losslessness harness with the reference's result dictionaries:
verify_lossless  -- FixedVideoCompressor.verify_lossless (fixed_video_compressor.py:217-285)
verify_bit_exact -- verify_true_lossless.verify_bit_exact (verify_true_lossless.py:338-492),
                    without the OpenCV diagnostic image dumps.
verify_max_error -- the near-lossless mode's guarantee (ImprovedVideoCompressor(max_error=...)); the reference has no counterpart.
quality          -- per-frame error statistics and PSNR of a decoded clip, measured on the GPU (rbf_error_stats); no counterpart either.
verify_container -- a container against its own frame digests (ImprovedVideoCompressor(frame_digests=True)): needs no originals.
Unlike the reference (which unwraps with `hasattr(x, 'data')` and then crashes on unequal plain
ndarrays, whose `.data` is a memoryview) both accept plain ndarrays and YUVFrame wrappers."""
import numpy as np


def _arr(frame):
    d = getattr(frame, "data", None)
    return d if isinstance(d, np.ndarray) else np.asarray(frame)


def verify_lossless(original_frames, decompressed_frames):
    if len(original_frames) != len(decompressed_frames):
        return {"lossless": False,
                "reason": f"Frame count mismatch: {len(original_frames)} vs {len(decompressed_frames)}",
                "avg_difference": float("inf")}
    exact, diff_frames, max_diff, max_diff_frame = 0, [], 0, -1
    for i, (o, d) in enumerate(zip(original_frames, decompressed_frames)):
        o, d = _arr(o), _arr(d)
        if np.array_equal(o, d):
            exact += 1
            continue
        frame_diff = np.mean(np.abs(o.astype(np.float32) - d.astype(np.float32)))
        diff_frames.append(i)
        if frame_diff > max_diff:
            max_diff, max_diff_frame = frame_diff, i
    ok = exact == len(original_frames)
    return {"lossless": ok, "exact_lossless": ok,
            "avg_difference": 0.0 if not diff_frames else max_diff,   # worst frame, as the reference reports it
            "max_difference": max_diff, "max_diff_frame": max_diff_frame,
            "exact_frame_matches": exact, "total_frames": len(original_frames), "diff_frames": diff_frames}


def verify_bit_exact(original_frames, decompressed_frames, color_space="BGR", verbose=False):
    if len(original_frames) != len(decompressed_frames):
        return {"success": False,
                "error": f"Frame count mismatch: {len(original_frames)} vs {len(decompressed_frames)}"}
    exact, diff_frames, details = 0, [], []
    for i, (o, d) in enumerate(zip(original_frames, decompressed_frames)):
        o, d = _arr(o), _arr(d)
        if o.shape != d.shape:
            diff_frames.append(i)
            details.append({"frame": i, "error": f"Shape mismatch: {o.shape} vs {d.shape}"})
            continue
        if np.array_equal(o, d):
            exact += 1
            continue
        diff_frames.append(i)
        diff = np.abs(o.astype(np.int16) - d.astype(np.int16))
        where = np.where(diff > 0)
        examples = []
        for j in range(min(10, len(where[0]))):
            c = tuple(axis[j] for axis in where)
            examples.append({"coordinates": str(c), "original_value": int(o[c]),
                             "decompressed_value": int(d[c]), "difference": int(diff[c])})
        details.append({"frame": i, "differences_found": len(where[0]), "examples": examples})
    result = {"success": exact == len(original_frames), "frames_compared": len(original_frames),
              "exact_matches": exact, "different_frames": len(diff_frames),
              "different_frame_indices": diff_frames, "diff_details": details}
    if verbose:
        print(f"Bit-exact verification: {'SUCCESS' if result['success'] else 'FAILED'}")
        print(f"  Exact frame matches: {exact}/{len(original_frames)}")
    return result


def verify_max_error(original_frames, decoded_frames, max_error, keyframe_interval=None):
    """The near-lossless guarantee: every decoded sample within max_error of the original.  Returns frame_count, max_abs_error (the worst
    sample, exact integer arithmetic), worst_frame (its index, -1 when every frame is exact), within_bound, and -- when keyframe_interval
    is given -- keyframes_exact: every frame t with t % keyframe_interval == 0 equals its original.  A frame-count or shape mismatch is
    not within any bound: within_bound False with a `reason`.
    max_error may also be anything ImprovedVideoCompressor(error_bounds=...) accepts (container.bounds_frame: per-channel bounds, an
    (H, W) or an (H, W, C) array): within_bound then says that every sample is within ITS bound, over_bound counts those that are not,
    and the result's max_error is the largest entry of the bound frame."""
    if not (isinstance(max_error, (int, np.integer)) and not isinstance(max_error, bool)):
        return _verify_bound_frame(original_frames, decoded_frames, max_error, keyframe_interval)
    out = {"frame_count": len(original_frames), "max_error": int(max_error), "max_abs_error": 0, "worst_frame": -1, "within_bound": False}
    if len(original_frames) != len(decoded_frames):
        out["reason"] = f"Frame count mismatch: {len(original_frames)} vs {len(decoded_frames)}"
        return out
    keys_exact = True
    for i, (o, d) in enumerate(zip(original_frames, decoded_frames)):
        o, d = _arr(o), _arr(d)
        if o.shape != d.shape:
            out["reason"] = f"Shape mismatch in frame {i}: {o.shape} vs {d.shape}"
            return out
        worst = int(np.abs(o.astype(np.int64) - d.astype(np.int64)).max()) if o.size else 0
        if worst > out["max_abs_error"]:
            out["max_abs_error"], out["worst_frame"] = worst, i
        if keyframe_interval and i % int(keyframe_interval) == 0 and worst:
            keys_exact = False
    out["within_bound"] = out["max_abs_error"] <= int(max_error)
    if keyframe_interval:
        out["keyframes_exact"] = keys_exact
    return out


def _verify_bound_frame(original_frames, decoded_frames, error_bounds, keyframe_interval):
    """verify_max_error against a bound per sample."""
    from .container import bounds_frame
    bounds_frame(error_bounds)                                   # (refuses what is no bound at all, whatever the frames are)
    out = {"frame_count": len(original_frames), "max_error": None, "max_abs_error": 0, "worst_frame": -1, "within_bound": False, "over_bound": 0}
    if len(original_frames) != len(decoded_frames):
        out["reason"] = f"Frame count mismatch: {len(original_frames)} vs {len(decoded_frames)}"
        return out
    keys_exact, E = True, None
    for i, (o, d) in enumerate(zip(original_frames, decoded_frames)):
        o, d = _arr(o), _arr(d)
        if o.shape != d.shape:
            out["reason"] = f"Shape mismatch in frame {i}: {o.shape} vs {d.shape}"
            return out
        if E is None or E.shape != o.shape or E.dtype != o.dtype:
            E = bounds_frame(error_bounds, o.shape, o.dtype)
        diff = np.abs(o.astype(np.int64) - d.astype(np.int64))
        worst = int(diff.max()) if o.size else 0
        out["over_bound"] += int(np.count_nonzero(diff > E))
        if worst > out["max_abs_error"]:
            out["max_abs_error"], out["worst_frame"] = worst, i
        if keyframe_interval and i % int(keyframe_interval) == 0 and worst:
            keys_exact = False
    out["max_error"] = None if E is None else int(E.max())
    out["within_bound"] = out["over_bound"] == 0
    if keyframe_interval:
        out["keyframes_exact"] = keys_exact
    return out


def quality_rows(rows, samples, bits):
    """The per-frame dicts of a quality report from rbf_error_stats rows (_native.ERROR_ROW; a frame of `samples` samples of `bits` bits):
    max_abs_error, mse = sse / samples, psnr = 10 log10((2^bits - 1)^2 / mse) -- inf for an exact frame --, changed_samples, over_bound."""
    peak2 = float(((1 << bits) - 1) ** 2)
    out = []
    for r in rows:
        sse = int(r["sse"])
        mse = sse / samples
        out.append({"max_abs_error": int(r["max_abs"]), "mse": mse, "psnr": float("inf") if sse == 0 else 10.0 * float(np.log10(peak2 / mse)),
                    "changed_samples": int(r["differing"]), "over_bound": int(r["over_bound"])})
    return out


def quality(original_frames, decoded_frames, error_bounds=None, ctx=None):
    """What did the decoded clip lose?  One dict per frame (quality_rows) from two lists of frames of one shape and dtype (uint8 / uint16,
    (H, W) or (H, W, C) with C <= 4), measured on the GPU by rbf_error_stats: both lists are uploaded in chunks of at most 64 frames and
    compared where they lie.  error_bounds: None -- over_bound counts against 0, so it equals changed_samples; an integer -- against that
    bound (a max_error=d clip); anything ImprovedVideoCompressor(error_bounds=...) accepts -- against the bound frame.  ctx: the library
    context to use (default: the process's).  The same numbers as ImprovedVideoCompressor(quality_report=True).last_quality, which needs
    no decode."""
    from . import _native as nat
    from .container import bounds_frame
    if len(original_frames) != len(decoded_frames):
        raise ValueError(f"Frame count mismatch: {len(original_frames)} vs {len(decoded_frames)}")
    if not original_frames:
        return []
    first = _arr(original_frames[0])
    if first.dtype not in (np.uint8, np.uint16) or first.ndim not in (2, 3) or (first.ndim == 3 and not 1 <= first.shape[2] <= 4):
        raise ValueError("quality compares uint8 / uint16 frames of up to four channels, got %r of %s" % (first.shape, first.dtype))
    scalar = isinstance(error_bounds, (int, np.integer)) and not isinstance(error_bounds, bool)
    if scalar and not 0 <= int(error_bounds) <= np.iinfo(first.dtype).max:
        raise ValueError("error_bounds %r does not fit a %d-bit sample" % (error_bounds, 8 * first.dtype.itemsize))
    E = None if error_bounds is None or scalar else bounds_frame(error_bounds, first.shape, first.dtype)
    H, W, C, sb = nat.frame_geometry(first)
    ctx = ctx or nat.default_context()
    CHUNK = 64
    fb = first.nbytes
    count = min(CHUNK, len(original_frames))
    a, b, e = ctx.alloc(fb * count), ctx.alloc(fb * count), None
    out = []
    try:
        if E is not None:
            e = ctx.alloc(fb)
            nat.check(nat.lib().rbf_memcpy_h2d(ctx.handle, e.ptr, E.ctypes.data, fb))
        for lo in range(0, len(original_frames), CHUNK):
            blocks = []
            for frames in (original_frames, decoded_frames):
                part = [_arr(f) for f in frames[lo:lo + CHUNK]]
                if any(f.shape != first.shape or f.dtype != first.dtype for f in part):
                    raise ValueError("quality needs frames of one shape and dtype (%r of %s)" % (first.shape, first.dtype))
                blocks.append(np.ascontiguousarray(np.stack(part)))
            for buf, block in zip((a, b), blocks):
                nat.check(nat.lib().rbf_memcpy_h2d(ctx.handle, buf.ptr, block.ctypes.data, block.nbytes))
            rows = np.zeros(len(blocks[0]), dtype=nat.ERROR_ROW)
            nat.check(nat.lib().rbf_error_stats(ctx.handle, a.ptr, fb, b.ptr, fb, len(rows), W, H, C, sb, None if e is None else e.ptr,
                                                int(error_bounds) if scalar else 0, rows.ctypes.data))
            out += quality_rows(rows, H * W * C, 8 * sb)
    finally:
        for buf in (a, b, e):
            if buf is not None:
                buf.free()
    return out


def verify_container(path_or_bytes, **compressor_kwargs):
    """Decode a container (a path, or its bytes) and check every frame against the digests it stores (integrity.py), without raising on a
    frame mismatch: {"frames": frames decoded, "checked": frames compared with a stored digest, "bad": [indices of the frames whose digest
    does not match], "trailer": "ok" | "absent" (nothing to check against) | "damaged" (the trailer itself is not usable: the frames are
    decoded, none is checked)}.  compressor_kwargs go to the ImprovedVideoCompressor that decodes (chain_chunk_frames: its attribute of
    that name).  What the records themselves make undecodable still raises: a plain ValueError whose text names the record's index in
    the stream -- never struct.error, IndexError, zlib.error, OverflowError, a numpy broadcasting error or an RbfError (decompress_video
    has the contract) -- and no frame is reported that the records do not code."""
    from . import container
    from .video_compressor import ImprovedVideoCompressor
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        blob = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            blob = f.read()
    records = container.parse(blob)
    try:
        _, stored = container.split_trailer([r for r in records if r[0] != container.PANS])     # (a pan table is the decoder's to judge)
        trailer = "absent" if stored is None else "ok"
    except ValueError:
        trailer = "damaged"
        records = [r for r in records if r[0] != container.DIGESTS]
    chunk = compressor_kwargs.pop("chain_chunk_frames", None)
    comp = ImprovedVideoCompressor(**compressor_kwargs)
    if chunk is not None:
        comp.chain_chunk_frames = int(chunk)
    try:
        frames = comp.decompress_video(compressed_frames=records, on_mismatch="collect")
        return {"frames": len(frames), "checked": comp.last_integrity["checked"], "bad": list(comp.last_bad_frames), "trailer": trailer}
    finally:
        comp.close()
