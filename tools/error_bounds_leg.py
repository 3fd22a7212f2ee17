#!/usr/bin/env python3
"""error_bounds_leg.py -- near-lossless with a bound per sample (ImprovedVideoCompressor(error_bounds=...)) and the GPU quality report
(quality_report=True) on the clip of near_lossless_leg.py: 1920x1080 YUV444, 300 frames, sensor_noise=1, keyframe interval 30, 8 bits,
mask_channels="all".  Per (hold mode, sample codec) four bound settings:
  scalar1      max_error=1, today's call: the yardstick
  uniform1     error_bounds = a bound frame of 1 everywhere: must write the bytes of scalar1 (`same_bytes_as_scalar1`)
  per_channel  error_bounds=(1, 2, 2): chroma tolerates more than luma
  roi          1 everywhere, 0 inside the centre quarter: an exact region of interest
and per row ONE JSON line: keyframes, mean mask density of the inter-frames, pairs through the Bloom kernels (l > 0), container bytes,
the median compress_video seconds of --runs alternating runs without and with quality_report, verify_max_error of the decoded clip
against the bound frame, and the mean PSNR of last_quality next to that of verify.quality of the decoded clip (`quality_agrees`: the two
lists are equal, dict by dict).  Recorded: profiles/r17_error_bounds.txt.

--profile: one 61-frame 1080p 8-bit block (frames 0..60: two keyframes inside) through GopCoder, --reps times on freshly uploaded frames,
with max_error=1, with the uniform bound frame of 1 (GopCoder sends it through the _map kernels: the same decisions as max_error=1, so
like for like against the scalar twins) and with the roi bound frame, both hold modes, keep_originals=True and error_stats() after every
encode: k_hold_map / k_lookahead_map next to their scalar twins and k_error_stats next to k_residual_mask_any_gop in one trace, for
`rocprofv3 --kernel-trace --stats -- python tools/error_bounds_leg.py --profile` (kernel trace alone: no counters in the same run)."""
import argparse
import gc
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ["scalar1", "uniform1", "per_channel", "roi"]


def bounds_of(setting, shape):
    """(the compressor's keywords, what verify_max_error and verify.quality compare against)."""
    H, W, C = shape
    if setting == "scalar1":
        return {"max_error": 1}, 1
    if setting == "uniform1":
        return {"error_bounds": np.ones(shape, dtype=np.uint8)}, 1
    if setting == "per_channel":
        return {"error_bounds": (1, 2, 2)}, (1, 2, 2)
    roi = np.ones((H, W), dtype=np.uint8)
    roi[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 0
    return {"error_bounds": roi}, roi


def encode(frames, interval, codec, mode, kw, report):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec=codec, hold_mode=mode, quality_report=report, **kw)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    dt = time.perf_counter() - t0
    gc.enable()
    records, last_quality = comp.last_compressed_frames, comp.last_quality
    comp.close()
    return res, records, last_quality, dt


def describe(frames, records, res, last_quality, against, interval, twin=None):
    """(sha256 of the container, the row's facts).  twin: (sha256, facts, last_quality) of a row that must have written the same bytes --
    when it has, and reported the same quality, its decode and its verification are this row's too and are not repeated."""
    from new_bloom_filter_repo_amd.frame_codec import parse_record
    from new_bloom_filter_repo_amd.verify import quality, verify_max_error
    from new_bloom_filter_repo_amd.video_compressor import INTER, INTER_RICE, ImprovedVideoCompressor
    H, W, C = frames[0].shape
    density, bloom, inter = [], 0, 0
    for ty, rec in records:
        if ty in (INTER, INTER_RICE):
            d = parse_record("f64", rec[1:])
            inter += 1
            bloom += 1 if d["witness_bits"] > 0 else 0
            density.append(d["value_count"] / C / (H * W))
    blob = ImprovedVideoCompressor._container(records)
    digest = hashlib.sha256(blob).hexdigest()
    if twin is not None and twin[0] == digest and twin[2] == last_quality:
        return digest, dict(twin[1], verified_as_its_twin=True)
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads the container
    dec = dec_comp.decompress_video(compressed_frames=ImprovedVideoCompressor._parse_container(blob))
    dec_comp.close()
    dec = [np.asarray(getattr(d, "data", d)) for d in dec]
    v = verify_max_error(frames, dec, against, keyframe_interval=interval)
    t0 = time.perf_counter()
    decoded_quality = quality(frames, dec, against)
    t_quality = time.perf_counter() - t0

    def mean_psnr(q):
        finite = [r["psnr"] for r in q if r["psnr"] != float("inf")]
        return round(float(np.mean(finite)), 4) if finite else None
    return digest, {"keyframes": res["keyframes"], "inter_frames": inter, "mean_mask_density": round(float(np.mean(density)), 5) if density else None,
                  "bloom_pairs": bloom, "container_bytes": len(blob), "verify_max_error": v, "mean_psnr_last_quality": mean_psnr(last_quality),
                  "mean_psnr_decoded": mean_psnr(decoded_quality), "quality_agrees": last_quality == decoded_quality,
                  "over_bound": sum(r["over_bound"] for r in last_quality), "verify_quality_s": round(t_quality, 3)}


def profile(reps):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd import container
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F, sensor_noise=1))
    roi = container.bounds_frame(bounds_of("roi", (H, W, 3))[0]["error_bounds"], (H, W, 3), np.uint8)
    ctx = nat.Context(0)
    for mode in ("first", "lookahead"):
        for name, kw in (("scalar1", {"max_error": 1}), ("uniform1", {"error_bounds": np.ones_like(roi)}), ("roi", {"error_bounds": roi})):
            coder = GopCoder(ctx, W, H, F, run_starts=[30, 60], mask_channels=3, hold_mode=mode, keep_originals=True, **kw)
            ctx.timing(True)
            ctx.timing_reset()
            for _ in range(reps):
                coder.load_frames(frames)                 # (the hold rewrites the block: every repetition holds the original frames)
                coder.encode()
                coder.results_packed()
                rows = coder.error_stats()
            ctx.sync()
            tm = {k: [round(v[0], 4), v[1]] for k, v in ctx.timing_read().items() if v[1]}
            coder.close()
            print(json.dumps({"profile": "error_bounds", "hold_mode": mode, "bounds": name, "reps": reps, "frames": F, "width": W, "height": H,
                              "max_abs": int(rows["max_abs"].max()), "over_bound": int(rows["over_bound"].sum()),
                              "event_ms_and_launches": tm}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--codecs", nargs="+", default=["zlib", "rice"])
    ap.add_argument("--hold-modes", nargs="+", default=["first", "lookahead"])
    ap.add_argument("--settings", nargs="+", default=SETTINGS, choices=SETTINGS)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        profile(a.reps)
        return
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    frames = make_camera_gop(2026, a.width, a.height, a.frames, sensor_noise=1)
    shape = frames[0].shape
    combos = [(mode, codec, s) for mode in a.hold_modes for codec in a.codecs for s in a.settings]
    seconds = {(c, report): [] for c in combos for report in (False, True)}
    facts, blobs, twins = {}, {}, {}                       # (blobs: the containers' sha256)
    for run in range(a.runs):                              # alternating: every combination once per round, without and with the report
        for mode, codec, s in combos:
            kw, against = bounds_of(s, shape)
            for report in (False, True):
                res, records, last_quality, dt = encode(frames, a.interval, codec, mode, kw, report)
                seconds[((mode, codec, s), report)].append(dt)
                if run == 0 and report:
                    twin = twins.get((mode, codec, "scalar1")) if s == "uniform1" else None
                    blobs[(mode, codec, s)], facts[(mode, codec, s)] = describe(frames, records, res, last_quality, against, a.interval, twin)
                    twins[(mode, codec, s)] = (blobs[(mode, codec, s)], facts[(mode, codec, s)], last_quality)
                del records
                print("run %d: %s %s %s report=%s %.3f s" % (run, mode, codec, s, report, dt), file=sys.stderr, flush=True)
    for mode, codec, s in combos:
        row = dict({"leg": "error_bounds", "bits": 8, "width": a.width, "height": a.height, "frames": a.frames, "keyframe_interval": a.interval,
                    "sensor_noise": 1, "hold_mode": mode, "sample_codec": codec, "bounds": s,
                    "compress_video_s_median": round(statistics.median(seconds[((mode, codec, s), False)]), 3),
                    "compress_video_s_median_quality_report": round(statistics.median(seconds[((mode, codec, s), True)]), 3), "runs": a.runs},
                   **facts[(mode, codec, s)])
        if s == "uniform1" and (mode, codec, "scalar1") in blobs:
            row["same_bytes_as_scalar1"] = blobs[(mode, codec, s)] == blobs[(mode, codec, "scalar1")]
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
