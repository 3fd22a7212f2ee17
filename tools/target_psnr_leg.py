#!/usr/bin/env python3
"""target_psnr_leg.py -- the PSNR target (ImprovedVideoCompressor(max_error=cap, target_psnr=T)) on camera footage whose sensor noise
varies from run to run (synthetic.make_camera_gop without noise + synthetic.add_run_noise: run r carries noise of +-amplitudes[r]), next
to the fixed bounds max_error = 1 / 2 / 4 of the same run.

Default: a 1920x1080 8-bit YUV444 clip of 300 frames, keyframe interval 30 (ten runs), mask_channels="all", sample_codec="rice", both
hold modes; per (hold mode, setting) ONE JSON line with the container bytes, the median compress_video seconds of --runs alternating
runs (the settings take turns, so a drifting clock hits them alike), the bound every run got (a fixed bound: the same for all) and the
PSNR every run achieved over all samples of all its frames, from last_quality.  --out: a file the lines are appended to.

--profile: does the sweep kernel earn its place?  One 61-frame 1080p block (runs of 30, 30 and 1 frames), D candidates
(container.sweep_candidates(cap); --caps 4 16 gives D = 4 and D = 8), per hold mode: ONE rbf_hold_sweep call against the composed route
through the entries that existed before it -- for each candidate a device copy of the block (rbf_memcpy_d2d), the hold entry on the copy,
rbf_error_stats of the block against the copy and the all-channel mask counts of the copy (rbf_residual_mask_batch_ex) -- in one
process, on one block, taking turns --reps times; both as wall milliseconds from the first call to the stream's synchronisation, median,
with the event time of the hold kernels alone (RBF_K_HOLD) next to them.  Recorded: profiles/r23_target_psnr.txt."""
import argparse
import ctypes
import gc
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_clip(width, height, frames, interval, amplitudes):
    from new_bloom_filter_repo_amd.synthetic import add_run_noise, make_camera_gop
    return add_run_noise(np.stack(make_camera_gop(2026, width, height, frames)), interval, amplitudes, seed=2026)


def encode(frames, interval, mode, max_error, target):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec="rice", max_error=max_error,
                                   hold_mode=mode, target_psnr=target, quality_report=True)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    dt = time.perf_counter() - t0
    gc.enable()
    quality, bounds, timing = comp.last_quality, comp.last_run_bounds, comp.last_timing
    comp.close()
    return res, quality, bounds, timing, dt


def run_psnr(quality, interval, samples):
    """PSNR per run of `interval` frames over all samples of all its frames (inf for an exact run), from a per-frame quality report."""
    out = []
    for lo in range(0, len(quality), interval):
        rows = quality[lo:lo + interval]
        mse = sum(r["mse"] for r in rows) / len(rows)
        out.append(round(10 * math.log10(255.0 ** 2 / mse), 3) if mse else float("inf"))
    return out


def profile(width, height, caps, reps, amplitudes):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd import container
    W, H, F, C = width, height, 61, 3
    x = make_clip(W, H, F, 30, amplitudes)
    fb, n = x[0].nbytes, W * H
    ctx = nat.Context(0)
    lib = nat.lib()
    src, dst = ctx.alloc(F * fb), ctx.alloc(F * fb)
    mstride = nat.packed_stride(n)
    masks, ones = ctx.alloc(mstride * (F - 1)), ctx.alloc(8 * (F - 1))
    src.upload(x.reshape(-1).view(np.uint8))
    starts = (ctypes.c_uint8 * F)()
    starts[30] = starts[60] = 1
    for cap in caps:
        cands = container.sweep_candidates(cap)
        arr = (ctypes.c_uint32 * len(cands))(*cands)
        for mode in ("first", "lookahead"):
            look = int(mode == "lookahead")
            hold = lib.rbf_temporal_lookahead_runs if look else lib.rbf_temporal_hold_runs
            rows = np.zeros((3, len(cands)), dtype=nat.SWEEP_ROW)
            err = np.zeros(F, dtype=nat.ERROR_ROW)

            def sweep():
                nat.check(lib.rbf_hold_sweep(ctx.handle, src.ptr, fb, F, W, H, C, 1, starts, look, arr, len(cands), rows.ctypes.data))

            def composed():
                for d in cands:
                    nat.check(lib.rbf_memcpy_d2d(ctx.handle, dst.ptr, src.ptr, F * fb))
                    nat.check(hold(ctx.handle, dst.ptr, fb, F, W, H, C, 1, d, starts))
                    nat.check(lib.rbf_residual_mask_batch_ex(ctx.handle, dst.ptr, fb, F, W, H, W * C, C, 1, 0, None, masks.ptr, mstride, ones.ptr, C))
                    nat.check(lib.rbf_error_stats(ctx.handle, src.ptr, fb, dst.ptr, fb, F, W, H, C, 1, None, d, err.ctypes.data))

            sweep(); composed(); ctx.sync()                    # warm: scratch allocated, code objects loaded
            times = {"sweep": [], "composed": []}
            ctx.timing(1 << nat.K_HOLD)
            ctx.timing_reset()
            for _ in range(reps):
                for name, fn in (("sweep", sweep), ("composed", composed)):
                    ctx.sync()
                    t0 = time.perf_counter()
                    fn()
                    ctx.sync()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            hold_ms, hold_launches = ctx.timing_read()["hold"]
            ctx.timing(0)
            ms = {k: round(statistics.median(v), 3) for k, v in times.items()}
            print(json.dumps({"profile": "hold_sweep", "hold_mode": mode, "candidates": cands, "frames": F, "width": W, "height": H, "reps": reps,
                              "sweep_ms_median": ms["sweep"], "composed_ms_median": ms["composed"],
                              "composed_over_sweep": round(ms["composed"] / ms["sweep"], 2),
                              "hold_kernels_event_ms_per_candidate": round(hold_ms / max(1, reps * len(cands)), 3),
                              "hold_launches": hold_launches, "rows_run0_sse": [int(v) for v in rows[0]["sse"]]}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--amplitudes", type=int, nargs="+", default=[0, 1, 2, 3, 1, 0, 2, 1, 3, 0])
    ap.add_argument("--max-errors", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--targets", type=float, nargs="+", default=[44.0, 46.0, 48.0])
    ap.add_argument("--cap", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--caps", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        profile(a.width, a.height, a.caps, a.reps, a.amplitudes)
        return
    frames = make_clip(a.width, a.height, a.frames, a.interval, a.amplitudes)
    samples = frames[0].size
    combos = [(mode, me, None) for mode in ("first", "lookahead") for me in a.max_errors] + \
             [(mode, a.cap, T) for mode in ("first", "lookahead") for T in a.targets]
    seconds, facts = {c: [] for c in combos}, {}
    for run in range(a.runs):                              # alternating: every setting once per round
        for combo in combos:
            mode, me, T = combo
            res, quality, bounds, timing, dt = encode(frames, a.interval, mode, me, T)
            seconds[combo].append(dt)
            if run == 0:
                facts[combo] = {"container_bytes": res["compressed_size"], "keyframes": res["keyframes"],
                                "run_bounds": [d for _, d, _, _ in bounds] if T is not None else [me] * ((a.frames + a.interval - 1) // a.interval),
                                "run_psnr_db": run_psnr(quality, a.interval, samples),
                                "max_abs_error": max(r["max_abs_error"] for r in quality),
                                "hold_sweep_s": round(timing.get("hold_sweep", 0.0), 4)}
            print("run %d: %s max_error %d target %s %.3f s" % (run, mode, me, T, dt), file=sys.stderr, flush=True)
    for combo in combos:
        mode, me, T = combo
        row = dict({"leg": "target_psnr", "width": a.width, "height": a.height, "frames": a.frames, "keyframe_interval": a.interval,
                    "noise_amplitudes": a.amplitudes, "sample_codec": "rice", "hold_mode": mode, "max_error": me, "target_psnr": T,
                    "compress_video_s_median": round(statistics.median(seconds[combo]), 3), "runs": a.runs}, **facts[combo])
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
