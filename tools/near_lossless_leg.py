#!/usr/bin/env python3
"""near_lossless_leg.py -- the near-lossless mode (ImprovedVideoCompressor(max_error=...)) on footage with sensor noise
(synthetic.make_camera_gop(sensor_noise=1): every sample of every frame carries a level of noise, so the exact all-channel mask is almost
all ones, every pair passes its mask through uncoded and the Bloom kernels never run).  max_error = 0 is the yardstick of the same run.

Default: a 1920x1080 YUV444 clip of 300 frames, keyframe interval 30, 8- and 16-bit, mask_channels="all"; per (bits, sample codec,
max_error) ONE JSON line with the keyframe count, the mean mask density of the inter-frames, how many of them went through the Bloom
kernels (l > 0), the container bytes, the median compress_video seconds of --runs alternating runs (the combinations take turns, so a
drifting clock hits them alike) and verify_max_error of the decoded clip.  Recorded: profiles/r12_near_lossless_leg.txt.
--hold-mode first | lookahead | both (default first: the r12 table) picks the decision rule of max_error > 0 (ImprovedVideoCompressor's
hold_mode; `both`: a line per rule, the look-ahead's with `container_bytes_vs_first`), --sensor-noise the noise amplitude of the clip,
--out a file the lines are appended to.  Recorded: profiles/r15_lookahead_hold.txt (8-bit, --hold-mode both: --sensor-noise 1
--max-errors 1 2, and --sensor-noise 2 --max-errors 2 3 4).

--profile: one 61-frame 1080p 8-bit block (frames 0..60: two keyframes inside) through one GopCoder(max_error=2), --reps times, each time on
freshly uploaded frames: k_temporal_hold next to k_residual_mask_any_gop on the same block, for `rocprofv3 --kernel-trace --stats --
python tools/near_lossless_leg.py --profile` (kernel trace alone: no counters in the same run).  With --hold-mode both the same block
then goes through GopCoder(hold_mode="lookahead") in the same process: k_temporal_lookahead and k_lookahead_fill in the same trace;
--profile-max-error sets the bound of both (default 2, r12's)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def encode(frames, interval, codec, max_error, hold_mode="first"):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec=codec, max_error=max_error,
                                   hold_mode=hold_mode if max_error else "first")
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    dt = time.perf_counter() - t0
    gc.enable()
    records = comp.last_compressed_frames
    comp.close()
    return res, records, dt


def describe(frames, records, res, max_error, interval):
    from new_bloom_filter_repo_amd.frame_codec import parse_record
    from new_bloom_filter_repo_amd.verify import verify_max_error
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
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads the container
    dec = dec_comp.decompress_video(compressed_frames=ImprovedVideoCompressor._parse_container(blob))
    dec_comp.close()
    v = verify_max_error(frames, dec, max_error, keyframe_interval=interval)
    return {"keyframes": res["keyframes"], "inter_frames": inter, "mean_mask_density": round(float(np.mean(density)), 5) if density else None,
            "bloom_pairs": bloom, "container_bytes": len(blob), "verify_max_error": v}


def profile(reps, max_error, hold_modes=("first",)):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F, sensor_noise=1))
    ctx = nat.Context(0)
    for mode in hold_modes:
        coder = GopCoder(ctx, W, H, F, run_starts=[30, 60], mask_channels=3, max_error=max_error, hold_mode=mode)
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(reps):
            coder.load_frames(frames)                     # (the hold rewrites the block: every repetition holds the original frames)
            coder.encode()
            coder.results_packed()
        ctx.sync()
        tm = {k: [round(v[0], 4), v[1]] for k, v in ctx.timing_read().items() if v[1]}
        coder.close()
        print(json.dumps({"profile": "near_lossless", "hold_mode": mode, "max_error": max_error, "reps": reps, "frames": F, "width": W, "height": H,
                          "event_ms_and_launches": tm}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--max-errors", type=int, nargs="+", default=[0, 1, 2, 4])
    ap.add_argument("--codecs", nargs="+", default=["zlib", "rice"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hold-mode", choices=["first", "lookahead", "both"], default="first")
    ap.add_argument("--sensor-noise", type=int, default=1)
    ap.add_argument("--profile-max-error", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = ["first", "lookahead"] if a.hold_mode == "both" else [a.hold_mode]
    if a.profile:
        profile(a.reps, a.profile_max_error, modes)
        return
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16, sensor_noise=a.sensor_noise)
        combos = [(codec, me, mode) for codec in a.codecs for me in a.max_errors for mode in (modes if me else modes[:1])]
        seconds, facts = {c: [] for c in combos}, {}
        for run in range(a.runs):                          # alternating: every combination once per round
            for codec, me, mode in combos:
                res, records, dt = encode(frames, a.interval, codec, me, mode)
                seconds[(codec, me, mode)].append(dt)
                if run == 0:
                    facts[(codec, me, mode)] = describe(frames, records, res, me, a.interval)
                del records
                print("run %d: %s max_error %d %s %.3f s" % (run, codec, me, mode, dt), file=sys.stderr, flush=True)
        for codec, me, mode in combos:
            row = dict({"leg": "near_lossless", "bits": bits, "width": a.width, "height": a.height, "frames": a.frames,
                        "keyframe_interval": a.interval, "sensor_noise": a.sensor_noise, "sample_codec": codec, "max_error": me,
                        "compress_video_s_median": round(statistics.median(seconds[(codec, me, mode)]), 3), "runs": a.runs},
                       **facts[(codec, me, mode)])
            if me and a.hold_mode != "first":              # (the default's lines stay the r12 ones)
                row["hold_mode"] = mode
                if mode == "lookahead" and (codec, me, "first") in facts:
                    row["container_bytes_vs_first"] = round(row["container_bytes"] / facts[(codec, me, "first")]["container_bytes"], 4)
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")
        del frames
        gc.collect()


if __name__ == "__main__":
    main()
