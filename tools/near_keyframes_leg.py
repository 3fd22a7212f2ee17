#!/usr/bin/env python3
"""near_keyframes_leg.py -- bounded-error keyframes (ImprovedVideoCompressor(bounded_keyframes=True), record type 7) on the noisy clip of
the near-lossless legs (synthetic.make_camera_gop(2026, sensor_noise=1): 300 frames of 1920x1080 YUV444, keyframe interval 30), sample
codec rice.  Three near-lossless settings -- max_error=2 with the first-value hold, max_error=1 with the look-ahead hold, error_bounds
(1, 2, 2) with the look-ahead hold -- each with the keyword off and on in the same process, the runs alternating (a drifting clock hits
both alike).  Per (setting, keyword) ONE JSON line: container bytes, keyframe and inter-frame record bytes (split as in
sample_codec_leg.py), record types, median compress_video and decompress_video seconds of --runs runs, the worst error and the mean PSNR
of the decoded clip (verify.quality), verify_max_error, whether last_quality equals verify.quality of the decoded clip, and -- on the
keyword-on line -- the keyframe-bytes ratio against the keyword-off line of the same run (the yardstick).
--only-off: the keyword-off lines alone (the comparison of two source trees: one process per tree, in alternation).

--profile: one 61-frame 1080p block (frames 0..60, keyframes 0, 30, 60) through one GopCoder(max_error=2) with quantise_run_starts and
the type-3 keyframe coder next to it, --reps times on freshly uploaded frames, then the decode of a type-7 and a type-3 keyframe, for
`rocprofv3 --kernel-trace --stats -- python tools/near_keyframes_leg.py --profile` (kernel trace alone: no counters in the same run):
k_keyquant_u / k_keyquant_apply next to k_rice_intra_u and k_temporal_hold, k_keyquant_rebuild next to k_rice_intra_rebuild."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = [("first_d2", dict(max_error=2), 2), ("lookahead_d1", dict(max_error=1, hold_mode="lookahead"), 1),
            ("lookahead_122", dict(error_bounds=(1, 2, 2), hold_mode="lookahead"), (1, 2, 2))]


def run_once(frames, interval, near, keyword, want_quality):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    kw = dict(bounded_keyframes=True) if keyword else {}
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec="rice", quality_report=want_quality, **near, **kw)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    t_c = time.perf_counter() - t0
    gc.enable()
    records, reported = comp.last_compressed_frames, comp.last_quality
    comp.close()
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads the container
    t0 = time.perf_counter()
    dec = dec_comp.decompress_video(compressed_frames=records)
    t_d = time.perf_counter() - t0
    dec_comp.close()
    return res, records, reported, dec, t_c, t_d


def describe(frames, records, reported, dec, bound, interval):
    from new_bloom_filter_repo_amd.verify import quality, verify_max_error
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    q = quality(list(frames), dec, error_bounds=bound)
    finite = [r["psnr"] for r in q if np.isfinite(r["psnr"])]
    return {"container_bytes": ImprovedVideoCompressor._container_size(records),
            "keyframe_record_bytes": sum(4 + 1 + len(r) for ty, r in records if ty in (1, 3, 7)),
            "inter_record_bytes": sum(4 + 1 + len(r) for ty, r in records if ty in (2, 4)),
            "record_types": sorted({ty for ty, _ in records}), "keyframes": sum(1 for ty, _ in records if ty in (1, 3, 7)),
            "worst_error": max(r["max_abs_error"] for r in q), "mean_psnr_db": round(float(np.mean(finite)), 3) if finite else None,
            "exact_frames": len(q) - len(finite), "last_quality_equals_verify_quality": reported == q,
            "verify_max_error": verify_max_error(list(frames), dec, bound, keyframe_interval=interval)}


def profile(reps):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.sample_codec import SampleCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F, sensor_noise=1))
    ctx = nat.Context(0)
    codec = SampleCoder(ctx)
    coder = GopCoder(ctx, W, H, F, run_starts=[30, 60], mask_channels=3, max_error=2)
    exact = codec.encode_frames([frames[0], frames[30], frames[60]])       # the type-3 streams of the same three keyframes: k_rice_intra_u
    t0 = time.perf_counter()
    for _ in range(reps):
        coder.load_frames(frames)
        streams = coder.quantise_run_starts(codec)
        coder.encode()
        coder.results_packed()
    ctx.sync()
    dt = (time.perf_counter() - t0) / reps
    for _ in range(reps):
        codec.decode_near_frame(streams[30], H, W, 3, 1, [2, 2, 2])
        codec.decode_frame(exact[1], H, W, 3, 1)
    ctx.sync()
    coder.close()
    codec.close()
    print(json.dumps({"profile": "near_keyframes", "reps": reps, "frames": F, "width": W, "height": H, "block_seconds_mean": round(dt, 4),
                      "type7_stream_bytes": [len(streams[j]) for j in sorted(streams)], "type3_stream_bytes": [len(s) for s in exact]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--sensor-noise", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        profile(a.reps)
        return
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    frames = make_camera_gop(2026, a.width, a.height, a.frames, sensor_noise=a.sensor_noise)
    combos = [(name, near, bound, keyword) for name, near, bound in SETTINGS for keyword in ((False,) if a.only_off else (False, True))]
    seconds, facts = {(c[0], c[3]): ([], []) for c in combos}, {}
    for run in range(a.runs):                              # alternating: every combination once per round
        for name, near, bound, keyword in combos:
            first = run == 0
            res, records, reported, dec, t_c, t_d = run_once(frames, a.interval, near, keyword, want_quality=first and not a.only_off)
            if first and not a.only_off:                   # (the report costs a copy of the block: timed runs go without it)
                facts[(name, keyword)] = describe(frames, records, reported, dec, bound, a.interval)
            else:
                seconds[(name, keyword)][0].append(t_c)
                seconds[(name, keyword)][1].append(t_d)
                if first:
                    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
                    facts[(name, keyword)] = {"container_bytes": ImprovedVideoCompressor._container_size(records)}
            del records, dec
            gc.collect()
            print("run %d: %s bounded_keyframes=%s %.3f s / %.3f s" % (run, name, keyword, t_c, t_d), file=sys.stderr, flush=True)
    for name, near, bound, keyword in combos:
        tc, td = seconds[(name, keyword)]
        row = dict({"leg": "near_keyframes", "setting": name, "bounded_keyframes": keyword, "width": a.width, "height": a.height, "frames": a.frames,
                    "keyframe_interval": a.interval, "sensor_noise": a.sensor_noise, "sample_codec": "rice",
                    "compress_video_s_median": round(statistics.median(tc), 3) if tc else None, "compress_video_s_all": [round(t, 3) for t in tc],
                    "decompress_video_s_median": round(statistics.median(td), 3) if td else None, "timed_runs": len(tc)}, **facts[(name, keyword)])
        if keyword and "keyframe_record_bytes" in row:
            off = facts[(name, False)]
            row["keyframe_bytes_vs_off"] = round(row["keyframe_record_bytes"] / off["keyframe_record_bytes"], 4)
            row["container_bytes_vs_off"] = round(row["container_bytes"] / off["container_bytes"], 4)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
