#!/usr/bin/env python3
"""mask_channels_leg.py -- the all-channel mask mode against the luma mask on a camera-like clip (synthetic.make_camera_gop: a smooth
texture, 1 % of the pixels perturbed per frame, BT.601 YUV444, so chroma changes where luma does not).  bench.py measures the synthetic
clips, on which both modes code the same frames; this leg is where they differ.

Default: a 1920x1080 YUV444 clip of 300 frames, keyframe interval 30, 8- and 16-bit; per (bits, mode) ONE JSON line with the keyframe
count, the container bytes, ImprovedVideoCompressor.compress_video / decompress_video seconds, last_timing["gpu_encode"] (the GPU block
passes), last_timing["value_gather"] (gather of the changed values, with the uncovered-change count in luma mode) and whether the decoded
clip is bit-exact.  Recorded: profiles/r07_mask_channels_leg.txt.

--profile MODE: one 61-frame 1080p 8-bit block (frames 0..60: two keyframes inside) through one GopCoder, --reps times: the mask kernel,
the Bloom kernels and the changed-value gather of that mode, for `rocprofv3 --kernel-trace --stats -- python tools/mask_channels_leg.py
--profile luma|all`.  Recorded: profiles/r07_mask_channels_kernel_stats_luma.csv, profiles/r07_mask_channels_kernel_stats_all.csv."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def leg(frames, bits, mode, interval):
    from new_bloom_filter_repo_amd.verify import verify_bit_exact
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels=mode)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    t_c = time.perf_counter() - t0
    gc.enable()
    tm = dict(comp.last_timing or {})
    blob = ImprovedVideoCompressor._container(comp.last_compressed_frames)
    comp.close()
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads either mode's container
    recs = ImprovedVideoCompressor._parse_container(blob)
    t0 = time.perf_counter()
    dec = dec_comp.decompress_video(compressed_frames=recs)
    t_d = time.perf_counter() - t0
    exact = verify_bit_exact(frames, dec, color_space="YUV")["success"]
    dec_comp.close()
    H, W = frames[0].shape[:2]
    return {"leg": "mask_channels", "mode": mode, "bits": bits, "width": W, "height": H, "frames": len(frames), "keyframe_interval": interval,
            "keyframes": res["keyframes"], "container_bytes": len(blob), "compress_video_s": round(t_c, 3), "decompress_video_s": round(t_d, 3),
            "gpu_encode_s": round(tm.get("gpu_encode", 0.0), 4), "value_gather_s": round(tm.get("value_gather", 0.0), 4), "bit_exact": bool(exact)}


def profile(mode, reps):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F))
    ctx = nat.Context(0)
    coder = GopCoder(ctx, W, H, F, run_starts=[30, 60], mask_channels=3 if mode == "all" else 1)
    coder.load_frames(frames)
    for _ in range(reps):
        coder.encode()
        coder.results_packed()
        coder.gather_values(check_uncovered=mode == "luma")
    ctx.sync()
    coder.close()
    print(json.dumps({"profile": mode, "reps": reps, "frames": F, "width": W, "height": H}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--profile", choices=["luma", "all"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.profile:
        profile(a.profile, a.reps)
        return
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16)
        for mode in ("luma", "all"):
            print(json.dumps(leg(frames, bits, mode, a.interval)), flush=True)
        del frames
        gc.collect()


if __name__ == "__main__":
    main()
