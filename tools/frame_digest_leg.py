#!/usr/bin/env python3
"""frame_digest_leg.py -- what the frame digests (ImprovedVideoCompressor(frame_digests=True), integrity.py) cost on the product surface.
frame_digests=False is the yardstick of the same run.

Default: a 1920x1080 YUV444 camera clip (synthetic.make_camera_gop) of 300 frames, keyframe interval 30, mask_channels="all"; per (bits,
frame_digests) ONE JSON line with the median compress_video and decompress_video seconds of --runs alternating runs (the two settings take
turns, so a drifting clock hits them alike), the container bytes and the decoder's last_integrity.  Recorded: profiles/r14_frame_digest.txt.

--profile: one 61-frame 1080p block (frames 0..60: two keyframes inside), 8- and 16-bit, through one GopCoder with the all-channel mask,
--reps times: encode() and frame_digests() on the same resident block, so that k_frame_digest stands next to k_residual_mask_any_gop --
both read the block's bytes once -- in ONE `rocprofv3 --kernel-trace --stats -- python tools/frame_digest_leg.py --profile` (kernel trace
alone: no counters in the same run).  The library has no kernel id for the digest: its time comes from the trace.  Plain against
non-temporal loads: build a second library with -DRBF_DIGEST_NT=1 (make -C new_bloom_filter_repo_amd/csrc OUT=<path> CXXFLAGS="<the
Makefile's> -DRBF_DIGEST_NT=1") and run the same trace with RBF_LIB_PATH=<path>."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def encode(frames, interval, digests):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", frame_digests=digests)
    gc.disable()
    t0 = time.perf_counter()
    comp.compress_video(list(frames), input_color_space="YUV")
    dt = time.perf_counter() - t0
    gc.enable()
    records = comp.last_compressed_frames
    comp.close()
    return records, dt


def decode(records):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor()
    gc.disable()
    t0 = time.perf_counter()
    frames = comp.decompress_video(compressed_frames=records)
    dt = time.perf_counter() - t0
    gc.enable()
    integrity = comp.last_integrity
    comp.close()
    return frames, dt, integrity


def profile(reps, bits):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.integrity import frame_digest
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    ctx = nat.Context(0)
    for b in bits:
        frames = np.stack(make_camera_gop(2026, W, H, F, dtype=np.uint8 if b == 8 else np.uint16))
        coder = GopCoder(ctx, W, H, F, sample_bytes=b // 8, run_starts=[30, 60], mask_channels=3)
        coder.load_frames(frames)
        for _ in range(reps):
            coder.encode()
            got = coder.frame_digests()
            coder.results_packed()
        ctx.sync()
        ok = [int(got[f]) for f in (0, 30, 60)] == [frame_digest(frames[f]) for f in (0, 30, 60)]
        coder.close()
        print(json.dumps({"profile": "frame_digest", "bits": b, "reps": reps, "frames": F, "width": W, "height": H,
                          "block_bytes": int(frames.nbytes), "digests_match_numpy_twin": ok, "library": nat.LIB_PATH}), flush=True)
        del frames
        gc.collect()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.profile:
        profile(a.reps, a.bits)
        return
    from new_bloom_filter_repo_amd import container
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16)
        enc, dec, facts = {False: [], True: []}, {False: [], True: []}, {}
        for run in range(a.runs):                          # alternating: both settings once per round
            for digests in (False, True):
                records, dt = encode(frames, a.interval, digests)
                enc[digests].append(dt)
                out, dt, integrity = decode(records)
                dec[digests].append(dt)
                if run == 0:
                    exact = all(np.array_equal(np.asarray(getattr(o, "data", o)), f) for o, f in zip(out, frames))
                    facts[digests] = {"container_bytes": container.size(records), "bit_exact": exact, "last_integrity": integrity}
                del records, out
        for digests in (False, True):
            print(json.dumps(dict({"leg": "frame_digest", "bits": bits, "width": a.width, "height": a.height, "frames": a.frames,
                                   "keyframe_interval": a.interval, "frame_digests": digests, "runs": a.runs,
                                   "compress_video_s_median": round(statistics.median(enc[digests]), 3),
                                   "decompress_video_s_median": round(statistics.median(dec[digests]), 3),
                                   "compress_video_s": [round(x, 3) for x in enc[digests]],
                                   "decompress_video_s": [round(x, 3) for x in dec[digests]]}, **facts[digests])), flush=True)
        del frames
        gc.collect()


if __name__ == "__main__":
    main()
