#!/usr/bin/env python3
"""sample_codec_leg.py -- the GPU sample codec (ImprovedVideoCompressor(sample_codec="rice")) against the zlib-9 record formats on the
camera-like clip of tools/mask_channels_leg.py (synthetic.make_camera_gop, seed 2026: 1920x1080 YUV444, 300 frames, keyframe interval 30).

Default: per (mask mode, bits, sample codec) ONE JSON line: keyframes, container bytes split into keyframe and inter-frame records,
compress_video / decompress_video seconds as the median of --reps runs (the zlib and rice runs alternate in the same call; decode by a fresh
default compressor) and whether the decoded clip is bit-exact.  Recorded: profiles/r08_sample_codec_leg.txt.

--profile: one 61-frame 1080p 16-bit block (frames 0..60, two keyframes inside, the all-channel mask) through one GopCoder with its
residual streams, the streams applied back onto their predecessors, and five keyframes encoded and decoded, --reps times, for
`rocprofv3 --kernel-trace --stats -- python tools/sample_codec_leg.py --profile`.  Recorded: profiles/r08_sample_codec_kernel_stats_1080p16.csv."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(frames, mode, codec, interval):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels=mode, sample_codec=codec)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    t_c = time.perf_counter() - t0
    gc.enable()
    recs = comp.last_compressed_frames
    comp.close()
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads either codec's container
    t0 = time.perf_counter()
    dec = dec_comp.decompress_video(compressed_frames=recs)
    t_d = time.perf_counter() - t0
    dec_comp.close()
    return res, recs, dec, t_c, t_d


def leg(frames, bits, mode, interval, reps):
    from new_bloom_filter_repo_amd.verify import verify_bit_exact
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    times = {"zlib": ([], []), "rice": ([], [])}
    rows = {}
    for rep in range(reps):
        for codec in ("zlib", "rice"):                    # alternating: both codecs see the same machine state
            res, recs, dec, t_c, t_d = run(frames, mode, codec, interval)
            times[codec][0].append(t_c)
            times[codec][1].append(t_d)
            if rep == 0:
                key = sum(4 + 1 + len(r) for ty, r in recs if ty in (1, 3))
                inter = sum(4 + 1 + len(r) for ty, r in recs if ty in (2, 4))
                rows[codec] = {"keyframes": res["keyframes"], "container_bytes": ImprovedVideoCompressor._container_size(recs),
                               "keyframe_record_bytes": key, "inter_record_bytes": inter,
                               "record_types": sorted({ty for ty, _ in recs}),
                               "bit_exact": bool(verify_bit_exact(frames, dec, color_space="YUV")["success"])}
            del res, recs, dec
            gc.collect()
    H, W = frames[0].shape[:2]
    out = []
    for codec in ("zlib", "rice"):
        r = {"leg": "sample_codec", "mode": mode, "bits": bits, "sample_codec": codec, "width": W, "height": H, "frames": len(frames),
             "keyframe_interval": interval}
        r.update(rows[codec])
        r["compress_video_s"] = round(statistics.median(times[codec][0]), 3)
        r["decompress_video_s"] = round(statistics.median(times[codec][1]), 3)
        r["runs_compress_s"] = [round(t, 3) for t in times[codec][0]]
        r["runs_decompress_s"] = [round(t, 3) for t in times[codec][1]]
        out.append(r)
    z, c = out
    c["container_vs_zlib"] = round(c["container_bytes"] / z["container_bytes"], 4)
    c["compress_vs_zlib"] = round(c["compress_video_s"] / z["compress_video_s"], 3)
    c["decompress_vs_zlib"] = round(c["decompress_video_s"] / z["decompress_video_s"], 3)
    return out


def profile(reps):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.sample_codec import SampleCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F, dtype=np.uint16))
    ctx = nat.Context(0)
    codec = SampleCoder(ctx)
    coder = GopCoder(ctx, W, H, F, sample_bytes=2, run_starts=[30, 60], mask_channels=3)
    coder.load_frames(frames)
    keys = [frames[i] for i in (0, 15, 30, 45, 60)]
    sizes = []
    for _ in range(reps):
        coder.encode()
        rows = coder.results_packed()
        res = coder.results()
        streams = coder.rice_streams([r["ones"] for r in rows], codec)
        codec.apply_chain(frames[0], [r["mask"] for r in res[:29]], streams[:29])
        kstreams = codec.encode_frames(keys[:4]) + codec.encode_frames(keys[4:])
        for s in kstreams:
            codec.decode_frame(s, H, W, 3, 2)
        sizes = [len(s) for s in kstreams]
    ctx.sync()
    coder.close()
    codec.close()
    print(json.dumps({"profile": "sample_codec", "reps": reps, "frames": F, "width": W, "height": H, "bits": 16, "keyframe_stream_bytes": sizes}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--modes", nargs="+", default=["all", "luma"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        profile(a.reps)
        return
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16)
        for mode in a.modes:
            for row in leg(frames, bits, mode, a.interval, a.reps):
                print(json.dumps(row), flush=True)
        del frames
        gc.collect()


if __name__ == "__main__":
    main()
