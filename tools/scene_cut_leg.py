#!/usr/bin/env python3
"""scene_cut_leg.py -- scene-cut detection (ImprovedVideoCompressor(scene_cuts=True)) on a clip that has cuts, and what it costs on one that
has none.  scene_cuts=False is the yardstick of the same run.

Default: a 1920x1080 8-bit YUV444 clip of 300 frames spliced from synthetic.make_camera_gop scenes every 75 frames (cuts at 75, 150 and
225; 150 is a keyframe by the rule already), keyframe interval 30, mask_channels="all"; scene_cuts off / on x zlib / rice x two modes --
max_error=0, and max_error=1 with hold_mode="lookahead" on the sensor_noise=1 version of the clip.  Per combination ONE JSON line with
the keyframe count, the cut list, the container bytes, the median compress_video seconds of --runs alternating runs (the combinations
take turns, so a drifting clock hits them alike) and the round trip through a fresh default compressor: bit-exact, or verify_max_error
plus "every cut frame is exact".  Then the same off / on pair on a clip WITHOUT a cut (one 300-frame scene, lossless): what the keyword
costs when it finds nothing.  --out: a file the lines are appended to.  Recorded: profiles/r16_scene_cuts.txt.

--profile: one 61-frame 1080p 8-bit block (frames 0..60 of the sensor_noise=1 scene: keyframes 30 and 60 inside) through one
GopCoder(max_error=2): load_frames, cut_stats, encode, --reps times on freshly uploaded frames -- k_cut_stats next to k_temporal_hold and
the mask kernel on the same block, for `rocprofv3 --kernel-trace --stats -- python tools/scene_cut_leg.py --profile` (kernel trace alone:
no counters in the same run)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"lossless": dict(max_error=0, sensor_noise=0), "lookahead1": dict(max_error=1, hold_mode="lookahead", sensor_noise=1)}


def spliced_clip(width, height, frames, scene_frames, sensor_noise):
    """Scenes of scene_frames frames (make_camera_gop seeds 2026, 2027, ...), one after the other; the scenes are independent: a thread each."""
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    lens = [min(scene_frames, frames - s) for s in range(0, frames, scene_frames)]
    with ThreadPoolExecutor(len(lens)) as pool:
        parts = list(pool.map(lambda a: make_camera_gop(2026 + a[0], width, height, a[1], sensor_noise=sensor_noise), enumerate(lens)))
    return [f for part in parts for f in part]


def encode(frames, interval, codec, mode, cuts):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    kw = {k: v for k, v in MODES[mode].items() if k != "sensor_noise"}
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec=codec, scene_cuts=cuts, **kw)
    gc.disable()
    t0 = time.perf_counter()
    res = comp.compress_video(list(frames), input_color_space="YUV")
    dt = time.perf_counter() - t0
    gc.enable()
    records, found, tm = comp.last_compressed_frames, list(comp.last_scene_cuts), dict(comp.last_timing)
    comp.close()
    return res, records, found, tm, dt


def describe(frames, records, res, found, tm, mode, interval):
    from new_bloom_filter_repo_amd.verify import verify_max_error
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    blob = ImprovedVideoCompressor._container(records)
    dec_comp = ImprovedVideoCompressor()                  # a fresh default decoder reads the container
    dec = dec_comp.decompress_video(compressed_frames=ImprovedVideoCompressor._parse_container(blob))
    dec_comp.close()
    dec = [np.asarray(getattr(d, "data", d)) for d in dec]
    me = MODES[mode]["max_error"]
    out = {"keyframes": res["keyframes"], "scene_cuts": found, "container_bytes": len(blob), "cut_stats_s": round(tm.get("cut_stats", 0.0), 4)}
    if me:
        out["verify_max_error"] = verify_max_error(frames, dec, me, keyframe_interval=interval)
        out["cut_frames_exact"] = all(np.array_equal(dec[t], frames[t]) for t in found)
    else:
        out["bit_exact"] = len(dec) == len(frames) and all(np.array_equal(d, f) for d, f in zip(dec, frames))
    return out


def profile(reps):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.container import cut_frames
    from new_bloom_filter_repo_amd.gop import GopCoder
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    W, H, F = 1920, 1080, 61
    frames = np.stack(make_camera_gop(2026, W, H, F, sensor_noise=1))
    ctx = nat.Context(0)
    coder = GopCoder(ctx, W, H, F, run_starts=[30, 60], mask_channels=3, max_error=2)
    found = None
    for _ in range(reps):
        coder.load_frames(frames)                         # (the hold rewrites the block: every repetition looks at the original frames)
        found = cut_frames(coder.cut_stats(tolerance=2), [30, 60])
        coder.encode()
        coder.results_packed()
    ctx.sync()
    coder.close()
    print(json.dumps({"profile": "scene_cuts", "max_error": 2, "reps": reps, "frames": F, "width": W, "height": H, "cuts_found": found}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--scene-frames", type=int, default=75)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--codecs", nargs="+", default=["zlib", "rice"])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-plain-clip", action="store_true", help="skip the clip without cuts")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        profile(a.reps)
        return

    def leg(clip_name, frames, mode, codecs):
        combos = [(codec, cuts) for codec in codecs for cuts in (False, True)]
        seconds, facts = {c: [] for c in combos}, {}
        for run in range(a.runs):                          # alternating: every combination once per round
            for codec, cuts in combos:
                res, records, found, tm, dt = encode(frames, a.interval, codec, mode, cuts)
                seconds[(codec, cuts)].append(dt)
                if run == 0:
                    facts[(codec, cuts)] = describe(frames, records, res, found, tm, mode, a.interval)
                del records
                print("run %d: %s %s %s scene_cuts=%s %.3f s" % (run, clip_name, mode, codec, cuts, dt), file=sys.stderr, flush=True)
        for codec, cuts in combos:
            row = dict({"leg": "scene_cuts", "clip": clip_name, "width": a.width, "height": a.height, "frames": len(frames),
                        "keyframe_interval": a.interval, "mode": mode, "sample_codec": codec, "scene_cuts_on": cuts,
                        "compress_video_s_median": round(statistics.median(seconds[(codec, cuts)]), 3), "runs": a.runs}, **facts[(codec, cuts)])
            if cuts:
                off = facts[(codec, False)]["container_bytes"]
                row["container_bytes_vs_off"] = round(row["container_bytes"] / off, 4)
                row["seconds_vs_off"] = round(statistics.median(seconds[(codec, True)]) / statistics.median(seconds[(codec, False)]), 3)
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")

    for mode in a.modes:
        frames = spliced_clip(a.width, a.height, a.frames, a.scene_frames, MODES[mode]["sensor_noise"])
        leg("spliced_every_%d" % a.scene_frames, frames, mode, a.codecs)
        del frames
        gc.collect()
    if not a.no_plain_clip:
        frames = spliced_clip(a.width, a.height, a.frames, a.frames, 0)
        leg("one_scene", frames, "lossless", a.codecs)


if __name__ == "__main__":
    main()
