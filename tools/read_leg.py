#!/usr/bin/env python3
"""read_leg.py -- what reading PART of a container costs (ImprovedVideoCompressor.read_frames) next to reading all of it.
decompress_video is the yardstick of the same run.

Default: a 1920x1080 YUV444 camera clip (synthetic.make_camera_gop) of 300 frames, keyframe interval 30, mask_channels="all",
sample_codec="rice", 8 and 16 bits; per (bits, row) ONE JSON line with the median wall seconds of --runs alternating runs (the rows take
turns inside every run, so a drifting clock hits them alike), last_read of the first run, and the bytes downloaded.  Rows:
decompress_video | read_frames of the whole clip at scale 1, 2, 4, 8 | the whole clip, a 256x256 region | the whole clip, a ragged
1001x601 region at (16, 1) at scale 2 (both kernels of the view in one call) | frames 135..164 at full size | every 10th frame at scale
4.  Every row's frames are checked against the numpy twin (view.view_host) of decompress_video's in the first run.
--out FILE appends every JSON line to FILE as well: the lines of profiles/r22_read_frames.txt are this tool's, as it wrote them.

--yardstick [--root TREE] [--label NAME]: decompress_video alone, of the package in TREE (default: this tree), and a digest of the frames
it returned -- one process per tree, taking turns, is how this tree is held against its parent commit.  The line names the tree by
NAME and the library by its path inside the tree.

--profile: ONE 41-frame chunk of the 8-bit clip (a keyframe and 41 type-4 records) through SampleCoder.apply_chain, --reps times without
a view, with the whole frame at scales 1 and 4 and with the ragged region at scale 2, so that k_frame_view and k_frame_view_px stand
next to k_rice_inter_add of the same chunk in ONE `rocprofv3 --kernel-trace --stats -- python tools/read_leg.py --profile` (kernel trace
alone: no counters in the same run)."""
import argparse
import gc
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = None                                                 # --out: a file every JSON line is appended to


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def ragged_region(width, height):
    """A region whose rows start on 16 bytes (x0 = 16) and whose sides are odd: the wide kernel takes its whole tiles, the per-sample
    kernel its tail columns and its ragged last row, in one call."""
    return (16, 1, min(1001, width - 16), min(601, height - 1))


def data(f):
    return np.asarray(getattr(f, "data", f))


def encode(frames, interval):
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor(keyframe_interval=interval, mask_channels="all", sample_codec="rice")
    comp.compress_video(list(frames), input_color_space="YUV")
    records = list(comp.last_compressed_frames)
    comp.close()
    return records


def timed(fn):
    """(result, seconds) of fn(comp) on a fresh default compressor; the call ends with the frames on the host."""
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    comp = ImprovedVideoCompressor()
    gc.disable()
    t0 = time.perf_counter()
    out = fn(comp)
    dt = time.perf_counter() - t0
    gc.enable()
    info = getattr(comp, "last_read", None)
    comp.close()
    return out, dt, info


def rows_of(width, height, nframes):
    side = min(256, width, height)
    roi = ((width - side) // 2 // 16 * 16, (height - side) // 2, side, side)
    a, b = min(135, nframes // 2), min(165, nframes)
    return [("decompress_video", None),
            ("read_frames whole clip, scale 1", dict()),
            ("read_frames whole clip, scale 2", dict(scale=2)),
            ("read_frames whole clip, scale 4", dict(scale=4)),
            ("read_frames whole clip, scale 8", dict(scale=8)),
            ("read_frames whole clip, region %dx%d" % (side, side), dict(roi=roi)),
            ("read_frames whole clip, ragged region %dx%d at (16, 1), scale 2" % ragged_region(width, height)[2:], dict(roi=ragged_region(width, height), scale=2)),
            ("read_frames frames %d..%d, full size" % (a, b - 1), dict(start=a, stop=b)),
            ("read_frames every 10th frame, scale 4", dict(step=10, scale=4))]


def yardstick(a):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16)
        records = encode(frames, a.interval)
        times, sha = [], None
        for _ in range(a.runs + 1):                        # (the first run warms the process up and is not counted)
            out, dt, _ = timed(lambda comp: comp.decompress_video(compressed_frames=list(records)))
            times.append(dt)
            if sha is None:
                h = hashlib.sha256()
                for f in out:
                    h.update(np.ascontiguousarray(data(f)).tobytes())
                sha = h.hexdigest()[:16]
            del out
        emit({"leg": "read_frames yardstick", "tree": a.label, "library": os.path.relpath(nat.LIB_PATH, os.path.abspath(a.root)), "bits": bits,
              "frames": a.frames, "decompress_video_s_median": round(statistics.median(times[1:]), 3),
              "decompress_video_s": [round(x, 3) for x in times[1:]], "frames_sha256_16": sha})
        del frames, records
        gc.collect()


def profile(a):
    from new_bloom_filter_repo_amd import _native as nat
    from new_bloom_filter_repo_amd.sample_codec import SampleCoder, parse_key_record
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    from new_bloom_filter_repo_amd.view import View, view_host
    F = 42
    frames = make_camera_gop(2026, a.width, a.height, F, dtype=np.uint8)
    records = encode(frames, F)                            # one keyframe, 41 inter-frames: one chunk of the chain
    comp = ImprovedVideoCompressor()
    lane = comp._get_lanes(1)[0]
    whole = comp._decode_run(frames[0], [r for _, r in records[1:]], lane, types=[t for t, _ in records[1:]])
    ok = all(np.array_equal(data(w), f) for w, f in zip(whole, frames[1:]))
    for _ in range(a.reps):
        for roi, scale in ((None, None), (None, 1), (None, 4), (ragged_region(a.width, a.height), 2)):
            view = None if scale is None else View(roi, scale)
            got = comp._decode_run(frames[0], [r for _, r in records[1:]], lane, types=[t for t, _ in records[1:]], view=view)
            if scale:
                ok = ok and np.array_equal(data(got[-1]), view_host(frames[-1], roi, scale))
    lane.ctx.sync()
    comp.close()
    emit({"profile": "read_frames", "frames": F, "width": a.width, "height": a.height, "reps": a.reps, "views_match_numpy_twin": bool(ok),
          "library": os.path.relpath(nat.LIB_PATH, os.path.abspath(a.root))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--interval", type=int, default=30)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global OUT
    OUT = a.out
    sys.path.insert(0, os.path.abspath(a.root))
    if a.yardstick:
        return yardstick(a)
    if a.profile:
        return profile(a)
    from new_bloom_filter_repo_amd.synthetic import make_camera_gop
    from new_bloom_filter_repo_amd.view import view_host
    rows = rows_of(a.width, a.height, a.frames)
    for bits in a.bits:
        frames = make_camera_gop(2026, a.width, a.height, a.frames, dtype=np.uint8 if bits == 8 else np.uint16)
        records = encode(frames, a.interval)
        del frames
        gc.collect()
        times, facts, full = {name: [] for name, _ in rows}, {}, None
        for run in range(a.runs + 1):                      # (run 0 warms every row's shapes up and checks the frames; it is not counted)
            for name, kw in rows:                          # alternating: every row once per run
                if kw is None:
                    out, dt, info = timed(lambda comp: comp.decompress_video(compressed_frames=list(records)))
                else:
                    out, dt, info = timed(lambda comp: comp.read_frames(compressed_frames=list(records), **kw))
                if run == 0:
                    if kw is None:
                        full = [data(f) for f in out]
                        facts[name] = {"frames_returned": len(out), "downloaded_bytes": int(sum(f.nbytes for f in full))}
                    else:
                        want = full[kw.get("start", 0):kw.get("stop"):kw.get("step", 1)]
                        same = len(out) == len(want) and all(np.array_equal(data(o), view_host(w, kw.get("roi"), kw.get("scale", 1))) for o, w in zip(out, want))
                        facts[name] = dict(info, equals_view_host_of_decompress_video=bool(same))
                else:
                    times[name].append(dt)
                del out
        for name, _ in rows:
            emit(dict({"leg": "read_frames", "bits": bits, "width": a.width, "height": a.height, "frames": a.frames, "keyframe_interval": a.interval,
                       "row": name, "runs": a.runs, "seconds_median": round(statistics.median(times[name]), 4),
                       "seconds": [round(x, 4) for x in times[name]]}, **facts[name]))
        del records, full
        gc.collect()


if __name__ == "__main__":
    main()
