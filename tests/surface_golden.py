"""What the video surface does today, pinned as data: the constructor's outcome over a grid of keywords (tests/golden/surface_refusals.json)
and one compress + decompress per feature configuration on small synthetic clips (tests/golden/surface_containers.json).  Shared by
tools/gen_surface_golden.py, which writes the two files, and by test_surface_options_cpu.py / test_gpu_surface_golden.py, which recompute
them.  Public API only, so the same file runs against an older checkout of the package."""
import hashlib
import itertools
import json
import os
import string
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFUSALS = os.path.join(GOLDEN, "surface_refusals.json")
CONTAINERS = os.path.join(GOLDEN, "surface_containers.json")

# ---------------------------------------------------------------------------------------------------------------------- the constructor
_MAP = np.zeros((4, 6), dtype=np.int64)
_MAP[1, 2] = 3
GRID = [("gop_batching", [True, False]),
        ("inter_frames", [None, False, True]),
        ("keyframe_interval", [1, 30]),
        ("mask_channels", ["luma", "all", "bad"]),
        ("sample_codec", ["zlib", "rice", "x"]),
        ("max_error", [0, 2, -1, True]),
        ("hold_mode", ["first", "lookahead", "x"]),
        ("scene_cuts", [False, True]),
        ("error_bounds", [None, (1, 2, 2), _MAP, "2"]),
        ("pan_range", [0, 4, 33, True]),
        ("bounded_keyframes", [False, True])]
SYMBOLS = string.ascii_letters + string.digits


def grid_description():
    """The grid as JSON data (an array is named, not spelled out)."""
    return {name: ["int64 array (4, 6), [1, 2] = 3, else 0" if isinstance(v, np.ndarray) else repr(v) for v in values] for name, values in GRID}


def constructor_outcome(cls, kw):
    """'ok', or '<exception type>: <message>' of cls(**kw)."""
    try:
        cls(**kw)
    except Exception as e:                       # noqa: BLE001  (whatever it raises is the outcome)
        return "%s: %s" % (type(e).__name__, e)
    return "ok"


def refusal_table(cls):
    """(outcomes, index): the distinct outcomes of the grid in order of first appearance, and one character of SYMBOLS per combination
    (itertools.product order, the last keyword fastest)."""
    names = [name for name, _ in GRID]
    outcomes, index = [], []
    for values in itertools.product(*[v for _, v in GRID]):
        o = constructor_outcome(cls, dict(zip(names, values)))
        if o not in outcomes:
            outcomes.append(o)
        index.append(SYMBOLS[outcomes.index(o)])
    return outcomes, "".join(index)


# ---------------------------------------------------------------------------------------------------------------------- the containers
W, H, T, I, B = 96, 64, 19, 4, 8                 # frames of W x H; T frames, a keyframe every I, blocks of B: two full blocks and a tail of 3
_clips = {}


def clip(name):
    """The clips of the configurations, built once: lists of T frames."""
    if name not in _clips:
        from new_bloom_filter_repo_amd.synthetic import make_camera_gop, make_gop, make_panning_gop
        if name == "gop8":
            frames = make_gop(701, W, H, T, p=0.08)
        elif name == "gop16":
            frames = make_gop(702, W, H, T, p=0.08, dtype=np.uint16)
        elif name == "chroma_only":              # frame 5 is frame 4 with one chroma sample changed: the luma mask cannot say that
            frames = [f.copy() for f in clip("gop8")]
            frames[5] = frames[4].copy()
            frames[5][3, 7, 1] ^= 1
        elif name == "camera":
            frames = make_camera_gop(703, W, H, T)
        elif name == "grey":
            frames = [np.ascontiguousarray(f[:, :, 0]) for f in clip("gop8")]
        elif name == "odd_shape":                # frame 10 has another width: its block cannot be batched
            frames = [f.copy() for f in clip("gop8")]
            frames[10] = np.ascontiguousarray(frames[10][:, :W - 2])
        elif name == "noise1":
            frames = make_camera_gop(704, W, H, T, sensor_noise=1)
        elif name == "noise2":
            frames = make_camera_gop(705, W, H, T, sensor_noise=2)
        elif name == "splice":                   # two scenes, the second from frame 10 on (no keyframe of the rule)
            frames = make_camera_gop(706, W, H, T, sensor_noise=1)[:10] + make_camera_gop(707, W, H, T, sensor_noise=1)[10:]
        elif name == "pan":
            frames = make_panning_gop(708, W, H, T, (2, 1))
        elif name == "pan_splice":               # the second scene starts at frame 10, inside the panned run 8 .. 11
            frames = make_panning_gop(11, W, H, T, (2, 1))[:10] + make_panning_gop(12, W, H, T, (2, 1))[10:]
        else:
            raise KeyError(name)
        _clips[name] = frames
    return _clips[name]


def _bound_map():
    e = np.full((H, W), 2, dtype=np.int64)
    e[:16, :32] = 0
    return e


# (name, clip, constructor keywords besides keyframe_interval=I and block_frames=B, keywords of this file)
#   color_space: compress_video's; shards: [(start, stop)] coded by encode_range one after the other, each from its halo frame on
CONFIGS = [
    ("defaults", "gop8", {}, {}),
    ("uint16_all", "gop16", dict(mask_channels="all"), {}),
    ("luma_chroma_only_frame", "chroma_only", {}, {}),
    ("rice_all", "camera", dict(mask_channels="all", sample_codec="rice"), {}),
    ("frame_by_frame_zlib", "gop8", dict(gop_batching=False), {}),
    ("frame_by_frame_rice", "gop8", dict(gop_batching=False, sample_codec="rice"), {}),
    ("all_keyframes", "gop8", dict(inter_frames=False), {}),
    ("grey", "grey", dict(inter_frames=True), dict(color_space="BGR")),
    ("odd_shape", "odd_shape", {}, {}),
    ("max_error_2", "noise1", dict(mask_channels="all", max_error=2), {}),
    ("lookahead_2", "noise2", dict(mask_channels="all", max_error=2, hold_mode="lookahead"), {}),
    ("bounds_uniform", "noise1", dict(mask_channels="all", error_bounds=(2, 2, 2)), {}),
    ("bounds_channels", "noise1", dict(mask_channels="all", error_bounds=(1, 3, 3)), {}),
    ("bounds_map", "noise1", dict(mask_channels="all", error_bounds=_bound_map()), {}),
    ("scene_cuts", "splice", dict(mask_channels="all", scene_cuts=True), {}),
    ("scene_cuts_max_error_2", "splice", dict(mask_channels="all", scene_cuts=True, max_error=2), {}),
    ("pan", "pan", dict(mask_channels="all", pan_range=4), {}),
    ("pan_cut_digests_quality", "pan_splice", dict(mask_channels="all", pan_range=4, scene_cuts=True, frame_digests=True, quality_report=True), {}),
    ("digests", "gop8", dict(frame_digests=True), {}),
    ("defaults_one_lane", "gop8", dict(gpu_lanes=1), {}),
    ("defaults_blocks_of_6", "gop8", dict(block_frames=6), {}),
    ("shards", "gop8", {}, dict(shards=[(0, 6), (6, T)])),
    ("bounded_keyframes", "noise1", dict(mask_channels="all", sample_codec="rice", max_error=2, bounded_keyframes=True), {}),
]
SAME_BYTES = [("bounds_uniform", "max_error_2"), ("defaults_one_lane", "defaults"), ("defaults_blocks_of_6", "defaults")]
QUALITY_INTS = ("max_abs_error", "changed_samples", "over_bound")


def canonical_hash(records):
    """sha256 over a container's records in a form that does not depend on the zlib build: per record the type byte, then for type 1 the
    decoded frame (shape, dtype, whether it carries planes, bytes), for type 2 the record's fields with the value field inflated, for types
    3 to 7 the raw body."""
    from new_bloom_filter_repo_amd.frame_codec import FixedVideoCompressor, YUVFrame, frame_data, parse_record
    h = hashlib.sha256()
    keys = FixedVideoCompressor(verbose=False)
    for ty, rec in records:
        h.update(struct.pack("<B", ty))
        if ty == 1:
            frame = keys.decompress_frame(rec)
            a = frame_data(frame)
            h.update(repr((a.shape, a.dtype.str, isinstance(frame, YUVFrame))).encode())
            h.update(np.ascontiguousarray(a).tobytes())
        elif ty == 2:
            d = parse_record("f64", rec[1:])
            h.update(rec[:1])
            h.update(struct.pack("<fIdIII", d["p"], d["n"], d["k"], d["bitmap_bits"], d["witness_bits"], d["value_count"]))
            for part in (bytes(d["bitmap"]), bytes(d["witness"]), zlib.decompress(d["values_z"])):
                h.update(struct.pack("<I", len(part)))
                h.update(part)
        else:
            h.update(struct.pack("<I", len(rec)))
            h.update(bytes(rec))
    return h.hexdigest()


def run_config(name):
    """One configuration: compress, then decompress with a fresh default compressor; the entry of surface_containers.json."""
    from new_bloom_filter_repo_amd import container
    from new_bloom_filter_repo_amd.dist import halo_start
    from new_bloom_filter_repo_amd.frame_codec import frame_data
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    _, clip_name, kw, extra = next(c for c in CONFIGS if c[0] == name)
    frames = [f.copy() for f in clip(clip_name)]
    kw = dict(dict(keyframe_interval=I, block_frames=B), **kw)
    entry = {}
    with ImprovedVideoCompressor(**kw) as comp:
        if "shards" in extra:
            records = []
            for start, stop in extra["shards"]:
                first = halo_start(start, I)
                records += comp.encode_range(frames[first:], first, start, stop)
        else:
            comp.compress_video(frames, input_color_space=extra.get("color_space", "YUV"))
            records = comp.last_compressed_frames
        entry["scene_cuts"] = [int(t) for t in comp.last_scene_cuts]
        entry["pans"] = [[int(v) for v in row] for row in comp.last_pans]
        entry["pan_offsets"] = {str(k): [int(v[0]), int(v[1])] for k, v in sorted(comp.last_pan_offsets.items())}
        entry["digests"] = None if comp.last_digests is None else ["%016x" % d for d in comp.last_digests]
        entry["quality"] = None if comp.last_quality is None else [[int(row[k]) for k in QUALITY_INTS] for row in comp.last_quality]
    blob = container.write(records)
    entry["canonical_sha256"] = canonical_hash(records)
    entry["container_bytes"] = len(blob)
    entry["types"] = "".join(str(ty) for ty, _ in records)
    with ImprovedVideoCompressor() as fresh:
        decoded = fresh.decompress_video(compressed_frames=container.parse(blob))
        entry["integrity"] = fresh.last_integrity
    h = hashlib.sha256()
    for f in decoded:
        a = np.ascontiguousarray(frame_data(f))
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    entry["decoded_sha256"] = h.hexdigest()
    entry["decoded_frames"] = len(decoded)
    return entry


def load(path):
    with open(path, encoding="utf-8") as f:
        return json.load(f)
