"""The product side of the surface sweeps (test_gpu_surface_twin.py, test_gpu_surface_geometries.py): compress a clip, write and parse
the container, decode it with a fresh compressor -- and the ONE comparison of what came out with what surface_twin.twin predicts.  A test
helper: not collected.  Needs the native library and a GPU."""
import numpy as np

from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.integrity import build_trailer
from new_bloom_filter_repo_amd.verify import verify_max_error
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor


def encode_with(comp, clip, color_space, shards=None, I=None):
    """The container `comp` writes for the clip as [(type, record)] -- frame records, then the pan table and the digest trailer as
    compress_video appends them -- and what the call left behind (compress_video: with its last_timing).  shards: [(start, stop)] for
    encode_range, each from its halo frame on (I: the keyframe interval)."""
    frames = [f.copy() for f in clip]
    if shards is None:
        comp.compress_video(frames, input_color_space=color_space)
        records = list(comp.last_compressed_frames)
        out = dict(scene_cuts=list(comp.last_scene_cuts), pans=list(comp.last_pans), pan_offsets=dict(comp.last_pan_offsets),
                   digests=comp.last_digests, quality=comp.last_quality, timing=dict(comp.last_timing))
    else:
        if color_space == "YUV":                 # what compress_video does to YUV input before it plans the ranges
            frames = [comp.compressor.add_yuv_info_to_frame(f) for f in frames]
        records, out = [], dict(scene_cuts=[], pans=[], pan_offsets={}, digests=[], quality=[])
        for start, stop in shards:
            first = start if start % I == 0 else start - 1
            records += comp.encode_range(frames[first:], first, start, stop)
            out["scene_cuts"] += comp.last_scene_cuts
            out["pans"] += comp.last_pans
            out["pan_offsets"].update({start + k: v for k, v in comp.last_pan_offsets.items()})
            out["digests"] = None if comp.last_digests is None else out["digests"] + comp.last_digests
            out["quality"] = None if comp.last_quality is None else out["quality"] + comp.last_quality
        if out["pan_offsets"]:
            records.append((container.PANS, container.build_pans(out["pan_offsets"])))
        if out["digests"] is not None:
            records.append((container.DIGESTS, build_trailer(out["digests"])))
    out["records"] = records
    return out


def encode(clip, keywords, color_space, shards=None):
    """encode_with on a compressor of its own."""
    with ImprovedVideoCompressor(**keywords) as comp:
        return encode_with(comp, clip, color_space, shards, keywords["keyframe_interval"])


def decode_with(dec, records):
    """The frames `dec` rebuilds from the written and parsed container, and its last_integrity."""
    out = dec.decompress_video(compressed_frames=container.parse(container.write(records)))
    return [np.asarray(getattr(d, "data", d)) for d in out], dec.last_integrity


def decode(records, **how):
    """decode_with on a fresh default compressor.  how: constructor keywords of the decoder, and chain_chunk_frames."""
    chunk = how.pop("chain_chunk_frames", None)
    fresh = ImprovedVideoCompressor(**how)
    if chunk:
        fresh.chain_chunk_frames = chunk
    try:
        return decode_with(fresh, records)
    finally:
        fresh.close()


def same_frames(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def assert_is_twin(got, tw, x, keywords):
    """Everything the twin predicts, bit for bit.  got: encode()'s dict with `decoded` and `integrity` from decode(); tw: twin()'s
    dict; x: the clip; keywords: the constructor's."""
    T = len(x)
    assert [ty for ty, _ in got["records"]] == tw["kinds"]
    assert got["scene_cuts"] == tw["scene_cuts"]
    assert [tuple(int(v) for v in row) for row in got["pans"]] == tw["pans"]
    assert {int(i): (int(o[0]), int(o[1])) for i, o in got["pan_offsets"].items()} == tw["pan_offsets"]
    bad = [t for t, (a, b) in enumerate(zip(got["decoded"], tw["decoded"])) if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b)]
    assert len(got["decoded"]) == T and not bad, bad
    if keywords.get("frame_digests"):
        assert [int(d) for d in got["digests"]] == tw["digests"]
        assert got["integrity"]["frames"] == got["integrity"]["checked"] == T
    else:
        assert got["digests"] is None and got["integrity"]["checked"] == 0
    if keywords.get("quality_report"):
        rows = tw["quality"]
        assert [(q["max_abs_error"], q["changed_samples"], q["over_bound"]) for q in got["quality"]] == \
               [(int(r["max_abs"]), int(r["differing"]), int(r["over_bound"])) for r in rows]
        samples = x[0].size
        assert [q["mse"] for q in got["quality"]] == [int(r["sse"]) / samples for r in rows]
    else:
        assert got["quality"] is None
    if not keywords.get("max_error") and keywords.get("error_bounds") is None:
        assert same_frames(got["decoded"], x)
    else:
        v = verify_max_error(list(x), got["decoded"], keywords["max_error"] if "max_error" in keywords else keywords["error_bounds"])
        assert v["within_bound"] and v["frame_count"] == T, v
