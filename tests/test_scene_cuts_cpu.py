"""Scene-cut detection without a GPU: the statistic's reference (scene_cut_ref.py) on the values include/rbf.h pins, the rule on spliced
clips and on a clip without a cut, container.cut_frames, the keyword's validation, and the additive C ABI entry."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container, dist
from new_bloom_filter_repo_amd.synthetic import make_gop
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor, _BlockRecords
from scene_cut_ref import cut_frames, cut_stats, glen, ratio, rice_map, two_scenes


def test_glen_table():
    assert [int(glen(u)) for u in (0, 1, 2, 255, 65535)] == [1, 3, 3, 17, 33]
    assert [int(glen(u)) for u in (3, 6, 7, 254, 256, 65534)] == [5, 5, 7, 15, 17, 31]
    u = np.arange(0, 70000)
    assert np.array_equal(glen(u), 2 * np.floor(np.log2(u + 1.0)).astype(np.int64) + 1)
    # the mapping is the sample codec's: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...; the far end of the range is 2^B - 1
    assert [int(rice_map(d, 8)) for d in (0, -1, 1, -2, 127, 128, -128)] == [0, 1, 2, 3, 254, 255, 255]
    assert int(rice_map(0x8000, 16)) == 65535 and int(glen(rice_map(0x8000, 16))) == 33


def test_glen_of_a_residual_needs_no_mapping():
    """What the kernels compute (rbf_kernels_cut.h): glen(rice_map(d)) = 65 - 2 clz32(|s|), |s| = min(|d|, 2^B - |d|) -- for every residual."""
    for bits in (8, 16):
        full = 1 << bits
        d = np.arange(-full + 1, full)                          # x - pred of two B-bit samples
        a = np.abs(d)
        s = np.minimum(a, full - a)
        clz = np.where(s == 0, 32, 31 - np.floor(np.log2(np.maximum(s, 1))).astype(np.int64))
        assert np.array_equal(glen(rice_map(d, bits)), 65 - 2 * clz), bits


def test_stats_by_hand():
    """Two 2x3 single-channel frames small enough to do on paper."""
    a = np.array([[10, 10, 10], [10, 10, 10]], dtype=np.uint8)
    b = np.array([[10, 11, 10], [12, 10, 7]], dtype=np.uint8)
    s = cut_stats(np.stack([a, b]), 0)
    # moving: 11, 12, 7.  inter: d = 1, 2, -3 -> u = 2, 4, 5 -> glen 3, 5, 5
    # intra preds: 0, 10, 11 | 10 (above), 12, 10 -> d = 10, 1, -1 | 2, -2, -3 -> u = 20, 2, 1 | 4, 3, 5 -> glen 9, 3, 3 | 5, 5, 5
    assert s.tolist() == [[3, 13, 30]]
    assert cut_stats(np.stack([a, b]), 2).tolist() == [[1, 5, 30]]
    assert cut_stats(np.stack([a, b]), 255).tolist() == [[0, 0, 30]]
    x = np.zeros((2, 1, 2), dtype=np.uint16)
    x[1, 0, 0] = 0x8000                                          # the true unsigned difference: 32768 apart
    # pixel 0 moves: u = 65535, 33 bits; pixel 1 does not (and is not counted).  intra: 0x8000 against 0, then 0 against 0x8000: 33 each
    assert cut_stats(x, 32767).tolist() == [[1, 33, 33 + 33]]
    assert cut_stats(x, 32768).tolist() == [[0, 0, 66]]


CONFIGS = [(np.uint8, 0, 0), (np.uint8, 1, 2), (np.uint8, 2, 4), (np.uint16, 0, 0), (np.uint16, 1, 2), (np.uint16, 2, 4)]


@pytest.mark.parametrize("dtype,noise,tol", CONFIGS, ids=["%s_noise%d_tol%d" % (np.dtype(d).name, a, t) for d, a, t in CONFIGS])
def test_rule_finds_the_splice_of_two_scenes(dtype, noise, tol):
    clip = two_scenes(320, 180, 6, dtype=dtype, sensor_noise=noise)
    stats = cut_stats(clip, tol)
    ratios = [ratio(r) for r in stats]
    print(np.dtype(dtype).name, noise, tol, ["%.4f" % r for r in ratios])
    assert cut_frames(stats) == [6] == container.cut_frames(stats)
    assert all(r <= 0.02 for j, r in enumerate(ratios, start=1) if j != 6), ratios
    assert ratios[5] >= 1.63, ratios


def test_rule_finds_no_cut_in_a_clip_without_one():
    stats = cut_stats(np.stack(make_gop(5, 320, 180, 6)), 0)
    ratios = [ratio(r) for r in stats]
    print(["%.4f" % r for r in ratios])
    assert cut_frames(stats) == [] == container.cut_frames(stats)
    assert all(abs(r - 0.09) < 0.01 for r in ratios), ratios


def test_cut_frames_applies_the_rule_and_skips_run_starts():
    stats = np.array([[5, 100, 50], [5, 10, 50], [5, 46, 50], [5, 45, 50], [0, 0, 0], [1, 2 ** 40, 2 ** 40]], dtype=np.uint64)
    for fn in (container.cut_frames, cut_frames):
        assert fn(stats) == [1, 3, 6], "strictly greater; integers beyond 2^32"
        assert fn(stats, run_starts=[3]) == [1, 6]
        assert fn(stats, run_starts=(1, 3, 6)) == []
        assert fn(stats[:0]) == []
    assert container.cut_frames([(1, 2, 2)]) == [1] and container.cut_frames([(0, 2, 2)]) == []


def test_surface_keyword_and_its_refusals():
    sig = inspect.signature(ImprovedVideoCompressor.__init__)
    assert sig.parameters["scene_cuts"].default is False
    comp = ImprovedVideoCompressor()
    assert comp.scene_cuts is False and comp.last_scene_cuts == []
    assert ImprovedVideoCompressor(scene_cuts=True, mask_channels="all").scene_cuts is True
    for kw in (dict(gop_batching=False), dict(inter_frames=False), dict(keyframe_interval=1)):
        with pytest.raises(ValueError, match="scene_cuts"):
            ImprovedVideoCompressor(scene_cuts=True, **kw)
        ImprovedVideoCompressor(scene_cuts=False, **kw)
    assert _BlockRecords().cuts == ()
    assert inspect.signature(dist.encode_video_sharded).parameters["scene_cuts"].default is False


def test_header_declares_the_entry_additively():
    hdr = open(os.path.join(REPO, "include", "rbf.h"), encoding="utf-8").read()
    assert re.search(r"\bint\s+rbf_cut_stats\s*\(", hdr)
    assert nat._PROTOS["rbf_cut_stats"] == (nat._int, [nat._vp, nat._vp, nat._u64, nat._u32, nat._u32, nat._u32, nat._u32, nat._u32, nat._u32, nat._vp])
    assert int(re.search(r"#define\s+RBF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4, "additive: the ABI version stays"
    ids = re.findall(r"#define\s+(RBF_K_\w+)\s+(\d+)", hdr)
    assert len(ids) == 15 and dict(ids)["RBF_K_COUNT"] == "14", "no new RBF_K_ id: the statistic is not a timed kernel of the step"
    doc = open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8").read()
    assert "rbf_cut_stats" in doc
    api = open(os.path.join(REPO, "new_bloom_filter_repo_amd", "csrc", "rbf_api.hip"), encoding="utf-8").read()
    assert '#include "rbf_kernels_cut.h"' in api and re.search(r"\bint\s+rbf_cut_stats\s*\(", api)
