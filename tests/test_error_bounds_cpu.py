"""Near-lossless with a bound per sample, the CPU tier: the numpy references (tests/error_bounds_ref.py) keep the properties include/rbf.h
promises for rbf_temporal_hold_runs_map / rbf_temporal_lookahead_runs_map, container.bounds_frame normalises and refuses, the
constructors refuse what max_error > 0 refuses, verify_max_error takes a bound frame, and the new kernels use no scratch."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from error_bounds_ref import (ROW, error_stats_ref, hold_map_ref, hold_ref, lookahead_map_ref, lookahead_ref, random_clip, test_bounds,
                              update_counts)
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.gop import GopCoder
from new_bloom_filter_repo_amd.verify import quality_rows, verify_max_error
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = [(3, np.uint8), (3, np.uint16), (4, np.uint8), (0, np.uint8), (0, np.uint16), (2, np.uint16)]
IDS = ["c%d_%s" % (c, np.dtype(d).name) for c, d in SWEEP]
STARTS = [4, 5]


def clip_of(C, dtype):
    return random_clip(100 * C + 67, 9, 5, 67, C, dtype)


@pytest.mark.parametrize("C,dtype", SWEEP, ids=IDS)
def test_uniform_bound_frame_is_the_scalar_rule(C, dtype):
    x = clip_of(C, dtype)
    for d in (0, 1, 3, int(np.iinfo(dtype).max)):
        E = np.full(x.shape[1:], d, dtype=dtype)
        assert np.array_equal(hold_map_ref(x, STARTS, E), hold_ref(x, STARTS, d)), d
        y, s = lookahead_map_ref(x, STARTS, E)
        y0, s0 = lookahead_ref(x, STARTS, d)
        assert np.array_equal(y, y0) and np.array_equal(s, s0), d


@pytest.mark.parametrize("C,dtype", SWEEP, ids=IDS)
def test_properties_under_a_bound_per_sample(C, dtype):
    x = clip_of(C, dtype)
    E, rect = test_bounds(x.shape[1:], dtype, seed=C)
    top = int(np.iinfo(dtype).max)
    assert (E[rect] == 0).all() and (E[:, -2:] == top).all() and 0 < E[0, :-2].max() <= 300
    assert dtype == np.uint8 or (E == 300).any()
    held = hold_map_ref(x, STARTS, E)
    ahead, _ = lookahead_map_ref(x, STARTS, E)
    for y in (held, ahead):
        assert (np.abs(y.astype(np.int64) - x.astype(np.int64)) <= E.astype(np.int64)).all(), "|y - x| <= E everywhere"
        for t in [0] + STARTS:
            assert np.array_equal(y[t], x[t]), "a run's first frame is exact"
        assert np.array_equal(y[(slice(None),) + rect], x[(slice(None),) + rect]), "bounds of zero: exact in every frame"
        assert not np.array_equal(y, x), "the clip moves by less than some bounds: something is held"
    assert np.array_equal(hold_map_ref(held, STARTS, E), held), "the hold is idempotent"
    assert (update_counts(ahead, STARTS) <= update_counts(held, STARTS)).all(), "the look-ahead never updates a pixel more often"


def test_bounds_frame_normalises_the_three_forms():
    H, W, C = 5, 7, 3
    E = container.bounds_frame((1, 2, 3), (H, W, C), np.uint8)
    assert E.shape == (H, W, C) and E.dtype == np.uint8 and (E == np.array([1, 2, 3])).all()
    assert np.array_equal(container.bounds_frame([1, 2, 3], (H, W, C), np.uint16), E.astype(np.uint16))
    m = np.arange(H * W).reshape(H, W)
    E = container.bounds_frame(m, (H, W, C), np.uint16)
    assert E.shape == (H, W, C) and E.dtype == np.uint16 and all(np.array_equal(E[..., c], m) for c in range(C))
    full = np.arange(H * W * C, dtype=np.int32).reshape(H, W, C)
    E = container.bounds_frame(full, (H, W, C), np.uint8)
    assert E.dtype == np.uint8 and np.array_equal(E, full) and E.flags.c_contiguous
    assert np.array_equal(container.bounds_frame(m.astype(np.uint8), (H, W), np.uint8), m)      # gray frames: the (H, W) form
    assert np.array_equal(container.bounds_frame([4], (H, W), np.uint8), np.full((H, W), 4))
    assert container.bounds_frame((65535, 0, 7), (H, W, C), np.uint16)[0, 0, 0] == 65535
    assert container.uniform_bound(np.full((H, W, C), 2, dtype=np.uint8)) == 2 and container.uniform_bound(E) is None
    assert container.bounds_frame((1, 2, 3)).tolist() == [1, 2, 3]                              # without a frame: the values only
    assert "_native" not in inspect.getsource(container), "the bound frame is host work: no native library"


@pytest.mark.parametrize("bad", ["2", "123", 1.5, (1.0, 2.0, 2.0), np.ones((5, 7)), True, (True, 1, 2), np.ones((5, 7), dtype=bool), (-1, 2, 2),
                                 np.full((5, 7), -3), (1, 2, 256), np.full((5, 7, 3), 256), (1, 2), (1, 2, 3, 4), np.ones((7, 5), dtype=np.uint8),
                                 np.ones((5, 7, 4), dtype=np.uint8), np.ones((1, 5, 7, 3), dtype=np.uint8), 3, None, [], [[1, 2], [3]]],
                         ids=lambda b: re.sub(r"\W+", "_", repr(b))[:24])
def test_bounds_frame_refuses(bad):
    with pytest.raises(ValueError):
        container.bounds_frame(bad, (5, 7, 3), np.uint8)


def test_bounds_frame_fits_the_sample_width():
    assert container.bounds_frame((1, 2, 256), (5, 7, 3), np.uint16)[0, 0, 2] == 256
    with pytest.raises(ValueError, match="16-bit"):
        container.bounds_frame((1, 2, 65536), (5, 7, 3), np.uint16)
    with pytest.raises(ValueError):
        container.bounds_frame((1, 2, 3), (5, 7, 3), np.float32)


def test_surface_keywords_and_their_refusals():
    sig = inspect.signature(ImprovedVideoCompressor.__init__)
    assert sig.parameters["error_bounds"].default is None and sig.parameters["quality_report"].default is False
    assert sig.parameters["max_error"].default == 0
    comp = ImprovedVideoCompressor()
    assert comp.error_bounds is None and comp.quality_report is False and comp.last_quality is None and comp.max_error == 0
    ok = dict(mask_channels="all", inter_frames=True)
    assert ImprovedVideoCompressor(error_bounds=(1, 2, 2), **ok).error_bounds == (1, 2, 2)
    assert ImprovedVideoCompressor(error_bounds=(1, 2, 2), hold_mode="lookahead", **ok).hold_mode == "lookahead", "look-ahead with error_bounds alone"
    assert ImprovedVideoCompressor(error_bounds=(1, 2, 2), max_error=0, quality_report=True, **ok).quality_report is True
    assert ImprovedVideoCompressor(quality_report=True).quality_report is True, "a quality report needs no bound"
    with pytest.raises(ValueError, match="error_bounds and max_error"):
        ImprovedVideoCompressor(error_bounds=(1, 2, 2), max_error=1, **ok)
    for kw in (dict(mask_channels="luma"), dict(mask_channels="all", gop_batching=False), dict(mask_channels="all", inter_frames=False),
               dict(mask_channels="all", keyframe_interval=1), dict()):
        with pytest.raises(ValueError, match="error_bounds"):
            ImprovedVideoCompressor(error_bounds=(1, 2, 2), **kw)
        if kw:
            with pytest.raises(ValueError, match="max_error"):      # the refusals of max_error > 0, which stay what they were
                ImprovedVideoCompressor(max_error=1, **kw)
    for bad in ("2", 1.5, (1.0, 2.0), True, (-1, 0, 0), 3):
        with pytest.raises(ValueError):
            ImprovedVideoCompressor(error_bounds=bad, **ok)
    with pytest.raises(ValueError, match="lookahead"):
        ImprovedVideoCompressor(hold_mode="lookahead", **ok)


def test_gop_coder_refuses_before_it_touches_the_device():
    E = np.ones((4, 8, 3), dtype=np.uint8)
    sig = inspect.signature(GopCoder.__init__)
    assert sig.parameters["error_bounds"].default is None and sig.parameters["keep_originals"].default is False
    for kw in (dict(mask_channels=1), dict(mask_channels=3, planar_luma=True), dict(mask_channels=3, threshold=1.0), dict(mask_channels=3, max_error=1)):
        with pytest.raises(ValueError):
            GopCoder(None, 8, 4, 3, channels=3, error_bounds=E, **kw)
    for bad in ((1, 1, 1), np.ones((4, 8), dtype=np.uint8), E.astype(np.uint16), np.ones((8, 4, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="bound frame"):
            GopCoder(None, 8, 4, 3, channels=3, mask_channels=3, error_bounds=bad)


def test_verify_max_error_with_a_bound_frame():
    x = random_clip(1, 7, 5, 6, 3, np.uint16)
    E, rect = test_bounds(x.shape[1:], np.uint16, seed=3)
    y = hold_map_ref(x, [3, 6], E)
    v = verify_max_error(list(x), list(y), E, keyframe_interval=3)
    assert v["within_bound"] and v["keyframes_exact"] and v["over_bound"] == 0 and v["max_error"] == 65535 and v["frame_count"] == 7
    assert v["max_abs_error"] == int(np.abs(y.astype(np.int64) - x.astype(np.int64)).max()) > 0
    z = y.copy()
    r, c = rect[0].start, rect[1].start
    z[4, r, c, 1] ^= 1                                        # one level off inside the exact rectangle: far inside the clip's largest bound
    v = verify_max_error(list(x), list(z), E, keyframe_interval=3)
    assert not v["within_bound"] and v["over_bound"] == 1 and v["keyframes_exact"]
    per_channel = (0, 3, 3)
    y = hold_map_ref(x, [3, 6], container.bounds_frame(per_channel, x.shape[1:], x.dtype))
    assert verify_max_error(list(x), list(y), per_channel)["within_bound"]
    assert np.array_equal(y[..., 0], x[..., 0]), "channel 0 has bound 0"
    assert not verify_max_error(list(x), list(hold_ref(x, [3, 6], 3)), per_channel)["within_bound"]
    v = verify_max_error(list(x), list(y[:-1]), per_channel)
    assert not v["within_bound"] and "mismatch" in v["reason"]
    with pytest.raises(ValueError):
        verify_max_error(list(x), list(y), "3")
    assert verify_max_error(list(x), list(x), 0)["within_bound"], "the scalar path is what it was"


def test_error_stats_ref_against_hand_computed_rows():
    a = np.zeros((2, 2, 3, 2), dtype=np.uint16)
    b = a.copy()
    b[0, 0, 0, 0], b[0, 1, 2, 1], a[0, 0, 1, 0] = 3, 65535, 0x8000           # differences 3, 65535 and 32768 (no int16 wrap)
    rows = error_stats_ref(a, b, 3)
    assert rows.dtype == ROW == nat.ERROR_ROW
    assert rows[0].tolist() == (9 + 65535 ** 2 + 32768 ** 2, 3, 2, 65535, 0) and rows[1].tolist() == (0, 0, 0, 0, 0)
    E = np.zeros((2, 3, 2), dtype=np.uint16)
    E[1, 2, 1], E[0, 1, 0] = 65535, 32767
    assert error_stats_ref(a, b, E)[0].tolist() == (9 + 65535 ** 2 + 32768 ** 2, 3, 2, 65535, 0)     # 3 > 0 and 32768 > 32767
    E[0, 1, 0] = 32768
    assert error_stats_ref(a, b, E)[0]["over_bound"] == 1
    q = quality_rows(rows, 12, 16)
    assert q[1] == {"max_abs_error": 0, "mse": 0.0, "psnr": float("inf"), "changed_samples": 0, "over_bound": 0}
    mse = (9 + 65535 ** 2 + 32768 ** 2) / 12
    assert q[0]["mse"] == mse and abs(q[0]["psnr"] - 10 * np.log10(65535 ** 2 / mse)) < 1e-12 and q[0]["changed_samples"] == 3
    u8 = error_stats_ref(np.zeros((1, 150, 150, 3), np.uint8), np.full((1, 150, 150, 3), 255, np.uint8))
    assert int(u8[0]["sse"]) == 150 * 150 * 3 * 255 ** 2 > 2 ** 32


def test_header_binding_and_library_carry_the_entries():
    hdr = open(os.path.join(REPO, "include", "rbf.h"), encoding="utf-8").read()
    so = os.path.join(REPO, "new_bloom_filter_repo_amd", "librbf_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("rbf_temporal_hold_runs_map", "rbf_temporal_lookahead_runs_map", "rbf_error_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in nat.exported_symbols() and re.search(r"\bT %s\b" % name, syms), name
    assert nat._PROTOS["rbf_temporal_hold_runs_map"] == nat._PROTOS["rbf_temporal_lookahead_runs_map"] == \
        (nat._int, [nat._vp, nat._vp, nat._u64, nat._u32, nat._u32, nat._u32, nat._u32, nat._u32, nat._vp, nat._vp])
    assert re.search(r"typedef struct \{ uint64_t sse, differing, over_bound; uint32_t max_abs, reserved; \} rbf_error_row;", hdr)
    assert nat.ERROR_ROW.itemsize == 32
    assert int(re.search(r"#define\s+RBF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4, "additive: the ABI version stays"


def test_new_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900, check=True).stdout
    rows = [ln.split() for ln in out.splitlines() if ln.startswith(("k_hold_map", "k_lookahead_map", "k_error_"))]
    names = {" ".join(r[:-6]) for r in rows}
    types = [(s, c) for s in ("char", "short") for c in (1, 2, 3, 4)]
    want = {"%s<unsigned %s, %d>" % (k, s, c) for k in ("k_hold_map", "k_lookahead_map") for s, c in types}
    want |= {"k_error_stats<unsigned %s, %d, %s>" % (s, c, m) for s, c in types for m in ("true", "false")}
    want |= {"%s<unsigned %s>" % (k, s) for k in ("k_hold_map_px", "k_lookahead_map_px", "k_error_stats_px") for s in ("char", "short")}
    want |= {"k_error_reduce"}
    assert names == want, names ^ want
    for r in rows:
        assert r[-4] == "0" and r[-3] == "0", r             # scratch bytes, VGPR spills
