"""The near-lossless mode without a GPU: the numpy reference of the temporal hold has the properties the mode rests on (bound, closed loop,
idempotence, no int16 wrap), every Python layer refuses what the mode cannot do before it reaches the library, the block predicate of
container.py, make_camera_gop's sensor_noise keyword, verify_max_error, and the library side: the entry is declared, bound and exported and
no k_temporal_hold instantiation uses scratch memory."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from near_lossless_ref import all_channel_masks, hold_ref, random_clip
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.synthetic import make_camera_gop
from new_bloom_filter_repo_amd.verify import verify_max_error


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("C", [0, 1, 3, 4])
def test_reference_properties(dtype, C):
    x = random_clip(7 + C, 9, 6, 11, C, dtype)
    starts = [4, 5]
    assert np.array_equal(hold_ref(x, starts, 0), x), "max_error 0 is the identity"
    for delta in (1, 3, int(np.iinfo(dtype).max)):
        y = hold_ref(x, starts, delta)
        assert y.dtype == x.dtype and y.shape == x.shape
        assert int(np.abs(y.astype(np.int64) - x.astype(np.int64)).max()) <= delta, "the bound holds on every sample"
        for t in (0, 4, 5):
            assert np.array_equal(y[t], x[t]), "run starts are untouched"
        assert np.array_equal(hold_ref(y, starts, delta), y), "idempotent"
        if delta == np.iinfo(dtype).max:                    # nothing can exceed it: every run collapses to its first frame
            assert all(np.array_equal(y[t], y[0]) for t in range(4)) and all(np.array_equal(y[t], y[5]) for t in range(5, 9))
        if C >= 3:                                          # a pixel is updated whole: it equals the frame's or the held one
            same_as_x = (y[1:] == x[1:]).all(-1)
            same_as_prev = (y[1:] == y[:-1]).all(-1)
            assert (same_as_x | same_as_prev).all()
    assert not np.shares_memory(hold_ref(x, starts, 1), x)


def test_reference_closes_the_loop_on_a_ramp():
    F = 10
    x = (np.arange(F, dtype=np.uint8)[:, None, None, None] + np.full((1, 2, 3, 3), 40, dtype=np.uint8)).astype(np.uint8)
    y = hold_ref(x, [], 2)
    updated = [t for t in range(1, F) if not np.array_equal(y[t], y[t - 1])]
    assert updated == [3, 6, 9]
    assert all(np.array_equal(y[t], x[t]) for t in updated) and np.array_equal(y[5], x[3])
    # an open-loop comparison against x_{t-1} (the thresholded luma diff) never updates: |x_t - x_{t-1}| = 1 <= 2
    assert not (np.abs(x[1:].astype(int) - x[:-1].astype(int)) > 2).any()


def test_reference_has_no_int16_wrap():
    x = np.zeros((3, 1, 2, 3), dtype=np.uint16)
    x[1, 0, 0, 1] = 0x8000                                  # int16 arithmetic calls this difference 0 (abs(-32768) stays negative)
    x[2, 0, 0, 1] = 0x8000
    x[2, 0, 1, 2] = 65535
    y = hold_ref(x, [], 32767)
    assert np.array_equal(y, x), "0x8000 and 65535 are updates"
    y = hold_ref(x, [], 32768)
    assert y[1, 0, 0, 1] == 0 and y[2, 0, 0, 1] == 0 and y[2, 0, 1, 2] == 65535
    assert not hold_ref(x, [], 65535)[1:].any()


def test_all_channel_masks_helper():
    x = random_clip(3, 5, 4, 5, 3, np.uint8)
    m = all_channel_masks(x, [2])
    assert m.shape == (4, 20) and not m[1].any()
    assert np.array_equal(m[0], (x[0] != x[1]).any(-1).reshape(-1))


# ------------------------------------------------------------------ validation (no library needed)
class _NoCtx:
    """A context that must never be used: the argument checks come first."""
    handle = None

    def alloc(self, nbytes):
        raise AssertionError("allocated before the argument check")


def test_gop_coder_refuses_what_the_hold_cannot_do():
    from new_bloom_filter_repo_amd.gop import GopCoder
    bad = (dict(mask_channels=1), dict(mask_channels=2), dict(mask_channels=3, planar_luma=True), dict(mask_channels=3, threshold=1.0),
           dict(mask_channels=3, threshold=None, adaptive=(10.0, 3.0, 30.0)), dict(mask_channels=3, max_error=256))
    for kw in bad:
        kw = dict(dict(max_error=2), **kw)
        with pytest.raises(ValueError):
            GopCoder(_NoCtx(), 64, 32, 4, **kw)
    for kw in (dict(channels=1, planar_luma=True), dict(channels=1, threshold=2.0)):
        with pytest.raises(ValueError):
            GopCoder(_NoCtx(), 64, 32, 4, max_error=2, **kw)
    for me in (-1, 1.5, "2", None, True):
        with pytest.raises(ValueError):
            GopCoder(_NoCtx(), 64, 32, 4, mask_channels=3, max_error=me)
    with pytest.raises(AssertionError):                      # a good combination gets as far as the allocator
        GopCoder(_NoCtx(), 64, 32, 4, mask_channels=3, max_error=2)
    with pytest.raises(AssertionError):
        GopCoder(_NoCtx(), 64, 32, 4, channels=1, max_error=2)
    with pytest.raises(AssertionError):
        GopCoder(_NoCtx(), 64, 32, 4, channels=3, sample_bytes=2, mask_channels=3, max_error=65535)


def test_surface_refuses_what_the_mode_cannot_do():
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    assert ImprovedVideoCompressor().max_error == 0
    assert ImprovedVideoCompressor(mask_channels="all", max_error=2).max_error == 2
    assert ImprovedVideoCompressor(mask_channels="all", max_error=np.int64(3)).max_error == 3
    for kw in (dict(), dict(mask_channels="luma"), dict(mask_channels="all", inter_frames=False), dict(mask_channels="all", gop_batching=False),
               dict(mask_channels="all", keyframe_interval=1)):
        with pytest.raises(ValueError):
            ImprovedVideoCompressor(max_error=2, **kw)
    for me in (-1, 0.5, "1", None, True):
        with pytest.raises(ValueError):
            ImprovedVideoCompressor(mask_channels="all", max_error=me)


def test_encode_range_refuses_blocks_that_start_inside_a_run():
    """plan_range's blocks overlap by the frame they read but do not code: block b+1 starts at frame lo + block_frames - 1.  With
    keyframe_interval 6 that is a keyframe again for block_frames 7 (6 + 1: frames 0..6, 6..12, ...) and for 12 and 13, and is not for
    8, 5 or 9: those raise, before anything touches the GPU (no library is loaded here)."""
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    frames = [np.zeros((4, 4, 3), dtype=np.uint8) for _ in range(25)]
    for bf, raises in ((8, True), (5, True), (9, True), (7, False), (12, False), (13, False)):
        _, blocks = container.plan_range(0, 0, len(frames), 6, bf, True)
        assert bool(container.blocks_off_keyframes(blocks, 0, 6)) == raises, bf
        if raises:
            comp = ImprovedVideoCompressor(keyframe_interval=6, block_frames=bf, mask_channels="all", max_error=1)
            with pytest.raises(ValueError) as e:
                comp.encode_range(frames, 0, 0, len(frames))
            assert "block_frames" in str(e.value) and "keyframe_interval" in str(e.value) and "keyframe" in str(e.value)
            assert comp._lanes == [], "raised before a context was made"
    # a range that starts inside a run (a shard that cuts a GOP): its halo frame is a keyframe by the rule, the second block's first is not
    comp = ImprovedVideoCompressor(keyframe_interval=6, block_frames=12, mask_channels="all", max_error=1)
    with pytest.raises(ValueError):
        comp.encode_range(frames[3:], 3, 4, len(frames))
    assert container.plan_range(0, 0, 25, 6, 8, False)[1] == []      # without inter-frames there are no blocks: nothing to hold or to refuse


# ------------------------------------------------------------------ the container predicate
def test_blocks_off_keyframes_hand_written():
    # first_index 0, keyframe_interval 30, 100 frames
    for bf, want_blocks, off in ((30, [(0, 30), (30, 60), (60, 90), (90, 100)], []),           # (frames 30, 60, 90 are keyframes: no block codes them)
                                 (60, [(0, 60), (60, 100)], []),
                                 (45, [(0, 45), (44, 89), (88, 100)], [44, 88])):
        _, blocks = container.plan_range(0, 0, 100, 30, bf, True)
        assert [(lo, end) for lo, end, _ in blocks] == want_blocks, bf
        assert [b[0] for b in container.blocks_off_keyframes(blocks, 0, 30)] == off, bf
    # first_index 37: frame 37 has no predecessor among the frames handed in, so it is a keyframe of this call; 60 and 90 are by the rule
    for bf, off in ((30, [66, 95]), (60, [96]), (45, [81])):
        _, blocks = container.plan_range(37, 37, 100, 30, bf, True)
        assert blocks[0][0] == 37
        assert [b[0] for b in container.blocks_off_keyframes(blocks, 37, 30)] == off, bf
    _, blocks = container.plan_range(37, 37, 60, 30, 30, True)                                  # ... and a range that ends before the second block
    assert container.blocks_off_keyframes(blocks, 37, 30) == []
    assert container.blocks_off_keyframes([], 0, 30) == []
    assert container.blocks_off_keyframes([(30, 60, []), (31, 60, [])], 0, 30) == [(31, 60, [])]
    # the default block of the surface satisfies it for every interval up to 128
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    for I in (2, 3, 6, 30, 64, 65, 100, 128):
        comp = ImprovedVideoCompressor(keyframe_interval=I, mask_channels="all", max_error=1)
        _, blocks = container.plan_range(0, 0, 5 * I + 3, I, comp.block_frames, True)
        assert blocks and container.blocks_off_keyframes(blocks, 0, I) == [], I


# ------------------------------------------------------------------ synthetic input
# sha256 of the frames' bytes as make_camera_gop(seed, 96, 64, 4, dtype=...) returned them before the sensor_noise keyword existed
CAMERA_GOP_DIGESTS = {
    (5, "uint8"): "bfd4ce39da4b3522b3ccf288b76f2cb087f43df5a4f82f03fceb988c285d1155",
    (5, "uint16"): "c06dea8adfe00c4387a1509fd7576cd8765f5e8122a3294df9abf94b10acf7b7",
    (2024, "uint8"): "29723e6790b1e3a8159506fe292e1472f29a4967582255da8e323dacceec1bd8",
    (2024, "uint16"): "4aaea25635a8a6dd115a6778fae7ccf5b1a7454a3e46e9a84ee97b67ddc6d714",
}


@pytest.mark.parametrize("seed", [5, 2024])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_sensor_noise_zero_is_todays_clip(seed, dtype):
    frames = make_camera_gop(seed, 96, 64, 4, dtype=dtype)
    digest = hashlib.sha256(b"".join(f.tobytes() for f in frames)).hexdigest()
    assert digest == CAMERA_GOP_DIGESTS[(seed, np.dtype(dtype).name)]
    again = make_camera_gop(seed, 96, 64, 4, dtype=dtype, sensor_noise=0)
    assert all(np.array_equal(a, b) for a, b in zip(frames, again))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_sensor_noise_clip(dtype):
    T, a, delta = 13, 1, 2
    frames = np.stack(make_camera_gop(9, 96, 64, T, dtype=dtype, sensor_noise=a))
    assert frames.shape == (T, 64, 96, 3) and frames.dtype == dtype
    again = np.stack(make_camera_gop(9, 96, 64, T, dtype=dtype, sensor_noise=a))
    assert np.array_equal(frames, again)
    exact = all_channel_masks(frames, [])
    assert exact.mean() > 0.9, "with sensor noise the exact all-channel mask is almost all ones"
    starts = [6, 12]
    y = hold_ref(frames, starts, delta)
    assert int(np.abs(y.astype(np.int64) - frames.astype(np.int64)).max()) <= delta
    held = all_channel_masks(y, starts)
    coded = [f for f in range(T - 1) if f + 1 not in starts]
    assert 0 < held[coded].mean() < 0.03, "the hold leaves the moving pixels (and swallows every static one: |x_t - y| <= 2a <= max_error)"
    assert all(held[f].any() for f in coded)
    # the moving set jumps by more than 2a + max_error in some sample: nearly all of it gets through the hold
    moved = float(held[coded].mean())
    assert moved > 0.005, moved                             # (Bernoulli(0.01) per pair)


# ------------------------------------------------------------------ verify_max_error
def test_verify_max_error():
    x = random_clip(1, 7, 5, 6, 3, np.uint16)
    v = verify_max_error(list(x), list(x.copy()), 0, keyframe_interval=3)
    assert v == {"frame_count": 7, "max_error": 0, "max_abs_error": 0, "worst_frame": -1, "within_bound": True, "keyframes_exact": True}
    y = hold_ref(x, [3, 6], 3)
    v = verify_max_error(list(x), list(y), 3, keyframe_interval=3)
    assert v["within_bound"] and v["keyframes_exact"] and 0 < v["max_abs_error"] <= 3 and v["worst_frame"] not in (-1, 0, 3, 6)
    assert "keyframes_exact" not in verify_max_error(list(x), list(y), 3)
    z = y.copy()
    z[4, 2, 2, 1] = (int(x[4, 2, 2, 1]) + 40000) % 65536          # 40000 or 25536 away: int16 arithmetic would get the first wrong
    v = verify_max_error(list(x), list(z), 3, keyframe_interval=3)
    assert not v["within_bound"] and v["worst_frame"] == 4 and v["max_abs_error"] in (40000, 25536) and v["keyframes_exact"]
    z = y.copy()
    z[3, 0, 0, 0] ^= 1
    v = verify_max_error(list(x), list(z), 3, keyframe_interval=3)
    assert v["within_bound"] and not v["keyframes_exact"]
    v = verify_max_error(list(x), list(y[:-1]), 3)
    assert not v["within_bound"] and v["frame_count"] == 7 and "mismatch" in v["reason"]


# ------------------------------------------------------------------ the library
def test_entry_in_header_bindings_and_library():
    name = "rbf_temporal_hold_runs"
    hdr = open(os.path.join(REPO, "include", "rbf.h"), encoding="utf-8").read()
    so = os.path.join(REPO, "new_bloom_filter_repo_amd", "librbf_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in nat.exported_symbols()
    assert re.search(r"\bT %s\b" % name, syms)
    assert nat._PROTOS[name] == (nat._int, [nat._vp, nat._vp, nat._u64, nat._u32, nat._u32, nat._u32, nat._u32, nat._u32, nat._u32, nat._vp])
    assert int(re.search(r"#define\s+RBF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4, "additive: the ABI version stays"
    assert int(re.search(r"#define\s+RBF_K_COUNT\s+(\d+)", hdr).group(1)) == len(nat.KERNEL_NAMES) == nat.K_HOLD + 1
    assert nat.KERNEL_NAMES[int(re.search(r"#define\s+RBF_K_HOLD\s+(\d+)", hdr).group(1))] == "hold"


def test_hold_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900, check=True).stdout
    rows = [ln.split() for ln in out.splitlines() if ln.startswith("k_temporal_hold")]
    names = {" ".join(r[:-6]) for r in rows}
    want = {"k_temporal_hold<unsigned %s, %d>" % (s, c) for s in ("char", "short") for c in (1, 2, 3, 4)}
    want |= {"k_temporal_hold_px<unsigned char>", "k_temporal_hold_px<unsigned short>"}
    assert names == want, names ^ want
    for r in rows:
        assert r[-4] == "0" and r[-3] == "0", r             # scratch bytes, VGPR spills
