"""CPU: what the frame-preparation sweep (tests/test_gpu_frame_prep_sweep.py) rests on -- the layout builder of tests/frame_prep_ref.py, the
proof that every one of the sweep's inputs would show a wrong kernel (a misread layout, another border rule, a signed compare, a frame
mixed with its neighbour), ADAPTIVE_GUARD at the sizes the product runs, and the adaptive clips with their exact undecided frames."""
import math

import numpy as np
import pytest

import frame_prep_ref as fp
from new_bloom_filter_repo_amd import engine as E


# ------------------------------------------------------------------ the layout builder
@pytest.mark.parametrize("dtype,C,name", fp.A_CASES, ids=fp.A_IDS)
def test_layout_round_trip(dtype, C, name):
    clip = fp.a_clip(dtype, C)
    lay = fp.make_layout(name, clip.shape, dtype)
    sb = np.dtype(dtype).itemsize
    buf = lay.place(clip)
    assert buf.dtype == np.uint8 and len(buf) == lay.nbytes
    assert np.array_equal(lay.read(buf), clip)
    # the layouts are what the sweep says they are, in bytes
    dense = fp.A_W * C * sb
    assert lay.pixel_stride == C * sb
    assert lay.row_pitch == dense + (C * sb + sb if name in ("pitch", "all") else 0)
    assert lay.frame_stride == fp.A_H * lay.row_pitch + (3 * sb if name in ("stride", "all") else 0)
    assert lay.base == (sb if name in ("base", "all") else 0)
    assert lay.row_pitch % sb == 0 and lay.frame_stride % sb == 0
    assert len(lay.misreadings()) == {"dense": 0, "pitch": 1, "stride": 1, "base": 1, "all": 3}[name]
    # the clip's bytes and nothing else depend on the clip
    other = lay.place(fp.random_clip(1, *clip.shape, dtype))
    own = np.zeros(lay.nbytes, bool)
    for b in range(sb):
        own[lay.offsets() + b] = True
    assert own.sum() == clip.nbytes and np.array_equal(buf[~own], other[~own])


@pytest.mark.parametrize("dtype,C,name", [c for c in fp.A_CASES if c[2] != "dense"], ids=[i for i in fp.A_IDS if not i.endswith("dense")])
def test_every_layout_is_non_vacuous(dtype, C, name):
    """A reader that takes the dense pitch, the dense frame stride or base 0 instead of the layout's finds another luma, another gray and
    other moments -- in the call as a whole and in its last frame, which every misreading moves."""
    clip = fp.a_clip(dtype, C)
    lay = fp.make_layout(name, clip.shape, dtype)
    buf = lay.place(clip)
    luma, (_, moments) = fp.luma_ref(clip), fp.noise_ref(clip)
    gray = fp.gray_ref(clip) if C >= 3 else None
    for what, as_if in lay.misreadings():
        wrong = lay.read(buf, **as_if)
        assert not np.array_equal(fp.luma_ref(wrong)[-1], luma[-1]), what
        wm = fp.noise_ref(wrong)[1]
        assert wm[-1] != moments[-1] and wm[-1][1] != moments[-1][1], what
        if gray is not None:
            assert not np.array_equal(fp.gray_ref(wrong)[-1], gray[-1]), what


# ------------------------------------------------------------------ the border rule
def test_median5_edge_is_the_oracles():
    from oracle import oracle as orc
    p = fp.edge_plane(17, 9, np.uint16)
    assert fp.median5(p) is not None and np.array_equal(fp.median5(p, "edge"), orc.median_blur5(p))
    padded = np.pad(p, 2, mode="edge")
    assert fp.median5(p)[0, 0] == sorted(padded[0:5, 0:5].reshape(-1).tolist())[12]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_every_edge_shape_is_non_vacuous(dtype):
    """Seed fp.EDGE_SEED = 1 (the first one tried that holds for all 90 shapes of W >= 3, H >= 3 at both depths): a reflected border
    and a zero border give other moments than the replicated one.  Shapes with W < 3 or H < 3 cannot be reflected by two pixels; the zero
    border is checked for them too, wherever the plane has a pixel (all of them)."""
    for W in fp.EDGE_WS:
        for H in fp.EDGE_HS:
            p = fp.edge_plane(W, H, dtype)
            want = fp.moments_of(fp.residual(p))
            zero = fp.moments_of(fp.residual(p, "constant"))
            assert zero != want and zero[1] != want[1], (W, H, "zero border")
            if W >= 3 and H >= 3:
                refl = fp.moments_of(fp.residual(p, "reflect"))
                assert refl != want and refl[1] != want[1], (W, H, "reflected border")
                sym = fp.moments_of(fp.residual(p, "symmetric"))
                assert sym != want, (W, H, "symmetric border")


# ------------------------------------------------------------------ orderings
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_ordering_planes_are_non_vacuous(dtype):
    top = fp.top_of(dtype)
    planes = dict(fp.ordering_planes(dtype))
    for name in ("zero_top_0.40_0.60", "zero_top_0.45_0.55", "zero_top_0.50_0.50"):
        for f in range(2):
            ones = fp.windows_ones(planes[name][f, :, :, 0] == top)
            assert (ones == 12).any() and (ones == 13).any(), (name, f)          # both layers of the 0-1 proof, on the device
    for name in [n for n in planes if n.startswith("v_v1")]:
        for f in range(2):
            d = fp.residual(planes[name][f, :, :, 0])
            assert set(np.unique(d).tolist()) == {-1, 0, 1}, (name, f)
    for f in range(2):
        assert fp.moments_of(fp.residual(planes["constant"][f, :, :, 0])) == [0, 0]
    n = fp.A_W * fp.A_H
    # a third of the pixels at +top (the replicated left border turns one column to -top) | a third at -top: s1 is strongly negative
    up, down = (fp.moments_of(fp.residual(planes["columns"][f, :, :, 0])) for f in range(2))
    assert up[0] > 0.3 * n * top and up[1] > 0.3 * n * top * top
    assert down[0] < -0.3 * n * top and down[1] > 0.3 * n * top * top
    full = [fp.moments_of(fp.residual(planes["full_range"][f, :, :, 0])) for f in range(2)]
    assert full[0] != full[1] and min(m[1] for m in full) > n * (top // 8) ** 2
    if np.dtype(dtype).itemsize == 2:
        # the network replayed with signed 16-bit compares.  The middle of 25 values is the same under a REVERSED order, so two levels
        # astride the sign bit only catch a network whose minimum and maximum disagree about the sign; three levels catch any signed one.
        assert len(fp.median_net()) == 140
        for f in range(2):
            p = planes["full_range"][f, :, :, 0]
            assert np.array_equal(fp.median5_network(p), fp.median5(p))
            assert np.array_equal(fp.median5_network(p, True, True), fp.median5_signed16(p))
        for name, wrong in (("sign_bit_pair", [(True, False), (False, True)]), ("sign_bit_three", [(True, True), (True, False), (False, True)])):
            for f in range(2):
                p = planes[name][f, :, :, 0]
                want = fp.moments_of(fp.residual(p))
                for smin, smax in wrong:
                    got = fp.moments_of(fp.residual(p, median=lambda q: fp.median5_network(q, smin, smax)))
                    assert got != want and got[1] != want[1], (name, f, smin, smax)
        spikes = np.zeros((24, 100), np.uint16)                                  # the existing spike plane does NOT tell them apart
        spikes[::6, ::7] = 65535
        assert fp.moments_of(fp.residual(spikes, median=fp.median5_signed16)) == fp.moments_of(fp.residual(spikes))
    assert fp.ORDERING_NAMES[np.dtype(dtype).name] == list(planes)


# ------------------------------------------------------------------ many frames
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_many_frames_are_all_different(dtype):
    """Row f of a 300-frame call cannot be had from frame f - 1 or f + 1, and the second call's rows not from the first call's."""
    for C in (1, 3):
        first, second = fp.many_clips(dtype, C)
        assert first.shape == (300, 3, 5, C) and second.shape == (2, 3, 5, C)
        m1, m2 = fp.noise_ref(first)[1], fp.noise_ref(second)[1]
        assert all(m1[f] != m1[f + 1] and m1[f][1] != m1[f + 1][1] for f in range(299))
        assert all(m2[f] != m1[f] and m2[f][1] != m1[f][1] and m2[f][1] != 0 for f in range(2))
        luma = fp.luma_ref(first)
        assert all(not np.array_equal(luma[f], luma[f + 1]) for f in range(299))
        if C == 3:
            gray = fp.gray_ref(first)
            assert all(not np.array_equal(gray[f], gray[f + 1]) for f in range(299))
        lay = fp.many_layout(first.shape, dtype)
        assert lay.frame_stride == first[0].nbytes + 3 * first.dtype.itemsize
        assert np.array_equal(lay.read(lay.place(first)), first)
        wrong = lay.read(lay.place(first), frame_stride=first[0].nbytes)
        assert all(fp.noise_ref(wrong[f:f + 1])[1][0] != m1[f] for f in (1, 150, 299))


# ------------------------------------------------------------------ gray
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_gray_colours_pin_the_rounding_term(dtype):
    from oracle import oracle as orc
    top = fp.top_of(dtype)
    col = fp.gray_colours(dtype)
    assert len(col) == 16 and col[:7].tolist() == [[0, 0, 0], [top, top, top], [top, 0, 0], [0, top, 0], [0, 0, top], [1, 2, 3], [top - 1, top, top - 2]]
    want, trunc = orc.bgr_to_gray(col), fp.gray_without_rounding(col)
    assert want[:2].tolist() == [0, top]
    under, over = list(range(10, 16, 2)), list(range(11, 16, 2))
    assert np.array_equal(want[under], trunc[under]) and np.array_equal(want[over], trunc[over] + 1)
    assert sum(int(w) != int(t) for w, t in zip(want[7:10], trunc[7:10])) >= 1, "a single-channel maximum rounds up"
    for C in (3, 4):
        clips = fp.gray_clips(dtype, C)
        assert [(name, clip.shape) for name, clip in clips] == [("7x1", (1, 1, 7, C)), ("1x7", (1, 7, 1, C)), ("9x1", (1, 1, 9, C)), ("1x9", (1, 9, 1, C))]
        for name, clip in clips:
            assert np.array_equal(fp.gray_ref(clip).reshape(-1), want[:7] if "7" in name else want[7:]), name
            assert np.array_equal(clip[..., :3].reshape(-1, 3), col[:7] if "7" in name else col[7:])


# ------------------------------------------------------------------ ADAPTIVE_GUARD at the sizes the product runs
def guard_planes(W, H, rng):
    n = W * H
    yield "gauss_0.6", np.rint(rng.normal(0, 0.6, (H, W))).astype(np.int64)
    yield "gauss_3000", np.rint(rng.normal(0, 3000, (H, W))).astype(np.int64)
    yield "spikes_4pct", np.where(rng.random((H, W)) < 0.04, 65535, 0).astype(np.int64)
    yield "columns_top_0_0", np.broadcast_to(np.array([65535, 0, 0], np.int64)[np.arange(W) % 3], (H, W)).copy()
    yield "minus_top_with_0.1pct_top", np.where(rng.random((H, W)) < 0.001, 65535, -65535).astype(np.int64)
    one = np.zeros((H, W), np.int64)
    one[H // 2, W // 3] = 1
    yield "single_1", one
    assert n == one.size


def guard_error(d):
    """|np.std of the float32 plane - the exact standard deviation| / exact, plus 2^-22 for the float32 roundings of the level and of
    level * tolerance, which the band's float64 rule does not make."""
    n, s1, s2 = d.size, int(d.sum()), int((d * d).sum())
    exact = math.sqrt(n * s2 - s1 * s1) / n
    assert exact > 0
    return abs(float(np.std(d.astype(np.float32))) - exact) / exact + 2.0 ** -22


def test_guard_covers_float32_std_at_1080p_and_2160p():
    """The residual planes numpy's float32 np.std is worst at -- large n, large mean against a small spread, huge values -- at 1920x1080
    and 3840x2160.  Measured (numpy's pairwise float32 sum, generator seed 2160): between 2.8e-7 and 1.58e-6 over the twelve
    planes, the 2^-22 included; the maximum, 1.58e-6, is the 2160p plane at -65535 with 0.1 % at +65535 (1.41e-6 for the 2160p columns) --
    63 times inside ADAPTIVE_GUARD = 1e-4."""
    rng = np.random.default_rng(2160)
    worst = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        for name, d in guard_planes(W, H, rng):
            worst[(W, H, name)] = guard_error(d)
    print("guard errors:", {k: "%.3g" % v for k, v in worst.items()}, "max %.3g" % max(worst.values()))
    assert len(worst) == 12
    for key, err in worst.items():
        assert err < E.ADAPTIVE_GUARD, (key, err)


# ------------------------------------------------------------------ the adaptive clips
@pytest.mark.parametrize("W,H,dtype", fp.ADAPTIVE_CASES, ids=fp.ADAPTIVE_IDS)
def test_band_brackets_the_oracle_and_leaves_one_frame_undecided(W, H, dtype):
    clip, want, bands, undecided = fp.adaptive_case(W, H, dtype)
    assert clip.shape == (5, H, W, 3) and clip.dtype == dtype and len(want) == len(bands) == 4
    for w, (lo, hi) in zip(want, bands):
        assert lo <= w <= hi and hi - lo <= 1
    assert undecided == [2], undecided                              # frames count from 0; frame 2 is the searched one
    decided = {w for w, (lo, hi) in zip(want, bands) if lo == hi}
    assert len(decided) >= 2 and all(3 < w < 30 for w in want), want   # the clamp hides nothing
    # the search that found the clip still finds it
    if (W, H) == (131, 19):
        assert fp.search_adaptive_frames(W, H, dtype) == fp.ADAPTIVE_CLIPS[(W, H, np.dtype(dtype).name)]
