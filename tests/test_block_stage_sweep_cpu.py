"""The conditions of tests/test_gpu_block_stage_sweep_bounds_pan.py on the CPU, on the references alone: the lane clips are not vacuous
under their bound frames, the bounds matter where a kernel could mis-address them, the quality report has something to count in the third
workgroup and in the tail, the planted maxima are strict, every far decoy changes the reference result, and every candidate of a planted
pan clip is the one zero of its pair's table -- so a seed or a shape that makes a GPU test vacuous fails here and never reaches the device.
pan_ref.sad_tables, the vectorised SAD table those clips need, is proven equal to pan_ref.sad_table."""
import numpy as np
import pytest

import block_layout as bl
import pan_ref
from error_bounds_ref import error_stats_ref


@pytest.mark.parametrize("rule", bl.MAP_RULES)
@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_lane_clips_under_their_bound_frames(dtype, C, rule):
    """Not vacuous, and the bounds matter: the reference under the aliased bound frame differs inside the third workgroup and the tail."""
    x, E = bl.lane_clip(dtype, C), bl.lane_bounds(dtype, C)
    assert E.shape == x.shape[1:] and E.dtype == x.dtype
    want = bl.map_ref(rule, x, bl.LANE_STARTS, E)
    assert bl.lane_non_vacuous(x, want, bl.rule_lane_pixels(rule))
    shape = bl.LaneShape(bl.LANE_N, bl.rule_lane_pixels(rule))
    (lo, hi), (t0, t1) = shape.workgroup(2), shape.tail()
    alias = bl.aliased_bounds(E, shape.lane_pixels).reshape(bl.LANE_N, C)
    flat = E.reshape(bl.LANE_N, C)
    assert np.array_equal(alias[lo:hi], flat[:hi - lo]) and np.array_equal(alias[t0:t1], flat[:5])
    keep = np.ones(bl.LANE_N, dtype=bool)
    keep[lo:hi] = keep[t0:t1] = False
    assert np.array_equal(alias[keep], flat[keep]), "only the third workgroup and the tail are aliased"
    in_wg, in_tail = bl.bounds_matter(x, want, rule, E)
    print("%s %s c%d: the aliased reference differs in %d pixel-frames of workgroup 2, %d of the tail" % (rule, np.dtype(dtype).name, C, in_wg, in_tail))
    assert in_wg > 0 and in_tail > 0


@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_quality_report_of_the_lane_clips(dtype, C):
    """Nothing is over the frame the block was held under, something over half of it and over 0 -- in the third workgroup and in the tail, on
    their own -- and each planted maximum is the one largest difference of its frame."""
    a, E = bl.lane_clip(dtype, C), bl.lane_bounds(dtype, C)
    b = bl.map_ref("hold", a, bl.LANE_STARTS, E)
    wg, tail = bl.stats_regions()
    assert (wg, tail) == ((8192, 8784), (8784, 8789))
    for name, bounds in bl.stats_bounds(E):
        rows = error_stats_ref(a, b, bounds)
        assert (not rows["over_bound"].any()) if name == "frame" else (rows["over_bound"].sum() > 0), name
        for lo, hi in (wg, tail):
            sse, differing, over = bl.region_stats(a, b, bounds, lo, hi)
            print("%s c%d, bounds %s, pixels [%d, %d): sse %d, differing %d, over %d" % (np.dtype(dtype).name, C, name, lo, hi, sse, differing, over))
            assert sse > 0 and differing > 0 and (over > 0 or name == "frame"), (name, lo, hi)
    a2, b2, places = bl.plant_maxima(a, b)
    assert [(f, p) for f, p, _ in places] == [(2, 8786), (4, 8783), (5, 4095)]
    assert bl.maxima_are_strict(a2, b2, places)
    assert not bl.maxima_are_strict(a, b, places), "the maxima are the planted samples, not the clip's"
    top = int(np.iinfo(dtype).max)
    rows = error_stats_ref(a2, b2, E)
    assert [int(rows["max_abs"][f]) for f, _, _ in places] == [top] * 3 and int(rows["max_abs"][3]) == 0, "frame 3 starts a run"


@pytest.mark.parametrize("rule", bl.MAP_RULES)
@pytest.mark.parametrize("dtype,C", bl.FAR_MAP_CASES, ids=bl.FAR_MAP_IDS)
def test_far_map_decoys_change_the_held_block(dtype, C, rule):
    assert bl.far_map_decoys_matter(rule, *bl.far_map_case(rule, dtype, C))


@pytest.mark.parametrize("dtype,C", bl.FAR_MAP_CASES, ids=bl.FAR_MAP_IDS)
def test_far_stats_decoys_change_the_report(dtype, C):
    a, b, E, a_decoys, b_decoys = bl.far_stats_case(dtype, C)
    assert not error_stats_ref(a, b, E)["over_bound"].any() and error_stats_ref(a, b, E)["differing"][1:].all()
    for bounds in bl.FAR_STATS_BOUNDS:
        assert bl.far_stats_decoys_matter(a, b, E if bounds == "frame" else bounds, a_decoys, b_decoys), bounds


def test_far_pan_decoys_change_the_rows():
    x, decoys, rows = bl.far_pan_case()
    W, H, R = bl.FAR_PAN
    assert x.shape == (3, H, W, 3) and x.dtype == np.uint8
    xs, ys = pan_ref.grid_points(W, H, R)
    assert -(-len(xs) // 16) == 3 and -(-len(ys) // 8) == 3, "3 x 3 tiles of 16 x 8 grid points"
    assert all(r["moving_zero"] > 0 for r in rows) and any((r["dx"], r["dy"]) != (0, 0) for r in rows)
    assert bl.far_pan_decoys_matter(x, decoys, rows)


@pytest.mark.parametrize("W,H,pb", bl.FAR_ROLLS, ids=bl.FAR_ROLL_IDS)
def test_far_roll_decoys_change_the_frames(W, H, pb):
    assert ((W * pb) % 16 == 0) == (pb == 4), "64 pixels of 4 bytes: rows of whole vectors; 67 pixels of 3 bytes: the byte path"
    assert bl.far_roll_decoys_matter(*bl.far_roll_case(W, H, pb))


# ------------------------------------------------------------------ pan search: the vectorised table, and the planted candidates
@pytest.mark.parametrize("W,H,R,C,dtype", [(19, 11, 1, 0, np.uint8), (25, 17, 4, 2, np.uint8), (41, 30, 3, 3, np.uint16), (67, 33, 4, 1, np.uint16),
                                           (12, 11, 2, 4, np.uint8)])
def test_vectorised_sad_tables_equal_the_reference(W, H, R, C, dtype):
    rng = np.random.default_rng(W + R)
    frames = rng.integers(0, int(np.iinfo(dtype).max) + 1, (4, H, W) + ((C,) if C else ()), dtype=dtype)
    tables = pan_ref.sad_tables(frames, R)
    assert tables.shape == (3, 2 * R + 1, 2 * R + 1) and tables.dtype == np.int64
    for p in range(3):
        want = pan_ref.sad_table(frames[p], frames[p + 1], R)
        assert {(dx, dy): int(tables[p, dy + R, dx + R]) for dx, dy in want} == want


def test_planted_ranges_are_where_the_lane_mapping_changes():
    """Every range at which a lane's chunk of candidates changes, and the first range of the second and third instantiation."""
    changes = [R for R in range(1, 33) if R == 1 or bl.pan_chunk(R) != bl.pan_chunk(R - 1)]
    assert changes == [1, 8, 11, 14, 16, 18, 21, 23, 25, 26, 28, 30, 32]
    assert bl.PLANTED_RANGES == sorted(changes + [9, 17])
    assert [bl.pan_chunk(R) for R in (8, 16, 32)] == [2, 5, 22], "the register bounds CH of the three instantiations"
    assert all(bl.pan_chunk(R) <= bl.pan_chunk(RM) for RM, lo in ((8, 1), (16, 9), (32, 17)) for R in range(lo, RM + 1))


@pytest.mark.parametrize("R,dtype", [(R, np.uint8) for R in bl.PLANTED_RANGES] + [(17, np.uint16)], ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
def test_planted_candidates_are_the_one_zero_of_their_table(R, dtype):
    frames, shifts, tables = bl.planted_candidates(R, dtype)
    nd = 2 * R + 1
    assert frames.shape == (nd * nd + 1, 2 * R + 9, 2 * R + 17, 2) and tables.shape == (nd * nd, nd, nd)
    xs, ys = pan_ref.grid_points(2 * R + 17, 2 * R + 9, R)
    assert (len(xs), len(ys)) == (3, 2), "3 x 2 grid points: one tile"
    assert shifts[0] == (-R, -R) and shifts[1] == (-R + 1, -R) and shifts[-1] == (R, R) and len(set(shifts)) == nd * nd
    assert bl.planted_zero_is_unique(shifts, tables, R)
    if R <= 9:
        rows = bl.planted_rows(frames, shifts, tables, R)
        assert all(r["moving_best"] == 0 for r in rows), "the clip is rolled: with its shift nothing moves"
        assert all((r["moving_zero"] == 0) == ((r["dx"], r["dy"]) == (0, 0)) for r in rows)
        want = pan_ref.stat_rows(frames[:8], R, 0)
        assert rows[:7] == want, "the rows of the first pairs are pan_ref.stat_rows'"
