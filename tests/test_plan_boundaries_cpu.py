"""The boundary table of tests/plan_boundaries.py against the planner itself (csrc/rbf_plan.h through tests/c/plan_cases.cpp, a plain
host build: no GPU).  Every row is a transition of the planner's decision and nothing changes within 128 bits on either side of it; a
sweep of m = 2 .. 2^24 in steps of 128 bits, with every m between two samples that differ, finds exactly the table's rows -- so a row
moved by 128 bits fails, and so does a planner constant (LDS_LIMIT, MAX_INSERT_TILES, F64MOD_M_*, an LDS layout size) changed without
the table; and on both sides of every row the dynamic LDS the host launches with stays within LDS_LIMIT.  The table is what
tests/test_gpu_plan_boundaries.py runs on the device: this test passes before anything of it goes to a GPU."""
import pytest

import plan_boundaries as B


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if B.GXX is None:
        pytest.skip("g++ not found: tests/c/plan_cases.cpp is built with a plain host compiler, not with hipcc")
    return B.build_plan_cases(tmp_path_factory.mktemp("plan_boundaries"))


def test_table_is_well_formed():
    assert len(set(B.ROWS)) == len(B.ROWS)
    for r in B.ROWS:
        assert r.knobs in B.KNOBS and r.first == r.last + 1 and 128 < r.last and r.first + 128 <= B.SWEEP_END and 1 <= r.frames <= 128, r
        assert r.coded in (1, r.frames) and (r.frames, r.coded) == ((2, 1) if r.known else (r.frames, r.frames)), r


@pytest.mark.parametrize("row", B.ROWS, ids=B.row_id)
def test_row_is_a_transition(exe, row):
    """The decision differs between the row's two m, and is the same from 128 bits below to `last` and from `first` to 128 bits above."""
    below, last, first, above = B.plans(exe, [(row, m) for m in (row.last - 128, row.last, row.first, row.first + 128)])
    assert last["decision"] != first["decision"], (row, last["decision"])
    assert below["decision"] == last["decision"], (row, below["decision"], last["decision"])
    assert first["decision"] == above["decision"], (row, first["decision"], above["decision"])


@pytest.mark.parametrize("row", B.ROWS, ids=B.row_id)
def test_launch_lds_within_the_limit(exe, row):
    """On both sides of a row: the bytes of dynamic LDS the host launches the query kernel with (k_query_u64: two image buffers and the
    frame records; k_query_s64t: s64t_lds_bytes of its tile; the Barrett kernels: their buffers) and the LDS insert kernels with."""
    for m, p in zip((row.last, row.first), B.plans(exe, [(row, m) for m in (row.last, row.first)])):
        limit = int(p["lds_limit"])
        assert int(p["launch_query_lds"]) <= limit, (row, m, p["launch_query_lds"])
        if p["fast_insert"] == "1":
            assert int(p["insert_lds"]) <= limit, (row, m, p["insert_lds"])
        if p["query"] in ("1", "2", "3"):                         # an LDS query kernel holds a tile of the filter
            assert int(p["launch_query_lds"]) > 0
            tile_words = int(p["query_tile_words"]) if p["query"] != "1" else (int(p["fwords_max"]) + 3) // 4 * 4
            assert int(p["launch_query_lds"]) >= min(tile_words, (int(p["fwords_max"]) + 3) // 4 * 4) * 4, (row, m)
            assert int(p["query_tiles"]) * tile_words >= int(p["fwords_max"]), (row, m)
        if p["fast_insert"] == "1":                               # ... and the insert's tiles cover the filter
            assert int(p["insert_tiles"]) * int(p["insert_tile_words"]) >= int(p["fwords_max"]), (row, m)
        assert int(p["image_stride"]) >= int(p["fwords_max"]) and int(p["image_stride"]) % 4 == 0


@pytest.mark.parametrize("knobs,known,frames,coded", B.SWEEPS, ids=["%s-%s-%df-%dcoded" % (k, "known" if o else "unknown", f, c) for k, o, f, c in B.SWEEPS])
def test_sweep_finds_the_table_and_nothing_else(exe, knobs, known, frames, coded):
    found = B.sweep(exe, knobs, known, frames, coded)
    assert all(first == last + 1 and before != after for last, first, before, after in found)
    want = B.sweep_rows(knobs, known, frames, coded)
    assert [(last, first) for last, first, _, _ in found] == [(r.last, r.first) for r in want], (found, want)


@pytest.mark.parametrize("row", B.GOP_ROWS, ids=B.row_id)
def test_gop_cases_straddle_their_rows(exe, row):
    """The frame sizes and counts of changed pixels the GOP test of the device submits (plan_boundaries.gop_case; rbf_plan_batch needs
    no GPU): for the batch rbf_encode_gop makes of them -- two pairs, the first coded -- the two planned filters get the row's two
    decisions."""
    from new_bloom_filter_repo_amd import _native as nat
    planned = [B.gop_case(row, side, nat.lib(), nat.FilterParams)[3] for side in B.SIDES]
    assert row.last - 128 < planned[0] <= row.last and row.first <= planned[1] < row.first + 128
    got = B.plans(exe, [(row, m) for m in planned + [row.last, row.first]])
    assert got[0]["decision"] == got[2]["decision"] != got[3]["decision"] == got[1]["decision"], (row, planned)


def test_barrett_only_ignores_the_counts(exe):
    """barrett_only never takes the table insert, so no two-phase insert either: one table serves both entry points."""
    assert B.sweep(exe, "barrett_only", True, 1) == B.sweep(exe, "barrett_only", False, 1)


def test_small_m_reduction_ends_at_two_to_the_thirty(exe):
    at, past = B.plans(exe, [(("default", False, 1, 1), B.SMALL_M_END), (("default", False, 1, 1), B.SMALL_M_END + 1)])
    assert (at["small_m"], past["small_m"]) == ("1", "0")
    assert at["decision"] == past["decision"]                    # the same (generic) kernels, the other reduction
