"""The device on both sides of every row of the planner's boundary table (tests/plan_boundaries.py; tests/test_plan_boundaries_cpu.py
proves the table against the planner): the last filter size of one kernel combination and the first of the next, where an LDS budget
is used to the last byte and where a tile count, a SAFE dword offset or an image pitch changes.  Everything is compared bit for bit
with the C oracle (orc_compress): filter, filter_ones, witness_bits, witness; and every decode is fed the ORACLE's filter and witness,
so that a decoder bug cannot hide behind a matching encoder bug.  An LDS access past the allocation reads zeros on this chip instead
of faulting: only such a comparison shows it, and only on a filter that is well filled -- the oracle's filter of every case is
between 20 % and 60 % full (k* x ones / m = 0.5: 39 %), so a set bit read as clear and a clear bit read as set both change the witness.

Shapes: the smallest that keep that fill, n = 2 m / k* pixels at density 0.25 with n % 8 == 5; the GOP rows need the n whose planned
filter is the row's (n = 3.2 m).  The oracle's results are computed ahead of the tests on a few threads (plan_boundaries.References)."""
import collections

import numpy as np
import pytest

import plan_boundaries as B
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import params as P
from new_bloom_filter_repo_amd.engine import BloomEngine
from new_bloom_filter_repo_amd.gop import GopCoder

pytestmark = pytest.mark.gpu

SEEDS = P.SEEDS_VIDEO
RAN = collections.Counter()             # (row, side) -> times run; test_every_row_ran_on_both_sides reads it


@pytest.fixture(scope="module")
def refs(oracle):
    """every oracle result of this file, named in the order the tests below ask for them"""
    oracle.lib()
    r = B.References()
    for row in B.BATCH_ROWS:
        for side in B.SIDES:
            r.plan(("batch", row, side), B.batch_reference, oracle, SEEDS, *B.batch_case(row, side))
    for j in range(B.FRAMES_OTHERS):
        r.plan(("other", j), B.other_reference, oracle, SEEDS, j)
    for m in sorted({getattr(row, side) for row in B.FRAME_ROWS for side in B.SIDES}):
        r.plan(("edge", m), B.edge_reference, oracle, SEEDS, m)
    for j in range(len(B.MIXED)):
        r.plan(("mixed", j), B.mixed_reference, oracle, SEEDS, j)
    for i, row in enumerate(B.GOP_ROWS):
        for side in B.SIDES:
            W, H, ones, m = B.gop_case(row, side, nat.lib(), nat.FilterParams)
            r.plan(("gop", row, side), B.gop_reference, oracle, SEEDS, 9000 + i, W, H, ones, m)
    yield r
    r.close()


@pytest.fixture(scope="module")
def engines():
    """one context and engine per knob set, made when first asked for"""
    made = {}

    def get(knobs):
        if knobs not in made:
            ctx = nat.Context(0)
            ctx.force_generic(B.KNOBS[knobs])
            made[knobs] = (ctx, BloomEngine(ctx))
        return made[knobs]
    yield get
    for ctx, eng in made.values():
        eng.close()
        ctx.close()


def encode_decode(eng, n, frames, what):
    """frames: the References of one batch.  Encode their masks and compare every coded frame; decode the oracle's filters and
    witnesses in one call and compare every coded frame's mask."""
    plist = [P.filter_params(ref.k, ref.m) for ref in frames]
    eng.upload_masks(np.stack([np.packbits(ref.mask) for ref in frames]), n)
    out = eng.encode(n, plist, SEEDS)
    for f, (r, ref) in enumerate(zip(out, frames)):
        if ref.m:
            B.check_encoded(r, ref, (what, "frame", f, "m", ref.m, "k*", ref.k))
        else:
            assert r["witness_bits"] == 0, (what, "frame", f, "is not coded")
    dec = eng.decode(n, plist, [ref.filter for ref in frames], [ref.witness[1] for ref in frames], SEEDS)
    for f, ref in enumerate(frames):
        if ref.m:
            B.check_decoded(dec[f], ref, (what, "frame", f, "m", ref.m, "k*", ref.k))


# ---- a. batch entry, counts unknown: one frame ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", B.SIDES)
@pytest.mark.parametrize("row", B.BATCH_ROWS, ids=B.row_id)
def test_batch_entry_on_both_sides_of_a_row(refs, engines, row, side):
    n, m, k, _ = B.batch_case(row, side)
    assert n <= B.MAX_PIXELS and n % 512 and n % 8
    ref = refs.get(("batch", row, side))
    assert (ref.m, ref.k, len(ref.mask)) == (m, k, n)
    encode_decode(engines(row.knobs)[1], n, [ref], (B.row_id(row), side))
    RAN[row, side] += 1


# ---- b. the rows that depend on the frame count ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def others(refs):
    """the frames around the boundary filter (plan_boundaries.other_frame), shared by every batch below and left unchanged"""
    frames = [refs.get(("other", j)) for j in range(B.FRAMES_OTHERS)]
    coded = [ref for ref in frames if ref.m]
    assert [j for j, ref in enumerate(frames) if not ref.m] == list(B.FRAMES_UNCODED)
    assert len({ref.m for ref in coded}) > len(coded) // 2 and len({ref.k for ref in coded}) == len(B.KSTARS)
    for ref in coded:
        assert B.FILL[0] <= ref.fill <= B.FILL[1] and ref.m < min(row.last for row in B.FRAME_ROWS), (ref.m, ref.k, ref.fill)
    return frames


@pytest.fixture(scope="module")
def edges(refs):
    return {m: refs.get(("edge", m)) for m in sorted({getattr(row, side) for row in B.FRAME_ROWS for side in B.SIDES})}


@pytest.mark.parametrize("side", B.SIDES)
@pytest.mark.parametrize("row", B.FRAME_ROWS, ids=B.row_id)
def test_frame_count_rows_as_batches(others, edges, engines, row, side):
    """Batches of row.frames frames whose largest filter sits at the boundary, once as frame 0 and once as the last frame; the other
    frames are smaller filters with their own m, k* and masks, two of them with m = 0 -- and once more with every frame coded."""
    edge = edges[getattr(row, side)]
    eng = engines(row.knobs)[1]
    for where, frames in B.batches_of(row, edge, others):
        assert len(frames) == row.frames and all(ref.m < edge.m for ref in frames if ref is not edge)
        assert sum(1 for ref in frames if not ref.m) == (0 if "all coded" in where else 2)
        encode_decode(eng, B.FRAMES_PIXELS, frames, (B.row_id(row), side, "boundary filter", where))
    RAN[row, side] += 1


# ---- c. one batch across both ends of the FP64 range -------------------------------------------------------------------------------------
def test_mixed_batch_across_both_ends_of_the_fp64_range(refs, engines):
    """m = 32767, 32768, 8388607 and 8388608 in one batch: whatever split over the kernel families the library makes, every frame
    matches the oracle, encoded and decoded."""
    frames = [refs.get(("mixed", j)) for j in range(len(B.MIXED))]
    assert [ref.m for ref in frames] == [32767, 32768, 8388607, 8388608]
    encode_decode(engines("default")[1], B.MIXED_PIXELS, frames, "mixed")
    encode_decode(engines("default")[1], B.MIXED_PIXELS, frames[::-1], "mixed, reversed")


# ---- d. GOP entry, counts known ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", B.SIDES)
@pytest.mark.parametrize("row", B.GOP_ROWS, ids=B.row_id)
def test_gop_entry_on_both_sides_of_a_row(refs, engines, row, side):
    """rbf_encode_gop on luma-only frames: one coded pair (frame 1 is frame 0 with exactly `ones` pixels changed, `ones` found on the
    host so that the planned filter lies within 128 bits of the row, on its side) and one unchanged pair.  The rows are those of
    that batch of two (tests/test_plan_boundaries_cpu.py checks on the host that the two planned filters get different decisions)."""
    assert (row.frames, row.coded) == (2, 1)                     # what rbf_encode_gop plans for the three frames below: two pairs, one coded
    W, H, ones, m = B.gop_case(row, side, nat.lib(), nat.FilterParams)
    assert row.last - 128 < m <= row.last if side == "last" else row.first <= m <= row.first + 128
    n = W * H
    assert n % 512 and n % 8 and ones <= B.DENSITY * n
    frames, ref, k = refs.get(("gop", row, side))
    ctx, eng = engines(row.knobs)
    what = (B.row_id(row), side, "n", n, "ones", ones, "m", m)
    with GopCoder(ctx, W, H, 3, channels=1) as coder:
        coder.load_frames(frames)
        coder.encode()
        coded, unchanged = coder.results()
    assert B.same_bits(coded["mask"], np.packbits(ref.mask), n), (what, "mask")
    assert (coded["k"], coded["l"]) == (k, m) and coded["ones"] == ones, (what, coded["k"], coded["l"])
    B.check_encoded(coded, ref, what)
    assert unchanged["l"] == 0 and unchanged["witness_bits"] == 0 and unchanged["ones"] == 0 and not np.any(unchanged["mask"]), what
    dec = eng.decode(n, [P.filter_params(k, m)], [ref.filter], [ref.witness[1]], SEEDS)
    B.check_decoded(dec[0], ref, what)
    RAN[row, side] += 1


def test_every_row_ran_on_both_sides():
    """No row of the table may be left out: what ran above is every row, on both sides, once."""
    assert len(B.BATCH_ROWS) + len(B.FRAME_ROWS) + len(B.GOP_ROWS) == len(B.ROWS)
    assert RAN == collections.Counter({(row, side): 1 for row in B.ROWS for side in B.SIDES})
    assert sum(RAN.values()) == 2 * len(B.ROWS)
