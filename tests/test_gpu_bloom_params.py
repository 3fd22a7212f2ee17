"""The Bloom core under filter lengths and activation thresholds that sit ON the pixel hashes (tests/bloom_params.py;
tests/test_bloom_params_cpu.py proves on the CPU that every case has its property and pins which kernels every batch reaches):

  thresholds  T equal to a pixel's activation hash and one above it, 0, 1, 2^64 - 1, the smallest and the largest hash, the fullest
              16-bit tag: `ha < T` in its three forms -- the plain compare, the tag shortcut of insert_tab_steps, the activation ranks.
  lengths     m at which a set pixel's first position is 0 or m - 1, its step 0 or m - 1, position + step m or m - 1, in the FP64 range
              and below it, with floor_k 0, 1, 2, 5, 6 and 64.
  ranks       batches of 1, 2, 3, 5, 127 and 128 coded frames with equal, distinct and unsorted, duplicated and interleaved thresholds.

Everything goes through BloomEngine.encode / decode with explicit (m, floor_k, T) under every knob of bloom_rows.KNOBS and 32; the length
cases also through rbf_filter_insert_indices / rbf_filter_query_indices.  The reference is integer arithmetic on the oracle's hashes,
computed once per process whatever the knob; every decode is fed the REFERENCE's filter and witness.  Bit-exact comparisons only."""
import numpy as np
import pytest

import bloom_params as bp
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd.engine import BloomEngine, DeviceFilter

pytestmark = pytest.mark.gpu

SEEDS = pytest.mark.parametrize("seeds", bp.SEED_TRIPLES, ids=bp.SEED_IDS)
KNOBS = pytest.mark.parametrize("knob", bp.KNOBS, ids=bp.KNOB_IDS)


@pytest.fixture(scope="module")
def engines():
    """one context and engine per knob, made when first asked for"""
    made = {}

    def get(knob):
        if knob not in made:
            ctx = nat.Context(0)
            ctx.force_generic(knob)
            made[knob] = (ctx, BloomEngine(ctx))
        return made[knob][1]
    yield get
    for ctx, eng in made.values():
        eng.close()
        ctx.close()


def run_batch(eng, oracle, cases, what):
    """One batch: encode the cases' masks and compare every coded frame's filter bytes, filter_ones, witness_bits and witness bytes with
    the reference; decode the reference's filters and witnesses and compare every mask (a frame that is not coded decodes to zeros)."""
    frames = [bp.frame_of(oracle, c) for c in cases]
    seeds = cases[0].seeds
    assert all(c.seeds == seeds for c in cases)
    plist = [(fr.m, fr.floor_k, fr.T) for fr in frames]
    eng.upload_masks(np.stack([np.packbits(fr.mask) for fr in frames]), bp.N)
    out = eng.encode(bp.N, plist, seeds)
    for c, fr, r in zip(cases, frames, out):
        where = (what, c.name)
        if not fr.m:
            assert r["witness_bits"] == 0 and r["filter_ones"] == 0, (where, "a frame that is not coded")
            continue
        assert np.array_equal(r["filter"], fr.filter[:(fr.m + 7) // 8]), (where, "filter")
        assert r["filter_ones"] == fr.filter_ones, (where, "filter_ones", r["filter_ones"], fr.filter_ones)
        assert r["witness_bits"] == fr.witness_bits, (where, "witness_bits", r["witness_bits"], fr.witness_bits)
        assert np.array_equal(r["witness"], fr.witness[:(fr.witness_bits + 7) // 8]), (where, "witness")
    dec = eng.decode(bp.N, plist, [fr.filter[:(fr.m + 7) // 8] for fr in frames], [fr.witness[:(fr.witness_bits + 7) // 8] for fr in frames], seeds)
    for c, fr, row in zip(cases, frames, dec):
        want = np.packbits(fr.mask) if fr.m else np.zeros((bp.N + 7) // 8, np.uint8)
        assert np.array_equal(row, want), ((what, c.name), "decode of the reference's filter and witness")


@KNOBS
@SEEDS
def test_thresholds_on_the_activation_hashes(oracle, engines, seeds, knob):
    """Sixteen frames in one batch: every T / T + 1 pair side by side, so the rank search of the FP64 query kernels also sees thresholds
    one apart."""
    th = bp.threshold_cases(oracle, seeds)
    run_batch(engines(knob), oracle, th.cases, ("thresholds", hex(knob)))
    run_batch(engines(knob), oracle, th.cases[::-1], ("thresholds, reversed", hex(knob)))


@KNOBS
@pytest.mark.parametrize("batch", bp.LENGTH_BATCHES)
@SEEDS
def test_lengths_that_put_a_remainder_on_an_edge(oracle, engines, seeds, batch, knob):
    """Per condition one batch of one filter length with every floor_k (bloom_params.length_cases): `f64` fits LDS twice and takes
    k_insert_tab + k_query_u64 by default, `f64far` is the same pixel's largest length (k_query_s64t, the generic insert) in a batch of its
    own -- the planner plans a batch by its largest filter --, `small` lies below the FP64 range, a tiny filter behind a roomy one."""
    lengths = bp.length_cases(oracle, seeds)
    ran = 0
    for cond in bp.CONDITIONS:
        if (batch, cond) in lengths.cases:
            run_batch(engines(knob), oracle, lengths.cases[batch, cond], ("lengths", hex(knob)))
            ran += 1
    assert ran == len(bp.CONDITIONS) or batch == "f64far"


@KNOBS
@pytest.mark.parametrize("count", bp.RANK_COUNTS)
@SEEDS
def test_whole_batches_for_the_rank_search(oracle, engines, seeds, count, knob):
    batches = bp.rank_batches(oracle, seeds)
    for kind in bp.RANK_KINDS:
        run_batch(engines(knob), oracle, batches[count, kind], ("ranks", count, kind, hex(knob)))


@pytest.mark.parametrize("batch", bp.LENGTH_BATCHES)
@SEEDS
def test_lengths_through_the_per_index_surface(oracle, seeds, batch):
    """rbf_filter_insert_indices / rbf_filter_query_indices with explicit parameters, twice per case: the selected pixel and its two
    neighbours alone into an empty filter (the filter is then exactly their positions), then with 200 random indices; the inserted
    indices and 203 others queried."""
    lengths = bp.length_cases(oracle, seeds)
    with nat.Context(0) as ctx:
        for cond in bp.CONDITIONS:
            for c in lengths.cases.get((batch, cond), ()):
                for ins, q in bp.index_lists(c):
                    bits, verdicts = bp.index_reference(oracle, c, ins, q)
                    with DeviceFilter(ctx, c.m) as f:
                        f.insert(ins, c.floor_k, c.T, seeds)
                        assert np.array_equal(f.bits(), bits), (c.name, len(ins), "filter")
                        assert np.array_equal(f.query(q, c.floor_k, c.T, seeds), verdicts), (c.name, len(ins), "verdicts")
                        assert np.array_equal(f.bits(), bits), (c.name, len(ins), "the query leaves the filter alone")
