"""tests/foreign_decode.py on the CPU: every case has the property it is named for, the reference is the oracle's decompress wherever the
witness is long enough, the replay of k_expand_mask's window gives the reference on every case, and every mutant of the window differs
from it on its named case -- so the device comparison of tests/test_gpu_foreign_decode.py can fail."""
import numpy as np
import pytest

import bloom_params as bp
import bloom_rows as br
import foreign_decode as fd


@pytest.fixture(scope="module")
def batches(oracle):
    return fd.batches(oracle)


def test_the_geometries():
    assert fd.N == 509 * 257 == 130813 and fd.N % 64 == 61
    assert fd.MANY_N == 799 * 11 and fd.MANY_N % 64 != 0
    assert all(m >= br.F64_MIN for m in fd.F64_M) and all(m < br.F64_MIN for m in fd.SMALL_M)
    assert fd.GRID_M < bp.F64_RANGE[1]


def test_pass_rates_no_encoder_reaches(oracle, batches):
    rates = fd.rate_frames(oracle)
    assert rates["all_ones_k1"].passes.all() and rates["all_ones_k64"].passes.all() and rates["k0_T0"].passes.all()
    assert not rates["all_zero_k2"].passes.any() and rates["all_zero_k2"].floor_k >= 1
    assert not fd.sentinel(oracle, fd.N).passes.any() and not fd.sentinel(oracle, fd.MANY_N).passes.any()
    assert (rates["k0_T0"].floor_k, rates["k0_T0"].T) == (0, 0) and not rates["k0_T0"].bits.any(), "nothing is probed: the filter does not matter"
    assert (rates["k0_Tmax"].floor_k, rates["k0_Tmax"].T) == (0, fd.U64_MAX)
    rate = rates["k0_Tmax"].passes.mean()
    assert 0.65 < rate < 0.75, rate
    # all ones: the mask is the first n witness bits, whatever the parameters
    b = batches["rates"]
    for f in (0, 8):
        assert b.frames[f].passes.all()
        assert np.array_equal(fd.reference_mask(b.frames[f].passes, b.witness[f], b.stride), np.unpackbits(b.witness[f])[:fd.N])
    # a frame that passes n positions in front of one that passes none
    assert b.frames[0].passes.sum() == fd.N and not b.frames[1].passes.any() and (b.witness[1] == 0xFF).all()
    # the ragged last word full
    for name in ("all_ones_k1", "grid"):
        c, _ = fd.word_counts(rates[name].passes)
        assert c[-1] == 61, name
    # the pad bits of a full-length witness row are ones: a kernel that deals them out shows
    assert np.unpackbits(b.witness[0])[fd.N:].all() and b.stride * 8 - fd.N == 3


def test_the_grid_of_window_shapes(oracle, batches):
    """Words with c = 64, c >= 33 and c = 1 at every r = o & 31, from the filter of a chosen pixel set (the few false positives of a
    roomy filter included: the grid is read off the pass set the reference computes)."""
    grid = fd.rate_frames(oracle)["grid"]
    chosen = fd.grid_pixels()
    assert grid.passes[chosen].all()
    extra = int(grid.passes.sum()) - len(set(chosen.tolist()))
    assert 0 <= extra < 64, extra
    pairs = fd.cr_pairs(grid.passes)
    for r in range(32):
        assert (64, r) in pairs, ("c = 64", r)
        assert (1, r) in pairs, ("c = 1", r)
        assert any((c, r) in pairs for c in range(33, 64)), ("c >= 33", r)
    assert fd.third_dword_words(grid.passes) >= 64
    # the family frames: hundreds of (c, r) pairs more, and third dwords in every one of them
    every = set(pairs)
    for fr in batches["family_f64"].frames + batches["family_small"].frames:
        if not fd.is_sentinel(fr):
            assert fd.third_dword_words(fr.passes) > 100, fr.name
            every |= fd.cr_pairs(fr.passes)
    assert len(every) > 600, len(every)
    # ... and over every batch of the geometry, the figure DESIGN.md 7 and profiles/r27_foreign_decode.txt quote
    for b in batches.values():
        if b.n == fd.N:
            for fr in b.frames:
                every |= fd.cr_pairs(fr.passes)
    assert len(every) == 1214, len(every)


def test_witness_strides(oracle, batches):
    rates = fd.rate_frames(oracle)
    for fr, tag in ((rates["k0_Tmax"], "rich"), (rates["all_ones_k1"], "all")):
        passes = int(fr.passes.sum())
        exact = (passes + 63) // 64 * 8
        want = {"exact": exact, "minus8": exact - 8, "minus16": exact - 16, "eight": 8}
        for name, stride in want.items():
            b = batches["stride_%s_%s" % (tag, name)]
            assert b.stride == stride and b.frames[0] is fr and fd.is_sentinel(b.frames[1]) and (b.witness[1] == 0xFF).all()
            mask = fd.reference_mask(fr.passes, b.witness[0], b.stride)
            late = np.flatnonzero(fr.passes)[b.stride * 8:]
            assert not mask[late].any() and (len(late) > 0) == (name != "exact"), (tag, name)
    rich = rates["k0_Tmax"]
    c, o = fd.word_counts(rich.passes)
    for kind in ("last_is_last", "second_is_past", "third_is_past"):
        b = batches["window_" + kind]
        stride, w = fd.window_stride(rich.passes, kind)
        assert b.stride == stride and stride % 8 == 0
        d0, dl, s32 = int(o[w]) >> 5, int(o[w] + c[w] - 1) >> 5, stride // 4
        if kind == "last_is_last":
            assert dl == d0 + 2 == s32 - 1
        elif kind == "second_is_past":
            assert dl >= d0 + 1 == s32
        else:
            assert dl == d0 + 2 == s32


def test_families_and_batch_sizes(oracle, batches):
    for name, lengths in (("family_f64", fd.F64_M), ("family_small", fd.SMALL_M)):
        coded = [fr for fr in batches[name].frames if not fd.is_sentinel(fr)]
        assert tuple(fr.floor_k for fr in coded) == fd.FLOOR_KS and all(fr.m in lengths for fr in coded)
        for fr in coded:
            assert 0.3 < fr.passes.mean() < 0.9, (fr.name, fr.passes.mean())   # neither empty nor saturated (a filter of 521 bits: as its draw falls)
    mixed = [fr for fr in batches["family_mixed"].frames if not fd.is_sentinel(fr)]
    assert sum(fr.m >= br.F64_MIN for fr in mixed) == 6 and sum(fr.m < br.F64_MIN for fr in mixed) == 6
    assert all(fr.m < br.F64_MIN for fr in batches["family_small"].frames), "sentinels included: no frame of it takes an FP64 kernel"
    assert [len(batches["frames_%d" % c].frames) for c in (2, 128, 130)] == [2, 128, 130] and len(batches["one_frame"].frames) == 1
    b = batches["frames_130"]
    assert len(b.frames) > br.MAX_BATCH and not fd.is_sentinel(b.frames[128]) and b.frames[128].passes.any(), "the second chunk starts on a frame that passes"
    assert b.stride == br.packed_stride(fd.MANY_N) - 8 and b.frames[0].passes.all(), "an all-pass row one word short"
    assert set(fd.KNOB_BATCHES) <= set(batches)


def test_the_reference_is_the_oracles_where_the_witness_is_long_enough(oracle, batches):
    checked = 0
    for b in batches.values():
        if b.n != fd.N:
            continue
        for f, fr in enumerate(b.frames):
            if fr.k is None or int(fr.passes.sum()) > b.stride * 8:
                continue
            wit = np.zeros(fr.n, np.uint8)
            have = np.unpackbits(b.witness[f])[:fr.n]
            wit[:len(have)] = have
            want = oracle.decompress(fr.bits, wit, fr.n, fr.k, fd.SEEDS)
            assert np.array_equal(fd.reference_mask(fr.passes, b.witness[f], b.stride), want), (b.name, f, fr.name)
            checked += 1
    assert checked >= 20
    enc, src = fd.encoder_pair_batch(oracle)
    for f, (fr, s) in enumerate(zip(enc.frames, src)):
        assert np.array_equal(fd.reference_mask(fr.passes, enc.witness[f], enc.stride), s.mask), f
        assert int(fr.passes.sum()) == s.witness_bits


def test_the_replay_of_the_window_gives_the_reference(batches):
    for name, b in batches.items():
        if b.n != fd.N:
            continue
        want = fd.expected_rows(b)
        for f, fr in enumerate(b.frames):
            if fd.is_sentinel(fr) and f != 1:
                continue
            for base in (0, 8):
                got = fd.replay(b, f, base=base)
                assert got is not None and np.array_equal(got, want[f]), (name, f, base)
            if name not in ("rates", "grid", "family_mixed"):
                break                                              # (the stride batches repeat one frame: its first row says it)
    b = batches["frames_130"]
    want = fd.expected_rows(b)
    for f in (0, 2, 127, 128, 129):
        assert np.array_equal(fd.replay(b, f), want[f]), f


@pytest.mark.parametrize("mutant", fd.MUTANTS)
def test_every_mutant_differs_from_the_reference_on_its_case(batches, mutant):
    name, f = fd.MUTANT_CASES[mutant]
    b = batches[name]
    want = fd.expected_rows(b)[f]
    got = fd.replay(b, f, mutant)
    assert got is None or not np.array_equal(got, want), (mutant, name, f)
    assert np.array_equal(fd.replay(b, f), want)
    if mutant == "no_stride_clamp":                                # what the mutant takes instead: the sentinel row's ones
        assert got is not None and int(np.unpackbits(got).sum()) > int(np.unpackbits(want).sum())
