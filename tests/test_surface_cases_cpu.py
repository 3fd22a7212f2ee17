"""The surface sweep's cases and its composed twin, proven on the CPU (no GPU, no native library): the legality predicate of
surface_cases.py is the constructor's over the full product of its axes; the cases cover every legal pair; every case's clip exercises
what the case turns on, by conditions on the twin's output; the twin has the properties the GPU file then asks of the product; and every
stage of the composition, and its place in the order, changes the output of some case -- so test_gpu_surface_twin.py fails when the
product gets one of them wrong."""
import numpy as np
import pytest

import error_bounds_ref as eb
import near_key_ref as nk
import pan_ref
import scene_cut_ref
import surface_cases as sc
import surface_twin as st
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.surface_options import check_blocks, check_options

I, T = sc.I, sc.T
KEY_KINDS, INTER_KINDS = (st.KEY, st.KEY_RICE, st.KEY_NEAR), (st.INTER, st.INTER_RICE)
RULE_KEYS = [t for t in range(T) if t % I == 0]


def constructor_says(c):
    """None when the product takes the assignment, else its refusal: check_options (the constructor), check_blocks on the plan of every
    range the case codes (encode_range), and the bound frame against the clip's frames (encode_range, before any upload)."""
    kw = sc.keywords(c)
    try:
        o = check_options(**kw)
        for start, stop in (sc.shards(c) or [(0, T)]):
            first = start if start % I == 0 else start - 1
            check_blocks(o, container.plan_range(first, start, stop, I, o.block_frames, True)[1], first, I)
        if o.error_bounds is not None:
            container.bounds_frame(o.error_bounds, sc.frame_shape(c), sc.frame_dtype(c))
    except ValueError as e:
        return str(e)
    return None


def test_the_predicate_is_the_constructor_over_the_full_product():
    n = legal = 0
    for c in sc.product():
        said = constructor_says(c)
        assert (sc.legal(c) is None) == (said is None), (c, sc.legal(c), said)
        n, legal = n + 1, legal + (said is None)
    assert n == int(np.prod([len(v) for _, v in sc.AXES])) and 0 < legal < n


def test_every_legal_pair_is_covered_and_every_case_is_legal():
    idx, ok = sc._index_table()
    want = sc.legal_pairs(idx[ok])
    assert all(sc.legal(c) is None for c in sc.CASES)
    rows = np.array([[sc.AXES[a][1].index(c[name]) for a, name in enumerate(sc.NAMES)] for c in sc.CASES])
    got = sc.legal_pairs(rows)
    missing = {ab: want[ab] - got[ab] for ab in want if want[ab] - got[ab]}
    assert not missing, missing
    assert 20 <= len(sc.CASES) <= 60 and len(set(sc.IDS)) == len(sc.IDS)
    # a pair that never occurs is illegal for a reason legal() states: e.g. a luma mask with any near-lossless mode
    a, b = sc.NAMES.index("mask_channels"), sc.NAMES.index("near")
    assert all((0, v) not in want[(a, b)] for v in range(1, len(sc.NEAR)))
    assert sc.covering_array() + sc.EXTRA == sc.CASES       # deterministic


def _diff(c, tw):
    x = np.stack(sc.clip(c)).astype(np.int64)
    return x, np.stack(tw["decoded"]).astype(np.int64)


@pytest.mark.parametrize("k", range(len(sc.CASES)), ids=sc.IDS)
def test_the_case_exercises_what_it_turns_on(k):
    c, tw = sc.CASES[k], sc.twin_of(k)
    x, y = _diff(c, tw)
    kinds = tw["kinds"][:T]
    E = st.bound_frame(sc.keywords(c), x.shape[1:], sc.frame_dtype(c))
    assert len(tw["decoded"]) == T and all(d.shape == sc.frame_shape(c) and d.dtype == sc.frame_dtype(c) for d in tw["decoded"])
    assert (np.abs(x - y) <= E).all()                                        # every decoded sample within its bound
    inter = [t for t in range(T) if kinds[t] in INTER_KINDS]
    assert inter and all(kinds[t] in KEY_KINDS for t in RULE_KEYS)
    if c["near"] == "off":
        assert np.array_equal(x, y)
    else:
        kept = sum(int((y[t] != x[t]).sum()) for t in inter)
        released = sum(int(((np.abs(x[t] - y[t - 1]) > E) & (y[t] == x[t])).sum()) for t in inter)
        assert kept > 0 and released > 0, (kept, released)
    if c["pan_range"]:
        assert tw["pans"] and tw["pan_offsets"] and tw["kinds"][T] == st.PANS
    else:
        assert not tw["pans"] and not tw["pan_offsets"] and st.PANS not in tw["kinds"]
    if c["scene_cuts"]:
        assert sc.CUT in tw["scene_cuts"]
        if c["pan_range"]:
            assert tw["scene_cuts"] == [sc.CUT]
    else:
        assert tw["scene_cuts"] == []
    if c["bounded_keyframes"]:
        keys = sorted(set(RULE_KEYS) | set(tw["scene_cuts"]))
        assert all(kinds[t] == st.KEY_NEAR and (y[t] != x[t]).any() for t in keys)
    else:
        assert st.KEY_NEAR not in kinds
    if c["mask_channels"] == "luma" and c["layout"] != "grey":
        fallen = [t for t in range(T) if kinds[t] in KEY_KINDS and t not in RULE_KEYS and t not in tw["scene_cuts"]]
        assert fallen and inter, (fallen, inter)
    assert (tw["digests"] is not None) == c["frame_digests"] == (tw["kinds"][-1] == st.DIGESTS)
    assert (tw["quality"] is not None) == c["quality_report"]


def test_a_pan_and_cuts_case_rebases_a_cut_that_carries_an_offset():
    """The cut frame's offset before the re-base: what the alignment alone gives it."""
    hits = []
    for k, c in enumerate(sc.CASES):
        if c["pan_range"] and c["scene_cuts"] and c["route"] == "whole":
            kw = dict(sc.keywords(c), scene_cuts=False)
            before = st.twin(sc.clip(c), kw)["pan_offsets"]
            if before.get(sc.CUT, (0, 0)) != (0, 0):
                hits.append(k)
    assert hits


def test_all_features_off_is_the_identity():
    for c in sc.CASES:
        if c["near"] == "off" and not c["pan_range"]:
            tw = st.twin(sc.clip(c), dict(keyframe_interval=I, mask_channels="all"))
            assert all(np.array_equal(a, b) for a, b in zip(tw["decoded"], sc.clip(c)))
            if not (c["layout"] == "grey" and c["dtype"] == "u16"):          # (one 16-bit channel: the mask is the luma mask, blind to 0x8000)
                assert tw["kinds"] == [st.KEY if t % I == 0 else st.INTER for t in range(T)]


def test_the_invariance_subset_covers_every_mode_and_both_sample_types():
    ks = sc.invariance_cases()
    assert {sc.CASES[k]["near"] for k in ks} == set(sc.NEAR) and {sc.CASES[k]["dtype"] for k in ks} == {"u8", "u16"}


@pytest.mark.parametrize("k", sc.invariance_cases(), ids=[sc.IDS[k] for k in sc.invariance_cases()])
def test_the_decoded_clip_does_not_depend_on_blocks_lanes_codec_or_shards(k):
    c, tw = sc.CASES[k], sc.twin_of(k)
    for change in (dict(block_frames=I), dict(block_frames=2 * I), dict(block_frames=3 * I), dict(gpu_lanes=1), dict(gpu_lanes=3),
                   dict(sample_codec="zlib"), dict(sample_codec="rice"), dict(route="whole"), dict(route="shards")):
        other = dict(c, **change)
        if sc.legal(other) is not None:
            continue
        got = st.twin(sc.clip(other), sc.keywords(other), sc.shards(other))
        assert all(np.array_equal(a, b) for a, b in zip(got["decoded"], tw["decoded"])), change
        assert got["scene_cuts"] == tw["scene_cuts"] and got["pans"] == tw["pans"] and got["pan_offsets"] == tw["pan_offsets"], change
        if "sample_codec" not in change:
            assert got["kinds"] == tw["kinds"], change


# ---- one feature on: the twin is that feature's own reference ---------------------------------------------------------------------------
def _case(**want):
    return next(c for c in sc.CASES if all(c[k] == v for k, v in want.items()))


def test_one_feature_on_is_that_features_reference():
    base = dict(keyframe_interval=I, block_frames=3 * I, mask_channels="all")
    blocks = [(0, 12, [4, 8]), (12, T, [4])]
    assert st.plan(0, 0, T, I, 3 * I) == blocks == [tuple(b) for b in container.plan_range(0, 0, T, I, 3 * I, True)[1]]

    def per_block(x, fn):
        return np.concatenate([fn(np.stack(x[lo:end]), starts) for lo, end, starts in blocks])
    x = sc.clip(_case(near="first_d2", dtype="u8", layout="yuv"))
    E = np.empty(x[0].shape, np.int64)
    E[...] = (1, 3, 3)
    for kw, fn in ((dict(max_error=2), lambda s, r: eb.hold_ref(s, r, 2)),
                   (dict(max_error=1, hold_mode="lookahead"), lambda s, r: eb.lookahead_ref(s, r, 1)[0]),
                   (dict(error_bounds=(1, 3, 3)), lambda s, r: eb.hold_map_ref(s, r, E)),
                   (dict(error_bounds=(1, 3, 3), hold_mode="lookahead"), lambda s, r: eb.lookahead_map_ref(s, r, E)[0])):
        tw = st.twin(x, dict(base, **kw))
        assert np.array_equal(np.stack(tw["decoded"]), per_block(x, fn)), kw
    # bounded keyframes and a hold: the hold of the clip whose run firsts had been Y all along
    y = [nk.quantise(f, [2, 2, 2])[0] if t % I == 0 else f for t, f in enumerate(x)]
    tw = st.twin(x, dict(base, max_error=2, bounded_keyframes=True, sample_codec="rice"))
    assert np.array_equal(np.stack(tw["decoded"]), per_block(y, lambda s, r: eb.hold_ref(s, r, 2)))
    # cuts alone: the rule on the statistic of every block
    tw = st.twin(x, dict(base, scene_cuts=True))
    want = [lo + j for lo, end, starts in blocks for j in scene_cut_ref.cut_frames(scene_cut_ref.cut_stats(np.stack(x[lo:end]), 0), starts)]
    assert tw["scene_cuts"] == want and sc.CUT in want
    # pan alone: the stabilised block, its offsets and its adopted pairs
    p = sc.clip(_case(pan_range=sc.R, near="off"))
    tw = st.twin(p, dict(base, pan_range=sc.R))
    for lo, end, starts in blocks:
        S, offs, adopted, _ = pan_ref.stabilise(p[lo:end], sc.R, 0, starts)
        for j in range(1, end - lo):
            assert np.array_equal(tw["coded"][lo + j], S[j]) and tw["pan_offsets"].get(lo + j, (0, 0)) == tuple(offs[j])
        assert [r for r in tw["pans"] if lo < r[0] < end] == [(lo + j, dx, dy) for j, dx, dy in adopted]
    assert all(np.array_equal(a, b) for a, b in zip(tw["decoded"], p))
    # digests alone: FD1 of the frames; quality alone: zeros
    tw = st.twin(x, dict(base, frame_digests=True, quality_report=True))
    assert tw["digests"] == [pan_ref.fd1(f.tobytes()) for f in x] and not tw["quality"]["differing"].any()


# ---- every stage and its place in the order matter -----------------------------------------------------------------------------------
def _same(a, b):
    if a["kinds"] != b["kinds"] or a["scene_cuts"] != b["scene_cuts"] or a["pans"] != b["pans"] or a["pan_offsets"] != b["pan_offsets"]:
        return False
    if a["digests"] != b["digests"]:
        return False
    return all(np.array_equal(u, v) for u, v in zip(a["decoded"], b["decoded"]))


@pytest.mark.parametrize("mutant", [m for m in st.MUTANTS if m not in st.GEOMETRY_MUTANTS])      # (those: test_surface_geometries_cpu.py)
def test_the_cases_tell_the_mutant_from_the_twin(mutant):
    caught = [sc.IDS[k] for k in range(len(sc.CASES)) if not _same(sc.twin_of(k), sc.twin_of(k, mutant))]
    assert caught, mutant
