"""tests/value_key_ref.py on the CPU: the shapes, masks, lists and keys of the value / key sweep reach the paths they are meant to reach and
the references say something there -- so a seed or a table that does not never reaches the GPU test.

On the filter fills: a whole-filter comparison against a filter that is 20..60 % full is asked for wherever the COUNT of keys is this
project's to choose: the long index list, the decimal keys that rebuild it, and the three-keys-per-length set at m = 2003 (added for that
reason).  The short index lists (at most 257 indices) and the per-length keys at m = 1 000 003 and 16 777 259 have their counts fixed by
what they cover, and are far emptier; their fills are computed and pinned below as well, from the other side."""
import numpy as np
import pytest

import value_key_ref as vk
from oracle import pyref


# ------------------------------------------------------------------ A, B: shapes and masks
def all_shapes():
    return [(vk.H, vk.W), (vk.BIG_H, vk.BIG_W), (vk.SMALL_H, vk.SMALL_W)]


def test_no_shape_is_a_multiple_of_a_word_or_a_segment():
    for h, w in all_shapes():
        assert (h * w) % 64 and (h * w) % vk.SEG, (h, w)
    assert vk.H * vk.W == 8777 and vk.segments(vk.H * vk.W) == 9
    assert vk.BIG_H * vk.BIG_W == 1052651 and vk.segments(vk.BIG_H * vk.BIG_W) == 1028


def test_the_large_shape_carries_into_a_second_round_of_the_scan():
    n = vk.BIG_H * vk.BIG_W
    assert vk.segments(n) > vk.SCAN_ROUND
    for name, mask in list(vk.big_masks(n, 4200).items()) + [(None, m) for m in vk.big_clip().masks]:
        assert mask[vk.SCAN_ROUND * vk.SEG:].sum() > 0, name
        assert mask[:vk.SCAN_ROUND * vk.SEG].sum() > 0, "the carry is not zero either"


@pytest.mark.parametrize("dtype,C,kind", vk.VALUE_CASES, ids=vk.VALUE_IDS)
def test_layouts_and_masks(dtype, C, kind):
    lay = vk.layout(kind, dtype, C)
    assert lay.pixel_stride % lay.sb == 0 and lay.row_pitch % lay.sb == 0, "no unaligned 16-bit access"
    assert lay.flat == (kind == "flat") and (lay.pixel_stride > C * lay.sb) == (kind == "pixels")
    assert vk.sample_byte_map(lay).sum() == lay.n * C * lay.sb
    masks = vk.mask_set(lay.n, 4000)
    assert list(masks) == list(vk.MASK_NAMES)
    assert masks["empty"].sum() == 0 and masks["full"].all()
    assert np.flatnonzero(masks["first"]).tolist() == [0] and np.flatnonzero(masks["last"]).tolist() == [lay.n - 1]
    assert 0.05 < masks["p07"].mean() < 0.09 and 0.88 < masks["p90"].mean() < 0.92
    s = masks["seg3_empty_seg4_full"]
    assert not s[3 * vk.SEG:4 * vk.SEG].any() and s[4 * vk.SEG:5 * vk.SEG].all() and s[:3 * vk.SEG].any() and s[5 * vk.SEG:].any()
    blk, stride = vk.mask_block([masks["p07"], masks["full"]], lay.n)
    ps = vk.packed_stride(lay.n)
    assert stride == ps + 64 and stride % 8 == 0 and len(blk) == 2 * stride
    assert (blk[ps:stride] == 0xFF).all() and (blk[stride + ps:] == 0xFF).all(), "set bits between and behind the rows"
    assert np.array_equal(np.unpackbits(blk[:ps])[:lay.n], masks["p07"]) and not np.unpackbits(blk[stride:stride + ps])[lay.n:].any()


@pytest.mark.parametrize("dtype,C,kind", vk.VALUE_CASES, ids=vk.VALUE_IDS)
def test_every_scatter_changes_every_masked_sample_and_no_other_byte(dtype, C, kind):
    lay = vk.layout(kind, dtype, C)
    frame = vk.frame_bytes(lay, 4001)
    legal = vk.sample_byte_map(lay)
    for name, mask in vk.mask_set(lay.n, 4000).items():
        vals = vk.scatter_values(frame, lay, mask, 4002)
        have = vk.gather_ref(frame, lay, mask)
        assert vals.dtype == lay.dtype and len(vals) == mask.sum() * C and (vals != have).all(), name
        out = vk.scatter_ref(frame, lay, mask, vals)
        assert np.array_equal(vk.gather_ref(out, lay, mask), vals), name
        changed = out != frame
        assert not changed[~legal].any(), "padding and the samples past `channels` stay"
        m2 = mask.reshape(lay.H, lay.W)
        assert not vk.pixel_bytes(changed, lay)[~m2].any(), "pixels outside the mask stay"
        assert (vk.samples(out, lay)[m2] != vk.samples(frame, lay)[m2]).all(), "every masked sample changes"


def test_large_scatter_changes_every_masked_sample():
    lay = vk.layout("flat", np.uint8, 1, vk.BIG_H, vk.BIG_W)
    frame = vk.frame_bytes(lay, 4201)
    for name, mask in vk.big_masks(lay.n, 4200).items():
        vals = vk.scatter_values(frame, lay, mask, 4202)
        out = vk.scatter_ref(frame, lay, mask, vals)
        assert np.array_equal(out != frame, mask), name


@pytest.mark.parametrize("dtype,C,kind", vk.BATCH_CASES, ids=vk.BATCH_IDS)
def test_batch_reference_and_uncovered_counts(dtype, C, kind):
    clip = vk.sweep_clip(dtype, C, kind)
    ref = vk.batch_ref(clip)
    counts = np.diff(ref.offsets.astype(np.int64))
    assert counts[1] == 0 and counts[2] == clip.lay.n and counts[0] > 0 and counts[3] > 0
    assert len(ref.values) == counts.sum() * C and ref.values.dtype == clip.lay.dtype
    assert ref.uncovered[3] == vk.CHROMA_PIXELS, "the changes pair 3's mask misses"
    assert ref.uncovered[2] == 0, "the full mask leaves nothing uncovered"
    assert ref.uncovered[0] > 0 and ref.uncovered[1] > ref.uncovered[0], "random frames differ nearly everywhere"
    if C > 1:                      # pair 3's mask IS the difference of sample 0
        a = vk.samples(clip.block, clip.lay, 3 * clip.frame_stride)
        b = vk.samples(clip.block, clip.lay, 4 * clip.frame_stride)
        assert np.array_equal((a[..., 0] != b[..., 0]).reshape(-1), clip.masks[3])


def test_capacity_cuts():
    dtype, C, kind = vk.CAPACITY_CASE
    assert (dtype, C, kind) in vk.BATCH_CASES
    off = [int(o) for o in vk.batch_ref(vk.sweep_clip(dtype, C, kind)).offsets]
    caps = vk.capacities(off)
    assert 0 in caps.values() and off[-1] in caps.values() and off[-1] - 1 in caps.values() and 1 in caps.values()
    assert any(c in off[1:-1] for c in caps.values()), "a cut on a pair boundary"
    inside = [c for c in caps.values() if any(lo < c < hi for lo, hi in zip(off, off[1:]))]
    assert caps["mid-pair-2"] in inside and caps["boundary+1"] in inside and off[2] < caps["mid-pair-2"] < off[3]
    assert max(caps.values()) <= off[-1]


def test_small_and_big_clips():
    small = vk.small_clip()
    assert small.F == 301 and len(small.masks) == 300 and small.lay.n == 63
    counts = np.array([m.sum() for m in small.masks])
    assert (counts == 0).sum() >= 40 and (counts > 0).sum() >= 200
    big = vk.big_clip()
    ref = vk.batch_ref(big)
    assert big.F == 3 and ref.uncovered[0] > 0 and ref.uncovered[1] == 0


# ------------------------------------------------------------------ C: index lists
def fill(bits):
    return float(np.asarray(bits).mean())


def test_long_lists_take_the_second_trip_and_the_filter_is_half_full(oracle):
    lc = vk.long_case(oracle)
    assert vk.LONG_N > vk.GRID_LIMIT and len(lc.query) == vk.LONG_N > vk.GRID_LIMIT
    assert np.array_equal(np.sort(lc.query), np.arange(vk.LONG_N)) and not np.array_equal(lc.query, np.arange(vk.LONG_N))
    ones = np.flatnonzero(lc.mask)
    assert len(lc.insert) == len(ones) + vk.LONG_DUPLICATES and np.array_equal(np.unique(lc.insert), ones)
    assert 0.20 < fill(lc.filt) < 0.60 and 0.20 < fill(lc.filt_or) < 0.60, (fill(lc.filt), fill(lc.filt_or))
    assert len(lc.extra) == vk.LONG_EXTRA == len(set(lc.extra.tolist())) and not lc.filt[lc.extra].any(), "bits the insert does not set"
    assert lc.filt_or.sum() == lc.filt.sum() + vk.LONG_EXTRA
    assert lc.verdicts[ones].all() and 0 < lc.verdicts[lc.mask == 0].mean() < 0.5, "no false negative, some false positives"
    assert (lc.verdicts_or >= lc.verdicts).all() and (lc.verdicts_or != lc.verdicts).any(), "the extra bits change some verdicts"
    # the long list against the short lists' reference, on a sample
    f = oracle.RationalFilter(vk.LONG_M, vk.LONG_K, vk.SEEDS_VIDEO)
    f.bit_array[:] = lc.filt_or
    for i in lc.query[:2000]:
        assert f.check_index(int(i)) == bool(lc.verdicts_or[i])


def test_decimal_blob_is_str(oracle):
    idx = np.array([0, 9, 10, 99, 100, 12345, 999999, 1000000, vk.U32_MAX, 7], dtype=np.uint32)
    blob, off = vk.decimal_blob(idx)
    assert [bytes(blob[off[i]:off[i + 1]]) for i in range(len(idx))] == [str(int(i)).encode() for i in idx]
    assert (blob[off[-1]:] == vk.TAIL_BYTE).all() and len(blob) == off[-1] + vk.BLOB_TAIL
    lc = vk.long_case(oracle)
    blob, off = vk.decimal_blob(lc.query)
    assert len(off) == vk.LONG_N + 1 > vk.GRID_LIMIT and 13e6 < len(blob) < 16e6
    for i in (0, 1, 77, vk.LONG_N - 1):
        assert bytes(blob[off[i]:off[i + 1]]) == str(int(lc.query[i])).encode()


def test_short_lists():
    lists = vk.short_lists()
    assert sorted(len(v) for v in lists.values()) == [1, 1, 255, 256, 257]
    assert lists["1-zero"].tolist() == [0] and lists["1-max"].tolist() == [vk.U32_MAX]
    for name in ("255", "256", "257"):
        lst = lists[name]
        assert lst.dtype == np.uint32 and 0 in lst and vk.U32_MAX in lst and set(vk.DIGIT_EDGES) <= set(lst.tolist())
        assert {len(str(int(i))) for i in lst} == set(range(1, 11))
        q = vk.short_queries(lst)
        assert set(lst.tolist()) <= set(q.tolist()) and len(set(q.tolist()) - set(lst.tolist())) >= 250
    assert {int(k) for k in vk.SHORT_K} == {0, 1, 2, 64} and 64.5 in vk.SHORT_K and 0.5 in vk.SHORT_K


def test_short_list_fills_and_both_references_agree(oracle):
    """The short lists' filters are full at the tiny m and nearly empty at the long ones (the count is fixed at <= 257); for k* <= 2.5 the
    fill is printed into the assertion.  The byte-per-bit reference and the position reference agree where both apply."""
    lst = vk.short_lists()["257"]
    q = vk.short_queries(lst)
    for m in (65, 1000003):
        for k in vk.SHORT_K:
            for seeds in vk.INDEX_SEEDS:
                packed, verdicts = vk.short_ref(oracle, m, k, seeds, lst, q)
                pos, verdicts2 = vk.short_ref_positions(oracle, m, k, seeds, lst, q)
                assert np.array_equal(vk.set_positions(packed), pos) and np.array_equal(verdicts, verdicts2), (m, k)
                if m == 1000003 and k <= 2.5:
                    assert len(pos) / m < 0.001 and 0 < verdicts.sum() < len(q), "sparse: yes for the list, no for (nearly) all others"
                    assert k < 1 or verdicts.sum() <= len(lst) + 2          # floor_k = 0: a key that is not activated has no probe to fail


# ------------------------------------------------------------------ D: keys
def test_key_set():
    keys, others = vk.key_sets()
    assert len(keys) == 3 * 132 and sorted({len(k) for k in keys}) == list(range(132))
    for n in range(1, 132):
        ks = [k for k in keys if len(k) == n]
        assert len(ks) == 3 and {k[0] for k in ks} >= {0x00, 0xFF}
        if n > 1:
            assert {k[-1] for k in ks} >= {0x00, 0xFF}
    assert len({b for k in keys for b in k}) == 256, "bytes of all 256 values"
    empties = [i for i, k in enumerate(keys) if not k]
    assert empties and 0 not in empties and len(keys) - 1 not in empties
    assert any(len(keys[i - 1]) and len(keys[i + 1]) for i in empties), "an empty key between two others"
    blob, off = vk.key_blob(keys)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8)), "keys start at every alignment"
    assert (blob[off[-1]:] == vk.TAIL_BYTE).all() and len(blob) - off[-1] == vk.BLOB_TAIL
    assert len(others) == len(keys) and not set(others) & set(keys) and max(len(k) for k in others) == 135
    q, inserted = vk.key_queries(keys, others)
    assert inserted.sum() == len(keys) and len(q) == len(keys) + len(others)


def test_key_filter_fills_and_verdicts(oracle):
    keys, others = vk.key_sets()
    q, inserted = vk.key_queries(keys, others)
    fills = {}
    for m in vk.KEY_M:
        for seeds in vk.KEY_SEEDS:
            bits, verdicts = vk.rational_key_ref(oracle, m, vk.KEY_K, seeds, keys, q)
            fills[m] = fill(bits)
            assert verdicts[inserted].all()
            if m == vk.KEY_M_LARGE:
                assert (verdicts[~inserted] == 0).mean() > 0.5
            if m == 2003:
                assert 0.20 < fills[m] < 0.60, fills[m]
                assert 0 < verdicts[~inserted].mean() < 1, "both answers among the keys that were not inserted"
    assert fills[1000003] < 0.002 and fills[vk.KEY_M_LARGE] < 0.0001, "396 keys: the count is fixed by the lengths to cover"


def test_references_agree_with_the_pure_python_xxh64(oracle):
    keys, others = vk.key_sets()
    seeds = sorted({s for t in vk.KEY_SEEDS + vk.INDEX_SEEDS for s in t} | set(range(0, 64, 9)))
    sample = keys[::5] + others[::17]
    assert {len(k) for k in sample} >= {0, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128} or len({len(k) for k in sample}) > 60
    for k in sample:
        for s in seeds:
            assert oracle.xxh64(k, s) == pyref.xxh64(k, s), (len(k), s)
    for i in (0, 9, 10, 12345678, vk.U32_MAX):
        for s in vk.SEEDS_WIDE:
            assert oracle.hash_index(i, s) == pyref.xxh64(str(i).encode(), s)
    # a whole small filter, built without the C oracle
    m, s = 2003, vk.KEY_SEEDS[2]
    bits, _ = vk.rational_key_ref(oracle, m, vk.KEY_K, s, keys[:60], [])
    want = np.zeros(m, dtype=np.uint8)
    for k in keys[:60]:
        h1, h2 = pyref.xxh64(k, s[0]), pyref.xxh64(k, s[1])
        cnt = 2 + (1 if pyref.xxh64(k, s[2]) / ((1 << 64) - 1) < vk.KEY_K - 2 else 0)
        for j in range(cnt):
            want[(h1 + j * h2) % m] = 1
    assert np.array_equal(bits, want)
    std, _ = vk.standard_key_ref(oracle, m, 7, keys[:60], [])
    want = np.zeros(m, dtype=np.uint8)
    for k in keys[:60]:
        for j in range(7):
            want[pyref.xxh64(k, j) % m] = 1
    assert np.array_equal(std, want)
