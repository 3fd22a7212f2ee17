"""The changed-value kernels and the per-index / string-key filter surface against plain references, where the rest of the suite reaches
them only through a few fixtures or compares them with themselves (tests/value_key_ref.py holds the cases and the references,
tests/test_value_key_ref_cpu.py proves them non-vacuous):

  A  rbf_gather_values / rbf_scatter_values (k_mask_segment_counts, k_scan_segments, k_values): u8 / u16 x C = 1..4 x flat, padded rows,
     padded pixels x seven masks on 131x67; 1031x1021, where the segment scan carries into a second round; the error paths;
  B  rbf_gather_values_batch (k_frame_offsets, k_gather_words, k_uncovered_changes): the same types and layouts on five frames, every
     capacity cut, 300 pairs in one call, the large shape, no uncovered counts;
  C  rbf_filter_insert_indices / rbf_filter_query_indices: a list longer than the 8192 x 256 threads of one trip, short lists around one
     workgroup at filter lengths 1 .. 2^30 + 1 with floor_k 0 .. 64 and seeds past 32 bits; the error paths;
  D  rbf_filter_insert_keys / rbf_filter_query_keys and the device's full XXH64: raw byte keys of every length 0..131 at every alignment
     under three seed triples, the standard filter up to 64 hashes, and the decimal keys that must rebuild C's long filter bit for bit.

Everything is byte-exact.  Every buffer the device could write is pre-filled with 0xEE, has 64 bytes of slack and is compared WHOLE: the
legal region against the reference, the rest against the sentinel; the buffers the device only reads are compared with what was uploaded.
The C ABI is called directly: engine.py's helpers pass flat layouts and str(x) keys only."""
import ctypes

import numpy as np
import pytest

import value_key_ref as vk
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import params as P

pytestmark = pytest.mark.gpu

PEAK = {"live": 0, "largest": 0}


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()
    print("\nvalue/key sweep: peak of the test's own device buffers %.1f MiB, largest single one %.1f MiB"
          % (PEAK["live"] / 2.0 ** 20, PEAK["largest"] / 2.0 ** 20))


class Buf:
    """A device buffer of `nbytes` legal bytes and SLACK more, all of it SENTINEL until something is uploaded."""

    def __init__(self, ctx, nbytes, host=None):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.dev = ctx.alloc(self.nbytes + vk.SLACK)
        live = sum(b.nbytes for b in ctx._buffers)
        PEAK["live"], PEAK["largest"] = max(PEAK["live"], live), max(PEAK["largest"], self.dev.nbytes)
        self.ptr = self.dev.ptr
        self.reset(host)

    def reset(self, host=None):
        nat.check(nat.lib().rbf_memset(self.ctx.handle, self.ptr, vk.SENTINEL, self.dev.nbytes))
        self.host = None
        if host is not None:
            self.host = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
            assert self.host.nbytes <= self.nbytes
            if self.host.nbytes:
                self.dev.upload(self.host)
        return self

    def zero(self, nbytes):
        if nbytes:
            nat.check(nat.lib().rbf_memset(self.ctx.handle, self.ptr, 0, int(nbytes)))

    def read(self, legal, what=""):
        """The first `legal` bytes; everything behind them must still be the sentinel."""
        raw = self.dev.download()
        assert (raw[legal:] == vk.SENTINEL).all(), "%s: bytes behind the legal region are written" % what
        return raw[:legal]

    def unchanged(self, what=""):
        """A buffer the device only reads holds what was uploaded (and the sentinel behind it)."""
        got = self.read(self.host.nbytes, what)
        assert np.array_equal(got, self.host), "%s: an input buffer is written" % what

    def free(self):
        self.dev.free()


def same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %d (got 0x%02x, want 0x%02x)"
                             % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def ok(rc, what=""):
    assert rc == nat.RBF_OK, (what, rc, nat.lib().rbf_last_error())


# ------------------------------------------------------------------ A: gather and scatter
def gather(ctx, lay, fb, mb, vb, cb, channels=None, pixel_stride=None, row_pitch=None, count=True):
    return nat.lib().rbf_gather_values(ctx.handle, fb.ptr, lay.W, lay.H, lay.row_pitch if row_pitch is None else row_pitch,
                                       lay.pixel_stride if pixel_stride is None else pixel_stride, lay.sb,
                                       lay.C if channels is None else channels, mb.ptr, vb.ptr, cb.ptr if count else None)


def scatter(ctx, lay, fb, mb, vb, channels=None, pixel_stride=None, row_pitch=None):
    return nat.lib().rbf_scatter_values(ctx.handle, fb.ptr, lay.W, lay.H, lay.row_pitch if row_pitch is None else row_pitch,
                                        lay.pixel_stride if pixel_stride is None else pixel_stride, lay.sb,
                                        lay.C if channels is None else channels, mb.ptr, vb.ptr)


def gather_scatter_cases(ctx, lay, frame, masks, seed):
    n = lay.n
    fb, mb = Buf(ctx, lay.nbytes), Buf(ctx, vk.packed_stride(n) + vk.ROW_GAP)
    vb, cb = Buf(ctx, n * lay.C * lay.sb), Buf(ctx, 8)
    try:
        for name, mask in masks.items():
            what = "%s %s" % (lay.kind, name)
            blk, _ = vk.mask_block([mask], n)
            want = vk.gather_ref(frame, lay, mask)
            fb.reset(frame), mb.reset(blk), vb.reset(), cb.reset()
            ok(gather(ctx, lay, fb, mb, vb, cb), what)
            assert int(cb.read(8, what).view(np.uint64)[0]) == int(mask.sum()), what
            same(vb.read(want.nbytes, what + " gather"), want, what + " gather")
            fb.unchanged(what), mb.unchanged(what)
            # the way back: other values into the same pixels
            vals = vk.scatter_values(frame, lay, mask, seed)
            assert (vals != want).all()
            vb.reset(vals)
            ok(scatter(ctx, lay, fb, mb, vb), what)
            same(fb.read(lay.nbytes, what + " scatter"), vk.scatter_ref(frame, lay, mask, vals), what + " scatter")
            vb.unchanged(what), mb.unchanged(what)
    finally:
        for b in (fb, mb, vb, cb):
            b.free()


@pytest.mark.parametrize("dtype,C,kind", vk.VALUE_CASES, ids=vk.VALUE_IDS)
def test_gather_and_scatter_in_every_layout(ctx, dtype, C, kind):
    lay = vk.layout(kind, dtype, C)
    gather_scatter_cases(ctx, lay, vk.frame_bytes(lay, 4001), vk.mask_set(lay.n, 4000), 4002)


def test_gather_and_scatter_past_one_round_of_the_segment_scan(ctx):
    """1028 segments: the scan of the segment counts carries its first 1024 into the second round."""
    lay = vk.layout("flat", np.uint8, 1, vk.BIG_H, vk.BIG_W)
    gather_scatter_cases(ctx, lay, vk.frame_bytes(lay, 4201), vk.big_masks(lay.n, 4200), 4202)


def test_gather_and_scatter_error_paths_touch_nothing(ctx):
    lay = vk.layout("rows", np.uint16, 3)
    frame, mask = vk.frame_bytes(lay, 4001), vk.mask_set(lay.n, 4000)["p07"]
    blk, _ = vk.mask_block([mask], lay.n)
    vals = vk.scatter_values(frame, lay, mask, 4002)
    fb, mb, vb, cb = Buf(ctx, lay.nbytes, frame), Buf(ctx, len(blk), blk), Buf(ctx, vals.nbytes), Buf(ctx, 8)
    bad = [dict(channels=0), dict(channels=5), dict(pixel_stride=lay.C * lay.sb - lay.sb), dict(row_pitch=lay.W * lay.pixel_stride - 2)]
    try:
        for kw in bad:
            assert gather(ctx, lay, fb, mb, vb, cb, **kw) == nat.RBF_EINVAL, kw
        assert gather(ctx, lay, fb, mb, vb, cb, count=False) == nat.RBF_EINVAL
        ctx.sync()
        assert len(vb.read(0)) == 0 and len(cb.read(0)) == 0, "neither output is written"
        fb.unchanged(), mb.unchanged()
        vb.reset(vals)
        for kw in bad:
            assert scatter(ctx, lay, fb, mb, vb, **kw) == nat.RBF_EINVAL, kw
        ctx.sync()
        fb.unchanged(), mb.unchanged(), vb.unchanged()
    finally:
        for b in (fb, mb, vb, cb):
            b.free()


# ------------------------------------------------------------------ B: the batch gather
def run_batch(ctx, clip, ref, capacity=None, uncovered=True, what=""):
    lay, pairs = clip.lay, clip.F - 1
    total = int(ref.offsets[-1])
    cap = total if capacity is None else capacity
    blk, mstride = vk.mask_block(clip.masks, lay.n)
    fb, mb = Buf(ctx, len(clip.block), clip.block), Buf(ctx, len(blk), blk)
    vb, ob, ub = Buf(ctx, ref.values.nbytes), Buf(ctx, 8 * clip.F), Buf(ctx, 8 * pairs)
    try:
        ok(nat.lib().rbf_gather_values_batch(ctx.handle, fb.ptr, clip.frame_stride, clip.F, lay.W, lay.H, lay.row_pitch, lay.pixel_stride,
                                             lay.sb, lay.C, mb.ptr, mstride, vb.ptr, cap, ob.ptr, ub.ptr if uncovered else None), what)
        keep = min(cap, total) * lay.C * lay.sb
        same(vb.read(keep, what + " values"), ref.values.view(np.uint8)[:keep], what + " values")
        assert ob.read(8 * clip.F, what).view(np.uint64).tolist() == ref.offsets.tolist(), what + ": the offsets are the full ones"
        if uncovered:
            assert ub.read(8 * pairs, what).view(np.uint64).tolist() == ref.uncovered.tolist(), what
        else:
            assert len(ub.read(0, what)) == 0
        fb.unchanged(what), mb.unchanged(what)
    finally:
        for b in (fb, mb, vb, ob, ub):
            b.free()


@pytest.mark.parametrize("dtype,C,kind", vk.BATCH_CASES, ids=vk.BATCH_IDS)
def test_batch_gather_in_every_layout(ctx, dtype, C, kind):
    clip = vk.sweep_clip(dtype, C, kind)
    ref = vk.batch_ref(clip)
    assert ref.uncovered[3] == vk.CHROMA_PIXELS and ref.uncovered[2] == 0
    run_batch(ctx, clip, ref, what=kind)


def test_batch_gather_capacity_cuts_and_no_uncovered_counts(ctx):
    clip = vk.sweep_clip(*vk.CAPACITY_CASE)
    ref = vk.batch_ref(clip)
    for name, cap in vk.capacities(ref.offsets).items():
        run_batch(ctx, clip, ref, capacity=cap, what="capacity " + name)
    run_batch(ctx, clip, ref, uncovered=False, what="no uncovered counts")


def test_batch_gather_300_pairs(ctx):
    clip = vk.small_clip()
    run_batch(ctx, clip, vk.batch_ref(clip), what="300 pairs")


def test_batch_gather_past_one_round_of_the_segment_scan(ctx):
    clip = vk.big_clip()
    run_batch(ctx, clip, vk.batch_ref(clip), what="1031x1021")


# ------------------------------------------------------------------ C, D: the filter calls
def device_params(m, k_star=1.0, floor_k=None):
    fp = nat.params_array([P.filter_params(k_star, m)])
    if floor_k is not None:
        fp[0].floor_k = floor_k
    return fp


def device_seeds(seeds):
    return nat.Seeds(*[int(s) for s in seeds])


class Filter:
    """A device filter of m bits (whole 32-bit words, zero or `preload`) in front of its slack."""

    def __init__(self, ctx, m):
        self.m, self.legal = m, vk.filter_bytes(m)
        self.buf = Buf(ctx, self.legal)

    def clear(self, preload=None):
        self.buf.reset(preload)
        if preload is None:
            self.buf.zero(self.legal)
        return self

    def read(self, what=""):
        return self.buf.read(self.legal, what)

    @property
    def ptr(self):
        return self.buf.ptr

    def free(self):
        self.buf.free()


def insert_indices(ctx, f, fp, sd, ib, count):
    return nat.lib().rbf_filter_insert_indices(ctx.handle, f.ptr, fp, ctypes.byref(sd), ib.ptr if ib else None, count)


def query_indices(ctx, f, fp, sd, ib, count, ob):
    return nat.lib().rbf_filter_query_indices(ctx.handle, f.ptr, fp, ctypes.byref(sd), ib.ptr if ib else None, count, ob.ptr if ob else None)


@pytest.fixture(scope="module")
def long_case(oracle):
    return vk.long_case(oracle)


def test_index_lists_longer_than_one_trip_of_the_grid(ctx, long_case):
    lc = long_case
    assert len(lc.query) > vk.GRID_LIMIT and not lc.filt[lc.extra].any()
    fp, sd = device_params(vk.LONG_M, vk.LONG_K), device_seeds(vk.SEEDS_VIDEO)
    preload = np.zeros(vk.LONG_M, dtype=np.uint8)
    preload[lc.extra] = 1
    f = Filter(ctx, vk.LONG_M).clear(vk.pack_filter(preload))
    ib, qb, ob = Buf(ctx, lc.insert.nbytes, lc.insert), Buf(ctx, lc.query.nbytes, lc.query), Buf(ctx, len(lc.query))
    try:
        ok(insert_indices(ctx, f, fp, sd, ib, len(lc.insert)))
        same(f.read("insert"), vk.pack_filter(lc.filt_or), "the filter is the oracle's OR the bits it held")
        ok(query_indices(ctx, f, fp, sd, qb, len(lc.query), ob))
        same(ob.read(len(lc.query), "query"), lc.verdicts_or[lc.query], "verdicts")
        same(f.read("query"), vk.pack_filter(lc.filt_or), "the query leaves the filter alone")
        ib.unchanged(), qb.unchanged()
    finally:
        for b in (f, ib, qb, ob):
            b.free()


def short_case(ctx, oracle, f, m, k, seeds, name, lst, bufs):
    what = "m=%d k*=%s seeds=%s list=%s" % (m, k, seeds[0], name)
    q = vk.short_queries(lst)
    fp, sd = device_params(m, k), device_seeds(seeds)
    assert fp[0].floor_k == int(k)
    ib, qb, ob = bufs
    ib.reset(lst), qb.reset(q), ob.reset()
    f.clear()
    ok(insert_indices(ctx, f, fp, sd, ib, len(lst)), what)
    got = f.read(what)
    ok(query_indices(ctx, f, fp, sd, qb, len(q), ob), what)
    verdicts = ob.read(len(q), what)
    if m <= vk.BYTE_PER_BIT_MAX:
        want, want_verdicts = vk.short_ref(oracle, m, k, seeds, lst, q)
        same(got, want, what + " filter")
    else:
        want, want_verdicts = vk.short_ref_positions(oracle, m, k, seeds, lst, q)
        assert np.array_equal(vk.set_positions(got), want), what + " set positions"
    same(verdicts, want_verdicts, what + " verdicts")
    ib.unchanged(what), qb.unchanged(what)


@pytest.mark.parametrize("m", vk.SHORT_M)
def test_short_index_lists(ctx, oracle, m):
    """Counts on both sides of one workgroup x every k* x both seed triples.  Past 2^24 bits the filter is compared by its set positions,
    and -- a 128 MiB download each -- the list of 257 runs with every k* and seed triple, the other lists with k* = 2.3 and the video seeds:
    the count only sizes the grid, which does not depend on m."""
    lists = vk.short_lists()
    f = Filter(ctx, m)
    bufs = (Buf(ctx, 4 * 257), Buf(ctx, 4 * 700), Buf(ctx, 700))
    try:
        for name, lst in lists.items():
            for k in vk.SHORT_K:
                for seeds in vk.INDEX_SEEDS:
                    if m > vk.BYTE_PER_BIT_MAX and name != "257" and (k, seeds) != (2.3, vk.SEEDS_VIDEO):
                        continue
                    short_case(ctx, oracle, f, m, k, seeds, name, lst, bufs)
    finally:
        for b in (f,) + bufs:
            b.free()


def test_index_error_paths(ctx):
    m = 1000003
    f = Filter(ctx, m).clear()
    lst = vk.short_lists()["255"]
    ib, ob = Buf(ctx, lst.nbytes, lst), Buf(ctx, len(lst))
    sd = device_seeds(vk.SEEDS_VIDEO)
    try:
        assert insert_indices(ctx, f, device_params(m, floor_k=65), sd, ib, len(lst)) == nat.RBF_ERANGE
        assert query_indices(ctx, f, device_params(m, floor_k=65), sd, ib, len(lst), ob) == nat.RBF_ERANGE
        zero = device_params(1)
        zero[0].m = 0
        assert insert_indices(ctx, f, zero, sd, ib, len(lst)) == nat.RBF_EINVAL
        assert query_indices(ctx, f, zero, sd, ib, len(lst), ob) == nat.RBF_EINVAL
        ok(insert_indices(ctx, f, device_params(m, 2.3), sd, None, 0))
        ok(query_indices(ctx, f, device_params(m, 2.3), sd, None, 0, None))
        ctx.sync()
        assert not f.read().any() and len(ob.read(0)) == 0
        ib.unchanged()
    finally:
        for b in (f, ib, ob):
            b.free()


# ---- D
def insert_keys(ctx, f, fp, sd, standard_k, kb, fb, count):
    return nat.lib().rbf_filter_insert_keys(ctx.handle, f.ptr, fp, ctypes.byref(sd), standard_k, kb.ptr, fb.ptr, count)


def query_keys(ctx, f, fp, sd, standard_k, kb, fb, count, ob):
    return nat.lib().rbf_filter_query_keys(ctx.handle, f.ptr, fp, ctypes.byref(sd), standard_k, kb.ptr, fb.ptr, count, ob.ptr)


class KeyBuffers:
    """The inserted keys and the queried ones (the inserted and as many others, shuffled) on the device."""

    def __init__(self, ctx):
        self.keys, others = vk.key_sets()
        self.queries, self.inserted = vk.key_queries(self.keys, others)
        blob, off = vk.key_blob(self.keys)
        qblob, qoff = vk.key_blob(self.queries)
        self.bufs = [Buf(ctx, len(blob), blob), Buf(ctx, off.nbytes, off), Buf(ctx, len(qblob), qblob), Buf(ctx, qoff.nbytes, qoff),
                     Buf(ctx, len(self.queries))]

    def run(self, ctx, f, fp, sd, standard_k, what):
        kb, kf, qb, qf, ob = self.bufs
        ob.reset()
        f.clear()
        ok(insert_keys(ctx, f, fp, sd, standard_k, kb, kf, len(self.keys)), what)
        filt = f.read(what)
        ok(query_keys(ctx, f, fp, sd, standard_k, qb, qf, len(self.queries), ob), what)
        verdicts = ob.read(len(self.queries), what)
        for b in self.bufs[:4]:
            b.unchanged(what)
        return filt, verdicts

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.fixture(scope="module")
def key_buffers(ctx):
    kb = KeyBuffers(ctx)
    yield kb
    kb.free()


@pytest.mark.parametrize("m", vk.KEY_M)
def test_byte_keys_of_every_length_rational(ctx, oracle, key_buffers, m):
    kb = key_buffers
    f = Filter(ctx, m)
    try:
        for seeds in vk.KEY_SEEDS:
            what = "m=%d seeds=%s" % (m, seeds)
            bits, want_verdicts = vk.rational_key_ref(oracle, m, vk.KEY_K, seeds, kb.keys, kb.queries)
            assert want_verdicts[kb.inserted].all()
            if m == vk.KEY_M_LARGE:
                assert (want_verdicts[~kb.inserted] == 0).mean() > 0.5
            filt, verdicts = kb.run(ctx, f, device_params(m, vk.KEY_K), device_seeds(seeds), 0, what)
            same(filt, vk.pack_filter(bits), what + " filter")
            same(verdicts, want_verdicts, what + " verdicts")
    finally:
        f.free()


@pytest.mark.parametrize("m", (2003, 1000003))
def test_byte_keys_of_every_length_standard(ctx, oracle, key_buffers, m):
    kb = key_buffers
    f = Filter(ctx, m)
    sd = device_seeds((77, 78, 79))                 # unused by the standard filter: its seeds are 0 .. k-1
    try:
        for k in vk.STANDARD_K:
            what = "m=%d standard_k=%d" % (m, k)
            bits, want_verdicts = vk.standard_key_ref(oracle, m, k, kb.keys, kb.queries)
            filt, verdicts = kb.run(ctx, f, device_params(m), sd, k, what)
            same(filt, vk.pack_filter(bits), what + " filter")
            same(verdicts, want_verdicts, what + " verdicts")
        f.clear()
        kbuf, kf, qb, qf, ob = kb.bufs
        ob.reset()
        assert insert_keys(ctx, f, device_params(m), sd, 65, kbuf, kf, len(kb.keys)) == nat.RBF_ERANGE
        assert query_keys(ctx, f, device_params(m), sd, 65, qb, qf, len(kb.queries), ob) == nat.RBF_ERANGE
        ctx.sync()
        assert not f.read().any() and len(ob.read(0)) == 0
    finally:
        f.free()


def test_decimal_keys_rebuild_the_index_filter(ctx, long_case):
    """str(i) through the string surface == i through the index surface: the same filter bit for bit, the same verdict for every
    position -- and more keys than one trip of k_keys' grid covers."""
    lc = long_case
    blob, off = vk.decimal_blob(lc.insert)
    qblob, qoff = vk.decimal_blob(lc.query)
    assert len(qoff) - 1 > vk.GRID_LIMIT
    fp, sd = device_params(vk.LONG_M, vk.LONG_K), device_seeds(vk.SEEDS_VIDEO)
    f = Filter(ctx, vk.LONG_M).clear()
    kb, kf = Buf(ctx, len(blob), blob), Buf(ctx, off.nbytes, off)
    qb, qf, ob = Buf(ctx, len(qblob), qblob), Buf(ctx, qoff.nbytes, qoff), Buf(ctx, len(lc.query))
    try:
        ok(insert_keys(ctx, f, fp, sd, 0, kb, kf, len(lc.insert)))
        same(f.read("insert"), vk.pack_filter(lc.filt), "the filter of the index surface")
        ok(query_keys(ctx, f, fp, sd, 0, qb, qf, len(lc.query), ob))
        same(ob.read(len(lc.query), "query"), lc.verdicts[lc.query], "verdicts")
        for b in (kb, kf, qb, qf):
            b.unchanged()
    finally:
        for b in (f, kb, kf, qb, qf, ob):
            b.free()
