"""The GOP mask stage (A1) on the device, bit for bit against tests/mask_stage.py's numpy reference: every instantiation of the fast kernels
on one-hot clips and value grids (a), temporal chunks and the packed count tally on clips whose every pair has another count (b), the
two-level ticket and the fused finish at the workgroup counts that take its branches apart (c), the handoff from the fast kernel to the
generic one and the layouts either takes (d).  Every output lies in a poisoned block between poisoned guards; nothing but the first
ceil(n / 64) * 8 bytes of a mask row and ones[0 .. pairs) may change.  tests/test_mask_stage_cpu.py shows that these cases tell a wrong
kernel from a right one."""
import ctypes

import numpy as np
import pytest

import mask_stage as ms
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import params as P

pytestmark = pytest.mark.gpu

PLAIN = ms.Placement(0, 0, 0, 0, 0)
_REF = {}


def ref(key, frames, thr, mc, run_starts=None):
    """ref_masks, computed once per named case and shared by the knobs and placements that run it."""
    if key not in _REF:
        _REF[key] = ms.ref_masks(frames, None, thr, mc, run_starts)
    return _REF[key]


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.force_generic(0)
    c.close()


class Resident:
    """A clip on the device under a placement, and poisoned blocks for what the mask stage writes."""

    def __init__(self, ctx, samples, W, H, pl=PLAIN, ones_base=0):
        self.ctx, self.W, self.H, self.pl = ctx, W, H, pl
        self.F, self.n, C = samples.shape
        assert self.n == W * H
        self.sb = samples.dtype.itemsize
        raw, self.fstride, self.pitch, self.ps = ms.place(samples, W, H, pl)
        self.used = ms.packed_stride(self.n)
        self.mblock = ms.Block(self.F - 1, self.used + pl.mask_extra)
        self.oblock = ms.Block(1, (self.F - 1) * 8, ones_base)
        self.bufs = [ctx.alloc(raw.nbytes + 16), ctx.alloc(self.mblock.nbytes), ctx.alloc(self.oblock.nbytes)]
        self.bufs[0].upload(raw)
        self.frames_ptr = self.bufs[0].ptr + pl.base

    def outputs(self):
        """Poison both blocks; (masks_dev, ones_dev)."""
        return self.mblock.place(self.bufs[1]), self.oblock.place(self.bufs[2])

    def mask_args(self, thr, table):
        tab = (ctypes.c_int32 * (self.F - 1))(*table) if table is not None else None
        m, o = self.outputs()
        return (self.ctx.handle, self.frames_ptr, self.fstride, self.F, self.W, self.H, self.pitch, self.ps, self.sb, int(thr), tab, m, self.mblock.stride, o)

    def mask(self, thr=0, table=None, mc=1):
        rc = nat.lib().rbf_residual_mask_batch_ex(*self.mask_args(thr, table), mc)
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
        return self.fetch()

    def fetch(self):
        """(rows [pairs, used], ones [pairs]) after the stream has drained; the poison around them is held here."""
        self.ctx.sync()
        mraw, oraw = self.bufs[1].download(self.mblock.nbytes), self.bufs[2].download(self.oblock.nbytes)
        assert self.mblock.untouched(mraw, self.used), "the mask stage wrote outside the first ceil(n / 64) * 8 bytes of a mask row"
        assert self.oblock.untouched(oraw, (self.F - 1) * 8), "the mask stage wrote outside ones[0 .. pairs)"
        return self.mblock.rows(mraw)[:, :self.used].copy(), self.oblock.rows(oraw)[0].view("<u8").astype(np.int64)

    def untouched_everywhere(self):
        self.ctx.sync()
        mraw, oraw = self.bufs[1].download(self.mblock.nbytes), self.bufs[2].download(self.oblock.nbytes)
        return bool((mraw == ms.POISON).all() and (oraw == ms.POISON).all())

    def close(self):
        for b in self.bufs:
            b.free()


def held(got, want, tag):
    rows, ones = got
    wrows, wones = want
    bad = [f for f in range(len(wones)) if not np.array_equal(rows[f], wrows[f])]
    assert not bad, (tag, "mask rows", bad[:8])
    assert ones.tolist() == [int(v) for v in wones], (tag, "ones", [(f, int(a), int(b)) for f, (a, b) in enumerate(zip(ones, wones)) if a != b][:8])


# ------------------------------------------------------------------ (a) one-hot clips and value grids
KERNEL_KNOBS = [(k, knob) for k in ms.KERNELS for knob in ms.knobs_of(k)]      # (knob bit 2 selects nothing in the all-channel kernels)


@pytest.mark.parametrize("kernel,knob", KERNEL_KNOBS, ids=["%s-%s" % (k.name, ms.KNOB_IDS[ms.KNOBS.index(knob)]) for k, knob in KERNEL_KNOBS])
def test_one_hot_clips_and_value_grids(ctx, kernel, knob):
    mc = kernel.mask_channels
    ctx.force_generic(knob)
    try:
        for x in ms.XORS:
            frames = ms.one_hot_clip(kernel.sample_bytes, kernel.pixel_bytes, x)
            r = Resident(ctx, frames, 64, 32)
            want = ref((kernel.name, "one_hot", x), frames, 0, mc)
            held(r.mask(0, None, mc), want, (kernel.name, knob, "one_hot", hex(x)))
            if mc == 1:                                           # thresholds from a table: no THR0 shortcut
                held(r.mask(0, [0] * (r.F - 1), mc), want, (kernel.name, knob, "one_hot table", hex(x)))
            r.close()
        grid = ms.grid_clip(kernel)
        W, H = (256, 256) if kernel.sample_bytes == 1 else (128, 128)
        r = Resident(ctx, grid, W, H)
        for thr in ms.thresholds_of(kernel):
            held(r.mask(thr, None, mc), ref((kernel.name, "grid", thr), grid, thr, mc), (kernel.name, knob, "grid", thr))
        r.close()
        if mc == 1:
            # a different threshold per pair; the table takes no negative entry, so it runs the others of the list
            tab = [t for t in ms.thresholds_of(kernel) if t >= 0]
            clip = ms.grid_clip(kernel, 0, len(tab))
            r = Resident(ctx, clip, W, H)
            held(r.mask(0, tab, 1), ref((kernel.name, "grid table"), clip, tab, 1), (kernel.name, knob, "grid table"))
            held(r.mask(5, tab[::-1], 1), ref((kernel.name, "grid table reversed"), clip, tab[::-1], 1), (kernel.name, knob, "grid table reversed"))
            rc = nat.lib().rbf_residual_mask_batch_ex(*r.mask_args(0, [-1] + tab[1:]), 1)
            assert rc == nat.RBF_EINVAL and r.untouched_everywhere()
            r.close()
    finally:
        ctx.force_generic(0)


# ------------------------------------------------------------------ (b) chunks and the count tally
def chunk_runs(ctx, r, frames, kernel, P, counts, tag):
    mc = kernel.mask_channels
    want = ref((kernel.name, "count", P, r.n), frames, 0, mc)
    assert want[1].tolist() == counts
    for c in ms.CHUNK_KNOBS:
        ctx.force_generic(c << 8)
        held(r.mask(0, None, mc), want, tag + (c, "plain"))
        if mc == 1:
            held(r.mask(0, ms.count_thresholds(P), 1), want, tag + (c, "table"))
            held(r.mask(63, None, 1), want, tag + (c, "thr 63"))


@pytest.mark.parametrize("P", ms.CHUNK_PAIRS, ids=lambda p: "pairs%d" % p)
@pytest.mark.parametrize("kernel", ms.CHUNK_KERNELS, ids=[k.name for k in ms.CHUNK_KERNELS])
def test_chunks_and_counts_on_count_clips(ctx, kernel, P):
    frames, counts = ms.count_clip(P, kernel, 4096)
    r = Resident(ctx, frames, 64, 64)
    try:
        chunk_runs(ctx, r, frames, kernel, P, counts, (kernel.name, P))
    finally:
        ctx.force_generic(0)
        r.close()


class Gop:
    """The buffers of rbf_encode_runs_begin_ex + rbf_encode_gop_finish around a Resident clip: filters, witnesses, poisoned stats."""

    def __init__(self, ctx, r, stats_base=0):
        self.ctx, self.r = ctx, r
        self.pairs = r.F - 1
        L = nat.lib()
        self.fstride, self.wstride = int(L.rbf_filter_stride_min(r.n)), nat.packed_stride(r.n)
        self.sblock = ms.Block(1, self.pairs * 8 * nat.STATS_PER_FRAME, stats_base)
        self.bufs = [ctx.alloc(self.fstride * self.pairs + 64), ctx.alloc(self.wstride * self.pairs + 64), ctx.alloc(self.sblock.nbytes)]
        self.seeds = nat.Seeds(*P.SEEDS_VIDEO)
        self.params, self.k = (nat.FilterParams * self.pairs)(), (ctypes.c_double * self.pairs)()

    def prepare(self, thr=0, table=None, run_starts=None, mc=1):
        """Poison ones, masks and stats (uploads wait for the stream); the arguments of the begin."""
        r = self.r
        starts = None
        if run_starts is not None:
            starts = (ctypes.c_uint8 * r.F)(*[1 if t in set(run_starts) else 0 for t in range(r.F)])
        a = r.mask_args(thr, table)
        return (*a[:11], starts, ctypes.byref(self.seeds), a[11], a[12], a[13], self.bufs[0].ptr, self.fstride, self.bufs[1].ptr, self.wstride,
                self.sblock.place(self.bufs[2]), mc)

    def begin(self, thr=0, table=None, run_starts=None, mc=1, args=None):
        rc = nat.lib().rbf_encode_runs_begin_ex(*(args or self.prepare(thr, table, run_starts, mc)))
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()

    def finish(self):
        ready = ctypes.c_int(-1)
        assert nat.lib().rbf_encode_gop_poll(self.ctx.handle, ctypes.byref(ready)) == nat.RBF_OK and ready.value in (0, 1)
        rc = nat.lib().rbf_encode_gop_finish(self.ctx.handle, self.params, self.k)
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()

    def check(self, want, run_starts, tag):
        """Masks and ones against the reference; params_out / k_out against rbf_plan_batch of the reference's counts -- the host got
        them; stats: all words of an m == 0 pair and of a skipped pair are 0."""
        r = self.r
        held(r.fetch(), want, tag)
        ones = (ctypes.c_uint64 * self.pairs)(*[int(v) for v in want[1]])
        wp, wk = (nat.FilterParams * self.pairs)(), (ctypes.c_double * self.pairs)()
        nat.check(nat.lib().rbf_plan_batch(r.n, ones, self.pairs, 1, wp, wk))
        skipped = set(ms.skipped_pairs(r.F, run_starts))
        sraw = self.bufs[2].download(self.sblock.nbytes)
        assert self.sblock.untouched(sraw, self.pairs * 8 * nat.STATS_PER_FRAME), (tag, "stats guards")
        stats = self.sblock.rows(sraw)[0].view("<u8").reshape(self.pairs, nat.STATS_PER_FRAME)
        for f in range(self.pairs):
            fk = nat.PAIR_SKIPPED if f in skipped else int(wp[f].floor_k)
            got = (int(self.params[f].m), int(self.params[f].floor_k), int(self.params[f].threshold), self.k[f])
            assert got == (int(wp[f].m), fk, int(wp[f].threshold), wk[f]), (tag, "params", f, got)
            if f in skipped:
                assert got[0] == 0 and want[1][f] == 0
            if got[0] == 0:
                assert not stats[f].any(), (tag, "stats of an m == 0 pair", f, stats[f].tolist())
        return stats

    def close(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("P", ms.CHUNK_PAIRS, ids=lambda p: "pairs%d" % p)
@pytest.mark.parametrize("kernel", ms.CHUNK_KERNELS, ids=[k.name for k in ms.CHUNK_KERNELS])
def test_chunks_of_runs_through_the_gop_entries(ctx, kernel, P):
    frames, counts = ms.count_clip(P, kernel, 1024)
    r = Resident(ctx, frames, 32, 32)
    g = Gop(ctx, r)
    mc = kernel.mask_channels
    try:
        for name, starts in ms.run_patterns(P + 1).items():
            want = ref((kernel.name, "runs", P, name), frames, 0, mc, starts)
            for c in ms.CHUNK_KNOBS:
                ctx.force_generic(c << 8)
                g.begin(0, None, starts if starts else None, mc)
                g.finish()
                g.check(want, starts, (kernel.name, P, name, c))
            if mc == 1 and starts:
                ctx.force_generic(0)
                g.begin(0, ms.count_thresholds(P), starts, 1)
                g.finish()
                g.check(want, starts, (kernel.name, P, name, "table"))
    finally:
        ctx.force_generic(0)
        g.close()
        r.close()


@pytest.mark.parametrize("pattern", sorted(ms.TABLE_PATTERNS))
@pytest.mark.parametrize("kernel", ms.CHUNK_KERNELS, ids=[k.name for k in ms.CHUNK_KERNELS])
def test_chunk_tables_at_the_limit(ctx, kernel, pattern):
    """255 and 256 entries fit the chunk table; 257 fall back to uniform chunks and skip through the thresholds."""
    F, starts, _ = ms.TABLE_PATTERNS[pattern]
    frames, counts = ms.count_clip(F - 1, kernel, 1024)
    r = Resident(ctx, frames, 32, 32)
    g = Gop(ctx, r)
    try:
        want = ref((kernel.name, pattern), frames, 0, kernel.mask_channels, starts)
        assert want[1].tolist() == [0 if f % 2 else c for f, c in enumerate(counts)]
        g.begin(0, None, starts, kernel.mask_channels)
        g.finish()
        g.check(want, starts, (kernel.name, pattern))
    finally:
        g.close()
        r.close()


# ------------------------------------------------------------------ (c) tickets and the fused finish
def gop_round(ctx, t, stats_base=0, separate=0, seed=0):
    """Begin one GOP of a ticket shape; returns what check needs after the finish."""
    frames = ms.ticket_clip(t, seed)
    r = Resident(ctx, frames, t.W, t.H)
    g = Gop(ctx, r, stats_base)
    ctx.force_generic(t.chunks << 8)
    ctx.option(nat.OPT_SEPARATE_FINISH, separate)
    g.begin()
    return frames, r, g


@pytest.mark.parametrize("t", ms.TICKETS, ids=ms.TICKET_IDS)
def test_tickets_and_fused_finish(ctx, t):
    frames = ms.ticket_clip(t)
    want = ref(("ticket", t), frames, 0, 1)
    try:
        for separate in (0, 1):
            _, r, g = gop_round(ctx, t, separate=separate)
            g.finish()
            stats = g.check(want, None, (t, "separate" if separate else "fused"))
            assert any(int(p.m) for p in g.params) and stats.any()             # some pair is coded: its stats arrive behind the clear
            g.close()
            r.close()
    finally:
        ctx.force_generic(0)
        ctx.option(nat.OPT_SEPARATE_FINISH, 0)


def test_back_to_back_rounds_leave_tickets_and_accumulator_at_zero(ctx):
    """Three GOPs of different workgroup counts on one context with no rbf_ctx_sync between them, then a plain mask batch that counts into
    the same accumulator: tickets or counts left behind by one launch show in the next one's ones."""
    rounds = []
    try:
        shapes = [ms.TICKETS[i] for i in ms.SEQUENCE]
        clips = [(ms.ticket_clip(t, 1), t) for t in shapes]
        last = ms.count_clip(9, ms.KERNELS[0], 4096)[0]
        tail = Resident(ctx, last, 64, 64)
        tail_args = tail.mask_args(0, None)
        for frames, t in clips:
            r = Resident(ctx, frames, t.W, t.H)
            g = Gop(ctx, r)
            rounds.append((frames, t, r, g, g.prepare()))
        ctx.option(nat.OPT_SEPARATE_FINISH, 0)
        for frames, t, r, g, args in rounds:                      # uploads and allocations are done: from here on nothing waits for the stream
            ctx.force_generic(t.chunks << 8)
            g.begin(args=args)
            g.finish()
        ctx.force_generic(0)
        assert nat.lib().rbf_residual_mask_batch(*tail_args) == nat.RBF_OK
        for frames, t, r, g, _ in rounds:
            g.check(ref(("ticket sequence", t), frames, 0, 1), None, ("sequence", t))
        held(tail.fetch(), ref(("ticket sequence tail",), last, 0, 1), "mask batch behind the sequence")
        tail.close()
    finally:
        ctx.force_generic(0)
        for _, _, r, g, _ in rounds:
            g.close()
            r.close()


@pytest.mark.parametrize("case", ["stats_at_8_mod_16", "ragged_frame"])
def test_fallbacks_of_the_fused_finish_give_the_same(ctx, case):
    """A clear region that is not 16-byte aligned, a frame with a tail behind its whole segments: the finish is its own launch, silently."""
    t = ms.Ticket(208, 256, 6, 5, 65, False) if case == "stats_at_8_mod_16" else ms.Ticket(209, 256, 6, 5, None, False)
    frames = ms.ticket_clip(t._replace(nwg=65))
    try:
        r = Resident(ctx, frames, t.W, t.H)
        g = Gop(ctx, r, 8 if case == "stats_at_8_mod_16" else 0)
        ctx.force_generic(t.chunks << 8)
        g.begin()
        g.finish()
        stats = g.check(ref(("fallback", case), frames, 0, 1), None, case)
        assert stats.any()
        g.close()
        r.close()
    finally:
        ctx.force_generic(0)


# ------------------------------------------------------------------ (d) handoff and layouts
@pytest.mark.parametrize("kernel", ms.KERNELS, ids=ms.KERNEL_IDS)
def test_handoff_and_layouts(ctx, kernel):
    mc = kernel.mask_channels
    paths = set()
    for W, H in ms.HANDOFF_SIZES:
        n = W * H
        frames = ms.handoff_clip(kernel, n)
        for pl in ms.placements(kernel):
            r = Resident(ctx, frames, W, H, pl, ones_base=8 if pl.base else 0)
            for thr in ([0, 2] if mc == 1 else [0]):
                held(r.mask(thr, None, mc), ref((kernel.name, "handoff", n, thr), frames, thr, mc), (kernel.name, W, H, pl, thr))
            paths.add((ms.takes_fast_path(kernel, pl, n, r.F - 1), n % ms.SEG != 0))
            r.close()
    assert paths == {(True, True), (True, False), (False, True), (False, False)}      # fast alone, fast + tail, generic alone at both kinds of size


@pytest.mark.parametrize("pairs", [12288, 12289])
def test_lds_boundary_of_the_pair_counters(ctx, pairs):
    """12288 pairs x 4 bytes are the 48 KiB of counters the fast kernel may take; one more pair goes to the generic kernel."""
    rng = np.random.default_rng(pairs)
    n = 1024
    steps = (rng.random((pairs, n)) < 0.25).astype(np.uint8) * rng.integers(1, 256, (pairs, n), dtype=np.uint8)
    frames = np.empty((pairs + 1, n), np.uint8)
    frames[0] = rng.integers(0, 256, n, dtype=np.uint8)
    frames[1:] = np.bitwise_xor.accumulate(steps, axis=0) ^ frames[0]
    bits = frames[1:] != frames[:-1]
    assert ms.takes_fast_path(ms.KERNELS[0], PLAIN, n, pairs) == (pairs == 12288)
    r = Resident(ctx, frames.reshape(pairs + 1, n, 1), 32, 32)
    try:
        rows, ones = r.mask(0, None, 1)
        assert ones.tolist() == bits.sum(1).tolist()
        for f in (0, 1, 2, 127, 128, 129, 6143, 6144, pairs - 2, pairs - 1):      # sampled rows against the reference ...
            want, _ = ms.ref_masks(frames.reshape(pairs + 1, n, 1)[f:f + 2], None, 0, 1)
            assert np.array_equal(rows[f], want[0]), f
        assert np.array_equal(rows, np.packbits(bits, axis=1))                    # ... and every row against "the byte changed", which is A1 at threshold 0 for 8 bits
    finally:
        r.close()
