"""The block-stage sweep (tests/test_gpu_block_stage_sweep.py: A several workgroups and a ragged end, B far offsets with decoys, C one
context whose scratch shrinks, grows and is shared) for the stages that came after it: the holds with a bound per sample
(rbf_temporal_hold_runs_map, rbf_temporal_lookahead_runs_map), the quality report (rbf_error_stats), the pan search (rbf_pan_search) and
the roll (rbf_roll_frames).

  A  every (sample type, channels) instantiation of the _map holds and of the report on 799x11 frames under a bound frame that differs
     from pixel to pixel, so that a bound tile or a pixel of another workgroup gives another answer; and the pan search with EVERY
     candidate of a range planted once, at every range at which the lane -> candidate mapping of k_pan_sad changes;
  B  frames past 2^31 and 2^32 -- the report with one block far and the other near, so that its two strides differ by gigabytes, and the
     roll, which WRITES there; and the keyframe quantiser (rbf_rice_encode_intra_near), which reads and WRITES its listed frames at
     frame_index[f] * frame_stride;
  C  err_partials through shrinking and growing calls, and search, roll, report and hold interleaved on one context; the quantiser's
     index list and the sample coder's u buffer, which it shares with rbf_rice_encode_inter and the two keyframe decoders.

The `ctx` and `far` fixtures are the sweep's, imported by name: module-scoped here as there, so the far block of this module is allocated
after the sweep's own is freed.  tests/test_block_stage_sweep_cpu.py proves every condition asserted here on the CPU."""
import ctypes

import numpy as np
import pytest

import block_layout as bl
import near_key_ref as nk
import pan_ref
import sample_codec_ref as ref
from error_bounds_ref import error_stats_ref
from new_bloom_filter_repo_amd import _native as nat
from test_gpu_block_stage_sweep import GEOMETRIES, GUARD, ctx, far, frames_are, lane_layouts, near, near_read, on_one_context_then_fresh, put_frames  # noqa: F401
from test_gpu_error_bounds import check_block, map_call, same_rows, stats_call
from new_bloom_filter_repo_amd import sample_codec
from test_gpu_near_keyframes import decode_into_poison as decode_near_into_poison
from test_gpu_near_keyframes import POISON as NEAR_POISON, encode_block as encode_near_block
from test_gpu_pan import as_rows, roll_call, roll_offsets, search
from test_gpu_sample_codec import decode_into_poison as decode_intra_into_poison
from test_gpu_sample_codec_sweep import encode_inter
from test_sample_codec_cpu import COUNTS as INTER_COUNTS, clip as inter_clip

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ A: every instantiation, several workgroups, a ragged end
def map_in_every_workgroup(ctx, rule, dtype, C):
    x, E = bl.lane_clip(dtype, C), bl.lane_bounds(dtype, C)
    want = bl.map_ref(rule, x, bl.LANE_STARTS, E)
    assert bl.lane_non_vacuous(x, want, bl.rule_lane_pixels(rule))
    in_wg, in_tail = bl.bounds_matter(x, want, rule, E)
    assert in_wg > 0 and in_tail > 0, "another pixel's bounds give another block, in the third workgroup and in the tail"
    fb, sb = x[0].nbytes, x.dtype.itemsize
    buf, ebuf = ctx.alloc(2 + bl.LANE_F * (fb + 32) + GUARD), ctx.alloc(16 + fb + GUARD)
    try:
        for pad, base in lane_layouts(x):
            rc, got, host = map_call(ctx, rule, buf, ebuf, x, E, bl.LANE_STARTS, pad=pad, base=base)
            assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
            check_block(got, host, x, want, pad, base)
        # a bound frame one sample off under aligned frames: the per-pixel kernels over the whole frame, first pixel 0, 35 workgroups
        pad = lane_layouts(x)[0][0]
        rc, got, host = map_call(ctx, rule, buf, ebuf, x, E, bl.LANE_STARTS, pad=pad, ebase=sb)
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
        check_block(got, host, x, want, pad, 0)
    finally:
        buf.free()
        ebuf.free()


@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_hold_map_in_every_workgroup(ctx, dtype, C):
    map_in_every_workgroup(ctx, "hold", dtype, C)


@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_lookahead_map_in_every_workgroup(ctx, dtype, C):
    map_in_every_workgroup(ctx, "lookahead", dtype, C)


@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_error_stats_in_every_workgroup(ctx, dtype, C):
    """The report of a block held under E: nothing over E, something over E // 2 and over 0; then with three planted maxima.  Both layouts
    for A and for B: lane tiles with a tail when both are aligned, the per-pixel kernel as soon as one is not."""
    a, E = bl.lane_clip(dtype, C), bl.lane_bounds(dtype, C)
    b = bl.map_ref("hold", a, bl.LANE_STARTS, E)
    a2, b2, places = bl.plant_maxima(a, b)
    assert bl.maxima_are_strict(a2, b2, places)
    top, fb = int(np.iinfo(dtype).max), a[0].nbytes
    bufs = [ctx.alloc(2 + bl.LANE_F * (fb + 48) + GUARD), ctx.alloc(2 + bl.LANE_F * (fb + 48) + GUARD), ctx.alloc(16 + fb + GUARD)]
    try:
        for name, bounds in bl.stats_bounds(E):
            for lo, hi in bl.stats_regions():
                sse, differing, over = bl.region_stats(a, b, bounds, lo, hi)
                assert sse > 0 and differing > 0 and (over > 0 or name == "frame"), (name, lo, hi)
            for pa, pb, planted in ((a, b, False), (a2, b2, True)):
                want = error_stats_ref(pa, pb, bounds)
                if not planted:
                    assert (not want["over_bound"].any()) if name == "frame" else (want["over_bound"].sum() > 0), name
                else:
                    assert [int(want["max_abs"][f]) for f, _, _ in places] == [top] * 3
                for a_pad, a_base in lane_layouts(a):
                    for b_pad, b_base in lane_layouts(a):
                        rc, rows = stats_call(ctx, bufs, pa, pb, bounds, a_pad=a_pad, b_pad=b_pad, a_base=a_base, b_base=b_base)
                        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
                        assert same_rows(rows, want), (name, planted, (a_pad, a_base), (b_pad, b_base), rows, want)
    finally:
        for buf in bufs:
            buf.free()


PLANTED = [(R, np.uint8) for R in bl.PLANTED_RANGES] + [(17, np.uint16)]


@pytest.mark.parametrize("R,dtype", PLANTED, ids=["R%d_%s" % (R, np.dtype(d).name) for R, d in PLANTED])
def test_every_candidate_is_found_where_it_is_planted(ctx, R, dtype):
    """One call of (2R+1)^2 pairs: pair p is rolled by candidate p, the one zero of its SAD table.  The search has to answer with that shift
    and a sad_best of 0 in every pair, so every candidate sum of the range is formed over its own window and stored by its own lane.
    R = 32 is 4225 pairs and 50 MB; nearly all of its time (0.85 s on an MI355X host) is the numpy reference of the pairs' tables and counts."""
    frames, shifts, tables = bl.planted_candidates(R, dtype)
    assert bl.planted_zero_is_unique(shifts, tables, R)
    want = as_rows(bl.planted_rows(frames, shifts, tables, R))
    rc, got = search(ctx, frames, R, 0)
    assert rc == 0, nat.lib().rbf_last_error()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d pairs, the first: %s" % (bad.size, len(want), [(shifts[p], got[p], want[p]) for p in bad[:4]])


# ------------------------------------------------------------------ B: far offsets, with decoys instead of faults
@pytest.mark.parametrize("dtype,C", bl.FAR_MAP_CASES, ids=bl.FAR_MAP_IDS)
@pytest.mark.parametrize("rule", bl.MAP_RULES)
def test_far_frames_hold_map_and_lookahead_map(ctx, far, rule, dtype, C):
    """One run of three frames under a bound frame in a small near block: frames 1 and 2 are rewritten past 2^31 and 2^32."""
    x, decoys, E, want = bl.far_map_case(rule, dtype, C)
    assert bl.far_map_decoys_matter(rule, x, decoys, E, want)
    lay, ptr = put_frames(far, x, decoys)
    eb = near(ctx, E.nbytes).upload(E)
    fn = nat.lib().rbf_temporal_hold_runs_map if rule == "hold" else nat.lib().rbf_temporal_lookahead_runs_map
    try:
        rc = fn(ctx.handle, ptr, lay.stride, 3, bl.LANE_W, bl.LANE_H, C, x.dtype.itemsize, eb.ptr, None)
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
        ctx.sync()
        assert np.array_equal(near_read(eb, E.nbytes), E.reshape(-1).view(np.uint8)), "the bound frame is only read"
    finally:
        eb.free()
    frames_are(lay, far, decoys, want)


@pytest.mark.parametrize("dtype,C", bl.FAR_MAP_CASES, ids=bl.FAR_MAP_IDS)
@pytest.mark.parametrize("side", ["a_far_b_near", "a_near_b_far"])
def test_far_frames_error_stats(ctx, far, side, dtype, C):
    """One block far, the other in a small near block -- its stride padded to 16 (the lane tiles and their tail), then dense (the per-pixel
    kernel) -- so the two strides differ by 2 GiB; against the bound frame and against a scalar."""
    a, b, E, a_decoys, b_decoys = bl.far_stats_case(dtype, C)
    for bounds in bl.FAR_STATS_BOUNDS:
        assert bl.far_stats_decoys_matter(a, b, E if bounds == "frame" else bounds, a_decoys, b_decoys), bounds
    a_far = side == "a_far_b_near"
    far_block, near_block, decoys = (a, b, a_decoys) if a_far else (b, a, b_decoys)
    fb, raw = a[0].nbytes, near_block.reshape(3, -1).view(np.uint8)
    lay, ptr = put_frames(far, far_block, decoys)
    eb = near(ctx, E.nbytes).upload(E)
    rows = np.zeros(3, dtype=nat.ERROR_ROW)
    try:
        for stride in (fb + (-fb) % 16, fb):
            assert (stride % 16 == 0) == (stride != fb)
            image = np.full(3 * stride, 0xFF, dtype=np.uint8)
            for f in range(3):
                image[f * stride:f * stride + fb] = raw[f]
            nb = near(ctx, image.size).upload(image)
            try:
                blocks = (ptr, lay.stride, nb.ptr, stride) if a_far else (nb.ptr, stride, ptr, lay.stride)
                for bounds in bl.FAR_STATS_BOUNDS:
                    scalar = bounds != "frame"
                    rows.view(np.uint8)[:] = 0xFF
                    rc = nat.lib().rbf_error_stats(ctx.handle, *blocks, 3, bl.LANE_W, bl.LANE_H, C, a.dtype.itemsize, None if scalar else eb.ptr,
                                                   bounds if scalar else 0, rows.ctypes.data)
                    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
                    want = error_stats_ref(a, b, bounds if scalar else E)
                    assert same_rows(rows, want), (stride, bounds, rows, want)
                assert np.array_equal(near_read(nb, image.size), image), "the near block is only read"
            finally:
                nb.free()
        assert np.array_equal(near_read(eb, E.nbytes), E.reshape(-1).view(np.uint8)), "the bound frame is only read"
    finally:
        eb.free()
    frames_are(lay, far, decoys, far_block)


def test_far_frames_pan_search(ctx, far):
    """k_pan_sad's (pair + 1) * frame_stride and k_pan_moving's two frame bases, past 2^31 and 2^32: every number of both rows."""
    x, decoys, want = bl.far_pan_case()
    assert bl.far_pan_decoys_matter(x, decoys, want)
    W, H, R = bl.FAR_PAN
    lay, ptr = put_frames(far, x, decoys)
    out = np.full(2 * nat.PAN_ROW.itemsize, 0xFF, dtype=np.uint8)
    rc = nat.lib().rbf_pan_search(ctx.handle, ptr, lay.stride, 3, W, H, 3, 1, R, 0, None, out.ctypes.data)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(out.view(nat.PAN_ROW), as_rows(want)), (out.view(nat.PAN_ROW), want)
    frames_are(lay, far, decoys, x)


@pytest.mark.parametrize("W,H,pb", bl.FAR_ROLLS, ids=bl.FAR_ROLL_IDS)
def test_far_frames_roll(ctx, far, W, H, pb):
    """The roll reads frame[j] * frame_stride into its scratch and copies back to the same place: a truncated write changes a decoy."""
    x, decoys, offsets, want = bl.far_roll_case(W, H, pb)
    assert bl.far_roll_decoys_matter(x, decoys, offsets, want)
    lay, ptr = put_frames(far, x, decoys)
    flat = (ctypes.c_int32 * 6)(*[int(v) for o in offsets for v in o])
    rc = nat.lib().rbf_roll_frames(ctx.handle, ptr, lay.stride, 3, W, H, pb, flat)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    frames_are(lay, far, decoys, want)


@pytest.mark.parametrize("dtype,C,bounds", bl.FAR_KEYQUANT_CASES, ids=bl.FAR_KEYQUANT_IDS)
def test_far_frames_keyframe_quantiser(ctx, far, dtype, C, bounds):
    """k_keyquant_u reads and k_keyquant_apply rewrites frames + frame_index[f] * frame_stride: frames 1 and 2 of the block are listed,
    past 2^31 and 2^32; frame 0 is not and stays.  Streams and frames are the twin's; a truncated read gives another stream, a truncated
    write changes a decoy."""
    x, decoys, want, streams = bl.far_keyquant_case(dtype, C, bounds)
    assert bl.far_keyquant_decoys_matter(x, decoys, want, streams, bounds)
    lay, ptr = put_frames(far, x, decoys)
    listed = bl.FAR_KEYQUANT_LISTED
    sb = x.dtype.itemsize
    cap = len(listed) * sample_codec.max_stream_bytes(x[0].size, 8 * sb)
    out = near(ctx, cap)
    sizes = (ctypes.c_uint64 * len(listed))()
    try:
        rc = nat.lib().rbf_rice_encode_intra_near(ctx.handle, ptr, lay.stride, (ctypes.c_uint32 * len(listed))(*listed), len(listed), bl.LANE_W, bl.LANE_H,
                                                  C, sb, (ctypes.c_uint32 * C)(*bounds), out.ptr, cap, sizes)
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
        ctx.sync()
        assert [int(v) for v in sizes] == [len(s) for s in streams]
        got = near_read(out, cap).tobytes()
        assert got[:sum(sizes)] == b"".join(streams) and got[sum(sizes):] == b"\xff" * (cap - sum(sizes))
    finally:
        out.free()
    frames_are(lay, far, decoys, want)


# ------------------------------------------------------------------ C: scratch that shrinks, and scratch that stages share
def stats_step(a, b, bounds):
    """A step of on_one_context_then_fresh: the report of (a, b) on lane tiles with a tail, checked against the reference."""
    want = error_stats_ref(a, b, bounds)
    assert want["differing"].any()
    fb = a[0].nbytes
    pad = (-fb) % 16

    def call(c):
        bufs = [c.alloc(len(a) * (fb + pad) + GUARD), c.alloc(len(a) * (fb + pad) + GUARD), c.alloc(fb + GUARD)]
        try:
            rc, rows = stats_call(c, bufs, a, b, bounds, a_pad=pad, b_pad=pad)
        finally:
            for buf in bufs:
                buf.free()
        assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
        assert same_rows(rows, want), (rows, want)
        return rows
    return call


def test_one_context_error_partials_shrink_and_grow():
    """16 rows of nine frames, 8 rows of three, 4 rows of nine, 16 of nine again; a bound frame in the first geometry, a scalar in the others."""
    from error_bounds_ref import hold_map_ref, random_clip, test_bounds
    steps = []
    for i, (F, W, H, dtype, C, starts) in enumerate(GEOMETRIES):
        a = random_clip(9700 + W, F, H, W, C, dtype)
        E = test_bounds(a.shape[1:], dtype, seed=C)[0]
        steps.append(stats_step(a, hold_map_ref(a, starts, E), E if i == 0 else 1))
    on_one_context_then_fresh(steps, [0, 1, 2, 0])


def test_one_context_pan_roll_report_and_hold_interleaved():
    """rbf_pan_search, rbf_roll_frames, rbf_error_stats and rbf_temporal_hold_runs_map as a GopCoder with pan_range, error_bounds and
    keep_originals calls them, at two geometries of search and roll: interleaved, none twice in a row."""
    def pan(W, H, R, tolerance, run_starts, nframes):
        frames, _ = pan_ref.planted_clip(W, H, R, np.uint8, nframes=nframes)
        want = as_rows(pan_ref.stat_rows(frames, R, tolerance, run_starts=run_starts or ()))

        def call(c):
            rc, got = search(c, frames, R, tolerance, run_starts=run_starts)
            assert rc == 0, nat.lib().rbf_last_error()
            assert np.array_equal(got, want), (got, want)
            return got
        return call

    def roll(W, H, pb, pad):
        offs = roll_offsets(W, H)                                  # twelve frames, ten of them rolled: two chunks of the scratch
        x = np.random.default_rng(9800 + W).integers(0, 256, (len(offs), H, W, pb), dtype=np.uint8)
        want = np.stack([pan_ref.roll(f, ox, oy) for f, (ox, oy) in zip(x, offs)])
        fb = H * W * pb

        def call(c):
            rc, got = roll_call(c, x, offs, pad)
            assert rc == 0, nat.lib().rbf_last_error()
            assert bool((got[:, fb:] == 0xA5).all()) and np.array_equal(got[:, :fb].reshape(x.shape), want)
            return got
        return call

    def report():
        a, E = bl.lane_clip(np.uint8, 3), bl.lane_bounds(np.uint8, 3)
        return stats_step(a, bl.map_ref("hold", a, bl.LANE_STARTS, E), E)

    def hold():
        x, E = bl.lane_clip(np.uint16, 2), bl.lane_bounds(np.uint16, 2)
        want = bl.map_ref("hold", x, bl.LANE_STARTS, E)
        fb = x[0].nbytes
        pad = (-fb) % 16

        def call(c):
            buf, ebuf = c.alloc(len(x) * (fb + pad) + GUARD), c.alloc(fb + GUARD)
            try:
                rc, got, host = map_call(c, "hold", buf, ebuf, x, E, bl.LANE_STARTS, pad=pad)
            finally:
                buf.free()
                ebuf.free()
            assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
            check_block(got, host, x, want, pad, 0)
            return got
        return call

    steps = [pan(320, 180, 8, 0, None, 4), roll(64, 16, 4, 0), report(), pan(67, 33, 4, 1, [2], 8), roll(67, 33, 3, 5), hold()]
    on_one_context_then_fresh(steps, [0, 1, 2, 3, 4, 5, 2, 0, 3, 1, 5, 4])


def as_bytes(streams):
    return [np.frombuffer(bytes(b), np.uint8) for b in streams]


def test_one_context_keyframe_quantiser_shares_the_sample_coders_scratch():
    """ctx->keyq (the listed indices) and the sample coder's u buffer through near-encode calls whose count and frame size shrink and grow,
    with rbf_rice_encode_inter, rbf_rice_decode_intra_near and rbf_rice_decode_intra -- which fill the same u buffer -- between them."""
    def near_encode(F, H, W, C, dtype, listed, bounds):
        rng = np.random.default_rng(9900 + W)
        shape = (H, W) if C is None else (H, W, C)
        block = rng.integers(0, int(np.iinfo(dtype).max) + 1, (F,) + shape).astype(dtype)
        block += (np.arange(W, dtype=dtype) * 3).reshape((1, 1, W) + (1,) * (len(shape) - 2))      # (a gradient under the noise: residuals of every size)
        want = [nk.stream(block[f], list(bounds)) for f in listed]
        assert all(not np.array_equal(Y, block[f]) for (Y, _), f in zip(want, listed))

        def call(c):
            codec = sample_codec.SampleCoder(c)
            try:
                streams, after, pad = encode_near_block(c, codec, block, listed, list(bounds))
            finally:
                codec.close()
            assert (pad == NEAR_POISON).all()
            for f in range(F):
                assert np.array_equal(after[f], want[listed.index(f)][0] if f in listed else block[f]), f
            assert streams == [s for _, s in want]
            return [after] + as_bytes(streams)
        return call

    def inter():
        frames, _, packed, streams = inter_clip(3, np.uint8)

        def call(c):
            rc, sizes, blob, cap = encode_inter(c, frames, packed, INTER_COUNTS)
            assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
            assert sizes == [len(s) for s in streams] and blob[:sum(sizes)] == b"".join(streams)
            return as_bytes([blob[:sum(sizes)]])
        return call

    def decode_near():
        X = np.random.default_rng(9950).integers(0, 65536, (33, 67, 3)).astype(np.uint16)
        d = [2, 0, 5]
        Y, stream = nk.stream(X, d)

        def call(c):
            rc, back, pad = decode_near_into_poison(c, stream, X.shape, X.dtype, d)
            assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
            assert np.array_equal(back, Y) and (pad == NEAR_POISON).all()
            return back
        return call

    def decode_intra():
        X = np.random.default_rng(9960).integers(0, 256, (21, 130, 4)).astype(np.uint8)
        stream = ref.encode(ref.intra_u(X, 8), 8)

        def call(c):
            rc, back = decode_intra_into_poison(c, stream, X.shape, X.dtype)
            assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
            assert np.array_equal(back, X)
            return back
        return call

    steps = [near_encode(*g) for g in bl.KEYQUANT_STEPS] + [inter(), decode_near(), decode_intra()]
    on_one_context_then_fresh(steps, bl.KEYQUANT_ORDER)
