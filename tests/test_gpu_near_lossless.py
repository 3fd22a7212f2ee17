"""The near-lossless mode on the GPU: the temporal hold (rbf_temporal_hold_runs: the 16-byte lane tiles, the ragged tail, the per-pixel
kernel of unaligned layouts) equals the numpy reference byte for byte and writes nothing it should not, GopCoder(max_error=...) codes the
held block exactly, and ImprovedVideoCompressor(max_error=...) writes containers a fresh default compressor decodes to the held clip --
within the bound, keyframes exact, smaller than the lossless container of the same noisy clip."""
import ctypes

import numpy as np
import pytest

from near_lossless_ref import all_channel_masks, hold_ref, random_clip
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd.frame_codec import parse_record
from new_bloom_filter_repo_amd.gop import GopCoder
from new_bloom_filter_repo_amd.synthetic import make_camera_gop
from new_bloom_filter_repo_amd.verify import verify_max_error
from new_bloom_filter_repo_amd.video_compressor import INTER, INTER_RICE, ImprovedVideoCompressor
from test_gpu_bench_shape import decode_back

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 512


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def geometry(frames):
    F, H, W = frames.shape[:3]
    return F, H, W, (frames.shape[3] if frames.ndim == 4 else 1), frames.dtype.itemsize


def hold_call(ctx, buf, frames, delta, starts, pad=0, base=0, nframes=None, channels=None, sample_bytes=None, stride=None):
    """Lay `frames` out in the device block `buf` (frame f at base + f * (frame bytes + pad), every other byte poisoned), call the entry
    and return (rc, the block's bytes, the layout's stride)."""
    F, H, W, C, sb = geometry(frames)
    fb = H * W * C * sb
    st = fb + pad
    host = np.full(buf.nbytes, POISON, dtype=np.uint8)
    assert base + F * st + GUARD <= buf.nbytes
    raw = frames.reshape(F, -1).view(np.uint8)
    for f in range(F):
        host[base + f * st:base + f * st + fb] = raw[f]
    buf.upload(host)
    rs = None
    if starts is not None:
        rs = (ctypes.c_uint8 * F)()
        for t in starts:
            rs[t] = 1
    rc = nat.lib().rbf_temporal_hold_runs(ctx.handle, buf.ptr + base, st if stride is None else stride, F if nframes is None else nframes, W, H,
                                          C if channels is None else channels, sb if sample_bytes is None else sample_bytes, delta, rs)
    ctx.sync()
    return rc, buf.download(), host


def check_block(got, host, frames, want, pad, base):
    """The frames in `got` equal `want`, and every byte outside them is what was uploaded (padding between frames, the guard behind)."""
    F, H, W, C, sb = geometry(frames)
    fb = H * W * C * sb
    st = fb + pad
    inside = np.zeros(got.size, dtype=bool)
    for f in range(F):
        lo = base + f * st
        inside[lo:lo + fb] = True
        assert np.array_equal(got[lo:lo + fb], want[f].reshape(-1).view(np.uint8)), "frame %d" % f
    assert np.array_equal(got[~inside], host[~inside]), "a byte outside the frames was written"
    assert (got[base + F * st:] == POISON).all(), "the guard behind the last frame"


SWEEP = [(3, np.uint8), (3, np.uint16), (4, np.uint8), (1, np.uint8), (1, np.uint16), (2, np.uint16)]
SHAPES = [(64, 32), (67, 5)]       # whole lane tiles | a ragged tail and an odd width: 3-byte pixels straddle dwords and 16-byte vectors


@pytest.mark.parametrize("W,H", SHAPES, ids=["64x32", "67x5"])
@pytest.mark.parametrize("C,dtype", SWEEP, ids=["c%d_%s" % (c, np.dtype(d).name) for c, d in SWEEP])
def test_hold_equals_reference(ctx, C, dtype, W, H):
    top = int(np.iinfo(dtype).max)
    clip = random_clip(100 * C + W, 9, H, W, C, dtype)
    fb = clip[0].nbytes
    aligned = (-fb) % 16 + 16                                   # padded by at least 16 bytes to a multiple of 16: the lane tiles with a ragged tail
    buf = ctx.alloc(2 + 9 * (fb + 32) + GUARD)
    refs = {}
    try:
        for F, starts in ((2, []), (9, []), (9, [4, 5])):
            x = clip[:F]
            for delta in (0, 1, 3, top):
                want = refs[(F, tuple(starts), delta)] = hold_ref(x, starts, delta)
                if delta == top:
                    assert all(np.array_equal(want[t], want[0]) for t in range(min(F, 4))), "every run collapses to its first frame"
                for pad in (0, aligned, 2):                         # dense | padded to 16-byte alignment | padded by 2: the unaligned path
                    rc, got, host = hold_call(ctx, buf, x, delta, starts, pad=pad)
                    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
                    check_block(got, host, x, want, pad, 0)
        # a base that is not 16-byte aligned, NULL run starts, and the per-pixel kernel on a layout the lane tiles would take
        x, want = clip, refs[(9, (), 3)]
        rc, got, host = hold_call(ctx, buf, x, 3, None, pad=0, base=2)
        assert rc == nat.RBF_OK
        check_block(got, host, x, want, 0, 2)
        ctx.force_generic(1)
        try:
            rc, got, host = hold_call(ctx, buf, x, 3, [4, 5], pad=aligned)
        finally:
            ctx.force_generic(0)
        assert rc == nat.RBF_OK
        check_block(got, host, x, refs[(9, (4, 5), 3)], aligned, 0)
        # idempotent: a second call on the held block changes nothing
        want = refs[(9, (4, 5), 1)]
        rc, got, host = hold_call(ctx, buf, want, 1, [4, 5])
        assert rc == nat.RBF_OK
        check_block(got, host, want, want, 0, 0)
    finally:
        buf.free()


@pytest.mark.parametrize("C,dtype", SWEEP, ids=["c%d_%s" % (c, np.dtype(d).name) for c, d in SWEEP])
def test_hold_decides_per_pixel_at_the_bound(ctx, C, dtype):
    """Every third pixel is a `centre`: one of its samples (each channel in turn, both signs) differs by exactly delta (held) while its two
    neighbours -- the pixels it shares dwords with -- differ by delta + 1 in one sample (updated); then the other way round."""
    W, H, delta = 66, 2, 3
    n = W * H
    base = np.full((n, C), 100, dtype=np.int64) + (np.arange(n)[:, None] * 7 + np.arange(C)[None, :] * 3) % 50
    idx = np.arange(n)
    centre = idx % 3 == 1
    chan = (idx // 3) % C
    sign = np.where((idx // (3 * C)) % 2 == 0, 1, -1)
    pad = (-n * C * np.dtype(dtype).itemsize) % 16             # a 16-byte aligned stride: the lane tiles (8 lanes) and a tail of 4 pixels
    buf = ctx.alloc(2 * (n * C * np.dtype(dtype).itemsize + pad) + GUARD)
    try:
        for centre_diff, other_diff in ((delta, delta + 1), (delta + 1, delta)):
            nxt = base.copy()
            nxt[idx, chan] += sign * np.where(centre, centre_diff, other_diff)
            x = np.stack([base, nxt]).astype(dtype).reshape(2, H, W, C)
            if C == 1:
                x = x[..., 0]
            want = hold_ref(x, [], delta)
            w = want.reshape(2, n, C)
            held = (w[1] == w[0]).all(-1)
            assert np.array_equal(held, centre if centre_diff == delta else ~centre), "the construction"
            rc, got, host = hold_call(ctx, buf, x, delta, [], pad=pad)
            assert rc == nat.RBF_OK
            check_block(got, host, x, want, pad, 0)
    finally:
        buf.free()


def test_hold_ramp_and_16_bit_extremes(ctx):
    F = 10
    x = (np.arange(F, dtype=np.uint8)[:, None, None, None] + np.full((1, 4, 20, 3), 40, dtype=np.uint8)).astype(np.uint8)
    buf = ctx.alloc(x.nbytes + GUARD)
    try:
        rc, got, host = hold_call(ctx, buf, x, 2, [])
        assert rc == nat.RBF_OK
        y = got[:x.nbytes].reshape(x.shape)
        assert [t for t in range(1, F) if not np.array_equal(y[t], y[t - 1])] == [3, 6, 9], "the loop is closed: a drift is caught"
        check_block(got, host, x, hold_ref(x, [], 2), 0, 0)
    finally:
        buf.free()
    x = np.zeros((3, 2, 16, 3), dtype=np.uint16)
    x[1:, 0, 5, 1] = 0x8000                                   # int16 arithmetic calls this difference 0
    x[2, 1, 9, 2] = 65535
    x[1:, 1, 15, 0] = 0x7FFF
    buf = ctx.alloc(x.nbytes + GUARD)
    try:
        for delta in (32767, 32768, 65534, 65535):
            want = hold_ref(x, [], delta)
            if delta == 32767:
                assert want[1, 0, 5, 1] == 0x8000 and want[2, 1, 9, 2] == 65535 and want[1, 1, 15, 0] == 0, "0x8000 and 65535 are updates"
            rc, got, host = hold_call(ctx, buf, x, delta, [])
            assert rc == nat.RBF_OK
            check_block(got, host, x, want, 0, 0)
    finally:
        buf.free()


def test_hold_leaves_frames_alone_and_refuses_bad_arguments(ctx):
    x = random_clip(5, 4, 8, 32, 3, np.uint8)
    x16 = random_clip(6, 4, 8, 32, 3, np.uint16)
    buf = ctx.alloc(x16.nbytes + 64 + GUARD)
    try:
        for kw in (dict(delta=0), dict(delta=3, nframes=1), dict(delta=3, nframes=0), dict(delta=255, nframes=1, stride=1)):
            kw = dict(kw)
            rc, got, host = hold_call(ctx, buf, x, kw.pop("delta"), [], **kw)
            assert rc == nat.RBF_OK, (kw, nat.lib().rbf_last_error())
            assert np.array_equal(got, host), kw
        ctx.timing(1 << nat.K_HOLD)
        ctx.timing_reset()
        bad = [(x, dict(delta=3, channels=0)), (x, dict(delta=3, channels=5)), (x, dict(delta=3, sample_bytes=3)), (x, dict(delta=3, sample_bytes=0)),
               (x, dict(delta=256)), (x, dict(delta=0xFFFFFFFF)), (x16, dict(delta=65536)), (x, dict(delta=3, stride=x[0].nbytes - 1)),
               (x, dict(delta=3, stride=0)), (x16, dict(delta=3, base=1)), (x16, dict(delta=3, pad=1))]
        for frames, kw in bad:
            kw = dict(kw)
            rc, got, host = hold_call(ctx, buf, frames, kw.pop("delta"), [], **kw)
            assert rc < 0 and nat.lib().rbf_last_error(), kw
            assert np.array_equal(got, host), kw
        assert ctx.timing_read()["hold"][1] == 0, "a refused call launches nothing"
        rc, got, host = hold_call(ctx, buf, x, 3, [2])
        assert rc == nat.RBF_OK
        check_block(got, host, x, hold_ref(x, [2], 3), 0, 0)
        ms, launches = ctx.timing_read()["hold"]
        assert launches == 1 and ms > 0, "the hold has a timing id of its own"
        assert nat.lib().rbf_temporal_hold_runs(None, buf.ptr, x[0].nbytes, 4, 32, 8, 3, 1, 3, None) < 0
    finally:
        ctx.timing(False)
        buf.free()


# ------------------------------------------------------------------ GopCoder
def test_gop_coder_codes_the_held_block(ctx):
    W, H, F, starts, delta = 96, 64, 13, [6], 2
    n = W * H
    x = np.stack(make_camera_gop(31, W, H, F, sensor_noise=1))
    y = hold_ref(x, starts, delta)
    want = all_channel_masks(y, starts)
    assert all_channel_masks(x, starts).mean() > 0.8 > 0.05 > want.mean()
    coder = GopCoder(ctx, W, H, F, channels=3, sample_bytes=1, run_starts=starts, mask_channels=3, max_error=delta)
    try:
        coder.load_frames(x)
        coder.encode()
        res = coder.results()
        assert np.array_equal(coder.frames.numpy(ctx, y.nbytes).view(np.uint8), y.reshape(-1)), "the resident block is its held sequence"
        coded = []
        for f in range(F - 1):
            if f + 1 in starts:
                assert res[f].get("skipped") and res[f]["ones"] == 0
                continue
            assert np.array_equal(res[f]["mask"], np.packbits(want[f])), f
            assert res[f]["ones"] == int(want[f].sum()) > 0, f
            coded.append(res[f])
        decode_back(ctx, coded, n, "near_lossless")
        vals = coder.gather_values()
        for f in range(F - 1):
            assert np.array_equal(vals[f], y[f + 1].reshape(n, 3)[want[f]].reshape(-1)), f
        coder.encode()                                          # idempotent: the held block again
        again = coder.results()
        for a, b in zip(res, again):
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]), k
    finally:
        coder.close()


# ------------------------------------------------------------------ the product surface
T, I, DELTA = 13, 6, 2
_clips, _lossless = {}, {}


def clip_and_reference(dtype):
    """The noisy clip, its held sequence with runs cut at the keyframes, and the reference's set-bit count per frame -- computed once."""
    key = np.dtype(dtype).name
    if key not in _clips:
        x = np.stack(make_camera_gop(77, 96, 64, T, dtype=dtype, sensor_noise=1))
        starts = list(range(I, T, I))
        y = hold_ref(x, starts, DELTA)
        ones = [0] + [int(m.sum()) for m in all_channel_masks(y, starts)]
        _clips[key] = (x, y, ones)
    return _clips[key]


def encode(frames, cs="YUV", **kw):
    comp = ImprovedVideoCompressor(keyframe_interval=I, mask_channels="all", **kw)
    try:
        res = comp.compress_video(list(frames), input_color_space=cs)
        return res, comp.last_compressed_frames, ImprovedVideoCompressor._container(comp.last_compressed_frames)
    finally:
        comp.close()


def lossless_container(dtype, codec):
    key = (np.dtype(dtype).name, codec)
    if key not in _lossless:
        res, _, blob = encode(clip_and_reference(dtype)[0], sample_codec=codec)
        _lossless[key] = (res, blob)
    return _lossless[key]


def decode_fresh(blob):
    fresh = ImprovedVideoCompressor()
    try:
        dec = fresh.decompress_video(compressed_frames=ImprovedVideoCompressor._parse_container(blob))
    finally:
        fresh.close()
    return [np.asarray(getattr(d, "data", d)) for d in dec]


@pytest.mark.parametrize("lanes,extra", [(1, {}), (2, {}), (2, {"block_frames": I})], ids=["lanes1", "lanes2", "lanes2_two_blocks"])
@pytest.mark.parametrize("codec", ["zlib", "rice"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_surface_near_lossless(dtype, codec, lanes, extra):
    x, y, ones = clip_and_reference(dtype)
    assert int(np.abs(y.astype(np.int64) - x.astype(np.int64)).max()) <= DELTA
    res0, blob0 = lossless_container(dtype, codec)
    assert "max_error" not in res0
    res, records, blob = encode(x, sample_codec=codec, max_error=DELTA, gpu_lanes=lanes, **extra)
    assert res["max_error"] == DELTA
    assert res["keyframes"] == res0["keyframes"] == 3
    dec = decode_fresh(blob)
    assert len(dec) == T and all(np.array_equal(d, want) for d, want in zip(dec, y)), "decodes to the held clip, exactly"
    v = verify_max_error(list(x), dec, DELTA, keyframe_interval=I)
    assert v["within_bound"] and v["keyframes_exact"] and v["frame_count"] == T, v
    for t, (ty, rec) in enumerate(records):
        if t % I == 0:
            assert ty not in (INTER, INTER_RICE)
            continue
        assert ty == (INTER_RICE if codec == "rice" else INTER), t
        assert parse_record("f64", rec[1:])["value_count"] == 3 * ones[t], t
    assert len(blob) < len(blob0), (len(blob), len(blob0))


def test_surface_single_channel_clip():
    x3, _, _ = clip_and_reference(np.uint8)
    x = np.ascontiguousarray(x3[..., 0])
    starts = list(range(I, T, I))
    y = hold_ref(x, starts, DELTA)
    res0, _, blob0 = encode(x, cs="BGR", inter_frames=True)
    res, records, blob = encode(x, cs="BGR", inter_frames=True, max_error=DELTA)
    assert res["keyframes"] == res0["keyframes"] == 3 and res["max_error"] == DELTA
    dec = decode_fresh(blob)
    assert all(d.shape == x[0].shape and np.array_equal(d, want) for d, want in zip(dec, y))
    v = verify_max_error(list(x), dec, DELTA, keyframe_interval=I)
    assert v["within_bound"] and v["keyframes_exact"]
    want_ones = [0] + [int(m.sum()) for m in all_channel_masks(y, starts)]
    for t, (ty, rec) in enumerate(records):
        if t % I:
            assert ty == INTER and parse_record("f64", rec[1:])["value_count"] == want_ones[t], t
    assert len(blob) < len(blob0)
