"""Frame digests on the GPU: the kernel (rbf_frame_digest_batch: the 16-byte fast path, the generic path, every level count) equals the
numpy twin bit for bit on every layout, GopCoder.frame_digests() describes the frames a decoder returns (after the hold, too), and the
product surface writes a trailer, checks it on decode on the device and names the frame a structurally valid but wrong record damages."""
import numpy as np
import pytest

from frame_digest_ref import KNOWN, pattern
from near_lossless_ref import random_clip
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.gop import GopCoder
from new_bloom_filter_repo_amd.integrity import IntegrityError, digests_device, frame_digest, parse_trailer
from new_bloom_filter_repo_amd.verify import verify_container, verify_max_error
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor

pytestmark = pytest.mark.gpu

F = 5
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 6633, 13266, 172800, 2098176]
POISON64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


_twin = {}


def twin(L):
    """(the F frames of L pattern bytes each, their digests by the numpy twin), computed once per length."""
    if L not in _twin:
        frames = pattern(F * L).reshape(F, L)
        _twin[L] = (frames, [frame_digest(frames[f]) for f in range(F)])
    return _twin[L]


def run(ctx, frames, stride, base, nframes, tail):
    """Lay the frames out `stride` apart from byte `base` of a fresh device block that ends `tail` bytes behind the last frame's last byte
    (every byte that is not a frame's is 0xFF), poison the output, call the entry: (rc, the nframes digests, the entry behind them)."""
    count, L = frames.shape
    size = base + (count - 1) * stride + L + tail
    host = np.full(size, 0xFF, dtype=np.uint8)
    for f in range(count):
        host[base + f * stride:base + f * stride + L] = frames[f]
    buf = ctx.alloc(size).upload(host)
    out = ctx.alloc(8 * (count + 1)).upload(np.full(count + 1, POISON64, dtype=np.uint64))
    try:
        rc = nat.lib().rbf_frame_digest_batch(ctx.handle, buf.ptr + base, stride, nframes, L, out.ptr)
        ctx.sync()
        got = out.download(dtype=np.uint64)
        assert np.array_equal(buf.download(), host), "the frames are only read"
    finally:
        buf.free()
        out.free()
    assert (got[nframes:] == POISON64).all(), "nothing is written behind the digests of the call's frames"
    return rc, [int(g) for g in got[:nframes]]


@pytest.mark.parametrize("L", SIZES)
def test_kernel_equals_the_twin(ctx, L):
    frames, want = twin(L)
    if L in KNOWN:
        assert want[0] == KNOWN[L]
    up16 = (L + 15) // 16 * 16
    layouts = [("dense", L, 0, 0), ("dense, poison behind", L, 0, 64),
               ("stride of 16s, the block ends at the last byte", up16, 0, 0), ("stride of 16s, poison behind", up16, 0, 64)]
    layouts += [("base + %d" % b, up16, b, 64) for b in (1, 2, 4, 8)] + [("dense, base + 1", L, 1, 3)]
    for name, stride, base, tail in layouts:
        rc, got = run(ctx, frames, stride, base, F, tail)
        assert rc == nat.RBF_OK, (name, nat.lib().rbf_last_error())
        assert got == want, (name, [hex(g) for g in got], [hex(w) for w in want])
    for stride in (up16, L):                                       # one frame (any stride goes, 0 too), and none
        rc, got = run(ctx, frames[:1], stride, 0, 1, 0)
        assert rc == nat.RBF_OK and got == want[:1]
    rc, got = run(ctx, frames[:1], 0, 0, 1, 0)
    assert rc == nat.RBF_OK and got == want[:1]
    rc, got = run(ctx, frames, up16, 0, 0, 0)
    assert rc == nat.RBF_OK and got == []
    if L % 16 == 0:                                                # the generic path on a layout the fast path takes
        ctx.force_generic(1)
        try:
            rc, got = run(ctx, frames, L, 0, F, 0)
        finally:
            ctx.force_generic(0)
        assert rc == nat.RBF_OK and got == want


def test_kernel_refuses_what_it_cannot_hash(ctx):
    buf, out = ctx.alloc(64), ctx.alloc(64)
    try:
        lib = nat.lib()
        assert lib.rbf_frame_digest_batch(ctx.handle, buf.ptr, 16, 2, 0, out.ptr) == nat.RBF_EINVAL
        assert b"frame_bytes" in lib.rbf_last_error()
        assert lib.rbf_frame_digest_batch(ctx.handle, buf.ptr, 15, 2, 16, out.ptr) == nat.RBF_EINVAL
        assert b"stride" in lib.rbf_last_error()
        assert lib.rbf_frame_digest_batch(ctx.handle, None, 16, 2, 16, out.ptr) == nat.RBF_EINVAL
        assert lib.rbf_frame_digest_batch(ctx.handle, buf.ptr, 16, 2, 16, None) == nat.RBF_EINVAL
        assert lib.rbf_frame_digest_batch(ctx.handle, buf.ptr, 16, 2, 16, out.ptr + 4) == nat.RBF_EINVAL
        assert lib.rbf_frame_digest_batch(ctx.handle, None, 0, 0, 0, None) == nat.RBF_OK, "no frames: a no-op, whatever else is passed"
        # digests_device is the same call plus one download
        buf.upload(pattern(64))
        got = digests_device(ctx, buf.ptr, 16, 4, 16)
        assert got.dtype == np.uint64 and [int(g) for g in got] == [frame_digest(pattern(64)[16 * f:16 * f + 16]) for f in range(4)]
        assert digests_device(ctx, buf.ptr, 16, 0, 16).size == 0
    finally:
        buf.free()
        out.free()


# ------------------------------------------------------------------ the coder
def default_decode(records):
    dec = ImprovedVideoCompressor()
    try:
        return dec.decompress_video(compressed_frames=list(records))
    finally:
        dec.close()


@pytest.mark.parametrize("W,H,dtype", [(67, 33, np.uint8), (320, 180, np.uint16)], ids=["67x33_u8", "320x180_u16"])
def test_coder_digests_are_the_frames_digests(ctx, W, H, dtype):
    clip = random_clip(W, 12, H, W, 3, dtype)
    coder = GopCoder(ctx, W, H, 12, channels=3, sample_bytes=clip.dtype.itemsize, mask_channels=3, run_starts=[8])
    try:
        coder.load_frames(clip)
        coder.encode()
        got = coder.frame_digests()
        coder.results_packed()
    finally:
        coder.close()
    assert got.dtype == np.uint64 and [int(g) for g in got] == [frame_digest(clip[f]) for f in range(12)]


@pytest.mark.parametrize("W,H,dtype", [(67, 33, np.uint8), (320, 180, np.uint16)], ids=["67x33_u8", "320x180_u16"])
def test_coder_digests_follow_the_hold(ctx, W, H, dtype):
    """max_error=2: the digests are those of the frames a default decoder returns for the container of the same block."""
    rng = np.random.default_rng(W)
    top = int(np.iinfo(dtype).max)
    still = rng.integers(0, top + 1, (H, W, 3))
    noisy = np.clip(still[None] + rng.integers(-1, 2, (12, H, W, 3)), 0, top)              # +-1 around a still image: all of it is held
    moving = rng.integers(0, top + 1, (12, H, W, 3))
    where = rng.random((12, H, W, 1)) < 0.03                                               # ~3 % of the pixels move for real
    clip = np.where(where, moving, noisy).astype(dtype)
    coder = GopCoder(ctx, W, H, 12, channels=3, sample_bytes=clip.dtype.itemsize, mask_channels=3, max_error=2, run_starts=[8])
    try:
        coder.load_frames(clip)
        coder.encode()
        got = [int(g) for g in coder.frame_digests()]
    finally:
        coder.close()
    comp = ImprovedVideoCompressor(keyframe_interval=8, mask_channels="all", max_error=2, inter_frames=True)
    try:
        comp.compress_video([f for f in clip], input_color_space="YUV")
        decoded = default_decode(comp.last_compressed_frames)
    finally:
        comp.close()
    assert verify_max_error(list(clip), decoded, 2, keyframe_interval=8)["within_bound"]
    assert not all(np.array_equal(np.asarray(getattr(d, "data", d)), c) for d, c in zip(decoded, clip)), "the hold changed something"
    assert got == [frame_digest(d) for d in decoded]


# ------------------------------------------------------------------ the surface
MODES = [(mc, codec, dtype, 0) for mc in ("luma", "all") for codec in ("zlib", "rice") for dtype in (np.uint8, np.uint16)]
MODES += [("all", "zlib", np.uint8, 2), ("all", "rice", np.uint16, 2)]
T, W0, H0, INTERVAL = 24, 96, 64, 8


def surface_clip(dtype, seed=0):
    """24 frames of 96x64x3: a still image in which a few percent of the pixels change per frame -- every sample of a changed pixel, so
    that the luma mask covers every change and every frame off the keyframe grid is an inter-frame in either mask mode."""
    rng = np.random.default_rng(11 + seed)
    top = int(np.iinfo(dtype).max)
    still = rng.integers(0, top + 1, (H0, W0, 3)).astype(dtype)
    fresh = rng.integers(0, top + 1, (T, H0, W0, 3)).astype(dtype)
    where = rng.random((T, H0, W0, 1)) < 0.04
    clip = np.empty((T, H0, W0, 3), dtype=dtype)
    cur = still.copy()
    for t in range(T):
        if t:
            differs = (fresh[t] != cur).all(axis=-1, keepdims=True)
            cur = np.where(where[t] & differs, fresh[t], cur)
        clip[t] = cur
    return clip


_clips = {}


def clip_of(dtype):
    key = np.dtype(dtype).name
    if key not in _clips:
        _clips[key] = surface_clip(dtype)
        _clips[key].setflags(write=False)
    return _clips[key]


def encode(clip, **kw):
    comp = ImprovedVideoCompressor(keyframe_interval=INTERVAL, inter_frames=True, **kw)
    try:
        comp.compress_video([f for f in clip], input_color_space="YUV")
        return list(comp.last_compressed_frames), comp.last_digests
    finally:
        comp.close()


def data(frame):
    return np.asarray(getattr(frame, "data", frame))


@pytest.mark.parametrize("mc,codec,dtype,max_error", MODES, ids=["%s-%s-%s-e%d" % (m, c, np.dtype(d).name, e) for m, c, d, e in MODES])
def test_surface_round_trip(mc, codec, dtype, max_error):
    clip = clip_of(dtype)
    kw = dict(mask_channels=mc, sample_codec=codec, max_error=max_error)
    records, digests = encode(clip, frame_digests=True, **kw)
    assert records[-1][0] == container.DIGESTS and len(records) == T + 1
    blob = container.write(records)
    assert blob[:4] == b"BFV2"
    frame_records, stored = container.split_trailer(container.parse(blob))
    assert len(frame_records) == T and stored == [int(d) for d in digests] == parse_trailer(records[-1][1])
    assert sum(1 for ty, _ in frame_records if ty in container.INTERS) == T - T // INTERVAL, "every frame off the keyframe grid is an inter-frame"
    dec = ImprovedVideoCompressor()
    try:
        decoded = dec.decompress_video(compressed_frames=container.parse(blob))
        integrity = dec.last_integrity
    finally:
        dec.close()
    if max_error:
        v = verify_max_error(list(clip), decoded, max_error, keyframe_interval=INTERVAL)
        assert v["within_bound"] and v["keyframes_exact"], v
    else:
        assert all(np.array_equal(data(d), c) for d, c in zip(decoded, clip)), "bit-exact"
    assert set(integrity) == {"frames", "checked", "device", "host"}
    assert integrity["frames"] == T and integrity["checked"] == T and integrity["device"] >= 21, integrity
    assert integrity["device"] + integrity["host"] == T
    assert stored == [frame_digest(d) for d in decoded], "the stored digests are the numpy twin's of the decoded frames"
    # frame_digests=False is today's container, byte for byte
    plain, none = encode(clip, frame_digests=False, **kw)
    legacy, _ = encode(clip, **kw)
    assert none is None and container.write(plain) == container.write(legacy) == container.write(frame_records)
    dec = ImprovedVideoCompressor()
    try:
        again = dec.decompress_video(compressed_frames=container.parse(container.write(plain)))
        assert dec.last_integrity == {"frames": T, "checked": 0, "device": 0, "host": 0}
    finally:
        dec.close()
    assert all(np.array_equal(data(a), data(d)) for a, d in zip(again, decoded))
    # verify_digests=False reads the digest container without looking at the trailer's digests
    dec = ImprovedVideoCompressor(verify_digests=False)
    try:
        unchecked = dec.decompress_video(compressed_frames=container.parse(blob))
        assert dec.last_integrity["checked"] == 0 and dec.last_integrity["frames"] == T
    finally:
        dec.close()
    assert all(np.array_equal(data(a), data(d)) for a, d in zip(unchecked, decoded))
    assert verify_container(blob) == {"frames": T, "checked": T, "bad": [], "trailer": "ok"}
    assert verify_container(container.write(plain)) == {"frames": T, "checked": 0, "bad": [], "trailer": "absent"}


def test_surface_host_routes_agree():
    """gop_batching=False (every frame digested by the host twin from the originals) stores the digests the batched route takes on the
    device, and its decoder, frame by frame, checks them all."""
    clip = clip_of(np.uint8)
    batched, d0 = encode(clip, frame_digests=True, mask_channels="all")
    one_by_one, d1 = encode(clip, frame_digests=True, mask_channels="all", gop_batching=False)
    assert [int(d) for d in d0] == [int(d) for d in d1] == [frame_digest(f) for f in clip]
    dec = ImprovedVideoCompressor(gop_batching=False)
    try:
        decoded = dec.decompress_video(compressed_frames=one_by_one)
        assert dec.last_integrity["checked"] == T and dec.last_integrity["frames"] == T
    finally:
        dec.close()
    assert all(np.array_equal(data(d), c) for d, c in zip(decoded, clip))


# ------------------------------------------------------------------ detection
def tampered_pair(t):
    """(clip X, X', the pixel): X' is X with one sample of one pixel changed at frame t, at a pixel inside X's mask of that frame (t off the
    keyframe grid) or anywhere (a keyframe)."""
    clip = clip_of(np.uint8)
    other = clip.copy()
    if t % INTERVAL:
        ys, xs = np.nonzero((clip[t] != clip[t - 1]).any(axis=-1))
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    else:
        y, x = 5, 7
    other[t, y, x, 1] ^= 0x10
    return clip, other, (y, x)


def still_wrong(clip, t, pixel):
    """The frames a wrong sample at `pixel` of frame t reaches: t and every later frame of its run in which the pixel is not rewritten."""
    y, x = pixel
    bad = [t]
    u = t + 1
    while u < T and u % INTERVAL and not (clip[u, y, x] != clip[u - 1, y, x]).any():
        bad.append(u)
        u += 1
    return bad


@pytest.mark.parametrize("codec,t", [("zlib", 11), ("rice", 11), ("zlib", 8), ("rice", 8), ("zlib", 0)],
                         ids=["inter-type2", "inter-type4", "key-type1", "key-type3", "first-key-type1"])
def test_a_valid_but_wrong_record_is_named(codec, t):
    clip, other, pixel = tampered_pair(t)
    kw = dict(mask_channels="all", sample_codec=codec, frame_digests=True)
    good, _ = encode(clip, **kw)
    wrong, _ = encode(other, **kw)
    assert good[t][0] == wrong[t][0] == {("zlib", True): container.INTER, ("rice", True): container.INTER_RICE,
                                         ("zlib", False): container.KEY, ("rice", False): container.KEY_RICE}[(codec, bool(t % INTERVAL))]
    assert good[t][1] != wrong[t][1]
    mixed = list(good)
    mixed[t] = wrong[t]                                            # structurally valid: only the digest can notice
    expect_bad = still_wrong(clip, t, pixel)
    key_record = t - t % INTERVAL
    for chunk in (1, 4, 64):
        dec = ImprovedVideoCompressor()
        dec.chain_chunk_frames = chunk
        try:
            with pytest.raises(IntegrityError) as e:
                dec.decompress_video(compressed_frames=list(mixed))
        finally:
            dec.close()
        assert e.value.frame == t and e.value.key_record == key_record
        assert e.value.expected == frame_digest(clip[t]) and e.value.got != e.value.expected
        assert isinstance(e.value, ValueError)
        report = verify_container(container.write(mixed), chain_chunk_frames=chunk)
        assert report == {"frames": T, "checked": T, "bad": expect_bad, "trailer": "ok"}, (chunk, report)
    # without the check the damage goes through unnoticed -- which is what the trailer is for
    dec = ImprovedVideoCompressor(verify_digests=False)
    try:
        decoded = dec.decompress_video(compressed_frames=list(mixed))
    finally:
        dec.close()
    assert [u for u in range(T) if not np.array_equal(data(decoded[u]), clip[u])] == expect_bad


def test_a_changed_stored_digest_names_exactly_that_frame():
    clip = clip_of(np.uint8)
    records, digests = encode(clip, frame_digests=True, mask_channels="all")
    from new_bloom_filter_repo_amd.integrity import build_trailer
    for t in (0, 13, 23):
        lied = [int(d) for d in digests]
        lied[t] ^= 1 << 40
        mixed = records[:-1] + [(container.DIGESTS, build_trailer(lied))]
        dec = ImprovedVideoCompressor()
        try:
            with pytest.raises(IntegrityError) as e:
                dec.decompress_video(compressed_frames=mixed)
        finally:
            dec.close()
        assert (e.value.frame, e.value.expected, e.value.got) == (t, lied[t], int(digests[t]))
        assert verify_container(container.write(mixed))["bad"] == [t]
    # a damaged trailer is not a damaged frame
    blob = bytearray(container.write(records))
    blob[-12] ^= 0x01
    report = verify_container(bytes(blob))
    assert report["trailer"] == "damaged" and report["bad"] == [] and report["checked"] == 0 and report["frames"] == T
    dec = ImprovedVideoCompressor()
    try:
        with pytest.raises(ValueError) as e:
            dec.decompress_video(compressed_frames=container.parse(bytes(blob)))
        assert not isinstance(e.value, IntegrityError)
    finally:
        dec.close()
