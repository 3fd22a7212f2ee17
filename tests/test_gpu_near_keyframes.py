"""GPU tier of the bounded-error keyframes (rbf_rice_encode_intra_near / rbf_rice_decode_intra_near, ImprovedVideoCompressor(
bounded_keyframes=True), record type 7).  The kernels run the rule's closed form; the twin they are held against (tests/near_key_ref.py)
walks the loop as include/rbf.h states it: reconstructions are bit-exact and streams byte-exact, for every frame height and width around
the kernels' spans (256 samples of a row per workgroup on the encode side, 64 pixels per tile and 4 rows per workgroup on the decode
side), every channel count, both sample depths, the bounds and the inputs of the CPU tier.  Then the surface: type 7 at every keyframe,
a fresh default compressor decodes within the bound, the inter-frames are those of a clip whose keyframes had been the twin's Y all
along, and the keyword combines with the other block stages."""
import ctypes

import numpy as np
import pytest

import near_key_ref as nk
import sample_codec_ref as ref
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd import sample_codec as sc
from new_bloom_filter_repo_amd.integrity import IntegrityError
from new_bloom_filter_repo_amd.synthetic import make_camera_gop, make_panning_gop
from new_bloom_filter_repo_amd.verify import quality, verify_max_error
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
from test_near_keyframes_cpu import KINDS, frame_of

pytestmark = pytest.mark.gpu

POISON = 0xA5
PAD = 4096
SPAN = 256                                   # samples of a row per workgroup of k_keyquant_u / k_keyquant_apply


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def codec(ctx):
    c = sc.SampleCoder(ctx)
    yield c
    c.close()


def geometry(shape):
    return shape[0], shape[1], (shape[2] if len(shape) == 3 else 1)


def fit(bounds, C):
    """A case's bounds for C channels: one number for all, or the tuple cut / continued with its last entry."""
    if np.ndim(bounds) == 0:
        return [int(bounds)] * C
    return [int(bounds[min(c, len(bounds) - 1)]) for c in range(C)]


def encode_block(ctx, codec, block, indices, bounds):
    """rbf_rice_encode_intra_near on a resident block (F, H, W[, C]) with PAD poison bytes behind it: (streams, the block afterwards, the
    padding afterwards)."""
    F = block.shape[0]
    H, W, C = geometry(block.shape[1:])
    fb = block[0].nbytes
    buf = ctx.alloc(F * fb + PAD)
    try:
        buf.upload(np.full(PAD, POISON, np.uint8), F * fb)
        buf.upload(block)
        streams = codec.encode_near(buf.ptr, fb, F, indices, W, H, C, block.dtype.itemsize, bounds)
        raw = buf.download()
        return streams, raw[:F * fb].view(block.dtype).reshape(block.shape), raw[F * fb:]
    finally:
        buf.free()


def decode_into_poison(ctx, stream, shape, dtype, bounds):
    """rbf_rice_decode_intra_near of host bytes into a poisoned device frame with PAD poison bytes behind it: (rc, frame, padding)."""
    H, W, C = geometry(shape)
    nbytes = H * W * C * np.dtype(dtype).itemsize
    fb = ctx.alloc(nbytes + PAD)
    try:
        fb.upload(np.full(nbytes + PAD, POISON, np.uint8))
        src = np.frombuffer(bytes(stream), np.uint8)
        d = (ctypes.c_uint32 * C)(*bounds)
        rc = nat.lib().rbf_rice_decode_intra_near(ctx.handle, src.ctypes.data, src.nbytes, W, H, C, np.dtype(dtype).itemsize, d, fb.ptr)
        ctx.sync()
        raw = fb.download()
        return rc, raw[:nbytes].view(dtype).reshape(shape), raw[nbytes:]
    finally:
        fb.free()


def check_frame(ctx, codec, X, bounds):
    """One frame through both entries against the twin."""
    H, W, C = geometry(X.shape)
    d = fit(bounds, C)
    Y, want = nk.stream(X, d)
    streams, after, pad = encode_block(ctx, codec, X[None], [0], d)
    assert np.array_equal(after[0], Y), (X.shape, d)
    assert streams[0] == want, (X.shape, d)
    assert (pad == POISON).all()
    rc, back, pad = decode_into_poison(ctx, want, X.shape, X.dtype, d)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(back, Y) and (pad == POISON).all(), (X.shape, d)


BOUNDS = {np.uint8: [1, 2, 7, (1, 2, 2), (0, 3, 3), 127, 6], np.uint16: [1, 2, 7, (1, 2, 2), (0, 3, 3), 300, 32767, 3]}
LAYOUTS = [(C, dt) for C in (None, 1, 3, 4) for dt in (np.uint8, np.uint16)]
LAYOUT_IDS = ["c%s_%s" % (C, np.dtype(dt).name) for C, dt in LAYOUTS]


def widths(C):
    T = -(-SPAN // (C or 1))                 # pixels of a row a workgroup of the encode kernels spans
    return sorted({1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3})


@pytest.mark.parametrize("C,dtype", LAYOUTS, ids=LAYOUT_IDS)
def test_every_shape_against_the_twin(ctx, codec, C, dtype):
    """H in {1, 2, 63, 64, 65, 130} x W around the kernels' spans; bounds and inputs rotate so that every one meets several shapes."""
    bounds = BOUNDS[dtype]
    i = 0
    for H in (1, 2, 63, 64, 65, 130):
        for W in widths(C):
            shape = (H, W) if C is None else (H, W, C)
            check_frame(ctx, codec, frame_of(KINDS[(i // 2) % len(KINDS)], shape, dtype, seed=i), bounds[i % len(bounds)])
            i += 1


@pytest.mark.parametrize("C,dtype", LAYOUTS, ids=LAYOUT_IDS)
def test_every_bound_and_input_against_the_twin(ctx, codec, C, dtype):
    T = -(-SPAN // (C or 1))
    shape = (65, T + 1) if C is None else (65, T + 1, C)
    for bounds in BOUNDS[dtype]:
        for kind in KINDS:
            check_frame(ctx, codec, frame_of(kind, shape, dtype, seed=3), bounds)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_listed_frames_of_a_block_and_nothing_else(ctx, codec, dtype):
    shape = (37, 91, 3)
    block = np.stack([frame_of(KINDS[f % len(KINDS)], shape, dtype, seed=f) for f in range(7)])
    listed, d = [1, 3, 6], [1, 2, 2]
    for f in (0, 2, 4, 5):
        block[f].view(np.uint8)[...] = POISON
    streams, after, pad = encode_block(ctx, codec, block, listed, d)
    assert len(streams) == 3 and (pad == POISON).all()
    for f in range(7):
        if f in listed:
            Y, want = nk.stream(block[f], d)
            assert np.array_equal(after[f], Y) and streams[listed.index(f)] == want, f
        else:
            assert (after[f].view(np.uint8) == POISON).all(), f
    # the rule is a pure function of (X, d), and Y is a fixed point of it: a second pass over the quantised block changes nothing
    streams2, after2, _ = encode_block(ctx, codec, after, listed, d)
    assert np.array_equal(after2, after) and streams2 == streams


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_a_stream_under_parameters_no_encoder_picks_decodes(ctx, dtype):
    bits = 8 * np.dtype(dtype).itemsize
    X = frame_of("ramp", (33, 67, 3), dtype)
    d = [2, 0, 5]
    Y, cheapest = nk.stream(X, d)
    chunks = -(-X.size // ref.CHUNK)
    costs = ref.chunk_costs(nk.quantise(X, d)[1], bits)
    legal = np.where(costs <= costs[:, bits:], costs, -1)                           # (a chunk never has more words than its raw samples)
    legal[np.arange(chunks), costs.argmin(axis=1)] = -1
    for ks in ([bits] * chunks, [int(k) if row[k] >= 0 else bits for k, row in zip(legal.argmax(axis=1), legal)]):
        odd = nk.stream(X, d, ks=ks)[1]
        assert odd != cheapest
        rc, back, pad = decode_into_poison(ctx, odd, X.shape, dtype, d)
        assert rc == nat.RBF_OK and np.array_equal(back, Y) and (pad == POISON).all()


def test_refusals_write_nothing(ctx, codec):
    L = nat.lib()
    H, W, C, F = 9, 21, 3, 3
    fb = H * W * C
    frames = ctx.alloc(F * fb)
    cap = F * sc.max_stream_bytes(fb, 8)
    out = ctx.alloc(cap)
    sizes = (ctypes.c_uint64 * F)()
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    try:
        frames.upload(np.full(F * fb, POISON, np.uint8))
        out.upload(np.full(cap, POISON, np.uint8))
        enc = lambda idx, channels=C, bounds=(1, 2, 2), capacity=cap: L.rbf_rice_encode_intra_near(
            ctx.handle, frames.ptr, fb, u32(*idx), len(idx), W, H, channels, 1, u32(*bounds), out.ptr, capacity, sizes)
        for what, rc in (("channels 5", enc([0], channels=5, bounds=(1, 1, 1, 1, 1))), ("a bound over 65535", enc([0], bounds=(1, 65536, 1))),
                         ("short capacity", enc([0, 2], capacity=2 * sc.max_stream_bytes(fb, 8) - 4)), ("index past any block", enc([0, 65535])),
                         ("descending indices", enc([2, 1])), ("a frame twice", enc([1, 1])), ("no frames", enc([]))):
            assert rc == nat.RBF_EINVAL and L.rbf_last_error(), what
        with pytest.raises(ValueError, match="inside the block of 3 frames"):       # an index >= nframes: the binding knows the block's size
            codec.encode_near(frames.ptr, fb, F, [0, 3], W, H, C, 1, [1, 2, 2])
        ctx.sync()
        assert (frames.download() == POISON).all() and (out.download() == POISON).all()
    finally:
        frames.free()
        out.free()
    X = frame_of("noise", (H, W, C), np.uint8)
    good = nk.stream(X, [1, 2, 2])[1]
    other = nk.stream(frame_of("noise", (H, W + 1, C), np.uint8), [1, 2, 2])[1]
    flipped = bytearray(good)
    flipped[8] = 9                                                                   # k = 9 > B
    for what, bad in (("truncated", good[:-4]), ("ragged", good[:-1]), ("header only", good[:8]), ("another frame's", other), ("k > B", bytes(flipped))):
        rc, back, pad = decode_into_poison(ctx, bad, X.shape, np.uint8, [1, 2, 2])
        assert rc == nat.RBF_EINVAL and (back.view(np.uint8) == POISON).all() and (pad == POISON).all(), what
    H_, W_, C_ = geometry(X.shape)
    src = np.frombuffer(good, np.uint8)
    dst = ctx.alloc(X.nbytes)
    try:
        assert L.rbf_rice_decode_intra_near(ctx.handle, src.ctypes.data, src.nbytes, W_, H_, C_, 1, u32(1, 70000, 2), dst.ptr) == nat.RBF_EINVAL
        assert L.rbf_rice_decode_intra_near(ctx.handle, src.ctypes.data, src.nbytes, W_, H_, 5, 1, u32(1, 2, 2, 2, 2), dst.ptr) == nat.RBF_EINVAL
    finally:
        dst.free()


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
W, H, I, T, BLOCK = 96, 80, 4, 13, 8
KEYFRAMES = [0, 4, 8, 12]
_clip = {}


def clip():
    if "x" not in _clip:
        _clip["x"] = np.stack(make_camera_gop(19, W, H, T, sensor_noise=1))
    return _clip["x"]


def encode(frames, **kw):
    kw = dict(dict(keyframe_interval=I, mask_channels="all", sample_codec="rice", block_frames=BLOCK), **kw)
    comp = ImprovedVideoCompressor(**kw)
    try:
        res = comp.compress_video(list(frames), input_color_space="YUV")
        return res, comp.last_compressed_frames, comp
    finally:
        comp.close()


def decode_fresh(records, **kw):
    fresh = ImprovedVideoCompressor()
    try:
        dec = fresh.decompress_video(compressed_frames=container.parse(container.write(records)), **kw)
        return [np.asarray(getattr(d, "data", d)) for d in dec], fresh.last_integrity
    finally:
        fresh.close()


def twin_clip(x, bounds, keys=KEYFRAMES):
    y = x.copy()
    for t in keys:
        y[t] = nk.quantise(x[t], fit(bounds, 3))[0]
    return y


NEAR = [("first_d2", dict(max_error=2), 2), ("lookahead_d1", dict(max_error=1, hold_mode="lookahead"), 1),
        ("first_122", dict(error_bounds=(1, 2, 2)), (1, 2, 2)), ("lookahead_122", dict(error_bounds=(1, 2, 2), hold_mode="lookahead"), (1, 2, 2))]


@pytest.mark.parametrize("name,near,bound", NEAR, ids=[n for n, _, _ in NEAR])
def test_surface_codes_keyframes_within_the_bound(name, near, bound):
    x = clip()
    res, records, _ = encode(x, bounded_keyframes=True, **near)
    types = [ty for ty, _ in records]
    assert [t for t, ty in enumerate(types) if ty == container.KEY_NEAR] == KEYFRAMES and res["bounded_keyframes"] == 4 and res["keyframes"] == 4
    assert all(ty == container.INTER_RICE for t, ty in enumerate(types) if t not in KEYFRAMES)
    dec, _ = decode_fresh(records)
    v = verify_max_error(list(x), dec, bound, keyframe_interval=I)
    assert v["within_bound"] and v["frame_count"] == T and not v["keyframes_exact"], v
    y = twin_clip(x, bound)
    for t in KEYFRAMES:                          # the record is the twin's, byte for byte, and decodes to the twin's Y
        assert records[t][1] == nk.record(x[t], fit(bound, 3), yuv=1)[1], t
        assert np.array_equal(dec[t], y[t]), t
    # the inter-frames hang off Y: they are the records of the same call, keyword off, on a clip whose keyframes had been Y all along
    _, plain, _ = encode(y, **near)
    for t in range(T):
        if t not in KEYFRAMES:
            assert plain[t] == records[t], t
    dec_plain, _ = decode_fresh(plain)
    assert all(np.array_equal(a, b) for a, b in zip(dec, dec_plain))
    # and without the keyword the container has no type 7 and exact keyframes
    _, off, _ = encode(x, **near)
    assert [ty for ty, _ in off] == [container.KEY_RICE if t in KEYFRAMES else container.INTER_RICE for t in range(T)]
    key_bytes = lambda recs: sum(len(recs[t][1]) for t in KEYFRAMES)                 # (the inter-frames may grow: they are held against Y, not X)
    assert key_bytes(records) < key_bytes(off), (key_bytes(records), key_bytes(off), container.size(records), container.size(off))


def test_a_keyframe_two_blocks_hold_decodes_to_the_twins_y():
    """block_frames = 9: frame 8 is the last frame of the block (0 .. 8) and the first of the block (8 .. 12)."""
    x = clip()
    assert [(lo, end) for lo, end, _ in container.plan_range(0, 0, T, I, 9, True)[1]] == [(0, 9), (8, 13)]
    for lanes in (1, 2):
        _, records, _ = encode(x, bounded_keyframes=True, max_error=2, block_frames=9, gpu_lanes=lanes, frame_digests=True)
        assert [t for t, (ty, _) in enumerate(records[:T]) if ty == container.KEY_NEAR] == KEYFRAMES
        assert records[8][1] == nk.record(x[8], [2, 2, 2], yuv=1)[1]
        dec, integrity = decode_fresh(records)
        assert np.array_equal(dec[8], nk.quantise(x[8], [2, 2, 2])[0]) and integrity["checked"] == T
        assert verify_max_error(list(x), dec, 2)["within_bound"]


def test_a_planted_scene_cut_is_a_type_7_record():
    x = clip().copy()
    x[6:] = np.stack(make_camera_gop(23, W, H, T - 6, sensor_noise=1))          # another scene from frame 6 on
    res, records, comp = encode(x, bounded_keyframes=True, max_error=2, scene_cuts=True)
    assert res["scene_cuts"] == [6] and records[6][0] == container.KEY_NEAR
    assert [t for t, (ty, _) in enumerate(records) if ty == container.KEY_NEAR] == [0, 4, 6, 8, 12]
    dec, _ = decode_fresh(records)
    assert verify_max_error(list(x), dec, 2)["within_bound"]
    assert np.array_equal(dec[6], nk.quantise(x[6], [2, 2, 2])[0])
    _, plain, _ = encode(twin_clip(x, 2, [0, 4, 6, 8, 12]), max_error=2, scene_cuts=True)
    assert all(plain[t] == records[t] for t in range(T) if records[t][0] == container.INTER_RICE)


def test_digests_and_quality_report_describe_the_decoded_clip():
    x = clip()
    res, records, comp = encode(x, bounded_keyframes=True, error_bounds=(1, 2, 2), hold_mode="lookahead", frame_digests=True, quality_report=True)
    assert records[-1][0] == container.DIGESTS and len(records) == T + 1
    dec, integrity = decode_fresh(records)
    assert integrity == {"frames": T, "checked": T, "device": T, "host": 0}
    want = quality(list(x), dec, error_bounds=(1, 2, 2))
    assert comp.last_quality == want
    for t in KEYFRAMES:
        assert want[t]["changed_samples"] > 0 and 0 < want[t]["max_abs_error"] <= 2 and want[t]["over_bound"] == 0, t
    # one flipped payload byte of a type-7 record is caught: by the stream's own checks, or by the frame's digest
    t = 4
    rec = bytearray(records[t][1])
    rec[len(rec) - 9] ^= 0x10
    damaged = records[:t] + [(container.KEY_NEAR, bytes(rec))] + records[t + 1:]
    with pytest.raises((IntegrityError, ValueError)):
        decode_fresh(damaged)


def test_pan_alignment_combines_with_bounded_keyframes():
    w, h = 64, 48
    x = np.stack(make_panning_gop(31, w, h, 9, (2, 1), sensor_noise=1))
    res, records, _ = encode(x, bounded_keyframes=True, max_error=2, pan_range=4, block_frames=9)
    assert [t for t, (ty, _) in enumerate(records) if ty == container.KEY_NEAR] == [0, 4, 8]
    dec, _ = decode_fresh(records)
    v = verify_max_error(list(x), dec, 2, keyframe_interval=I)
    assert v["within_bound"] and v["frame_count"] == 9, v
    for t in (0, 4, 8):                          # a run first has offset 0: its slot is the caller's frame
        assert np.array_equal(dec[t], nk.quantise(x[t], [2, 2, 2])[0]), t
