"""GPU sweep of the sample codec's kernels (csrc/rbf_kernels_rice.h) against the numpy reference (tests/sample_codec_ref.py), bit-exact:
every Rice parameter an encoder can pick, with and without escape codes; an escape code at every bit offset of a word; hand-built streams
under parameters no encoder picks (k = B - 1 among them), decode only; rbf_rice_encode_inter / rbf_rice_apply_inter called directly on
masks crafted so that empty streams are first, last and adjacent and a stream's n lands on 1023 .. 1026 samples; additions that wrap; and
the refusals of rbf_rice_apply_inter, none of which writes a frame.  tests/test_sample_codec_cpu.py proves on the reference alone that
these inputs hit what they claim."""
import ctypes

import numpy as np
import pytest

import sample_codec_ref as ref
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import sample_codec as sc
from test_gpu_sample_codec import decode_into_poison, frame_of_u
from test_sample_codec_cpu import (COUNTS, FORCED, FORCED_N, H, INTER, INTER_IDS, NPX, SWEEP, SWEEP_IDS, SWEEP_N, W, clip, forced_values,
                                   mixed_stream, short_chain, table_of)

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------ values, through the keyframe path
def encodes_to_and_decodes_from(ctx, codec, u, bits):
    frame = frame_of_u(u, bits)
    assert np.array_equal(ref.intra_u(frame, bits), u)
    want = ref.encode(u, bits)
    assert codec.encode_frames([frame])[0] == want
    rc, got = decode_into_poison(ctx, want, frame.shape, frame.dtype)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(got, frame)


@pytest.mark.parametrize("bits,k,every", SWEEP, ids=SWEEP_IDS)
def test_every_reachable_k_encodes_to_the_reference_bytes_and_back(ctx, codec, bits, k, every):
    u = ref.values_for_k(bits, k, SWEEP_N, 100 * bits + k, escape_every=every)
    encodes_to_and_decodes_from(ctx, codec, u, bits)


@pytest.mark.parametrize("bits", [8, 16])
def test_an_escape_code_at_every_bit_offset(ctx, codec, bits):
    encodes_to_and_decodes_from(ctx, codec, ref.escape_offsets(bits), bits)


def decodes_but_is_not_canonical(ctx, codec, u, bits, ks):
    forced = ref.encode(u, bits, ks=ks)
    assert list(table_of(forced, u.size)[0]) == list(ks)
    frame = frame_of_u(u, bits)
    rc, got = decode_into_poison(ctx, forced, frame.shape, frame.dtype)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(got, frame)
    again = codec.encode_frames([got])[0]
    assert again == ref.encode(u, bits) and again != forced


@pytest.mark.parametrize("bits,k", FORCED, ids=["b%d_k%d" % c for c in FORCED])
def test_hand_built_streams_under_any_legal_k_decode(ctx, codec, bits, k):
    decodes_but_is_not_canonical(ctx, codec, forced_values(bits, k, FORCED_N, 7 * bits + k), bits, [k, k])


@pytest.mark.parametrize("bits", [8, 16])
def test_a_stream_with_a_different_k_in_every_chunk_decodes(ctx, codec, bits):
    u, ks = mixed_stream(bits)
    decodes_but_is_not_canonical(ctx, codec, u, bits, ks)


# ------------------------------------------------------------------ rbf_rice_encode_inter / rbf_rice_apply_inter, called directly
POISON = 8


def encode_inter(ctx, frames, packed, ones):
    """rbf_rice_encode_inter on uploaded frames and mask rows, into a block filled with 0xA5: (rc, the sizes, the whole block, capacity)."""
    T, C = frames.shape[0], frames.shape[3]
    sb = frames.dtype.itemsize
    stride = nat.packed_stride(NPX)
    cap = sum(sc.max_stream_bytes(int(o) * C, 8 * sb) for o in ones)
    fb = ctx.alloc(frames.nbytes).upload(frames)
    mb = ctx.alloc(len(packed) * stride).upload(nat.mask_rows(packed, NPX))
    ob = ctx.alloc(cap + POISON).upload(np.full(cap + POISON, 0xA5, np.uint8))
    sizes = (ctypes.c_uint64 * (T - 1))()
    cnt = (ctypes.c_uint64 * (T - 1))(*[int(o) for o in ones])
    try:
        rc = nat.lib().rbf_rice_encode_inter(ctx.handle, fb.ptr, frames[0].nbytes, T, W, H, C, sb, mb.ptr, stride, cnt, ob.ptr, cap, sizes)
        ctx.sync()
        return rc, [int(s) for s in sizes], ob.download().tobytes(), cap
    finally:
        for b in (fb, mb, ob):
            b.free()


@pytest.mark.parametrize("C,dtype", INTER, ids=INTER_IDS)
def test_encode_inter_of_ragged_streams_is_the_reference(ctx, C, dtype):
    frames, _, packed, streams = clip(C, dtype)
    rc, sizes, block, cap = encode_inter(ctx, frames, packed, COUNTS)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert sizes == [len(s) for s in streams]
    total = sum(sizes)
    off = 0
    for f, s in enumerate(streams):
        assert block[off:off + len(s)] == s, f
        off += len(s)
    assert total <= cap and block[cap:] == b"\xa5" * POISON
    assert block[total:] == b"\xa5" * (cap + POISON - total)              # the sizes sum to the bytes written


@pytest.mark.parametrize("C,dtype", [(3, np.uint8), (1, np.uint16)], ids=["c3_uint8", "c1_uint16"])
def test_encode_inter_of_only_empty_streams(ctx, C, dtype):
    frames, _, _, _ = clip(C, dtype)
    same = np.repeat(frames[:1], 12, axis=0)
    empty = [np.zeros((NPX + 7) // 8, np.uint8)] * 11
    rc, sizes, block, cap = encode_inter(ctx, same, empty, [0] * 11)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert sizes == [8] * 11 and cap == 88
    assert block[:88] == ref.encode([], 8 * np.dtype(dtype).itemsize) * 11
    assert block[88:] == b"\xa5" * POISON


@pytest.mark.parametrize("delta", [1, -1])
def test_encode_inter_refuses_a_wrong_count(ctx, delta):
    frames, _, packed, _ = clip(3, np.uint8)
    ones = list(COUNTS)
    ones[4] += delta
    rc, _, block, cap = encode_inter(ctx, frames, packed, ones)
    assert rc == nat.RBF_EINVAL
    msg = nat.lib().rbf_last_error()
    assert b"pair 4" in msg and b"341" in msg, msg
    assert block[cap:] == b"\xa5" * POISON
    rc, sizes, _, _ = encode_inter(ctx, frames, packed, COUNTS)           # and the context still codes the right counts
    assert rc == nat.RBF_OK and sizes == [len(s) for s in clip(3, np.uint8)[3]]


def apply_inter(ctx, base, packed, streams):
    """rbf_rice_apply_inter of the whole chain in ONE call from `base` into a block poisoned with 0xFF: (rc, frames 1 .. count)."""
    count = len(streams)
    stride = nat.packed_stride(NPX)
    fb = ctx.alloc((count + 1) * base.nbytes).upload(np.full((count + 1) * base.nbytes, 0xFF, np.uint8))
    fb.upload(base, 0)
    mb = ctx.alloc(count * stride).upload(nat.mask_rows(packed, NPX))
    blob = np.frombuffer(b"".join(bytes(s) for s in streams), dtype=np.uint8)
    sizes = (ctypes.c_uint64 * count)(*[len(s) for s in streams])
    try:
        rc = nat.lib().rbf_rice_apply_inter(ctx.handle, blob.ctypes.data, sizes, count, W, H, base.shape[2], base.dtype.itemsize, mb.ptr, stride,
                                            fb.ptr)
        ctx.sync()
        out = fb.download(count * base.nbytes, offset=base.nbytes).view(base.dtype).reshape((count,) + base.shape)
        assert np.array_equal(fb.download(base.nbytes).view(base.dtype).reshape(base.shape), base)
        return rc, out
    finally:
        fb.free()
        mb.free()


@pytest.mark.parametrize("C,dtype", INTER, ids=INTER_IDS)
def test_apply_inter_rebuilds_the_chain_in_one_call_and_in_chunks(ctx, codec, C, dtype):
    frames, _, packed, streams = clip(C, dtype)
    rc, out = apply_inter(ctx, frames[0], packed, streams)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(out, frames[1:])
    for chunk_frames in (1, 4, 64):
        got = codec.apply_chain(frames[0], packed, streams, chunk_frames=chunk_frames)
        assert len(got) == 11 and np.array_equal(np.stack(got), frames[1:]), chunk_frames


@pytest.mark.parametrize("C,dtype", [(3, np.uint8), (4, np.uint16), (1, np.uint16)], ids=["c3_uint8", "c4_uint16", "c1_uint16"])
def test_apply_inter_adds_modulo_the_sample_width(ctx, codec, C, dtype):
    """Frames that also differ OUTSIDE their masks, samples at both ends of the range: the rebuilt chain is not the clip but what the
    format's rule gives, frame t = frame t-1 with (pred + s) mod 2^B at mask t's pixels, s from the original pair."""
    bits = 8 * np.dtype(dtype).itemsize
    rng = np.random.default_rng(bits + C)
    ends = np.array([0, 1, (1 << bits) - 2, (1 << bits) - 1])
    orig = ends[rng.integers(0, 4, (5, H, W, C))].astype(dtype)
    masks = [rng.random((H, W)) < 0.5 for _ in range(4)]
    packed = [np.packbits(m.reshape(-1)) for m in masks]
    streams = [ref.encode(ref.inter_u(orig[t], orig[t + 1], masks[t], bits), bits) for t in range(4)]
    want = [orig[0].astype(np.int64)]
    for t in range(4):
        nxt = want[-1].copy()
        s = (orig[t + 1].astype(np.int64) - orig[t].astype(np.int64)) & ((1 << bits) - 1)
        nxt[masks[t]] = (nxt[masks[t]] + s[masks[t]]) & ((1 << bits) - 1)
        want.append(nxt)
    want = np.stack(want[1:]).astype(dtype)
    assert np.array_equal(want[0][masks[0]], orig[1][masks[0]]) and not np.array_equal(want, orig[1:])
    wrapped = want[1].astype(np.int64) < want[0].astype(np.int64) + ((orig[2].astype(np.int64) - orig[1].astype(np.int64)) & ((1 << bits) - 1))
    assert (wrapped & masks[1][..., None]).any()                           # pred + s passed 2^B somewhere
    rc, out = apply_inter(ctx, orig[0], packed, streams)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(out, want)
    got = codec.apply_chain(orig[0], packed, streams, chunk_frames=3)
    assert np.array_equal(np.stack(got), want)


# ------------------------------------------------------------------ refusals of rbf_rice_apply_inter
def broken_third_streams(C, bits, good):
    """(name, the bytes to send as the third stream, a word of the refusal's message)."""
    n, _, _ = sc.stream_info(good)
    nch, hdr = sc.nchunks(n), sc.header_bytes(n)
    u = ref.decode(good)[0]
    ks = table_of(good, n)[0]
    assert nch >= 2 and ks.max() < bits
    # a valid stream of one pixel too many: rice_parse accepts it and k_rice_decode decodes it inside its own words; the host then
    # compares n with the mask's count, before any frame is written
    yield "one_pixel_more", ref.encode(np.concatenate([u, u[:C]]), bits), b"its mask marks"
    # n is not whole pixels: refused on the host in the loop over the streams, before anything is launched
    yield "n_not_whole_pixels", ref.encode(np.concatenate([u, u[:1]]), bits), b"not whole pixels"
    # words[0] off by one: rice_parse, before launch (the table no longer matches the stream's length)
    table = bytearray(good)
    table[8 + nch] ^= 1
    yield "table_off_by_one_word", bytes(table), b"sample stream 2"
    # k = B + 1: rice_parse, before launch
    bad_k = bytearray(good)
    bad_k[8] = bits + 1
    yield "k_above_b", bytes(bad_k), b"k = "
    # every payload bit set under k < B: rice_parse accepts the table; k_rice_decode reads escape after escape from the LDS copy of the
    # declared words (widx < words <= RICE_WMAX), runs out of them half way through the chunk and sets the error word
    corrupt = bytearray(good)
    corrupt[hdr:] = b"\xff" * (len(good) - hdr)
    yield "codes_run_past_the_words", bytes(corrupt), b"corrupt"


@pytest.mark.parametrize("C,dtype", [(3, np.uint16), (4, np.uint8)], ids=["c3_uint16", "c4_uint8"])
def test_apply_inter_refuses_a_broken_third_stream_before_it_writes(ctx, C, dtype):
    frames, packed, streams = short_chain(C, dtype)
    bits = 8 * np.dtype(dtype).itemsize
    top = np.iinfo(dtype).max
    rc, out = apply_inter(ctx, frames[0], packed, streams)
    assert rc == nat.RBF_OK and np.array_equal(out, frames[1:])
    names = []
    for name, third, word in broken_third_streams(C, bits, streams[2]):
        rc, out = apply_inter(ctx, frames[0], packed, streams[:2] + [third])
        msg = nat.lib().rbf_last_error()
        assert rc == nat.RBF_EINVAL, (name, rc, msg)
        assert msg and word in msg, (name, msg)
        assert (out == top).all(), name + ": every stream is checked before the first frame is written"
        names.append(name)
    assert len(names) == 5
    rc, out = apply_inter(ctx, frames[0], packed, streams)                 # the same context then applies the valid chain
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(out, frames[1:])
