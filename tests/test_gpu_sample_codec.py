"""GPU tier of the sample codec (rbf_rice_* / ImprovedVideoCompressor(sample_codec="rice")): the kernels' streams are the numpy
reference's bytes (tests/sample_codec_ref.py) for arbitrary values, keyframes of every shape and channel count and a GopCoder block's pairs;
reference bytes decode back on poisoned buffers; bad streams are refused without a fault; and the product surface round trips camera-like
clips bit-exactly on every route, in containers smaller than the zlib mode's, sharded or not.  The sweep of the kernels' own code paths --
every Rice parameter, escape codes at every bit offset, hand-built streams under parameters no encoder picks, rbf_rice_encode_inter /
rbf_rice_apply_inter called directly on ragged and empty streams, and the refusals of rbf_rice_apply_inter -- is
tests/test_gpu_sample_codec_sweep.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import sample_codec_ref as ref
from conftest import REPO
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import sample_codec as sc
from new_bloom_filter_repo_amd.gop import GopCoder
from new_bloom_filter_repo_amd.synthetic import make_camera_gop
from new_bloom_filter_repo_amd.verify import verify_bit_exact
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
from test_sample_codec_cpu import CASES, samples

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


def decode_into_poison(ctx, stream, frame_shape, dtype):
    """rbf_rice_decode_intra of host bytes into a device frame poisoned with 0xFF: (rc, the frame)."""
    H, W = frame_shape[:2]
    C = frame_shape[2] if len(frame_shape) == 3 else 1
    nbytes = H * W * C * np.dtype(dtype).itemsize
    fb = ctx.alloc(nbytes)
    try:
        fb.upload(np.full(nbytes, 0xFF, np.uint8))
        src = np.frombuffer(bytes(stream), np.uint8)
        rc = nat.lib().rbf_rice_decode_intra(ctx.handle, src.ctypes.data, src.nbytes, W, H, C, np.dtype(dtype).itemsize, fb.ptr)
        ctx.sync()
        return rc, fb.download(nbytes).view(dtype).reshape(frame_shape)
    finally:
        fb.free()


def frame_of_u(u, bits):
    """A 1 x N single-channel frame whose keyframe u values are exactly u (the GPU codes arbitrary values through the keyframe path)."""
    s = ref.from_u(u, bits)
    return ref.rebuild_scan(s, (1, len(u), 1), bits).astype(np.uint8 if bits == 8 else np.uint16)


VALUES = [c for c in CASES if c[1]]                                  # (N = 0: the empty stream of a pair without changes, below)


@pytest.mark.parametrize("bits,n,kind", VALUES, ids=["b%d_n%d_%s" % c for c in VALUES])
def test_values_encode_to_the_reference_bytes_and_back(ctx, codec, bits, n, kind):
    u = samples(kind, n, bits, n + bits)
    frame = frame_of_u(u, bits)
    assert np.array_equal(ref.intra_u(frame, bits), u)
    want = ref.encode(u, bits)
    assert codec.encode_frames([frame])[0] == want
    rc, got = decode_into_poison(ctx, want, frame.shape, frame.dtype)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(got, frame)


def keyframe(shape, C, dtype, seed):
    H, W = shape
    if H * W >= 320 * 180:
        f = make_camera_gop(seed, W, H, 1, dtype=dtype)[0]
    else:
        f = np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, (H, W, 3)).astype(dtype)
    if C is None:
        return np.ascontiguousarray(f[..., 0])
    if C == 4:
        return np.ascontiguousarray(np.concatenate([f, f[..., :1] ^ 5], axis=2))
    return np.ascontiguousarray(f[..., :C])


KEYS = [(shape, C, dt) for shape in ((1, 1), (17, 5), (180, 320), (1080, 1920)) for C in (None, 1, 3, 4) for dt in (np.uint8, np.uint16)]


@pytest.mark.parametrize("shape,C,dtype", KEYS, ids=["%dx%d_c%s_%s" % (s[1], s[0], C, np.dtype(d).name) for s, C, d in KEYS])
def test_keyframes_encode_to_the_reference_bytes_and_decode_back(ctx, codec, shape, C, dtype):
    frame = keyframe(shape, C, dtype, shape[0] + (C or 0))
    bits = 8 * np.dtype(dtype).itemsize
    want = ref.encode(ref.intra_u(frame, bits), bits)
    got = codec.encode_frames([frame])
    assert got[0] == want
    rc, back = decode_into_poison(ctx, want, frame.shape, dtype)
    assert rc == nat.RBF_OK, nat.lib().rbf_last_error()
    assert np.array_equal(back, frame)
    if shape[0] * shape[1] < 10000:                                   # several frames in one call: the streams back to back
        other = (frame ^ 1).astype(dtype)
        two = codec.encode_frames([frame, other])
        assert two == [want, ref.encode(ref.intra_u(other, bits), bits)]


@pytest.mark.parametrize("mc,dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16), (3, np.uint16)])
def test_gop_block_pairs_are_the_reference_streams(ctx, codec, mc, dtype):
    W, H, F = 320, 184, 13
    frames = np.stack(make_camera_gop(500 + mc, W, H, F, moving=0.02, dtype=dtype))
    frames[7] = frames[6]                                             # a pair without changes
    starts = [4, 9]
    coder = GopCoder(ctx, W, H, F, channels=3, sample_bytes=np.dtype(dtype).itemsize, run_starts=starts, mask_channels=mc)
    try:
        coder.load_frames(frames)
        coder.encode()
        rows = coder.results_packed()
        ones = [r["ones"] for r in rows]
        res = coder.results()
        streams = coder.rice_streams(ones, codec)
        bits = 8 * np.dtype(dtype).itemsize
        assert len(streams) == F - 1
        for f in range(F - 1):
            if f + 1 in starts:
                assert streams[f] == ref.encode([], bits), f             # skipped pair: the empty stream
                continue
            mask = np.unpackbits(res[f]["mask"])[:W * H].reshape(H, W)
            assert int(mask.sum()) == ones[f]
            assert streams[f] == ref.encode(ref.inter_u(frames[f], frames[f + 1], mask, bits), bits), f
        assert ones[6] == 0 and streams[6] == ref.encode([], bits)
        # the apply direction rebuilds every coded pair from its predecessor
        for f in (0, 5, 10):
            out = codec.apply_chain(frames[f], [res[f]["mask"]], [streams[f]])
            if mc == 3:
                assert np.array_equal(out[0], frames[f + 1]), f
            else:                                                     # luma mask: the masked pixels take frame f+1's samples
                m = np.unpackbits(res[f]["mask"])[:W * H].reshape(H, W).astype(bool)
                want = frames[f].copy()
                want[m] = frames[f + 1][m]
                assert np.array_equal(out[0], want), f
    finally:
        coder.close()


def test_bad_streams_are_refused_without_a_fault(ctx, codec):
    frame = make_camera_gop(7, 96, 64, 1, dtype=np.uint16)[0]          # smooth: Rice-coded chunks (k < B)
    good = bytearray(ref.encode(ref.intra_u(frame, 16), 16))
    rc, out = decode_into_poison(ctx, good, frame.shape, np.uint16)
    assert rc == nat.RBF_OK and np.array_equal(out, frame)
    nch = sc.nchunks(frame.size)
    table = bytearray(good)
    table[8 + nch] ^= 1                                               # words[0] off by one: the table no longer matches the length
    bad_k = bytearray(good)
    bad_k[8] = 17                                                     # k > B
    for bad in (table, bad_k, good[:-4], good[:4] + b"\x08" + good[5:]):
        rc, out = decode_into_poison(ctx, bad, frame.shape, np.uint16)
        assert rc == nat.RBF_EINVAL, nat.lib().rbf_last_error()
        assert (out == 0xFFFF).all(), "refused before launch: the frame stays untouched"
        assert nat.lib().rbf_last_error()
    ks = np.frombuffer(bytes(good), np.uint8, nch, 8)
    assert (ks < 16).any()
    hdr = sc.header_bytes(frame.size)
    corrupt = bytearray(good)
    corrupt[hdr:] = b"\xff" * (len(good) - hdr)                       # every code an escape: the codes run past their words
    rc, out = decode_into_poison(ctx, corrupt, frame.shape, np.uint16)
    assert rc == nat.RBF_EINVAL and b"corrupt" in nat.lib().rbf_last_error()
    assert (out == 0xFFFF).all()
    # and the context is still good for a valid stream
    rc, out = decode_into_poison(ctx, good, frame.shape, np.uint16)
    assert rc == nat.RBF_OK and np.array_equal(out, frame)
    # encode: a capacity below the raw bound and wrong channel counts are refused
    fb = ctx.alloc(frame.nbytes).upload(frame)
    ob = ctx.alloc(1 << 16)
    sizes = (ctypes.c_uint64 * 1)()
    try:
        cap = sc.max_stream_bytes(frame.size, 16)
        assert nat.lib().rbf_rice_encode_intra(ctx.handle, fb.ptr, frame.nbytes, 1, 96, 64, 3, 2, ob.ptr, cap - 4, sizes) == nat.RBF_EINVAL
        assert nat.lib().rbf_rice_encode_intra(ctx.handle, fb.ptr, frame.nbytes, 1, 96, 64, 5, 2, ob.ptr, 1 << 16, sizes) == nat.RBF_EINVAL
        assert nat.lib().rbf_rice_encode_intra(ctx.handle, fb.ptr, frame.nbytes, 1, 96, 64, 3, 3, ob.ptr, 1 << 16, sizes) == nat.RBF_EINVAL
    finally:
        fb.free()
        ob.free()


# ------------------------------------------------------------------ the product surface
def blob_of(comp, frames):
    res = comp.compress_video(list(frames), input_color_space="YUV")
    assert res["keyframes"] == sum(1 for ty, _ in comp.last_compressed_frames if ty in (1, 3))
    return ImprovedVideoCompressor._container(comp.last_compressed_frames)


@pytest.mark.parametrize("dtype,mode", [(np.uint8, "all"), (np.uint8, "luma"), (np.uint16, "all"), (np.uint16, "luma")],
                         ids=["u8_all", "u8_luma", "u16_all", "u16_luma"])
def test_rice_surface_round_trips_on_every_route(dtype, mode):
    T = 47
    frames = make_camera_gop(2030, 320, 184, T, dtype=dtype)
    comp = ImprovedVideoCompressor(keyframe_interval=20, mask_channels=mode, sample_codec="rice")
    blob = blob_of(comp, frames)
    tm = dict(comp.last_timing)
    comp.close()
    zl = ImprovedVideoCompressor(keyframe_interval=20, mask_channels=mode)
    zblob = blob_of(zl, frames)
    ztm = dict(zl.last_timing)
    zl.close()
    assert set(tm) == set(ztm), set(tm) ^ set(ztm)
    recs = ImprovedVideoCompressor._parse_container(blob)
    types = {ty for ty, _ in recs}
    assert types <= {3, 4} and 3 in types, types
    if mode == "all":
        assert [ty for ty, _ in recs].count(3) == 3
    assert len(blob) < len(zblob), (len(blob), len(zblob))
    fresh = ImprovedVideoCompressor()
    dec = fresh.decompress_video(compressed_frames=recs)
    v = verify_bit_exact(frames, dec, color_space="YUV")
    assert v["success"] and v["exact_matches"] == T, v.get("different_frame_indices", [])[:8]
    assert all(type(d).__name__ == "YUVFrame" for d in dec)
    fresh.close()
    seq = ImprovedVideoCompressor(gop_batching=False)                # the frame-by-frame decoder reads it too
    dec2 = seq.decompress_video(compressed_frames=recs)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(dec, dec2))
    seq.close()
    for kw in (dict(gpu_lanes=1), dict(gpu_lanes=3, block_frames=7), dict(block_frames=13), dict(gop_batching=False)):
        other = ImprovedVideoCompressor(keyframe_interval=20, mask_channels=mode, sample_codec="rice", **kw)
        assert blob_of(other, frames) == blob, kw
        other.close()


def test_rice_surface_plain_arrays_and_2d_frames():
    """Non-YUV input: keyframes decode to plain arrays; 2-D frames travel as channels 0."""
    frames = [f[..., 0].copy() for f in make_camera_gop(9, 96, 40, 9)]
    comp = ImprovedVideoCompressor(keyframe_interval=4, inter_frames=True, sample_codec="rice")
    comp.compress_video(list(frames), input_color_space="BGR")
    recs = comp.last_compressed_frames
    comp.close()
    assert recs[0][0] == 3 and recs[0][1][12] == 0
    dec = ImprovedVideoCompressor().decompress_video(compressed_frames=recs)
    assert all(isinstance(d, np.ndarray) and np.array_equal(d, f) for d, f in zip(dec, frames))


WORKER = r'''
import json, os, sys, datetime
import numpy as np
sys.path.insert(0, %(repo)r)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
T, I = 61, 30
import torch, torch.distributed as dist
torch.cuda.set_device(0)
torch.cuda.init()
dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=600))
from new_bloom_filter_repo_amd import _native as nat, dist as D
from new_bloom_filter_repo_amd.synthetic import make_camera_gop
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
clip = make_camera_gop(78, 320, 184, T)                     # the same clip on every rank
start, stop = D.shard_range(T, world, rank)
first = D.halo_start(start, I)
ctx = nat.Context(0)
blob = D.encode_video_sharded(clip[first:stop], first, T, keyframe_interval=I, ctx=ctx, mask_channels="all", sample_codec="rice")
out = None
if rank == 0:
    comp = ImprovedVideoCompressor(keyframe_interval=I, ctx=ctx, mask_channels="all", sample_codec="rice")
    single = ImprovedVideoCompressor._container(comp.encode_range(clip, 0, 0, T))
    comp.close()
    types = [ty for ty, _ in ImprovedVideoCompressor._parse_container(blob)]
    out = {"same": blob == single, "bytes": len(blob), "inter": types.count(4), "key": types.count(3)}
dist.barrier()
dist.destroy_process_group()
if out is not None:
    print(json.dumps(out), flush=True)
'''


def test_sharded_rice_container_equals_single_process(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_sample_codec_tests", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    worker = tmp_path / "worker.py"
    worker.write_text(WORKER % {"repo": REPO})
    out_path = tmp_path / "rank0.out"
    os.environ.pop("RANK", None)
    with open(out_path, "w") as f:
        rc = bench.launch_ranks(2, [sys.executable, str(worker)], stdout0=f)
    text = out_path.read_text()
    assert rc == 0, text[-3000:]
    res = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
    assert res["same"] and res["inter"] == 58 and res["key"] == 3, res
