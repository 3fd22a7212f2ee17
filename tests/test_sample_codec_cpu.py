"""CPU tier of the sample codec (ImprovedVideoCompressor(sample_codec="rice")): the format pinned by literal vectors and the numpy
reference (tests/sample_codec_ref.py), the k tie rule, the scan rebuild of keyframes, the type-3 / type-4 records and containers, the
keyword's validation, and the new kernels' registers (no scratch, no spills).  No GPU needed."""
import functools
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import sample_codec_ref as ref
from conftest import REPO
from new_bloom_filter_repo_amd import sample_codec as sc
from new_bloom_filter_repo_amd.frame_codec import YUVFrame, build_record, parse_record
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor

VEC8 = bytes.fromhex("05000000" "08000000" "02" "0100" "00" "b0f83f00")
VEC16 = bytes.fromhex("02000000" "10000000" "10" "0100" "00" "ffff0000")


def test_literal_vectors():
    assert ref.encode([0, 3, 1, 2, 40], 8) == VEC8
    assert ref.encode([65535, 0], 16) == VEC16
    assert [int(x) for x in ref.decode(VEC8)[0]] == [0, 3, 1, 2, 40]
    assert [int(x) for x in ref.decode(VEC16)[0]] == [65535, 0]
    assert sc.stream_info(VEC8) == (5, 8, len(VEC8)) and sc.stream_info(VEC16) == (2, 16, len(VEC16))


def samples(kind, n, bits, seed):
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    if kind == "geometric":
        return np.minimum(rng.geometric(0.15, n) - 1, top)
    if kind == "uniform":
        return rng.integers(0, top + 1, n)
    return np.full(n, 0 if kind == "zeros" else top)


CASES = [(bits, n, kind) for bits in (8, 16) for n in (0, 1, 5, 1023, 1024, 1025, 3000) for kind in ("geometric", "uniform", "zeros", "max")]


@pytest.mark.parametrize("bits,n,kind", CASES, ids=["b%d_n%d_%s" % c for c in CASES])
def test_reference_round_trip(bits, n, kind):
    u = samples(kind, n, bits, n + bits)
    blob = ref.encode(u, bits)
    got, b = ref.decode(blob)
    assert b == bits and np.array_equal(got, u)
    assert sc.stream_info(blob) == (n, bits, len(blob))
    assert len(blob) <= sc.max_stream_bytes(n, bits)          # k = B bounds every stream: incompressible content does not grow
    assert len(blob) % 4 == 0 and sc.header_bytes(n) == (8 + 3 * sc.nchunks(n) + 3) // 4 * 4
    if kind == "max" and n:
        assert set(np.frombuffer(blob, np.uint8, sc.nchunks(n), 8)) == {bits}      # escapes cost more than raw: stored
    if kind == "zeros" and n:
        assert set(np.frombuffer(blob, np.uint8, sc.nchunks(n), 8)) == {0}


def test_escape_codes_round_trip():
    """A chunk whose k < B still meets values far above it: 16 one-bits then the B raw bits."""
    for bits in (8, 16):
        u = np.zeros(1000, dtype=np.int64)
        u[::97] = (1 << bits) - 1
        blob = ref.encode(u, bits)
        assert blob[8] < bits
        assert np.array_equal(ref.decode(blob)[0], u)


def test_k_tie_goes_to_the_smallest_k():
    costs = ref.chunk_costs([0, 3, 1, 2, 40], 8)[0]
    assert costs[2] == costs[3] == 25 and costs.min() == 25 and VEC8[8] == 2
    costs = ref.chunk_costs(np.full(100, 127), 8)[0]                   # k = 6, 7 and 8 (raw) all cost 8 bits a sample
    assert costs[6] == costs[7] == costs[8] == 800 and costs.min() == 800
    assert ref.encode(np.full(100, 127), 8)[8] == 6


def test_mapping_is_a_bijection():
    for bits in (8, 16):
        d = np.arange(1 << bits)
        u = ref.to_u(d, bits)
        assert sorted(u.tolist()) == list(range(1 << bits))
        assert np.array_equal(ref.from_u(u, bits), d)
        assert ref.to_u([-1], bits)[0] == 1 and ref.to_u([1], bits)[0] == 2


@pytest.mark.parametrize("shape,bits", [((1, 1), 8), ((17, 5), 16), ((9, 13, 3), 8), ((6, 7, 4), 16), ((5, 4, 1), 8)])
def test_scan_rebuild_equals_sequential(shape, bits):
    frame = np.random.default_rng(sum(shape)).integers(0, 1 << bits, shape)
    s = ref.from_u(ref.intra_u(frame, bits), bits)
    assert np.array_equal(ref.rebuild_sequential(s, shape, bits), frame)
    assert np.array_equal(ref.rebuild_scan(s, shape, bits), frame)


def test_key_records_and_containers():
    frame = np.random.default_rng(1).integers(0, 256, (6, 5, 3)).astype(np.uint8)
    stream = ref.encode(ref.intra_u(frame, 8), 8)
    rec = sc.key_record(YUVFrame(frame), stream)
    assert rec[:14] == struct.pack("<IIIBB", 6, 5, 1, 3, 1) and rec[14:] == stream
    d = sc.parse_key_record(rec)
    assert (d["height"], d["width"], d["itemsize"], d["channels"], d["yuv"], bytes(d["stream"])) == (6, 5, 1, 3, 1, stream)
    gray = frame[..., 0].copy()
    assert sc.key_record(gray, ref.encode(ref.intra_u(gray, 8), 8))[12:14] == b"\x00\x00"     # 2-D frame: channels 0, no yuv
    for bad in (rec[:-4], rec[:8] + struct.pack("<I", 2) + rec[12:], rec[:12] + b"\x02" + rec[13:]):
        with pytest.raises(ValueError):
            sc.parse_key_record(bad)
    # type 4: type 2's bytes with the stream in the value field
    prev, cur = frame, frame.copy()
    cur[2, 3] += 1
    mask = (prev != cur).any(-1)
    vstream = ref.encode(ref.inter_u(prev, cur, mask, 8), 8)
    body = struct.pack("<B", 1) + build_record("f64", 0.01, 30, 2.5, 30, np.packbits(mask.reshape(-1)).tobytes(), 0, b"", 3, vstream)
    r = parse_record("f64", body[1:])
    assert r["value_count"] == 3 and r["values_z"] == vstream and sc.stream_info(vstream) == (3, 8, len(vstream))
    blob = ImprovedVideoCompressor._container([(3, rec), (4, body), (1, b"zz")])
    assert blob[:4] == b"BFV2" and len(blob) == ImprovedVideoCompressor._container_size([(3, rec), (4, body), (1, b"zz")])
    assert ImprovedVideoCompressor._parse_container(blob) == [(3, rec), (4, body), (1, b"zz")]
    assert ImprovedVideoCompressor._container([(3, rec)])[:4] == b"BFV2"            # only all-type-1 streams are 'BFVC'
    with pytest.raises(ValueError, match="unknown record type 5"):
        ImprovedVideoCompressor().decompress_video(compressed_frames=[(3, rec), (5, b"x")])
    with pytest.raises(ValueError, match="preceding keyframe"):
        ImprovedVideoCompressor().decompress_video(compressed_frames=[(4, body)])


def test_which_keyframes_type_3_carries():
    f8 = np.zeros((4, 6, 3), np.uint8)
    assert sc.key_format(f8) == (3, 0) and sc.key_format(f8[..., 0]) == (0, 0) and sc.key_format(np.zeros((4, 6, 1), np.uint16)) == (1, 0)
    y = YUVFrame(f8.copy())
    assert sc.key_format(y) == (3, 1)
    y.yuv_info["u_plane"]                                                          # a lazily copied plane is still the frame's own
    assert sc.key_format(y) == (3, 1)
    assert sc.key_format(np.zeros((4, 6, 3), np.float32)) is None
    assert sc.key_format(np.zeros((4, 6, 5), np.uint8)) is None
    foreign = YUVFrame(f8.copy())
    foreign.yuv_info = {"format": "YUV420", "y_plane": f8[..., 0], "u_plane": f8[:2, :3, 1], "v_plane": f8[:2, :3, 2]}
    assert sc.key_format(foreign) is None
    same = YUVFrame(f8.copy())
    same.yuv_info = {"format": "YUV444", "y_plane": f8[..., 0].copy(), "u_plane": f8[..., 1].copy(), "v_plane": f8[..., 2].copy()}
    assert sc.key_format(same) == (3, 1)


def test_sample_codec_keyword():
    assert ImprovedVideoCompressor().sample_codec == "zlib"
    assert ImprovedVideoCompressor(sample_codec="rice").sample_codec == "rice"
    assert ImprovedVideoCompressor(sample_codec="rice", inter_frames=True, mask_channels="all").sample_codec == "rice"
    with pytest.raises(ValueError):
        ImprovedVideoCompressor(sample_codec="lz4")
    with pytest.raises(ValueError):
        ImprovedVideoCompressor(sample_codec="rice", inter_frames=False)
    from new_bloom_filter_repo_amd import dist
    assert inspect.signature(dist.encode_video_sharded).parameters["sample_codec"].default == "zlib"


def test_sample_codec_kernels_do_not_spill():
    out = subprocess.run(["python", os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    rows = {ln[:84].strip(): ln[84:].split() for ln in out.splitlines() if ln.startswith("k_rice_")}
    for name in ("k_rice_intra_u", "k_rice_inter_u", "k_rice_cost", "k_rice_scan", "k_rice_headers", "k_rice_write", "k_rice_decode",
                 "k_rice_intra_rebuild", "k_rice_inter_add"):
        hits = [n for n in rows if n.startswith(name)]
        assert hits, (name, sorted(rows))
        for n in hits:
            assert rows[n][2] == "0" and rows[n][3] == "0", (n, rows[n])


# ------------------------------------------------------------------ inputs of the device sweep (tests/test_gpu_sample_codec_sweep.py)
# Proved here, on the reference alone, to hit what they claim: every reachable k, escape codes at every bit offset of a word, and
# hand-built streams under parameters no encoder picks.
SWEEP_N = 3 * 1024 + 77
SWEEP = [(bits, k, every) for bits in (8, 16) for k in range(bits - 1) for every in (0, 131)]
SWEEP_IDS = ["b%d_k%d_%s" % (b, k, "esc" if e else "plain") for b, k, e in SWEEP]
FORCED = [(bits, k) for bits in (8, 16) for k in range(bits + 1)]
FORCED_N = 1024 + 77


def table_of(blob, n):
    """(k, words) of every chunk of a stream of n samples."""
    c = sc.nchunks(n)
    return np.frombuffer(blob, np.uint8, c, 8).astype(int), np.frombuffer(blob, "<u2", c, 8 + c).astype(int)


def escapes_under(u, k, bits):
    """How many values of u take the escape code under k."""
    return 0 if k >= bits else int(((np.asarray(u) >> k) >= ref.ESC).sum())


def forced_values(bits, k, n, seed):
    """Values that fit a chunk written under k (its words stay within ceil(samples * B / 32), the cap every decoder checks) while another
    k is cheaper: the values that pick k - 1 (k = 0: those that pick 1; k = B: those that pick B - 2) cost k + 1 <= B bits each under k
    -- for k = B - 1 that is every value below 2^(B-1), at exactly B bits.  Where 2^B - 1 escapes under k and there is room (k <= B - 3),
    every 131st value is an escape."""
    j = 1 if k == 0 else min(k - 1, bits - 2)
    every = 131 if ((1 << bits) - 1) >> k >= ref.ESC and k <= bits - 3 else 0
    return ref.values_for_k(bits, j, n, seed, escape_every=every)


def mixed_stream(bits):
    """(u, ks): four chunks under k = 0, B, a middle k with escapes, and B - 1 on the ragged tail."""
    mid = bits // 2 - 1
    u = np.concatenate([forced_values(bits, 0, 1024, 1), samples("uniform", 1024, bits, 2), forced_values(bits, mid, 1024, 3),
                        forced_values(bits, bits - 1, 77, 4)])
    return u, [0, bits, mid, bits - 1]


@pytest.mark.parametrize("bits,k,every", SWEEP, ids=SWEEP_IDS)
def test_values_for_k_pick_k_in_every_chunk(bits, k, every):
    u = ref.values_for_k(bits, k, SWEEP_N, 100 * bits + k, escape_every=every)
    assert u.size == SWEEP_N and u.min() >= 0 and u.max() < 1 << bits
    blob = ref.encode(u, bits)
    ks, _ = table_of(blob, SWEEP_N)
    assert set(ks) == {k}, ks
    claimed = bool(every) and ((1 << bits) - 1) >> k >= ref.ESC          # k <= 3 at 8 bits, k <= 11 at 16 bits
    assert claimed == (bool(every) and k <= bits - 5)
    assert (escapes_under(u, k, bits) > 0) == claimed
    if every:
        assert int((u == (1 << bits) - 1).sum()) >= SWEEP_N // every
    assert np.array_equal(ref.decode(blob)[0], u)


def test_values_for_k_refuses_the_unreachable_k():
    for bits in (8, 16):
        for k in (-1, bits - 1, bits):
            with pytest.raises(ValueError):
                ref.values_for_k(bits, k, 10, 0)


@pytest.mark.parametrize("bits", [8, 16])
def test_no_chunk_picks_k_b_minus_1(bits):
    """k = B - 1 is never the cheapest-then-smallest parameter.  (1) A chunk with a value >= 2^(B-1): under k = B - 1 that value costs
    q + 1 + k = B + 1 bits and every other one B, more than the B bits a value of k = B, so k = B beats it.  (2) All values below 2^(B-1):
    k = B - 1 costs exactly B bits a value; under k = B - 2, q <= 1, so a value costs at most B -- no more in total, and the tie goes to the
    smaller k.  Either way argmin != B - 1; only a hand-built stream carries it."""
    rng = np.random.default_rng(bits)
    half, quarter = 1 << (bits - 1), 1 << (bits - 2)
    chunks = [rng.integers(quarter, half, 1024), rng.integers(0, quarter, 1024), np.full(1024, half - 1), np.full(1024, quarter),
              np.zeros(1024, dtype=np.int64), np.full(1, half - 1), np.full(77, half - 1)]
    one_high = rng.integers(0, half, 1024)
    one_high[500] = half
    top_high = rng.integers(quarter, half, 1024)
    top_high[0] = (1 << bits) - 1
    chunks += [one_high, top_high, np.full(1024, half), np.full(3, half)]
    for hi in (2, 5, quarter, half, half + 1, 1 << bits):                 # random chunks of every magnitude, full and ragged
        for n in (1, 7, 1023, 1024):
            chunks.append(rng.integers(0, hi, n))
    for t in range(200):
        k = int(rng.integers(0, bits + 1))
        chunks.append(np.minimum(rng.geometric(1.0 / (1 << k), int(rng.integers(1, 1025))) - 1, (1 << bits) - 1))
    for u in chunks:
        costs = ref.chunk_costs(u, bits)[0]
        assert costs.argmin() != bits - 1, (u[:8], costs)
        if u.max() < half:
            assert costs[bits - 1] == u.size * bits >= costs[bits - 2]
        else:
            assert costs[bits - 1] > costs[bits]


@pytest.mark.parametrize("bits", [8, 16])
def test_escape_offsets_start_an_escape_at_every_bit_of_a_word(bits):
    u = ref.escape_offsets(bits)
    assert u.size <= 1024 and set(u.tolist()) == {0, (1 << bits) - 1}
    blob = ref.encode(u, bits)
    ks, words = table_of(blob, u.size)
    assert list(ks) == [0]
    starts = ref.escape_starts(u, 0, bits)
    assert len(starts) == ref.ESCAPE_RUNS == escapes_under(u, 0, bits)
    assert {int(s) & 31 for s in starts} == set(range(32))
    payload = int.from_bytes(blob[sc.header_bytes(u.size):], "little")
    code = 0xFFFF | ((1 << bits) - 1) << 16
    for s in starts:                                                       # the positions are those of the stream's own bits
        assert (payload >> int(s)) & ((1 << (16 + bits)) - 1) == code
    if bits == 16:                                                         # a 32-bit code on a word of its own, and one that leaves one bit of it
        assert int(starts[0]) == 0 and words[0] > 1
        assert any(int(s) & 31 == 31 for s in starts)
    assert np.array_equal(ref.decode(blob)[0], u)


@pytest.mark.parametrize("bits,k", FORCED, ids=["b%d_k%d" % c for c in FORCED])
def test_forced_k_streams_are_legal_and_decode(bits, k):
    u = forced_values(bits, k, FORCED_N, 7 * bits + k)
    blob = ref.encode(u, bits, ks=[k, k])
    ks, words = table_of(blob, FORCED_N)
    assert list(ks) == [k, k]
    for ci, ns in enumerate((1024, 77)):                                   # rice_parse's acceptance cap
        assert 1 <= words[ci] <= (ns * bits + 31) // 32, (ci, words[ci])
    assert sc.stream_info(blob) == (FORCED_N, bits, len(blob))
    assert np.array_equal(ref.decode(blob)[0], u)
    canon = ref.encode(u, bits)
    assert k not in table_of(canon, FORCED_N)[0] and canon != blob          # a legal k that is not the cheapest
    if k == bits - 1:
        assert u.max() < 1 << (bits - 1)
    if k <= bits - 5:
        assert escapes_under(u, k, bits) > 0


@pytest.mark.parametrize("bits", [8, 16])
def test_mixed_k_stream_is_legal_and_decodes(bits):
    u, ks = mixed_stream(bits)
    assert u.size == SWEEP_N and len(set(ks)) == 4 and ks[-1] == bits - 1
    blob = ref.encode(u, bits, ks=ks)
    got, words = table_of(blob, u.size)
    assert list(got) == ks
    for ci in range(4):
        ns = min(1024, u.size - 1024 * ci)
        assert 1 <= words[ci] <= (ns * bits + 31) // 32
    assert escapes_under(u[2048:3072], ks[2], bits) > 0
    assert np.array_equal(ref.decode(blob)[0], u)
    assert ref.encode(u, bits) != blob


def test_forced_k_arguments_are_checked():
    u = np.arange(1030)
    assert ref.encode(u % 200, 8, ks=None) == ref.encode(u % 200, 8)
    for ks in ([3], [3, 3, 3], [3, 9], [-1, 3]):
        with pytest.raises(ValueError):
            ref.encode(u % 200, 8, ks=ks)


# ------------------------------------------------------------------ clips of the sweep's direct rbf_rice_encode_inter / rbf_rice_apply_inter calls
W, H = 67, 33
NPX = W * H                                                           # 2211: three 1024-pixel segments, 35 live bits in the last mask word
COUNTS = [0, 0, 1, 256, 341, 342, 1024, 1025, 2211, 0, 0]
SINGLE = [NPX - 1, 1024, 0]                                            # the lone bit: in the ragged last word, first of a segment, pixel 0
INTER = [(C, dt) for C in (1, 3, 4) for dt in (np.uint8, np.uint16)]
INTER_IDS = ["c%d_%s" % (C, np.dtype(dt).name) for C, dt in INTER]


def mask_with(count, seed, single):
    m = np.zeros(NPX, dtype=bool)
    if count == 1:
        m[single] = True
    else:
        m[np.random.default_rng(seed).choice(NPX, count, replace=False)] = True
    return m.reshape(H, W)


@functools.lru_cache(maxsize=None)
def clip(C, dtype):
    """(frames, masks, packed masks, reference streams) of 12 frames: frame t differs from frame t-1 at mask t-1's pixels only, by small
    steps in even pairs (small k) and to fresh uniform samples in odd ones (k = B).  Computed once; the tests leave it unchanged."""
    bits = 8 * np.dtype(dtype).itemsize
    rng = np.random.default_rng(1000 * C + bits)
    single = SINGLE[(INTER.index((C, dtype))) % 3]
    frames = [rng.integers(0, 1 << bits, (H, W, C)).astype(dtype)]
    masks = []
    for f, count in enumerate(COUNTS):
        m = mask_with(count, 50 * C + f, single)
        nxt = frames[-1].copy()
        if f % 2 == 0:
            nxt[m] = (nxt[m].astype(np.int64) + rng.integers(-3, 4, (count, C))).astype(dtype)        # (wraps mod 2^B)
        else:
            nxt[m] = rng.integers(0, 1 << bits, (count, C)).astype(dtype)
        masks.append(m)
        frames.append(nxt)
    frames = np.stack(frames)
    frames.setflags(write=False)
    packed = [np.packbits(m.reshape(-1)) for m in masks]
    streams = [ref.encode(ref.inter_u(frames[f], frames[f + 1], masks[f], bits), bits) for f in range(len(COUNTS))]
    return frames, masks, packed, streams


def test_the_inter_clips_are_what_they_claim():
    for C, dt in INTER:
        frames, masks, _, streams = clip(C, dt)
        bits = 8 * np.dtype(dt).itemsize
        assert [int(m.sum()) for m in masks] == COUNTS
        ns = [sc.stream_info(s)[0] for s in streams]
        assert ns == [c * C for c in COUNTS]
        tables = [set(table_of(s, n)[0]) for s, n in zip(streams, ns)]
        assert bits in tables[7] and max(tables[6]) < bits               # one call mixes parameters
        for f, m in enumerate(masks):
            assert np.array_equal(frames[f][~m], frames[f + 1][~m])
    assert {n for C in (1, 3, 4) for n in (c * C for c in COUNTS)} >= {1023, 1024, 1025, 1026}
    assert {SINGLE[i % 3] for i in range(len(INTER))} == set(SINGLE)
    assert sorted({SINGLE[INTER.index((C, np.uint16)) % 3] for C in (1, 3, 4)}) == sorted(SINGLE)


@functools.lru_cache(maxsize=None)
def short_chain(C, dtype):
    """(frames, packed masks, streams) of a chain of three pairs by small steps (every chunk Rice-coded, k < B); the third stream has
    several chunks."""
    bits = 8 * np.dtype(dtype).itemsize
    rng = np.random.default_rng(77 + C + bits)
    frames = [rng.integers(0, 1 << bits, (H, W, C)).astype(dtype)]
    masks = []
    for count in (300, 1, 1100):
        m = mask_with(count, 9 * count, 1024)
        nxt = frames[-1].copy()
        nxt[m] = (nxt[m].astype(np.int64) + rng.integers(-3, 4, (count, C))).astype(dtype)
        masks.append(m)
        frames.append(nxt)
    frames = np.stack(frames)
    frames.setflags(write=False)
    streams = [ref.encode(ref.inter_u(frames[t], frames[t + 1], masks[t], bits), bits) for t in range(3)]
    return frames, [np.packbits(m.reshape(-1)) for m in masks], streams


def test_the_short_chain_is_rice_coded():
    for C, dt in ((3, np.uint16), (4, np.uint8)):
        frames, packed, streams = short_chain(C, dt)
        bits = 8 * np.dtype(dt).itemsize
        assert [int(np.unpackbits(p)[:NPX].sum()) for p in packed] == [300, 1, 1100]
        n = sc.stream_info(streams[2])[0]
        assert n == 1100 * C and sc.nchunks(n) >= 2 and table_of(streams[2], n)[0].max() < bits
