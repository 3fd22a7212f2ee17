"""CPU tier of the sample codec (ImprovedVideoCompressor(sample_codec="rice")): the format pinned by literal vectors and the numpy
reference (tests/sample_codec_ref.py), the k tie rule, the scan rebuild of keyframes, the type-3 / type-4 records and containers, the
keyword's validation, and the new kernels' registers (no scratch, no spills).  No GPU needed."""
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
