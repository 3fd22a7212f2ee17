"""CPU tier of the bounded-error keyframes (ImprovedVideoCompressor(bounded_keyframes=True), record type 7): the numpy twin of the rule
(tests/near_key_ref.py), which walks the loop as include/rbf.h states it, keeps every sample within its bound on inputs that exercise the
upper clamp, every residue of the division, an escape code and a wrapping exact channel, and equals the rule's closed form (a state
below 0, which would exercise the lower clamp, cannot occur: every state is a non-negative multiple of its step, which is asserted); its decoder gives back the quantised frame; the record's parser refuses what include/rbf.h says
it refuses; the keyword's default and refusals; the C ABI's prototypes; the container's stream checks know type 7; and the kernels'
integer reciprocal is the division over its whole range.  The kernels against the twin: tests/test_gpu_near_keyframes.py."""
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import near_key_ref as nk
import sample_codec_ref as ref
from conftest import REPO
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd import sample_codec as sc
from new_bloom_filter_repo_amd.frame_codec import YUVFrame
from new_bloom_filter_repo_amd.surface_options import check_options
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor, _BlockRecords


def frame_of(kind, shape, dtype, seed=0):
    """The inputs of both tiers: `noise` (full range), `ramp` (smooth), `zeros`, `top` (constant maximum), `edges` (alternating extremes
    with a little noise: the states go above 2^B - 1 where the step allows it), `spikes` (flat with rare extremes: escape codes)."""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed + sum(shape))
    if kind == "noise":
        a = rng.integers(0, top + 1, shape)
    elif kind == "ramp":
        H, W = shape[:2]
        a = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 2) * (top // 255)
        a = a[..., None] + np.arange(int(np.prod(shape[2:], dtype=int)) or 1) * 5 if len(shape) == 3 else a
        a = a % (top + 1)
    elif kind == "zeros":
        a = np.zeros(shape, dtype=np.int64)
    elif kind == "top":
        a = np.full(shape, top, dtype=np.int64)
    elif kind == "spikes":
        a = np.where(rng.integers(0, 37, shape) == 0, top, 0)
    else:
        a = np.where(rng.integers(0, 2, shape) > 0, top - rng.integers(0, 4, shape), rng.integers(0, 4, shape))
    return np.ascontiguousarray(np.asarray(a).reshape(shape).astype(dtype))


CASES = [((9, 40, 3), np.uint8, 6), ((5, 9, 3), np.uint16, 3), ((9, 40, 3), np.uint8, 1), ((9, 40, 3), np.uint8, 2), ((9, 40, 3), np.uint8, 7), ((7, 33, 3), np.uint8, (1, 2, 2)),
         ((7, 33, 3), np.uint8, (0, 3, 3)), ((5, 70), np.uint8, 127), ((6, 35, 4), np.uint16, 300), ((6, 35, 1), np.uint16, 32767),
         ((4, 50, 3), np.uint16, (0, 3, 3)), ((1, 1), np.uint8, 2), ((1, 7, 3), np.uint16, 1), ((66, 1, 3), np.uint8, 2)]
KINDS = ("noise", "ramp", "zeros", "top", "edges", "spikes")


def channels_of(shape):
    return shape[2] if len(shape) == 3 else 1


@pytest.mark.parametrize("shape,dtype,bounds", CASES, ids=[("%s_%s_d%s" % ("x".join(map(str, s)), np.dtype(t).name, b)).replace(" ", "") for s, t, b in CASES])
def test_twin_keeps_the_bound_and_decodes_to_y(shape, dtype, bounds):
    C = channels_of(shape)
    d = nk.as_bounds(bounds, C)
    bits = 8 * np.dtype(dtype).itemsize
    for kind in KINDS:
        X = frame_of(kind, shape, dtype)
        Y, u, S = nk.quantise(X, d)
        err = np.abs(X.astype(np.int64) - Y.astype(np.int64)).reshape(shape[0], shape[1], C)
        for c in range(C):
            assert int(err[..., c].max()) <= d[c], (kind, c)
            if d[c] == 0:
                assert np.array_equal(Y.reshape(shape[0], shape[1], C)[..., c], X.reshape(shape[0], shape[1], C)[..., c])
            assert S[..., c].min() >= 0 and S[..., c].max() <= (1 << bits) - 1 + d[c]       # (the rule's range is [-d, ...]: 0 is what it comes to)
            assert not (S[..., c] % (2 * d[c] + 1)).any()
        Yc, Sc = nk.closed_form(X, d)
        assert np.array_equal(Yc, Y) and np.array_equal(Sc, S), kind
        assert u.max() < 1 << bits and u.size == X.size
        assert np.array_equal(nk.rebuild(u, shape, dtype, d), Y), kind
        if X.size <= 1200:                       # the bit-walking decoder: through the stream's bytes as well
            assert np.array_equal(nk.decode(ref.encode(u, bits), shape, dtype, d), Y), kind
        again, _, _ = nk.quantise(X, d)          # a pure function of (X, d)
        assert np.array_equal(again, Y)


def test_inputs_are_not_vacuous():
    """On the twin alone: the upper clamp, every residue of |e| + d modulo t for each step used, an escaping u, and a wrapping q of an
    exact channel all occur in the inputs above (the GPU tier runs the same generator).  A state below 0 never occurs, on any input:
    the chain starts at 0 and moves in multiples of t, so a negative state would be at least t > d below its sample."""
    below = above = escaped = wrapped = False
    residues = {}
    for shape, dtype, bounds in CASES:
        C = channels_of(shape)
        d = nk.as_bounds(bounds, C)
        bits = 8 * np.dtype(dtype).itemsize
        for kind in KINDS:
            X = frame_of(kind, shape, dtype)
            trace = {}
            Y, u, S = nk.quantise(X, d, trace)
            for t, seen in trace["residues"].items():
                residues.setdefault(t, set()).update(seen)
            for c in range(C):
                if d[c]:
                    below |= bool((S[..., c] < 0).any())
                    above |= bool((S[..., c] > (1 << bits) - 1).any())
                else:
                    x = X.astype(np.int64).reshape(shape[0], shape[1], C)[..., c]
                    wrapped |= bool((np.abs(np.diff(x, axis=1)) >= 1 << (bits - 1)).any())
            costs = ref.chunk_costs(u, bits)
            ks = costs.argmin(axis=1)
            kk = np.repeat(ks, ref.CHUNK)[:u.size]
            escaped |= bool(((kk < bits) & ((u >> np.minimum(kk, bits)) >= ref.ESC)).any())
    assert above and escaped and wrapped and not below
    for t, seen in residues.items():
        if t <= 15:                              # (the large steps have more residues than a small frame has samples)
            assert seen == set(range(t)), (t, sorted(set(range(t)) - seen))
    assert {3, 5, 7, 13, 15} <= set(residues)


def test_reciprocal_is_the_division_over_its_whole_range():
    """floor(n / t) = mulhi(n, m) >> sh for every numerator the kernels can meet, n <= 2^16 - 1 + 2 * 65535 (rbf_kernels_keyquant.h)."""
    n = np.arange(0, (1 << 16) + 2 * 65535, dtype=np.uint64)
    steps = list(range(3, 204, 2)) + [255, 257, 511, 513, 601, 4095, 4097, 32767, 32769, 65535, 65537, 131069, 131071]
    for t in steps:
        m, sh = nk.reciprocal(t)
        assert 0 < m <= (1 << 31) + 1 and 0 <= sh < 32
        assert np.array_equal(((n * np.uint64(m)) >> np.uint64(32)) >> np.uint64(sh), n // np.uint64(t)), t


def test_near_key_record_layout_and_refusals():
    frame = frame_of("noise", (6, 5, 3), np.uint8)
    Y, want = nk.record(frame, (1, 2, 2), yuv=1)
    stream = nk.stream(frame, (1, 2, 2))[1]
    rec = sc.near_key_record(YUVFrame(frame), (1, 2, 2), stream)
    assert rec == want
    assert rec[:14] == struct.pack("<IIIBB", 6, 5, 1, 3, 1) and rec[14:16] == b"\x01\x03" and rec[16:22] == struct.pack("<3H", 1, 2, 2)
    assert rec[22:24] == b"\0\0" and rec[24:] == stream
    d = sc.parse_near_key_record(rec)
    assert (d["height"], d["width"], d["itemsize"], d["channels"], d["yuv"], d["bounds"], bytes(d["stream"])) == (6, 5, 1, 3, 1, [1, 2, 2], stream)
    assert nk.parse(rec)[5] == [1, 2, 2]
    gray = frame_of("ramp", (4, 9), np.uint16)
    g = sc.near_key_record(gray, [300], nk.stream(gray, 300)[1])
    assert g == nk.record(gray, 300)[1] and g[12:18] == b"\x00\x00\x01\x01" + struct.pack("<H", 300) and g[18:20] == b"\0\0"
    assert sc.parse_near_key_record(g)["bounds"] == [300] and sc.parse_near_key_record(g)["channels"] == 0
    four = frame_of("noise", (3, 3, 4), np.uint8)
    f = sc.near_key_record(four, [1, 1, 1, 0], nk.stream(four, (1, 1, 1, 0))[1])
    assert len(f) - len(nk.stream(four, (1, 1, 1, 0))[1]) == 24 and sc.parse_near_key_record(f)["bounds"] == [1, 1, 1, 0]
    other = nk.stream(frame_of("noise", (6, 5, 3), np.uint16), (1, 2, 2))[1]
    short = nk.stream(frame_of("noise", (6, 4, 3), np.uint8), (1, 2, 2))[1]
    bad = {"version": rec[:14] + b"\x02" + rec[15:], "n": rec[:15] + b"\x02" + rec[16:], "padding": rec[:22] + b"\x01" + rec[23:],
           "stream B": rec[:24] + other, "stream N": rec[:24] + short, "truncated": rec[:-4], "head only": rec[:15],
           "itemsize": rec[:8] + struct.pack("<I", 3) + rec[12:], "channels": rec[:12] + b"\x05" + rec[13:]}
    for name, b in bad.items():
        with pytest.raises(ValueError):
            sc.parse_near_key_record(b)
        with pytest.raises(ValueError):
            nk.parse(b)
    with pytest.raises(ValueError):
        sc.near_key_record(frame, (1, 2), stream)
    with pytest.raises(ValueError):
        sc.near_key_record(frame, (1, 2, 65536), stream)


def test_keyword_default_and_refusals():
    sig = inspect.signature(ImprovedVideoCompressor.__init__)
    assert sig.parameters["bounded_keyframes"].default is False and list(sig.parameters)[-1] == "bounded_keyframes"
    assert list(inspect.signature(check_options).parameters)[-1] == "bounded_keyframes"
    assert ImprovedVideoCompressor().bounded_keyframes is False
    ok = dict(bounded_keyframes=True, sample_codec="rice", mask_channels="all", inter_frames=True, keyframe_interval=4, max_error=2)
    assert ImprovedVideoCompressor(**ok).bounded_keyframes is True
    for extra in (dict(hold_mode="lookahead"), dict(scene_cuts=True), dict(frame_digests=True), dict(quality_report=True), dict(pan_range=4),
                  dict(max_error=0, error_bounds=(1, 2, 2)), dict(max_error=0, error_bounds=[0, 0, 3])):
        assert ImprovedVideoCompressor(**dict(ok, **extra)).bounded_keyframes is True
    for extra, match in ((dict(sample_codec="zlib"), "sample_codec='rice'"), (dict(max_error=0), "max_error > 0 or error_bounds"),
                         (dict(max_error=0, error_bounds=(0, 0, 0)), "all zero"),
                         (dict(max_error=0, error_bounds=np.ones((4, 6), np.int64)), "one bound per channel"),
                         (dict(max_error=0, error_bounds=np.ones((4, 6, 3), np.int64)), "one bound per channel"),
                         (dict(mask_channels="luma"), "mask_channels='all'"), (dict(gop_batching=False), "gop_batching=True"),
                         (dict(keyframe_interval=1), "inter-frames")):
        with pytest.raises(ValueError, match=match):
            ImprovedVideoCompressor(**dict(ok, **extra))
    from new_bloom_filter_repo_amd import dist
    assert "bounded_keyframes" not in inspect.signature(dist.encode_video_sharded).parameters
    assert _BlockRecords().near_keys == {}


def test_prototypes_in_header_binding_and_library():
    hdr = open(os.path.join(REPO, "include", "rbf.h")).read()
    clean = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = nat.lib()
    for name, nargs in (("rbf_rice_encode_intra_near", 13), ("rbf_rice_decode_intra_near", 9)):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, clean)
        assert m and m.group(1).count(",") + 1 == nargs == len(nat._PROTOS[name][1]), name
        assert hasattr(lib, name)
    assert "t_c = 2 d_c + 1" in hdr and "floor((|e| + d_c) / t_c)" in hdr            # the rule is in the header
    assert len(re.findall(r"#define RBF_K_[A-Z]+ ", hdr)) == 15                       # no new kernel id


def test_container_checks_know_type_7():
    K, KR, KN, I, IR = container.KEY, container.KEY_RICE, container.KEY_NEAR, container.INTER, container.INTER_RICE
    assert KN == 7 and KN in container.KEY_TYPES and container.KEYS == (K, KR)
    container.check_types([KN, IR, IR, KN, IR, K, I, KR])
    assert container.inter_runs([KN, IR, IR, KN, IR, K, I, KR]) == [(0, 1, 3), (3, 4, 5), (5, 6, 7)]
    assert container.inter_runs([KN, KN]) == []
    with pytest.raises(ValueError, match="unknown record type 8"):
        container.check_types([KN, 8])
    rec = nk.record(frame_of("noise", (4, 4, 3), np.uint8), 1)[1]
    blob = container.write([(KN, rec), (K, b"zz")])
    assert blob[:4] == b"BFV2" and container.parse(blob) == [(KN, rec), (K, b"zz")] and container.size([(KN, rec), (K, b"zz")]) == len(blob)


def test_keyframe_quantiser_kernels_do_not_spill():
    out = subprocess.run(["python", os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    rows = {ln[:84].strip(): ln[84:].split() for ln in out.splitlines() if ln.startswith("k_keyquant_")}
    for name in ("k_keyquant_u", "k_keyquant_apply", "k_keyquant_rebuild"):
        hits = [n for n in rows if n.startswith(name)]
        assert hits, (name, sorted(rows))
        for n in hits:
            vgprs, sgprs, scratch, spills = rows[n][:4]
            assert scratch == "0" and spills == "0", (n, rows[n])
    assert len(rows) == 6                                                            # both sample widths of each
