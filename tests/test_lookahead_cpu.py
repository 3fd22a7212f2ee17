"""The look-ahead hold without a GPU: the numpy reference (lookahead_ref.py) has the properties the mode rests on -- the bound, untouched
run firsts, mask == segment starts, never more updates per pixel than the first-value hold, and strictly fewer on camera noise at
max_error = noise amplitude -- and agrees with a scalar transcription of the rule; the Python layers validate hold_mode before they reach
the library; the header declares the entry, the ABI version stays, and no look-ahead kernel uses scratch memory."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from lookahead_ref import lookahead_ref, update_counts
from near_lossless_ref import all_channel_masks, hold_ref, random_clip
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd.gop import GopCoder
from new_bloom_filter_repo_amd.synthetic import make_camera_gop
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor


def scalar_lookahead(seq, e, top):
    """One pixel, one run: seq is a list of sample tuples.  The rule of include/rbf.h, word for word."""
    out = [tuple(seq[0])]
    prev = list(seq[0])
    lo, hi = list(seq[0]), list(seq[0])                        # anchored: |x_t - x_0| <= e  <=>  x_0 lies in x_t's window
    first, starts = 0, []
    C = len(prev)

    def close(end):
        v = [min(max(prev[c], lo[c]), hi[c]) for c in range(C)]
        for _ in range(max(first, 1), end):
            out.append(tuple(v))
        prev[:] = v

    for t in range(1, len(seq)):
        xl = [max(0, seq[t][c] - e) for c in range(C)]
        xh = [min(top, seq[t][c] + e) for c in range(C)]
        nlo = [max(lo[c], xl[c]) for c in range(C)]
        nhi = [min(hi[c], xh[c]) for c in range(C)]
        if any(nlo[c] > nhi[c] for c in range(C)):
            close(t)
            first = t
            starts.append(t)
            lo, hi = xl, xh
        else:
            lo, hi = nlo, nhi
    close(len(seq))
    return out, starts


@pytest.mark.parametrize("starts", [(), (4,)], ids=["one_run", "two_runs"])
@pytest.mark.parametrize("e", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("C", [0, 3, 4])
def test_reference_properties(C, dtype, e, starts):
    x = random_clip(11 + C, 9, 6, 11, C, dtype)
    y, bits = lookahead_ref(x, starts, e)
    assert y.dtype == x.dtype and y.shape == x.shape and not np.shares_memory(y, x)
    assert int(np.abs(y.astype(np.int64) - x.astype(np.int64)).max()) <= e, "the bound holds on every sample"
    for t in (0,) + tuple(starts):
        assert np.array_equal(y[t], x[t]) and not bits[t].any(), "run firsts are untouched"
    assert np.array_equal(all_channel_masks(y, starts), bits[1:].reshape(8, -1)), "the exact mask is the set of segment starts"
    assert (update_counts(y, starts) <= update_counts(hold_ref(x, starts, e), starts)).all(), "never more updates than the first-value hold"
    # the scalar transcription, pixel by pixel and run by run
    top = int(np.iinfo(dtype).max)
    xs = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    ys = y if y.ndim == 4 else y[..., None]
    cuts = [0] + list(starts) + [9]
    for a, b in zip(cuts, cuts[1:]):
        for i in range(6):
            for j in range(11):
                want, st = scalar_lookahead([tuple(int(s) for s in xs[t, i, j]) for t in range(a, b)], e, top)
                assert [tuple(int(s) for s in ys[t, i, j]) for t in range(a, b)] == want, (a, i, j)
                assert [a + t for t in st] == [t for t in range(a, b) if bits[t, i, j]], (a, i, j)


def test_reference_at_the_bound_and_the_range_ends():
    e = 3
    for top, dtype in ((255, np.uint8), (65535, np.uint16)):
        for J in (50, 0, top - 2 * e - 1):                    # mid-range | the window's floor clamps at 0 | its ceiling clamps at M
            x0 = J + 20 if J < 20 else J - 20
            seq = [x0, J, J + 2 * e, J, J + 2 * e + 1]
            x = np.array(seq, dtype=dtype).reshape(5, 1, 1)
            y, bits = lookahead_ref(x, (), e)
            assert [int(v) for v in y.reshape(-1)] == [x0, J + e, J + e, J + e, J + e + 1], (top, J)     # (the last segment's window is [J + e + 1, ..]: prev is clamped to its floor)
            assert [bool(b) for b in bits.reshape(-1)] == [False, True, False, False, True]
    x = np.array([0, 0x8000, 0x8000, 0], dtype=np.uint16).reshape(4, 1, 1)
    y, bits = lookahead_ref(x, (), 0x7FFF)
    assert [int(v) for v in y.reshape(-1)] == [0, 1, 1, 1], "0 and 0x8000 are 32768 apart: the windows [1, 65535] and [0, 32767] still meet"
    # one channel breaks: the whole pixel opens a segment, the other channels keep their value
    x = np.array([[10, 20, 30], [10, 20, 40], [11, 21, 40]], dtype=np.uint8).reshape(3, 1, 1, 3)
    y, bits = lookahead_ref(x, (), 2)
    assert bits.reshape(-1).tolist() == [False, True, False]
    assert y.reshape(3, 3).tolist() == [[10, 20, 30], [10, 20, 38], [10, 20, 38]]


def test_fewer_updates_than_the_hold_on_camera_noise():
    x = np.stack(make_camera_gop(2026, 96, 64, 12, sensor_noise=1))
    y, bits = lookahead_ref(x, (), 1)
    look, first = int(update_counts(y, ()).sum()), int(update_counts(hold_ref(x, (), 1), ()).sum())
    assert look == int(bits.sum()) and look < first, (look, first)


def test_not_idempotent():
    x = np.array([10, 13, 16, 19], dtype=np.uint8).reshape(4, 1, 1)
    y, _ = lookahead_ref(x, (), 1)
    z, _ = lookahead_ref(y, (), 1)
    assert int(np.abs(y.astype(int) - x.astype(int)).max()) <= 1
    assert y.reshape(-1).tolist() == [10, 12, 15, 18] and not np.array_equal(z, y), "stabbing the output again merges segments"


# ------------------------------------------------------------------ the Python layers
def test_constructors_validate_hold_mode():
    for bad in ("next", "", None, 1, "FIRST"):
        with pytest.raises(ValueError, match="hold_mode"):
            ImprovedVideoCompressor(mask_channels="all", max_error=1, hold_mode=bad)
        with pytest.raises(ValueError, match="hold_mode"):
            GopCoder(None, 8, 8, 3, channels=3, mask_channels=3, max_error=1, hold_mode=bad)
    with pytest.raises(ValueError, match="max_error"):
        ImprovedVideoCompressor(mask_channels="all", hold_mode="lookahead")
    with pytest.raises(ValueError, match="max_error"):
        GopCoder(None, 8, 8, 3, channels=3, mask_channels=3, hold_mode="lookahead")
    with pytest.raises(ValueError, match="mask_channels"):       # today's conditions of max_error > 0 apply unchanged
        ImprovedVideoCompressor(max_error=1, hold_mode="lookahead")
    with pytest.raises(ValueError, match="gop_batching"):
        ImprovedVideoCompressor(mask_channels="all", max_error=1, hold_mode="lookahead", gop_batching=False)
    with pytest.raises(ValueError, match="planar_luma"):
        GopCoder(None, 8, 8, 3, channels=3, mask_channels=3, max_error=1, hold_mode="lookahead", planar_luma=True)
    for kw in (dict(), dict(hold_mode="first"), dict(max_error=1, mask_channels="all"), dict(max_error=1, mask_channels="all", hold_mode="lookahead")):
        comp = ImprovedVideoCompressor(**kw)
        assert comp.hold_mode == kw.get("hold_mode", "first")
        comp.close()


# ------------------------------------------------------------------ the library
def test_entry_in_header_bindings_and_library():
    name = "rbf_temporal_lookahead_runs"
    hdr = open(os.path.join(REPO, "include", "rbf.h"), encoding="utf-8").read()
    so = os.path.join(REPO, "new_bloom_filter_repo_amd", "librbf_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in nat.exported_symbols()
    assert re.search(r"\bT %s\b" % name, syms)
    assert nat._PROTOS[name] == nat._PROTOS["rbf_temporal_hold_runs"], "the hold's signature"
    assert int(re.search(r"#define\s+RBF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4, "additive: the ABI version stays"
    assert name in open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8").read()


def test_lookahead_kernels_use_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900, check=True).stdout
    rows = [ln.split() for ln in out.splitlines() if ln.startswith(("k_temporal_lookahead", "k_lookahead_fill"))]
    names = {" ".join(r[:-6]) for r in rows}
    want = {"%s<unsigned %s, %d>" % (k, s, c) for k in ("k_temporal_lookahead", "k_lookahead_fill") for s in ("char", "short") for c in (1, 2, 3, 4)}
    want |= {"k_temporal_lookahead_px<unsigned char>", "k_temporal_lookahead_px<unsigned short>"}
    assert names == want, names ^ want
    for r in rows:
        assert r[-4] == "0" and r[-3] == "0", r             # scratch bytes, VGPR spills
