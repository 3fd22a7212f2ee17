"""Frame views without a GPU: the numpy twin (view.view_host) against the naive reference (view_ref.py) over every geometry, channel
count, depth, scale and region of the sweep; the rounding pinned in both directions; every sweep input told apart from the views a
wrong kernel would compute; the C twin of csrc/rbf_view.h -- the header the kernels include -- under a plain g++; container.read_span
on hand-written type lists; and the library side: the entry is declared, bound and exported, the RBF_K_ count stays, no view kernel
spills."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from view_ref import CHANNELS, DTYPES, GEOMETRIES, SCALES, noise_frame, regions, view_ref, view_ref_stack
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.container import INTER, INTER_RICE, KEY, KEY_NEAR, KEY_RICE, read_span, span_records
from new_bloom_filter_repo_amd.view import View, check_region, view_host, view_shape

GXX = shutil.which("g++")


def sweep():
    for gi, (W, H) in enumerate(GEOMETRIES):
        for C in CHANNELS:
            for dtype in DTYPES:
                yield W, H, C, dtype, 1000 * gi + 10 * C + np.dtype(dtype).itemsize


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("W,H", GEOMETRIES)
def test_view_host_equals_the_naive_reference(W, H):
    for w_, h_, C, dtype, seed in sweep():
        if (w_, h_) != (W, H):
            continue
        a = noise_frame(W, H, C, dtype, seed)
        for s in SCALES:
            for roi in regions(W, H, s):
                got = view_host(a, roi, s)
                want = view_ref(a, roi, s)
                assert got.dtype == a.dtype and got.shape == want.shape == view_shape(roi, s, a.shape), (roi, s, got.shape)
                assert np.array_equal(got, want), (W, H, C, dtype, roi, s)
        assert np.array_equal(view_host(a), a) and np.array_equal(view_host(a, None, 1), view_ref(a))


def test_stack_reference_equals_the_naive_reference():
    frames = [noise_frame(37, 9, 3, np.uint16, 50 + i) for i in range(3)]
    for s in SCALES:
        for roi in regions(37, 9, s):
            got = view_ref_stack(frames, roi, s)
            assert all(np.array_equal(got[i], view_ref(f, roi, s)) for i, f in enumerate(frames)), (roi, s)


def test_rounding_is_pinned_in_both_directions():
    for dtype in DTYPES:
        top = np.iinfo(dtype).max
        for q in (0, 1, 100, top - 1):
            up = np.array([[q, q + 1], [q + 1, q]], dtype=dtype)           # 4q + 2 -> q + 1
            down = np.array([[q, q], [q + 1, q]], dtype=dtype)             # 4q + 1 -> q
            for f in (view_host, view_ref):
                assert f(up, None, 2).tolist() == [[q + 1]] and f(down, None, 2).tolist() == [[q]], (dtype, q)
            # a ragged block of 3 pixels: a 3 x 1 frame at scale 4
            low = np.array([[q, q + 1, q]], dtype=dtype)                   # 3q + 1 -> q
            high = np.array([[q + 1, q, q + 1]], dtype=dtype)              # 3q + 2 -> q + 1
            for f in (view_host, view_ref):
                assert f(low, None, 4).tolist() == [[q]] and f(high, None, 4).tolist() == [[q + 1]], (dtype, q)
    full = np.full((8, 8, 3), 65535, dtype=np.uint16)                      # the sum is 64 * 65535: a 16-bit (or 22-bit) sum would wrap
    assert view_host(full, None, 8).tolist() == [[[65535] * 3]] == view_ref(full, None, 8).tolist()
    assert (64 * 65535) % 65536 != 64 * 65535


def test_sweep_inputs_tell_wrong_kernels_apart():
    """Non-vacuity: for every input of the sweep with the room for it, the view differs from the view one pixel off in x and in y, from
    the floor-rounded view and from the view whose ragged blocks are divided by s^2 -- a kernel that ignores x0 or y0, truncates or
    divides by the full block is caught by the data, not only by the shapes."""
    told = {"x": 0, "y": 0, "floor": 0, "ragged": 0}
    for W, H, C, dtype, seed in sweep():
        a = noise_frame(W, H, C, dtype, seed)
        for s in SCALES:
            for x0, y0, w, h in regions(W, H, s):
                want = view_ref(a, (x0, y0, w, h), s)
                if x0 + w < W and want.size >= 16:                         # (enough output samples that one of them moves: a mean of 64 can stay)
                    assert not np.array_equal(want, view_ref(a, (x0 + 1, y0, w, h), s)), ("x0", W, H, C, s)
                    told["x"] += 1
                if y0 + h < H and want.size >= 16:
                    assert not np.array_equal(want, view_ref(a, (x0, y0 + 1, w, h), s)), ("y0", W, H, C, s)
                    told["y"] += 1
                if s > 1 and want.size >= 16:                              # (enough output samples that one of them rounds up: each does with probability 1/2)
                    assert not np.array_equal(want, view_ref(a, (x0, y0, w, h), s, rounding="floor")), ("floor", W, H, C, s)
                    told["floor"] += 1
                if s > 1 and (w % s or h % s):                             # (a ragged block of noise never sums to zero)
                    assert not np.array_equal(want, view_ref(a, (x0, y0, w, h), s, ragged_div="full")), ("ragged", W, H, C, s)
                    told["ragged"] += 1
    assert all(v > 50 for v in told.values()), told


def test_regions_and_scales_are_checked():
    a = np.zeros((9, 12, 3), np.uint8)
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (11, 0, 2, 1), (0, 8, 1, 2), (0, 0, 13, 1), (0, 0), "abcd", (0, 0, 1.5, 2),
                (True, 0, 1, 1)):
        with pytest.raises(ValueError):
            view_host(a, bad, 1)
    for bad in (0, 3, 5, 16, -1, 2.5, 2.0, np.float32(4), "2", None, True):
        with pytest.raises(ValueError):
            view_host(a, None, bad)
    with pytest.raises(ValueError):
        view_host(a.astype(np.float32))
    assert check_region(None, 4, 9, 12) == (0, 0, 12, 9)
    assert View((1, 2, 5, 3), 2).shape(a.shape) == (2, 3, 3)


# ------------------------------------------------------------------ the C twin, by a plain host compiler
@pytest.fixture(scope="module")
def view_cases(tmp_path_factory):
    if GXX is None:
        pytest.skip("g++ not found: tests/c/view_cases.cpp is built with a plain host compiler, not with hipcc")
    tmp = tmp_path_factory.mktemp("view")
    exe = str(tmp / "view_cases")
    r = subprocess.run([GXX, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror",
                        os.path.join(REPO, "tests", "c", "view_cases.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, tmp


def test_c_twin_self_check(view_cases):
    out = subprocess.run([view_cases[0], "check"], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"ok \d+\n", out.stdout), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) > 10000


def test_c_twin_equals_the_naive_reference(view_cases):
    exe, tmp = view_cases
    for W, H, C, dtype, s, roi in ((67, 33, 3, np.uint8, 4, (3, 1, 61, 30)), (37, 9, 4, np.uint16, 8, None), (16, 1, 1, np.uint8, 2, (1, 0, 15, 1)),
                                   (9, 9, 3, np.uint16, 1, (2, 3, 5, 4)), (1030, 2, 1, np.uint16, 2, None), (5, 3, 4, np.uint8, 8, None)):
        a = noise_frame(W, H, C, dtype, W + H)
        path = str(tmp / "frame.bin")
        a.tofile(path)
        x0, y0, w, h = roi or (0, 0, W, H)
        out = subprocess.run([exe, "view", path] + [str(v) for v in (a.dtype.itemsize, W, H, C, x0, y0, w, h, s)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert [int(v) for v in out.stdout.split()] == view_ref(a, roi, s).reshape(-1).tolist(), (W, H, C, dtype, s, roi)


def test_c_plan_says_which_kernel_takes_what(view_cases):
    exe, _ = view_cases

    def plan(*args):
        out = subprocess.run([exe, "plan"] + [str(v) for v in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return tuple(int(v) for v in out.stdout.split())          # out_w out_h tile tiles_x wide_cols wide_rows
    assert plan(1920, 3, 0, 1920, 1080, 4, 1) == (480, 270, 4, 120, 480, 270)        # 1080p YUV444 at a quarter: the wide kernel alone
    assert plan(1920, 3, 0, 1920, 1080, 1, 1) == (1920, 1080, 16, 120, 1920, 1080)
    assert plan(96, 3, 0, 96, 64, 2, 1) == (48, 32, 8, 6, 48, 32)
    assert plan(96, 3, 16, 75, 61, 2, 1) == (38, 31, 8, 4, 32, 30)                   # both kernels in one call: tail columns and a ragged row
    assert plan(96, 3, 1, 64, 64, 2, 1)[3:] == (0, 0, 0)                             # an odd corner: rows no longer start on 16 bytes
    assert plan(67, 3, 0, 67, 33, 2, 1)[3:] == (0, 0, 0)                             # 201-byte rows
    assert plan(96, 3, 0, 96, 64, 2, 0)[3:] == (0, 0, 0)                             # base or stride not 16-byte shaped
    assert plan(96, 6, 0, 96, 1, 8, 1) == (12, 1, 1, 0, 0, 0)                        # no full row of blocks


@pytest.mark.skipif(GXX is None, reason="g++ not found")
def test_c_twin_is_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, host code only, with AddressSanitizer and UBSan linked in: its own main runs it, nothing is preloaded."""
    exe = str(tmp_path / "view_cases_san")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([GXX] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this g++ cannot link the sanitizer runtimes")     # (decided on a one-line program: a failure of the real build below is a failure)
    r = subprocess.run([GXX] + flags + [os.path.join(REPO, "tests", "c", "view_cases.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    a = noise_frame(37, 9, 3, np.uint16, 7)
    path = str(tmp_path / "frame.bin")
    a.tofile(path)
    out = subprocess.run([exe, "view", path, "2", "37", "9", "3", "1", "1", "36", "8", "8"], capture_output=True, text=True)
    assert out.returncode == 0 and [int(v) for v in out.stdout.split()] == view_ref(a, (1, 1, 36, 8), 8).reshape(-1).tolist(), out.stderr[-4000:]


# ------------------------------------------------------------------ span planning
K, I, K3, I4, K7 = KEY, INTER, KEY_RICE, INTER_RICE, KEY_NEAR


def gops(key, inter, count, interval):
    return [key if t % interval == 0 else inter for t in range(count)]


def test_read_span_inside_one_run():
    types = gops(K3, I4, 45, 15)
    assert read_span(types, 20, 27) == ([], [(15, 16, 27, list(range(4, 11)))])
    assert span_records(*read_span(types, 20, 27)) == 1 + 11


def test_read_span_across_three_runs():
    types = gops(K, I, 45, 15)
    keys, runs = read_span(types, 10, 35)
    assert keys == [15, 30]
    assert runs == [(0, 1, 15, [9, 10, 11, 12, 13]), (15, 16, 30, list(range(14))), (30, 31, 35, [0, 1, 2, 3])]
    assert span_records(keys, runs) == 15 + 15 + 5
    assert read_span(types, 20, 37) == ([30], [(15, 16, 30, list(range(4, 14))), (30, 31, 37, list(range(6)))])
    assert span_records(*read_span(types, 20, 37)) == 15 + 7 == 22


def test_read_span_ending_on_a_keyframe():
    types = gops(K3, I4, 45, 15)
    assert read_span(types, 14, 16) == ([15], [(0, 1, 15, [13])])
    assert span_records(*read_span(types, 14, 16)) == 15 + 1          # the first run whole, and the keyframe behind it
    assert read_span(types, 12, 15) == ([], [(0, 1, 15, [11, 12, 13])])


def test_read_span_lone_keyframes_and_cuts():
    types = [K3, I4, I4, K7, K3, I4, K7, I4, I4, I4, K3]              # lone type-7 at 3, a cut keyframe at 6 off the interval, a lone type-3 last
    assert container.inter_runs(types) == [(0, 1, 3), (4, 5, 6), (6, 7, 10)]
    assert read_span(types) == ([0, 3, 4, 6, 10], [(0, 1, 3, [0, 1]), (4, 5, 6, [0]), (6, 7, 10, [0, 1, 2])])
    assert span_records(*read_span(types)) == len(types)
    assert read_span(types, 3, 4) == ([3], [])
    assert read_span(types, 10, None) == ([10], []) and span_records([10], []) == 1
    assert read_span(types, 6, 9) == ([6], [(6, 7, 9, [0, 1])])
    assert read_span(types, 8, 9) == ([], [(6, 7, 9, [1])]) and span_records(*read_span(types, 8, 9)) == 3


def test_read_span_step_skips_whole_runs():
    types = gops(K, I4, 45, 5)
    keys, runs = read_span(types, 3, 45, 7)                            # 3, 10, 17, 24, 31, 38
    assert keys == [10] and runs == [(0, 1, 4, [2]), (15, 16, 18, [1]), (20, 21, 25, [3]), (30, 31, 32, [0]), (35, 36, 39, [2])]
    assert span_records(keys, runs) == 1 + 4 + 3 + 5 + 2 + 4
    keys, runs = read_span(gops(K3, I4, 45, 15), 3, 45, 7)
    assert keys == [] and runs == [(0, 1, 11, [2, 9]), (15, 16, 25, [1, 8]), (30, 31, 39, [0, 7])]
    assert read_span(gops(K, I, 40, 4), 0, None, 8) == ([0, 8, 16, 24, 32], [])      # only keyframes: no run takes a lane


def test_read_span_single_frames_and_clamping():
    assert read_span([K]) == ([0], []) and read_span([K3], 0, 1, 1) == ([0], []) and read_span([K7], 0, 99, 5) == ([0], [])
    types = gops(K, I, 45, 15)
    assert read_span(types, 44, 45) == ([], [(30, 31, 45, [13])])
    assert read_span(types, 15, 16) == ([15], [])                     # a span holding only a keyframe
    assert read_span(types, 40, 1000) == read_span(types, 40, None) == read_span(types, 40, 45)
    for bad in (dict(step=0), dict(step=-1), dict(start=-1), dict(start=45), dict(start=10, stop=10), dict(start=10, stop=3), dict(start=100, stop=None),
                dict(start=1.5), dict(step=True)):
        with pytest.raises(ValueError):
            read_span(types, **bad)


# ------------------------------------------------------------------ header, binding, library
def test_entry_is_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "rbf.h")) as f:
        hdr = f.read()
    m = re.search(r"\bint\s+rbf_frame_view_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m and m.group(1).count(",") + 1 == 16 == len(nat._PROTOS["rbf_frame_view_batch"][1])
    assert nat._PROTOS["rbf_frame_view_batch"] == (nat._int, [nat._vp, nat._vp, nat._u64, nat.ctypes.POINTER(nat._u32), nat._u32] + [nat._u32] * 9
                                                   + [nat._vp, nat._u64])
    ids = re.findall(r"#define\s+(RBF_K_\w+)\s+(\d+)", hdr)
    assert len(ids) == 15 and dict(ids)["RBF_K_COUNT"] == "14", "no new RBF_K_ id: untimed, like rbf_cut_stats"
    assert len(nat.KERNEL_NAMES) == 14 and int(re.search(r"#define\s+RBF_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert hasattr(nat.lib(), "rbf_frame_view_batch")
    with open(os.path.join(REPO, "new_bloom_filter_repo_amd", "csrc", "rbf_api.hip")) as f:
        api = f.read()
    assert '#include "rbf_kernels_view.h"' in api
    with open(os.path.join(REPO, "new_bloom_filter_repo_amd", "csrc", "rbf_view.h")) as f:
        assert "hip" not in f.read().replace("__HIPCC__", "").replace("hipcc", "").lower().replace("no hip header", ""), "the arithmetic header takes any host compiler"


def test_view_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if ln.startswith("k_frame_view")]
    assert len([r for r in rows if r.startswith("k_frame_view<")]) == 32 and len([r for r in rows if r.startswith("k_frame_view_px<")]) == 8, rows
    for ln in rows:
        vgprs, _, scratch, spills = ln.split()[-6:-2]                 # the six columns behind the name: VGPRs, SGPRs, scratch, spills, waves/SIMD, LDS
        assert scratch == "0" and spills == "0" and int(vgprs) <= 128, ln
