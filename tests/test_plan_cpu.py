"""The launch planner (csrc/rbf_plan.h) keeps the decisions its comments justify with measurements: slices per frame, the tile counts at
which a filter leaves the LDS kernels (MAX_INSERT_TILES / MAX_QUERY_TILES), which frame sizes take the two-phase insert and which
query kernel.  A change of one of them costs speed without failing any other test (the same kind of silent change
tests/test_kernel_resources_cpu.py guards against).  The planner is pure host code: tests/c/plan_cases.cpp is cross-compiled with
hipcc and runs without a GPU.

Where the expected values come from: the planner of the commit BEFORE the host layer was split into headers (make_plan inside
rbf_api.hip, run on the CPU over the same cases), not from the code under test.  `ones = int(p * n)` for every frame."""
import ctypes
import os
import shutil
import subprocess

import pytest

from new_bloom_filter_repo_amd import _native as nat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# query: 0 generic (k_query), 1 whole filter in LDS (k_query_u64 with probe_image=1, else k_query_lds), 2 k_query_tiled, 3 k_query_s64t
# name, n, frames, p, CUs, rbf_ctx_force_generic flags, RBF_OPT_INSERT_SLICES, counts known, p of frame 0 (mixed batch), m, expected lines
CASES = [
    ("1080p", 2073600, 29, 0.0889, 256, 0, 0, 0, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("1080p_ones", 2073600, 29, 0.0889, 256, 0, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("1080p_4gops", 2073600, 116, 0.0889, 256, 0, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=2 per_tile=232 insert_group=116 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("1440p", 3686400, 29, 0.0889, 256, 0, 0, 0, None, 1087357, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=16 insert_tile_words=24064 insert_tiles=2 query_tile_words=33980 insert_lds=163840 query_lds=135936 nseg=7200 words_per_seg=8",
    }),
    ("1440p_ones", 3686400, 29, 0.0889, 256, 0, 0, 1, None, 1087357, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=1 probe_image=1 S=8 per_tile=232 insert_group=29 insert_tile_words=33980 insert_tiles=1 query_tile_words=33980 insert_lds=135920 query_lds=135936 nseg=7200 words_per_seg=8",
    }),
    ("2160p", 8294400, 29, 0.0889, 256, 0, 0, 0, None, 2446557, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=8 insert_tile_words=24064 insert_tiles=4 query_tile_words=38228 insert_lds=163840 query_lds=152928 nseg=16200 words_per_seg=8",
    }),
    ("2160p_ones", 8294400, 29, 0.0889, 256, 0, 0, 1, None, 2446557, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=1 probe_image=1 S=8 per_tile=232 insert_group=16 insert_tile_words=38228 insert_tiles=2 query_tile_words=38228 insert_lds=152912 query_lds=152928 nseg=16200 words_per_seg=8",
    }),
    ("180p", 57600, 29, 0.07, 256, 0, 0, 0, None, 15556, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=488 insert_tiles=1 query_tile_words=0 insert_lds=69536 query_lds=3904 nseg=113 words_per_seg=8",
    }),
    ("1080p_static", 2073600, 29, 0.0005, 256, 0, 0, 0, None, 14809, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=464 insert_tiles=1 query_tile_words=0 insert_lds=69440 query_lds=3712 nseg=4050 words_per_seg=8",
    }),
    ("1080p_mixed", 2073600, 29, 0.0889, 256, 0, 0, 1, 0.0005, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152928 nseg=4050 words_per_seg=8",
        "small": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=32 per_tile=32 insert_group=1 insert_tile_words=464 insert_tiles=1 query_tile_words=0 insert_lds=69440 query_lds=3712 nseg=4050 words_per_seg=8",
        "big": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=224 insert_group=28 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("1080p_force_generic", 2073600, 29, 0.0889, 256, 1, 0, 1, None, 611639, {
        "plan": "fast_insert=0 query=0 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=0 nseg=2025 words_per_seg=16",
    }),
    ("1080p_single_buffer", 2073600, 29, 0.0889, 256, 2, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=0 insert_tab=1 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=76464 nseg=4050 words_per_seg=8",
    }),
    ("1080p_barrett_only", 2073600, 29, 0.0889, 256, 8, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=0 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152928 nseg=4050 words_per_seg=8",
    }),
    ("1080p_no_hash_table", 2073600, 29, 0.0889, 256, 32, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=0 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("2160p_no_two_phase", 8294400, 29, 0.0889, 256, 128, 0, 1, None, 2446557, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=8 insert_tile_words=24064 insert_tiles=4 query_tile_words=38228 insert_lds=163840 query_lds=152928 nseg=16200 words_per_seg=8",
    }),
    ("1080p_tile_1KiB", 2073600, 29, 0.0889, 256, 0x40000, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=3 double_buffer=1 insert_tab=1 two_phase=1 probe_image=1 S=3 per_tile=87 insert_group=1 insert_tile_words=256 insert_tiles=75 query_tile_words=256 insert_lds=1024 query_lds=1040 nseg=4050 words_per_seg=8",
    }),
    ("1080p_tile_8KiB", 2073600, 29, 0.0889, 256, 0x200000, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=3 double_buffer=1 insert_tab=1 two_phase=1 probe_image=1 S=8 per_tile=232 insert_group=3 insert_tile_words=2048 insert_tiles=10 query_tile_words=2048 insert_lds=8192 query_lds=8208 nseg=4050 words_per_seg=8",
    }),
    ("1080p_tile_8KiB_insert_tab", 2073600, 29, 0.0889, 256, 0x200080, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=3 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=8 per_tile=232 insert_group=3 insert_tile_words=2048 insert_tiles=10 query_tile_words=2048 insert_lds=75776 query_lds=8208 nseg=4050 words_per_seg=8",
    }),
    ("16K", 132710400, 4, 0.0889, 256, 0, 0, 1, None, 39144914, {
        "plan": "fast_insert=0 query=0 double_buffer=0 insert_tab=0 two_phase=0 probe_image=0 S=5 per_tile=20 insert_group=1 insert_tile_words=24064 insert_tiles=51 query_tile_words=40960 insert_lds=163840 query_lds=163840 nseg=129600 words_per_seg=16",
    }),
    ("1080p_120cus", 2073600, 29, 0.0889, 120, 0, 0, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=4 per_tile=116 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
    ("2160p_120cus", 8294400, 29, 0.0889, 120, 0, 0, 1, None, 2446557, {
        "plan": "fast_insert=1 query=3 double_buffer=0 insert_tab=1 two_phase=1 probe_image=1 S=8 per_tile=232 insert_group=7 insert_tile_words=38228 insert_tiles=2 query_tile_words=38228 insert_lds=152912 query_lds=152928 nseg=16200 words_per_seg=8",
    }),
    ("1080p_insert_slices_4", 2073600, 29, 0.0889, 256, 0, 4, 1, None, 611639, {
        "plan": "fast_insert=1 query=1 double_buffer=1 insert_tab=1 two_phase=0 probe_image=1 S=4 per_tile=116 insert_group=29 insert_tile_words=19116 insert_tiles=1 query_tile_words=0 insert_lds=144048 query_lds=152960 nseg=4050 words_per_seg=8",
    }),
]


@pytest.fixture(scope="module")
def plan_cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_cases")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror",
                        os.path.join(REPO, "tests", "c", "plan_cases.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def filter_bits(n, p):
    ones = (ctypes.c_uint64 * 1)(int(p * n))
    par = (nat.FilterParams * 1)()
    assert nat.lib().rbf_plan_batch(n, ones, 1, 1, par, None) == 0
    return par[0].m


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planner_decisions(plan_cases, case):
    _, n, frames, p, cus, flags, slices, have_ones, p0, m, want = case
    assert filter_bits(n, p) == m
    line = "%d %d %d %d %d %d %d" % (n, frames, cus, flags, slices, have_ones, m)
    if p0 is not None:
        line += " %d" % filter_bits(n, p0)
    out = subprocess.run([plan_cases], input=line + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = {}
    for ln in out.stdout.splitlines():
        tag, *fields = ln.split()
        got[tag] = dict(f.split("=") for f in fields)
    assert sorted(got) == sorted(want), out.stdout
    for tag, text in want.items():
        for field in text.split():
            key, value = field.split("=")
            assert got[tag][key] == value, (tag, key, got[tag][key], value)
    coded = frames - 1 if p0 is not None else frames            # slices: S for every coded frame of the plan, none for the others
    for tag in got:
        s = [int(x, 16) for x in got[tag]["slices"].strip(",").split(",")]
        count = {"plan": frames, "small": 1, "big": coded}[tag]
        assert len(s) == frames and sorted(s) == [0] * (frames - count) + [int(got[tag]["S"])] * count, (tag, s)


def test_mixed_batch_splits_into_halves_that_share_their_segments(plan_cases):
    """One nearly static frame among 28 ordinary ones: undivided the batch falls back to the Barrett kernels (no probe image, no table
    insert); split, the 28 keep the FP64 kernels, and both halves cut the frame into the same segments -- the condition under which
    encode and decode run the split."""
    want = next(c for c in CASES if c[0] == "1080p_mixed")[-1]
    whole, small, big = (dict(f.split("=") for f in want[t].split()) for t in ("plan", "small", "big"))
    assert whole["probe_image"] == "0" and whole["insert_tab"] == "0"
    assert big["probe_image"] == "1" and big["insert_tab"] == "1" and big["query"] == "1"
    assert (small["nseg"], small["words_per_seg"]) == (big["nseg"], big["words_per_seg"]) == (whole["nseg"], whole["words_per_seg"])
