"""The dense-block stages' host arithmetic without a GPU: csrc/rbf_block_plan.h -- the header the entry points of rbf_api.hip stand on --
built with a plain g++ (tests/c/block_plan_cases.cpp).  The lane split against block_layout.LaneShape, the mirror the GPU sweeps place
their frames by; the block checks against a table of codes written down from the entry points as they were before they shared the header;
the run walk against a five-line walk, over every marking of eight frames."""
import os
import re
import shutil
import subprocess

import pytest

from block_layout import WG_THREADS, LaneShape
from conftest import REPO

GXX = shutil.which("g++")
SRC = os.path.join(REPO, "tests", "c", "block_plan_cases.cpp")
CSRC = os.path.join(REPO, "new_bloom_filter_repo_amd", "csrc")
OK, EINVAL, ERANGE = 0, -22, -34
NMAX = 4200


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    if GXX is None:
        pytest.skip("g++ not found: tests/c/block_plan_cases.cpp is built with a plain host compiler, not with hipcc")
    exe = str(tmp_path_factory.mktemp("block_plan") / "block_plan_cases")
    r = subprocess.run([GXX, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, (args[:3], out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def test_self_check(cases):
    out = run(cases, "check")
    assert re.fullmatch(r"ok \d+\n", out) and int(out.split()[1]) > 200000, out[-2000:]


# ------------------------------------------------------------------ the lane split
@pytest.mark.parametrize("unit", [8, 16])
@pytest.mark.parametrize("vec", [0, 1])
def test_lane_split_equals_lane_shape(cases, unit, vec):
    """hold, look-ahead, cut statistics, quality report: lanes of `unit` pixels, 256 to a workgroup, four rows of partial sums each."""
    rows = [[int(v) for v in ln.split()] for ln in run(cases, "splits", unit, WG_THREADS, WG_THREADS, 4, vec, NMAX).splitlines()]
    assert len(rows) == NMAX
    crossed = set()
    for n, (units, first_px, bx_vec, bx_px, nrows, tail_row_base) in enumerate(rows, start=1):
        shape = LaneShape(n, unit)
        lanes, first_tail, workgroups = (shape.lanes, shape.first_tail, shape.workgroups) if vec else (0, 0, 0)
        assert (units, first_px, bx_vec) == (lanes, first_tail, workgroups), n
        assert first_px + (shape.tail()[1] - first_tail) == n and first_px % unit == 0
        assert bx_px == -(-(n - first_tail) // WG_THREADS) and nrows == (bx_vec + bx_px) * 4 and tail_row_base == bx_vec * 4, n
        if vec and bx_vec:
            assert shape.workgroup(bx_vec - 1)[1] == first_px and shape.workgroup(bx_vec - 1)[0] < first_px, n       # the last workgroup is not empty
        crossed.add((bx_vec, bx_px))
    if vec:
        assert {b for b, _ in crossed} == ({0, 1, 2, 3} if unit == 8 else {0, 1, 2})       # the range crosses one and two workgroups of lanes
    else:
        assert max(p for _, p in crossed) == -(-NMAX // WG_THREADS) == 17


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("vec", [0, 1])
def test_sweep_split_is_the_same_function(cases, tile, vec):
    """The hold sweep: the unit is a workgroup's tile of 256 / groups pixels, one to a workgroup; the tail takes a tile's worth of pixels
    per workgroup; a row per wave of the tile."""
    rows = [[int(v) for v in ln.split()] for ln in run(cases, "splits", tile, 1, tile, tile // 64, vec, NMAX).splitlines()]
    for n, (units, first_px, bx_vec, bx_px, nrows, tail_row_base) in enumerate(rows, start=1):
        shape = LaneShape(n, tile)
        tiles = shape.lanes if vec else 0
        assert (units, bx_vec, first_px) == (tiles, tiles, tiles * tile) and first_px == (shape.first_tail if vec else 0), n
        assert bx_px == -(-(n - first_px) // tile) and (bx_px <= 1 if vec else True), n
        assert nrows == (tiles + bx_px) * (tile // 64) and tail_row_base == tiles * (tile // 64), n


# ------------------------------------------------------------------ the block checks
W, H = 8, 4
A = 0x7F0000001000          # a base: aligned for everything
# (channels, sample bytes, stride, frames, base, the entry waives the stride of a single frame) -> (check_block_shape, check_block_at);
# the codes as rbf_api.hip's entry points returned them when each carried its own copy: check_layout's for the shape, "frames
# misaligned" and "frame stride ... smaller than a frame" behind it.  None: not reached.
BLOCK_TABLE = [
    # channels 0..5 at one byte
    ((0, 1, 32, 3, A, 0), (EINVAL, None)), ((1, 1, 32, 3, A, 0), (OK, OK)), ((2, 1, 64, 3, A, 0), (OK, OK)), ((3, 1, 96, 3, A, 0), (OK, OK)),
    ((4, 1, 128, 3, A, 0), (OK, OK)), ((5, 1, 160, 3, A, 0), (EINVAL, None)),
    # ... and at two
    ((0, 2, 64, 3, A, 0), (EINVAL, None)), ((1, 2, 64, 3, A, 0), (OK, OK)), ((2, 2, 128, 3, A, 0), (OK, OK)), ((3, 2, 192, 3, A, 0), (OK, OK)),
    ((4, 2, 256, 3, A, 0), (OK, OK)), ((5, 2, 320, 3, A, 0), (EINVAL, None)),
    # sample bytes 0..3
    ((1, 0, 32, 3, A, 0), (EINVAL, None)), ((3, 0, 96, 3, A, 0), (EINVAL, None)), ((1, 3, 96, 3, A, 0), (EINVAL, None)), ((3, 3, 288, 3, A, 0), (EINVAL, None)),
    ((0, 0, 0, 3, A, 0), (EINVAL, None)), ((5, 3, 480, 3, A, 0), (EINVAL, None)),
    # the stride: one byte short, exact, padded
    ((3, 1, 95, 3, A, 0), (OK, EINVAL)), ((3, 1, 96, 3, A, 0), (OK, OK)), ((3, 1, 97, 3, A, 0), (OK, OK)), ((3, 1, 4096, 3, A, 0), (OK, OK)),
    ((1, 1, 31, 2, A, 0), (OK, EINVAL)), ((1, 1, 33, 2, A, 0), (OK, OK)), ((3, 1, 0, 3, A, 0), (OK, EINVAL)),
    # ... of two-byte samples: an odd stride is the shape's ("frame stride misaligned"), one sample short is the block's
    ((3, 2, 191, 3, A, 0), (EINVAL, None)), ((3, 2, 193, 3, A, 0), (EINVAL, None)), ((3, 2, 190, 3, A, 0), (OK, EINVAL)), ((3, 2, 192, 3, A, 0), (OK, OK)),
    ((3, 2, 194, 3, A, 0), (OK, OK)),
    # the waiver: a single frame's stride is not looked at by rbf_error_stats, rbf_roll_frames, rbf_frame_digest_batch; by the others it is
    ((3, 1, 95, 1, A, 1), (OK, OK)), ((3, 1, 95, 2, A, 1), (OK, EINVAL)), ((3, 1, 95, 1, A, 0), (OK, EINVAL)), ((3, 1, 95, 2, A, 0), (OK, EINVAL)),
    ((3, 1, 0, 1, A, 1), (OK, OK)), ((3, 2, 190, 1, A, 1), (OK, OK)), ((3, 2, 190, 2, A, 1), (OK, EINVAL)), ((3, 2, 190, 1, A, 0), (OK, EINVAL)),
    ((3, 2, 191, 1, A, 1), (EINVAL, None)),                      # (an odd stride stays the shape's, waiver or not)
    ((3, 1, 95, 0, A, 1), (OK, OK)), ((3, 1, 95, 0, A, 0), (OK, EINVAL)),      # (no frame: as `frames > 1 && ...` had it; the entries return before they ask)
    # the base: off by one
    ((3, 2, 192, 3, A + 1, 0), (OK, EINVAL)), ((1, 2, 64, 3, A + 1, 0), (OK, EINVAL)), ((3, 2, 192, 3, A + 2, 0), (OK, OK)), ((3, 1, 96, 3, A + 1, 0), (OK, OK)),
    ((3, 2, 192, 1, A + 1, 1), (OK, EINVAL)), ((3, 2, 190, 1, A + 1, 1), (OK, EINVAL)), ((5, 2, 320, 3, A + 1, 0), (EINVAL, None)),
]


def test_block_checks_return_the_entry_points_codes(cases):
    out = run(cases, "block", *["%d,%d,%d,%d,%d,%d,%d,%d" % (W, H, c, sb, stride, frames, base, waive) for (c, sb, stride, frames, base, waive), _ in BLOCK_TABLE])
    lines = out.splitlines()
    assert len(lines) == len(BLOCK_TABLE)
    for (row, (shape, at)), ln in zip(BLOCK_TABLE, lines):
        got_shape, got_at, text = ln.split()
        assert int(got_shape) == shape and (got_at == "-" if at is None else int(got_at) == at), (row, ln)
        assert int(text) == (1 if shape or at else 0), (row, ln)                      # a refusal leaves a text
    # an empty frame is the shape's too
    assert run(cases, "block", "0,4,3,1,96,3,%d,0" % A, "8,0,3,1,96,3,%d,0" % A).split() == ["-22", "-", "1"] * 2
    assert {c for (c, _, _, _, _, _), _ in BLOCK_TABLE} == set(range(6)) and {sb for (_, sb, _, _, _, _), _ in BLOCK_TABLE} == set(range(4))


def test_the_two_texts_live_in_one_place():
    """What the entry points used to carry a copy of each."""
    text = ""
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            text += f.read()
    assert text.count("frames misaligned for") == 1 and text.count("smaller than a frame of") == 1
    with open(os.path.join(CSRC, "rbf_block_plan.h"), encoding="utf-8") as f:
        hdr = f.read()
    assert "frames misaligned for" in hdr and "smaller than a frame of" in hdr
    assert "hip" not in hdr.lower().replace("no hip header", "").replace("rbf_api.hip", ""), "the header takes any host compiler"


# ------------------------------------------------------------------ the run walk
def walk(marks, nframes):
    starts = [0] + [t for t in range(1, nframes) if marks is not None and marks[t]]
    return [(a, b - a) for a, b in zip(starts, starts[1:] + [nframes])]


def test_run_walk_over_every_marking_of_eight_frames(cases):
    F = 8
    markings = ["0" + format(m, "07b") for m in range(1 << 7)]
    set0 = ["1" + m[1:] for m in ("00000000", "00100100", "01111111")]                # frame 0's byte set: it changes nothing
    lines = run(cases, "runs", F, "null", *(markings + set0)).splitlines()
    assert len(lines) == 1 + len(markings) + len(set0)
    parse = lambda ln: [tuple(int(v) for v in run_.split(":")) for run_ in ln.split()]
    assert parse(lines[0]) == walk(None, F) == [(0, 8)]
    for m, ln in zip(markings + set0, lines[1:]):
        assert parse(ln) == walk([int(ch) for ch in m], F), m
    for m, ln in zip(set0, lines[1 + len(markings):]):
        assert ln == lines[1 + markings.index("0" + m[1:])]
    assert len({ln for ln in lines[1:1 + len(markings)]}) == 128                      # every marking is another walk
    assert run(cases, "runs", 1, "null", "0", "1").split() == ["0:1"] * 3


# ------------------------------------------------------------------ under the sanitizers
@pytest.mark.skipif(GXX is None, reason="g++ not found")
def test_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, host code only, with AddressSanitizer and UBSan linked in: its own main runs it, nothing is preloaded."""
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([GXX] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this g++ cannot link the sanitizer runtimes")     # (decided on a one-line program: a failure of the real build below is a failure)
    exe = str(tmp_path / "block_plan_cases_san")
    r = subprocess.run([GXX] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert run(exe, "check").startswith("ok ")
    assert run(exe, "runs", 8, "null", "01010101", "11111111").splitlines()[2].split() == ["%d:1" % t for t in range(8)]
    assert run(exe, "block", "8,4,3,2,190,2,%d,1" % (A + 1)).split() == ["0", "-22", "1"]
    assert len(run(exe, "splits", 16, 256, 256, 4, 1, 100).splitlines()) == 100
