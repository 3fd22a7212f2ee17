"""The filter sizes at which the default launch planner (make_plan, csrc/rbf_plan.h) changes its mind, as data, and what the two test
files that use them share: tests/test_plan_boundaries_cpu.py proves the table against the planner (every row is a transition, a sweep
finds no other), tests/test_gpu_plan_boundaries.py runs the device on both sides of every row against the C oracle.

A row is (knobs, counts known, frames, coded, last, first, name): `last` is the last m of the old plan and `first` = last + 1 the first
m of the new one, for a batch of `frames` frames of which the first `coded` have a filter of that many bits and the others none, on a
device of 256 CUs.  "Counts known" is rbf_encode_gop, which knows the masks' set-bit counts on the host (the two-phase insert); unknown
is rbf_bloom_encode_batch and every decode.  The counts-known rows are those of the batch the GOP test submits: two pairs, the first
coded, the second unchanged -- k_query_u64's LDS budget counts every frame of the batch, coded or not, so its hand-over lies 128 bits
lower there than for one frame.  Whoever changes LDS_LIMIT, MAX_INSERT_TILES, MAX_QUERY_TILES, F64MOD_M_MIN / F64MOD_M_MAX or an LDS
layout (rbf_geometry.h) moves rows of this table: the CPU test then fails until the table follows, and the GPU test runs the new sizes.

The decision a row separates is the `decision` field tests/c/plan_cases.cpp prints: fast_insert, query kernel, double_buffer,
insert_tab, two_phase, probe_image, insert tiles, query tiles -- each as the launch code reads it (double_buffer only where
k_query_lds runs, the insert's fields only where an LDS insert runs)."""
import collections
import concurrent.futures
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
CUS = 256
KNOBS = {"default": 0, "barrett_only": 8}                       # rbf_ctx_force_generic flags
SWEEP_END = 1 << 24
SMALL_M_END = 1 << 30                                           # last m of the small-m reduction (Plan::small_m), far beyond the sweep

Row = collections.namedtuple("Row", "knobs known frames coded last first name")


def _rows(knobs, known, frames, named, coded=None):
    return [Row(knobs, known, frames, coded or frames, first - 1, first, name) for first, name in named]


INSERT_TILES = [(770049, "insert_tiles_2"), (1540097, "insert_tiles_3"), (2310145, "insert_tiles_4"), (3080193, "insert_tiles_5"),
                (3850241, "insert_tiles_6"), (4620289, "insert_tiles_7"), (5390337, "insert_generic")]

ROWS = (
    # default knobs, counts unknown: k_insert_lds / k_insert_tab, k_query_lds / k_query_u64 / k_query_s64t (2 to 7 tiles; from 5 tiles
    # on next to the generic insert, whose k_filter_reduce writes the probe image in place) / k_query
    _rows("default", False, 1, [(32768, "fp64_begins"), (654977, "u64_to_s64t")] + INSERT_TILES +
          [(1294209, "s64t_tiles_2"), (2588417, "s64t_tiles_3"), (3882625, "s64t_tiles_4"), (5176833, "s64t_tiles_5"),
           (6471041, "s64t_tiles_6"), (7765249, "s64t_tiles_7"), (8388608, "fp64_ends")]) +
    # ... k_query_u64's LDS: two image buffers + 32 bytes per frame of the batch + one more record
    _rows("default", False, 29, [(651393, "u64_to_s64t")]) +
    _rows("default", False, 128, [(638721, "u64_to_s64t")]) +
    # default knobs, counts known: k_insert_positions + k_insert_records from two queue-sized tiles on, record tiles of all of LDS;
    # past insert_generic the counts reach no decision, the rows are the counts-unknown ones through the other entry point
    _rows("default", True, 2, coded=1, named=[(32768, "fp64_begins"), (654849, "u64_to_s64t"), (770049, "two_phase_begins"), (1294209, "s64t_tiles_2"),
                               (1310721, "record_tiles_2"), (2588417, "s64t_tiles_3"), (2621441, "record_tiles_3"),
                               (3882625, "s64t_tiles_4"), (3932161, "record_tiles_4"), (5176833, "s64t_tiles_5"),
                               (5242881, "record_tiles_5"), (5390337, "insert_generic"), (6471041, "s64t_tiles_6"),
                               (7765249, "s64t_tiles_7"), (8388608, "fp64_ends")]) +
    # barrett_only: k_insert_lds, k_query_lds double / single buffer, k_query_tiled, k_query
    _rows("barrett_only", False, 1, [(655361, "lds_single_buffer"), (1310721, "tiled_2"), (2621441, "tiled_3"), (3932161, "query_generic")] +
          INSERT_TILES) +
    _rows("barrett_only", False, 128, [(655361, "lds_single_buffer")])
)


def row_id(row):
    return "%s-%s-%df-%d-%s" % (row.knobs, "known" if row.known else "unknown", row.frames, row.first, row.name)


SWEEPS = sorted({(r.knobs, r.known, r.frames, r.coded) for r in ROWS})     # the batch shapes the table has rows for
BASE_FRAMES = {False: 1, True: 2}                                         # the shape that holds all rows of a (knobs, counts known)


def sweep_rows(knobs, known, frames, coded):
    """The rows a sweep of m over this batch shape must find: its own, and of the base shape's those that do not depend on the frame
    count (the ones whose name the shape has no row of its own for)."""
    own = {r.name: r for r in ROWS if (r.knobs, r.known, r.frames, r.coded) == (knobs, known, frames, coded)}
    base = [r for r in ROWS if (r.knobs, r.known, r.frames) == (knobs, known, BASE_FRAMES[known])]
    return sorted(list(own.values()) + [r for r in base if r.name not in own], key=lambda r: r.first)


# ---- the planner on the CPU ---------------------------------------------------------------------------------------------------------
def build_plan_cases(tmp_dir):
    """tests/c/plan_cases.cpp built with a plain host compiler, as tests/test_plan_cpu.py builds it."""
    exe = os.path.join(str(tmp_dir), "plan_cases")
    r = subprocess.run([GXX, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror",
                        os.path.join(REPO, "tests", "c", "plan_cases.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def plans(exe, cases):
    """cases: (row or (knobs, known, frames, coded), m).  One process; returns one dict of the fields of the `plan` line per case."""
    text = ""
    for shape, m in cases:
        knobs, known, frames, coded = shape[:4]
        assert coded in (1, frames)                             # plan_cases: every frame m, or frame 0 alone (m0)
        text += "%d %d %d %d 0 %d %s\n" % (1 << 22, frames, CUS, KNOBS[knobs], known, "%d" % m if coded == frames else "0 %d" % m)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert len(lines) == len(cases) and all(ln[0] == "plan" for ln in lines), out.stdout[-2000:]
    return [dict(f.split("=") for f in ln[1:]) for ln in lines]


def sweep(exe, knobs, known, frames, coded=None, lo=2, hi=SWEEP_END, step=128):
    """[(last, first, decision before, decision after)] of every change of the decision for m in lo .. hi"""
    out = subprocess.run([exe], input="sweep %d %d %d %d %d %d %d %d %d\n" % (1 << 22, frames, CUS, KNOBS[knobs], known, lo, hi, step, coded or frames),
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "swept lo=%d hi=%d step=%d" % (lo, hi, step), lines[-1:]
    found = []
    for ln in lines[:-1]:
        tag, *fields = ln.split()
        d = dict(f.split("=") for f in fields)
        assert tag == "transition"
        found.append((int(d["last"]), int(d["first"]), d["before"], d["after"]))
    return found


# ---- inputs of the device tests -----------------------------------------------------------------------------------------------------
KSTARS = (2.3, 0.7, 1.0, 3.25, 5.5)     # floor(k*) 0 .. 5: the three modes of k_query_s64t, the row classes of k_query_u64
DENSITY = 0.25
MAX_PIXELS = 8 << 20
LOAD = 0.5                              # k* x ones / m: the oracle's filter is then 1 - exp(-0.5) = 39 % full
FILL = (0.20, 0.60)


def ragged(n):
    """n moved within its group of eight to n % 8 == 5: then n % 8 != 0 and n % 512 != 0"""
    return n - n % 8 + 5 if n % 8 != 5 else n


def pixels_for(m, k):
    return ragged(int(LOAD * m / (DENSITY * k)))


def kstar_for(index, m):
    """k* of the index-th case: the cycle over KSTARS; where that would take more than MAX_PIXELS pixels (small k* on a large filter)
    the next k* of the cycle that does not."""
    for j in range(len(KSTARS)):
        k = KSTARS[(index + j) % len(KSTARS)]
        if pixels_for(m, k) <= MAX_PIXELS:
            return k
    raise AssertionError("no k* of the cycle keeps m = %d below %d pixels" % (m, MAX_PIXELS))


def random_mask(seed, n, density):
    """uint8 [n] of 0 / 1, about density x n ones (PCG64 bytes against a threshold: exact enough, and fast for millions of pixels)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 16, n, dtype=np.uint16) < int(density * 65536)).astype(np.uint8)


Reference = collections.namedtuple("Reference", "mask m k filter witness filter_ones fill")


def reference(oracle, mask, m, k, seeds):
    """The C oracle's filter and witness of one mask (orc_compress), packed the way the library returns them."""
    n = len(mask)
    bits = np.zeros(m, dtype=np.uint8)
    witness = np.zeros(n, dtype=np.uint8)
    u8p = ctypes.c_void_p
    w = oracle.lib().orc_compress(u8p(mask.ctypes.data), n, m, float(k), (ctypes.c_uint64 * 3)(*seeds), u8p(bits.ctypes.data), u8p(witness.ctypes.data))
    ones = int(np.count_nonzero(bits))
    return Reference(mask, m, k, np.packbits(bits), (int(w), np.packbits(witness[:w])), ones, ones / m)


class References:
    """Oracle results computed ahead of the tests that compare against them, on a few threads (orc_compress holds no Python lock): the
    oracle walking n pixels is most of a case's time.  plan() names the work in the order the tests will ask for it; get(key) starts
    that piece and the next few, so that no more than `ahead` results wait in memory, and hands the result out once."""

    def __init__(self, workers=8, ahead=8):
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers)
        self.order, self.work, self.futures, self.ahead = [], {}, {}, ahead

    def plan(self, key, fn, *args):
        if key not in self.work:
            self.order.append(key)
            self.work[key] = (fn, args)

    def get(self, key):
        at = self.order.index(key)
        for k in self.order[at:at + self.ahead]:
            if k not in self.futures:
                self.futures[k] = self.pool.submit(self.work[k][0], *self.work[k][1])
        result = self.futures[key].result()
        self.order.remove(key)
        del self.futures[key], self.work[key]
        return result

    def close(self):
        for f in self.futures.values():
            f.cancel()
        self.pool.shutdown(wait=True)


def same_bits(a, b, nbits):
    """two packed bit vectors agree in their first nbits bits"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    whole, rest = nbits // 8, nbits % 8
    if len(a) < (nbits + 7) // 8 or len(b) < (nbits + 7) // 8 or not np.array_equal(a[:whole], b[:whole]):
        return False
    return rest == 0 or (int(a[whole]) ^ int(b[whole])) >> (8 - rest) == 0


def check_encoded(r, ref, what):
    """one frame of BloomEngine.encode / GopCoder.results against its Reference: filter bytes, filter_ones, witness_bits, witness bytes"""
    assert FILL[0] <= ref.fill <= FILL[1], (what, "the oracle's filter is %.1f %% full" % (100 * ref.fill))
    assert same_bits(r["filter"], ref.filter, ref.m), (what, "filter")
    assert r["filter_ones"] == ref.filter_ones, (what, "filter_ones")
    assert r["witness_bits"] == ref.witness[0], (what, "witness_bits")
    assert same_bits(r["witness"], ref.witness[1], ref.witness[0]), (what, "witness")


def check_decoded(dec_row, ref, what):
    n = len(ref.mask)
    assert same_bits(dec_row, np.packbits(ref.mask), n), (what, "decode of the oracle's filter and witness")


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
SIDES = ("last", "first")
BATCH_ROWS = [r for r in ROWS if not r.known and r.frames == 1]           # one frame through BloomEngine.encode / decode
FRAME_ROWS = [r for r in ROWS if not r.known and r.frames > 1]            # a batch of that many frames
GOP_ROWS = [r for r in ROWS if r.known]                                   # GopCoder (rbf_encode_gop)


def batch_case(row, side):
    """(n, m, k*, mask seed) of a one-frame row: both sides share the pixels, the mask and k*"""
    index = BATCH_ROWS.index(row)
    k = kstar_for(index, row.first)
    return pixels_for(row.first, k), getattr(row, side), k, 1000 + index


def batch_reference(oracle, seeds, n, m, k, seed):
    return reference(oracle, random_mask(seed, n, DENSITY), m, k, seeds)


# The frame-count rows share their pixels and the frames around the boundary filter: 127 smaller filters inside the FP64 range (so that
# the batch is one launch under the default knobs too), each with its own m, k* and mask at the same load, two of them not coded.
FRAMES_KSTAR = 5.5
FRAMES_PIXELS = pixels_for(max(r.first for r in FRAME_ROWS), FRAMES_KSTAR)
FRAMES_UNCODED = (3, 17)
FRAMES_MOST = max(r.frames for r in FRAME_ROWS)
FRAMES_OTHERS = FRAMES_MOST - 1 + len(FRAMES_UNCODED)                      # the last two stand in for the uncoded ones in an all-coded batch


def batches_of(row, edge, others):
    """The batches of a frame-count row around its boundary filter `edge`: (what, frames).  The boundary filter first and last among
    frames of which two are not coded; and last among frames that are all coded -- only then does k_query_u64 get the record of every
    frame of the batch and use the LDS the planner budgeted to the last byte."""
    rest = others[:row.frames - 1]
    full = [others[FRAMES_MOST - 1 + FRAMES_UNCODED.index(j)] if j in FRAMES_UNCODED else ref for j, ref in enumerate(rest)]
    return (("first", [edge] + rest), ("last", rest + [edge]), ("last, all coded", full + [edge]))


def other_frame(j):
    """(m, k*, density, mask seed) of the j-th frame around the boundary filter"""
    k = KSTARS[j % len(KSTARS)]
    if j in FRAMES_UNCODED:
        return 0, k, 0.1, 5000 + j
    cap = min(600000, int(k * FRAMES_PIXELS * DENSITY / LOAD))
    m = 32768 + (j * 37123) % (cap - 32768)
    return m, k, LOAD * m / (k * FRAMES_PIXELS), 5000 + j


def other_reference(oracle, seeds, j):
    m, k, density, seed = other_frame(j)
    mask = random_mask(seed, FRAMES_PIXELS, density)
    return reference(oracle, mask, m, k, seeds) if m else Reference(mask, 0, k, np.zeros(0, np.uint8), (0, np.zeros(0, np.uint8)), 0, 0.0)


def edge_reference(oracle, seeds, m):
    return reference(oracle, random_mask(4999, FRAMES_PIXELS, DENSITY), m, FRAMES_KSTAR, seeds)


MIXED = ((32767, 2.3), (32768, 0.7), (8388607, 3.25), (8388608, 5.5))     # one batch across both ends of the FP64 range
MIXED_PIXELS = pixels_for(8388608, 5.5)


def mixed_reference(oracle, seeds, j):
    m, k = MIXED[j]
    return reference(oracle, random_mask(7000 + j, MIXED_PIXELS, LOAD * m / (k * MIXED_PIXELS)), m, k, seeds)


GOP_DENSITY, GOP_DENSITY_MAX = 0.11, 0.125       # l / n = 0.311 and 0.317: the planned filter grows with the density up to the second


def bits_per_pixel(p):
    """l / n of the reference's geometry at density p: k* = log2((1 - p) ln^2 2 / p), l = p n k* / ln 2"""
    return p * math.log2((1 - p) * math.log(2) ** 2 / p) / math.log(2)


def planned_bits(lib, params_type, n, ones):
    """m of rbf_plan_batch for a frame of n pixels with `ones` changed ones (host only)"""
    par = (params_type * 1)()
    assert lib.rbf_plan_batch(n, (ctypes.c_uint64 * 1)(ones), 1, 1, par, None) == 0
    return par[0].m


def gop_case(row, side, lib, params_type):
    """(W, H, ones, m): a frame size and a count of changed pixels whose planned filter lies within 128 bits of the row on `side` --
    (last - 128, last] or [first, first + 128).  Odd W and H: n % 8 != 0."""
    lo, hi = (row.last - 127, row.last) if side == "last" else (row.first, row.first + 127)
    target = int(lo / bits_per_pixel(GOP_DENSITY))
    W = int((target * 16 / 9) ** 0.5) | 1
    H = -(-target // W) | 1
    n = W * H
    a, b = 1, int(GOP_DENSITY_MAX * n)                          # m grows with ones up to there: the smallest count that reaches lo
    assert planned_bits(lib, params_type, n, b) >= lo, (row, side)
    while a < b:
        mid = (a + b) // 2
        if planned_bits(lib, params_type, n, mid) >= lo:
            b = mid
        else:
            a = mid + 1
    m = planned_bits(lib, params_type, n, a)
    assert lo <= m <= hi, (row, side, m)
    assert a / n <= DENSITY
    return W, H, a, m


def gop_frames(seed, W, H, ones):
    """three luma frames: a random one, the same with exactly `ones` pixels changed, and that one again; and the mask of the change"""
    n = W * H
    rng = np.random.default_rng(seed)
    mask = random_mask(seed + 1, n, ones / n)
    surplus = int(mask.sum(dtype=np.int64)) - ones
    if surplus:
        pool = np.flatnonzero(mask == (1 if surplus > 0 else 0))
        mask[rng.choice(pool, abs(surplus), replace=False)] ^= 1
    f0 = rng.integers(0, 256, n, dtype=np.uint8)
    f1 = f0 + mask * np.uint8(37)
    return np.stack([f0, f1, f1]).reshape(3, H, W), mask


def gop_reference(oracle, seeds, seed, W, H, ones, m):
    """(frames, Reference, k*): the oracle's own mask, geometry, filter and witness of the changed pair"""
    frames, mask = gop_frames(seed, W, H, ones)
    n = W * H
    want = oracle.residual_mask(frames[0], frames[1], 0.0).reshape(-1)
    assert np.array_equal(want, mask) and int(want.sum(dtype=np.int64)) == ones
    k, l = oracle.optimal_params(n, np.sum(want) / n)
    assert l == m, (l, m)
    return frames, reference(oracle, want, l, k, seeds), k
