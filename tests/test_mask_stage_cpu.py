"""The mask-stage sweep without a GPU: the reference of tests/mask_stage.py against the C oracle and the committed fixtures, the wrong
rules a kernel could have against the cases the GPU sweep (tests/test_gpu_mask_stage_sweep.py) runs -- each must be exposed by a case that
is named here -- and the chunk planner (csrc/rbf_mask_plan.h), built with a plain g++ (tests/c/mask_plan_cases.cpp), over every block
length, chunk knob and run pattern of the sweep, plain and under the sanitizers."""
import collections
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mask_stage as ms
from conftest import REPO, load_json, load_npz

GXX = shutil.which("g++")
SRC = os.path.join(REPO, "tests", "c", "mask_plan_cases.cpp")
CSRC = os.path.join(REPO, "new_bloom_filter_repo_amd", "csrc")


# ------------------------------------------------------------------ the reference
def oracle_rows(oracle, frames, thr):
    """The C oracle's residual_mask over the luma of (F, n, C) frames, packed as ref_masks packs."""
    F, n = frames.shape[:2]
    rows, ones = np.zeros((F - 1, ms.packed_stride(n)), np.uint8), np.zeros(F - 1, np.int64)
    for f in range(F - 1):
        m = oracle.residual_mask(np.ascontiguousarray(frames[f][:, 0]), np.ascontiguousarray(frames[f + 1][:, 0]), float(thr)).reshape(-1)
        rows[f, :(n + 7) // 8] = np.packbits(m)
        ones[f] = int(m.sum())
    return rows, ones


@pytest.mark.parametrize("kernel", [ms.KERNELS[0], ms.KERNELS[2]], ids=["u8", "u16"])
def test_reference_equals_the_oracle_on_grids_and_random_clips(oracle, kernel):
    rng = np.random.default_rng(5)
    rand = rng.integers(0, 1 << (8 * kernel.sample_bytes), (4, 3000, 1)).astype(ms.dtype_of(kernel.sample_bytes))
    near = rand.copy()
    near[1:] = near[0] + rng.integers(-2, 3, (3, 3000, 1)).astype(near.dtype)       # small differences, wrapping at both ends
    for frames in (ms.grid_clip(kernel), rand, near):
        for thr in ms.thresholds_of(kernel):
            rows, ones = ms.ref_masks(frames, None, thr)
            want_rows, want_ones = oracle_rows(oracle, frames, thr)
            assert np.array_equal(rows, want_rows) and np.array_equal(ones, want_ones), (kernel.name, thr)
    # the grids hold what they claim
    a, b = ms.u8_grid() if kernel.sample_bytes == 1 else ms.u16_grid()
    if kernel.sample_bytes == 1:
        assert len(set(zip(a.tolist(), b.tolist()))) == 65536
    else:
        slots = {}
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            slots.setdefault((x, y), set()).add(i % 16)
        assert len(slots) == 1024 and all(len(s) == 16 for s in slots.values())
        assert set(ms.U16_EDGES) <= set(a.tolist())


def test_reference_equals_the_committed_masks():
    z = load_npz("g5_masks.npz")
    for r in load_json("g5_masks.json")["rows"]:
        name, thr = r["name"], r["thr"]
        prev, curr = z[name + "_prev"], z[name + "_curr"]
        want = z["%s_mask_%s" % (name, str(thr).replace(".", "_"))].reshape(-1)
        frames = np.stack([prev.reshape(-1, 1), curr.reshape(-1, 1)])
        rows, ones = ms.ref_masks(frames, None, int(np.floor(thr)))               # the device takes floor(threshold): the same bit for integers
        assert np.array_equal(np.unpackbits(rows[0])[:want.size], want) and int(ones[0]) == r["ones"], (name, thr)


def test_all_channel_reference_marks_what_the_luma_rule_ignores():
    k = ms.KERNELS[7]
    frames = ms.one_hot_clip(k.sample_bytes, k.pixel_bytes, 0x80)
    _, luma = ms.ref_masks(frames, None, 0, 1)
    rows, ones = ms.ref_masks(frames, None, 0, k.mask_channels)
    assert (ones == 1).all() and luma.sum() == 16                 # luma: the low byte of sample 0 only; 0x8000 on its high byte is not a change
    for t in range(len(ones)):
        px, _ = ms.one_hot_byte(t, k.pixel_bytes)
        assert np.unpackbits(rows[t])[px] == 1


# ------------------------------------------------------------------ the clips hold what they claim
@pytest.mark.parametrize("kernel", ms.KERNELS, ids=ms.KERNEL_IDS)
def test_one_hot_clips(kernel):
    zero_pairs = 0
    for x in ms.XORS:
        frames = ms.one_hot_clip(kernel.sample_bytes, kernel.pixel_bytes, x)
        assert frames.shape == (16 * kernel.pixel_bytes + 1, 2048, ms.samples_per_pixel(kernel))
        raw = frames.view(np.uint8).reshape(frames.shape[0], -1)
        for t in range(frames.shape[0] - 1):
            d = np.flatnonzero(raw[t] ^ raw[t + 1])
            px, byte = ms.one_hot_byte(t, kernel.pixel_bytes)
            assert d.tolist() == [px * kernel.pixel_bytes + byte] and raw[t, d[0]] ^ raw[t + 1, d[0]] == x
        _, ones = ms.ref_masks(frames, None, 0, kernel.mask_channels)
        assert set(ones.tolist()) <= {0, 1}
        zero_pairs += int((ones == 0).sum())
        if kernel.mask_channels >= 2:
            assert (ones == 1).all()
    # the reference decides which pairs are all-zero: the bytes the luma rule does not read, and 0x80 on a 16-bit luma's high byte
    luma_bytes = 16 * kernel.sample_bytes
    want_zero = 0 if kernel.mask_channels >= 2 else 3 * (16 * kernel.pixel_bytes - luma_bytes) + (16 if kernel.sample_bytes == 2 else 0)
    assert zero_pairs == want_zero
    lanes = {(7 * t + 3) % 64 for t in range(16 * kernel.pixel_bytes)}
    assert len(lanes) >= 16


@pytest.mark.parametrize("P", ms.CHUNK_PAIRS)
def test_count_clips(P):
    for kernel, n in ((ms.CHUNK_KERNELS[0], 4096), (ms.CHUNK_KERNELS[1], 1024)):
        frames, counts = ms.count_clip(P, kernel, n)
        for thr in ([0, ms.count_thresholds(P)] if kernel.mask_channels == 1 else [0]):
            _, ones = ms.ref_masks(frames, None, thr, kernel.mask_channels)
            assert ones.tolist() == counts
        assert len(set(counts)) == P and n in counts and (P < 3 or 0 in counts)
        if P >= 2:
            e = counts.index(n)
            assert e % 2 == 0 and counts[e + 1] == n - 1
    assert max(ms.count_thresholds(P)) < 0x40 and all(a != b for a, b in zip(ms.count_thresholds(P), ms.count_thresholds(P)[1:]))


# ------------------------------------------------------------------ the planner, built with a plain host compiler
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    if GXX is None:
        pytest.skip("g++ not found: tests/c/mask_plan_cases.cpp is built with a plain host compiler, not with hipcc")
    exe = str(tmp_path_factory.mktemp("mask_plan") / "mask_plan_cases")
    r = subprocess.run([GXX, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


Plan = collections.namedtuple("Plan", "grid_y count ppc skip_in_table chunks")


def plan_many(exe, jobs):
    """jobs: [(nframes, wanted, fast_segs, skip bytes or None)] -> [Plan]; chunks: [(first pair, pairs, skipped)], the uniform ones spelled out."""
    text = "".join("%d %d %d %s\n" % (F, w, segs, "null" if skip is None else "".join("1" if s else "0" for s in skip)) for F, w, segs, skip in jobs)
    out = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(jobs)
    plans = []
    for (F, _, _, _), ln in zip(jobs, lines):
        tok = ln.split()
        grid_y, count, ppc, sit = (int(v) for v in tok[:4])
        chunks = [tuple(int(v) for v in e.split(":")) for e in tok[4:]]
        chunks = [(a, b, bool(c)) for a, b, c in chunks] if count else ms.uniform_chunks(F - 1, ppc)
        assert len(chunks) == grid_y
        plans.append(Plan(grid_y, count, ppc, bool(sit), chunks))
    return plans


def test_planner_self_check(cases):
    out = subprocess.run([cases, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"ok \d+\n", out.stdout) and int(out.stdout.split()[1]) > 200000, out.stdout[-2000:]


def check_plan(p, F, skip, tag):
    pairs = F - 1
    cover = np.zeros(pairs, np.int64)
    for f0, cnt, skipped in p.chunks:
        assert cnt >= 1 and f0 + cnt <= pairs, tag                # every pairs[y] & 0x7FFF is nonzero
        cover[f0:f0 + cnt] += 1
        if p.count:
            assert (skip[f0:f0 + cnt] != 0).all() if skipped else not skip[f0:f0 + cnt].any(), tag      # no coded chunk spans a run start; skip chunks hold skipped pairs only
    assert (cover == 1).all(), tag                                # every pair in exactly one chunk: grid.y covers all pairs
    assert p.count <= ms.MASK_MAX_CHUNKS and p.grid_y == len(p.chunks), tag
    if skip is None:
        assert p.count == 0 and not p.skip_in_table, tag
    else:
        assert p.skip_in_table == (p.count != 0), tag


def test_planner_properties(cases):
    lengths = list(range(2, 301))
    jobs, skips = [], []
    for F in lengths:
        pats = [None] + [ms.skip_bytes(F, s) for s in ms.run_patterns(F).values()]
        for wanted in range(32):
            for sk in pats:
                jobs.append((F, wanted, 1 if F % 2 else 4, sk))
    plans = plan_many(cases, jobs)
    for job, p in zip(jobs, plans):
        check_plan(p, job[0], job[3], job[:3])
        F, wanted, segs, sk = job
        if wanted and sk is None:                                 # one run: the knob is the chunk count, up to one pair per chunk
            assert p.grid_y <= min(wanted, F - 1) and p.ppc == -(-(F - 1) // min(wanted, F - 1)), job[:3]
    assert len(plans) > 50000


def test_planner_at_the_table_limit(cases):
    jobs = [(F, 0, 1, ms.skip_bytes(F, starts)) for F, starts, _ in ms.TABLE_PATTERNS.values()]
    p255, p256, p257 = plan_many(cases, jobs)
    for p, (F, starts, entries) in zip((p255, p256), list(ms.TABLE_PATTERNS.values())[:2]):
        assert p.count == p.grid_y == entries and p.skip_in_table
        check_plan(p, F, ms.skip_bytes(F, starts), entries)
    # one entry too many: uniform chunks over everything, the skipped pairs through their thresholds
    F = ms.TABLE_PATTERNS["table257"][0]
    assert p257.count == 0 and not p257.skip_in_table and p257.ppc == 1 and p257.grid_y == F - 1
    # a block too long for 15-bit chunk lengths takes the fallback whatever its runs
    sk = np.zeros(0x8000 - 1, np.uint8)
    sk[100] = 1
    big, small = plan_many(cases, [(0x8000, 4, 4, sk), (0x7FFF, 4, 4, sk[:-1])])
    assert big.count == 0 and not big.skip_in_table and big.grid_y == 4 and small.count and small.skip_in_table
    check_plan(small, 0x7FFF, sk[:-1], "0x7FFF frames")
    assert (100, 1, True) in small.chunks


def test_ticket_table_gives_the_grids_it_claims(cases):
    jobs = [(t.frames, t.chunks, t.W * t.H // ms.SEG, None) for t in ms.TICKETS]
    for t, p in zip(ms.TICKETS, plan_many(cases, jobs)):
        assert t.W * t.H % ms.SEG == 0                             # whole segments: the fused finish
        nwg = -(-(t.W * t.H // ms.SEG) // ms.WG_WAVES) * p.grid_y
        assert nwg == t.nwg and p.grid_y == t.chunks, t
        assert t.wide == any(cnt > 64 for _, cnt, _ in p.chunks), t
        mine, groups = ms.ticket_groups(nwg)
        assert sum(mine) == nwg and groups == sum(1 for m in mine if m)
    hit = {t.nwg for t in ms.TICKETS}
    assert {1, 2, 63, 64, 65, 127, 128, 129} <= hit and max(hit) > 1000
    assert sum(1 for t in ms.TICKETS if t.wide and t.nwg > 1) >= 2
    assert len({ms.TICKETS[i].nwg for i in ms.SEQUENCE}) == 3


# ------------------------------------------------------------------ every wrong rule is exposed by a case the GPU sweep runs
def sweep_cases(kernel):
    """(name, frames, threshold) of part (a) of the GPU sweep for one kernel."""
    for x in ms.XORS:
        yield "one_hot_xor%02x" % x, ms.one_hot_clip(kernel.sample_bytes, kernel.pixel_bytes, x), 0
    grid = ms.grid_clip(kernel)
    for thr in ms.thresholds_of(kernel):
        yield "grid_thr%d" % thr, grid, thr


@pytest.mark.parametrize("kernel", ms.KERNELS, ids=ms.KERNEL_IDS)
def test_bit_and_byte_mutants_are_killed_per_kernel(kernel):
    todo = {m for m in ms.BIT_MUTANTS if ms.mutant_applies(m, kernel)}
    assert {"lsb_first"} | {"byte_%d_wrong" % k for k in range(kernel.pixel_bytes)} <= todo
    killed = {}
    for name, frames, thr in sweep_cases(kernel):
        rows, ones = ms.ref_masks(frames, None, thr, kernel.mask_channels)
        for m in sorted(todo - set(killed)):
            mrows, mones = ms.mutant_masks(m, frames, kernel, thr)
            if not (np.array_equal(rows, mrows) and np.array_equal(ones, mones)):
                killed[m] = name
        if len(killed) == len(todo):
            break
    assert set(killed) == todo, sorted(todo - set(killed))
    # the byte mutants fall to the one-hot clips, the value mutants to a clip that reaches 0x8000 or an equal pair
    assert all(killed[m].startswith("one_hot") for m in killed if m.startswith("byte_"))


def chunk_families(cases):
    """{(P, chunks knob): Plan} of part (b) of the GPU sweep at 64x64."""
    keys = [(P, c) for P in ms.CHUNK_PAIRS for c in ms.CHUNK_KNOBS]
    return dict(zip(keys, plan_many(cases, [(P + 1, c, 4, None) for P, c in keys])))


def test_chunk_and_tally_mutants_are_killed_per_family(cases):
    fam = chunk_families(cases)
    exposed = {m: [] for m in ms.CHUNK_MUTANTS}
    for (P, c), p in fam.items():
        counts = np.array(ms.counts_of(P, 4096))
        lens = [cnt for _, cnt, _ in p.chunks]
        reach = {"chunk_first_pair_dropped": any(f0 > 0 and counts[f0] for f0, _, _ in p.chunks),
                 "chunk_first_pair_twice": any(f0 > 0 and counts[f0] for f0, _, _ in p.chunks),
                 "tally_halves_swapped": max(lens) >= 2, "tally_not_flushed": max(lens) > 128}
        for m, reachable in reach.items():
            _, mones = ms.chunk_mutant(m, None, counts, p.chunks)
            assert (not np.array_equal(mones, counts)) == bool(reachable), (m, P, c)      # wherever the rule can act, the counts show it
            if reachable:
                exposed[m].append((P, c))
    assert (129, 1) in exposed["tally_not_flushed"] and (299, 2) in exposed["tally_not_flushed"]      # a flush in a first and in a second chunk
    assert len(fam[(299, 2)].chunks) == 2 and fam[(299, 2)].chunks[1][1] > 128
    assert {P for P, _ in exposed["chunk_first_pair_dropped"]} == set(ms.CHUNK_PAIRS) - {1}
    assert (3, 0) in exposed["tally_halves_swapped"] or (3, 1) in exposed["tally_halves_swapped"]
    # more chunks asked for than there are pairs
    assert fam[(3, 31)].grid_y == 3 and fam[(1, 31)].grid_y == 1
    # runs, at 32x32: a skipped pair that is diffed shows in the counts of every pattern that skips a pair which changes
    jobs, keys = [], []
    for P in ms.CHUNK_PAIRS:
        for name, starts in ms.run_patterns(P + 1).items():
            if starts:
                jobs.append((P + 1, 0, 1, ms.skip_bytes(P + 1, starts)))
                keys.append((P, name, starts))
    silent = []
    for (P, name, starts), p in zip(keys, plan_many(cases, jobs)):
        counts = np.array(ms.counts_of(P, 1024))
        true = counts.copy()
        true[ms.skipped_pairs(P + 1, starts)] = 0
        if np.array_equal(true, counts):
            silent.append((P, name))
        else:
            exposed["skipped_pair_diffed"].append((P, name))
    assert silent == [(3, "at_last")], silent                       # the one family whose only skipped pair is the clip's unchanged one
    assert all(exposed[m] for m in ms.CHUNK_MUTANTS)


def test_mutant_list_is_the_issue_s():
    assert set(ms.MUTANTS) == set(ms.BIT_MUTANTS) | set(ms.CHUNK_MUTANTS) and len(ms.MUTANTS) == 17
    k = ms.KERNELS[0]
    frames, _ = ms.count_clip(5, k, 1024)
    rows, ones = ms.ref_masks(frames, None, 0, 1, run_starts=[2])
    mrows, mones = ms.mutant_masks("skipped_pair_diffed", frames, k, 0, run_starts=[2])
    assert ones[1] == 0 and not rows[1].any() and mones[1] == 1023 and mrows[1].any()


# ------------------------------------------------------------------ where the planner lives
def test_the_planner_takes_any_host_compiler():
    with open(os.path.join(CSRC, "rbf_mask_plan.h"), encoding="utf-8") as f:
        hdr = f.read()
    assert "static uint32_t plan_mask_chunks(" in hdr and "struct MaskChunks" in hdr and "MASK_MAX_CHUNKS = 256" in hdr and "MASK_CHUNK_SKIP = 0x8000u" in hdr
    assert re.findall(r'#include\s+[<"]([^>"]+)', hdr) == ["rbf_plan.h", "algorithm", "cstdint"], "the header takes any host compiler"
    for name in ("rbf_api.hip", "rbf_kernels_mask.h"):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            text = f.read()
        assert "struct MaskChunks" not in text and "plan_mask_chunks(const Knobs" not in text, name
    assert ms.MASK_MAX_CHUNKS == 256


@pytest.mark.skipif(GXX is None, reason="g++ not found")
def test_planner_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, host code only, with AddressSanitizer and UBSan linked in: its own main runs it, nothing is preloaded."""
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([GXX] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this g++ cannot link the sanitizer runtimes")     # (decided on a one-line program: a failure of the real build below is a failure)
    exe = str(tmp_path / "mask_plan_cases_san")
    r = subprocess.run([GXX] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout[-2000:], out.stderr[-2000:])
    jobs = [(F, 0, 1, ms.skip_bytes(F, starts)) for F, starts, _ in ms.TABLE_PATTERNS.values()]
    assert [p.count for p in plan_many(exe, jobs)] == [255, 256, 0]
