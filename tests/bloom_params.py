"""Filter lengths and activation thresholds chosen ON the pixel hashes -- the cases and the exact reference of tests/
test_gpu_bloom_params.py; a helper, not a test (tests/test_bloom_params_cpu.py proves on the CPU that every case has its property).

Every other Bloom-core test takes (m, floor_k, T) from a density through params.filter_params, so its T sits on a float64 rounding
boundary and its remainders are whatever the index hashes give.  Here the test knows every pixel's three hashes (oracle.hash_index, once
per seed triple) and picks the integer parameters of the C ABI so that they collide with them:

  thresholds  T equal to a pixel's activation hash and one above it (the plain `ha < T` of the Barrett and generic kernels, the tag
              shortcut of insert_tab_steps, the activation ranks of the FP64 query kernels), the ends of the range, the fullest 16-bit tag.
  lengths     m with h1 % m == 0 or m - 1, h2 % m == 0 or m - 1, h1 % m + h2 % m == m or m - 1 for a set pixel: where the folds of
              mod_m_f64, rows_reduce4, mod_m_small, mod_m and of the probe step min(s2, s2 - m) decide the result.  One filter length per
              batch (length_cases): a batch is planned by its largest filter, so a length meant for k_query_u64 and its row passes
              (rows_reduce4 exists only there) must not share a batch with one that does not fit LDS twice.
  ranks       whole batches of 1, 2, 3, 5, 127 and 128 coded frames whose thresholds are equal, distinct and unsorted, partly
              duplicated, and interleaved with frames that are not coded.

One geometry, n = 509 x 257 = 130813 (n % 64 = 61; the decimal keys cross 99999 / 100000), two seed triples.  The reference (`reference`)
is numpy uint64 arithmetic on explicit (m, floor_k, T) and never goes through a k*.

Masks.  The threshold and rank frames take the seeded mask of density 0.09 (BASE_DENSITY) with the case's pixels forced.  A length frame
thins that mask to LOAD / (floor_k + T / 2^64) x m set pixels when it holds more (`Case.keep`), so that the filter stays about 40 % full:
under the whole mask every filter below 2^15 bits is all ones, and a saturated filter passes whatever position the kernel forms.  The
selected pixel is found among the set pixels of the whole mask and is forced set in the thinned one.  (At m near n / 3 a frame of the
other tests holds a few pixels of each of these conditions by chance; here one is there by construction, at every length class, every
floor_k and in every kernel family, whatever the hashes of a later geometry give.)

k_insert_positions / k_insert_records run only inside rbf_encode_gop, which plans its own parameters, and the HASHED k_insert_tab only
for frames whose hash table would pass 96 MB (3.1 M pixels): both are out of reach of explicit parameters at this geometry."""
import collections
import json
import os
import subprocess

import numpy as np

import bloom_rows as br
import plan_boundaries as pb
import value_key_ref as vk
from new_bloom_filter_repo_amd import params as P

W, H = 509, 257
N = W * H
U64_MAX = (1 << 64) - 1
SEED_TRIPLES = (tuple(int(s) for s in P.SEEDS_VIDEO), vk.SEEDS_WIDE)
SEED_IDS = ("video", "wide")
KNOBS = br.KNOBS + [32]                                            # 32: no hash table, the insert kernel hashes (k_insert_lds)
KNOB_IDS = br.KNOB_IDS + ["hash_in_insert"]
BASE_DENSITY, BASE_SEED = 0.09, 2500
LOAD = 0.5                                                         # probes per filter bit of a thinned length frame: 1 - exp(-0.5) = 39 % full
F64_RANGE = (1 << 15, 1 << 23)                                    # the FP64 kernels by default, the Barrett kernels under knob 8
SMALL_RANGE = (2, 1 << 15)                                         # always the Barrett kernels
F64_FIT = 638721                                                   # from here on 128 frames no longer fit k_query_u64's LDS (plan_boundaries.ROWS)
SMALL_MIN = 1024                                                   # a filter with room to show a wrong position
LENGTH_BATCHES = ("f64", "f64far", "small")
LENGTH_FLOOR_K = (0, 1, 2, 5, 6, 64)                               # 0 rides on T = 2^64 - 1; 5 | 6: the end of the row passes
LENGTH_T = 1 << 63                                                 # every other length frame: about half of the pixels take the extra probe
SEARCH_PIXELS = 64
CONDITIONS = ("pos_0", "pos_m-1", "step_0", "step_m-1", "sum_m", "sum_m-1")
# (floor_k, m) of the threshold and rank frames, cycled: every class of k_query_u64 (1 .. 5, then everything else), each about 40 % full
# under the whole mask, every m inside the FP64 range and small enough for two LDS buffers next to 128 frame records
GEOMETRIES = ((1, 40009), (2, 60013), (3, 80021), (5, 120011), (4, 100003), (6, 150001), (0, 32771))
RANK_COUNTS = (1, 2, 3, 5, 127, 128)
RANK_KINDS = ("equal", "distinct", "duplicates", "interleaved")
RANK_PINNED = 4                                                    # frames of a rank batch whose tie is made to matter (the others: as it comes)
INDEX_RANDOM = 200
KERNELS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bloom_params_kernels.json")


# ------------------------------------------------------------------ hashes and masks
_HASHES, _RESIDUES, _FRAMES = {}, {}, {}


def hashes(oracle, seeds):
    """(h1, h2, ha): uint64 [N] each, XXH64(str(i), seed) of every pixel index, from the C oracle.  Cached per seed triple."""
    seeds = tuple(int(s) for s in seeds)
    if seeds not in _HASHES:
        fn = oracle.lib().orc_hash_index
        _HASHES[seeds] = tuple(np.array([fn(i, s) for i in range(N)], dtype=np.uint64) for s in seeds)
    return _HASHES[seeds]


def base_mask():
    return pb.random_mask(BASE_SEED, N, BASE_DENSITY)


Case = collections.namedtuple("Case", "name seeds m floor_k T set clear keep")
Case.__new__.__defaults__ = ((), (), 1.0)


def uncoded(seeds, name="uncoded"):
    return Case(name, seeds, 0, 0, 0)


def case_mask(case):
    """The case's mask: the base mask, thinned to the fraction `keep` (seeded by m), with the case's pixels forced."""
    mask = base_mask()
    if case.keep < 1.0:
        mask &= (np.random.default_rng(7000 + case.m).random(N) < case.keep).astype(np.uint8)
    mask[np.array(case.set, np.int64)] = 1
    mask[np.array(case.clear, np.int64)] = 0
    return mask


# ------------------------------------------------------------------ the reference
def residues(h, m):
    key = (id(h[0]), m)                                            # (the hash arrays are cached: one object per seed triple)
    if key not in _RESIDUES:
        if len(_RESIDUES) > 64:
            _RESIDUES.clear()
        _RESIDUES[key] = (h[0] % np.uint64(m), h[1] % np.uint64(m))
    return _RESIDUES[key]


def positions(h, m, j, idx):
    """(h1 % m + j * (h2 % m)) % m of the pixels idx: uint64 throughout (j <= 64, m < 2^32: no overflow)."""
    a, s = residues(h, m)
    return (a[idx] + np.uint64(j) * s[idx]) % np.uint64(m)


def activated(h, T, le=False):
    """ha < T.  le: the mistake the pairs are there to catch (ha <= T); tests/test_bloom_params_cpu.py shows that it fails them."""
    return h[2] <= np.uint64(T) if le else h[2] < np.uint64(T)


def filter_bits(h, mask, m, floor_k, T, le=False):
    """uint8 [m] of 0 / 1: the OR over the set pixels of positions j < floor_k, and j = floor_k iff the pixel is activated."""
    bits = np.zeros(m, np.uint8)
    on = np.flatnonzero(mask)
    for j in range(floor_k):
        bits[positions(h, m, j, on)] = 1
    bits[positions(h, m, floor_k, on[activated(h, T, le)[on]])] = 1
    return bits


def passing(h, bits, m, floor_k, T, idx, le=False):
    """bool per pixel of idx: every one of its positions is set in bits."""
    idx = np.asarray(idx, np.int64)
    ok = np.ones(len(idx), bool)
    for j in range(floor_k):
        alive = np.flatnonzero(ok)
        ok[alive] = bits[positions(h, m, j, idx[alive])] == 1
    alive = np.flatnonzero(ok)
    alive = alive[activated(h, T, le)[idx[alive]]]
    ok[alive] = bits[positions(h, m, floor_k, idx[alive])] == 1
    return ok


def reference(h, mask, m, floor_k, T, le=False):
    """bloom_rows.Frame of a mask under explicit integer parameters (k = 0.0: there is no k*).  The witness is the mask bits of the pixels
    that pass, in index order.  m == 0: the frame is not coded."""
    mask = np.ascontiguousarray(mask, np.uint8)
    none = np.zeros(0, np.uint8)
    if not m:
        return br.Frame(mask, int(mask.sum()), 0.0, 0, 0, 0, none, 0, 0, none)
    bits = filter_bits(h, mask, m, floor_k, T, le)
    witness = mask[passing(h, bits, m, floor_k, T, np.arange(len(mask)), le)]
    return br.Frame(mask, int(mask.sum()), 0.0, int(m), int(floor_k), int(T), br.padded(bits), int(bits.sum()), len(witness), br.padded(witness))


def frame_of(oracle, case):
    """The case's reference Frame.  Cached: computed once per process, whatever knob the device then runs."""
    if case[1:] not in _FRAMES:                                    # (frames of different batches share parameters and mask: the name is no part of the key)
        _FRAMES[case[1:]] = reference(hashes(oracle, case.seeds), case_mask(case), case.m, case.floor_k, case.T)
    return _FRAMES[case[1:]]


def same_output(a, b):
    return (a.filter.tobytes(), a.filter_ones, a.witness_bits, a.witness.tobytes()) == (b.filter.tobytes(), b.filter_ones, b.witness_bits, b.witness.tobytes())


# ------------------------------------------------------------------ thresholds
Thresholds = collections.namedtuple("Thresholds", "cases pairs tag members")
_THRESHOLDS = {}


def _pair(oracle, seeds, name, at, candidates, force, also=()):
    """(case at T = ha[i], case at T + 1) for the first pixel i of `candidates`, under the first geometry from `at` on, for which the two
    reference outputs differ.  force: "set" (with the pixels `also`) | "clear"."""
    ha = hashes(oracle, seeds)[2]
    for i in candidates:
        for g in range(len(GEOMETRIES)):
            fk, m = GEOMETRIES[(at + g) % len(GEOMETRIES)]
            forced = dict(set=tuple(also) or (int(i),)) if force == "set" else dict(clear=(int(i),))
            lo = Case("%s_%d" % (name, i), seeds, m, fk, int(ha[i]), **forced)
            hi = lo._replace(name=lo.name + "+1", T=int(ha[i]) + 1)
            if not same_output(frame_of(oracle, lo), frame_of(oracle, hi)):
                return lo, hi
            del _FRAMES[lo[1:]], _FRAMES[hi[1:]]
    raise AssertionError("no pixel of %s gives a pair that matters" % name)


def threshold_cases(oracle, seeds):
    """Thresholds(cases, pairs, tag, members): one Case per frame; pairs = indices (T, T + 1) into cases; the fullest 16-bit tag of the
    activation hashes and its pixels (forced set in the tag cases)."""
    seeds = tuple(int(s) for s in seeds)
    if seeds in _THRESHOLDS:
        return _THRESHOLDS[seeds]
    ha = hashes(oracle, seeds)[2]
    base = base_mask()
    cases, pairs = [], []

    def single(name, T, **forced):
        fk, m = GEOMETRIES[len(cases) % len(GEOMETRIES)]
        cases.append(Case(name, seeds, m, fk, int(T), **forced))

    def pair(name, candidates, force):
        lo, hi = _pair(oracle, seeds, name, len(cases), candidates, force)
        pairs.append((len(cases), len(cases) + 1))
        cases.extend([lo, hi])

    single("zero", 0)
    single("one", 1)
    single("all", U64_MAX)
    pair("min", [int(np.argmin(ha))], "set")
    pair("max", [int(np.argmax(ha))], "set")
    pair("set", np.flatnonzero(base)[:SEARCH_PIXELS], "set")
    pair("clear", np.flatnonzero(base == 0)[:SEARCH_PIXELS], "clear")
    tags = (ha >> np.uint64(48)).astype(np.int64)
    counts = np.bincount(tags, minlength=1 << 16)
    tag = int(np.argmax(counts))                                  # (the smallest of the fullest)
    members = tuple(int(i) for i in np.flatnonzero(tags == tag))
    by_hash = sorted(members, key=lambda i: int(ha[i]))
    mid = len(by_hash) // 2
    single("tag_floor", tag << 48, set=members)
    single("tag_ceiling", (tag << 48) | ((1 << 48) - 1), set=members)
    lo, hi = _pair(oracle, seeds, "tag_member", len(cases), by_hash[mid:] + by_hash[:mid], "set", also=members)
    pairs.append((len(cases), len(cases) + 1))
    cases.extend([lo, hi])
    single("tag_between", (int(ha[by_hash[mid - 1]]) + int(ha[by_hash[mid]])) // 2, set=members)
    _THRESHOLDS[seeds] = Thresholds(cases, pairs, tag, members)
    return _THRESHOLDS[seeds]


# ------------------------------------------------------------------ lengths
def condition_hits(h1, h2, lo, hi):
    """{condition: the m of lo .. hi - 1 that give it for a pixel with hashes h1, h2}: one numpy scan of the range."""
    ms = np.arange(lo, hi, dtype=np.uint64)
    r1, r2 = np.uint64(h1) % ms, np.uint64(h2) % ms
    last = ms - np.uint64(1)
    tests = (r1 == 0, r1 == last, r2 == 0, r2 == last, r1 + r2 == ms, r1 + r2 == last)
    return {c: ms[t].astype(np.int64) for c, t in zip(CONDITIONS, tests)}


def has_condition(h1, h2, m, cond):
    """The property itself, in Python integers (what the CPU test holds every selected case against)."""
    a, s = int(h1) % m, int(h2) % m
    return {"pos_0": a == 0, "pos_m-1": a == m - 1, "step_0": s == 0, "step_m-1": s == m - 1, "sum_m": a + s == m, "sum_m-1": a + s == m - 1}[cond]


Lengths = collections.namedtuple("Lengths", "found cases")
_LENGTHS = {}


def length_cases(oracle, seeds):
    """Lengths(found, cases).  The set pixels of the base mask are scanned in index order, the first SEARCH_PIXELS at most, every m of
    both ranges once per pixel.  found[(kind, condition)] = (pixel, m):
      f64     the first pixel that offers the condition at an m of [2^15, F64_FIT), with its smallest such m: a batch of these filters fits
              LDS twice, so it takes k_insert_tab + k_query_u64 by default and k_insert_lds + k_query_lds under knob 8
      f64far  that pixel's largest m of the whole range, where it lies at or above F64_FIT: k_query_s64t, and past 5.4 M bits the
              generic insert -- a batch of its own, because the planner plans a batch by its largest filter
      small   the first pixel that offers it at an m of [SMALL_MIN, 2^15), with its smallest such m
      tiny    the first pixel that offers it anywhere below 2^15, with its smallest m (2, 3, 7 ...: mod_m_small at its extreme; such a
              filter is nearly saturated and says little about a position, which is why `small` stands beside it)
    A condition no pixel offers is missing from `found`; the CPU test fails if that is an f64 or a small one.  cases[(batch, condition)]
    for batch in LENGTH_BATCHES: one Case per floor_k of LENGTH_FLOOR_K, the pixel and its two neighbours forced set; the `small` batch
    holds the tiny filter's six frames behind its own."""
    seeds = tuple(int(s) for s in seeds)
    if seeds in _LENGTHS:
        return _LENGTHS[seeds]
    h1, h2, _ = hashes(oracle, seeds)
    on = np.flatnonzero(base_mask())
    ones = len(on)
    found = {}
    need = [(k, c) for k in ("f64", "small", "tiny") for c in CONDITIONS]
    for i in on[:SEARCH_PIXELS]:
        if all(key in found for key in need):
            break
        big, low = condition_hits(h1[i], h2[i], *F64_RANGE), condition_hits(h1[i], h2[i], *SMALL_RANGE)
        for c in CONDITIONS:
            fit = big[c][big[c] < F64_FIT]
            if ("f64", c) not in found and len(fit):
                found["f64", c] = (int(i), int(fit[0]))
                if big[c][-1] >= F64_FIT:
                    found["f64far", c] = (int(i), int(big[c][-1]))
            roomy = low[c][low[c] >= SMALL_MIN]
            if ("small", c) not in found and len(roomy):
                found["small", c] = (int(i), int(roomy[0]))
            if ("tiny", c) not in found and len(low[c]):
                found["tiny", c] = (int(i), int(low[c][0]))

    def six(kind, c):
        if (kind, c) not in found or (kind == "tiny" and found[kind, c] == found.get(("small", c))):
            return []
        i, m = found[kind, c]
        forced = tuple(j for j in (i - 1, i, i + 1) if 0 <= j < N)
        out = []
        for fk in LENGTH_FLOOR_K:
            T = U64_MAX if fk == 0 else LENGTH_T
            keep = min(1.0, LOAD * m / ((fk + T / 2.0 ** 64) * ones))
            out.append(Case("%s-%s-px%d-m%d-k%d" % (kind, c, i, m, fk), seeds, m, fk, T, set=forced, keep=keep))
        return out

    cases = {}
    for c in CONDITIONS:
        for batch, kinds in (("f64", ("f64",)), ("f64far", ("f64far",)), ("small", ("small", "tiny"))):
            rows = [case for kind in kinds for case in six(kind, c)]
            if rows:
                cases[batch, c] = rows
    _LENGTHS[seeds] = Lengths(found, cases)
    return _LENGTHS[seeds]


def index_lists(case, seed=2600):
    """[(inserted, queried), ...] of the per-index surface for a length case.  `few`: the selected pixel and its two neighbours alone --
    the filter is then exactly their positions, whatever its length.  `many`: those and INDEX_RANDOM random indices, shuffled (which
    fill a filter of a few thousand bits).  queried: the inserted ones and INDEX_RANDOM + 3 others."""
    rng = np.random.default_rng(seed + case.m % 1000 + case.floor_k)
    out = []
    for extra in (0, INDEX_RANDOM):
        ins = rng.permutation(np.concatenate([np.array(case.set, np.int64), rng.integers(0, N, extra)])).astype(np.uint32)
        out.append((ins, rng.permutation(np.concatenate([ins.astype(np.int64), rng.integers(0, N, INDEX_RANDOM + 3)])).astype(np.uint32)))
    return out


def index_reference(oracle, case, inserted, queried):
    """(filter bits uint8 [m], verdicts bool per queried index) of inserting `inserted` into an empty filter of the case's parameters."""
    h = hashes(oracle, case.seeds)
    mask = np.zeros(N, np.uint8)
    mask[inserted] = 1
    bits = filter_bits(h, mask, case.m, case.floor_k, case.T)
    return bits, passing(h, bits, case.m, case.floor_k, case.T, queried)


# ------------------------------------------------------------------ whole batches for the rank search
_RANKS = {}


def tie_matters(oracle, case):
    """A frame whose T is the activation hash of a pixel: does `ha <= T` give another output?  (Only the pixels with ha == T change.)"""
    h = hashes(oracle, case.seeds)
    fr = frame_of(oracle, case)
    if not fr.m:
        return False
    bits = np.unpackbits(fr.filter)[:fr.m]
    for i in np.flatnonzero(h[2] == np.uint64(case.T)):
        extra_clear = bits[int(positions(h, fr.m, fr.floor_k, np.array([i]))[0])] == 0
        if extra_clear and (fr.mask[i] or all(bits[int(positions(h, fr.m, j, np.array([i]))[0])] for j in range(fr.floor_k))):
            return True
    return False


def rank_batches(oracle, seeds):
    """{(count, kind): [Case, ...]} for count of RANK_COUNTS and kind of RANK_KINDS.  Every threshold is the activation hash of a set
    pixel of the base mask, drawn in a seeded order that is not sorted; frame f has geometry GEOMETRIES[f % 7].  For the first
    RANK_PINNED frames of a batch the pixel is one whose tie matters (tie_matters)."""
    seeds = tuple(int(s) for s in seeds)
    if seeds in _RANKS:
        return _RANKS[seeds]
    ha = hashes(oracle, seeds)[2]
    pool = [int(i) for i in np.random.default_rng(2700).permutation(np.flatnonzero(base_mask()))]
    out = {}
    for count in RANK_COUNTS:
        take = iter(pool)

        def coded(f, pixel=None, pinned=False):
            fk, m = GEOMETRIES[f % len(GEOMETRIES)]
            while True:
                i = next(take) if pixel is None else pixel
                case = Case("rank%d_f%d_px%d" % (count, f, i), seeds, m, fk, int(ha[i]))
                if pixel is not None or not pinned or tie_matters(oracle, case):
                    return case, i
                del _FRAMES[case[1:]]

        distinct = [coded(f, pinned=f < RANK_PINNED) for f in range(count)]
        out[count, "distinct"] = [c for c, _ in distinct]
        first = distinct[0][1]
        out[count, "equal"] = [coded(f, pixel=first)[0] for f in range(count)]
        dup = [coded(f, pixel=distinct[f // 2][1])[0] if f % 3 == 1 else distinct[f][0] for f in range(count)]
        out[count, "duplicates"] = dup
        rows = list(dup)
        # frames that are not coded, so that the coded count differs from nframes: 127 coded frames fill a launch sequence of 128 rows, 128
        # spill into a second one
        gaps = {count // 2 + 1} if count == 127 else {0 if count == 1 else 1} | ({count // 2 + 1} if count in (5, 128) else set())
        for at in sorted(gaps, reverse=True):
            rows.insert(at, uncoded(seeds, "rank%d_uncoded_at%d" % (count, at)))
        out[count, "interleaved"] = rows
    _RANKS[seeds] = out
    return out


# ------------------------------------------------------------------ every batch the GPU test submits, and what the planner makes of it
def all_batches(oracle, seeds):
    """{name: [Case, ...]}: the threshold frames as one batch, the length cases per (range, condition), the rank compositions."""
    out = {"thresholds": threshold_cases(oracle, seeds).cases}
    for (batch, c), cases in sorted(length_cases(oracle, seeds).cases.items()):
        out["length-%s-%s" % (batch, c)] = cases
    for (count, kind), cases in rank_batches(oracle, seeds).items():
        out["rank-%d-%s" % (count, kind)] = cases
    return out


def chunks(cases):
    """The launch sequences of a batch: rows of MAX_BATCH frames (rbf_bloom_encode_batch, include/rbf.h)."""
    return [cases[at:at + br.MAX_BATCH] for at in range(0, len(cases), br.MAX_BATCH)]


def planner_table(exe, oracle):
    """{seed id: {batch: [per knob of KNOBS, in order, the decisions of the batch's launch sequences joined by "|"]}} from the planner twin
    (tests/c/plan_cases.cpp), in its `decision` notation (tests/bloom_rows.py).  No batch here is mixed: one plan per launch sequence,
    encode and decode alike."""
    table = {}
    for sid, seeds in zip(SEED_IDS, SEED_TRIPLES):
        table[sid] = {}
        for name, cases in all_batches(oracle, seeds).items():
            text = ""
            for knob in KNOBS:
                for ch in chunks(cases):
                    text += "batch %d %d %d 0 %d %s\n" % (N, pb.CUS, knob, len(ch), " ".join(str(c.m) for c in ch))
            out = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            lines = [ln.split() for ln in out.stdout.splitlines()]
            assert len(lines) == 2 * len(KNOBS) * len(chunks(cases)), (name, "a mixed batch prints its halves")
            decisions = []
            for head, plan in zip(lines[0::2], lines[1::2]):
                assert head[:2] == ["batch", "mixed=0"] and plan[0] == "plan", (name, head)
                decisions.append(dict(f.split("=") for f in plan[1:])["decision"])
            per = len(chunks(cases))
            table[sid][name] = ["|".join(decisions[k * per:(k + 1) * per]) for k in range(len(KNOBS))]
    return table


def write_table(table, path=KERNELS_JSON):
    """One line per batch, so that a row that moves shows as one line."""
    with open(path, "w") as f:
        f.write('{"knobs": %s' % json.dumps(KNOB_IDS))
        for sid in SEED_IDS:
            f.write(',\n"%s": {\n' % sid)
            f.write(",\n".join(' %s: %s' % (json.dumps(name), json.dumps(row)) for name, row in sorted(table[sid].items())))
            f.write("\n}")
        f.write("}\n")


def pinned_table():
    with open(KERNELS_JSON) as f:
        return json.load(f)


def kernels_of(decision):
    """The kernels a decision launches, by name (csrc/rbf_plan.h; tests/c/plan_cases.cpp prints the fields)."""
    fast, query, double, tab, two_phase, image = [int(x) for x in decision.split(".")[:6]]
    insert = "k_insert" if not fast else "k_insert_positions" if two_phase else "k_insert_tab" if tab else "k_insert_lds"
    q = {0: "k_query", 1: "k_query_u64" if image else "k_query_lds_double" if double else "k_query_lds_single", 2: "k_query_tiled", 3: "k_query_s64t"}[query]
    return insert, q
