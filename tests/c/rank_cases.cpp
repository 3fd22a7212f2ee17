// rank_cases.cpp -- the activation ranks of the FP64 query kernels (k_query_u64, rbf_kernels_query_f64.h; k_query_s64t,
// rbf_kernels_query_f64_tiled.h) against the plain compare they stand for: no GPU and no HIP compiler needed (g++ -std=c++17).
// The device side is RESTATED here, line for line -- tl[] holds the sorted thresholds of the coded frames, padded with ~0 up to
// 2 * MAX_BATCH entries; `top` is the largest power of two not above the coded count; r |= t <= h ? step : 0 -- and runs against the
// host's REAL c_f: query_table of csrc/rbf_plan.h, which this file includes the way tests/c/plan_cases.cpp does.  For every coded frame f
//     rank(h) <= c_f   <=>   h < T_f
// over every coded count 1 .. 128, with ties, with thresholds 0 and 2^64 - 1, frames that are not coded in between, both orders of the
// table (by class and the batch's own), and h in {t - 1, t, t + 1} of every threshold plus 0 and 2^64 - 2.  The rank must fit the byte
// the kernels keep it in (rank_le, rbf_f64_common.h), and every tl[] index the search forms must lie inside the padded array.
// Prints "ok <checks>" and returns 0, or the first violation and 1.  tests/test_bloom_params_cpu.py
#include "../../new_bloom_filter_repo_amd/csrc/rbf_plan.h"

#include <cstdio>
#include <vector>

static int fail(int code, const char *, ...) { return code; }

// ---- the device's search, restated ----------------------------------------------------------------------------------------------
struct Search {
    uint64_t tl[2 * MAX_BATCH];
    uint32_t top;
    // what thread t < 2 * MAX_BATCH does in the prologue: tl[t] = t < nactive ? tab.f[t].T : ~0
    Search(const FrameTable &q, uint32_t nactive)
    {
        for (uint32_t t = 0; t < 2u * MAX_BATCH; ++t) tl[t] = t < nactive ? q.f[t].T : ~0ull;
        top = 1;
        while (2u * top <= nactive) top *= 2u;
    }
    // -1: an index outside tl[]
    int rank(uint64_t h) const
    {
        uint32_t r = 0;
        for (uint32_t step = top; step; step >>= 1) {
            const uint32_t at = r + step - 1u;
            if (at >= 2u * MAX_BATCH) return -1;
            const uint64_t t = tl[at];
            r |= t <= h ? step : 0u;
        }
        return (int)r;
    }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()                                             // splitmix64
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static unsigned long long checks = 0;

// one batch: thresholds T[f] and floor_k[f] of nframes frames, coded[f] = the frame has a filter
static int run(const char *what, const std::vector<uint64_t> &T, const std::vector<uint32_t> &fk, const std::vector<bool> &coded)
{
    const uint32_t nframes = (uint32_t)T.size();
    FrameTable tab{};
    for (uint32_t f = 0; f < nframes; ++f) tab.f[f] = FrameDev{coded[f] ? 40009u + f : 0u, fk[f], T[f], 0};
    for (int by_class = 0; by_class < 2; ++by_class) {
        U64Classes cls{};
        uint32_t nactive;
        uint64_t empty[2];
        const FrameTable q = query_table(tab, nframes, by_class ? &cls : nullptr, &nactive, empty);
        uint32_t want_active = 0;
        for (uint32_t f = 0; f < nframes; ++f) want_active += coded[f];
        if (nactive != want_active) { printf("%s: nactive %u, coded %u\n", what, nactive, want_active); return 1; }
        if (!nactive) continue;
        const Search s(q, nactive);
        std::vector<uint64_t> hs = {0ull, ~0ull - 1ull};
        for (uint32_t f = 0; f < nframes; ++f)
            if (coded[f]) { hs.push_back(T[f] - 1ull); hs.push_back(T[f]); hs.push_back(T[f] + 1ull); }      // (wrapping at both ends: still hashes)
        for (uint32_t j = 0; j < nactive; ++j) {
            const uint32_t f = q.f[j].floor_k >> 16, c = (q.f[j].floor_k >> 8) & 0xFFu;
            if (f >= nframes || !coded[f] || (q.f[j].floor_k & 0xFFu) != (fk[f] & 0xFFu)) { printf("%s: entry %u names frame %u\n", what, j, f); return 1; }
            for (uint64_t h : hs) {
                const int r = s.rank(h);
                ++checks;
                if (r < 0) { printf("%s: coded %u h %llx: an index past tl[]\n", what, nactive, (unsigned long long)h); return 1; }
                if (r > 255) { printf("%s: coded %u h %llx: rank %d does not fit a byte\n", what, nactive, (unsigned long long)h, r); return 1; }
                if (((uint32_t)r <= c) != (h < T[f])) {
                    printf("%s: by_class %d coded %u frame %u T %llx h %llx: rank %d c_f %u\n", what, by_class, nactive, f, (unsigned long long)T[f],
                           (unsigned long long)h, r, c);
                    return 1;
                }
            }
        }
        // the rank of a lane without a pixel (its hash stays ~0): every entry counts, the padding included
        if (s.rank(~0ull) != (int)(2u * s.top - 1u) || 2u * s.top - 1u > 255u) { printf("%s: coded %u: rank of ~0 is %d\n", what, nactive, s.rank(~0ull)); return 1; }
    }
    return 0;
}

int main()
{
    for (uint32_t count = 1; count <= (uint32_t)MAX_BATCH; ++count) {
        std::vector<uint32_t> fk(count);
        std::vector<bool> all(count, true);
        for (uint32_t f = 0; f < count; ++f) fk[f] = f % 8;                                                   // every class of k_query_u64, 0 and 6, 7 in the last
        std::vector<uint64_t> T(count);
        // all equal -- in the middle and at both ends of the range
        for (uint64_t v : {0x8000000000000000ull, 0ull, ~0ull, 1ull, ~0ull - 1ull}) {
            std::fill(T.begin(), T.end(), v);
            if (run("equal", T, fk, all)) return 1;
        }
        // all distinct, in an order that is not sorted
        for (uint32_t f = 0; f < count; ++f) T[f] = rnd();
        if (run("distinct", T, fk, all)) return 1;
        // neighbours: t, t + 1, t + 2, ... in descending order
        for (uint32_t f = 0; f < count; ++f) T[f] = 0x123456789ABCDEFull + (count - f);
        if (run("neighbours", T, fk, all)) return 1;
        // duplicates mixed in, with 0 and 2^64 - 1 among them
        for (uint32_t f = 0; f < count; ++f) T[f] = f % 3 == 1 ? T[f / 2] : rnd();
        if (count > 1) T[count / 2] = 0;
        if (count > 2) T[0] = ~0ull;
        if (count > 3) T[count - 1] = ~0ull;
        if (count > 4) T[1] = 0;
        if (run("duplicates", T, fk, all)) return 1;
    }
    // frames that are not coded in between: the coded count differs from nframes
    for (uint32_t nframes = 2; nframes <= (uint32_t)MAX_BATCH; ++nframes) {
        std::vector<uint64_t> T(nframes);
        std::vector<uint32_t> fk(nframes);
        std::vector<bool> coded(nframes);
        for (uint32_t f = 0; f < nframes; ++f) {
            T[f] = f % 4 == 0 ? 0x4000000000000000ull : rnd();
            fk[f] = 1 + f % 6;
            coded[f] = f % 3 != 1;
        }
        if (run("interleaved", T, fk, coded)) return 1;
    }
    printf("ok %llu\n", checks);
    return 0;
}
