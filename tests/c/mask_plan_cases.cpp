// mask_plan_cases.cpp -- the temporal chunks of the GOP mask kernels as csrc/rbf_mask_plan.h plans them; no GPU and no HIP compiler
// needed (g++ -std=c++17).
//   plan:   lines "nframes wanted fast_segs skip" on stdin, skip = "null" or nframes - 1 characters '0' / '1' (pair p is not coded).
//           `wanted` is rbf_ctx_force_generic's bits 8..12 (0 = auto).  Prints per line
//             "grid_y count ppc skip_in_table first:pairs:skipped ..."   (the entries: only when count != 0)
//   check:  the properties of tests/test_mask_stage_cpu.py over nframes 2..300 x wanted 0..31 x fast_segs {1, 4, 2025} x the run patterns,
//           checked here as well so that the sanitizer build walks every table; prints "ok <plans>".
#include "../../new_bloom_filter_repo_amd/csrc/rbf_mask_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int fail(int code, const char *, ...) { return code; }

struct Planned {
    uint32_t grid_y;
    MaskChunks mc;
    bool skip_in_table;
};

static Planned plan(uint32_t nframes, uint32_t wanted, uint64_t fast_segs, const uint8_t *skip)
{
    Knobs k;
    k.set_flags((int)(wanted << 8));
    Planned p{};
    p.grid_y = plan_mask_chunks(k, nframes, fast_segs, skip, &p.mc, &p.skip_in_table);
    return p;
}

static void show(const Planned &p)
{
    printf("%u %u %u %d", p.grid_y, p.mc.count, p.mc.ppc, p.skip_in_table ? 1 : 0);
    for (uint32_t y = 0; y < p.mc.count; ++y)
        printf(" %u:%u:%d", p.mc.first[y], p.mc.pairs[y] & (MASK_CHUNK_SKIP - 1u), (p.mc.pairs[y] & MASK_CHUNK_SKIP) ? 1 : 0);
    printf("\n");
}

// every property of a plan, against the skip bytes it was made from; 0 = holds
static int holds(const Planned &p, uint32_t nframes, const uint8_t *skip)
{
    const uint32_t pairs = nframes - 1;
    std::vector<int> seen(pairs, 0);
    if (p.mc.count == 0) {                                        // uniform chunks: the kernel's own f0 / f1
        if (p.skip_in_table || p.mc.ppc == 0) return 1;
        if ((uint64_t)p.grid_y * p.mc.ppc < pairs) return 2;
        if (p.grid_y == 0 || (uint64_t)(p.grid_y - 1) * p.mc.ppc >= pairs) return 3;      // no empty chunk at the end
        return 0;
    }
    if (!skip || !p.skip_in_table || p.grid_y != p.mc.count || p.mc.count > MASK_MAX_CHUNKS) return 4;
    for (uint32_t y = 0; y < p.mc.count; ++y) {
        const uint32_t f0 = p.mc.first[y], len = p.mc.pairs[y] & (MASK_CHUNK_SKIP - 1u);
        const bool skipped = (p.mc.pairs[y] & MASK_CHUNK_SKIP) != 0;
        if (len == 0 || f0 + len > pairs) return 5;
        for (uint32_t f = f0; f < f0 + len; ++f) {
            if ((skip[f] != 0) != skipped) return 6;              // a coded chunk never spans a run start, a skip chunk only holds skipped pairs
            if (seen[f]++) return 7;
        }
    }
    for (uint32_t f = 0; f < pairs; ++f) if (seen[f] != 1) return 8;
    return 0;
}

static std::vector<std::vector<uint8_t>> patterns(uint32_t nframes)
{
    const uint32_t pairs = nframes - 1;
    auto from_starts = [&](std::vector<uint32_t> starts) {
        std::vector<uint8_t> s(pairs, 0);
        for (uint32_t t : starts) if (t >= 1 && t < nframes) s[t - 1] = 1;
        return s;
    };
    std::vector<std::vector<uint8_t>> out;
    std::vector<uint32_t> every2;
    for (uint32_t t = 2; t < nframes; t += 2) every2.push_back(t);
    out.push_back(from_starts({}));
    out.push_back(from_starts(every2));
    out.push_back(from_starts({nframes / 2, nframes / 2 + 1}));
    out.push_back(from_starts({1}));
    out.push_back(from_starts({nframes - 1}));
    out.push_back(std::vector<uint8_t>(pairs, 1));                // every frame a keyframe: nothing is coded
    return out;
}

static int check()
{
    unsigned long plans = 0;
    for (uint32_t nframes = 2; nframes <= 300; ++nframes)
        for (uint32_t wanted = 0; wanted < 32; ++wanted)
            for (uint64_t segs : {1ull, 4ull, 2025ull}) {
                const Planned none = plan(nframes, wanted, segs, nullptr);
                if (int r = holds(none, nframes, nullptr)) { printf("null nframes %u wanted %u: property %d\n", nframes, wanted, r); return 1; }
                ++plans;
                for (const auto &s : patterns(nframes)) {
                    const Planned p = plan(nframes, wanted, segs, s.data());
                    if (int r = holds(p, nframes, s.data())) { printf("nframes %u wanted %u: property %d\n", nframes, wanted, r); return 1; }
                    ++plans;
                }
            }
    // a block too long for 15-bit chunk lengths takes the uniform chunks, runs or not
    std::vector<uint8_t> s(0x8000 - 1, 0);
    s[100] = 1;
    const Planned big = plan(0x8000, 4, 4, s.data());
    if (big.mc.count != 0 || big.skip_in_table || holds(big, 0x8000, s.data())) { printf("nframes 0x8000: not the fallback\n"); return 1; }
    printf("ok %lu\n", plans + 1);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "check") return check();
    if (argc < 2 || std::string(argv[1]) != "plan") return 2;
    char *line = nullptr;
    size_t cap = 0;
    std::vector<char> skip_text(1 << 16);
    while (getline(&line, &cap, stdin) > 0) {
        unsigned nframes, wanted;
        unsigned long long segs;
        if (sscanf(line, "%u %u %llu %65535s", &nframes, &wanted, &segs, skip_text.data()) != 4 || nframes < 2 || wanted > 31 || segs < 1) { free(line); return 2; }
        const std::string st(skip_text.data());
        std::vector<uint8_t> skip;
        if (st != "null") {
            if (st.size() != nframes - 1) { free(line); return 2; }
            for (char ch : st) skip.push_back(ch == '1');
        }
        const Planned p = plan(nframes, wanted, segs, st == "null" ? nullptr : skip.data());
        if (int r = holds(p, nframes, st == "null" ? nullptr : skip.data())) { printf("property %d\n", r); free(line); return 1; }
        show(p);
    }
    free(line);
    return 0;
}
