// plan_cases.cpp -- prints the launch planner's decisions (csrc/rbf_plan.h), one line per case read from stdin; no GPU and no HIP
// compiler needed (g++ -std=c++17).
//   case:  n nframes cus flags insert_slices have_ones m [m0]
// flags: the argument of rbf_ctx_force_generic; insert_slices: RBF_OPT_INSERT_SLICES; every frame has a filter of m bits, frame 0
// one of m0 bits when m0 is given (a mixed batch: the two halves of split_by_family are planned and printed as well).
//   table: "table by_class full nframes", then one line "m floor_k T" per frame
// prints what query_table returns for that batch: nactive, the class counts (by_class = 1), the `empty` bits, with full = 1 every
// coded entry as m:M:floor_k:T (hex), and always the 64-bit FNV-1a of the table's bytes.
#include "../../new_bloom_filter_repo_amd/csrc/rbf_plan.h"

#include <cstdio>
#include <vector>

static int fail(int code, const char *, ...) { return code; }

static void show(const char *tag, const Plan &p, uint32_t nframes)
{
    printf("%s fast_insert=%d query=%d double_buffer=%d small_m=%d insert_tab=%d two_phase=%d f64_mod=%d probe_image=%d fwords_max=%u S=%u "
           "per_tile=%u insert_group=%u insert_tile_words=%u insert_tiles=%u query_tile_words=%u insert_lds=%zu query_lds=%zu nseg=%llu "
           "words_per_seg=%u image_stride=%u slices=",
           tag, p.fast_insert, (int)p.query, p.double_buffer, p.small_m, p.insert_tab, p.insert_two_phase, p.f64_mod, p.reads_probe_image(),
           p.fwords_max, p.S, p.per_tile, p.insert_group, p.insert_tile_words, p.insert_tiles, p.query_tile_words, p.insert_lds_bytes,
           p.query_lds_bytes, (unsigned long long)p.nseg, p.words_per_seg, p.image_stride_words);
    for (uint32_t f = 0; f < (uint32_t)MAX_BATCH; ++f)
        if (f < nframes || p.slices.n[f]) printf("%x,", p.slices.n[f]);
    printf("\n");
}

static int show_table(char *line)
{
    unsigned by_class, full, nframes;
    if (sscanf(line, "table %u %u %u", &by_class, &full, &nframes) != 3 || nframes > (unsigned)MAX_BATCH) return 2;
    FrameTable tab{};
    for (unsigned f = 0; f < nframes; ++f) {
        unsigned long long T;
        if (!fgets(line, 256, stdin) || sscanf(line, "%u %u %llu", &tab.f[f].m, &tab.f[f].floor_k, &T) != 3) return 2;
        tab.f[f].T = T;
    }
    U64Classes cls{};
    uint32_t nactive;
    uint64_t empty[2];
    const FrameTable q = query_table(tab, nframes, by_class ? &cls : nullptr, &nactive, empty);
    printf("table nactive=%u cls=", nactive);
    for (int k = 0; k < U64_CLASSES; ++k) printf(by_class ? "%u," : "-", cls.n[k]);
    printf(" empty=%llx,%llx", (unsigned long long)empty[0], (unsigned long long)empty[1]);
    for (uint32_t j = 0; full && j < nactive; ++j)
        printf(" %x:%llx:%x:%llx", q.f[j].m, (unsigned long long)q.f[j].M, q.f[j].floor_k, (unsigned long long)q.f[j].T);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < sizeof q; ++i) h = (h ^ reinterpret_cast<const unsigned char *>(&q)[i]) * 0x100000001b3ull;
    printf(" fnv=%016llx\n", (unsigned long long)h);
    return 0;
}

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "table", 5)) {
            if (int r = show_table(line)) return r;
            continue;
        }
        unsigned long long n;
        unsigned nframes, cus, slices, have_ones, m, m0;
        int flags;
        const int got = sscanf(line, "%llu %u %u %d %u %u %u %u", &n, &nframes, &cus, &flags, &slices, &have_ones, &m, &m0);
        if (got < 7 || nframes < 1 || nframes > (unsigned)MAX_BATCH) return 2;
        Knobs k;
        k.set_flags(flags);
        k.insert_slices = slices;
        std::vector<rbf_filter_params> params(nframes, rbf_filter_params{m, 1, 0}), small(nframes), big(nframes);
        if (got == 8) params[0].m = m0;
        show("plan", make_plan(k, cus, params.data(), nframes, n, have_ones != 0), nframes);
        if (split_by_family(params.data(), nframes, small.data(), big.data())) {
            show("small", make_plan(k, cus, small.data(), nframes, n, false), nframes);
            show("big", make_plan(k, cus, big.data(), nframes, n, have_ones != 0), nframes);
        }
    }
    return 0;
}
