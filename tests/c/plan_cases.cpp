// plan_cases.cpp -- prints the launch planner's decisions (csrc/rbf_plan.h), one line per case read from stdin; no GPU and no HIP
// compiler needed (g++ -std=c++17).
//   case:  n nframes cus flags insert_slices have_ones m [m0]
// flags: the argument of rbf_ctx_force_generic; insert_slices: RBF_OPT_INSERT_SLICES; every frame has a filter of m bits, frame 0
// one of m0 bits when m0 is given (a mixed batch: the two halves of split_by_family are planned and printed as well).
//   table: "table by_class full nframes", then one line "m floor_k T" per frame
// prints what query_table returns for that batch: nactive, the class counts (by_class = 1), the `empty` bits, with full = 1 every
// coded entry as m:M:floor_k:T (hex), and always the 64-bit FNV-1a of the table's bytes.
//   batch: "batch n cus flags have_ones nframes m_0 ... m_{nframes-1}": every frame its own filter size; see show_batch
//   sweep: "sweep n nframes cus flags have_ones lo hi step [coded]" (the first `coded` frames, default all, have a filter of m bits,
// the others none: the batch rbf_encode_gop submits for a GOP whose later pairs did not change)
// walks m = lo, lo + step, ... up to hi and, wherever the decision differs between two samples, every m in between: one line
// "transition last=M first=M+1 before=D after=D" per change.  D is the `decision` field every plan line carries too -- what the launch
// code (rbf_api.hip) reads to choose kernels and tile counts, see decision() -- next to query_tiles and the dynamic LDS the host would
// launch the query with (launch_query_lds; insert_lds is the insert kernels').  tests/test_plan_boundaries_cpu.py
#include "../../new_bloom_filter_repo_amd/csrc/rbf_plan.h"

#include <cstdio>
#include <vector>

static int fail(int code, const char *, ...) { return code; }

// tiles the query kernel walks: the tiled kernels' count, 1 for a whole filter in LDS, 0 for the global-memory kernel
static uint32_t query_tiles(const Plan &p)
{
    if (p.query == QueryKind::LdsWhole) return 1;
    if (p.query == QueryKind::Generic) return 0;
    return (p.fwords_max + p.query_tile_words - 1) / p.query_tile_words;
}

// bytes of dynamic LDS launch_query (rbf_api.hip) passes for a batch of `coded` coded frames
static size_t launch_query_lds(const Plan &p, uint32_t coded)
{
    if (p.query == QueryKind::LdsTiledF64) return s64t_lds_bytes(p.query_tile_words);
    if (p.reads_probe_image()) return p.query_lds_bytes + u64_geo_bytes(coded);
    return p.query == QueryKind::Generic ? 0 : p.query_lds_bytes;
}

// The plan as the launch code reads it: fast_insert.query.double_buffer.insert_tab.two_phase.probe_image.insert_tiles.query_tiles.
// Fields nothing reads in that state are 0: double_buffer outside k_query_lds (k_query_u64 always has two buffers, the tiled kernels
// one), the insert's tile count and kernel choice when k_insert runs.
static void decision(const Plan &p, char (&out)[64])
{
    const bool lds_barrett = p.query == QueryKind::LdsWhole && !p.reads_probe_image();
    snprintf(out, sizeof out, "%d.%d.%d.%d.%d.%d.%u.%u", p.fast_insert, (int)p.query, lds_barrett && p.double_buffer, p.insert_tab,
             p.insert_two_phase, p.reads_probe_image(), p.fast_insert ? p.insert_tiles : 0u, query_tiles(p));
}

static int sweep(const char *line)
{
    unsigned long long n;
    unsigned nframes, cus, have_ones, lo, hi, step, coded;
    int flags;
    const int got = sscanf(line, "sweep %llu %u %u %d %u %u %u %u %u", &n, &nframes, &cus, &flags, &have_ones, &lo, &hi, &step, &coded);
    if (got < 8 || nframes < 1 || nframes > (unsigned)MAX_BATCH || step < 1 || lo > hi) return 2;
    if (got < 9) coded = nframes;
    if (coded < 1 || coded > nframes) return 2;
    Knobs k;
    k.set_flags(flags);
    std::vector<rbf_filter_params> params(nframes);
    auto decide = [&](uint32_t m, char (&out)[64]) {
        for (unsigned f = 0; f < nframes; ++f) params[f] = rbf_filter_params{f < coded ? m : 0u, 1, 0};
        decision(make_plan(k, cus, params.data(), nframes, n, have_ones != 0), out);
    };
    char prev[64], cur[64], a[64], b[64];
    decide(lo, prev);
    for (uint64_t m0 = lo; m0 < hi;) {
        const uint64_t m1 = std::min<uint64_t>(m0 + step, hi);
        decide((uint32_t)m1, cur);
        if (strcmp(prev, cur)) {
            memcpy(a, prev, sizeof a);
            for (uint64_t m = m0 + 1; m <= m1; ++m) {
                decide((uint32_t)m, b);
                if (strcmp(a, b)) printf("transition last=%llu first=%llu before=%s after=%s\n", (unsigned long long)(m - 1), (unsigned long long)m, a, b);
                memcpy(a, b, sizeof a);
            }
        }
        memcpy(prev, cur, sizeof prev);
        m0 = m1;
    }
    printf("swept lo=%u hi=%u step=%u\n", lo, hi, step);
    return 0;
}

static void show(const char *tag, const Plan &p, uint32_t nframes)
{
    char d[64];
    decision(p, d);
    uint32_t coded = 0;
    for (uint32_t f = 0; f < (uint32_t)MAX_BATCH; ++f) coded += p.slices.n[f] != 0;
    printf("%s fast_insert=%d query=%d double_buffer=%d small_m=%d insert_tab=%d two_phase=%d f64_mod=%d probe_image=%d fwords_max=%u S=%u "
           "per_tile=%u insert_group=%u insert_tile_words=%u insert_tiles=%u query_tile_words=%u insert_lds=%zu query_lds=%zu nseg=%llu "
           "words_per_seg=%u image_stride=%u decision=%s query_tiles=%u launch_query_lds=%zu lds_limit=%zu slices=",
           tag, p.fast_insert, (int)p.query, p.double_buffer, p.small_m, p.insert_tab, p.insert_two_phase, p.f64_mod, p.reads_probe_image(),
           p.fwords_max, p.S, p.per_tile, p.insert_group, p.insert_tile_words, p.insert_tiles, p.query_tile_words, p.insert_lds_bytes,
           p.query_lds_bytes, (unsigned long long)p.nseg, p.words_per_seg, p.image_stride_words, d, query_tiles(p), launch_query_lds(p, coded), LDS_LIMIT);
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

// "batch n cus flags have_ones nframes m_0 ... m_{nframes-1}": a batch in which every frame has its own filter size (0: not coded), as
// rbf_bloom_encode_batch / rbf_bloom_decode_batch (have_ones = 0) or rbf_encode_gop_finish (1) plan it.  Prints the undivided plan and,
// when the batch is mixed, its two halves -- each with the conditions under which encode_chunk / decode_chunk (rbf_api.hip) run the
// halves instead of the whole: encode_split / decode_split.  tests/test_bloom_rows_cpu.py, tests/test_bloom_params_cpu.py
static int show_batch(char *line)
{
    unsigned long long n;
    unsigned cus, have_ones, nframes;
    int flags, used = 0;
    if (sscanf(line, "batch %llu %u %d %u %u%n", &n, &cus, &flags, &have_ones, &nframes, &used) < 5 || nframes < 1 || nframes > (unsigned)MAX_BATCH) return 2;
    std::vector<rbf_filter_params> params(nframes), small(nframes), big(nframes);
    char *at = line + used;
    for (unsigned f = 0; f < nframes; ++f) {
        char *end;
        const unsigned long long m = strtoull(at, &end, 10);
        if (end == at) return 2;
        params[f] = rbf_filter_params{(uint32_t)m, 1, 0};
        at = end;
    }
    Knobs k;
    k.set_flags(flags);
    const Plan pl = make_plan(k, cus, params.data(), nframes, n, have_ones != 0);
    const bool mixed = split_by_family(params.data(), nframes, small.data(), big.data());
    int encode_split = 0, decode_split = 0;
    if (mixed && k.fp64_kernels()) {
        const Plan ps = make_plan(k, cus, small.data(), nframes, n, false), pb = make_plan(k, cus, big.data(), nframes, n, have_ones != 0);
        const Plan pd = make_plan(k, cus, params.data(), nframes, n, false), pbd = make_plan(k, cus, big.data(), nframes, n, false);
        encode_split = !k.no_hash_table && pb.reads_probe_image() && pb.insert_tab && ps.nseg == pb.nseg && ps.words_per_seg == pb.words_per_seg;
        decode_split = pbd.reads_probe_image() && ps.nseg == pd.nseg && pbd.nseg == pd.nseg && ps.words_per_seg == pd.words_per_seg &&
                       pbd.words_per_seg == pd.words_per_seg;
    }
    printf("batch mixed=%d encode_split=%d decode_split=%d\n", mixed, encode_split, decode_split);
    show("plan", pl, nframes);
    if (mixed) {
        show("small", make_plan(k, cus, small.data(), nframes, n, false), nframes);
        show("big", make_plan(k, cus, big.data(), nframes, n, have_ones != 0), nframes);
    }
    return 0;
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "table", 5)) {
            if (int r = show_table(line)) return r;
            continue;
        }
        if (!strncmp(line, "batch", 5)) {
            if (int r = show_batch(line)) return r;
            continue;
        }
        if (!strncmp(line, "sweep", 5)) {
            if (int r = sweep(line)) return r;
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
