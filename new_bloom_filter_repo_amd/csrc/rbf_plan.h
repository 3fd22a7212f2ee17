// rbf_plan.h -- which kernels serve a batch, with what geometry, and the frame tables they read.  Pure host code over rbf_geometry.h
// and the C ABI's types: no HIP header, no context, so tests/c/plan_cases.cpp is built with a plain host compiler and runs on a machine
// without a GPU (tests/test_plan_cpu.py pins the measured crossovers below and the query tables).
#pragma once
#include "../../include/rbf.h"
#include "rbf_geometry.h"

#include <algorithm>
#include <cstring>

using namespace rbf;

static int fail(int code, const char *fmt, ...);                  // sets the thread's last-error text (rbf_host.h; a test brings its own)

// The test and tuning flags of a context, as rbf_ctx_force_generic / rbf_ctx_option decode them.
struct Knobs {
    bool force_generic = false;            // tests: never use the LDS fast path
    bool single_buffer = false;            // tests: fast query path without filter double-buffering
    bool force_generic_mask_bits = false;  // tests: per-pixel threshold compare even for threshold 0
    bool barrett_only = false;             // tests/tuning: never take the FP64 reductions (mod_m_f64)
    bool hash_rebuild = false;             // run k_hash_table for every batch instead of taking the table the last query kernel wrote
    bool no_hash_table = false;            // the insert kernel hashes the set positions itself
    bool no_two_phase = false;             // tiled k_insert_tab even when the filter needs several LDS tiles
    bool hash_positions = false;           // k_insert_positions hashes the set positions itself whatever the table size
    bool no_table_rewrite = false;         // the query kernel never rewrites the hash table, sole holder or not
    bool no_fused_finish = false;          // always the separate k_finish_ones launch (RBF_OPT_SEPARATE_FINISH)
    uint32_t mask_chunks = 0;              // tuning: temporal chunks of the GOP mask kernel (0 = auto)
    uint32_t tile_words = 0;               // tests/tuning: cap the LDS filter tile (dwords); forces the tiled kernels
    uint32_t insert_slices = 0;            // tuning (RBF_OPT_INSERT_SLICES): mask slices per frame of the single-tile insert, 0 = auto
    // rbf_ctx_force_generic's argument: bit 6 is unused, RBF_OPT_* options are not touched
    void set_flags(int on)
    {
        force_generic = on & 1;
        single_buffer = on & 2;
        force_generic_mask_bits = on & 4;
        barrett_only = on & 8;
        hash_rebuild = on & 16;
        no_hash_table = on & 32;
        no_two_phase = on & 128;
        mask_chunks = (uint32_t)(on >> 8) & 0x1F;               // tuning knob, bits 8..12
        hash_positions = on & (1 << 14);
        no_table_rewrite = on & (1 << 15);
        tile_words = ((uint32_t)on >> 16) << 6;                 // bits 16..31: LDS tile cap in units of 64 dwords
    }
    // the FP64 kernel families may run at all (a mixed batch is split over the two families only then)
    bool fp64_kernels() const { return !force_generic && !barrett_only && !single_buffer; }
};

// ------------------------------------------------------------------------------------------
// frame tables
// ------------------------------------------------------------------------------------------
static inline FrameDev frame_dev(const rbf_filter_params &p)
{
    return FrameDev{p.m, p.floor_k, p.threshold, p.m >= 2 ? (uint64_t)((((unsigned __int128)1) << 64) / p.m) : 0};
}

static int fill_table(const rbf_filter_params *params, uint32_t count, FrameTable *tab)
{
    memset(tab, 0, sizeof *tab);
    for (uint32_t f = 0; f < count; ++f) {
        if (params[f].floor_k > 64) return fail(RBF_ERANGE, "frame %u: floor_k %u > 64", f, params[f].floor_k);
        tab->f[f] = frame_dev(params[f]);
    }
    return RBF_OK;
}

// The FrameTable the FP64 query kernels read (k_query_u64, rbf_kernels_query_f64.h; k_query_s64t, rbf_kernels_query_f64_tiled.h), from
// the batch's plain table as fill_table leaves it (m, floor_k, T per frame; m == 0: not coded).  COMPACTED over the coded frames
// -- entry j: m, M = bits of -1.0 / m and floor_k = floor(k*) | c << 8 | frame index << 16 of the j-th coded frame (c = coded
// thresholds below the frame's own); T = j-th smallest threshold of the coded frames (the thresholds are only searched, so they need
// not follow the frames' order).
// `cls` non-null (k_query_u64): the coded frames are ORDERED BY CLASS of floor(k*) -- 1, 2, 3, 4, 5, then everything else -- and
// cls->n[k] counts class k; null (k_query_s64t): they keep the batch's order.  `empty`: bit f = frame f is not coded.
static FrameTable query_table(const FrameTable &tab, uint32_t nframes, U64Classes *cls, uint32_t *nactive, uint64_t (&empty)[2])
{
    FrameTable q;
    memset(&q, 0, sizeof q);
    if (cls) memset(cls, 0, sizeof *cls);
    empty[0] = empty[1] = 0;
    uint64_t sorted[MAX_BATCH];
    uint32_t coded = 0;
    for (uint32_t f = 0; f < nframes; ++f) {
        if (tab.f[f].m) sorted[coded++] = tab.f[f].T;
        else empty[f >> 6] |= 1ull << (f & 63);
    }
    std::sort(sorted, sorted + coded);
    uint32_t j = 0;
    for (int k = 0; k < (cls ? U64_CLASSES : 1); ++k)
        for (uint32_t f = 0; f < nframes; ++f) {
            if (!tab.f[f].m) continue;
            const uint32_t fk = tab.f[f].floor_k;
            if (cls && (fk >= 1u && fk <= 5u ? (int)fk - 1 : 5) != k) continue;
            const double ninv = -1.0 / (double)tab.f[f].m;
            const uint32_t below = (uint32_t)(std::lower_bound(sorted, sorted + coded, tab.f[f].T) - sorted);
            q.f[j].m = tab.f[f].m;
            memcpy(&q.f[j].M, &ninv, 8);
            q.f[j].floor_k = (fk & 0xFFu) | (below << 8) | (f << 16);
            q.f[j].T = sorted[j];
            if (cls) ++cls->n[k];
            ++j;
        }
    *nactive = coded;
    return q;
}

// ------------------------------------------------------------------------------------------
// the plan
// ------------------------------------------------------------------------------------------
// Which kernels serve a batch: the LDS-resident fast path needs the largest filter of the batch
// (plus per-wave staging) to fit one workgroup's 160 KiB of LDS; otherwise the generic kernels
// probe / set the filter in global memory.
constexpr size_t LDS_LIMIT = 160 * 1024;
// k_insert_positions: a pixel-index table larger than this is not worth gathering from (1440p, 118 MB: step 454 -> 425 us hashed;
// 2160p, 265 MB: insert 124 -> 97; re-measured with the 26-byte table of round 4: 1440p equal, 2160p 207 -> 192 Gpixel/s gathered,
// profiles/r04_bigtable.txt)
constexpr size_t HASH_TABLE_CACHE_BYTES = (size_t)96 << 20;
constexpr uint32_t MAX_INSERT_TILES = 7, MAX_QUERY_TILES = 3;     // measured crossovers, see plan_insert_tiles
// pixels x coded frames of a launch from which its one-shot data is moved with non-temporal accesses (rbf_lds_dma.h, cache-policy
// note): 1080p from 64 frames, 2160p from 16
constexpr uint64_t STREAM_MIN_PIXEL_FRAMES = 64ull * 1920 * 1080;

enum class QueryKind {
    Generic,       // k_query: probes in global memory
    LdsWhole,      // whole filter in LDS: k_query_u64 (FP64, probe image) when Plan::f64_mod, else k_query_lds (Barrett)
    LdsTiled,      // k_query_tiled: LDS tiles, Barrett
    LdsTiledF64,   // k_query_s64t: LDS tiles, FP64, probe image
};

struct Plan {
    bool fast_insert;            // LDS partial-filter insert (any filter size, tiled when needed)
    QueryKind query;
    bool double_buffer, small_m;
    bool insert_tab;             // insert through the hash table + FP64 reductions (same size condition, any LDS fit)
    bool insert_two_phase;       // ... as k_insert_positions + k_insert_records (filters of more than one LDS tile, counts known on the host)
    bool f64_mod;                // every coded frame has F64MOD_M_MIN <= m <= F64MOD_M_MAX: reductions through the FP64 pipe
    uint32_t fwords_max, S /* slices of a coded frame */, per_tile /* sum of slices */, insert_group /* coded frames per insert launch */;
    SliceTable slices;
    uint32_t insert_tile_words, insert_tiles, query_tile_words;
    size_t insert_lds_bytes, query_lds_bytes;
    uint64_t nseg; uint32_t words_per_seg;
    uint32_t image_stride_words;  // row pitch of the probe image (dwords, multiple of 4)
    // the query launch reads the probe image of the batch's filters, not the filters themselves
    bool reads_probe_image() const { return (query == QueryKind::LdsWhole || query == QueryKind::LdsTiledF64) && f64_mod; }
};

static inline uint32_t round_up4(uint32_t words) { return (words + 3u) & ~3u; }
static inline bool in_f64_range(uint32_t m) { return m >= F64MOD_M_MIN && m <= F64MOD_M_MAX; }
// bytes of the pixel-index hash table of n pixels (k_hash_table: 26 bytes per pixel inside an allocation of 32)
static inline size_t hash_table_bytes(uint64_t n) { return ((size_t)n + QL_SEG_PIXELS) * 32; }

// The LDS tile of a filter of `fwords` dwords: a multiple of four, at most `cap` dwords (itself a multiple of four), honouring the
// test knob.  `even`: a filter of several tiles is cut into tiles of equal size; otherwise into tiles of `cap` and a rest.
static uint32_t tile_words_for(uint32_t fwords, uint32_t cap, uint32_t knob, bool even)
{
    uint32_t tw = round_up4(fwords);
    if (tw > cap) {
        const uint32_t nt = (fwords + cap - 1) / cap;
        tw = even ? round_up4((fwords + nt - 1) / nt) : cap;
    }
    if (knob && knob < tw) tw = knob & ~3u;
    return tw < 4 ? 4 : tw;
}

struct BatchSizes {
    uint32_t mmax = 0, active = 0;       // largest filter, coded frames
    bool small_m = true;                 // every m in 2 .. 2^30
    bool all_f64 = true;                 // every coded frame in the FP64 range
};

static BatchSizes classify(const rbf_filter_params *params, uint32_t nframes)
{
    BatchSizes b;
    for (uint32_t f = 0; f < nframes; ++f) {
        const uint32_t m = params[f].m;
        if (m > b.mmax) b.mmax = m;
        if (m) ++b.active;
        if (m == 1 || m > (1u << 30)) b.small_m = false;
        if (m && !in_f64_range(m)) b.all_f64 = false;
    }
    return b;
}

// Insert: the whole partial filter in LDS next to the per-wave queues, else tiles of the largest size that fits.
// Tiling re-hashes (insert) / re-probes (query) every key once per tile, so its cost grows with the
// tile count while the global-memory kernels' does not.  Measured ps per (pixel, frame), 4K..16K frames:
// insert tiled 3.1 / 5.2 / 6.3 / 10.4 at 3 / 5 / 7 / 10 tiles vs 7.8 generic; query tiled 5.8 / 11.2 at
// 2 / 4 tiles vs 8.1-9.0 generic (round 1's large-frame runs: git history).  Past the crossover the generic kernels run
// (16K frames: 59 instead of 9 Gpixel/s).
static void plan_insert_tiles(Plan &p, const Knobs &k, const BatchSizes &b, bool have_ones)
{
    // the table-driven insert kernel has the larger per-wave queue; size the tiles for whichever may run
    const size_t queue_bytes = (size_t)IL_WAVES * (IT_WAVE_LDS_BYTES > IL_QUEUE * 4 ? IT_WAVE_LDS_BYTES : IL_QUEUE * 4);
    p.insert_tile_words = tile_words_for(p.fwords_max, (uint32_t)((LDS_LIMIT - queue_bytes) / 4) & ~3u, k.tile_words, false);
    p.insert_lds_bytes = (size_t)p.insert_tile_words * 4 + queue_bytes;
    p.insert_tiles = std::max(1u, (p.fwords_max + p.insert_tile_words - 1) / p.insert_tile_words);
    p.fast_insert = !k.force_generic && b.mmax > 0 && !(k.tile_words == 0 && p.insert_tiles > MAX_INSERT_TILES);
    p.insert_tab = p.fast_insert && b.all_f64 && !k.no_hash_table && !k.barrett_only;
    // Filters of several tiles, set-bit counts known (rbf_encode_gop): one walk of the masks into position records, then the tiles
    // are filled from the records -- no queues in that kernel, so a tile may take all of LDS.
    p.insert_two_phase = p.insert_tab && !k.no_two_phase && have_ones && p.insert_tiles > 1;
    if (p.insert_two_phase) {
        p.insert_tile_words = tile_words_for(p.fwords_max, (uint32_t)(LDS_LIMIT / 4) & ~3u, k.tile_words, true);
        p.insert_tiles = (p.fwords_max + p.insert_tile_words - 1) / p.insert_tile_words;
        p.insert_lds_bytes = (size_t)p.insert_tile_words * 4;
    }
}

static void plan_query(Plan &p, const Knobs &k, const BatchSizes &b, uint32_t nframes, uint64_t n)
{
    const size_t fbytes = (size_t)round_up4(p.fwords_max) * 4;
    const bool lds = !k.force_generic && b.mmax > 0;
    // k_query_u64 (FP64 reductions, probe image) is double-buffered only; its buffers end with the SAFE dwords
    // ... and it addresses its outputs with 32-bit offsets (pass bytes: frame * nseg * 64 + ...): a chunk of frames x pixels >= 2^35
    // goes to the tiled kernel, which keeps 64-bit row bases
    const bool u64_offsets_fit = (uint64_t)nframes * ((n + QL_SEG_PIXELS - 1) / QL_SEG_PIXELS) * (QL_SEG_PIXELS / 8) < (1ull << 32);
    // (filters that fit twice but leave no room for the frame records go to the tiled kernel: one buffer)
    p.f64_mod = b.all_f64 && !k.barrett_only && !k.single_buffer && u64_offsets_fit &&
                2 * (fbytes + 16) + u64_geo_bytes(nframes) <= LDS_LIMIT;
    const size_t qbytes = fbytes + (p.f64_mod ? 16 : 0);
    p.double_buffer = 2 * qbytes <= LDS_LIMIT && !k.single_buffer;
    p.query = QueryKind::Generic;
    if (lds && qbytes <= LDS_LIMIT && !k.tile_words) {
        p.query = QueryKind::LdsWhole;
        p.query_lds_bytes = (p.double_buffer ? 2 : 1) * qbytes;
    } else if (lds) {
        p.query = QueryKind::LdsTiled;
        p.query_tile_words = (uint32_t)(LDS_LIMIT / 4);
        if (k.tile_words && k.tile_words < p.query_tile_words) p.query_tile_words = k.tile_words & ~3u;
        if (p.query_tile_words < 4) p.query_tile_words = 4;
        p.query_lds_bytes = (size_t)std::min(p.query_tile_words, round_up4(p.fwords_max)) * 4;
        if (k.tile_words == 0 && (p.fwords_max + p.query_tile_words - 1) / p.query_tile_words > MAX_QUERY_TILES) p.query = QueryKind::Generic;
    }
    // FP64 geometries that do not fit LDS twice (or whose tile size a test caps): k_query_s64t, one buffer of maximal tiles
    if (lds && b.all_f64 && !k.barrett_only && !k.single_buffer && !p.reads_probe_image()) {
        // one buffer of tile_words + 4 dwords, k_query_s64t's geometry behind it
        const uint32_t cap = (uint32_t)((LDS_LIMIT - S64_GEO_BYTES) / 4 - 4) & ~3u;
        p.query = QueryKind::LdsTiledF64;
        p.query_tile_words = tile_words_for(p.fwords_max, cap, k.tile_words, true);
        p.query_lds_bytes = (size_t)(p.query_tile_words + 4) * 4;
        p.f64_mod = true;                                         // the probe image is needed
    }
    if (p.query != QueryKind::LdsWhole && p.query != QueryKind::LdsTiledF64) p.f64_mod = false;
    const uint32_t segpx = p.query == QueryKind::LdsWhole || p.query == QueryKind::LdsTiledF64 ? (uint32_t)QL_SEG_PIXELS
                         : p.query == QueryKind::LdsTiled ? (uint32_t)TQ_SEG_PIXELS : (uint32_t)SEG_PIXELS;
    p.nseg = (n + segpx - 1) / segpx;
    p.words_per_seg = segpx / 64;
}

// Slices per frame so that one launch has about one workgroup per CU (256 on MI355X).  With many frames or several
// tiles the quotient gets small (4K, 29 frames, 3 tiles: 2 slices -> 174 long workgroups), so the frames are
// inserted in groups of `insert_group` coded frames, each group one launch with >= INSERT_SLICES slices per frame
// (4K: 10 frames x 8 slices x 3 tiles = 240 workgroups).  Handing out uneven slices to use all 256 CUs was
// measured and buys nothing: a launch lasts as long as its largest slice.
static void plan_slices(Plan &p, const Knobs &k, uint32_t cus, uint32_t active, const rbf_filter_params *params, uint32_t nframes)
{
    constexpr uint32_t INSERT_SLICES = 8;
    const uint32_t units = std::max(1u, cus / p.insert_tiles);    // workgroups per tile layer
    uint32_t group = std::max(1u, units / INSERT_SLICES);         // coded frames per launch
    if (group > active) group = active ? active : 1;
    uint32_t base = std::min(std::max(1u, units / group), 32u);
    // Single-tile filters (every frame size up to 1080p): ONE insert launch for the whole batch -- up to 128 coded frames when several
    // GOPs ride in one block (rbf_encode_runs) -- of about one workgroup per CU: the largest power of two of slices per frame that fits.
    // An insert workgroup costs its filter tile twice over (zeroed, then written out as a partial the reduce kernel reads back), so fewer,
    // longer workgroups win: measured on 4 x 29 frames of 1080p (profiles/r05_sweep1.txt, r05_sweep2.txt) 8 slices in groups of 32 frames
    // (round 4) 155 us, 8 slices in one launch 135, 4 slices 117, 2 slices 115, 1 slice 212 (116 of 256 CUs), 3 slices 170 (a slice no
    // longer stays on one XCD); 2 x 29 frames: 4 slices 58, 2 slices 102; 29 frames: 8 slices 33, 4 slices 54, 16 slices 42.
    if (p.insert_tiles == 1 && !p.insert_two_phase && active) {
        group = active;
        base = 1;
        while (base * 2 * active <= units && base < 32) base *= 2;
        if (k.insert_slices) base = std::min(k.insert_slices, 32u);     // RBF_OPT_INSERT_SLICES (tuning)
    }
    p.insert_group = group;
    p.S = base;
    p.per_tile = 0;
    for (uint32_t f = 0; f < nframes; ++f) {
        const uint32_t sf = params[f].m ? base : 0u;
        p.slices.n[f] = (uint8_t)sf;
        p.per_tile += sf;
    }
}

// cus: compute units of the device; have_ones: the set-bit counts of the masks are known on the host (rbf_encode_gop)
static Plan make_plan(const Knobs &k, uint32_t cus, const rbf_filter_params *params, uint32_t nframes, uint64_t n, bool have_ones = false)
{
    Plan p{};
    const BatchSizes b = classify(params, nframes);
    p.small_m = b.small_m;
    p.fwords_max = (uint32_t)(((uint64_t)b.mmax + 31) / 32);
    p.image_stride_words = round_up4(p.fwords_max);
    plan_insert_tiles(p, k, b, have_ones);
    plan_query(p, k, b, nframes, n);
    plan_slices(p, k, cus, b.active, params, nframes);
    return p;
}

// A mixed batch -- coded frames inside AND outside the FP64 range -- as two batches over disjoint frame sets: `small` keeps the frames
// outside the range (Barrett kernels), `big` the ones inside (FP64 kernels); the others' m is 0.  false: the batch is not mixed.
static bool split_by_family(const rbf_filter_params *params, uint32_t nframes, rbf_filter_params *small, rbf_filter_params *big)
{
    uint32_t in_range = 0, out_of_range = 0;
    for (uint32_t f = 0; f < nframes; ++f) {
        small[f] = big[f] = params[f];
        if (!params[f].m) continue;
        ++(in_f64_range(params[f].m) ? in_range : out_of_range);
        (in_f64_range(params[f].m) ? small[f] : big[f]).m = 0;
    }
    return in_range && out_of_range;
}
