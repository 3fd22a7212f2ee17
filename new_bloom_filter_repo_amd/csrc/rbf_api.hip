// rbf_api.hip -- C ABI (include/rbf.h) over the gfx950 kernels: the mask stage, the encode / decode chunks and the entry points, in
// the order of the header.  One translation unit, split by #include:
//   rbf_plan.h       which kernels serve a batch, and the frame tables they read (pure host code over rbf_geometry.h)
//   rbf_mask_plan.h  the temporal chunks of the GOP mask kernels (pure host code; rbf_kernels_mask.h includes it)
//   rbf_host.h       errors, context and scratch memory, timing, the shared hash table, shared argument checks and launches
//   rbf_rice_host.h  host side of the sample codec
// and the kernels it launches, one header per stage (rbf_kernels.h: the generic path):
#include "rbf_host.h"
#include "rbf_kernels.h"
#include "rbf_kernels_noise.h"
#include "rbf_kernels_mask.h"
#include "rbf_kernels_hold.h"
#include "rbf_kernels_lookahead.h"
#include "rbf_kernels_barrett.h"
#include "rbf_kernels_insert_f64.h"
#include "rbf_kernels_reduce.h"
#include "rbf_kernels_query_f64.h"
#include "rbf_kernels_query_f64_tiled.h"
#include "rbf_kernels_witness.h"
#include "rbf_kernels_pack.h"
#include "rbf_kernels_digest.h"
#include "rbf_kernels_cut.h"
#include "rbf_kernels_error.h"
#include "rbf_kernels_sweep.h"
#include "rbf_kernels_pan.h"
#include "rbf_kernels_view.h"
#include "rbf_rice_host.h"
#include "rbf_kernels_keyquant.h"

#include <cmath>
#include <cstring>

// ------------------------------------------------------------------------------------------
// A1: the mask stage
// ------------------------------------------------------------------------------------------
struct MaskArgs {
    const void *frames; FrameLayout l; uint32_t nframes;
    int32_t thr_floor; const int32_t *thr_floors;     // ... or one threshold per pair (host array, nullable)
    void *masks; uint64_t mask_stride; uint64_t *ones;
    uint32_t channels;                                // 1: the luma mask; >= 2: the all-channel mask over that many samples
};

static int launch_finish_ones(rbf_ctx *ctx, uint64_t *ones_dev, uint32_t pairs, uint64_t *host_block, uint64_t token,
                              void *clear_a, size_t bytes_a, void *clear_b, size_t bytes_b)
{
    // regions that are not 16-byte shaped fall back to a memset (never the case for the library's own buffers)
    if (clear_a && (((uintptr_t)clear_a | bytes_a) & 15)) { HIP_TRY(hipMemsetAsync(clear_a, 0, bytes_a, ctx->stream)); clear_a = nullptr; bytes_a = 0; }
    if (clear_b && (((uintptr_t)clear_b | bytes_b) & 15)) { HIP_TRY(hipMemsetAsync(clear_b, 0, bytes_b, ctx->stream)); clear_b = nullptr; bytes_b = 0; }
    const uint64_t quads = bytes_a / 16 + bytes_b / 16;
    uint32_t blocks = (uint32_t)((quads + 256 * 4 - 1) / (256 * 4));       // ~4 stores per thread
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_finish_ones, dim3(blocks), dim3(256), 0, ctx->stream, ctx->ones_acc.p, ones_dev, pairs, host_block, token,
                       (uint4 *)clear_a, (uint64_t)(bytes_a / 16), (uint4 *)clear_b, (uint64_t)(bytes_b / 16));
    HIP_TRY(hipGetLastError());
    ctx->ones_acc_dirty = false;
    return RBF_OK;
}

// every argument check of the mask stage, with no side effect (rbf_encode_gop_begin runs it before it touches the stream)
static int check_mask_args(const MaskArgs &a)
{
    if (!a.frames || !a.masks || !a.ones) return fail(RBF_EINVAL, "null device pointer");
    LayoutRules rules;
    rules.min_frames = 2;
    if (int r = check_layout(a.l, a.nframes, rules)) return r;
    if (int r = check_frame_geometry((uint64_t)a.l.width * a.l.height, a.nframes - 1, a.mask_stride)) return r;
    if (a.thr_floors)
        for (uint32_t i = 0; i + 1 < a.nframes; ++i)
            if (a.thr_floors[i] < 0) return fail(RBF_EINVAL, "negative threshold %d for pair %u", a.thr_floors[i], i);
    if (a.channels == 0) return fail(RBF_EINVAL, "mask_channels must be 1 (luma) or the number of samples the all-channel mask compares");
    if (a.channels >= 2) {                                        // the all-channel mask is lossless only: threshold 0, no table
        if (a.thr_floor != 0 || a.thr_floors)
            return fail(RBF_EINVAL, "mask_channels %u: the all-channel mask takes no threshold (thr_floor %d, table %s)", a.channels, a.thr_floor,
                        a.thr_floors ? "given" : "none");
        if ((uint64_t)a.channels * a.l.sample_bytes > a.l.pixel_stride)
            return fail(RBF_EINVAL, "mask_channels %u x %u-byte samples exceed the pixel stride %u", a.channels, a.l.sample_bytes, a.l.pixel_stride);
    }
    return RBF_OK;
}

// The accumulator the mask kernels count into: zero whenever they start (k_finish_ones or the fused tail re-zeroes it).
static int prepare_ones_acc(rbf_ctx *ctx, uint32_t pairs)
{
    if (ctx->ones_acc.cap < (size_t)pairs * 8) {
        if (ctx->ones_acc.p) HIP_TRY(hipStreamSynchronize(ctx->stream));      // a kernel in flight may still count into the old one
        if (int r = ctx->ones_acc.alloc(((size_t)pairs + 64) * 8)) return r;
        ctx->ones_acc_dirty = true;
    }
    if (ctx->ones_acc_dirty) {                                    // a launch failed or was abandoned: counts AND tickets start from zero again
        HIP_TRY(hipMemsetAsync(ctx->ones_acc.p, 0, ctx->ones_acc.cap, ctx->stream));
        if (ctx->mask_ticket.p) HIP_TRY(hipMemsetAsync(ctx->mask_ticket.p, 0, (MASK_TICKETS + 1) * 4, ctx->stream));
    }
    ctx->ones_acc_dirty = true;                                   // until k_finish_ones has been enqueued
    return RBF_OK;
}

// (the temporal chunks of the fast mask kernel: plan_mask_chunks, rbf_mask_plan.h)

// Per-pair thresholds travel as kernel arguments (captured at launch, so the caller's array is free as soon as we return) into a
// device table.  A skipped pair gets INT32_MAX: `abs(diff) > thr` is then never true -- a zero row and a zero count.
static int store_thresholds(rbf_ctx *ctx, const MaskArgs &a, const uint8_t *skip)
{
    const uint32_t pairs = a.nframes - 1;
    if (int r = ctx->thr_tab.reserve((size_t)pairs * 4)) return r;
    for (uint32_t base = 0; base < pairs; base += ThrChunk::N) {
        ThrChunk c{};
        const uint32_t cnt = pairs - base < ThrChunk::N ? pairs - base : ThrChunk::N;
        for (uint32_t i = 0; i < cnt; ++i) c.v[i] = (skip && skip[base + i]) ? 0x7FFFFFFF : a.thr_floors ? a.thr_floors[base + i] : a.thr_floor;
        hipLaunchKernelGGL(k_store_thresholds, dim3(1), dim3(ThrChunk::N), 0, ctx->stream, c, ctx->thr_tab.p + base, cnt);
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// the fast mask kernel over the first fast_segs segments of 1024 pixels of every pair
static void launch_mask_gop(rbf_ctx *ctx, const MaskArgs &a, uint64_t fast_segs, uint32_t chunks, const MaskChunks &mc,
                            const int32_t *thr_tab_fast, const MaskFinish &fin)
{
    const uint32_t bx = (uint32_t)((fast_segs + WG_WAVES - 1) / WG_WAVES), pixel = a.l.pixel_stride;
    const size_t lds = (size_t)(a.nframes - 1) * 4;
    uint64_t *const acc = ctx->ones_acc.p;
    LaunchTimer t(ctx, RBF_K_MASK);
#define RBF_MASK_GOP(S, PB, Z) hipLaunchKernelGGL((k_residual_mask_gop<S, PB, true, Z>), dim3(bx, chunks), dim3(WG_THREADS), lds, ctx->stream,   \
                               (const uint8_t *)a.frames, a.l.frame_stride, a.nframes, fast_segs, a.thr_floor, thr_tab_fast,                    \
                               (uint16_t *)a.masks, a.mask_stride / 2, acc, mc, fin)
#define RBF_MASK_GOP2(S, PB) do { if (thr0) RBF_MASK_GOP(S, PB, true); else RBF_MASK_GOP(S, PB, false); } while (0)
#define RBF_MASK_ANY_GOP(S, PB) hipLaunchKernelGGL((k_residual_mask_any_gop<S, PB, true>), dim3(bx, chunks), dim3(WG_THREADS), lds, ctx->stream, \
                                (const uint8_t *)a.frames, a.l.frame_stride, a.nframes, fast_segs, thr_tab_fast, (uint16_t *)a.masks,           \
                                a.mask_stride / 2, acc, mc, fin)
    const bool thr0 = !thr_tab_fast && a.thr_floor == 0 && !ctx->knobs.force_generic_mask_bits;     // "luma changed": no per-pixel extraction
    if (a.channels >= 2) {
        if (pixel == 3) RBF_MASK_ANY_GOP(uint8_t, 3);
        else if (pixel == 4) RBF_MASK_ANY_GOP(uint8_t, 4);
        else if (pixel == 6) RBF_MASK_ANY_GOP(uint16_t, 6);
        else RBF_MASK_ANY_GOP(uint16_t, 8);
    }
    else if (a.l.sample_bytes == 1 && pixel == 1) RBF_MASK_GOP2(uint8_t, 1);
    else if (a.l.sample_bytes == 1) RBF_MASK_GOP2(uint8_t, 3);
    else if (pixel == 2) RBF_MASK_GOP2(uint16_t, 2);
    else RBF_MASK_GOP2(uint16_t, 6);
#undef RBF_MASK_ANY_GOP
#undef RBF_MASK_GOP2
#undef RBF_MASK_GOP
}

// the generic mask kernel over the mask words from first_word on (a ragged frame tail, or a layout the fast kernel does not take)
static void launch_mask_generic(rbf_ctx *ctx, const MaskArgs &a, uint64_t first_word, const int32_t *thr_tab)
{
    const uint64_t n = (uint64_t)a.l.width * a.l.height, rest = (n + 63) / 64 - first_word;
    uint64_t bx = (rest + WG_WAVES * 16 - 1) / (WG_WAVES * 16);      // ~16 words per wave
    if (bx < 1) bx = 1;
    if (bx > 65535) bx = 65535;
    const dim3 grid((uint32_t)bx, a.nframes - 1), block(WG_THREADS);
    LaunchTimer t(ctx, RBF_K_MASK);
    by_sample_width(a.l.sample_bytes, [&](auto s) {
        using S = decltype(s);
        if (a.channels >= 2)
            hipLaunchKernelGGL(k_residual_mask_any<S>, grid, block, 0, ctx->stream, (const uint8_t *)a.frames, a.l.frame_stride, a.l.width, n,
                               a.l.row_pitch, a.l.pixel_stride, a.channels, thr_tab, (uint64_t *)a.masks, a.mask_stride / 8, ctx->ones_acc.p, first_word);
        else
            hipLaunchKernelGGL(k_residual_mask<S>, grid, block, 0, ctx->stream, (const uint8_t *)a.frames, a.l.frame_stride, a.l.width, n,
                               a.l.row_pitch, a.l.pixel_stride, a.thr_floor, thr_tab, (uint64_t *)a.masks, a.mask_stride / 8, ctx->ones_acc.p, first_word);
    });
}

// The fused tail of the GOP mask kernel needs its ticket counters: allocated once, zero between launches.
static int prepare_mask_tickets(rbf_ctx *ctx)
{
    if (ctx->mask_ticket.p) return RBF_OK;
    if (int r = ctx->mask_ticket.alloc((MASK_TICKETS + 1) * 4)) return r;
    if (hipError_t e = hipMemsetAsync(ctx->mask_ticket.p, 0, (MASK_TICKETS + 1) * 4, ctx->stream)) {      // never keep tickets that were not zeroed
        ctx->mask_ticket.release();
        return fail(RBF_EIO, "hipMemsetAsync(mask tickets): %s", hipGetErrorString(e));
    }
    return RBF_OK;
}

// finish: hand the counts out through k_finish_ones.  gop_tail (rbf_encode_gop): publish + clears, fused into the mask kernel when it
// covers the frame.  skip (rbf_encode_runs): skip[p] != 0 = pair p is not coded (zero row, zero count).
static int residual_mask_impl(rbf_ctx *ctx, const MaskArgs &a, bool finish, const MaskFinish *gop_tail = nullptr, const uint8_t *skip = nullptr)
{
    if (int r = set_device(ctx)) return r;
    if (int r = check_mask_args(a)) return r;
    const FrameLayout &l = a.l;
    const bool any = a.channels >= 2;
    const uint64_t n = (uint64_t)l.width * l.height, nwords = (n + 63) / 64;
    const uint32_t pairs = a.nframes - 1;
    if (int r = prepare_ones_acc(ctx, pairs)) return r;
    // Fast path: flat frames, 16-byte aligned, whole 1024-pixel segments; the generic kernel does the rest.
    // (all-channel: 3 or 4 samples that fill the pixel; fewer samples than the pixel holds go to the generic kernel)
    const bool flat = l.row_pitch == (uint64_t)l.width * l.pixel_stride;
    const bool known = any ? (a.channels * l.sample_bytes == l.pixel_stride && (a.channels == 3 || a.channels == 4))
                           : (l.sample_bytes == 1 && (l.pixel_stride == 1 || l.pixel_stride == 3)) ||
                             (l.sample_bytes == 2 && (l.pixel_stride == 2 || l.pixel_stride == 6));
    const bool fast = !ctx->knobs.force_generic && flat && known && l.frame_stride % 16 == 0 && ((uintptr_t)a.frames % 16) == 0 &&
                      (size_t)pairs * 4 <= 48 * 1024;
    const uint64_t fast_segs = fast ? n / 1024 : 0, first_word = fast_segs * 16;
    MaskChunks mc{};
    bool skip_in_table = false;
    const uint32_t chunks = fast_segs ? plan_mask_chunks(ctx->knobs, a.nframes, fast_segs, skip, &mc, &skip_in_table) : 1;
    // A skipped pair that a kernel WITHOUT the chunk table sees (the generic kernel behind a ragged frame tail or an unaligned layout;
    // the fast kernel of a block with more runs than the table holds) is skipped through its threshold.
    const int32_t *thr_tab = nullptr, *thr_tab_fast = nullptr;
    if (a.thr_floors || (skip && (first_word < nwords || !skip_in_table))) {
        if (int r = store_thresholds(ctx, a, skip)) return r;
        thr_tab = ctx->thr_tab.p;
        if (a.thr_floors || (skip && !skip_in_table)) thr_tab_fast = ctx->thr_tab.p;
    }
    bool fused = false;
    if (fast_segs) {
        // the pass's tail (counts out, clears) rides in this launch when it is the only mask launch of the pass
        MaskFinish fin{};
        if (gop_tail && !ctx->knobs.no_fused_finish && first_word == nwords && !(((uintptr_t)gop_tail->clear_a | (uintptr_t)gop_tail->clear_b) & 15)) {
            if (int r = prepare_mask_tickets(ctx)) return r;
            fin = *gop_tail;
            fin.enabled = 1; fin.count = pairs; fin.ticket = ctx->mask_ticket.p; fin.ones_out = a.ones;
            fused = true;
        }
        launch_mask_gop(ctx, a, fast_segs, chunks, mc, thr_tab_fast, fin);
    }
    if (first_word < nwords) launch_mask_generic(ctx, a, first_word, thr_tab);
    HIP_TRY(hipGetLastError());
    if (fused) { ctx->ones_acc_dirty = false; return RBF_OK; }
    if (gop_tail) return launch_finish_ones(ctx, a.ones, pairs, gop_tail->host_block, gop_tail->token, gop_tail->clear_a, (size_t)gop_tail->quads_a * 16,
                                            gop_tail->clear_b, (size_t)gop_tail->quads_b * 16);
    if (finish) return launch_finish_ones(ctx, a.ones, pairs, nullptr, 0, nullptr, 0, nullptr, 0);
    return RBF_OK;
}

// ------------------------------------------------------------------------------------------
// A4 + A5 (encode), A6 (decode): one chunk of at most MAX_BATCH frames (the geometry table rides in the kernel arguments)
// ------------------------------------------------------------------------------------------
static int check_filter_strides(const rbf_filter_params *params, uint32_t nframes, uint64_t filter_stride_bytes)
{
    if (filter_stride_bytes % 8) return fail(RBF_EINVAL, "filter stride must be a multiple of 8");
    for (uint32_t f = 0; f < nframes; ++f) {
        const uint64_t need = (((uint64_t)params[f].m + 63) / 64) * 8;
        if (filter_stride_bytes < need)
            return fail(RBF_EINVAL, "frame %u: filter stride %llu < %llu", f, (unsigned long long)filter_stride_bytes, (unsigned long long)need);
    }
    return RBF_OK;
}

// what the query kernel writes: a pass word for every 64 positions and the pass count of every segment
static int reserve_query_outputs(rbf_ctx *ctx, const Plan &pl, uint32_t nframes)
{
    if (WG_THREADS % pl.words_per_seg) return fail(RBF_EINVAL, "segments of %u words do not tile a workgroup's chunk", pl.words_per_seg);
    if (int r = ctx->pass_words.reserve((size_t)nframes * pl.nseg * pl.words_per_seg * 8)) return r;
    return ctx->seg_cnt.reserve((size_t)nframes * pl.nseg * 4 + 16);     // + 16: the counts are read four to a load
}

// The scan in front of the compaction (encode) / expansion (decode): the start of every workgroup's range of witness bits, from the
// segment pass counts the query kernel left (k_chunk_offsets, one workgroup per frame).  Returns the workgroups per frame in *nchunks.
static int launch_chunk_offsets(rbf_ctx *ctx, const Plan &pl, uint32_t nframes, uint32_t *nchunks,
                                void *witnesses_dev = nullptr /* encode: zero the shared dwords */, uint64_t witness_stride_bytes = 0)
{
    const uint64_t bx = std::max<uint64_t>(1, (pl.nseg * pl.words_per_seg + WG_THREADS - 1) / WG_THREADS);      // one lane per 64-position word
    *nchunks = (uint32_t)bx;
    if (int r = ctx->chunk_off.reserve((size_t)nframes * bx * 4)) return r;
    LaunchTimer t(ctx, RBF_K_SCAN);
    hipLaunchKernelGGL(k_chunk_offsets, dim3(nframes), dim3(CO_THREADS), 0, ctx->stream, (const uint32_t *)ctx->seg_cnt.p, pl.nseg,
                       (uint32_t)WG_THREADS / pl.words_per_seg, *nchunks, ctx->chunk_off.p, (uint32_t *)witnesses_dev, witness_stride_bytes / 4);
    return RBF_OK;
}

struct QueryFlags {
    bool image_ready = false;        // the probe image of this batch has already been written (k_filter_reduce does it on the encode side)
    bool table_for_next = false;     // the next batch's insert gathers from the hash table: keep it cached
    bool quiet_passthrough = false;  // frames with m == 0 are another launch's: do not write their (empty) outputs
};

// A context that is the pixel-index hash table's only holder has k_query_u64 -- which hashes every index anyway -- write it again:
// 54 MB of identical values whose only purpose is to be in the Infinity Cache when the next batch's insert gathers from them (one
// pipeline: insert 47 -> 38 us, step 214 -> 209).  With several holders the table stays cached by being used.  (READING the hashes
// from the table instead of computing them was measured in round 4: 73.2 instead of 74.7 us alone with the 32-byte entries of
// that time, nothing in the step, 66 MB of extra traffic per launch -- not kept.)
static uint4 *table_to_rewrite(rbf_ctx *ctx, uint64_t n, const Seeds &sd)
{
    const SharedHashTable *sh = ctx->hash_shared;
    if (!sh || sh->n != n || !same_seeds(sh->seeds, sd) || ctx->knobs.no_hash_table || ctx->knobs.no_table_rewrite) return nullptr;
    std::lock_guard<std::mutex> lk(g_hash_mu);
    return sh->refs == 1 ? ctx->hash_tab : nullptr;
}

// query launch shared by encode and decode
static int launch_query(rbf_ctx *ctx, const Plan &pl, const BloomBatch &b, const FrameTable &tab, const QueryFlags &flags)
{
    const uint32_t nframes = b.nframes;
    const Seeds sd = to_dev(*b.seeds);
    const uint32_t *filters = (const uint32_t *)b.filters;
    uint64_t stride_words = b.filter_stride / 4;
    if (pl.reads_probe_image()) {
        if (int r = ctx->qimage.reserve((size_t)nframes * pl.image_stride_words * 4)) return r;
        if (!flags.image_ready) {
            const uint32_t bx = (pl.image_stride_words + WG_THREADS - 1) / WG_THREADS;
            hipLaunchKernelGGL(k_probe_image, dim3(bx, nframes), dim3(WG_THREADS), 0, ctx->stream, filters, stride_words, ctx->qimage.p,
                               (uint64_t)pl.image_stride_words);
        }
        filters = ctx->qimage.p;
        stride_words = pl.image_stride_words;
    }
    const uint32_t lds_waves = (uint32_t)((pl.nseg + QL_WAVES - 1) / QL_WAVES);      // grid of the LDS kernels: one wave per segment
    uint32_t nactive; uint64_t empty[2];
    LaunchTimer t(ctx, RBF_K_QUERY);
    if (pl.query == QueryKind::LdsTiledF64) {
        const FrameTable stab = query_table(tab, nframes, nullptr, &nactive, empty);
        if (flags.quiet_passthrough) empty[0] = empty[1] = 0;
        // 0: every coded frame has floor(k*) 1 or 2; 1: 0, 1 or 2; 2: anything (all frames walk their probes per tile)
        int mode = 0;
        for (uint32_t f = 0; f < nframes; ++f) {
            if (!tab.f[f].m) continue;
            if (tab.f[f].floor_k > 2) mode = 2;
            else if (tab.f[f].floor_k == 0 && mode < 1) mode = 1;
        }
        auto qkern = mode == 2 ? k_query_s64t<2> : mode == 1 ? k_query_s64t<1> : k_query_s64t<0>;
        if (int r = allow_big_lds((const void *)qkern)) return r;
        hipLaunchKernelGGL(qkern, dim3(lds_waves), dim3(QL_THREADS), s64t_lds_bytes(pl.query_tile_words), ctx->stream, b.n, nactive, stab, sd,
                           filters, stride_words, pl.query_tile_words, ctx->seg_cnt.p, pl.nseg, ctx->pass_words.p, empty[0], empty[1]);
    } else if (pl.reads_probe_image()) {
        uint4 *table_out = flags.table_for_next ? table_to_rewrite(ctx, b.n, sd) : nullptr;
        // k_query_u64: coded frames ordered by floor(k*), 32-byte frame records in LDS behind the two image buffers
        U64Classes cls;
        const FrameTable utab = query_table(tab, nframes, &cls, &nactive, empty);
        if (flags.quiet_passthrough) empty[0] = empty[1] = 0;
        // the 111-register kernel (two waves of a neighbour pipeline's mask / compaction kernels fit next to it on every SIMD) unless the
        // batch has floor(k*) = 4 or 5, which only the 118-register one passes in rows
        const bool wide = cls.n[3] + cls.n[4] > 0;                 // (always the wide one: measured, no better -- profiles/r04_feed_sweep2.txt)
        auto kern64 = wide ? k_query_u64w : k_query_u64;
        if (int r = allow_big_lds((const void *)kern64)) return r;
        hipLaunchKernelGGL(kern64, dim3(lds_waves), dim3(QL_THREADS), pl.query_lds_bytes + u64_geo_bytes(nactive), ctx->stream, b.n, nactive,
                           utab, cls, sd, filters, stride_words, pl.fwords_max, ctx->seg_cnt.p, pl.nseg, ctx->pass_words.p, table_out, empty[0],
                           empty[1]);
    } else if (pl.query == QueryKind::LdsWhole) {
        auto kern = pl.double_buffer ? (pl.small_m ? k_query_lds<true, true> : k_query_lds<true, false>)
                                     : (pl.small_m ? k_query_lds<false, true> : k_query_lds<false, false>);
        if (int r = allow_big_lds((const void *)kern)) return r;
        hipLaunchKernelGGL(kern, dim3(lds_waves), dim3(QL_THREADS), pl.query_lds_bytes, ctx->stream, b.n, nframes, tab, sd, filters, stride_words,
                           pl.fwords_max, ctx->seg_cnt.p, pl.nseg, ctx->pass_words.p);
    } else if (pl.query == QueryKind::LdsTiled) {
        auto kern = pl.small_m ? k_query_tiled<true> : k_query_tiled<false>;
        if (int r = allow_big_lds((const void *)kern)) return r;
        hipLaunchKernelGGL(kern, dim3(lds_waves), dim3(QL_THREADS), pl.query_lds_bytes, ctx->stream, b.n, nframes, tab, sd, filters, stride_words,
                           pl.query_tile_words, ctx->seg_cnt.p, pl.nseg, ctx->pass_words.p);
    } else {
        const uint64_t bx = (pl.nseg + WG_WAVES - 1) / WG_WAVES;
        hipLaunchKernelGGL(k_query, dim3((uint32_t)bx, nframes), dim3(WG_THREADS), 0, ctx->stream, b.n, tab, sd, filters, stride_words,
                           ctx->seg_cnt.p, pl.nseg, ctx->pass_words.p);
    }
    return RBF_OK;
}

// k_insert_positions, the first half of the two-kernel insert: one walk of the masks into position records
static int launch_insert_positions(rbf_ctx *ctx, const BloomBatch &b, const FrameTable &itab, const Seeds &sd, bool hashed_positions)
{
    HIP_TRY(hipMemsetAsync(ctx->ins_counters.p, 0, (size_t)b.nframes * 4, ctx->stream));
    const uint64_t groups = (((b.n + 7) >> 3) + IT_STEP_BYTES - 1) / IT_STEP_BYTES;
    uint64_t S1 = (uint64_t)ctx->cus * 4 / (b.nframes ? b.nframes : 1);           // ~4 workgroups of 4 waves per CU (2160p x 8: 96 us; 8 per CU: 115) ...
    if (S1 > groups / (IP_WAVES * 4)) S1 = groups / (IP_WAVES * 4);               // ... each wave with >= 4 steps
    S1 &= ~7ull;                                                                  // a slice stays on one XCD across frames
    if (S1 < 1) S1 = 1;
    if (int r = allow_big_lds((const void *)k_insert_records)) return r;
    LaunchTimer t(ctx, RBF_K_INSERT);
    auto pkern = hashed_positions ? k_insert_positions<true> : k_insert_positions<false>;
    hipLaunchKernelGGL(pkern, dim3((uint32_t)S1, b.nframes), dim3(IP_THREADS), 0, ctx->stream, (const uint8_t *)b.masks, b.mask_stride, b.n, itab,
                       hashed_positions ? nullptr : (const uint4 *)ctx->hash_tab, sd, ctx->ins_records.p, ctx->ins_counters.p);
    return RBF_OK;
}

// Whether the hash-table insert of this batch hashes its set positions itself (true) or gathers them from the shared table, which is
// then acquired -- built for this batch, or taken from whoever has it.
static bool settle_hash_table(rbf_ctx *ctx, const Plan &pl, const BloomBatch &b, const Seeds &sd)
{
    // A pixel-index table (an allocation of 32 B per pixel, process-wide, lives until the last context of its geometry goes) that would
    // crowd the 256 MB Infinity Cache is never built: the insert kernels hash their set positions on the spot instead (2160p, 265 MB:
    // 72 us against 96 with the gather) -- whichever insert kernel runs, with or without the masks' set-bit counts.
    const bool table_too_big = hash_table_bytes(b.n) > HASH_TABLE_CACHE_BYTES;
    if (table_too_big || (pl.insert_two_phase && ctx->knobs.hash_positions)) {
        // this context moved to a geometry that hashes: it no longer pins the old geometry's table
        if (ctx->hash_shared && (ctx->hash_shared->n != b.n || !same_seeds(ctx->hash_shared->seeds, *b.seeds))) hash_table_release(ctx);
        return true;
    }
    bool built = false;
    if (!hash_table_acquire(ctx, b.n, *b.seeds, &built)) return true;         // no device memory for the table: hash instead
    if (ctx->knobs.hash_rebuild && !built) launch_hash_table(ctx, b.n, sd, ctx->hash_tab);     // diagnostic: rewritten (same values) for every batch
    return false;
}

// LDS insert: partial filters per mask slice (k_insert_lds / k_insert_tab / k_insert_positions + k_insert_records), then k_filter_reduce
static int insert_fast(rbf_ctx *ctx, const Plan &pl, const BloomBatch &b, const FrameTable &tab, const uint64_t *ones_host, bool stream_once,
                       uint32_t *image)
{
    const uint32_t nframes = b.nframes;
    const Seeds sd = to_dev(*b.seeds);
    const uint64_t part_stride = round_up4(pl.fwords_max);          // 16-byte rows for the reduce kernel
    if (int r = ctx->partials.reserve((size_t)nframes * pl.S * part_stride * 4)) return r;
    const bool use_tab = pl.insert_tab;
    const bool hashed_positions = use_tab && settle_hash_table(ctx, pl, b, sd);
    const uint4 *hash_tab = hashed_positions ? nullptr : ctx->hash_tab;
    FrameTable itab = tab;                                         // k_insert_tab reads -1/m from the M field
    if (use_tab)
        for (uint32_t f = 0; f < nframes; ++f)
            if (itab.f[f].m) { const double ninv = -1.0 / (double)itab.f[f].m; memcpy(&itab.f[f].M, &ninv, 8); }
    auto ikern = pl.small_m ? k_insert_lds<true> : k_insert_lds<false>;
    if (int r = allow_big_lds((const void *)ikern)) return r;
    // one tile = the whole filter: the kernel without the in-tile test per probe
    const bool whole = pl.insert_tiles == 1;
    auto tkern = hashed_positions ? (whole ? k_insert_tab<true, true> : k_insert_tab<true, false>)
                                  : (whole ? k_insert_tab<false, true> : k_insert_tab<false, false>);
    if (int r = allow_big_lds((const void *)tkern)) return r;
    const bool two_phase = pl.insert_two_phase && use_tab;        // (its record memory was reserved by the caller)
    FrameTable rtab = tab;
    if (two_phase) {
        // itab.floor_k / rtab.T carry the index of the frame's first record (the kernels' own use of those fields: none)
        uint64_t first = 0;
        for (uint32_t f = 0; f < nframes; ++f) {
            itab.f[f].floor_k = (uint32_t)first;
            rtab.f[f].T = first;
            if (b.params[f].m) first += ones_host[f];
        }
        if (int r = launch_insert_positions(ctx, b, itab, sd, hashed_positions)) return r;
    }
    for (uint32_t f0 = 0; f0 < nframes;) {                        // groups of pl.insert_group coded frames
        SliceTable grp{};
        uint32_t per_tile = 0, coded = 0, f = f0;
        for (; f < nframes && coded < pl.insert_group; ++f) {
            grp.n[f] = pl.slices.n[f];
            per_tile += grp.n[f];
            coded += grp.n[f] ? 1u : 0u;
        }
        f0 = f;
        if (!per_tile) continue;
        const dim3 grid(per_tile * pl.insert_tiles), block(IL_THREADS);
        LaunchTimer t(ctx, RBF_K_INSERT);
        if (two_phase)
            hipLaunchKernelGGL(k_insert_records, grid, block, pl.insert_lds_bytes, ctx->stream, (const uint2 *)ctx->ins_records.p,
                               (const uint32_t *)ctx->ins_counters.p, rtab, ctx->partials.p, part_stride, pl.insert_tile_words, grp, per_tile, pl.S);
        else if (use_tab)
            hipLaunchKernelGGL(tkern, grid, block, pl.insert_lds_bytes, ctx->stream, (const uint8_t *)b.masks, b.mask_stride, b.n, itab, hash_tab, sd,
                               ctx->partials.p, part_stride, pl.insert_tile_words, grp, per_tile, pl.S);
        else
            hipLaunchKernelGGL(ikern, grid, block, pl.insert_lds_bytes, ctx->stream, (const uint8_t *)b.masks, b.mask_stride, b.n, tab, sd,
                               ctx->partials.p, part_stride, pl.insert_tile_words, grp, per_tile, pl.S);
    }
    LaunchTimer t(ctx, RBF_K_REDUCE);
    const uint64_t words = b.filter_stride / 4;
    const uint32_t vec_ok = (words % 4 == 0 && ((uintptr_t)b.filters % 16) == 0) ? 1u : 0u;
    const uint32_t bx = std::max(1u, (uint32_t)((words + WG_THREADS * 4 - 1) / (WG_THREADS * 4)));
    hipLaunchKernelGGL(stream_once ? k_filter_reduce<true> : k_filter_reduce<false>, dim3(bx, nframes), dim3(WG_THREADS), 0, ctx->stream,
                       (const uint32_t *)ctx->partials.p, part_stride, pl.S, pl.slices, tab, (uint32_t *)b.filters, words, b.stats, vec_ok, image,
                       (uint64_t)pl.image_stride_words);
    return RBF_OK;
}

// global-memory insert (k_insert), then k_filter_reduce with S = 1 in place: it only counts the set bits
static int insert_generic(rbf_ctx *ctx, const Plan &pl, const BloomBatch &b, const FrameTable &tab, uint32_t *image)
{
    HIP_TRY(hipMemsetAsync(b.filters, 0, (size_t)b.nframes * b.filter_stride, ctx->stream));
    const uint64_t words = b.filter_stride / 4;
    const uint64_t bx = std::min<uint64_t>(((b.n + 31) / 32 + WG_THREADS - 1) / WG_THREADS, 65535);
    {
        LaunchTimer t(ctx, RBF_K_INSERT);
        hipLaunchKernelGGL(k_insert, dim3((uint32_t)bx, b.nframes), dim3(WG_THREADS), 0, ctx->stream, (const uint32_t *)b.masks, b.mask_stride / 4,
                           b.n, tab, to_dev(*b.seeds), (uint32_t *)b.filters, words);
    }
    LaunchTimer t(ctx, RBF_K_REDUCE);
    SliceTable ones;
    memset(ones.n, 1, sizeof ones.n);
    const uint32_t bx2 = std::max(1u, (uint32_t)((words + WG_THREADS * 4 - 1) / (WG_THREADS * 4)));
    hipLaunchKernelGGL(k_filter_reduce<false>, dim3(bx2, b.nframes), dim3(WG_THREADS), 0, ctx->stream, (const uint32_t *)b.filters, words, 1u, ones,
                       tab, (uint32_t *)b.filters, words, b.stats, 0u, image, (uint64_t)pl.image_stride_words);
    return RBF_OK;
}

// `quiet_passthrough` / `compact`: see encode_chunk (a batch split over the two kernel families runs this twice)
// ones_host: nullable, the set bits of every mask
static int encode_chunk_pass(rbf_ctx *ctx, const BloomBatch &b, bool outputs_zeroed, const uint64_t *ones_host, bool quiet_passthrough, bool compact)
{
    const uint32_t nframes = b.nframes;
    uint64_t nrecords = 0;
    uint32_t coded = 0;
    for (uint32_t f = 0; f < nframes; ++f) {
        if (!b.params[f].m) continue;
        ++coded;
        if (ones_host) nrecords += ones_host[f];
    }
    Plan pl = make_plan(ctx->knobs, ctx->cus, b.params, nframes, b.n, ones_host && nrecords < (1ull << 32));
    // The two-kernel insert needs 8 bytes per set mask bit.  Without that memory the batch is re-planned as if the counts
    // were unknown (queue-sized tiles, k_insert_tab / k_insert_lds): slower, not an error.
    if (pl.insert_two_phase &&
        (ctx->ins_records.reserve((size_t)(nrecords ? nrecords : 1) * 8) || ctx->ins_counters.reserve((size_t)MAX_BATCH * 4))) {
        (void)hipGetLastError();
        pl = make_plan(ctx->knobs, ctx->cus, b.params, nframes, b.n, false);
    }
    FrameTable tab;
    if (int r = fill_table(b.params, nframes, &tab)) return r;
    // a block of several GOPs (or of large frames): its one-shot data must not evict the hash table and the probe images
    const bool stream_once = (uint64_t)coded * b.n >= STREAM_MIN_PIXEL_FRAMES;
    if (int r = reserve_query_outputs(ctx, pl, nframes)) return r;
    if (int r = ctx->seg_off.reserve((size_t)nframes * pl.nseg * 8)) return r;
    const bool want_image = pl.reads_probe_image();               // the reduce kernel also writes the FP64 query kernel's probe image
    if (want_image) if (int r = ctx->qimage.reserve((size_t)nframes * pl.image_stride_words * 4)) return r;
    uint32_t *image = want_image ? ctx->qimage.p : nullptr;
    if (!outputs_zeroed)                                           // (the witness rows need no clearing: k_chunk_offsets zeroes what the compaction shares)
        HIP_TRY(hipMemsetAsync(b.stats, 0, (size_t)nframes * RBF_STATS_PER_FRAME * 8, ctx->stream));
    if (int r = pl.fast_insert ? insert_fast(ctx, pl, b, tab, ones_host, stream_once, image) : insert_generic(ctx, pl, b, tab, image)) return r;
    // ---- query: pass word of every 64 positions + per-segment pass counts
    if (int r = launch_query(ctx, pl, b, tab, QueryFlags{want_image, pl.insert_tab, quiet_passthrough})) return r;
    // ---- witness: pext(mask, pass) of every word lands at its bit offset (scan fused in)
    if (compact) {
        uint32_t bx;
        if (int r = launch_chunk_offsets(ctx, pl, nframes, &bx, b.witnesses, b.witness_stride)) return r;
        LaunchTimer t(ctx, RBF_K_STITCH);
        hipLaunchKernelGGL(stream_once ? k_compact_witness<true> : k_compact_witness<false>, dim3(bx, nframes), dim3(WG_THREADS), 0, ctx->stream,
                           ctx->pass_words.p, ctx->seg_cnt.p, pl.nseg, pl.words_per_seg, (const uint64_t *)b.masks, b.mask_stride / 8, b.n,
                           (uint32_t *)b.witnesses, b.witness_stride / 4, b.stats, ctx->chunk_off.p);
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// One chunk of at most MAX_BATCH frames.  The FP64 kernels (hash-table insert, k_query_u64 / k_query_s64t) need EVERY coded filter of
// their launch inside F64MOD_M_MIN <= m <= F64MOD_M_MAX; a single nearly static frame (1080p: < ~0.2 % changed pixels) used to
// send its whole batch to the round-1 Barrett kernels.  A mixed batch is now coded in two passes over disjoint frame sets --
// first the out-of-range frames (Barrett kernels; they also write the empty outputs of every frame that is not theirs), then
// the in-range ones (FP64 kernels, told to leave the others' outputs alone) -- followed by one compaction over all frames.
// Only when both passes cut the frame into the same segments (pass bytes and segment counts are shared with the compaction).
static int encode_chunk(rbf_ctx *ctx, const BloomBatch &b, bool outputs_zeroed, const uint64_t *ones_host)
{
    rbf_filter_params small[MAX_BATCH], big[MAX_BATCH];
    if (ctx->knobs.fp64_kernels() && !ctx->knobs.no_hash_table && split_by_family(b.params, b.nframes, small, big)) {
        const Plan ps = make_plan(ctx->knobs, ctx->cus, small, b.nframes, b.n, false);
        const Plan pb = make_plan(ctx->knobs, ctx->cus, big, b.nframes, b.n, ones_host != nullptr);
        if (pb.reads_probe_image() && pb.insert_tab && ps.nseg == pb.nseg && ps.words_per_seg == pb.words_per_seg) {
            if (int r = encode_chunk_pass(ctx, b.with(small), outputs_zeroed, nullptr, false, false)) return r;
            return encode_chunk_pass(ctx, b.with(big), true, ones_host, true, true);
        }
    }
    return encode_chunk_pass(ctx, b, outputs_zeroed, ones_host, false, true);
}

static int encode_batch_impl(rbf_ctx *ctx, const BloomBatch &b, bool outputs_zeroed, const uint64_t *ones_host = nullptr)
{
    if (int r = set_device(ctx)) return r;
    if (!b.masks || !b.params || !b.seeds || !b.filters || !b.witnesses || !b.stats) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_frame_geometry(b.n, b.nframes, b.mask_stride)) return r;
    if (int r = check_filter_strides(b.params, b.nframes, b.filter_stride)) return r;
    if (int r = check_witness_stride(b.n, b.witness_stride)) return r;
    if (int r = check_base8(b.masks, "masks_dev")) return r;
    if (int r = check_base8(b.filters, "filters_dev")) return r;
    if (int r = check_base8(b.witnesses, "witnesses_dev")) return r;
    if (int r = check_base8(b.stats, "stats_dev")) return r;
    for (uint32_t f0 = 0; f0 < b.nframes; f0 += MAX_BATCH) {
        const uint32_t cnt = std::min(b.nframes - f0, (uint32_t)MAX_BATCH);
        if (int r = encode_chunk(ctx, b.rows(f0, cnt), outputs_zeroed, ones_host ? ones_host + f0 : nullptr)) return r;
    }
    return RBF_OK;
}

static int decode_chunk(rbf_ctx *ctx, const BloomBatch &b)
{
    const uint32_t nframes = b.nframes;
    const Plan pl = make_plan(ctx->knobs, ctx->cus, b.params, nframes, b.n);
    FrameTable tab;
    if (int r = fill_table(b.params, nframes, &tab)) return r;
    if (int r = reserve_query_outputs(ctx, pl, nframes)) return r;
    // mixed batch (see encode_chunk): the query runs twice over disjoint frame sets, the expansion once
    bool split = false;
    rbf_filter_params small[MAX_BATCH], big[MAX_BATCH];
    if (ctx->knobs.fp64_kernels() && split_by_family(b.params, nframes, small, big)) {
        const Plan ps = make_plan(ctx->knobs, ctx->cus, small, nframes, b.n), pb = make_plan(ctx->knobs, ctx->cus, big, nframes, b.n);
        if (pb.reads_probe_image() && ps.nseg == pl.nseg && pb.nseg == pl.nseg && ps.words_per_seg == pl.words_per_seg &&
            pb.words_per_seg == pl.words_per_seg) {
            FrameTable ts, tb;
            if (int r = fill_table(small, nframes, &ts)) return r;
            if (int r = fill_table(big, nframes, &tb)) return r;
            if (int r = launch_query(ctx, ps, b, ts, QueryFlags{})) return r;
            if (int r = launch_query(ctx, pb, b, tb, QueryFlags{false, false, /* quiet_passthrough */ true})) return r;
            split = true;
        }
    }
    if (!split) if (int r = launch_query(ctx, pl, b, tab, QueryFlags{})) return r;
    // one lane per 64-position word; the kernel sums the earlier segment counts itself (until round 4: k_scan_segments + k_expand_mask_p)
    uint32_t bx;
    if (int r = launch_chunk_offsets(ctx, pl, nframes, &bx)) return r;
    LaunchTimer t(ctx, RBF_K_EXPAND);
    hipLaunchKernelGGL(k_expand_mask, dim3(bx, nframes), dim3(WG_THREADS), 0, ctx->stream, ctx->pass_words.p, ctx->seg_cnt.p, pl.nseg,
                       pl.words_per_seg, (const uint32_t *)b.witnesses, b.witness_stride / 4, (uint64_t *)b.masks, b.mask_stride / 8, b.n,
                       ctx->chunk_off.p);
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ------------------------------------------------------------------------------------------
// helpers of single entry points
// ------------------------------------------------------------------------------------------
static LayoutRules frame_pass_rules(uint32_t samples)         // rbf_noise_moments_batch, rbf_bgr_to_gray_batch, rbf_extract_luma_batch
{
    LayoutRules r;
    r.samples = samples; r.min_frames = 1; r.max_frames = 65535;
    return r;
}

// rbf_bgr_to_gray_batch / rbf_extract_luma_batch: one output sample per pixel from frames whose pixels hold >= `samples` samples;
// kernel_of(sample type) names the kernel; timed_as: the RBF_K_* id, < 0 = not timed.
template <class KernelOf>
static int pixel_pass(rbf_ctx *ctx, const void *frames_dev, const FrameLayout &l, uint32_t nframes, uint32_t samples, void *out_dev, int timed_as,
                      KernelOf &&kernel_of)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !out_dev) return fail(RBF_EINVAL, "null device pointer");
    if (int r = check_layout(l, nframes, frame_pass_rules(samples))) return r;
    const uint64_t n = (uint64_t)l.width * l.height;
    const uint32_t bx = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 256 * 4 - 1) / (256 * 4), 1), 8192);      // ~4 pixels per thread
    LaunchTimer t(ctx, timed_as);
    by_sample_width(l.sample_bytes, [&](auto s) {
        hipLaunchKernelGGL(kernel_of(s), dim3(bx, nframes), dim3(256), 0, ctx->stream, (const uint8_t *)frames_dev, l.frame_stride, l.width, n,
                           l.row_pitch, l.pixel_stride, (decltype(s) *)out_dev);
    });
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// The per-index entry points (rbf_filter_{insert,query}_{indices,keys}): one filter, `count` indices or keys; have_arrays: none of the
// device arrays the call reads or writes is null (asked only when there is something to do).  standard_k: 0 for the index calls.
template <class Launch>
static int index_call(rbf_ctx *ctx, const void *filter_dev, const rbf_filter_params *p, const rbf_seeds *seeds, uint32_t standard_k,
                      uint64_t count, bool have_arrays, Launch &&launch)
{
    if (int r = set_device(ctx)) return r;
    if (!filter_dev || !seeds) return fail(RBF_EINVAL, "null pointer");
    if (!p) return fail(RBF_EINVAL, "params is null");
    if (p->m == 0) return fail(RBF_EINVAL, "filter length m must be >= 1");
    if (p->floor_k > 64) return fail(RBF_ERANGE, "floor_k %u > 64", p->floor_k);
    if (standard_k > 64) return fail(RBF_ERANGE, "standard_k %u > 64", standard_k);
    if (count == 0) return RBF_OK;
    if (!have_arrays) return fail(RBF_EINVAL, "null device array");
    {
        LaunchTimer t(ctx, RBF_K_INDEX);
        launch(frame_dev(*p), to_dev(*seeds), dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>((count + WG_THREADS - 1) / WG_THREADS, 1), 8192)));
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

static int values_common(rbf_ctx *ctx, void *frame_dev, uint32_t width, uint32_t height,
                         uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes, uint32_t sample_bytes,
                         uint32_t channels, const void *mask_dev, void *values_dev, uint64_t *count_dev, bool scatter)
{
    if (int r = set_device(ctx)) return r;
    if (!frame_dev || !mask_dev || !values_dev) return fail(RBF_EINVAL, "null device pointer");
    LayoutRules rules;
    rules.samples = channels; rules.channels = true; rules.aligned = false;      // (this entry point has never asked for sample alignment)
    if (int r = check_layout(FrameLayout{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, 0}, 1, rules)) return r;
    const uint64_t n = (uint64_t)width * height;
    if (n > 0xFFFFFFFFull) return fail(RBF_ERANGE, "frame too large");
    const uint64_t nseg = (n + SEG_PIXELS - 1) / SEG_PIXELS;
    const dim3 grid((uint32_t)((nseg + WG_WAVES - 1) / WG_WAVES)), block(WG_THREADS);
    LaunchTimer t(ctx, scatter ? RBF_K_SCATTER : RBF_K_GATHER);
    if (int r = count_and_scan_masks(ctx, mask_dev, 0, n, 1, count_dev)) return r;
    by_sample_width(sample_bytes, [&](auto s) {
        using S = decltype(s);
        auto kern = scatter ? k_values<S, true> : k_values<S, false>;
        hipLaunchKernelGGL(kern, grid, block, 0, ctx->stream, (uint8_t *)frame_dev, width, n, row_pitch_bytes, pixel_stride_bytes, channels,
                           (const uint64_t *)mask_dev, ctx->seg_off.p, nseg, (S *)values_dev);
    });
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ------------------------------------------------------------------------------------------
// the entry points, in the order of include/rbf.h
// ------------------------------------------------------------------------------------------
extern "C" {

int rbf_version(void) { return RBF_ABI_VERSION; }
const char *rbf_last_error(void) { return g_err; }

int rbf_device_count(int *count)
{
    if (!count) return fail(RBF_EINVAL, "count is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(RBF_EIO, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = c;
    return RBF_OK;
}

int rbf_ctx_create(int device, void *hip_stream, rbf_ctx **out)
{
    if (!out) return fail(RBF_EINVAL, "out is null");
    *out = nullptr;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(RBF_EINVAL, "device %d out of range (have %d)", device, count);
    HIP_TRY(hipSetDevice(device));
    rbf_ctx *c = new (std::nothrow) rbf_ctx();
    if (!c) return fail(RBF_ENOMEM, "out of host memory");
    c->device = device;
    int cus = 0;                                                   // workgroup counts are sized for THIS device
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = (uint32_t)cus;
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->owns_stream = false; }
    else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(RBF_EIO, "hipStreamCreate: %s", hipGetErrorString(e)); }
        c->owns_stream = true;
    }
    *out = c;
    return RBF_OK;
}

int rbf_ctx_destroy(rbf_ctx *ctx)
{
    if (!ctx) return RBF_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &t : ctx->pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto e : ctx->pool) (void)hipEventDestroy(e);
    hash_table_release(ctx);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;                                                    // frees the scratch buffers and the pinned block
    return RBF_OK;
}

int rbf_ctx_sync(rbf_ctx *ctx)
{
    if (int r = set_device(ctx)) return r;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RBF_OK;
}

int rbf_malloc(rbf_ctx *ctx, size_t bytes, void **out_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!out_dev) return fail(RBF_EINVAL, "out_dev is null");
    *out_dev = nullptr;
    if (bytes == 0) bytes = 8;
    hipError_t e = hipMalloc(out_dev, bytes);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RBF_ENOMEM : RBF_EIO, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return RBF_OK;
}

int rbf_free(rbf_ctx *ctx, void *ptr_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!ptr_dev) return RBF_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(ptr_dev));
    return RBF_OK;
}

int rbf_memset(rbf_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    if (int r = set_device(ctx)) return r;
    if (bytes == 0) return RBF_OK;
    if (!dst_dev) return fail(RBF_EINVAL, "dst_dev is null");
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    return RBF_OK;
}

int rbf_memcpy_h2d(rbf_ctx *ctx, void *dst_dev, const void *src, size_t bytes)
{
    if (int r = set_device(ctx)) return r;
    if (bytes == 0) return RBF_OK;
    if (!dst_dev || !src) return fail(RBF_EINVAL, "null pointer");
    HIP_TRY(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RBF_OK;
}

int rbf_memcpy_d2h(rbf_ctx *ctx, void *dst, const void *src_dev, size_t bytes)
{
    if (int r = set_device(ctx)) return r;
    if (bytes == 0) return RBF_OK;
    if (!dst || !src_dev) return fail(RBF_EINVAL, "null pointer");
    HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RBF_OK;
}

int rbf_memcpy_d2d(rbf_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes)
{
    if (int r = set_device(ctx)) return r;
    if (bytes == 0) return RBF_OK;
    if (!dst_dev || !src_dev) return fail(RBF_EINVAL, "null pointer");
    HIP_TRY(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return RBF_OK;
}

int rbf_timing_enable(rbf_ctx *ctx, int on)
{
    if (int r = set_device(ctx)) return r;
    if (!on) { if (int r = drain_timing(ctx)) return r; }
    ctx->timing = on == 1 ? 0xFFFFFFFFu : (uint32_t)on;
    return RBF_OK;
}

int rbf_ctx_force_generic(rbf_ctx *ctx, int on)
{
    if (!ctx) return fail(RBF_EINVAL, "null context");
    ctx->knobs.set_flags(on);
    return RBF_OK;
}

int rbf_ctx_option(rbf_ctx *ctx, int option, int64_t value)
{
    if (!ctx) return fail(RBF_EINVAL, "null context");
    switch (option) {
    case RBF_OPT_SEPARATE_FINISH: ctx->knobs.no_fused_finish = value != 0; return RBF_OK;
    case RBF_OPT_INSERT_SLICES: ctx->knobs.insert_slices = value < 0 ? 0u : (uint32_t)value; return RBF_OK;
    default: return fail(RBF_EINVAL, "unknown option %d", option);
    }
}

int rbf_timing_reset(rbf_ctx *ctx)
{
    if (int r = set_device(ctx)) return r;
    if (int r = drain_timing(ctx)) return r;
    for (int k = 0; k < RBF_K_COUNT; ++k) { ctx->total_ms[k] = 0; ctx->launches[k] = 0; }
    return RBF_OK;
}

int rbf_timing_read(rbf_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches)
{
    if (int r = set_device(ctx)) return r;
    if (kernel_id < 0 || kernel_id >= RBF_K_COUNT) return fail(RBF_EINVAL, "kernel id %d", kernel_id);
    if (int r = drain_timing(ctx)) return r;
    if (total_ms) *total_ms = ctx->total_ms[kernel_id];
    if (launches) *launches = ctx->launches[kernel_id];
    return RBF_OK;
}

// ---- host math
int rbf_optimal_params(uint64_t n, uint64_t ones, double *k_out, uint64_t *l_out)
{
    if (!k_out || !l_out) return fail(RBF_EINVAL, "null output");
    *k_out = 0.0; *l_out = 0;
    if (n == 0 || ones > n) return fail(RBF_EINVAL, "need 0 <= ones <= n, n > 0");
    // np.sum(uint8) / n : both operands become float64 (improved_video_compressor.py:211-212)
    const double p = (double)ones / (double)n;
    if (p <= 0.0001) return RBF_OK;                         // :174
    if (p >= 0.32453) return RBF_OK;                        // :177 (P_STAR)
    const double q = 1 - p;
    const double L = std::log(2.0);
    const double k = std::log2(q * std::pow(L, 2.0) / p);   // :185  (float ** int -> pow)
    if (std::isnan(k) || k <= 0) return RBF_OK;             // :188
    const double gamma = 1 / L;
    const double lf = p * (double)n * k * gamma;            // :193, left-to-right products
    const uint64_t l = (uint64_t)lf;                        // int(): truncation (lf > 0)
    *k_out = k > 0.1 ? k : 0.1;                             // max(0.1, k)
    *l_out = l > 1 ? l : 1;                                 // max(1, l)
    return RBF_OK;
}

int rbf_activation_threshold(double k_star, uint32_t *floor_k, uint64_t *threshold)
{
    if (!floor_k || !threshold) return fail(RBF_EINVAL, "null output");
    if (!(k_star >= 0.0) || k_star > 64.0) return fail(RBF_ERANGE, "k* = %g outside [0, 64]", k_star);
    const double fl = std::floor(k_star);
    *floor_k = (uint32_t)fl;
    const double pa = k_star - fl;                          // p_activation, :58
    if (!(pa > 0.0)) { *threshold = 0; return RBF_OK; }     // `x < 0.0` is never true
    // RN(h / (2^64-1)) >= pa  <=>  h / (2^64-1) > mid, mid = midpoint of pa and its predecessor
    // (no tie is possible: mid is dyadic with an odd numerator, 2^64-1 is odd).
    int ex;
    const double fr = std::frexp(pa, &ex);                  // pa = fr * 2^ex, fr in [0.5, 1)
    const uint64_t A = (uint64_t)std::ldexp(fr, 53);        // 2^52 <= A < 2^53
    const int s = ex - 53 - 2;                              // pa = 4A * 2^s
    const uint64_t N = (A == (1ull << 52)) ? 4 * A - 1 : 4 * A - 2;   // mid = N * 2^s
    const int sh = -s;                                      // pa < 1 -> sh >= 55
    if (sh >= 128) { *threshold = 1; return RBF_OK; }
    const unsigned __int128 X = (unsigned __int128)N * (unsigned __int128)0xFFFFFFFFFFFFFFFFull;
    *threshold = (uint64_t)(X >> sh) + 1;                   // floor(mid * (2^64-1)) + 1
    return RBF_OK;
}

int rbf_plan_batch(uint64_t n, const uint64_t *ones, uint32_t nframes, int guard_l_ge_n,
                   rbf_filter_params *params, double *k_out)
{
    if (!ones || !params) return fail(RBF_EINVAL, "null pointer");
    for (uint32_t f = 0; f < nframes; ++f) {
        double k = 0.0; uint64_t l = 0;
        if (int r = rbf_optimal_params(n, ones[f], &k, &l)) return r;
        // compress(): `p >= P_STAR` is already (0, 0) in _calculate_optimal_params (:177, :215)
        const bool skip = (l == 0) || (guard_l_ge_n && l >= n) || l > 0xFFFFFFFFull;
        params[f].m = 0; params[f].floor_k = 0; params[f].threshold = 0;
        if (!skip) {
            params[f].m = (uint32_t)l;
            if (int r = rbf_activation_threshold(k, &params[f].floor_k, &params[f].threshold)) return r;
        }
        if (k_out) k_out[f] = skip ? 0.0 : k;
    }
    return RBF_OK;
}

// ---- A1
int rbf_residual_mask_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                            uint32_t nframes, uint32_t width, uint32_t height,
                            uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                            void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev)
{
    return rbf_residual_mask_batch_ex(ctx, frames_dev, frame_stride_bytes, nframes, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes,
                                      thr_floor, thr_floors, masks_dev, mask_stride_bytes, ones_dev, 1);
}

int rbf_residual_mask_batch_ex(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                               uint32_t nframes, uint32_t width, uint32_t height,
                               uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                               uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                               void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev, uint32_t mask_channels)
{
    const FrameLayout l{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes};
    return residual_mask_impl(ctx, MaskArgs{frames_dev, l, nframes, thr_floor, thr_floors, masks_dev, mask_stride_bytes, ones_dev, mask_channels}, true);
}

// ---- A1, near-lossless: the temporal hold in front of the mask stage (rbf_kernels_hold.h) and the look-ahead hold
// (rbf_kernels_lookahead.h), each with one bound (max_error) or with a bound per sample (bounds_dev, a frame of bounds): the four entry
// points share their checks, their runs and their no-op cases.
struct HoldCall {
    void *frames_dev; uint64_t frame_stride_bytes; uint32_t nframes, width, height, channels, sample_bytes;
    bool lookahead, map;             // the rule; map: bounds_dev instead of max_error
    uint32_t max_error; const void *bounds_dev;
    const uint8_t *run_starts;
};

static int temporal_hold_impl(rbf_ctx *ctx, const HoldCall &c)
{
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk{c.width, c.height, c.channels, c.sample_bytes, c.frame_stride_bytes};
    const uint32_t sample_bytes = c.sample_bytes, channels = c.channels, nframes = c.nframes, max_error = c.max_error;
    const uint64_t frame_stride_bytes = c.frame_stride_bytes, n = blk.n();
    if (int r = check_block_shape(blk, nframes)) return r;
    if (c.map) {
        if (!c.bounds_dev) return fail(RBF_EINVAL, "null bounds_dev");
        if ((uintptr_t)c.bounds_dev % sample_bytes) return fail(RBF_EINVAL, "bounds misaligned for %u-byte samples", sample_bytes);
        if (nframes < 2) return RBF_OK;                           // y = x
    } else {
        if (max_error >> (8 * sample_bytes)) return fail(RBF_ERANGE, "max_error %u does not fit a %u-bit sample", max_error, 8 * sample_bytes);
        if (max_error == 0 || nframes < 2) return RBF_OK;         // y = x
    }
    if (!c.frames_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_block_at(blk, nframes, c.frames_dev)) return r;
    // lane tiles of 16 pixels through 16-byte accesses (look-ahead: 8 pixels, 8-byte accesses) where the layout allows them -- the frames'
    // base and stride, and the bound frame's base --, the per-pixel kernel for everything else
    const bool vec = !ctx->knobs.force_generic && lanes_aligned(c.lookahead ? 8 : 16, (uintptr_t)c.frames_dev, (uintptr_t)c.bounds_dev, frame_stride_bytes);
    const LaneSplit sp = split_lanes(n, c.lookahead ? LA_LANE_PIXELS : HOLD_LANE_PIXELS, WG_THREADS, WG_THREADS, WG_WAVES, vec);
    if (!sp.fits()) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)n);
    const uint64_t bits_stride = (n + 7) / 8;                     // look-ahead, the segment-start bits: a row per frame, a byte per lane tile
    if (c.lookahead && sp.units) { if (int r = ctx->hold_bits.reserve((size_t)nframes * bits_stride)) return r; }
    uint8_t *const frames = (uint8_t *)c.frames_dev, *const bits = ctx->hold_bits.p;
    const uint8_t *const bounds = (const uint8_t *)c.bounds_dev;
    HoldRuns runs{}; uint32_t count = 0;
    auto go = [&](auto kernel, uint64_t bx, auto... args) {      // `bx` workgroups per run of the flush
        hipLaunchKernelGGL(kernel, dim3((uint32_t)bx, count), dim3(WG_THREADS), 0, ctx->stream, frames, frame_stride_bytes, args..., runs);
    };
    auto flush = [&]() {
        if (!count) return;
        LaunchTimer t(ctx, RBF_K_HOLD);
        if (sp.units)
            by_sample_and_channels(sample_bytes, channels, [&](auto s, auto ch) {
                using S = decltype(s);
                constexpr int C = decltype(ch)::value;
                if (!c.lookahead && !c.map) go(k_temporal_hold<S, C>, sp.bx_vec, sp.units, max_error);
                else if (!c.lookahead) go(k_hold_map<S, C>, sp.bx_vec, sp.units, bounds);
                else if (!c.map) go(k_temporal_lookahead<S, C>, sp.bx_vec, sp.units, max_error, bits, bits_stride);
                else go(k_lookahead_map<S, C>, sp.bx_vec, sp.units, bounds, bits, bits_stride);
                if (c.lookahead) go(k_lookahead_fill<S, C>, sp.bx_vec, sp.units, bits, bits_stride);
            });
        if (sp.first_px < n)
            by_sample_width(sample_bytes, [&](auto s) {
                if (!c.lookahead && !c.map) go(k_temporal_hold_px<decltype(s)>, sp.bx_px, sp.first_px, n, channels, max_error);
                else if (!c.lookahead) go(k_hold_map_px<decltype(s)>, sp.bx_px, sp.first_px, n, channels, bounds);
                else if (!c.map) go(k_temporal_lookahead_px<decltype(s)>, sp.bx_px, sp.first_px, n, channels, max_error);
                else go(k_lookahead_map_px<decltype(s)>, sp.bx_px, sp.first_px, n, channels, bounds);
            });
        count = 0;
    };
    for_each_run(c.run_starts, nframes, [&](uint32_t first, uint32_t len) {
        if (len < 2) return 0;                                    // a run of one frame has nothing to hold
        runs.first[count] = first; runs.len[count] = len;
        if (++count == HOLD_MAX_RUNS) flush();
        return 0;
    });
    flush();
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

int rbf_temporal_hold_runs(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                           uint32_t max_error, const uint8_t *run_starts)
{
    return temporal_hold_impl(ctx, HoldCall{frames_dev, frame_stride_bytes, nframes, width, height, channels, sample_bytes, false, false, max_error, nullptr, run_starts});
}

int rbf_temporal_lookahead_runs(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                                uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                                uint32_t max_error, const uint8_t *run_starts)
{
    return temporal_hold_impl(ctx, HoldCall{frames_dev, frame_stride_bytes, nframes, width, height, channels, sample_bytes, true, false, max_error, nullptr, run_starts});
}

int rbf_temporal_hold_runs_map(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                               uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                               const void *bounds_dev, const uint8_t *run_starts)
{
    return temporal_hold_impl(ctx, HoldCall{frames_dev, frame_stride_bytes, nframes, width, height, channels, sample_bytes, false, true, 0, bounds_dev, run_starts});
}

int rbf_temporal_lookahead_runs_map(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                                    uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                                    const void *bounds_dev, const uint8_t *run_starts)
{
    return temporal_hold_impl(ctx, HoldCall{frames_dev, frame_stride_bytes, nframes, width, height, channels, sample_bytes, true, true, 0, bounds_dev, run_starts});
}

int rbf_bgr_to_gray_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                          uint32_t sample_bytes, void *gray_dev)
{
    const FrameLayout l{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes};
    return pixel_pass(ctx, frames_dev, l, nframes, 3, gray_dev, RBF_K_MASK, [](auto s) { return k_bgr_to_gray<decltype(s)>; });
}

int rbf_extract_luma_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                           uint32_t sample_bytes, void *luma_dev)
{
    const FrameLayout l{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes};
    // (untimed: an upload-time pass, not a kernel of the step)
    return pixel_pass(ctx, frames_dev, l, nframes, 1, luma_dev, -1, [](auto s) { return k_extract_luma<decltype(s)>; });
}

// A1, adaptive threshold: 5x5 median residual and its exact moments
int rbf_noise_moments_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                            uint32_t nframes, uint32_t width, uint32_t height,
                            uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, int64_t *moments_dev, float *noise_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !moments_dev) return fail(RBF_EINVAL, "null device pointer");
    const FrameLayout l{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes};
    if (int r = check_layout(l, nframes, frame_pass_rules(1))) return r;
    if ((uint64_t)width * height >= (1ull << 32)) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)width * height);
    const uint32_t by = (height + NZ_TILE_H - 1) / NZ_TILE_H;
    if (by > 65535) return fail(RBF_ERANGE, "frame height %u too large", height);
    HIP_TRY(hipMemsetAsync(moments_dev, 0, (size_t)nframes * 2 * sizeof(int64_t), ctx->stream));
    const dim3 grid((width + NZ_TILE_W - 1) / NZ_TILE_W, by, nframes), block(NZ_THREADS);
    LaunchTimer t(ctx, RBF_K_NOISE);
    by_sample_width(sample_bytes, [&](auto s) {
        hipLaunchKernelGGL(k_noise_moments<decltype(s)>, grid, block, 0, ctx->stream, (const uint8_t *)frames_dev, frame_stride_bytes, width, height,
                           row_pitch_bytes, pixel_stride_bytes, (unsigned long long *)moments_dev, noise_dev);
    });
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- A4 + A5
int rbf_bloom_encode_batch(rbf_ctx *ctx, const void *masks_dev, uint64_t mask_stride_bytes,
                           uint64_t n, uint32_t nframes, const rbf_filter_params *params,
                           const rbf_seeds *seeds,
                           void *filters_dev, uint64_t filter_stride_bytes,
                           void *witnesses_dev, uint64_t witness_stride_bytes,
                           uint64_t *stats_dev)
{
    return encode_batch_impl(ctx, BloomBatch{(void *)masks_dev, mask_stride_bytes, n, nframes, params, seeds, filters_dev, filter_stride_bytes,
                                             witnesses_dev, witness_stride_bytes, stats_dev}, false);
}

// The two halves of rbf_encode_gop (`..._masks()` -> host -> `..._blooms()`).  begin: every check, then the mask stage is
// enqueued and the call returns; finish: wait for the counts the mask kernel's last workgroup publishes into pinned host memory, the
// float64 parameter math, then insert / reduce / query / compaction are enqueued.  One GOP per context is between the two at a time;
// a caller with several contexts issues begin(k + 1) before finish(k), so that its thread never stands still while a mask kernel runs.
int rbf_encode_gop(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                   uint32_t nframes, uint32_t width, uint32_t height,
                   uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                   uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                   const rbf_seeds *seeds,
                   void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                   void *filters_dev, uint64_t filter_stride_bytes,
                   void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev,
                   rbf_filter_params *params_out, double *k_out)
{
    if (int r = rbf_encode_gop_begin(ctx, frames_dev, frame_stride_bytes, nframes, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes,
                                     thr_floor, thr_floors, seeds, masks_dev, mask_stride_bytes, ones_dev, filters_dev, filter_stride_bytes,
                                     witnesses_dev, witness_stride_bytes, stats_dev))
        return r;
    return rbf_encode_gop_finish(ctx, params_out, k_out);
}

int rbf_encode_gop_begin(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                         uint32_t nframes, uint32_t width, uint32_t height,
                         uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                         uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                         const rbf_seeds *seeds,
                         void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                         void *filters_dev, uint64_t filter_stride_bytes,
                         void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev)
{
    return rbf_encode_runs_begin(ctx, frames_dev, frame_stride_bytes, nframes, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes,
                                 thr_floor, thr_floors, nullptr, seeds, masks_dev, mask_stride_bytes, ones_dev, filters_dev, filter_stride_bytes,
                                 witnesses_dev, witness_stride_bytes, stats_dev);
}

int rbf_encode_gop_poll(rbf_ctx *ctx, int *ready)
{
    if (!ctx || !ready) return fail(RBF_EINVAL, "null pointer");
    if (!ctx->gop.active) return fail(RBF_EINVAL, "rbf_encode_gop_poll: no GOP has been begun on this context");
    *ready = __atomic_load_n((volatile uint64_t *)ctx->ones_pinned, __ATOMIC_ACQUIRE) == ctx->gop.token ? 1 : 0;
    return RBF_OK;
}

uint64_t rbf_filter_stride_min(uint64_t n)
{
    // l = int(p n k / ln 2) with k = log2((1 - p) ln(2)^2 / p) peaks at p = 0.13183 with l = 0.316053 n (improved_video_compressor.py:181-193)
    const uint64_t lmax = (uint64_t)(0.3161 * (double)n) + 2;
    return (lmax + 63) / 64 * 8;
}

int rbf_encode_runs_begin(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                          uint32_t nframes, uint32_t width, uint32_t height,
                          uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                          uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                          const uint8_t *run_starts, const rbf_seeds *seeds,
                          void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                          void *filters_dev, uint64_t filter_stride_bytes,
                          void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev)
{
    return rbf_encode_runs_begin_ex(ctx, frames_dev, frame_stride_bytes, nframes, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes,
                                    thr_floor, thr_floors, run_starts, seeds, masks_dev, mask_stride_bytes, ones_dev, filters_dev, filter_stride_bytes,
                                    witnesses_dev, witness_stride_bytes, stats_dev, 1);
}

// The pinned block [flag | ones...] of at least `pairs` counts and the host vectors the second half plans into.
static int reserve_gop_staging(rbf_ctx *ctx, uint32_t pairs)
{
    if (pairs <= ctx->host_cap) return RBF_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->ones_pinned) HIP_TRY(hipHostFree(ctx->ones_pinned));
    ctx->ones_pinned = nullptr; ctx->host_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&ctx->ones_pinned, (size_t)(pairs + 17) * sizeof(uint64_t), hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void **)&ctx->ones_mapped_dev, ctx->ones_pinned, 0));
    ctx->ones_pinned[0] = 0;
    try {                                                    // the C ABI never throws
        ctx->plan.resize(pairs + 16);
        ctx->plan_k.resize(pairs + 16);
    } catch (...) {
        return fail(RBF_ENOMEM, "out of host memory for %u frame plans", pairs);
    }
    ctx->host_cap = pairs + 16;
    return RBF_OK;
}

int rbf_encode_runs_begin_ex(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                             uint32_t nframes, uint32_t width, uint32_t height,
                             uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                             uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                             const uint8_t *run_starts, const rbf_seeds *seeds,
                             void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                             void *filters_dev, uint64_t filter_stride_bytes,
                             void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev, uint32_t mask_channels)
{
    if (!ctx) return fail(RBF_EINVAL, "null context");
    if (ctx->gop.active)
        return fail(RBF_EINVAL, "rbf_encode_runs_begin / rbf_encode_gop_begin: the previous block of this context has not been finished "
                                "(rbf_encode_gop_finish)");
    if (!filters_dev || !witnesses_dev || !stats_dev || !seeds) return fail(RBF_EINVAL, "null pointer");
    if (int r = set_device(ctx)) return r;
    // nothing below this block has run, and nothing of the caller's has been touched, when an argument is bad
    const FrameLayout l{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes};
    const MaskArgs mask{frames_dev, l, nframes, thr_floor, thr_floors, masks_dev, mask_stride_bytes, ones_dev, mask_channels};
    if (int r = check_mask_args(mask)) return r;
    const uint32_t pairs = nframes - 1;
    const uint64_t n = (uint64_t)width * height;
    if (int r = check_witness_stride(n, witness_stride_bytes)) return r;
    if (filter_stride_bytes % 8) return fail(RBF_EINVAL, "filter stride must be a multiple of 8");
    // the filters are planned in the second half, from the counts: the stride has to cover whatever the planner can produce for n pixels
    if (filter_stride_bytes < rbf_filter_stride_min(n))
        return fail(RBF_EINVAL, "rbf_encode_runs_begin / rbf_encode_gop_begin: filter stride %llu < rbf_filter_stride_min(%llu) = %llu",
                    (unsigned long long)filter_stride_bytes, (unsigned long long)n, (unsigned long long)rbf_filter_stride_min(n));
    if (int r = check_base8(masks_dev, "masks_dev")) return r;
    if (int r = check_base8(ones_dev, "ones_dev")) return r;
    if (int r = check_base8(filters_dev, "filters_dev")) return r;
    if (int r = check_base8(witnesses_dev, "witnesses_dev")) return r;
    if (int r = check_base8(stats_dev, "stats_dev")) return r;
    bool has_skip = false;
    if (run_starts) {
        try { ctx->run_skip.assign(pairs, 0); } catch (...) { return fail(RBF_ENOMEM, "out of host memory for %u pairs", pairs); }
        for (uint32_t p2 = 0; p2 < pairs; ++p2)
            if (run_starts[p2 + 1]) { ctx->run_skip[p2] = 1; has_skip = true; }
    }
    if (int r = reserve_gop_staging(ctx, pairs)) return r;
    // The GPU publishes the counts straight into host memory and clears the stats rows in the same pass -- inside the mask
    // kernel when it covers the whole frame, else through k_finish_ones -- so the only thing between the mask kernel and the
    // Bloom kernels is the host's float64 parameter math.  (The witness rows are not cleared any more: k_chunk_offsets zeroes the dwords
    // the compaction's workgroups share, the compaction writes everything else.)
    const uint64_t token = ++ctx->publish_token;
    MaskFinish tail{};
    tail.host_block = ctx->ones_mapped_dev; tail.token = token;
    tail.clear_a = nullptr; tail.quads_a = 0;
    tail.clear_b = (uint4 *)stats_dev;     tail.quads_b = (uint64_t)pairs * RBF_STATS_PER_FRAME * 8 / 16;
    if (int r = residual_mask_impl(ctx, mask, false, &tail, has_skip ? ctx->run_skip.data() : nullptr)) return r;
    rbf_ctx::PendingGop &g = ctx->gop;
    g.active = true; g.token = token; g.seeds = *seeds; g.has_skip = has_skip;
    g.batch = BloomBatch{masks_dev, mask_stride_bytes, n, pairs, nullptr, nullptr, filters_dev, filter_stride_bytes, witnesses_dev,
                         witness_stride_bytes, stats_dev};
    return RBF_OK;
}

int rbf_encode_runs(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                    uint32_t nframes, uint32_t width, uint32_t height,
                    uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                    uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                    const uint8_t *run_starts, const rbf_seeds *seeds,
                    void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                    void *filters_dev, uint64_t filter_stride_bytes,
                    void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev,
                    rbf_filter_params *params_out, double *k_out)
{
    if (int r = rbf_encode_runs_begin(ctx, frames_dev, frame_stride_bytes, nframes, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes,
                                      thr_floor, thr_floors, run_starts, seeds, masks_dev, mask_stride_bytes, ones_dev, filters_dev, filter_stride_bytes,
                                      witnesses_dev, witness_stride_bytes, stats_dev))
        return r;
    return rbf_encode_gop_finish(ctx, params_out, k_out);
}

int rbf_encode_gop_finish(rbf_ctx *ctx, rbf_filter_params *params_out, double *k_out)
{
    if (!ctx) return fail(RBF_EINVAL, "null context");
    if (!ctx->gop.active) return fail(RBF_EINVAL, "rbf_encode_gop_finish: no GOP has been begun on this context");
    if (int r = set_device(ctx)) return r;
    rbf_ctx::PendingGop g = ctx->gop;
    const uint32_t pairs = g.batch.nframes;
    ctx->gop.active = false;                                      // whatever happens below, the context is free for the next begin
    volatile uint64_t *flag = ctx->ones_pinned;
    for (uint64_t spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != g.token; ++spins) {
        if ((spins & 0xFFFF) == 0xFFFF) {                    // every ~65k polls make sure the stream is still alive
            hipError_t q = hipStreamQuery(ctx->stream);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(RBF_EIO, "stream failed while waiting for the mask kernel: %s", hipGetErrorString(q));
            if (q == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != g.token)
                return fail(RBF_EIO, "mask kernel finished without publishing its counts");
        }
        __builtin_ia32_pause();
    }
    if (g.has_skip)                                               // (zero by construction: a skipped pair's row is written as zeros and never counted)
        for (uint32_t p = 0; p < pairs; ++p) if (ctx->run_skip[p]) ctx->ones_pinned[1 + p] = 0;
    if (int r = rbf_plan_batch(g.batch.n, ctx->ones_pinned + 1, pairs, 1, ctx->plan.data(), ctx->plan_k.data())) return r;
    if (params_out) {
        memcpy(params_out, ctx->plan.data(), (size_t)pairs * sizeof(rbf_filter_params));
        if (g.has_skip) for (uint32_t p = 0; p < pairs; ++p) if (ctx->run_skip[p]) params_out[p].floor_k = RBF_PAIR_SKIPPED;
    }
    if (k_out) memcpy(k_out, ctx->plan_k.data(), (size_t)pairs * sizeof(double));
    g.batch.params = ctx->plan.data(); g.batch.seeds = &g.seeds;
    return encode_batch_impl(ctx, g.batch, true, ctx->ones_pinned + 1);
}

// ---- exact-size record of a batch (what the multi-GPU gather moves)
uint64_t rbf_record_max_bytes(uint32_t nframes, uint64_t n)
{
    // header + per frame: a filter (or the passthrough mask) and a witness of at most n bits each
    return (uint64_t)(RECORD_HEADER_WORDS + RECORD_ROW_WORDS * (uint64_t)nframes) * 8 + (uint64_t)nframes * 2 * (((n + 63) / 64) * 8);
}

int rbf_pack_records(rbf_ctx *ctx, uint32_t nframes, uint64_t n, const rbf_filter_params *params, const double *k,
                     const void *masks_dev, uint64_t mask_stride_bytes,
                     const void *filters_dev, uint64_t filter_stride_bytes,
                     const void *witnesses_dev, uint64_t witness_stride_bytes,
                     const uint64_t *stats_dev, void *record_dev, uint64_t capacity_bytes)
{
    if (int r = set_device(ctx)) return r;
    if (!params || !masks_dev || !filters_dev || !witnesses_dev || !stats_dev || !record_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_frame_geometry(n, nframes, mask_stride_bytes)) return r;
    if (filter_stride_bytes % 8 || witness_stride_bytes % 8 || ((uintptr_t)record_dev % 8))
        return fail(RBF_EINVAL, "strides and the record must be 8-byte aligned");
    if (int r = check_base8(masks_dev, "masks_dev")) return r;
    if (int r = check_base8(filters_dev, "filters_dev")) return r;
    if (int r = check_base8(witnesses_dev, "witnesses_dev")) return r;
    if (int r = check_base8(stats_dev, "stats_dev")) return r;
    const uint64_t header = (uint64_t)(RECORD_HEADER_WORDS + RECORD_ROW_WORDS * (uint64_t)nframes) * 8;
    if (capacity_bytes < header || capacity_bytes % 8)
        return fail(RBF_EINVAL, "record capacity %llu is smaller than the %llu-byte header or misaligned", (unsigned long long)capacity_bytes,
                    (unsigned long long)header);
    for (uint32_t f = 0; f < nframes; ++f)
        if (params[f].m && ((uint64_t)params[f].m + 63) / 64 * 8 > filter_stride_bytes)
            return fail(RBF_EINVAL, "frame %u: filter of %u bits exceeds the filter stride", f, params[f].m);
    if (int r = ctx->pack_base.reserve(((size_t)nframes / PACK_BATCH + 2) * 8)) return r;
    for (uint32_t first = 0; first < nframes; first += PACK_BATCH) {
        const uint32_t cnt = nframes - first < (uint32_t)PACK_BATCH ? nframes - first : (uint32_t)PACK_BATCH;
        PackTable tab{};
        for (uint32_t i = 0; i < cnt; ++i) {
            PackRow &r = tab.r[i];
            r.m = params[first + i].m; r.floor_k = params[first + i].floor_k; r.threshold = params[first + i].threshold;
            const double kv = k ? k[first + i] : 0.0;
            memcpy(&r.k_bits, &kv, 8);
        }
        LaunchTimer t(ctx, RBF_K_PACK);
        hipLaunchKernelGGL(k_pack_records, dim3(8, 2 * cnt), dim3(256), 0, ctx->stream, tab, first, cnt, nframes, n, stats_dev,
                           (const uint8_t *)masks_dev, mask_stride_bytes, (const uint8_t *)filters_dev, filter_stride_bytes,
                           (const uint8_t *)witnesses_dev, witness_stride_bytes, (uint64_t *)record_dev, capacity_bytes, ctx->pack_base.p);
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- A6
int rbf_bloom_decode_batch(rbf_ctx *ctx, const void *filters_dev, uint64_t filter_stride_bytes,
                           const void *witnesses_dev, uint64_t witness_stride_bytes,
                           uint64_t n, uint32_t nframes, const rbf_filter_params *params,
                           const rbf_seeds *seeds,
                           void *masks_dev, uint64_t mask_stride_bytes)
{
    if (int r = set_device(ctx)) return r;
    if (!filters_dev || !witnesses_dev || !params || !seeds || !masks_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_frame_geometry(n, nframes, mask_stride_bytes)) return r;
    if (int r = check_filter_strides(params, nframes, filter_stride_bytes)) return r;
    if (witness_stride_bytes % 8) return fail(RBF_EINVAL, "witness stride must be a multiple of 8");
    if (int r = check_base8(filters_dev, "filters_dev")) return r;
    if (int r = check_base8(witnesses_dev, "witnesses_dev")) return r;
    if (int r = check_base8(masks_dev, "masks_dev")) return r;
    const BloomBatch b{masks_dev, mask_stride_bytes, n, nframes, params, seeds, (void *)filters_dev, filter_stride_bytes,
                       (void *)witnesses_dev, witness_stride_bytes, nullptr};
    for (uint32_t f0 = 0; f0 < nframes; f0 += MAX_BATCH)
        if (int r = decode_chunk(ctx, b.rows(f0, std::min(nframes - f0, (uint32_t)MAX_BATCH)))) return r;
    return RBF_OK;
}

// ---- per-index surface
int rbf_filter_insert_indices(rbf_ctx *ctx, void *filter_dev, const rbf_filter_params *params,
                              const rbf_seeds *seeds, const uint32_t *indices_dev, uint64_t count)
{
    return index_call(ctx, filter_dev, params, seeds, 0, count, indices_dev != nullptr, [&](const FrameDev &fd, const Seeds &sd, dim3 grid) {
        hipLaunchKernelGGL(k_index_insert, grid, dim3(WG_THREADS), 0, ctx->stream, (uint32_t *)filter_dev, fd, sd, indices_dev, count);
    });
}

int rbf_filter_query_indices(rbf_ctx *ctx, const void *filter_dev, const rbf_filter_params *params,
                             const rbf_seeds *seeds, const uint32_t *indices_dev, uint64_t count,
                             uint8_t *out_dev)
{
    return index_call(ctx, filter_dev, params, seeds, 0, count, indices_dev && out_dev, [&](const FrameDev &fd, const Seeds &sd, dim3 grid) {
        hipLaunchKernelGGL(k_index_query, grid, dim3(WG_THREADS), 0, ctx->stream, (const uint32_t *)filter_dev, fd, sd, indices_dev, count, out_dev);
    });
}

int rbf_filter_insert_keys(rbf_ctx *ctx, void *filter_dev, const rbf_filter_params *params,
                           const rbf_seeds *seeds, uint32_t standard_k,
                           const uint8_t *keys_dev, const uint32_t *offsets_dev, uint64_t count)
{
    return index_call(ctx, filter_dev, params, seeds, standard_k, count, keys_dev && offsets_dev, [&](const FrameDev &fd, const Seeds &sd, dim3 grid) {
        hipLaunchKernelGGL(k_keys<true>, grid, dim3(WG_THREADS), 0, ctx->stream, (uint32_t *)filter_dev, fd, sd, standard_k, keys_dev, offsets_dev,
                           count, (uint8_t *)nullptr);
    });
}

int rbf_filter_query_keys(rbf_ctx *ctx, const void *filter_dev, const rbf_filter_params *params,
                          const rbf_seeds *seeds, uint32_t standard_k,
                          const uint8_t *keys_dev, const uint32_t *offsets_dev, uint64_t count,
                          uint8_t *out_dev)
{
    return index_call(ctx, filter_dev, params, seeds, standard_k, count, keys_dev && offsets_dev && out_dev,
                      [&](const FrameDev &fd, const Seeds &sd, dim3 grid) {
        hipLaunchKernelGGL(k_keys<false>, grid, dim3(WG_THREADS), 0, ctx->stream, (uint32_t *)filter_dev, fd, sd, standard_k, keys_dev, offsets_dev,
                           count, out_dev);
    });
}

// ---- A2 / A8
int rbf_gather_values(rbf_ctx *ctx, const void *frame_dev, uint32_t width, uint32_t height,
                      uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes, uint32_t sample_bytes,
                      uint32_t channels, const void *mask_dev, void *values_dev, uint64_t *count_dev)
{
    if (!count_dev) return fail(RBF_EINVAL, "count_dev is null");
    return values_common(ctx, (void *)frame_dev, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, channels, mask_dev, values_dev,
                         count_dev, false);
}

int rbf_gather_values_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                            uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, uint32_t channels, const void *masks_dev, uint64_t mask_stride_bytes,
                            void *values_dev, uint64_t capacity_pixels, uint64_t *offsets_dev, uint64_t *uncovered_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !masks_dev || !values_dev || !offsets_dev) return fail(RBF_EINVAL, "null device pointer");
    LayoutRules rules;
    rules.samples = channels; rules.channels = true; rules.min_frames = 2;
    if (int r = check_layout(FrameLayout{width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, frame_stride_bytes}, nframes, rules)) return r;
    const uint64_t n = (uint64_t)width * height;
    const uint32_t pairs = nframes - 1;
    if (pairs > 65535) return fail(RBF_ERANGE, "at most 65536 frames per call");
    if (int r = check_frame_geometry(n, pairs, mask_stride_bytes)) return r;
    const uint64_t nseg = (n + SEG_PIXELS - 1) / SEG_PIXELS, nwords = (n + 63) / 64;
    if (int r = ctx->pack_base.reserve(((size_t)pairs + 2) * 8)) return r;     // per-pair totals
    LaunchTimer t(ctx, RBF_K_GATHER);
    if (int r = count_and_scan_masks(ctx, masks_dev, mask_stride_bytes, n, pairs, ctx->pack_base.p)) return r;
    hipLaunchKernelGGL(k_frame_offsets, dim3(1), dim3(64), 0, ctx->stream, ctx->pack_base.p, offsets_dev, pairs);
    const dim3 grid((uint32_t)((nwords + WG_THREADS - 1) / WG_THREADS), pairs);
    by_sample_width(sample_bytes, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL(k_gather_words<S>, grid, dim3(WG_THREADS), 0, ctx->stream, (const uint8_t *)frames_dev, frame_stride_bytes, width, n,
                           row_pitch_bytes, pixel_stride_bytes, channels, (const uint64_t *)masks_dev, mask_stride_bytes / 8, ctx->seg_off.p, nseg,
                           offsets_dev, (S *)values_dev, capacity_pixels);
    });
    if (uncovered_dev) {
        HIP_TRY(hipMemsetAsync(uncovered_dev, 0, (size_t)pairs * 8, ctx->stream));
        const uint64_t bx = std::min<uint64_t>(std::max<uint64_t>((n + WG_THREADS * 8 - 1) / (WG_THREADS * 8), 1), 4096);
        by_sample_width(sample_bytes, [&](auto s) {
            hipLaunchKernelGGL(k_uncovered_changes<decltype(s)>, dim3((uint32_t)bx, pairs), dim3(WG_THREADS), 0, ctx->stream,
                               (const uint8_t *)frames_dev, frame_stride_bytes, width, n, row_pitch_bytes, pixel_stride_bytes, channels,
                               (const uint64_t *)masks_dev, mask_stride_bytes / 8, (unsigned long long *)uncovered_dev);
        });
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

int rbf_scatter_values(rbf_ctx *ctx, void *frame_dev, uint32_t width, uint32_t height,
                       uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes, uint32_t sample_bytes,
                       uint32_t channels, const void *mask_dev, const void *values_dev)
{
    return values_common(ctx, frame_dev, width, height, row_pitch_bytes, pixel_stride_bytes, sample_bytes, channels, mask_dev, (void *)values_dev,
                         nullptr, true);
}

// ---- sample codec (rbf_rice_host.h)
int rbf_rice_encode_intra(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                          void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !out_dev || !stream_bytes) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    if (nframes == 0 || nframes > 65535) return fail(RBF_EINVAL, "nframes must be 1..65535, got %u", nframes);
    const uint64_t n = (uint64_t)width * height * channels;
    if (int r = rice_check_dense(frame_stride_bytes, n, sample_bytes)) return r;
    RicePlan p;
    std::vector<uint64_t> ns;
    try { ns.assign(nframes, n); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    if (int r = rice_plan(ns.data(), nframes, 8 * sample_bytes, capacity_bytes, &p)) return r;
    if (int r = rice_stage(ctx, p)) return r;
    const dim3 grid((uint32_t)(((uint64_t)width * channels + WG_THREADS - 1) / WG_THREADS), height, nframes);
    int rc = RBF_OK;
    by_sample_width(sample_bytes, [&](auto s) {
        constexpr uint32_t B = 8 * sizeof s;
        hipLaunchKernelGGL(k_rice_intra_u<decltype(s)>, grid, dim3(WG_THREADS), 0, ctx->stream, (const uint8_t *)frames_dev, frame_stride_bytes, width,
                           channels, B, ctx->rice_u.p);
        rc = rice_encode_streams<B>(ctx, p, out_dev, stream_bytes);
    });
    return rc;
}

int rbf_rice_decode_intra(rbf_ctx *ctx, const void *stream, uint64_t stream_bytes, uint32_t width, uint32_t height,
                          uint32_t channels, uint32_t sample_bytes, void *frame_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!stream || !frame_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    const uint64_t want = (uint64_t)width * height * channels;
    std::vector<RiceChunk> ch;
    uint64_t n = 0;
    if (int r = rice_parse((const uint8_t *)stream, stream_bytes, 0, 8 * sample_bytes, 0, 0, &ch, &n)) return r;
    if (n != want)
        return fail(RBF_EINVAL, "the stream carries %llu samples, a %ux%ux%u frame has %llu", (unsigned long long)n, width, height, channels,
                    (unsigned long long)want);
    if (int r = rice_decode(ctx, stream, stream_bytes, ch, n)) return r;
    by_sample_width(sample_bytes, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL(k_rice_intra_rebuild<S>, dim3((height + WG_WAVES - 1) / WG_WAVES), dim3(WG_THREADS), 0, ctx->stream, ctx->rice_u.p, width,
                           height, channels, (uint32_t)(8 * sizeof s), (S *)frame_dev);
    });
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- bounded-error keyframes (rbf_kernels_keyquant.h)
// The per-channel table of a call: bounds (host, `channels` entries, each <= 65535) -> bound, step and the step's reciprocal.
static int keyquant_table(const uint32_t *bounds, uint32_t channels, KeyQuant *kq)
{
    *kq = KeyQuant{};
    for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t d = c < channels ? bounds[c] : 0;
        if (d > 65535) return fail(RBF_EINVAL, "bound %u of channel %u: a bound is at most 65535", d, c);
        const uint32_t t = 2 * d + 1;
        kq->d[c] = d; kq->t[c] = t;
        if (d) {
            uint32_t L = 0;
            while ((t >> (L + 1)) != 0) ++L;                       // floor(log2 t) >= 1
            const uint64_t K = 31 + L;
            kq->m[c] = (uint32_t)((((uint64_t)1 << K) + t - 1) / t);
            kq->sh[c] = L - 1;
        }
    }
    return RBF_OK;
}

int rbf_rice_encode_intra_near(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, const uint32_t *frame_index, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes, const uint32_t *bounds,
                               void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !frame_index || !bounds || !out_dev || !stream_bytes) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    if (count == 0 || count > 65535) return fail(RBF_EINVAL, "count must be 1..65535, got %u", count);
    for (uint32_t i = 0; i < count; ++i) {
        if (frame_index[i] >= 65535) return fail(RBF_EINVAL, "frame index %u: a block holds at most 65535 frames", frame_index[i]);
        if (i && frame_index[i] <= frame_index[i - 1])           // (a frame listed twice would have two streams)
            return fail(RBF_EINVAL, "frame indices must ascend: %u after %u", frame_index[i], frame_index[i - 1]);
    }
    const uint64_t n = (uint64_t)width * height * channels;
    if (int r = rice_check_dense(frame_stride_bytes, n, sample_bytes)) return r;
    KeyQuant kq;
    if (int r = keyquant_table(bounds, channels, &kq)) return r;
    RicePlan p;
    std::vector<uint64_t> ns;
    try { ns.assign(count, n); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    if (int r = rice_plan(ns.data(), count, 8 * sample_bytes, capacity_bytes, &p)) return r;
    if (int r = rice_stage(ctx, p)) return r;
    if (int r = ctx->keyq.reserve((size_t)count * 4)) return r;
    HIP_TRY(hipMemcpyAsync(ctx->keyq.p, frame_index, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));      // (pageable: staged before the call returns)
    const dim3 grid((uint32_t)(((uint64_t)width * channels + WG_THREADS - 1) / WG_THREADS), height, count);
    int rc = RBF_OK;
    by_sample_width(sample_bytes, [&](auto s) {
        using S = decltype(s);
        constexpr uint32_t B = 8 * sizeof s;
        hipLaunchKernelGGL(k_keyquant_u<S>, grid, dim3(WG_THREADS), 0, ctx->stream, (const uint8_t *)frames_dev, frame_stride_bytes, ctx->keyq.p,
                           width, channels, kq, ctx->rice_u.p);
        hipLaunchKernelGGL(k_keyquant_apply<S>, grid, dim3(WG_THREADS), 0, ctx->stream, (uint8_t *)frames_dev, frame_stride_bytes, ctx->keyq.p,
                           width, channels, kq);
        rc = rice_encode_streams<B>(ctx, p, out_dev, stream_bytes);
    });
    return rc;
}

int rbf_rice_decode_intra_near(rbf_ctx *ctx, const void *stream, uint64_t stream_bytes, uint32_t width, uint32_t height,
                               uint32_t channels, uint32_t sample_bytes, const uint32_t *bounds, void *frame_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!stream || !bounds || !frame_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    KeyQuant kq;
    if (int r = keyquant_table(bounds, channels, &kq)) return r;
    const uint64_t want = (uint64_t)width * height * channels;
    std::vector<RiceChunk> ch;
    uint64_t n = 0;
    if (int r = rice_parse((const uint8_t *)stream, stream_bytes, 0, 8 * sample_bytes, 0, 0, &ch, &n)) return r;
    if (n != want)
        return fail(RBF_EINVAL, "the stream carries %llu samples, a %ux%ux%u frame has %llu", (unsigned long long)n, width, height, channels,
                    (unsigned long long)want);
    if (int r = rice_decode(ctx, stream, stream_bytes, ch, n)) return r;
    by_sample_width(sample_bytes, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL(k_keyquant_rebuild<S>, dim3((height + WG_WAVES - 1) / WG_WAVES), dim3(WG_THREADS), 0, ctx->stream, ctx->rice_u.p, width,
                           height, channels, kq, (S *)frame_dev);
    });
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

int rbf_rice_encode_inter(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                          const void *masks_dev, uint64_t mask_stride_bytes, const uint64_t *ones,
                          void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes)
{
    if (int r = set_device(ctx)) return r;
    if (!frames_dev || !masks_dev || !ones || !out_dev || !stream_bytes) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    if (nframes < 2 || nframes > 65536) return fail(RBF_EINVAL, "nframes must be 2..65536, got %u", nframes);
    const uint64_t npx = (uint64_t)width * height;
    const uint32_t pairs = nframes - 1;
    if (int r = check_frame_geometry(npx, pairs, mask_stride_bytes)) return r;
    if (int r = rice_check_dense(frame_stride_bytes, npx * channels, sample_bytes)) return r;
    std::vector<uint64_t> ns, got;
    try { ns.resize(pairs); got.resize(pairs); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    for (uint32_t f = 0; f < pairs; ++f) {
        if (ones[f] > npx)
            return fail(RBF_EINVAL, "pair %u: %llu changed pixels in a frame of %llu", f, (unsigned long long)ones[f], (unsigned long long)npx);
        ns[f] = ones[f] * channels;
    }
    RicePlan p;
    if (int r = rice_plan(ns.data(), pairs, 8 * sample_bytes, capacity_bytes, &p)) return r;
    const uint64_t nseg = (npx + SEG_PIXELS - 1) / SEG_PIXELS, nwords = (npx + 63) / 64;
    if (int r = ctx->pack_base.reserve(((size_t)pairs + 2) * 8)) return r;
    if (int r = rice_stage(ctx, p)) return r;
    if (int r = count_and_scan_masks(ctx, masks_dev, mask_stride_bytes, npx, pairs, ctx->pack_base.p)) return r;
    const dim3 grid((uint32_t)((nwords + WG_THREADS - 1) / WG_THREADS), pairs);
    int rc = RBF_OK;
    by_sample_width(sample_bytes, [&](auto s) {
        constexpr uint32_t B = 8 * sizeof s;
        hipLaunchKernelGGL(k_rice_inter_u<decltype(s)>, grid, dim3(WG_THREADS), 0, ctx->stream, (const uint8_t *)frames_dev, frame_stride_bytes, npx,
                           channels, (const uint64_t *)masks_dev, mask_stride_bytes / 8, ctx->seg_off.p, nseg, (const RiceStream *)ctx->rice_tab.p, B,
                           ctx->rice_u.p);
        rc = rice_encode_streams<B>(ctx, p, out_dev, stream_bytes);
    });
    if (rc) return rc;
    // the counts the caller named must be the masks' (the producer never writes past them, so a wrong count gives a wrong stream)
    HIP_TRY(hipMemcpyAsync(got.data(), ctx->pack_base.p, (size_t)pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t f = 0; f < pairs; ++f)
        if (got[f] != ones[f])
            return fail(RBF_EINVAL, "pair %u: the mask marks %llu pixels, ones[%u] = %llu", f, (unsigned long long)got[f], f, (unsigned long long)ones[f]);
    return RBF_OK;
}

int rbf_rice_apply_inter(rbf_ctx *ctx, const void *streams, const uint64_t *stream_bytes, uint32_t count,
                         uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                         const void *masks_dev, uint64_t mask_stride_bytes, void *frames_dev)
{
    if (int r = set_device(ctx)) return r;
    if (!streams || !stream_bytes || !masks_dev || !frames_dev) return fail(RBF_EINVAL, "null pointer");
    if (int r = rice_check_frame(width, height, channels, sample_bytes)) return r;
    if (count == 0 || count > 65535) return fail(RBF_EINVAL, "count must be 1..65535, got %u", count);
    const uint64_t npx = (uint64_t)width * height, fbytes = npx * channels * sample_bytes;
    if (int r = check_frame_geometry(npx, count, mask_stride_bytes)) return r;
    std::vector<RiceChunk> ch;
    std::vector<uint64_t> n, first, got;
    try { n.resize(count); first.resize(count); got.resize(count); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    uint64_t off = 0, samples = 0;
    for (uint32_t j = 0; j < count; ++j) {
        if (int r = rice_parse((const uint8_t *)streams + off, stream_bytes[j], j, 8 * sample_bytes, off / 4, samples, &ch, &n[j])) return r;
        if (n[j] % channels)
            return fail(RBF_EINVAL, "sample stream %u: %llu samples are not whole pixels of %u samples", j, (unsigned long long)n[j], channels);
        first[j] = samples;
        samples += n[j];
        off += stream_bytes[j];
    }
    const uint64_t nseg = (npx + SEG_PIXELS - 1) / SEG_PIXELS, nwords = (npx + 63) / 64;
    if (int r = ctx->pack_base.reserve(((size_t)count + 2) * 8)) return r;
    if (int r = count_and_scan_masks(ctx, masks_dev, mask_stride_bytes, npx, count, ctx->pack_base.p)) return r;
    if (int r = rice_decode(ctx, streams, off, ch, samples)) return r;              // (waits: the mask counts are in as well)
    HIP_TRY(hipMemcpyAsync(got.data(), ctx->pack_base.p, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t j = 0; j < count; ++j)
        if (got[j] * channels != n[j])
            return fail(RBF_EINVAL, "sample stream %u carries %llu samples, its mask marks %llu pixels of %u samples", j, (unsigned long long)n[j],
                        (unsigned long long)got[j], channels);
    for (uint32_t j = 0; j < count; ++j) {                                          // every frame is checked: now the frames are written
        uint8_t *dst = (uint8_t *)frames_dev + (uint64_t)(j + 1) * fbytes;
        HIP_TRY(hipMemcpyAsync(dst, dst - fbytes, fbytes, hipMemcpyDeviceToDevice, ctx->stream));
        if (!n[j]) continue;
        const uint64_t *mask = (const uint64_t *)masks_dev + (uint64_t)j * (mask_stride_bytes / 8);
        by_sample_width(sample_bytes, [&](auto s) {
            using S = decltype(s);
            hipLaunchKernelGGL(k_rice_inter_add<S>, dim3((uint32_t)((nwords + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, ctx->stream,
                               (S *)dst, npx, channels, mask, ctx->seg_off.p + (uint64_t)j * nseg, ctx->rice_u.p + first[j], n[j] / channels,
                               ctx->rice_err.p);
        });
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- scene cuts: the statistics that decide whether a frame is cheaper as a keyframe (rbf_kernels_cut.h); read-only on the frames
int rbf_cut_stats(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                  uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                  uint32_t tolerance, uint64_t *stats_dev)
{
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk{width, height, channels, sample_bytes, frame_stride_bytes};
    if (int r = check_block_shape(blk, nframes)) return r;
    if (tolerance >> (8 * sample_bytes)) return fail(RBF_ERANGE, "tolerance %u does not fit a %u-bit sample", tolerance, 8 * sample_bytes);
    if (nframes < 2) return RBF_OK;                               // no pair
    if (!frames_dev || !stats_dev) return fail(RBF_EINVAL, "null pointer");
    if ((uintptr_t)stats_dev % 8) return fail(RBF_EINVAL, "stats_dev must be 8-byte aligned");
    if (int r = check_block_at(blk, nframes, frames_dev)) return r;
    // lane tiles of 16 pixels through 16-byte loads where the layout allows them, the per-pixel kernel for everything else
    const uint64_t n = blk.n();
    const bool vec = !ctx->knobs.force_generic && lanes_aligned(16, (uintptr_t)frames_dev, frame_stride_bytes);
    const LaneSplit sp = split_lanes(n, CUT_LANE_PIXELS, WG_THREADS, WG_THREADS, WG_WAVES, vec);
    if (!sp.fits()) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)n);
    const uint32_t pairs = nframes - 1;
    if (int r = ctx->cut_partials.reserve((size_t)pairs * sp.rows * CUT_STATS * 4)) return r;      // a row of three sums per wave and pair; every row is written by every call
    const uint8_t *const frames = (const uint8_t *)frames_dev;
    uint32_t *const partials = ctx->cut_partials.p;
    if (sp.units)
        by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) {
            hipLaunchKernelGGL((k_cut_stats<decltype(s), decltype(c)::value>), dim3((uint32_t)sp.bx_vec), dim3(WG_THREADS), 0, ctx->stream, frames,
                               frame_stride_bytes, nframes, sp.units, width, tolerance, partials, sp.rows);
        });
    if (sp.first_px < n)
        by_sample_width(sample_bytes, [&](auto s) {
            hipLaunchKernelGGL(k_cut_stats_px<decltype(s)>, dim3((uint32_t)sp.bx_px), dim3(WG_THREADS), 0, ctx->stream, frames, frame_stride_bytes,
                               nframes, sp.first_px, n, width, channels, tolerance, partials, sp.rows, sp.tail_row_base);
        });
    hipLaunchKernelGGL(k_cut_reduce, dim3(pairs), dim3(WG_THREADS), 0, ctx->stream, partials, sp.rows, stats_dev);
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- quality report: what a coded block differs from its originals by (rbf_kernels_error.h); read-only on both blocks, blocks until the
// rows are on the host
int rbf_error_stats(rbf_ctx *ctx, const void *a_dev, uint64_t a_stride_bytes, const void *b_dev, uint64_t b_stride_bytes, uint32_t nframes,
                    uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                    const void *bounds_dev, uint32_t bound, rbf_error_row *rows_host)
{
    static_assert(sizeof(ErrorRow) == sizeof(rbf_error_row) && sizeof(rbf_error_row) == 32, "the kernels write the ABI's rows");
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk_a{width, height, channels, sample_bytes, a_stride_bytes}, blk_b{width, height, channels, sample_bytes, b_stride_bytes};
    if (int r = check_block_shape(blk_a, nframes)) return r;
    if (int r = check_block_shape(blk_b, nframes)) return r;
    if (!bounds_dev && bound >> (8 * sample_bytes)) return fail(RBF_ERANGE, "bound %u does not fit a %u-bit sample", bound, 8 * sample_bytes);
    const uint64_t n = blk_a.n();
    if (n * channels > 0x80000000ull) return fail(RBF_ERANGE, "frame of %llu samples is too large", (unsigned long long)(n * channels));
    if (nframes == 0) return RBF_OK;
    if (!a_dev || !b_dev || !rows_host) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_block_at(blk_a, nframes, a_dev, true)) return r;        // (a single frame has no stride to look at)
    if (int r = check_block_at(blk_b, nframes, b_dev, true)) return r;
    if ((uintptr_t)bounds_dev % sample_bytes) return fail(RBF_EINVAL, "bounds misaligned for %u-byte samples", sample_bytes);
    // lane tiles of 16 pixels through 16-byte loads where every base and stride allows them, the per-pixel kernel for everything else
    const bool vec = !ctx->knobs.force_generic && lanes_aligned(16, (uintptr_t)a_dev, (uintptr_t)b_dev, (uintptr_t)bounds_dev, nframes == 1 ? 0 : a_stride_bytes | b_stride_bytes);
    const LaneSplit sp = split_lanes(n, ERR_LANE_PIXELS, WG_THREADS, WG_THREADS, WG_WAVES, vec);     // (at most 2^31 samples: it fits)
    if (int r = ctx->err_partials.reserve((size_t)nframes * sp.rows * ERR_WORDS * 4)) return r;      // a row per wave and frame; every row is written by every call
    if (int r = ctx->err_rows.reserve((size_t)nframes * sizeof(ErrorRow))) return r;
    const uint8_t *const a = (const uint8_t *)a_dev, *const b = (const uint8_t *)b_dev, *const bounds = (const uint8_t *)bounds_dev;
    uint32_t *const partials = ctx->err_partials.p;
    if (sp.units)
        by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) {
            by_value<0, 1>(bounds != nullptr, [&](auto map) {
                hipLaunchKernelGGL((k_error_stats<decltype(s), decltype(c)::value, decltype(map)::value != 0>), dim3((uint32_t)sp.bx_vec), dim3(WG_THREADS), 0, ctx->stream,
                                   a, a_stride_bytes, b, b_stride_bytes, nframes, sp.units, bounds, bound, partials, sp.rows);
            });
        });
    if (sp.first_px < n)
        by_sample_width(sample_bytes, [&](auto s) {
            hipLaunchKernelGGL(k_error_stats_px<decltype(s)>, dim3((uint32_t)sp.bx_px), dim3(WG_THREADS), 0, ctx->stream, a, a_stride_bytes, b,
                               b_stride_bytes, nframes, sp.first_px, n, channels, bounds, bound, partials, sp.rows, sp.tail_row_base);
        });
    return fold_rows_to_host(ctx, k_error_reduce, nframes, (ErrorRow *)ctx->err_rows.p, rows_host, partials, sp.rows);
}

// ---- hold sweep: what every candidate bound would do to every run of a block (rbf_kernels_sweep.h); read-only on the block, blocks
// until the rows are on the host
int rbf_hold_sweep(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                   uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                   const uint8_t *run_starts, int lookahead,
                   const uint32_t *candidates, uint32_t ncandidates, rbf_sweep_row *rows_host)
{
    static_assert(sizeof(SweepRow) == sizeof(rbf_sweep_row) && sizeof(rbf_sweep_row) == 24, "the kernels write the ABI's rows");
    static_assert(SWEEP_MAX_RUN * 4 * 255 * 255 <= 0xFFFFFFFFu / 64, "a wave's sse of a run fits 32 bits");
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk{width, height, channels, sample_bytes, frame_stride_bytes};
    if (int r = check_block_shape(blk, nframes)) return r;
    if (ncandidates < 1 || ncandidates > SWEEP_MAX_CANDIDATES) return fail(RBF_EINVAL, "ncandidates must be 1..%u, got %u", SWEEP_MAX_CANDIDATES, ncandidates);
    if (!candidates) return fail(RBF_EINVAL, "null candidates");
    uint64_t cands = 0;
    for (uint32_t i = 0; i < ncandidates; ++i) {
        if (i && candidates[i] <= candidates[i - 1])
            return fail(RBF_EINVAL, "candidates must strictly ascend: candidates[%u] = %u after %u", i, candidates[i], candidates[i - 1]);
        if (candidates[i] > 255) return fail(RBF_ERANGE, "candidate %u above 255", candidates[i]);
        cands |= (uint64_t)candidates[i] << (8 * i);
    }
    if (nframes == 0) return RBF_OK;
    if (!frames_dev || !rows_host) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_block_at(blk, nframes, frames_dev)) return r;
    HoldRuns runs{}; uint32_t count = 0;                          // a run of one frame keeps its rows (of zeros)
    if (int r = for_each_run(run_starts, nframes, [&](uint32_t first, uint32_t len) {
            if (count == HOLD_MAX_RUNS) return fail(RBF_ERANGE, "more than %u runs", HOLD_MAX_RUNS);
            if (len > SWEEP_MAX_RUN) return fail(RBF_ERANGE, "run of %u frames at frame %u: at most %u", len, first, SWEEP_MAX_RUN);
            runs.first[count] = first; runs.len[count++] = len;
            return 0;
        })) return r;
    // workgroup tiles through 16-byte loads where the layout allows them, the per-pixel kernel for everything else; more than four
    // candidates: two halves of a workgroup share a tile of half the size.  The lane unit is the tile, one to a workgroup
    const uint64_t n = blk.n();
    const uint32_t groups = ncandidates > SWEEP_GROUP ? 2 : 1, tile = WG_THREADS / groups;
    const bool vec = !ctx->knobs.force_generic && lanes_aligned(16, (uintptr_t)frames_dev, frame_stride_bytes);
    const LaneSplit sp = split_lanes(n, tile, 1, tile, tile / WAVE, vec);
    if (!sp.fits()) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)n);
    const uint32_t cells = count * ncandidates;
    if (int r = ctx->sweep_partials.reserve((size_t)cells * sp.rows * SWEEP_WORDS * 4)) return r;      // a row per wave, run and candidate; every row is written by every call
    if (int r = ctx->sweep_rows.reserve((size_t)cells * sizeof(SweepRow))) return r;
    const uint8_t *const frames = (const uint8_t *)frames_dev;
    uint32_t *const partials = ctx->sweep_partials.p;
    by_value<0, 1>(lookahead != 0, [&](auto la) {
        constexpr bool LA = decltype(la)::value != 0;
        if (sp.units)
            by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) {
                hipLaunchKernelGGL((k_hold_sweep<decltype(s), decltype(c)::value, LA>), dim3((uint32_t)sp.bx_vec, count), dim3(WG_THREADS), 0, ctx->stream, frames,
                                   frame_stride_bytes, groups, cands, ncandidates, partials, sp.rows, runs);
            });
        if (sp.first_px < n)
            by_sample_width(sample_bytes, [&](auto s) {
                hipLaunchKernelGGL((k_hold_sweep_px<decltype(s), LA>), dim3((uint32_t)sp.bx_px, count), dim3(WG_THREADS), 0, ctx->stream, frames, frame_stride_bytes,
                                   sp.first_px, n, channels, groups, cands, ncandidates, partials, sp.rows, sp.tail_row_base, runs);
            });
    });
    return fold_rows_to_host(ctx, k_sweep_reduce, cells, (SweepRow *)ctx->sweep_rows.p, rows_host, partials, sp.rows);
}

// ---- pan alignment: the global integer shift of every pair and the roll that makes the block still (rbf_kernels_pan.h)
int rbf_pan_search(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                   uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                   uint32_t range, uint32_t tolerance, const uint8_t *run_starts, rbf_pan_stat *out)
{
    static_assert(sizeof(PanRow) == sizeof(rbf_pan_stat) && sizeof(rbf_pan_stat) == 40, "the kernels write the ABI's rows");
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk{width, height, channels, sample_bytes, frame_stride_bytes};
    if (int r = check_block_shape(blk, nframes)) return r;
    if (range < 1 || range > (uint32_t)PAN_MAX_RANGE) return fail(RBF_EINVAL, "range must be 1..%d, got %u", PAN_MAX_RANGE, range);
    if (width <= 2 * range || height <= 2 * range)
        return fail(RBF_EINVAL, "a frame of %ux%u has no grid point for range %u: width and height must exceed 2 * range", width, height, range);
    if (tolerance >> (8 * sample_bytes)) return fail(RBF_EINVAL, "tolerance %u does not fit a %u-bit sample", tolerance, 8 * sample_bytes);
    if (nframes < 2) return RBF_OK;                               // no pair
    if (!frames_dev || !out) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_block_at(blk, nframes, frames_dev)) return r;
    const uint32_t pairs = nframes - 1;
    if (pairs > 65535) return fail(RBF_ERANGE, "at most 65536 frames per call, got %u", nframes);
    const uint32_t ngx = (width - 2 * range + PAN_GRID - 1) / PAN_GRID, ngy = (height - 2 * range + PAN_GRID - 1) / PAN_GRID;
    const uint32_t tiles_x = (ngx + PAN_TX - 1) / PAN_TX, tiles_y = (ngy + PAN_TY - 1) / PAN_TY;
    const uint64_t n = blk.n(), tiles = (uint64_t)tiles_x * tiles_y, nd = 2 * range + 1;
    const uint64_t bx = (n + WG_THREADS - 1) / WG_THREADS, rows = bx * WG_WAVES;
    if (tiles > 0x7FFFFFFFull || bx > 0x7FFFFFFFull) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)n);
    if (int r = ctx->pan_partials.reserve((size_t)pairs * tiles * nd * nd * 4)) return r;
    if (int r = ctx->pan_moving.reserve((size_t)pairs * rows * PAN_COUNTS * 4)) return r;
    if (int r = ctx->pan_rows.reserve((size_t)pairs * sizeof(PanRow))) return r;
    if (int r = ctx->pan_runs.reserve((size_t)nframes)) return r;
    std::vector<uint8_t> starts;
    try { starts.assign(nframes, 0); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    if (run_starts)
        for (uint32_t t = 1; t < nframes; ++t) starts[t] = run_starts[t] ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(ctx->pan_runs.p, starts.data(), nframes, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *const frames = (const uint8_t *)frames_dev, *const runs = ctx->pan_runs.p;
    PanRow *const prow = (PanRow *)ctx->pan_rows.p;
    const uint32_t lds = pan_sad_lds_bytes(range, sample_bytes);
    by_sample_width(sample_bytes, [&](auto s) {
        by_value<8, 16, 32>(range <= 8 ? 8 : range <= 16 ? 16 : 32, [&](auto rmax) {
            hipLaunchKernelGGL((k_pan_sad<decltype(s), decltype(rmax)::value>), dim3((uint32_t)tiles, pairs), dim3(WG_THREADS), lds, ctx->stream, frames, frame_stride_bytes,
                               width, height, channels, range, ngx, ngy, tiles_x, runs, ctx->pan_partials.p);
        });
    });
    hipLaunchKernelGGL(k_pan_pick, dim3(pairs), dim3(WG_THREADS), 0, ctx->stream, ctx->pan_partials.p, (uint32_t)tiles, range, runs, prow);
    by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) {
        hipLaunchKernelGGL((k_pan_moving<decltype(s), decltype(c)::value>), dim3((uint32_t)bx, pairs), dim3(WG_THREADS), 0, ctx->stream, frames, frame_stride_bytes,
                           width, height, tolerance, runs, prow, ctx->pan_moving.p, rows);
    });
    if (int r = ctx->pan_host.reserve_rows(pairs)) return r;      // (the rows pass through it: out is written only by a call that succeeded)
    if (int r = fold_rows_to_host(ctx, k_pan_moving_reduce, pairs, prow, ctx->pan_host.rows.data(), ctx->pan_moving.p, rows, runs)) return r;
    memcpy(out, ctx->pan_host.rows.data(), (size_t)pairs * sizeof(PanRow));
    return RBF_OK;
}

int rbf_roll_frames(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                    uint32_t width, uint32_t height, uint32_t pixel_bytes, const int32_t *offsets)
{
    if (int r = set_device(ctx)) return r;
    if (width == 0 || height == 0) return fail(RBF_EINVAL, "empty frame %ux%u", width, height);
    if (pixel_bytes < 1 || pixel_bytes > 8) return fail(RBF_EINVAL, "pixel_bytes must be 1..8, got %u", pixel_bytes);
    const uint64_t row_bytes = (uint64_t)width * pixel_bytes, frame_bytes = row_bytes * height;
    if (row_bytes > 0x7FFFFFFFull) return fail(RBF_ERANGE, "a row of %llu bytes is too long", (unsigned long long)row_bytes);
    if (nframes == 0) return RBF_OK;
    if (!frames_dev || !offsets) return fail(RBF_EINVAL, "null pointer");
    if (int r = check_frame_stride(frame_stride_bytes, frame_bytes, nframes, true)) return r;
    const bool vec = !ctx->knobs.force_generic && row_bytes % 16 == 0;
    const uint64_t per_thread = vec ? 16 : 1, bx = (frame_bytes + per_thread * WG_THREADS - 1) / (per_thread * WG_THREADS);
    if (bx > 0x7FFFFFFFull) return fail(RBF_ERANGE, "frame of %llu bytes is too large", (unsigned long long)frame_bytes);
    uint8_t *const frames = (uint8_t *)frames_dev;
    RollJobs jobs{};
    uint32_t cnt = 0;
    auto flush = [&]() -> int {
        if (!cnt) return RBF_OK;
        if (int r = ctx->roll_scratch.reserve((size_t)ROLL_CHUNK * frame_bytes)) return r;
        const dim3 grid((uint32_t)bx, cnt), block(WG_THREADS);
        if (vec)
            hipLaunchKernelGGL(k_roll_frames, grid, block, 0, ctx->stream, frames, frame_stride_bytes, (uint32_t)row_bytes, height, pixel_bytes, jobs, ctx->roll_scratch.p, frame_bytes);
        else
            hipLaunchKernelGGL(k_roll_frames_bytes, grid, block, 0, ctx->stream, frames, frame_stride_bytes, (uint32_t)row_bytes, height, pixel_bytes, jobs, ctx->roll_scratch.p, frame_bytes);
        HIP_TRY(hipGetLastError());
        for (uint32_t j = 0; j < cnt;) {                          // back into the block: frames that follow each other without a gap in one copy
            uint32_t e = j + 1;
            while (e < cnt && jobs.frame[e] == jobs.frame[e - 1] + 1 && frame_stride_bytes == frame_bytes) ++e;
            HIP_TRY(hipMemcpyAsync(frames + (uint64_t)jobs.frame[j] * frame_stride_bytes, ctx->roll_scratch.p + (uint64_t)j * frame_bytes,
                                   (size_t)(e - j) * frame_bytes, hipMemcpyDeviceToDevice, ctx->stream));
            j = e;
        }
        cnt = 0;
        return RBF_OK;
    };
    for (uint32_t f = 0; f < nframes; ++f) {
        const int64_t ox = ((int64_t)offsets[2 * f] % (int64_t)width + width) % width, oy = ((int64_t)offsets[2 * f + 1] % (int64_t)height + height) % height;
        if (!ox && !oy) continue;                                 // neither read nor written
        jobs.frame[cnt] = f; jobs.ox[cnt] = (uint32_t)ox; jobs.oy[cnt] = (uint32_t)oy;
        if (++cnt == ROLL_CHUNK)
            if (int r = flush()) return r;
    }
    return flush();
}

// ---- views: a region of the listed frames of a resident block, reduced by a box mean (rbf_view.h, rbf_kernels_view.h); read-only on
// the frames, nothing is written by a call that is refused
int rbf_frame_view_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                         const uint32_t *frame_index, uint32_t count,
                         uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                         uint32_t x0, uint32_t y0, uint32_t roi_w, uint32_t roi_h, uint32_t scale,
                         void *out_dev, uint64_t capacity_bytes)
{
    if (int r = set_device(ctx)) return r;
    const PackedBlock blk{width, height, channels, sample_bytes, frame_stride_bytes};
    const uint32_t pixel = blk.pixel();
    if (int r = check_block_shape(blk, count)) return r;
    if (!view_scale_ok(scale)) return fail(RBF_EINVAL, "scale must be 1, 2, 4 or 8, got %u", scale);
    if (roi_w == 0 || roi_h == 0) return fail(RBF_EINVAL, "empty region %ux%u", roi_w, roi_h);
    if ((uint64_t)x0 + roi_w > width || (uint64_t)y0 + roi_h > height)
        return fail(RBF_EINVAL, "region %ux%u at (%u, %u) leaves a frame of %ux%u", roi_w, roi_h, x0, y0, width, height);
    if (count == 0) return RBF_OK;
    if (!frames_dev || !frame_index || !out_dev) return fail(RBF_EINVAL, "null pointer");
    if ((uintptr_t)frames_dev % sample_bytes || (uintptr_t)out_dev % sample_bytes)
        return fail(RBF_EINVAL, "frames or views misaligned for %u-byte samples", sample_bytes);
    const uint64_t n = blk.n(), frame_bytes = blk.frame_bytes();
    if (frame_bytes / pixel != n || frame_bytes >> 48) return fail(RBF_ERANGE, "frame of %llu pixels is too large", (unsigned long long)n);
    if ((uint64_t)width * pixel > 0x7FFFFFFFull) return fail(RBF_ERANGE, "a row of %llu bytes is too long", (unsigned long long)width * pixel);
    if (int r = check_frame_stride(frame_stride_bytes, frame_bytes, count, false)) return r;
    for (uint32_t i = 1; i < count; ++i)
        if (frame_index[i] <= frame_index[i - 1])                 // (a frame listed twice would be viewed twice: ask for it once)
            return fail(RBF_EINVAL, "frame indices must ascend: %u after %u", frame_index[i], frame_index[i - 1]);
    const uint32_t last = frame_index[count - 1];
    if (frame_stride_bytes >> 48 || (uint64_t)last * frame_stride_bytes >> 62) return fail(RBF_ERANGE, "frame %u at stride %llu is out of reach", last, (unsigned long long)frame_stride_bytes);
    const bool aligned16 = !ctx->knobs.force_generic && lanes_aligned(16, (uintptr_t)frames_dev, frame_stride_bytes);
    const ViewPlan p = view_plan(width, pixel, x0, roi_w, roi_h, scale, aligned16);
    const uint64_t view_bytes = (uint64_t)p.out_w * p.out_h * pixel, need = view_bytes * count;
    if (capacity_bytes < need)
        return fail(RBF_EINVAL, "%u views of %llu bytes need %llu bytes, capacity is %llu", count, (unsigned long long)view_bytes, (unsigned long long)need,
                    (unsigned long long)capacity_bytes);
    const uintptr_t src_lo = (uintptr_t)frames_dev, src_hi = src_lo + (uint64_t)last * frame_stride_bytes + frame_bytes;      // the source span
    const uintptr_t out_lo = (uintptr_t)out_dev, out_hi = out_lo + need;
    if (out_lo < src_hi && src_lo < out_hi) return fail(RBF_EINVAL, "out_dev lies inside the source span: a view is never written over the frames");
    // what the wide kernel leaves: the columns behind its last whole tile (beside its rows), and the rows below them (whole rows)
    const uint32_t rects[2][4] = {{p.wide_cols, 0, p.out_w - p.wide_cols, p.wide_rows}, {0, p.wide_rows, p.out_w, p.out_h - p.wide_rows}};
    const uint64_t wide_lanes = (uint64_t)p.tiles_x * p.wide_rows, bx_wide = (wide_lanes + WG_THREADS - 1) / WG_THREADS;
    uint64_t bx_px[2];
    for (int r = 0; r < 2; ++r) bx_px[r] = ((uint64_t)rects[r][2] * rects[r][3] * channels + WG_THREADS - 1) / WG_THREADS;
    if (bx_wide > 0x7FFFFFFFull || bx_px[0] > 0x7FFFFFFFull || bx_px[1] > 0x7FFFFFFFull)
        return fail(RBF_ERANGE, "view of %ux%u pixels is too large", p.out_w, p.out_h);
    if (int r = ctx->view_index.reserve((size_t)count * 4)) return r;
    HIP_TRY(hipMemcpyAsync(ctx->view_index.p, frame_index, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));      // (pageable: staged before the call returns)
    const uint8_t *const frames = (const uint8_t *)frames_dev;
    const uint32_t row_bytes = (uint32_t)(width * pixel), out_row_bytes = p.out_w * pixel;
    const uint64_t roi_off = ((uint64_t)y0 * width + x0) * pixel;
    constexpr uint32_t MAX_Y = 65535;                             // frames of one launch (gridDim.y)
    for (uint32_t f0 = 0; f0 < count; f0 += MAX_Y) {
        const uint32_t cnt = count - f0 < MAX_Y ? count - f0 : MAX_Y;
        const uint32_t *const index = ctx->view_index.p + f0;
        uint8_t *const out = (uint8_t *)out_dev + (uint64_t)f0 * view_bytes;
        if (bx_wide)
            by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) {
                by_value<1, 2, 4, 8>(scale, [&](auto k) {
                    hipLaunchKernelGGL((k_frame_view<decltype(s), decltype(c)::value, decltype(k)::value>), dim3((uint32_t)bx_wide, cnt), dim3(WG_THREADS), 0,
                                       ctx->stream, frames, frame_stride_bytes, index, row_bytes, roi_off, p.tiles_x, p.wide_rows, out, view_bytes, out_row_bytes);
                });
            });
        for (int r = 0; r < 2; ++r) {
            if (!bx_px[r]) continue;
            const uint32_t *const q = rects[r];
            by_sample_width(sample_bytes, [&](auto s) {
                by_value<1, 2, 4, 8>(scale, [&](auto k) {
                    hipLaunchKernelGGL((k_frame_view_px<decltype(s), decltype(k)::value>), dim3((uint32_t)bx_px[r], cnt), dim3(WG_THREADS), 0, ctx->stream, frames,
                                       frame_stride_bytes, index, width, channels, x0, y0, roi_w, roi_h, p.out_w, q[0], q[1], q[2], q[3], out, view_bytes);
                });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

// ---- integrity: FD1 frame digests (rbf_digest.h, rbf_kernels_digest.h)
int rbf_frame_digest_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint64_t frame_bytes, uint64_t *digests_dev)
{
    if (int r = set_device(ctx)) return r;
    if (nframes == 0) return RBF_OK;
    if (frame_bytes == 0) return fail(RBF_EINVAL, "frame_bytes must be >= 1: an empty frame has no resident bytes to hash");
    if (!frames_dev || !digests_dev) return fail(RBF_EINVAL, "null device pointer");
    if ((uintptr_t)digests_dev % 8) return fail(RBF_EINVAL, "digests_dev must be 8-byte aligned");
    if (int r = check_frame_stride(frame_stride_bytes, frame_bytes, nframes, true)) return r;
    const uint32_t levels = fd1_levels(frame_bytes);
    const uint64_t words = fd1_scratch_words(frame_bytes);
    constexpr uint32_t MAX_Y = 65535;                             // frames of one launch (gridDim.y)
    if (int r = ctx->digest_lvl.reserve((size_t)(nframes < MAX_Y ? nframes : MAX_Y) * words * 8)) return r;
    for (uint32_t f0 = 0; f0 < nframes; f0 += MAX_Y) {
        const uint32_t cnt = nframes - f0 < MAX_Y ? nframes - f0 : MAX_Y;
        const uint8_t *src = (const uint8_t *)frames_dev + (uint64_t)f0 * frame_stride_bytes;
        uint64_t stride = frame_stride_bytes, len = frame_bytes;
        uint64_t *lvl = ctx->digest_lvl.p;                        // level k's hashes: cnt rows of fd1_blocks(len of level k) words
        for (uint32_t k = 0; k <= levels; ++k) {
            const bool top = k == levels;
            const uint64_t nb = fd1_blocks(len);
            uint64_t *dst = top ? digests_dev + f0 : lvl;
            const uint64_t dst_stride = top ? 1 : nb;
            // frames: 16-byte loads where base and stride allow them; the arrays of block hashes are 8-byte aligned: the generic path
            const bool aligned = k == 0 && !ctx->knobs.force_generic && (uintptr_t)src % 16 == 0 && (stride % 16 == 0 || cnt == 1);
            const uint32_t threads = top ? WAVE : WG_THREADS, waves_wg = threads / WAVE;
            uint64_t waves = (nb + FD1_BLOCKS_PER_WAVE - 1) / FD1_BLOCKS_PER_WAVE;
            if (waves > (1u << 20)) waves = 1u << 20;             // (a wave walks its blocks: any count is covered)
            const dim3 grid((uint32_t)((waves + waves_wg - 1) / waves_wg), cnt), block(threads);
            if (aligned)
                hipLaunchKernelGGL(k_frame_digest<true>, grid, block, 0, ctx->stream, src, stride, len, nb, (uint32_t)top, frame_bytes, dst, dst_stride);
            else
                hipLaunchKernelGGL(k_frame_digest<false>, grid, block, 0, ctx->stream, src, stride, len, nb, (uint32_t)top, frame_bytes, dst, dst_stride);
            src = (const uint8_t *)lvl; stride = nb * 8; len = nb * 8;
            lvl += (uint64_t)cnt * nb;
        }
    }
    HIP_TRY(hipGetLastError());
    return RBF_OK;
}

uint64_t rbf_frame_digest_host(const void *bytes, uint64_t nbytes)
{
    try { return fd1_host(bytes, (size_t)nbytes); }               // (the levels live in a std::vector: nothing may throw across the C ABI)
    catch (...) { (void)fail(RBF_ENOMEM, "no host memory for the digest levels of %llu bytes", (unsigned long long)nbytes); return 0; }
}

}  // extern "C"
