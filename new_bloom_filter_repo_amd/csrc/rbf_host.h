// rbf_host.h -- what every entry point of rbf_api.hip stands on: the last-error text, the context and its scratch memory, per-kernel
// timing, the process-wide pixel-index hash table, the Bloom rows' argument checks, and the shared launch helpers: the dispatch on sample type,
// channels and other template constants, the mask counts, the fold-and-fetch tail.  Frame layouts and block arithmetic: rbf_block_plan.h.
#pragma once
#include "rbf_kernels.h"
#include "rbf_kernels_insert_f64.h"
#include "rbf_block_plan.h"
#include "rbf_plan.h"

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                                    \
    do {                                                                                                                 \
        hipError_t e_ = (expr);                                                                                          \
        if (e_ != hipSuccess)                                                                                            \
            return fail(RBF_EIO, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);             \
    } while (0)

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
// Device scratch memory with one owner: grown on demand, never shrunk, freed with the context.  No pool and no cache: a buffer that
// is too small is freed and allocated anew, and its contents are not kept.
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                  // bytes
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    int alloc(size_t bytes)          // exactly `bytes`
    {
        release();
        HIP_TRY(hipMalloc((void **)&p, bytes));
        cap = bytes;
        return RBF_OK;
    }
    int reserve(size_t bytes) { return bytes <= cap ? RBF_OK : alloc(bytes + bytes / 4 + 256); }
};

struct Timed { int id; hipEvent_t a, b; };

// The rows of a batch: masks, filters, witnesses (and, on the encode side, stats).  Encode reads the masks and writes the rest; decode
// reads filters and witnesses and writes the masks.
struct BloomBatch {
    void *masks; uint64_t mask_stride;
    uint64_t n; uint32_t nframes; const rbf_filter_params *params; const rbf_seeds *seeds;
    void *filters; uint64_t filter_stride;
    void *witnesses; uint64_t witness_stride;
    uint64_t *stats;
    // frames first .. first + count - 1
    BloomBatch rows(uint32_t first, uint32_t count) const
    {
        BloomBatch b = *this;
        b.nframes = count; b.params = params + first;
        b.masks = (uint8_t *)masks + (uint64_t)first * mask_stride;
        b.filters = (uint8_t *)filters + (uint64_t)first * filter_stride;
        b.witnesses = (uint8_t *)witnesses + (uint64_t)first * witness_stride;
        if (stats) b.stats = stats + (uint64_t)first * RBF_STATS_PER_FRAME;
        return b;
    }
    BloomBatch with(const rbf_filter_params *other) const { BloomBatch b = *this; b.params = other; return b; }
};

struct rbf_ctx {
    int device = 0;
    uint32_t cus = 256;              // compute units of the device (hipDeviceAttributeMultiprocessorCount; MI355X: 256)
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    Knobs knobs;                     // rbf_ctx_force_generic / rbf_ctx_option
    // scratch
    DevBuf<uint32_t> seg_cnt;
    DevBuf<uint64_t> seg_off;
    DevBuf<uint32_t> chunk_off;      // k_chunk_offsets: where every compaction / expansion workgroup's witness bits start
    DevBuf<uint64_t> pass_words;
    DevBuf<uint32_t> partials;
    DevBuf<uint2> ins_records;       // two-kernel insert: 8 bytes per set mask bit of the batch
    DevBuf<uint32_t> ins_counters;   // ... and the records appended so far, per frame
    DevBuf<uint64_t> ones_acc;       // where the mask kernels count; k_finish_ones hands the counts out and re-zeroes it
    bool ones_acc_dirty = false;     // a call failed between the mask kernels and k_finish_ones
    DevBuf<uint32_t> mask_ticket;    // the fused tail of the GOP mask kernel: workgroups done so far (zero between launches)
    DevBuf<uint32_t> qimage;         // probe image of the batch's filters (FP64 query kernel)
    DevBuf<int32_t> thr_tab;         // per-pair thresholds of the mask kernels
    DevBuf<uint64_t> pack_base;      // running record size between pack chunks; per-row totals of count_and_scan_masks
    // sample codec (rbf_kernels_rice.h)
    DevBuf<uint16_t> rice_u;         // u values (encode) / s values (decode) of the call's streams
    DevBuf<uint32_t> rice_kw;        // per chunk: k | words << 8
    DevBuf<uint64_t> rice_off;       // per chunk: payload word offset (+ the total), then per stream
    DevBuf<void> rice_tab;           // the call's stream / chunk table
    DevBuf<void> rice_blob;          // uploaded streams (decode)
    DevBuf<uint32_t> rice_err;       // decode / apply error flag
    DevBuf<uint32_t> keyq;           // bounded-error keyframes (rbf_kernels_keyquant.h): the call's frame indices
    DevBuf<uint8_t> hold_bits;       // look-ahead hold (rbf_kernels_lookahead.h): the segment-start bits, nframes rows of ceil(n / 8) bytes
    DevBuf<uint64_t> digest_lvl;     // frame digests (rbf_kernels_digest.h): the block hashes of every level, per frame of the call
    DevBuf<uint32_t> cut_partials;   // scene-cut statistics (rbf_kernels_cut.h): three sums per wave and pair of the call
    DevBuf<uint32_t> err_partials;   // quality report (rbf_kernels_error.h): six words per wave and frame of the call
    DevBuf<void> err_rows;           // ... and the folded rows (rbf_error_row), a frame each, on their way to the host
    DevBuf<uint32_t> sweep_partials; // hold sweep (rbf_kernels_sweep.h): four words per wave, run and candidate of the call
    DevBuf<void> sweep_rows;         // ... and the folded rows (rbf_sweep_row), a (run, candidate) each, on their way to the host
    DevBuf<uint32_t> pan_partials;   // pan search (rbf_kernels_pan.h): (2R+1)^2 sums per tile and pair of the call
    DevBuf<uint32_t> pan_moving;     // ... two counts per wave and pair
    DevBuf<void> pan_rows;           // ... the folded rows (rbf_pan_stat), a pair each: the pick's shift stays here for the moving kernel
    DevBuf<uint8_t> pan_runs;        // ... the call's run starts, a byte per frame
    struct PanHost {                 // ... and the rows on their way to the caller's array
        std::vector<rbf_pan_stat> rows;
        int reserve_rows(size_t n) { try { if (rows.size() < n) rows.resize(n); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); } return RBF_OK; }
    } pan_host;
    DevBuf<uint8_t> roll_scratch;    // rbf_roll_frames: where a chunk of up to eight frames is rolled to before it is copied back
    DevBuf<uint32_t> view_index;     // rbf_frame_view_batch (rbf_kernels_view.h): the call's frame indices
    struct SharedHashTable *hash_shared = nullptr;               // the pixel-index hash table this context holds a reference to
    uint4 *hash_tab = nullptr;                                    // = hash_shared->table
    // host staging of encode_gop: device-visible pinned block [flag | ones...] the GPU publishes into
    uint64_t *ones_pinned = nullptr; size_t host_cap = 0;
    uint64_t *ones_mapped_dev = nullptr;     // device address of the same block
    uint64_t publish_token = 0;
    struct PendingGop {                      // between rbf_encode_gop_begin and rbf_encode_gop_finish
        bool active = false;
        uint64_t token = 0; rbf_seeds seeds{};
        BloomBatch batch{};                      // the caller's buffers; params and seeds are set by the second half
        bool has_skip = false;                   // ctx->run_skip[p] != 0: pair p crosses a keyframe and is not coded
    } gop;
    std::vector<uint8_t> run_skip;
    std::vector<rbf_filter_params> plan;
    std::vector<double> plan_k;
    // timing
    uint32_t timing = 0;             // bit k: bracket launches of kernel id k with HIP events
    std::vector<Timed> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[RBF_K_COUNT] = {0};
    uint64_t launches[RBF_K_COUNT] = {0};

    ~rbf_ctx() { if (ones_pinned) (void)hipHostFree(ones_pinned); }     // (the DevBuf members free themselves)
};

// Every entry point starts here.
static int set_device(rbf_ctx *ctx)
{
    if (!ctx) return fail(RBF_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return RBF_OK;
}

struct LaunchTimer {
    rbf_ctx *c; int id; hipEvent_t a = nullptr, b = nullptr; bool on; hipStream_t st;
    LaunchTimer(rbf_ctx *ctx, int kid /* < 0: never timed */) : c(ctx), id(kid), on(kid >= 0 && ((ctx->timing >> kid) & 1u)), st(ctx->stream)
    {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!c->pool.empty()) { e = c->pool.back(); c->pool.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
            return e;
        };
        a = get(); b = get();
        if (!a || !b) { on = false; return; }
        (void)hipEventRecord(a, st);
    }
    ~LaunchTimer()
    {
        if (!on) return;
        (void)hipEventRecord(b, st);
        try { c->pending.push_back({id, a, b}); }                 // timing is best effort; nothing may throw across the C ABI
        catch (...) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    }
};

static int drain_timing(rbf_ctx *ctx)
{
    if (ctx->pending.empty()) return RBF_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (auto &t : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            ctx->total_ms[t.id] += ms;
            ctx->launches[t.id] += 1;
        }
        try { ctx->pool.push_back(t.a); } catch (...) { (void)hipEventDestroy(t.a); }
        try { ctx->pool.push_back(t.b); } catch (...) { (void)hipEventDestroy(t.b); }
    }
    ctx->pending.clear();
    return RBF_OK;
}

static int allow_big_lds(const void *fn)
{
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
    return RBF_OK;
}

static inline Seeds to_dev(const rbf_seeds &s) { return Seeds{s.h1, s.h2, s.act}; }
template <class A, class B> static inline bool same_seeds(const A &a, const B &b) { return a.h1 == b.h1 && a.h2 == b.h2 && a.act == b.act; }

// ------------------------------------------------------------------------------------------
// The pixel-index hash table (k_hash_table, 26 bytes per pixel inside an allocation of 32: rbf_f64_common.h) depends on the
// device, the frame size and the seeds only, so the contexts of one process SHARE it: four pipelines coding 1080p GOPs gather from
// one 54 MB table that the 256 MB Infinity Cache can keep, instead of four private ones that it cannot (measured: 0.197 -> 0.18x ms
// per step).  Built once by the first context that needs it (on its stream; the others make their streams wait for the `ready`
// event), freed when the last reference goes.
// ------------------------------------------------------------------------------------------
struct SharedHashTable {
    int device; uint64_t n; rbf_seeds seeds;
    uint4 *table; size_t bytes;
    hipEvent_t ready;
    int refs;
    bool is_for(int dev, uint64_t pixels, const rbf_seeds &s) const { return device == dev && n == pixels && same_seeds(seeds, s); }
};
static std::mutex g_hash_mu;
static std::vector<SharedHashTable *> g_hash_tables;

static void hash_table_free(SharedHashTable *t)
{
    if (t->ready) (void)hipEventDestroy(t->ready);
    (void)hipFree(t->table);
    delete t;
}

static void hash_table_release(rbf_ctx *ctx)
{
    SharedHashTable *t = ctx->hash_shared;
    if (!t) return;
    (void)hipStreamSynchronize(ctx->stream);                      // my kernels no longer read it
    ctx->hash_shared = nullptr; ctx->hash_tab = nullptr;
    std::lock_guard<std::mutex> lk(g_hash_mu);
    if (--t->refs > 0) return;
    for (size_t i = 0; i < g_hash_tables.size(); ++i)
        if (g_hash_tables[i] == t) { g_hash_tables[i] = g_hash_tables.back(); g_hash_tables.pop_back(); break; }
    hash_table_free(t);
}

static void launch_hash_table(rbf_ctx *ctx, uint64_t n, const Seeds &sd, uint4 *table)
{
    const uint64_t segs = (n + QL_SEG_PIXELS - 1) / QL_SEG_PIXELS;
    LaunchTimer timer(ctx, RBF_K_HASHTAB);
    hipLaunchKernelGGL(k_hash_table, dim3((uint32_t)((segs + HT_THREADS / WAVE - 1) / (HT_THREADS / WAVE))), dim3(HT_THREADS), 0,
                       ctx->stream, n, sd, table);
}

// The table of (ctx->device, n, seeds) in ctx->hash_tab, built if nobody has it yet (*built).  false: no device memory (the caller
// hashes in the insert kernel instead).
static bool hash_table_acquire(rbf_ctx *ctx, uint64_t n, const rbf_seeds &seeds, bool *built)
{
    *built = false;
    if (ctx->hash_shared && ctx->hash_shared->is_for(ctx->device, n, seeds)) return true;
    hash_table_release(ctx);
    std::lock_guard<std::mutex> lk(g_hash_mu);
    for (SharedHashTable *t : g_hash_tables)
        if (t->is_for(ctx->device, n, seeds)) {
            if (hipStreamWaitEvent(ctx->stream, t->ready, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
            ++t->refs;
            ctx->hash_shared = t; ctx->hash_tab = t->table;
            return true;
        }
    SharedHashTable *t = new (std::nothrow) SharedHashTable{ctx->device, n, seeds, nullptr, hash_table_bytes(n), nullptr, 1};
    if (!t) return false;
    if (hipMalloc((void **)&t->table, t->bytes) != hipSuccess || hipEventCreateWithFlags(&t->ready, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        hash_table_free(t);
        return false;
    }
    launch_hash_table(ctx, n, to_dev(seeds), t->table);
    // a table whose kernel never ran must not be published to the other contexts of the process
    bool ok = hipGetLastError() == hipSuccess && hipEventRecord(t->ready, ctx->stream) == hipSuccess;
    if (ok) try { g_hash_tables.push_back(t); } catch (...) { ok = false; }
    if (!ok) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        hash_table_free(t);
        return false;
    }
    ctx->hash_shared = t; ctx->hash_tab = t->table;
    *built = true;
    return true;
}

// ------------------------------------------------------------------------------------------
// shared argument checks
// ------------------------------------------------------------------------------------------
static int check_frame_geometry(uint64_t n, uint32_t nframes, uint64_t mask_stride_bytes)
{
    if (n == 0 || n > 0xFFFFFFFFull) return fail(RBF_ERANGE, "n = %llu outside [1, 2^32-1]", (unsigned long long)n);
    if (nframes == 0) return fail(RBF_EINVAL, "nframes must be >= 1");
    if (mask_stride_bytes % 8 || mask_stride_bytes < ((n + 63) / 64) * 8)
        return fail(RBF_EINVAL, "mask stride %llu must be a multiple of 8 and >= %llu", (unsigned long long)mask_stride_bytes,
                    (unsigned long long)(((n + 63) / 64) * 8));
    return RBF_OK;
}

// A base the kernels address as 64-bit words: rows of packed bits (masks, filters, witnesses), the stats rows and the ones counts.
static int check_base8(const void *p, const char *name)
{
    if ((uintptr_t)p % 8) return fail(RBF_EINVAL, "%s must be 8-byte aligned", name);
    return RBF_OK;
}

static int check_witness_stride(uint64_t n, uint64_t witness_stride_bytes)
{
    if (witness_stride_bytes % 8 || witness_stride_bytes < ((n + 63) / 64) * 8) return fail(RBF_EINVAL, "witness stride too small or misaligned");
    return RBF_OK;
}

// ------------------------------------------------------------------------------------------
// shared launches
// ------------------------------------------------------------------------------------------
// Calls f with a zero of the sample type, so that a launch templated on it names its argument list once:
//   by_sample_width(sample_bytes, [&](auto s) { hipLaunchKernelGGL(k_x<decltype(s)>, ...); });
template <class F> static void by_sample_width(uint32_t sample_bytes, F &&f)
{
    if (sample_bytes == 1) f(uint8_t{});
    else f(uint16_t{});
}

// Calls f with v as a compile-time constant, v being V or one of Vs; the last of them takes every other v, as the else of an if-ladder does:
//   by_value<1, 2, 4, 8>(scale, [&](auto k) { hipLaunchKernelGGL((k_x<decltype(k)::value>), ...); });
template <uint32_t V, uint32_t... Vs, class F> static void by_value(uint32_t v, F &&f)
{
    if constexpr (sizeof...(Vs) > 0) { if (v != V) return by_value<Vs...>(v, f); }
    f(std::integral_constant<uint32_t, V>{});
}

// ... and with the sample type and the channel count (1..4), what the lane kernels are templated on:
//   by_sample_and_channels(sample_bytes, channels, [&](auto s, auto c) { hipLaunchKernelGGL((k_x<decltype(s), decltype(c)::value>), ...); });
template <class F> static void by_sample_and_channels(uint32_t sample_bytes, uint32_t channels, F &&f)
{
    by_sample_width(sample_bytes, [&](auto s) { by_value<1, 2, 3, 4>(channels, [&](auto c) { f(s, c); }); });
}

// The end of a stage that reports to the host: `fold`, a workgroup per row, folds the stage's partial sums into `count` rows on the device
// (fold(args..., rows_dev)); they are copied to rows_host, and the call waits for them.
template <class Row, class Kernel, class... Args> static int fold_rows_to_host(rbf_ctx *ctx, Kernel fold, uint32_t count, Row *rows_dev, void *rows_host, Args... args)
{
    hipLaunchKernelGGL(fold, dim3(count), dim3(WG_THREADS), 0, ctx->stream, args..., rows_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rows_host, rows_dev, (size_t)count * sizeof(Row), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RBF_OK;
}

// The set bits of `rows` mask rows of n pixels per 1024-pixel segment (ctx->seg_cnt), their exclusive scan per row (ctx->seg_off)
// and every row's total (totals_out, nullable).
static int count_and_scan_masks(rbf_ctx *ctx, const void *masks_dev, uint64_t mask_stride_bytes, uint64_t n, uint32_t rows, uint64_t *totals_out)
{
    const uint64_t nseg = (n + SEG_PIXELS - 1) / SEG_PIXELS;
    if (int r = ctx->seg_cnt.reserve((size_t)rows * nseg * 4)) return r;
    if (int r = ctx->seg_off.reserve((size_t)rows * nseg * 8)) return r;
    hipLaunchKernelGGL(k_mask_segment_counts, dim3((uint32_t)((nseg + WG_WAVES - 1) / WG_WAVES), rows), dim3(WG_THREADS), 0, ctx->stream,
                       (const uint64_t *)masks_dev, mask_stride_bytes / 8, n, ctx->seg_cnt.p, nseg);
    hipLaunchKernelGGL(k_scan_segments, dim3(rows), dim3(1024), 0, ctx->stream, ctx->seg_cnt.p, ctx->seg_off.p, nseg, totals_out, 1u);
    return RBF_OK;
}
