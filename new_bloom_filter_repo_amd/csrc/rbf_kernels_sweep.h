// rbf_kernels_sweep.h -- the hold sweep: what EVERY candidate bound would do to EVERY run of a block, in one read of the block
// (k_hold_sweep over workgroup tiles staged in LDS, its per-pixel twin k_hold_sweep_px for what the tiles do not cover, and
// k_sweep_reduce).  include/rbf.h (rbf_hold_sweep) has the normative text.  For run r and candidate e, with Y the block that
// k_temporal_hold (rbf_kernels_hold.h; LA = false) or k_temporal_lookahead + k_lookahead_fill (rbf_kernels_lookahead.h; LA = true) would
// leave with max_error = e:
//   sse     = sum of (x - y)^2 over every sample of the run's frames (the run's first frame is exact)
//   updates = (pixel, frame) pairs with y_t != y_{t-1}: the run's all-channel mask counts
//   max_abs = the largest |x - y|
// Nothing is written to the block.  A lane owns ONE pixel of one run (blockIdx.y) and walks the run's frames forward once with the
// state of up to SWEEP_GROUP = 4 candidates in registers; a call with more candidates splits them into two groups, and the two halves
// of a workgroup walk the SAME tile of pixels, one group each, so a frame's tile is still fetched once:
//   tile = WG_THREADS / groups pixels (256, or 128 with two groups), tile * PIXEL_BYTES contiguous bytes of a frame -- always whole
//   16-byte vectors -- which the workgroup's first threads load as uint4 (coalesced, one load per thread and frame at the most, the next
//   frame's in flight) into one of two LDS buffers; one barrier per frame; a lane then reads its pixel's samples from LDS.
// First-value rule: the state of a candidate is the held pixel.  Look-ahead rule: lo, hi and prev of rbf_kernels_lookahead.h; a segment's
// value v is known only when it closes, so the lane also keeps, per sample, the segment's first sample `ref` and of d = x - ref its sum
// S1, its sum of squares S2, its min and its max, and the segment's length n.  Every sample of a segment lies in a window of width 2e
// around v, so |d| <= 2e <= 510 and with n <= 128 frames: |S1| <= 65280, S2 <= 33.3e6 -- 32 bits with room.  On close, with w = v - ref:
//   sse += S2 - 2 w S1 + n w^2      max_abs = max(max_abs, dmax - w, w - dmin)
// (tests/test_hold_sweep_cpu.py holds this closed form against the holds themselves.)  The anchored segment is the free one with
// lo = hi = ref = x_0.  |x - y| <= e <= 255, so a lane's sse of a run is <= 127 * 4 * 255^2 = 33.0e6 and a wave's fits 32 bits.
// No atomics: a wave writes the sums of each of its candidates to a row of its own (every row a call reads is written by that call),
// k_sweep_reduce folds a (run, candidate)'s rows -- integer sums and a max, the result is deterministic.
#pragma once
#include "rbf_kernels_error.h"

#include <type_traits>

namespace rbf {

constexpr uint32_t SWEEP_MAX_CANDIDATES = 8, SWEEP_GROUP = 4, SWEEP_WORDS = 4, SWEEP_MAX_RUN = 128;     // a wave's row: sse, updates, max_abs, 0

struct SweepRow {                                                          // = rbf_sweep_row (include/rbf.h)
    uint64_t sse, updates;
    uint32_t max_abs, reserved;
};

// One candidate of one pixel under the first-value rule.  C: the samples of a pixel (the per-pixel kernel: 4, with zeros for those a pixel lacks).
template <int C> struct SweepFirst {
    uint32_t held[C];
    uint32_t sse = 0, updates = 0, worst = 0;
    __device__ __forceinline__ void init(const uint32_t *x)
    {
#pragma unroll
        for (int c = 0; c < C; ++c) held[c] = x[c];
    }
    __device__ __forceinline__ void step(const uint32_t *x, uint32_t e)
    {
        uint32_t w = 0, sq = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t d = __usad(x[c], held[c], 0u);
            w = max(w, d);
            sq += d * d;                                                   // (used only while every d <= e <= 255)
        }
        const bool upd = w > e;
        updates += upd ? 1u : 0u;
        sse += upd ? 0u : sq;
        worst = max(worst, upd ? 0u : w);
#pragma unroll
        for (int c = 0; c < C; ++c) held[c] = upd ? x[c] : held[c];
    }
};

// One candidate of one pixel under the look-ahead rule (see the file comment).  M: the sample type's largest value.
template <int C> struct SweepLook {
    int32_t lo[C], hi[C], prev[C], ref[C], s1[C], dmin[C], dmax[C];
    uint32_t s2[C], n = 1;
    uint32_t sse = 0, updates = 0, worst = 0;
    __device__ __forceinline__ void init(const uint32_t *x)
    {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            lo[c] = hi[c] = prev[c] = ref[c] = (int32_t)x[c];
            s1[c] = dmin[c] = dmax[c] = 0; s2[c] = 0;
        }
    }
    // the open segment ends: its value is clamp(prev, lo, hi), which becomes prev
    __device__ __forceinline__ void close()
    {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int32_t v = min(max(prev[c], lo[c]), hi[c]), w = v - ref[c];
            sse += (uint32_t)((int32_t)s2[c] - 2 * w * s1[c] + (int32_t)n * w * w);
            worst = max(worst, (uint32_t)max(dmax[c] - w, w - dmin[c]));
            prev[c] = v;
        }
    }
    __device__ __forceinline__ void step(const uint32_t *x, uint32_t e, int32_t M)
    {
        int32_t xl[C], xh[C];
        bool empty = false;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xl[c] = max(0, (int32_t)x[c] - (int32_t)e);
            xh[c] = min(M, (int32_t)x[c] + (int32_t)e);
            empty |= max(lo[c], xl[c]) > min(hi[c], xh[c]);
        }
        if (empty) {
            close();
            updates += 1;
        }
        n = empty ? 1u : n + 1;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ref[c] = empty ? (int32_t)x[c] : ref[c];
            const int32_t d = (int32_t)x[c] - ref[c];
            lo[c] = empty ? xl[c] : max(lo[c], xl[c]);
            hi[c] = empty ? xh[c] : min(hi[c], xh[c]);
            s1[c] = empty ? 0 : s1[c] + d;
            s2[c] = empty ? 0u : s2[c] + (uint32_t)(d * d);
            dmin[c] = empty ? 0 : min(dmin[c], d);
            dmax[c] = empty ? 0 : max(dmax[c], d);
        }
    }
};

// candidate i of the call: a byte of `cands` (candidates are <= 255, eight of them fill the 64 bits)
__device__ __forceinline__ uint32_t sweep_candidate(uint64_t cands, uint32_t i) { return (uint32_t)(cands >> (8 * i)) & 0xFFu; }

// A wave's sums of candidate `cand` of run `run` into its row: partials[((run * ncand + cand) * rows + row) * 4 ..].  Every lane of the
// wave calls this; lane 63 stores, if the candidate exists.
__device__ __forceinline__ void sweep_wave_store(uint32_t *__restrict__ partials, uint64_t rows, uint64_t row, uint32_t run, uint32_t ncand,
                                                 uint32_t cand, uint32_t sse, uint32_t updates, uint32_t worst)
{
    sse = wave_sum_to_lane63(sse);
    updates = wave_sum_to_lane63(updates);
    worst = wave_max_to_lane63(worst);
    if ((threadIdx.x & 63u) == 63u && cand < ncand) {
        uint32_t *out = partials + (((uint64_t)run * ncand + cand) * rows + row) * SWEEP_WORDS;
        out[0] = sse; out[1] = updates; out[2] = worst; out[3] = 0;
    }
}

// The walk of one lane: NEXT(i, x) gives the samples of the lane's pixel in frame f0 + i.  Candidates g0 .. g0 + 3 (those at or past
// ncand repeat the last one and are not stored).
template <typename SAMPLE, int C, bool LA, class State, class Next>
__device__ __forceinline__ void sweep_walk(State *st, uint32_t len, bool active, uint64_t cands, uint32_t ncand, uint32_t g0, Next &&next)
{
    constexpr int32_t M = sizeof(SAMPLE) == 2 ? 0xFFFF : 0xFF;
    uint32_t e[SWEEP_GROUP];
#pragma unroll
    for (uint32_t j = 0; j < SWEEP_GROUP; ++j) e[j] = sweep_candidate(cands, min(g0 + j, ncand - 1));
    uint32_t x[C];
    next(0u, x);
    if (active) {
#pragma unroll
        for (uint32_t j = 0; j < SWEEP_GROUP; ++j) st[j].init(x);
    }
    for (uint32_t i = 1; i < len; ++i) {
        next(i, x);
        if (active) {
#pragma unroll
            for (uint32_t j = 0; j < SWEEP_GROUP; ++j) {
                if constexpr (LA) st[j].step(x, e[j], M);
                else st[j].step(x, e[j]);
            }
        }
    }
    if constexpr (LA) {                                                    // the run's end ends every pixel's last segment
        if (active && len > 1) {
#pragma unroll
            for (uint32_t j = 0; j < SWEEP_GROUP; ++j) st[j].close();
        }
    }
}

// The tiles.  groups = 1: the workgroup's 256 threads own 256 consecutive pixels (blockIdx.x * 256 ..) and candidates 0..3; groups = 2:
// threads t and t + 128 own pixel blockIdx.x * 128 + t, candidates 0..3 and 4..7.  Requires frames and frame_stride to be multiples of
// 16 and gridDim.x * tile <= pixels of a frame: every lane has a pixel, nobody leaves before the last barrier.  Plain loads.
template <typename SAMPLE, int C, bool LA>
__global__ __launch_bounds__(WG_THREADS) void k_hold_sweep(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t groups,
                                                           uint64_t cands, uint32_t ncand, uint32_t *__restrict__ partials, uint64_t rows,
                                                           const HoldRuns runs)
{
    constexpr uint32_t PB = C * (uint32_t)sizeof(SAMPLE);
    __shared__ uint4 stage[2][WG_THREADS * PB / 16];
    const uint32_t tile = WG_THREADS / groups, k = threadIdx.x & (tile - 1), g = threadIdx.x >= tile ? 1u : 0u;
    const uint32_t nvec = tile * PB / 16;
    const uint32_t f0 = runs.first[blockIdx.y], len = runs.len[blockIdx.y];
    const uint8_t *const p = frames + (uint64_t)f0 * frame_stride + (uint64_t)blockIdx.x * tile * PB;
    const bool loader = threadIdx.x < nvec;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (loader) v = reinterpret_cast<const uint4 *>(p)[threadIdx.x];
    auto next = [&](uint32_t i, uint32_t *x) {
        if (loader) stage[i & 1][threadIdx.x] = v;                       // (the buffer's readers of frame i - 2 have passed frame i - 1's barrier)
        if (loader && i + 1 < len) v = reinterpret_cast<const uint4 *>(p + (uint64_t)(i + 1) * frame_stride)[threadIdx.x];
        __syncthreads();
        const SAMPLE *s = reinterpret_cast<const SAMPLE *>(stage[i & 1]) + k * C;
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = s[c];
    };
    const uint64_t row = (uint64_t)blockIdx.x * (tile / WAVE) + (k >> 6);
    using State = typename std::conditional<LA, SweepLook<C>, SweepFirst<C>>::type;
    State st[SWEEP_GROUP];
    sweep_walk<SAMPLE, C, LA>(st, len, true, cands, ncand, g * SWEEP_GROUP, next);
#pragma unroll
    for (uint32_t j = 0; j < SWEEP_GROUP; ++j)
        sweep_wave_store(partials, rows, row, blockIdx.y, ncand, g * SWEEP_GROUP + j, st[j].sse, st[j].updates, st[j].worst);
}

// The plain path: the same split of a workgroup, but a lane reads its pixel (first_pixel + its index, below n) sample by sample from
// memory, so neither the frames' base nor their stride need more than the samples' own alignment.  Covers the tail of a frame behind the
// tiles and whole frames of a layout the tiles do not take.  Its waves' rows follow the tiles' (row0).
template <typename SAMPLE, bool LA>
__global__ __launch_bounds__(WG_THREADS) void k_hold_sweep_px(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t first_pixel,
                                                              uint64_t n, uint32_t channels, uint32_t groups, uint64_t cands, uint32_t ncand,
                                                              uint32_t *__restrict__ partials, uint64_t rows, uint64_t row0, const HoldRuns runs)
{
    const uint32_t tile = WG_THREADS / groups, k = threadIdx.x & (tile - 1), g = threadIdx.x >= tile ? 1u : 0u;
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * tile + k;
    const bool active = px < n;
    const uint32_t f0 = runs.first[blockIdx.y], len = runs.len[blockIdx.y];
    const uint8_t *const p = frames + (uint64_t)f0 * frame_stride + px * channels * sizeof(SAMPLE);
    auto next = [&](uint32_t i, uint32_t *x) {                             // (loops of four with `c < channels` inside: the arrays stay in registers)
        const SAMPLE *s = reinterpret_cast<const SAMPLE *>(p + (uint64_t)i * frame_stride);
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) x[c] = active && c < channels ? (uint32_t)s[c] : 0u;
    };
    const uint64_t row = row0 + (uint64_t)blockIdx.x * (tile / WAVE) + (k >> 6);
    using State = typename std::conditional<LA, SweepLook<4>, SweepFirst<4>>::type;
    State st[SWEEP_GROUP];
    sweep_walk<SAMPLE, 4, LA>(st, len, active, cands, ncand, g * SWEEP_GROUP, next);
#pragma unroll
    for (uint32_t j = 0; j < SWEEP_GROUP; ++j)
        sweep_wave_store(partials, rows, row, blockIdx.y, ncand, g * SWEEP_GROUP + j, st[j].sse, st[j].updates, st[j].worst);
}

// out[run * ncand + cand] = the fold of that (run, candidate)'s rows: one workgroup each (blockIdx.x).
__global__ __launch_bounds__(WG_THREADS) void k_sweep_reduce(const uint32_t *__restrict__ partials, uint64_t rows, SweepRow *__restrict__ out)
{
    __shared__ uint64_t part[2][WG_THREADS];
    __shared__ uint32_t worst[WG_THREADS];
    const uint32_t *in = partials + (uint64_t)blockIdx.x * rows * SWEEP_WORDS;
    uint64_t acc[2] = {0, 0};
    uint32_t w = 0;
    for (uint64_t r = threadIdx.x; r < rows; r += WG_THREADS) {
        const uint32_t *q = in + r * SWEEP_WORDS;
        acc[0] += q[0];
        acc[1] += q[1];
        w = max(w, q[2]);
    }
    part[0][threadIdx.x] = acc[0]; part[1][threadIdx.x] = acc[1];
    worst[threadIdx.x] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        SweepRow r{0, 0, 0, 0};
        for (uint32_t i = 0; i < WG_THREADS; ++i) {
            r.sse += part[0][i]; r.updates += part[1][i];
            r.max_abs = max(r.max_abs, worst[i]);
        }
        out[blockIdx.x] = r;
    }
}

}  // namespace rbf
