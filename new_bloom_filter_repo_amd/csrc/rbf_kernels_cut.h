// rbf_kernels_cut.h -- scene-cut statistics of a block of dense interleaved frames (k_cut_stats, its plain per-pixel twin k_cut_stats_px
// for what the lane tiles do not cover, and k_cut_reduce): for every pair (t-1, t) of the block three integers that say whether frame t is
// cheaper as an inter-frame against frame t-1 or as a keyframe of its own.  include/rbf.h (rbf_cut_stats) has the normative text:
//   glen(u)    = 2 floor(log2(u + 1)) + 1, the Elias-gamma length of u + 1, with u = rice_map((x - pred) mod 2^B) -- the sample codec's mapping
//   moving     = pixels with a sample where |x_t[c] - x_{t-1}[c]| > tolerance (the true unsigned difference, as in the hold)
//   inter_bits = sum of glen over all samples of the moving pixels, pred = x_{t-1}
//   intra_bits = sum of glen over all samples of frame t with the type-3 predictor: the pixel to the left, in column 0 the pixel above,
//                0 for the first pixel (k_rice_intra_u)
// The kernels only read the frames.  No atomics: a wave writes its three sums of every pair to a row of its own (every row is written by
// every call, so nothing stale survives), k_cut_reduce folds a pair's rows into its uint64 -- integer sums, the result is deterministic.
#pragma once
#include "rbf_kernels_hold.h"

namespace rbf {

constexpr uint32_t CUT_LANE_PIXELS = HOLD_LANE_PIXELS, CUT_STATS = 3;      // moving, inter_bits, intra_bits

// glen(rice_map(x - pred)) without the mapping: with s the residual as a signed B-bit number, u + 1 is 2s + 1 (s >= 0) or 2|s| (s < 0), so
// floor(log2(u + 1)) = 1 + floor(log2 |s|) for either sign and glen = 2 floor(log2 |s|) + 3 = 65 - 2 clz32(|s|) -- which also holds at
// s = 0 with clz32(0) = 32.  |s| = min(a, 2^B - a) with a = |x - pred| (one v_sad_u32), the shorter way round the ring of 2^B residuals.
// (tests/test_scene_cuts_cpu.py checks the identity for every residual of both widths.)
template <typename SAMPLE>
__device__ __forceinline__ uint32_t cut_cost(uint32_t x, uint32_t pred)
{
    const uint32_t a = __usad(x, pred, 0u), wrap = (1u << (8 * sizeof(SAMPLE))) - a;
    return 65u - 2u * (uint32_t)__clz((int)(a < wrap ? a : wrap));
}

// sample s of a lane's tile held as dwords (s is a compile-time constant after unrolling)
template <typename SAMPLE>
__device__ __forceinline__ uint32_t cut_sample(const uint32_t *d, int s)
{
    if (sizeof(SAMPLE) == 2) return (d[s >> 1] >> (16 * (s & 1))) & 0xFFFFu;
    return (d[s >> 2] >> (8 * (s & 3))) & 0xFFu;
}

// The three sums of a wave for pair `pair` into its row: partials[(pair * rows + row) * 3 + j].  Every lane of the wave calls this.
__device__ __forceinline__ void cut_wave_store(uint32_t *__restrict__ partials, uint64_t rows, uint64_t row, uint32_t pair,
                                               uint32_t moving, uint32_t inter, uint32_t intra)
{
    moving = wave_sum_to_lane63(moving);       // (per lane <= 16 pixels x 4 samples x 33 bits: a wave's sum fits 32 bits with room)
    inter = wave_sum_to_lane63(inter);
    intra = wave_sum_to_lane63(intra);
    if ((threadIdx.x & 63u) == 63u) {
        uint32_t *out = partials + ((uint64_t)pair * rows + row) * CUT_STATS;
        out[0] = moving; out[1] = inter; out[2] = intra;
    }
}

// The lane tiles: lane L owns pixels 16 L .. 16 L + 15 (flat index) of EVERY frame of the block -- a whole number of 16-byte vectors --
// keeps frame t-1's tile in registers while it decides frame t, and has frame t+1's loads in flight (three tiles whose roles rotate, as
// in k_temporal_hold).  Every frame is read once; the intra term needs the pixel in front of the tile (one extra pixel load per frame,
// with the tile) and, for a pixel of the tile in column 0, the pixel one row up: W need not be a multiple of 16, so column 0 can fall
// anywhere in a tile (col0, a bit per pixel, is the same for every frame), but for frames wider than a few tiles almost no lane has one,
// so those loads sit under a branch that corrects the sums.  Requires frames and frame_stride to be multiples of 16 and
// lanes * 16 <= pixels of a frame.  No lane leaves early: the wave sums need all 64.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_cut_stats(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t nframes,
                                                          uint64_t lanes, uint32_t width, uint32_t tolerance,
                                                          uint32_t *__restrict__ partials, uint64_t rows)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)CUT_LANE_PIXELS * PB / 4, VEC = DW / 4;
    static_assert(DW % 4 == 0, "a lane's pixels are whole 16-byte vectors");
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    const bool active = lane < lanes;
    const uint64_t row = (uint64_t)blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const uint64_t i0 = lane * CUT_LANE_PIXELS;                    // the tile's first pixel
    const uint32_t delta2 = tolerance | (tolerance << 16);
    const uint8_t *const p = frames + i0 * (uint64_t)PB;
    uint32_t col0 = 0;                                             // bit k: pixel i0 + k is in column 0
    if (active) {
        uint32_t c = (uint32_t)(i0 % width);
#pragma unroll
        for (int k = 0; k < (int)CUT_LANE_PIXELS; ++k) {
            col0 |= (c == 0 ? 1u : 0u) << k;
            c = c + 1 == width ? 0 : c + 1;
        }
    }
    struct Tile {
        uint32_t d[DW], left[C];                                   // the lane's 16 pixels and the samples of pixel i0 - 1 (0 in front of pixel 0)
        __device__ __forceinline__ void zero()
        {
#pragma unroll
            for (int i = 0; i < DW; ++i) d[i] = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) left[c] = 0;
        }
        __device__ __forceinline__ void load(const uint8_t *q, bool has_left)
        {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
            if (has_left) {
                const SAMPLE *l = reinterpret_cast<const SAMPLE *>(q) - C;
#pragma unroll
                for (int c = 0; c < C; ++c) left[c] = l[c];
            }
        }
    };
    Tile ta, tb, tc;                                               // the roles prev, cur, next rotate
    ta.zero(); tb.zero(); tc.zero();
    if (active) {
        ta.load(p, false);
        tb.load(p + frame_stride, i0 > 0);
    }
    auto step = [&](const Tile &prev, const Tile &cur, Tile &nxt, uint32_t t) {
        if (active && t + 1 < nframes) nxt.load(p + (uint64_t)(t + 1) * frame_stride, i0 > 0);
        uint32_t ex[DW];
#pragma unroll
        for (int d = 0; d < DW; ++d) ex[d] = hold_exceed<SAMPLE>(prev.d[d], cur.d[d], delta2);
        uint32_t moving = 0, inter = 0, intra = 0;
#pragma unroll
        for (int k = 0; k < (int)CUT_LANE_PIXELS; ++k) {
            const int d0 = k * PB / 4, d1 = ((k + 1) * PB - 1) / 4;
            uint32_t any = 0;
#pragma unroll
            for (int d = d0; d <= d1; ++d) any |= ex[d] & hold_pixel_bytes<PB>(k, d);
            uint32_t bits = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint32_t x = cut_sample<SAMPLE>(cur.d, k * C + c);
                bits += cut_cost<SAMPLE>(x, cut_sample<SAMPLE>(prev.d, k * C + c));
                intra += cut_cost<SAMPLE>(x, k == 0 ? cur.left[c] : cut_sample<SAMPLE>(cur.d, (k - 1) * C + c));
            }
            moving += any ? 1u : 0u;
            inter += any ? bits : 0u;
        }
        if (col0) {                                                // rare: a pixel of the tile starts a row -- its predictor is the pixel above
            const SAMPLE *const q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)t * frame_stride);
#pragma unroll
            for (int k = 0; k < (int)CUT_LANE_PIXELS; ++k)
                if ((col0 >> k) & 1u) {
                    const bool first = i0 + k < width;             // pixel 0 of the frame: predictor 0
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const uint32_t x = cut_sample<SAMPLE>(cur.d, k * C + c);
                        const uint32_t was = k == 0 ? cur.left[c] : cut_sample<SAMPLE>(cur.d, (k - 1) * C + c);
                        const uint32_t above = first ? 0u : (uint32_t)q[((int64_t)k - (int64_t)width) * C + c];
                        intra += cut_cost<SAMPLE>(x, above) - cut_cost<SAMPLE>(x, was);
                    }
                }
        }
        if (!active) { moving = 0; inter = 0; intra = 0; }
        cut_wave_store(partials, rows, row, t - 1, moving, inter, intra);
    };
    // unrolled by three so that the rotation prev <- cur <- nxt costs no register moves
    for (uint32_t t = 1; t < nframes; t += 3) {
        step(ta, tb, tc, t);
        if (t + 1 < nframes) step(tb, tc, ta, t + 1);
        if (t + 2 < nframes) step(tc, ta, tb, t + 2);
    }
}

// The plain path: a thread owns ONE pixel (first_pixel + its index, below n) of every frame and reads it sample by sample, so neither the
// frames' base nor their stride need more than the samples' own alignment.  Covers the tail of a frame behind the lane tiles, frames of
// fewer than 16 pixels and whole frames of a layout the lane tiles do not take.  Its waves' rows follow the lane tiles' (row0).
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_cut_stats_px(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t nframes,
                                                             uint64_t first_pixel, uint64_t n, uint32_t width, uint32_t channels,
                                                             uint32_t tolerance, uint32_t *__restrict__ partials, uint64_t rows, uint64_t row0)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    const bool active = px < n;
    const uint64_t row = row0 + (uint64_t)blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    // the type-3 predictor's pixel: the one to the left, in column 0 the one above, none for pixel 0
    const bool has_pred = active && px > 0;
    const uint64_t pp = !has_pred ? 0 : (px % width == 0 ? px - width : px - 1);
    const uint8_t *const p = frames + px * channels * sizeof(SAMPLE), *const q = frames + pp * channels * sizeof(SAMPLE);
    uint32_t prev[4] = {0, 0, 0, 0};                               // (loops of four with `c < channels` inside: the arrays stay in registers)
    if (active) {
        const SAMPLE *x = reinterpret_cast<const SAMPLE *>(p);
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) prev[c] = x[c];
    }
    for (uint32_t t = 1; t < nframes; ++t) {
        uint32_t moving = 0, inter = 0, intra = 0;
        if (active) {
            const SAMPLE *x = reinterpret_cast<const SAMPLE *>(p + (uint64_t)t * frame_stride);
            const SAMPLE *l = reinterpret_cast<const SAMPLE *>(q + (uint64_t)t * frame_stride);
            uint32_t worst = 0;
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c)
                if (c < channels) {
                    const uint32_t cur = x[c], pred = has_pred ? (uint32_t)l[c] : 0u;
                    const uint32_t d = cur > prev[c] ? cur - prev[c] : prev[c] - cur;
                    worst = d > worst ? d : worst;
                    inter += cut_cost<SAMPLE>(cur, prev[c]);
                    intra += cut_cost<SAMPLE>(cur, pred);
                    prev[c] = cur;
                }
            moving = worst > tolerance ? 1u : 0u;
            inter = moving ? inter : 0u;
        }
        cut_wave_store(partials, rows, row, t - 1, moving, inter, intra);
    }
}

// stats[pair * 3 + j] = the sum of the pair's rows, as uint64: one workgroup per pair (blockIdx.x).
__global__ __launch_bounds__(WG_THREADS) void k_cut_reduce(const uint32_t *__restrict__ partials, uint64_t rows, uint64_t *__restrict__ stats)
{
    __shared__ uint64_t part[CUT_STATS][WG_THREADS];
    const uint32_t *in = partials + (uint64_t)blockIdx.x * rows * CUT_STATS;
    uint64_t acc[CUT_STATS] = {0, 0, 0};
    for (uint64_t r = threadIdx.x; r < rows; r += WG_THREADS)
#pragma unroll
        for (uint32_t j = 0; j < CUT_STATS; ++j) acc[j] += in[r * CUT_STATS + j];
#pragma unroll
    for (uint32_t j = 0; j < CUT_STATS; ++j) part[j][threadIdx.x] = acc[j];
    __syncthreads();
    if (threadIdx.x < CUT_STATS) {
        uint64_t s = 0;
        for (uint32_t i = 0; i < WG_THREADS; ++i) s += part[threadIdx.x][i];
        stats[(uint64_t)blockIdx.x * CUT_STATS + threadIdx.x] = s;
    }
}

}  // namespace rbf
