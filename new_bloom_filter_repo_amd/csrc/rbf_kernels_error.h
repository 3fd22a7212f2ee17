// rbf_kernels_error.h -- the quality report: what a coded block B differs from its originals A by (k_error_stats, its plain per-pixel
// twin k_error_stats_px for what the lane tiles do not cover, and k_error_reduce).  A and B are two blocks of dense interleaved frames of
// one geometry, each with a base and a stride of its own.  Per frame, over all its samples (include/rbf.h, rbf_error_stats):
//   sse        = sum of (a - b)^2, exact integers
//   differing  = samples with a != b
//   over_bound = samples with |a - b| > their bound: E[p][c] of a bound frame (the layout of a frame), or one scalar
//   max_abs    = the largest |a - b|
// |a - b| is the true unsigned difference, as in the hold (rbf_kernels_hold.h): packed max - min, two 16-bit samples or two bytes of a dword
// per instruction.  The kernels only read.  No atomics: a wave writes its sums of every frame to a row of its own (every row is written
// by every call, so nothing stale survives), k_error_reduce folds a frame's rows -- integer sums and a max, the result is deterministic.
#pragma once
#include "rbf_kernels_lookahead.h"

namespace rbf {

constexpr uint32_t ERR_LANE_PIXELS = HOLD_LANE_PIXELS, ERR_WORDS = 6;      // a wave's row: sse (low, high dword), differing, over_bound, max_abs, 0

struct ErrorRow {                                                          // = rbf_error_row (include/rbf.h)
    uint64_t sse, differing, over_bound;
    uint32_t max_abs, reserved;
};

__device__ __forceinline__ uint32_t err_add2(uint32_t a, uint32_t b)       // both halves, no carry between them
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(hold_h2, a) + __builtin_bit_cast(hold_h2, b));
}

// The largest value of the wave's 64 lanes, valid in lane 63: wave_sum_to_lane63's steps with max for + (a lane without a source reads 0).
__device__ __forceinline__ uint32_t wave_max_to_lane63(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, true));     // row_ror:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true));     // row_ror:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, true));     // row_bcast:15 -> rows 1 and 3
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, true));     // row_bcast:31 -> rows 2 and 3
    return v;
}

// What a lane has seen of one frame.  `diff`, `over` and `worst` are packed pairs of 16-bit fields, one per half of a plane: a lane has
// at most 16 pixels x 4 samples, so a field counts to 32 at the most.  sse: a lane's 64 squares of up to 65535^2 need 38 bits.
struct ErrAcc {
    uint64_t sse = 0;
    uint32_t diff = 0, over = 0, worst = 0;
    // d: |a - b| of two samples, one per half; e: their bounds
    __device__ __forceinline__ void add(uint32_t d, uint32_t e)
    {
        const uint32_t l = d & 0xFFFFu, h = d >> 16;
        sse += (uint64_t)(l * l) + (uint64_t)(h * h);                      // (65535^2 < 2^32)
        diff = err_add2(diff, la_min(d, 0x00010001u));
        over = err_add2(over, la_min(la_subs(d, e), 0x00010001u));
        worst = la_max(worst, d);
    }
    __device__ __forceinline__ void add1(uint32_t d, uint32_t e)           // one sample
    {
        sse += (uint64_t)(d * d);
        diff += d ? 1u : 0u;
        over += d > e ? 1u : 0u;
        worst = max(worst, d);
    }
};

// A wave's sums of frame f into its row: partials[(f * rows + row) * 6 ..].  Every lane of the wave calls this.  The 64-bit sse goes
// through the 32-bit wave sum in two parts of 20 and 18 bits: 64 lanes of either fit a dword.
__device__ __forceinline__ void err_wave_store(uint32_t *__restrict__ partials, uint64_t rows, uint64_t row, uint32_t f, const ErrAcc &a)
{
    const uint32_t lo = wave_sum_to_lane63((uint32_t)a.sse & 0xFFFFFu), hi = wave_sum_to_lane63((uint32_t)(a.sse >> 20));
    const uint32_t diff = wave_sum_to_lane63((a.diff & 0xFFFFu) + (a.diff >> 16));
    const uint32_t over = wave_sum_to_lane63((a.over & 0xFFFFu) + (a.over >> 16));
    const uint32_t worst = wave_max_to_lane63(max(a.worst & 0xFFFFu, a.worst >> 16));
    if ((threadIdx.x & 63u) == 63u) {
        const uint64_t sse = ((uint64_t)hi << 20) + lo;
        uint32_t *out = partials + ((uint64_t)f * rows + row) * ERR_WORDS;
        out[0] = (uint32_t)sse; out[1] = (uint32_t)(sse >> 32); out[2] = diff; out[3] = over; out[4] = worst; out[5] = 0;
    }
}

// The lane tiles: lane L owns pixels 16 L .. 16 L + 15 (flat index) of EVERY frame of both blocks -- a whole number of 16-byte vectors --
// loads its tile of the bound frame once (MAP; else every sample has the scalar `bound`) and walks the frames with the next frame's
// tiles of A and B in flight.  Requires a, b, bounds and both strides to be multiples of 16 and lanes * 16 <= pixels of a frame.  Plain
// loads: a lane's vectors are 16 * PIXEL_BYTES apart (the cache-policy note of k_temporal_hold).  No lane leaves early: the wave sums need all 64.
template <typename SAMPLE, int C, bool MAP>
__global__ __launch_bounds__(WG_THREADS) void k_error_stats(const uint8_t *__restrict__ a, uint64_t a_stride, const uint8_t *__restrict__ b,
                                                            uint64_t b_stride, uint32_t nframes, uint64_t lanes,
                                                            const uint8_t *__restrict__ bounds, uint32_t bound,
                                                            uint32_t *__restrict__ partials, uint64_t rows)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)ERR_LANE_PIXELS * PB / 4, VEC = DW / 4;
    static_assert(DW % 4 == 0, "a lane's pixels are whole 16-byte vectors");
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    const bool active = lane < lanes;
    const uint64_t row = (uint64_t)blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const uint64_t off = lane * (uint64_t)(ERR_LANE_PIXELS * PB);
    struct Tile {
        uint32_t d[DW];
        __device__ __forceinline__ void zero()
        {
#pragma unroll
            for (int i = 0; i < DW; ++i) d[i] = 0;
        }
        __device__ __forceinline__ void load(const uint8_t *q)
        {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
        }
    };
    // the bounds in the form of the planes below: of a dword's two 16-bit samples, or of its even (ee) and its odd (eo) bytes
    uint32_t ee[MAP ? DW : 1], eo[MAP && sizeof(SAMPLE) == 1 ? DW : 1];
    ee[0] = eo[0] = bound | (bound << 16);
    if (MAP && active) {
        Tile e;
        e.load(bounds + off);
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            ee[MAP ? d : 0] = sizeof(SAMPLE) == 2 ? e.d[d] : e.d[d] & 0x00FF00FFu;
            if (sizeof(SAMPLE) == 1) eo[MAP ? d : 0] = (e.d[d] >> 8) & 0x00FF00FFu;
        }
    } else if (MAP) {
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            ee[MAP ? d : 0] = 0;
            if (sizeof(SAMPLE) == 1) eo[MAP ? d : 0] = 0;
        }
    }
    Tile xa, xb, na, nb;                                           // this frame's tiles and the next one's
    xa.zero(); xb.zero(); na.zero(); nb.zero();
    if (active) {
        na.load(a + off);
        nb.load(b + off);
    }
    for (uint32_t f = 0; f < nframes; ++f) {
#pragma unroll
        for (int d = 0; d < DW; ++d) { xa.d[d] = na.d[d]; xb.d[d] = nb.d[d]; }
        if (active && f + 1 < nframes) {
            na.load(a + (uint64_t)(f + 1) * a_stride + off);
            nb.load(b + (uint64_t)(f + 1) * b_stride + off);
        }
        ErrAcc acc;
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            if (sizeof(SAMPLE) == 2) {
                acc.add(la_subs(la_max(xa.d[d], xb.d[d]), la_min(xa.d[d], xb.d[d])), ee[MAP ? d : 0]);
            } else {
                const uint32_t ae = xa.d[d] & 0x00FF00FFu, be = xb.d[d] & 0x00FF00FFu;
                const uint32_t ao = (xa.d[d] >> 8) & 0x00FF00FFu, bo = (xb.d[d] >> 8) & 0x00FF00FFu;
                acc.add(la_subs(la_max(ae, be), la_min(ae, be)), ee[MAP ? d : 0]);
                acc.add(la_subs(la_max(ao, bo), la_min(ao, bo)), eo[MAP ? d : 0]);
            }
        }
        err_wave_store(partials, rows, row, f, acc);               // (an inactive lane's tiles are zeros: it adds nothing)
    }
}

// The plain path: a thread owns ONE pixel (first_pixel + its index, below n) of every frame and reads it sample by sample, so neither the
// blocks' bases, nor their strides, nor `bounds` (NULL: the scalar `bound`) need more than the samples' own alignment.  Covers the tail
// of a frame behind the lane tiles and whole frames of a layout the lane tiles do not take.  Its waves' rows follow the lane tiles' (row0).
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_error_stats_px(const uint8_t *__restrict__ a, uint64_t a_stride, const uint8_t *__restrict__ b,
                                                               uint64_t b_stride, uint32_t nframes, uint64_t first_pixel, uint64_t n,
                                                               uint32_t channels, const uint8_t *__restrict__ bounds, uint32_t bound,
                                                               uint32_t *__restrict__ partials, uint64_t rows, uint64_t row0)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    const bool active = px < n;
    const uint64_t row = row0 + (uint64_t)blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const uint64_t off = px * channels * sizeof(SAMPLE);
    uint32_t e[4] = {bound, bound, bound, bound};                  // (loops of four with `c < channels` inside: the arrays stay in registers)
    if (active && bounds) {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(bounds + off);
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) e[c] = q[c];
    }
    for (uint32_t f = 0; f < nframes; ++f) {
        ErrAcc acc;
        if (active) {
            const SAMPLE *x = reinterpret_cast<const SAMPLE *>(a + (uint64_t)f * a_stride + off);
            const SAMPLE *y = reinterpret_cast<const SAMPLE *>(b + (uint64_t)f * b_stride + off);
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c)
                if (c < channels) {
                    const uint32_t u = x[c], v = y[c];
                    acc.add1(u > v ? u - v : v - u, e[c]);
                }
        }
        err_wave_store(partials, rows, row, f, acc);
    }
}

// out[f] = the fold of frame f's rows: one workgroup per frame (blockIdx.x).
__global__ __launch_bounds__(WG_THREADS) void k_error_reduce(const uint32_t *__restrict__ partials, uint64_t rows, ErrorRow *__restrict__ out)
{
    __shared__ uint64_t part[3][WG_THREADS];
    __shared__ uint32_t worst[WG_THREADS];
    const uint32_t *in = partials + (uint64_t)blockIdx.x * rows * ERR_WORDS;
    uint64_t acc[3] = {0, 0, 0};
    uint32_t w = 0;
    for (uint64_t r = threadIdx.x; r < rows; r += WG_THREADS) {
        const uint32_t *q = in + r * ERR_WORDS;
        acc[0] += (uint64_t)q[0] | ((uint64_t)q[1] << 32);
        acc[1] += q[2];
        acc[2] += q[3];
        w = max(w, q[4]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) part[j][threadIdx.x] = acc[j];
    worst[threadIdx.x] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        ErrorRow r{0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < WG_THREADS; ++i) {
            r.sse += part[0][i]; r.differing += part[1][i]; r.over_bound += part[2][i];
            r.max_abs = max(r.max_abs, worst[i]);
        }
        out[blockIdx.x] = r;
    }
}

}  // namespace rbf
