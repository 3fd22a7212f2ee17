// rbf_kernels_hold.h -- the near-lossless stage in front of the mask stage: the bounded-error temporal hold (k_temporal_hold, and its
// plain per-pixel twin k_temporal_hold_px for what the lane tiles do not cover), in place on a block of dense interleaved frames.
//
// Per pixel and run (a run = a keyframe of the caller's stream and the frames that hang off it):
//   y_0 = x_0;   y_t = y_{t-1} if |x_t[c] - y_{t-1}[c]| <= max_error for EVERY sample c of the pixel, else y_t = x_t (the whole pixel).
// The comparison is against the HELD pixel, not the previous input frame, so |y_t - x_t| <= max_error for every sample of every frame
// (a slow drift is caught as soon as it has left the bound), and y_t differs from y_{t-1} exactly at the pixels the hold let through:
// coding y with the exact all-channel mask path IS the near-lossless codec.  The difference is the true unsigned one: 16-bit samples
// 0 and 0x8000 are 32768 apart (no int16 wrap, unlike the luma rule of residual_bit).
//
// Holding y again gives y (idempotent): a held pixel is its own reference.  No atomics: the output is deterministic.
#pragma once
#include "rbf_kernels.h"

namespace rbf {

// The runs of one launch (blockIdx.y): run y is the frames first[y] .. first[y] + len[y] - 1, frame first[y] is never written.
constexpr uint32_t HOLD_MAX_RUNS = 128, HOLD_LANE_PIXELS = 16;
struct HoldRuns {
    uint32_t first[HOLD_MAX_RUNS], len[HOLD_MAX_RUNS];
};

typedef unsigned short hold_h2 __attribute__((ext_vector_type(2)));

// Both 16-bit halves of a and b at once: a half of the result is non-zero iff |a.half - b.half| > delta.half (v_pk_max_u16, v_pk_min_u16,
// v_pk_sub_u16 and its clamping form: max - min cannot wrap, the saturating subtraction of delta leaves what exceeds it).
__device__ __forceinline__ uint32_t hold_exceed16(uint32_t a, uint32_t b, uint32_t delta2)
{
    const hold_h2 x = __builtin_bit_cast(hold_h2, a), y = __builtin_bit_cast(hold_h2, b);
    const hold_h2 d = __builtin_elementwise_max(x, y) - __builtin_elementwise_min(x, y);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(d, __builtin_bit_cast(hold_h2, delta2)));
}

// A dword of samples: every sample's field of the result is non-zero iff that sample of a and b differs by more than the bound.  Bytes go
// through the 16-bit routine as their even and their odd half (the excess of a byte is < 256: it fits the byte it came from).
// The bounds come packed per half: `de` holds those of the dword's two 16-bit samples, or of its even bytes, `dodd` those of its odd
// bytes (unused at 16 bits).  One bound for every sample is de = dodd = bound | bound << 16.
template <typename SAMPLE>
__device__ __forceinline__ uint32_t hold_exceed(uint32_t a, uint32_t b, uint32_t de, uint32_t dodd)
{
    if (sizeof(SAMPLE) == 2) return hold_exceed16(a, b, de);
    const uint32_t even = hold_exceed16(a & 0x00FF00FFu, b & 0x00FF00FFu, de);
    const uint32_t odd = hold_exceed16((a >> 8) & 0x00FF00FFu, (b >> 8) & 0x00FF00FFu, dodd);
    return even | (odd << 8);
}
template <typename SAMPLE>
__device__ __forceinline__ uint32_t hold_exceed(uint32_t a, uint32_t b, uint32_t delta2)
{
    return hold_exceed<SAMPLE>(a, b, delta2, delta2);
}

// the bytes of dword d that belong to pixel k of a lane's 16 pixels of PB bytes each (compile-time after unrolling)
template <int PB>
__device__ __forceinline__ constexpr uint32_t hold_pixel_bytes(int k, int d)
{
    uint32_t m = 0;
    for (int b = 0; b < 4; ++b) {
        const int byte = 4 * d + b;
        if (byte >= k * PB && byte < (k + 1) * PB) m |= 0xFFu << (8 * b);
    }
    return m;
}

// One frame of one lane: `held` (the lane's 16 held pixels, DW dwords) against `cur` (the frame's).  On return `held` is y_t: the pixels
// with a sample out of bound are cur's, whole -- a pixel that straddles two dwords is selected in both with its own byte masks -- and
// the others are kept.  The decision is a select per pixel, there is no branch.
// MAP = false: one bound for every sample, de[0] = dodd[0] = delta2.  MAP = true: a bound per sample, de[d] / dodd[d] for dword d of the
// tile in hold_exceed's two-bound form (k_hold_map).
template <typename SAMPLE, int C, bool MAP = false>
__device__ __forceinline__ void hold_lane_step(uint32_t *held, const uint32_t *cur, const uint32_t *de, const uint32_t *dodd)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)HOLD_LANE_PIXELS * PB / 4;
    uint32_t ex[DW], take[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) {
        ex[d] = hold_exceed<SAMPLE>(held[d], cur[d], de[MAP ? d : 0], dodd[MAP ? d : 0]);
        take[d] = 0;
    }
#pragma unroll
    for (int k = 0; k < (int)HOLD_LANE_PIXELS; ++k) {
        const int d0 = k * PB / 4, d1 = ((k + 1) * PB - 1) / 4;     // the dwords pixel k has bytes in: one, or two (a straddling or an 8-byte pixel)
        uint32_t any = 0;
#pragma unroll
        for (int d = d0; d <= d1; ++d) any |= ex[d] & hold_pixel_bytes<PB>(k, d);
        const uint32_t upd = any ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int d = d0; d <= d1; ++d) take[d] |= upd & hold_pixel_bytes<PB>(k, d);
    }
#pragma unroll
    for (int d = 0; d < DW; ++d) held[d] = (cur[d] & take[d]) | (held[d] & ~take[d]);
}

// The lane tiles: lane L of the launch owns pixels 16 L .. 16 L + 15 of every frame of run blockIdx.y -- 16 * C * sizeof(SAMPLE) bytes, a
// whole number of 16-byte vectors -- keeps the held pixels in registers, streams the run's frames with 16-byte loads (two frames of
// prefetch in flight, as the mask kernel) and writes back only the vectors in which some pixel was held (the others already are y_t).
// Requires frames and frame_stride to be multiples of 16 and lanes * 16 <= pixels of a frame; the host sends the rest to k_temporal_hold_px.
// Cache policy (rbf_lds_dma.h): NOT the streaming accesses of the mask kernel.  A lane's vectors are 16 * PIXEL_BYTES apart, so one store
// instruction of a wave covers only part of every 128-byte line it touches; plain stores let L2 put the lines together (and find them
// there: the loads brought them in), streaming ones reach memory as partial lines.  Measured on a 61-frame 1080p 8-bit block
// (profiles/r12_near_lossless_leg.txt): streaming loads and stores 418 us, plain stores 186 us, plain loads and stores 156 us.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_temporal_hold(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t lanes,
                                                              uint32_t max_error, const HoldRuns runs)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)HOLD_LANE_PIXELS * PB / 4, VEC = DW / 4;
    static_assert(DW % 4 == 0, "a lane's pixels are whole 16-byte vectors");
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];      // frames f0 + 1 .. f1 - 1 are rewritten
    if (f1 - f0 < 2) return;
    const uint32_t delta2 = max_error | (max_error << 16);      // (8-bit: the bound of an even / odd byte sits in a half)
    uint8_t *const p = frames + lane * (uint64_t)(HOLD_LANE_PIXELS * PB);
    struct Frame {
        uint32_t d[DW];
        __device__ __forceinline__ void load(const uint8_t *q)
        {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
        }
    };
    Frame held, fa, fb, fc;                                       // the roles of fa, fb, fc rotate: two loads are in flight while a frame is decided
    held.load(p + (uint64_t)f0 * frame_stride);
    fa.load(p + (uint64_t)(f0 + 1) * frame_stride);
    if (f0 + 2 < f1) fb.load(p + (uint64_t)(f0 + 2) * frame_stride);
    auto step = [&](const Frame &cur, Frame &nxt2, uint32_t f) {
        if (f + 2 < f1) nxt2.load(p + (uint64_t)(f + 2) * frame_stride);
        hold_lane_step<SAMPLE, C>(held.d, cur.d, &delta2, &delta2);
        uint4 *const out = reinterpret_cast<uint4 *>(p + (uint64_t)f * frame_stride);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const uint32_t differs = (held.d[4 * i] ^ cur.d[4 * i]) | (held.d[4 * i + 1] ^ cur.d[4 * i + 1]) |
                                     (held.d[4 * i + 2] ^ cur.d[4 * i + 2]) | (held.d[4 * i + 3] ^ cur.d[4 * i + 3]);
            if (differs) out[i] = make_uint4(held.d[4 * i], held.d[4 * i + 1], held.d[4 * i + 2], held.d[4 * i + 3]);
        }
    };
    // unrolled by three so that the rotation cur <- nxt <- nxt2 costs no register moves
    for (uint32_t f = f0 + 1; f < f1; f += 3) {
        step(fa, fc, f);
        if (f + 1 < f1) step(fb, fa, f + 1);
        if (f + 2 < f1) step(fc, fb, f + 2);
    }
}

// k_temporal_hold with a bound per sample: `bounds` is one dense frame of bounds E[p][c] in the frames' own layout and sample type, a
// multiple of 16 like the frames.  The lane loads its tile of it ONCE per run, next to the run's first frame -- 1 / (run length) more
// traffic -- and keeps it in registers in the form hold_exceed wants (8 bits: the tile's even and its odd bytes, split once); the walk
// over the run is k_temporal_hold's.  |y_t - x_t| <= E[p][c]; a pixel whose bounds are 0 is exact.
// A sibling and not a template flag of k_temporal_hold: moving that kernel's body into a function both could share changes its register
// allocation (measured with tools/kernel_resources.py), and the scalar kernels are to stay the code objects they were.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_hold_map(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t lanes,
                                                         const uint8_t *__restrict__ bounds, const HoldRuns runs)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)HOLD_LANE_PIXELS * PB / 4, VEC = DW / 4;
    static_assert(DW % 4 == 0, "a lane's pixels are whole 16-byte vectors");
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];      // frames f0 + 1 .. f1 - 1 are rewritten
    if (f1 - f0 < 2) return;
    uint8_t *const p = frames + lane * (uint64_t)(HOLD_LANE_PIXELS * PB);
    struct Frame {
        uint32_t d[DW];
        __device__ __forceinline__ void load(const uint8_t *q)
        {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
        }
    };
    Frame held, fa, fb, fc;
    uint32_t de[DW], dodd[sizeof(SAMPLE) == 1 ? DW : 1];
    {
        Frame e;
        e.load(bounds + lane * (uint64_t)(HOLD_LANE_PIXELS * PB));
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            de[d] = sizeof(SAMPLE) == 2 ? e.d[d] : e.d[d] & 0x00FF00FFu;
            if (sizeof(SAMPLE) == 1) dodd[d] = (e.d[d] >> 8) & 0x00FF00FFu;
        }
    }
    held.load(p + (uint64_t)f0 * frame_stride);
    fa.load(p + (uint64_t)(f0 + 1) * frame_stride);
    if (f0 + 2 < f1) fb.load(p + (uint64_t)(f0 + 2) * frame_stride);
    auto step = [&](const Frame &cur, Frame &nxt2, uint32_t f) {
        if (f + 2 < f1) nxt2.load(p + (uint64_t)(f + 2) * frame_stride);
        hold_lane_step<SAMPLE, C, true>(held.d, cur.d, de, sizeof(SAMPLE) == 1 ? dodd : de);
        uint4 *const out = reinterpret_cast<uint4 *>(p + (uint64_t)f * frame_stride);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const uint32_t differs = (held.d[4 * i] ^ cur.d[4 * i]) | (held.d[4 * i + 1] ^ cur.d[4 * i + 1]) |
                                     (held.d[4 * i + 2] ^ cur.d[4 * i + 2]) | (held.d[4 * i + 3] ^ cur.d[4 * i + 3]);
            if (differs) out[i] = make_uint4(held.d[4 * i], held.d[4 * i + 1], held.d[4 * i + 2], held.d[4 * i + 3]);
        }
    };
    for (uint32_t f = f0 + 1; f < f1; f += 3) {
        step(fa, fc, f);
        if (f + 1 < f1) step(fb, fa, f + 1);
        if (f + 2 < f1) step(fc, fb, f + 2);
    }
}

// The plain path: a thread owns ONE pixel (first_pixel + its index, below n) of run blockIdx.y and reads and writes it sample by sample, so
// neither the frames' base nor their stride need more than the samples' own alignment.  Covers the tail of a frame behind the lane tiles,
// and whole frames of a layout the lane tiles do not take.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_temporal_hold_px(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t first_pixel,
                                                                 uint64_t n, uint32_t channels, uint32_t max_error, const HoldRuns runs)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (px >= n) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    uint8_t *const p = frames + px * channels * sizeof(SAMPLE);
    uint32_t held[4] = {0, 0, 0, 0};                             // (loops of four with `c < channels` inside: the arrays stay in registers)
    {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f0 * frame_stride);
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) held[c] = q[c];
    }
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        SAMPLE *q = reinterpret_cast<SAMPLE *>(p + (uint64_t)f * frame_stride);
        uint32_t cur[4] = {0, 0, 0, 0}, worst = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) {
                cur[c] = q[c];
                const uint32_t d = cur[c] > held[c] ? cur[c] - held[c] : held[c] - cur[c];
                worst = d > worst ? d : worst;
            }
        const bool upd = worst > max_error;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            held[c] = upd ? cur[c] : held[c];
            if (!upd && c < channels) q[c] = (SAMPLE)held[c];
        }
    }
}

// k_temporal_hold_px with a bound per sample: the pixel's bounds are read sample by sample from `bounds`, once per run, so any
// sample-aligned bound frame will do.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_hold_map_px(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t first_pixel,
                                                            uint64_t n, uint32_t channels, const uint8_t *__restrict__ bounds, const HoldRuns runs)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (px >= n) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    uint8_t *const p = frames + px * channels * sizeof(SAMPLE);
    uint32_t held[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
    {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f0 * frame_stride);
        const SAMPLE *b = reinterpret_cast<const SAMPLE *>(bounds + px * channels * sizeof(SAMPLE));
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) { held[c] = q[c]; e[c] = b[c]; }
    }
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        SAMPLE *q = reinterpret_cast<SAMPLE *>(p + (uint64_t)f * frame_stride);
        uint32_t cur[4] = {0, 0, 0, 0};
        bool upd = false;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) {
                cur[c] = q[c];
                upd |= (cur[c] > held[c] ? cur[c] - held[c] : held[c] - cur[c]) > e[c];
            }
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            held[c] = upd ? cur[c] : held[c];
            if (!upd && c < channels) q[c] = (SAMPLE)held[c];
        }
    }
}

}  // namespace rbf
