// rbf_kernels_lookahead.h -- the near-lossless stage's second decision rule: the look-ahead temporal hold (k_temporal_lookahead and
// k_lookahead_fill over lane tiles of 8 pixels, and the per-pixel k_temporal_lookahead_px for what the tiles do not cover), in place on a
// block of dense interleaved frames, over the same runs as k_temporal_hold (rbf_kernels_hold.h).
//
// The hold of rbf_kernels_hold.h keeps a pixel while every sample stays within e = max_error of the segment's FIRST value, so noise of
// +-a needs e >= 2a.  The bound itself only asks that a segment's samples fit one window of width 2e: a segment may run for as long as
// the windows [x_t - e, x_t + e] of its frames still have a point in common (greedy interval stabbing, the fewest segments for a fixed
// first value).  Per pixel and run, with M the sample type's largest value and true integer differences (no wrap):
//   y_0 = x_0.  The ANCHORED segment: while |x_t[c] - x_0[c]| <= e for every sample c, y_t = x_0 (the keyframe is coded exactly).
//   At the first frame t that breaks it a FREE segment opens: lo[c] = max(0, x_t[c] - e), hi[c] = min(M, x_t[c] + e).  A following frame
//   u narrows it: lo' = max(lo, max(0, x_u - e)), hi' = min(hi, min(M, x_u + e)); if lo'[c] > hi'[c] for ANY sample the segment ends at
//   u - 1 and a new one opens at u, else lo, hi = lo', hi'.  The run's end ends the last segment.
//   A free segment's value is v[c] = clamp(prev[c], lo[c], hi[c]), prev = the value of the segment before it (x_0 after the anchored
//   one); every frame of the segment gets v, the whole pixel.
// So |y_t - x_t| <= e everywhere; y_t != y_{t-1} exactly where a segment opens (the breaking sample's new window excludes prev[c]); the
// samples of a breaking pixel that can keep their value do (residual 0).  The anchored segment is the free one with lo = hi = x_0, which
// is how the kernels treat it.  NOT idempotent: stabbing y again can merge segments and double the error.  No atomics: deterministic.
//
// A segment's value is known only once it has ended, hence two sweeps.  Sweep 1 (k_temporal_lookahead) walks the run forward with lo, hi
// and prev in registers; when a pixel's segment closes it stores v into the pixel's slot of the segment's FIRST frame -- dead by then,
// its sample has gone into the window -- and it records the frames at which segments open in a scratch bitmap (a byte per lane tile and
// frame).  Sweep 2 (k_lookahead_fill) walks forward again: y_t = start bit ? frame[t] : y_{t-1}.
#pragma once
#include "rbf_kernels_hold.h"

namespace rbf {

constexpr uint32_t LA_LANE_PIXELS = 8;      // a lane tile: 8 pixels = one byte of the start bitmap, 8 * PIXEL_BYTES bytes = whole 8-byte vectors

__device__ __forceinline__ uint32_t la_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(hold_h2, a), __builtin_bit_cast(hold_h2, b)));
}
__device__ __forceinline__ uint32_t la_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(hold_h2, a), __builtin_bit_cast(hold_h2, b)));
}
__device__ __forceinline__ uint32_t la_adds(uint32_t a, uint32_t b)      // both halves, clamped at 0xFFFF
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(__builtin_bit_cast(hold_h2, a), __builtin_bit_cast(hold_h2, b)));
}
__device__ __forceinline__ uint32_t la_subs(uint32_t a, uint32_t b)      // both halves, clamped at 0
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(hold_h2, a), __builtin_bit_cast(hold_h2, b)));
}

// A lane's samples live in PLANES of two 16-bit halves, so that every step is a packed u16 instruction: a dword of 16-bit samples is
// one plane; a dword of bytes is two, its even bytes (plane 2d) and its odd bytes (plane 2d + 1), each byte in a half of its own.
template <typename SAMPLE, int C> struct LaGeom {
    static constexpr int PB = C * (int)sizeof(SAMPLE), DW = (int)LA_LANE_PIXELS * PB / 4, VEC = DW / 2;
    static constexpr int NP = sizeof(SAMPLE) == 2 ? DW : 2 * DW;
    static constexpr uint32_t TOP2 = sizeof(SAMPLE) == 2 ? 0xFFFFFFFFu : 0x00FF00FFu;
    // where sample s of the lane (pixel s / C, channel s % C) sits: its plane, and the half of it
    static constexpr int plane(int s) { return sizeof(SAMPLE) == 2 ? s / 2 : 2 * (s / 4) + (s & 1); }
    static constexpr int half(int s) { return sizeof(SAMPLE) == 2 ? s & 1 : (s >> 1) & 1; }
    // the halves of plane p that belong to pixel k
    static constexpr uint32_t mask(int k, int p)
    {
        uint32_t m = 0;
        for (int s = k * C; s < (k + 1) * C; ++s)
            if (plane(s) == p) m |= 0xFFFFu << (16 * half(s));
        return m;
    }
    static __device__ __forceinline__ void to_planes(const uint32_t *d, uint32_t *pl)
    {
#pragma unroll
        for (int i = 0; i < DW; ++i) {
            if (sizeof(SAMPLE) == 2) pl[i] = d[i];
            else { pl[2 * i] = d[i] & 0x00FF00FFu; pl[2 * i + 1] = (d[i] >> 8) & 0x00FF00FFu; }
        }
    }
    static __device__ __forceinline__ void load(const uint8_t *q, uint32_t *d)
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const uint2 v = reinterpret_cast<const uint2 *>(q)[i];
            d[2 * i] = v.x; d[2 * i + 1] = v.y;
        }
    }
};

// Sweep 1.  Lane L owns pixels 8 L .. 8 L + 7 of every frame of run blockIdx.y.  Frames f0 + 1 .. f1 - 1: the frame narrows every
// pixel's window; a pixel with a sample whose window has become empty closes its segment -- v goes to its slot of frame start[k], unless
// that is the run's first frame (the anchored segment: v = x_0 is there already, and that frame is never written) -- and opens the next
// one at this frame.  bits[f * bits_stride + L] gets the frame's start bits (bit k: pixel 8 L + k).  The state update is a select per
// pixel; only the store of a closing pixel is a branch.
// Requires frames and frame_stride to be multiples of 8 and lanes * 8 <= pixels of a frame.  Plain loads and stores, as the hold (see
// the cache-policy note there): a lane's vectors are 8 * PIXEL_BYTES apart and the sample stores are scattered, L2 puts the lines together.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_temporal_lookahead(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t lanes,
                                                                   uint32_t max_error, uint8_t *__restrict__ bits, uint64_t bits_stride,
                                                                   const HoldRuns runs)
{
    using G = LaGeom<SAMPLE, C>;
    constexpr int DW = G::DW, NP = G::NP, K = (int)LA_LANE_PIXELS;
    static_assert(DW % 2 == 0, "a lane's pixels are whole 8-byte vectors");
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    if (f1 - f0 < 2) return;
    const uint32_t e2 = max_error | (max_error << 16);
    uint8_t *const p = frames + lane * (uint64_t)(K * G::PB);
    uint32_t lo[NP], hi[NP], prev[NP], start[K];
    {
        uint32_t d[DW];
        G::load(p + (uint64_t)f0 * frame_stride, d);
        G::to_planes(d, prev);
#pragma unroll
        for (int i = 0; i < NP; ++i) lo[i] = hi[i] = prev[i];
#pragma unroll
        for (int k = 0; k < K; ++k) start[k] = f0;
    }
    // pixel k's closing segment: v = clamp(prev, lo, hi) in its planes, stored sample by sample into frame start[k]
    auto store_value = [&](int k, const uint32_t *v) {
        SAMPLE *const q = reinterpret_cast<SAMPLE *>(p + (uint64_t)start[k] * frame_stride);
#pragma unroll
        for (int s = k * C; s < (k + 1) * C; ++s) q[s] = (SAMPLE)(v[G::plane(s)] >> (16 * G::half(s)));
    };
    uint32_t nxt[DW];
    G::load(p + (uint64_t)(f0 + 1) * frame_stride, nxt);
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        uint32_t x[NP], xl[NP], xh[NP], bad[NP], v[NP];
        G::to_planes(nxt, x);
        if (f + 1 < f1) G::load(p + (uint64_t)(f + 1) * frame_stride, nxt);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            xl[i] = la_subs(x[i], e2);
            xh[i] = la_min(la_adds(x[i], e2), G::TOP2);
            v[i] = la_min(la_max(prev[i], lo[i]), hi[i]);           // (of the window BEFORE this frame: what a closing segment gets)
            lo[i] = la_max(lo[i], xl[i]);
            hi[i] = la_min(hi[i], xh[i]);
            bad[i] = la_subs(lo[i], hi[i]);                          // a half is non-zero iff its window is empty
        }
        uint32_t opened = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (G::mask(k, i)) any |= bad[i] & G::mask(k, i);
            if (any) {
                if (start[k] != f0) store_value(k, v);
                opened |= 1u << k;
            }
            const uint32_t upd = any ? 0xFFFFFFFFu : 0u;
            start[k] = any ? f : start[k];
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (G::mask(k, i)) {
                    const uint32_t m = upd & G::mask(k, i);
                    prev[i] = (v[i] & m) | (prev[i] & ~m);
                    lo[i] = (xl[i] & m) | (lo[i] & ~m);
                    hi[i] = (xh[i] & m) | (hi[i] & ~m);
                }
        }
        bits[(uint64_t)f * bits_stride + lane] = (uint8_t)opened;
    }
    // the run's end ends every pixel's last segment
    uint32_t v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = la_min(la_max(prev[i], lo[i]), hi[i]);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (start[k] != f0) store_value(k, v);
}

// Sweep 1 with a bound per sample: e = E[p][c], read from `bounds` -- one dense frame of bounds in the frames' own layout and sample
// type, a multiple of 8 like the frames.  The lane loads its tile ONCE per run and keeps it as planes (NP more registers), so the
// windows' saturating add and subtract take a plane of bounds where k_temporal_lookahead repeats one dword.  Everything else -- the
// stabbing, the clamp, the bitmap, and sweep 2, which never sees a bound -- is that kernel's.  (A sibling and not a template flag, for
// the reason given at k_hold_map.)
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_lookahead_map(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t lanes,
                                                              const uint8_t *__restrict__ bounds, uint8_t *__restrict__ bits,
                                                              uint64_t bits_stride, const HoldRuns runs)
{
    using G = LaGeom<SAMPLE, C>;
    constexpr int DW = G::DW, NP = G::NP, K = (int)LA_LANE_PIXELS;
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    if (f1 - f0 < 2) return;
    uint8_t *const p = frames + lane * (uint64_t)(K * G::PB);
    uint32_t e[NP], lo[NP], hi[NP], prev[NP], start[K];
    {
        uint32_t d[DW];
        G::load(bounds + lane * (uint64_t)(K * G::PB), d);
        G::to_planes(d, e);
        G::load(p + (uint64_t)f0 * frame_stride, d);
        G::to_planes(d, prev);
#pragma unroll
        for (int i = 0; i < NP; ++i) lo[i] = hi[i] = prev[i];
#pragma unroll
        for (int k = 0; k < K; ++k) start[k] = f0;
    }
    auto store_value = [&](int k, const uint32_t *v) {
        SAMPLE *const q = reinterpret_cast<SAMPLE *>(p + (uint64_t)start[k] * frame_stride);
#pragma unroll
        for (int s = k * C; s < (k + 1) * C; ++s) q[s] = (SAMPLE)(v[G::plane(s)] >> (16 * G::half(s)));
    };
    uint32_t nxt[DW];
    G::load(p + (uint64_t)(f0 + 1) * frame_stride, nxt);
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        uint32_t x[NP], xl[NP], xh[NP], bad[NP], v[NP];
        G::to_planes(nxt, x);
        if (f + 1 < f1) G::load(p + (uint64_t)(f + 1) * frame_stride, nxt);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            xl[i] = la_subs(x[i], e[i]);
            xh[i] = la_min(la_adds(x[i], e[i]), G::TOP2);
            v[i] = la_min(la_max(prev[i], lo[i]), hi[i]);
            lo[i] = la_max(lo[i], xl[i]);
            hi[i] = la_min(hi[i], xh[i]);
            bad[i] = la_subs(lo[i], hi[i]);
        }
        uint32_t opened = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (G::mask(k, i)) any |= bad[i] & G::mask(k, i);
            if (any) {
                if (start[k] != f0) store_value(k, v);
                opened |= 1u << k;
            }
            const uint32_t upd = any ? 0xFFFFFFFFu : 0u;
            start[k] = any ? f : start[k];
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (G::mask(k, i)) {
                    const uint32_t m = upd & G::mask(k, i);
                    prev[i] = (v[i] & m) | (prev[i] & ~m);
                    lo[i] = (xl[i] & m) | (lo[i] & ~m);
                    hi[i] = (xh[i] & m) | (hi[i] & ~m);
                }
        }
        bits[(uint64_t)f * bits_stride + lane] = (uint8_t)opened;
    }
    uint32_t v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = la_min(la_max(prev[i], lo[i]), hi[i]);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (start[k] != f0) store_value(k, v);
}

// Sweep 2, the same lanes: y = the run's first frame; a frame's pixels with their start bit set are the values sweep 1 left there and
// become y, the others take y, and the 8-byte vectors that change are written.  A lane whose byte of start bits is zero -- most lanes of
// most frames once the masks are sparse -- does not read the frame at all: it stores y over it (on footage with sensor noise the frame
// differs from y nearly everywhere, so those stores happen anyway, and the reads they would have needed do not).  The start bits are
// fetched two frames ahead, the frames they ask for one frame ahead.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_lookahead_fill(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t lanes,
                                                               const uint8_t *__restrict__ bits, uint64_t bits_stride, const HoldRuns runs)
{
    using G = LaGeom<SAMPLE, C>;
    constexpr int DW = G::DW, PB = G::PB, K = (int)LA_LANE_PIXELS;
    const uint64_t lane = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    if (f1 - f0 < 2) return;
    uint8_t *const p = frames + lane * (uint64_t)(K * PB);
    uint32_t y[DW], nxt[DW];
    G::load(p + (uint64_t)f0 * frame_stride, y);
    uint32_t b1 = bits[(uint64_t)(f0 + 1) * bits_stride + lane];                     // the start bits of frame f, and of frame f + 1
    uint32_t b2 = f0 + 2 < f1 ? bits[(uint64_t)(f0 + 2) * bits_stride + lane] : 0;
#pragma unroll
    for (int d = 0; d < DW; ++d) nxt[d] = 0;
    if (b1) G::load(p + (uint64_t)(f0 + 1) * frame_stride, nxt);
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        uint32_t cur[DW];
        const uint32_t b = b1;
#pragma unroll
        for (int d = 0; d < DW; ++d) cur[d] = nxt[d];
        b1 = b2;
        if (b1) G::load(p + (uint64_t)(f + 1) * frame_stride, nxt);                   // (b1 != 0 only if frame f + 1 is of this run)
        b2 = f + 2 < f1 ? bits[(uint64_t)(f + 2) * bits_stride + lane] : 0;
        uint2 *const out = reinterpret_cast<uint2 *>(p + (uint64_t)f * frame_stride);
        if (!b) {
#pragma unroll
            for (int i = 0; i < DW / 2; ++i) out[i] = make_uint2(y[2 * i], y[2 * i + 1]);
            continue;
        }
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            uint32_t take = 0;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (hold_pixel_bytes<PB>(k, d)) take |= ((b >> k) & 1u ? 0xFFFFFFFFu : 0u) & hold_pixel_bytes<PB>(k, d);
            y[d] = (cur[d] & take) | (y[d] & ~take);
        }
#pragma unroll
        for (int i = 0; i < DW / 2; ++i)
            if ((y[2 * i] ^ cur[2 * i]) | (y[2 * i + 1] ^ cur[2 * i + 1])) out[i] = make_uint2(y[2 * i], y[2 * i + 1]);
    }
}

// The plain path: a thread owns ONE pixel (first_pixel + its index, below n) of run blockIdx.y and reads and writes it sample by sample,
// so neither the frames' base nor their stride need more than the samples' own alignment.  It needs no bitmap: when the pixel's segment
// closes, the thread goes back over the segment's frames and writes v.  (The threads of a wave wait for the longest segment that closes
// at a frame; this path covers the last n % 8 pixels of a frame, and whole frames only of a layout the lane tiles do not take.)
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_temporal_lookahead_px(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t first_pixel,
                                                                      uint64_t n, uint32_t channels, uint32_t max_error, const HoldRuns runs)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (px >= n) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    if (f1 - f0 < 2) return;
    constexpr int32_t M = sizeof(SAMPLE) == 2 ? 0xFFFF : 0xFF;
    const int32_t e = (int32_t)max_error;
    uint8_t *const p = frames + px * channels * sizeof(SAMPLE);
    int32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, prev[4] = {0, 0, 0, 0};       // (loops of four with `c < channels` inside: registers)
    {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f0 * frame_stride);
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) lo[c] = hi[c] = prev[c] = q[c];
    }
    uint32_t start = f0 + 1;                                     // the first frame the open segment writes (the run's first frame is never written)
    auto close = [&](uint32_t end) {                             // frames start .. end - 1 get v = clamp(prev, lo, hi)
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) prev[c] = min(max(prev[c], lo[c]), hi[c]);
        for (uint32_t f = start; f < end; ++f) {
            SAMPLE *q = reinterpret_cast<SAMPLE *>(p + (uint64_t)f * frame_stride);
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c)
                if (c < channels) q[c] = (SAMPLE)prev[c];
        }
    };
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f * frame_stride);
        int32_t xl[4] = {0, 0, 0, 0}, xh[4] = {0, 0, 0, 0};
        bool empty = false;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) {
                const int32_t x = q[c];
                xl[c] = max(0, x - e);
                xh[c] = min(M, x + e);
                empty |= max(lo[c], xl[c]) > min(hi[c], xh[c]);
            }
        if (empty) {
            close(f);
            start = f;
        }
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            lo[c] = empty ? xl[c] : max(lo[c], xl[c]);
            hi[c] = empty ? xh[c] : min(hi[c], xh[c]);
        }
    }
    close(f1);
}

// k_temporal_lookahead_px with a bound per sample: the pixel's bounds are read sample by sample from `bounds`, once per run, so any
// sample-aligned bound frame will do.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_lookahead_map_px(uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t first_pixel,
                                                                 uint64_t n, uint32_t channels, const uint8_t *__restrict__ bounds,
                                                                 const HoldRuns runs)
{
    const uint64_t px = first_pixel + (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (px >= n) return;
    const uint32_t f0 = runs.first[blockIdx.y], f1 = f0 + runs.len[blockIdx.y];
    if (f1 - f0 < 2) return;
    constexpr int32_t M = sizeof(SAMPLE) == 2 ? 0xFFFF : 0xFF;
    uint8_t *const p = frames + px * channels * sizeof(SAMPLE);
    int32_t e[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, prev[4] = {0, 0, 0, 0};
    {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f0 * frame_stride);
        const SAMPLE *b = reinterpret_cast<const SAMPLE *>(bounds + px * channels * sizeof(SAMPLE));
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) { lo[c] = hi[c] = prev[c] = q[c]; e[c] = b[c]; }
    }
    uint32_t start = f0 + 1;
    auto close = [&](uint32_t end) {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) prev[c] = min(max(prev[c], lo[c]), hi[c]);
        for (uint32_t f = start; f < end; ++f) {
            SAMPLE *q = reinterpret_cast<SAMPLE *>(p + (uint64_t)f * frame_stride);
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c)
                if (c < channels) q[c] = (SAMPLE)prev[c];
        }
    };
    for (uint32_t f = f0 + 1; f < f1; ++f) {
        const SAMPLE *q = reinterpret_cast<const SAMPLE *>(p + (uint64_t)f * frame_stride);
        int32_t xl[4] = {0, 0, 0, 0}, xh[4] = {0, 0, 0, 0};
        bool empty = false;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < channels) {
                const int32_t x = q[c];
                xl[c] = max(0, x - e[c]);
                xh[c] = min(M, x + e[c]);
                empty |= max(lo[c], xl[c]) > min(hi[c], xh[c]);
            }
        if (empty) {
            close(f);
            start = f;
        }
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            lo[c] = empty ? xl[c] : max(lo[c], xl[c]);
            hi[c] = empty ? xh[c] : min(hi[c], xh[c]);
        }
    }
    close(f1);
}

}  // namespace rbf
