// rbf_kernels_keyquant.h -- bounded-error keyframes (record type 7, ImprovedVideoCompressor(bounded_keyframes=True)): a keyframe of a
// resident block is rebuilt within its channel's bound d instead of exactly, and the residuals the Rice coder sees shrink by the step
// t = 2d + 1.  The rule is normative (include/rbf.h) and is stated as a quantiser inside the keyframe predictor's loop: raster order,
// an integer state S per sample,
//   P(y, x) = S(y, x-1); P(y, 0) = S(y-1, 0); P(0, 0) = 0        (per channel: the type-3 neighbours)
//   d >= 1: e = X - P, q = sgn(e) * floor((|e| + d) / t), S = P + q t, Y = clamp(S, 0, 2^B - 1)
//   d == 0: q = (X - P) mod 2^B as B-bit two's complement, S = Y = X
//   u = 2q (q >= 0) or -2q - 1: rice_map of q's low B bits -- |q| <= (2^B + 1) / 3 < 2^(B-1)
// THE LOOP HAS A CLOSED FORM, which is what the encoder runs.  The chain starts at P = 0 and every step adds a multiple of t, so every
// P is a multiple of t; q is e / t rounded to the nearest integer (t is odd: no ties), hence S = P + t round((X - P) / t) =
// t round(X / t) = t I(X) with the lattice index I(X) = floor((X + d) / t), whatever the neighbours are, and q = I(X) - I(X_pred).
// (So S is never negative: the rule's lower clamp cannot bind; the upper one binds where a multiple of t lies in (2^B - 1, 2^B - 1 + d].)
// The encoder is therefore the type-3 producer k_rice_intra_u on the index image -- one lane per sample, no chain -- and the
// tests hold it against a twin that walks the loop as the rule states it.  I(Y) = I(X): the rule is idempotent.
// Encode: k_keyquant_u writes the u values into the sample coder's dense buffer (rbf_kernels_rice.h: cost -> scan -> headers -> write
// follow unchanged) from the frames as they are, then k_keyquant_apply writes Y over X -- a launch of its own, so that no lane reads a
// neighbour another lane is writing.  Decode: k_rice_decode, then k_keyquant_rebuild, the sibling of k_rice_intra_rebuild: prefix
// sums of q t in 32-bit wrap-around arithmetic (every true partial sum is in [0, 2^B - 1 + d]), then the clamp (d >= 1) or the mask
// (d == 0).  No atomics; the result is a pure function of (X, d).
#pragma once
#include "rbf_kernels_rice.h"

namespace rbf {

// Per channel: bound, step, and the step's reciprocal.  floor(n / t) = mulhi(n, m) >> sh for every n < 2^18 (the numerators are
// X + d < 2^17): with L = floor(log2 t) >= 1 (t is odd and >= 3), K = 31 + L and m = ceil(2^K / t) <= 2^31 + 1, m t = 2^K + r with
// 0 <= r < t, so n m / 2^K = n / t + n r / (t 2^K) and n r < 2^18 2^(L+1) <= 2^K: the excess is below 1 / t and the floor is that of
// n / t.  sh = K - 32 = L - 1.  (tests/test_near_keyframes_cpu.py restates it in integers over the whole range.)  d == 0: m = sh = 0.
struct KeyQuant {
    uint32_t d[4], t[4], m[4], sh[4];
};

struct KeyQuantChannel { uint32_t d, t, m, sh; };

__device__ __forceinline__ KeyQuantChannel keyquant_channel(const KeyQuant &kq, uint32_t c)
{
    auto pick = [c](const uint32_t (&v)[4]) { return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : v[3]; };      // (selects: no indexed copy of the table)
    return KeyQuantChannel{pick(kq.d), pick(kq.t), pick(kq.m), pick(kq.sh)};
}

// the lattice index of a sample: floor((x + d) / t); an exact channel's index is the sample
__device__ __forceinline__ uint32_t keyquant_index(uint32_t x, const KeyQuantChannel &k)
{
    return k.d ? __umulhi(x + k.d, k.m) >> k.sh : x;
}

// Producer: u of every sample of the `count` listed frames of a dense block, k_rice_intra_u's indexing and neighbours on the lattice
// indices; stream k's values start at u[k * height * width * channels].  Reads only.  grid (ceil(W*C / 256), H, count).
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_keyquant_u(
    const uint8_t *__restrict__ frames, uint64_t frame_stride, const uint32_t *__restrict__ frame_index, uint32_t width, uint32_t channels,
    KeyQuant kq, uint16_t *__restrict__ u)
{
    const uint64_t row = (uint64_t)width * channels;
    const uint64_t col = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (col >= row) return;
    const uint32_t y = blockIdx.y, f = blockIdx.z;
    const SAMPLE *x = (const SAMPLE *)(frames + (uint64_t)frame_index[f] * frame_stride);
    const KeyQuantChannel k = keyquant_channel(kq, (uint32_t)(col % channels));
    const uint64_t i = (uint64_t)y * row + col;
    uint32_t pred = 0;
    if (col >= channels) pred = keyquant_index(x[i - channels], k);
    else if (y > 0) pred = keyquant_index(x[i - row], k);
    u[(uint64_t)f * row * gridDim.y + i] = (uint16_t)rice_map(keyquant_index(x[i], k) - pred, 8 * sizeof(SAMPLE));
}

// Y over X in the listed frames: min(I(X) t, 2^B - 1); an exact channel is left alone.  Same grid; a lane writes the sample it read.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_keyquant_apply(
    uint8_t *__restrict__ frames, uint64_t frame_stride, const uint32_t *__restrict__ frame_index, uint32_t width, uint32_t channels, KeyQuant kq)
{
    const uint64_t row = (uint64_t)width * channels;
    const uint64_t col = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (col >= row) return;
    SAMPLE *x = (SAMPLE *)(frames + (uint64_t)frame_index[blockIdx.z] * frame_stride) + (uint64_t)blockIdx.y * row + col;
    const KeyQuantChannel k = keyquant_channel(kq, (uint32_t)(col % channels));
    if (k.d) *x = (SAMPLE)min(keyquant_index(*x, k) * k.t, (1u << (8 * sizeof(SAMPLE))) - 1u);
}

// Decode, one wave per row (k_rice_intra_rebuild's shape): q = s read as B-bit two's complement; S(y, 0) = the sum of q t down column 0
// over rows 0..y, S(y, x) = S(y, 0) + q t of columns 1..x as a running inclusive scan over 64-pixel tiles; Y = clamp(S) where d >= 1,
// S mod 2^B where d == 0.  Whatever the stream holds, only out[0 .. height * width * channels) is written.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_keyquant_rebuild(
    const uint16_t *__restrict__ s, uint32_t width, uint32_t height, uint32_t channels, KeyQuant kq, SAMPLE *__restrict__ out)
{
    constexpr uint32_t B = 8 * sizeof(SAMPLE), bmask = (1u << B) - 1u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t y = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    if (y >= height) return;
    const uint64_t row = (uint64_t)width * channels;
    auto term = [](uint32_t v, uint32_t t) { return (uint32_t)(((int32_t)(v << (32 - B)) >> (32 - B)) * (int32_t)t); };
    uint32_t col0[4] = {0, 0, 0, 0}, carry[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        if (c < channels) {
            uint32_t acc = 0;
            for (uint32_t r = lane; r <= y; r += WAVE) acc += term(s[(uint64_t)r * row + c], kq.t[c]);
            col0[c] = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_lane63(acc), 63);
        }
    }
    const uint16_t *srow = s + (uint64_t)y * row;
    SAMPLE *orow = out + (uint64_t)y * row;
    for (uint32_t x0 = 0; x0 < width; x0 += WAVE) {
        const uint32_t x = x0 + lane;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            if (c < channels) {
                const uint32_t v = x == 0 ? col0[c] : (x < width ? term(srow[(uint64_t)x * channels + c], kq.t[c]) : 0u);
                const uint32_t incl = wave_inclusive_scan(v) + carry[c];
                if (x < width)
                    orow[(uint64_t)x * channels + c] = (SAMPLE)(kq.d[c] ? (uint32_t)min(max((int32_t)incl, 0), (int32_t)bmask) : incl & bmask);
                carry[c] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        }
    }
}

}  // namespace rbf
