// rbf_kernels_view.h -- views of resident dense frames (k_frame_view, its per-sample twin k_frame_view_px): a region of every listed frame
// of a block, reduced by a box mean over s x s blocks, written back to back.  include/rbf.h (rbf_frame_view_batch) has the normative
// text, rbf_view.h the arithmetic both kernels and the host twin share:
//   output pixel (Y, X) covers x0 + sX .. min(x0 + sX + s, x0 + w) - 1 by y0 + sY .. min(y0 + sY + s, y0 + h) - 1, cnt pixels
//   per channel  out = floor((2 sum + cnt) / (2 cnt));  a full block: (sum + s^2/2) >> 2 log2 s;  s = 1: a crop
// The kernels only read the frames; frame j of the call is frame index[j] of the block, blockIdx.y = j.  A read-mostly, memory-bound
// pass: no LDS, no atomics, no scratch; every source byte inside the region is read once, every output sample written once.
#pragma once
#include "rbf_geometry.h"
#include "rbf_view.h"

namespace rbf {

// sample i of a lane's source row held as dwords (i is a compile-time constant after unrolling)
template <typename SAMPLE>
__device__ __forceinline__ uint32_t view_sample(const uint32_t *d, int i)
{
    if (sizeof(SAMPLE) == 2) return (d[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// The wide kernel: lane (Y, tx) owns the T = view_tile_pixels(S, pixel bytes) output pixels tx T .. tx T + T - 1 of output row Y -- full
// blocks only -- and reads their T S source pixels of each of the S source rows as whole 16-byte vectors (one to four per row).
// Requires every source row it touches to start on a 16-byte boundary (view_plan: base, frame stride, row bytes and the region's byte
// offset in a row are multiples of 16), tiles_x * T * S <= roi_w and wide_rows * S <= roi_h.  roi_off: the byte offset of the region's
// corner in a frame.  The T C results leave as dwords when the lane's output bytes are whole aligned dwords, else sample by sample.
template <typename SAMPLE, int C, int S>
__global__ __launch_bounds__(WG_THREADS) void k_frame_view(const uint8_t *__restrict__ frames, uint64_t frame_stride,
                                                           const uint32_t *__restrict__ index, uint32_t row_bytes, uint64_t roi_off,
                                                           uint32_t tiles_x, uint32_t wide_rows, uint8_t *__restrict__ out,
                                                           uint64_t view_bytes, uint32_t out_row_bytes)
{
    constexpr int PB = C * (int)sizeof(SAMPLE), T = (int)view_tile_pixels(S, PB), VEC = (int)view_tile_vectors(S, PB), N = T * C;
    constexpr uint32_t L2 = view_log2(S);
    static_assert(VEC * 16 == T * S * PB && VEC <= 4, "a lane's source pixels of a row are whole 16-byte vectors");
    const uint64_t id = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (id >= (uint64_t)tiles_x * wide_rows) return;
    const uint32_t Y = (uint32_t)(id / tiles_x), tx = (uint32_t)(id % tiles_x);
    const uint8_t *src = frames + (uint64_t)index[blockIdx.y] * frame_stride + roi_off + (uint64_t)Y * S * row_bytes + (uint64_t)tx * (VEC * 16);
    uint32_t acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0;
#pragma unroll
    for (int dy = 0; dy < S; ++dy) {
        uint32_t d[VEC * 4];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const uint4 q = reinterpret_cast<const uint4 *>(src + (uint64_t)dy * row_bytes)[v];
            d[4 * v] = q.x; d[4 * v + 1] = q.y; d[4 * v + 2] = q.z; d[4 * v + 3] = q.w;
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int dx = 0; dx < S; ++dx)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[t * C + c] += view_sample<SAMPLE>(d, (t * S + dx) * C + c);
    }
    uint8_t *dst = out + (uint64_t)blockIdx.y * view_bytes + (uint64_t)Y * out_row_bytes + (uint64_t)tx * (T * PB);
    constexpr int PER = 4 / (int)sizeof(SAMPLE);                   // samples of a dword
    if ((T * PB) % 4 == 0 && (uintptr_t)dst % 4 == 0) {
#pragma unroll
        for (int w = 0; w < (T * PB) / 4; ++w) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < PER; ++k) word |= view_round_full(acc[w * PER + k], L2) << (8 * (int)sizeof(SAMPLE) * k);
            reinterpret_cast<uint32_t *>(dst)[w] = word;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) reinterpret_cast<SAMPLE *>(dst)[i] = (SAMPLE)view_round_full(acc[i], L2);
    }
}

// The plain path: a lane owns ONE output sample (Y, X, c) and reads its block sample by sample, so nothing needs more than the samples'
// own alignment.  A launch covers the rectangle of output pixels X in [rx, rx + rw), Y in [ry, ry + rh) and nothing else: the entry
// launches it over what the wide kernel does not take -- the columns behind the last whole tile, the ragged last rows -- or over the
// whole view of a tiny frame, an unaligned region or layout.
template <typename SAMPLE, int S>
__global__ __launch_bounds__(WG_THREADS) void k_frame_view_px(const uint8_t *__restrict__ frames, uint64_t frame_stride,
                                                              const uint32_t *__restrict__ index, uint32_t width, uint32_t channels,
                                                              uint32_t x0, uint32_t y0, uint32_t roi_w, uint32_t roi_h, uint32_t out_w,
                                                              uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh,
                                                              uint8_t *__restrict__ out, uint64_t view_bytes)
{
    constexpr uint32_t L2 = view_log2(S);
    const uint64_t id = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (id >= (uint64_t)rh * rw * channels) return;
    const uint32_t c = (uint32_t)(id % channels);
    const uint64_t px = id / channels;
    const uint32_t X = rx + (uint32_t)(px % rw), Y = ry + (uint32_t)(px / rw);
    const uint32_t bw = view_block_len(roi_w, S, X), bh = view_block_len(roi_h, S, Y);
    const SAMPLE *p = reinterpret_cast<const SAMPLE *>(frames + (uint64_t)index[blockIdx.y] * frame_stride) +
                      ((uint64_t)(y0 + (uint64_t)S * Y) * width + x0 + (uint64_t)S * X) * channels + c;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t dy = 0; dy < (uint32_t)S; ++dy)
        if (dy < bh) {
#pragma unroll
            for (uint32_t dx = 0; dx < (uint32_t)S; ++dx)
                if (dx < bw) sum += p[((uint64_t)dy * width + dx) * channels];
        }
    reinterpret_cast<SAMPLE *>(out + (uint64_t)blockIdx.y * view_bytes)[((uint64_t)Y * out_w + X) * channels + c] =
        (SAMPLE)(bw * bh == (uint32_t)(S * S) ? view_round_full(sum, L2) : view_round(sum, bw * bh));
}

}  // namespace rbf
