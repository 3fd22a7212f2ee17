// rbf_view.h -- the index arithmetic of a frame view (include/rbf.h, rbf_frame_view_batch, has the normative text), shared by the kernels
// (rbf_kernels_view.h), the entry's launch plan, the host twin below and the CPU check (tests/c/view_cases.cpp).  No HIP header: any
// C++17 host compiler takes it; under hipcc the small functions are __host__ __device__, so the device runs the very lines the CPU check
// pins.
//
//   a view of a dense (H, W, C) frame: a region (x0, y0, w, h) with w, h >= 1, x0 + w <= W, y0 + h <= H, and a scale s in {1, 2, 4, 8}
//   output: dense (ceil(h/s), ceil(w/s), C); the block grid hangs off the region's corner
//   output pixel (Y, X) covers x0 + sX .. min(x0 + sX + s, x0 + w) - 1 by y0 + sY .. min(y0 + sY + s, y0 + h) - 1: cnt pixels
//   per channel  out = floor((2 sum + cnt) / (2 cnt))   -- half rounds up; a full block: (sum + s^2/2) >> 2 log2 s; s = 1: a crop
//   the largest numerator is 2 * 64 * 65535 + 64: 32 bits are enough
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RBF_VIEW_HD __host__ __device__ inline
#else
#define RBF_VIEW_HD inline
#endif

namespace rbf {

RBF_VIEW_HD constexpr bool view_scale_ok(uint32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }
RBF_VIEW_HD constexpr uint32_t view_log2(uint32_t s) { return s >= 8 ? 3 : s >= 4 ? 2 : s >= 2 ? 1 : 0; }
// output pixels along a region side of `len` source pixels
RBF_VIEW_HD constexpr uint32_t view_out_dim(uint32_t len, uint32_t s) { return (uint32_t)(((uint64_t)len + s - 1) / s); }
// source pixels block X of a side of `len` pixels has: s, or what is left in the ragged last block
RBF_VIEW_HD constexpr uint32_t view_block_len(uint32_t len, uint32_t s, uint32_t X)
{
    const uint64_t left = (uint64_t)len - (uint64_t)s * X;
    return left < s ? (uint32_t)left : s;
}
// the mean of cnt (1..64) samples that sum to `sum`, half rounding up
RBF_VIEW_HD constexpr uint32_t view_round(uint32_t sum, uint32_t cnt) { return (2u * sum + cnt) / (2u * cnt); }
// ... of a full block of s x s samples: the same number without the division
RBF_VIEW_HD constexpr uint32_t view_round_full(uint32_t sum, uint32_t log2s) { return (sum + ((1u << (2 * log2s)) >> 1)) >> (2 * log2s); }

// ---- the wide kernel's tiles.  A lane of k_frame_view owns `tile` output pixels of one output row: tile * s source pixels of each of s
// source rows, a whole number of 16-byte vectors -- tile = 16 / gcd(16, s * pixel_bytes), at most four vectors per row.
RBF_VIEW_HD constexpr uint32_t view_gcd(uint32_t a, uint32_t b) { return b == 0 ? a : view_gcd(b, a % b); }
RBF_VIEW_HD constexpr uint32_t view_tile_pixels(uint32_t s, uint32_t pixel_bytes) { return 16u / view_gcd(16u, s * pixel_bytes); }
RBF_VIEW_HD constexpr uint32_t view_tile_vectors(uint32_t s, uint32_t pixel_bytes) { return view_tile_pixels(s, pixel_bytes) * s * pixel_bytes / 16u; }

// What the two kernels of a call cover.  The wide kernel takes the output pixels X < wide_cols, Y < wide_rows -- full blocks only, in
// whole tiles -- when every source row it touches starts on a 16-byte boundary: base and frame stride (aligned16), the frame's row bytes
// and the region's byte offset in a row are all multiples of 16.  The per-sample kernel takes every other output pixel: the columns
// behind the last whole tile, the ragged last row and column of blocks, and the whole view of any other layout.
struct ViewPlan {
    uint32_t out_w, out_h;           // the view
    uint32_t tile, tiles_x;          // output pixels per lane of the wide kernel; its lanes per output row (0: no wide launch)
    uint32_t wide_cols, wide_rows;   // tiles_x * tile; the output rows of full blocks (0 when tiles_x is)
};

inline ViewPlan view_plan(uint32_t width, uint32_t pixel_bytes, uint32_t x0, uint32_t roi_w, uint32_t roi_h, uint32_t s, bool aligned16)
{
    ViewPlan p{};
    p.out_w = view_out_dim(roi_w, s);
    p.out_h = view_out_dim(roi_h, s);
    p.tile = view_tile_pixels(s, pixel_bytes);
    const bool rows16 = aligned16 && ((uint64_t)width * pixel_bytes) % 16 == 0 && ((uint64_t)x0 * pixel_bytes) % 16 == 0;
    p.tiles_x = rows16 ? (roi_w / s) / p.tile : 0;
    p.wide_rows = p.tiles_x ? roi_h / s : 0;
    if (p.wide_rows == 0) p.tiles_x = 0;
    p.wide_cols = p.tiles_x * p.tile;
    return p;
}

// ---- the host twin: the view of one dense frame, block by block (a little-endian host, as everything at this ABI)
template <typename SAMPLE>
inline void view_frame_host(const SAMPLE *src, uint32_t width, uint32_t channels, uint32_t x0, uint32_t y0, uint32_t roi_w, uint32_t roi_h,
                            uint32_t s, SAMPLE *dst)
{
    const uint32_t ow = view_out_dim(roi_w, s), oh = view_out_dim(roi_h, s);
    for (uint32_t Y = 0; Y < oh; ++Y)
        for (uint32_t X = 0; X < ow; ++X) {
            const uint32_t bw = view_block_len(roi_w, s, X), bh = view_block_len(roi_h, s, Y);
            for (uint32_t c = 0; c < channels; ++c) {
                uint32_t sum = 0;
                for (uint32_t dy = 0; dy < bh; ++dy)
                    for (uint32_t dx = 0; dx < bw; ++dx)
                        sum += src[((size_t)(y0 + s * Y + dy) * width + (x0 + s * X + dx)) * channels + c];
                dst[((size_t)Y * ow + X) * channels + c] = (SAMPLE)view_round(sum, bw * bh);
            }
        }
}

}  // namespace rbf
