// rbf_kernels_reduce.h -- from partial filters to what the query reads: k_filter_reduce ORs the partial filters the insert kernels of
// every family leave behind (rbf_kernels_barrett.h, rbf_kernels_insert_f64.h) into the packed filter, counts its set bits and, for the FP64
// query kernels, writes the probe image (rbf_f64_common.h) next to it; k_probe_image makes that image from a caller's filters (decode).
#pragma once
#include "rbf_kernels.h"
#include "rbf_lds_dma.h"

namespace rbf {

// OR the S partial filters of every frame into the final packed filter; count its set bits.
// 16-byte accesses (rows are 8-byte padded and 16-byte aligned bases are not guaranteed, so the
// vector path is taken only when both strides are multiples of 4 words and the bases are aligned).
template <bool STREAM>
__global__ __launch_bounds__(WG_THREADS) void k_filter_reduce(
    const uint32_t *partials, uint64_t part_stride_words32, uint32_t Smax /* row pitch of the partials, in slices */,
    const SliceTable slices /* partial filters per frame */,
    const FrameTable tab,
    uint32_t *filters /* may alias partials when Smax == 1 */, uint64_t filter_stride_words32,
    uint64_t *__restrict__ stats, uint32_t vec_ok,
    uint32_t *__restrict__ image /* nullable: probe image rows (~bswap of every dword) for the FP64 query kernel */, uint64_t image_stride_words32)
{
    __shared__ uint32_t red[WG_WAVES];
    const uint32_t f = blockIdx.y;
    const uint32_t S = slices.n[f];
    const uint32_t m = tab.f[f].m;
    const uint32_t fwords = m ? filter_words(m) : 0u;
    uint32_t *filt = filters + (uint64_t)f * filter_stride_words32;
    const uint32_t *part = partials + (uint64_t)f * Smax * part_stride_words32;
    uint32_t pc = 0;
    if (vec_ok) {
        const uint64_t quads = filter_stride_words32 >> 2;
        for (uint64_t q = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * WG_THREADS) {
            const uint64_t w = q << 2;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w < fwords) {
                // eight partials in flight (clamped slice index: a repeated partial ORs in nothing new); one load per loop
                // iteration waits for each L2 round trip in turn
                for (uint32_t s0 = 0; s0 < S; s0 += 8) {
                    uint4 x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t sj = s0 + j < S ? s0 + j : S - 1;
                        const uint4 *src = reinterpret_cast<const uint4 *>(part + (uint64_t)sj * part_stride_words32 + w);
                        x[j] = STREAM ? load_stream(src) : *src;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) { v.x |= x[j].x; v.y |= x[j].y; v.z |= x[j].z; v.w |= x[j].w; }
                }
                if (w + 1 >= fwords) v.y = 0;                    // words past the filter end hold LDS padding
                if (w + 2 >= fwords) v.z = 0;
                if (w + 3 >= fwords) v.w = 0;
            }
            if (m) {                                             // passthrough frames: filter untouched
                if (STREAM) store_stream(reinterpret_cast<uint4 *>(filt + w), v); else *reinterpret_cast<uint4 *>(filt + w) = v;
            }
            if (image && w < image_stride_words32)
                *reinterpret_cast<uint4 *>(image + (uint64_t)f * image_stride_words32 + w) =
                    make_uint4(~__builtin_bswap32(v.x), ~__builtin_bswap32(v.y), ~__builtin_bswap32(v.z), ~__builtin_bswap32(v.w));
            pc += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        }
    } else {
        for (uint64_t w = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; w < filter_stride_words32; w += (uint64_t)gridDim.x * WG_THREADS) {
            uint32_t v = 0;
            if (w < fwords)
                for (uint32_t s = 0; s < S; ++s) v |= part[(uint64_t)s * part_stride_words32 + w];
            if (m) filt[w] = v;
            if (image && w < image_stride_words32) image[(uint64_t)f * image_stride_words32 + w] = ~__builtin_bswap32(v);
            pc += __popc(v);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pc += __shfl_down(pc, d);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = pc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < WG_WAVES; ++k) t += red[k];
        if (t) atomicAdd((unsigned long long *)&stats[(uint64_t)f * 4 + 1], (unsigned long long)t);
    }
}

// Probe image of caller-supplied packed filters (decode): image[f][w] = ~bswap(filters[f][w]).
__global__ __launch_bounds__(WG_THREADS) void k_probe_image(const uint32_t *__restrict__ filters, uint64_t filter_stride_words32,
                                                            uint32_t *__restrict__ image, uint64_t image_stride_words32)
{
    const uint32_t f = blockIdx.y;
    for (uint64_t w = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; w < image_stride_words32; w += (uint64_t)gridDim.x * WG_THREADS)
        image[(uint64_t)f * image_stride_words32 + w] = w < filter_stride_words32 ? ~__builtin_bswap32(filters[(uint64_t)f * filter_stride_words32 + w]) : ~0u;
}

}  // namespace rbf
