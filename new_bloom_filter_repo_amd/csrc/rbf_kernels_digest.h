// rbf_kernels_digest.h -- the integrity stage: FD1 frame digests (rbf_digest.h has the arithmetic, include/rbf.h the normative text) of
// frames that are resident anyway -- the coder's block after the hold, the decoder's chain block before its download.
//
// One wave hashes one 4096-byte block: lane l owns the 16 bytes at 1024 r + 16 l of each of the block's four rows (four coalesced
// 16-byte loads per block), runs its eight rounds, and the 64 accumulators fold in six shuffle steps.  merge is not commutative, so the
// fold order is the format's: lane l takes lane l + d for d = 1, 2, 4 ... 32.  A wave walks the blocks of ONE level of ONE frame
// (blockIdx.y) and writes one uint64 per block; the host launches the levels one after the other for all frames of the call, so a call
// is 1 + fd1_levels(frame_bytes) launches whatever the frame count.  The zero padding is never materialised: a lane past the end of its
// level contributes zeros.
#pragma once
#include "rbf_digest.h"
#include "rbf_kernels.h"
#include "rbf_lds_dma.h"

// Cache policy: plain loads.  At encode the block was just read by the hold and the mask stage and will be read again by the gather, at
// decode it was just written by the scatter: the bytes are in L2 / the Infinity Cache or about to be wanted there.  RBF_DIGEST_NT=1
// builds the fast path with non-temporal loads instead (the A/B of tools/frame_digest_leg.py; DESIGN.md section 6 has both figures).
#ifndef RBF_DIGEST_NT
#define RBF_DIGEST_NT 0
#endif

namespace rbf {

constexpr uint32_t FD1_BLOCKS_PER_WAVE = 4;     // what the host sizes the grid for: enough blocks per wave for the prefetch to matter

// The 16 bytes at `a` (any alignment) of the byte range [lo, hi), a >= lo: bytes at or behind hi read as zero and NOTHING outside
// [lo, hi) is touched -- a dword that lies inside the range whole is one load, the (at most two) dwords across its ends are put together
// from byte loads.  This is the generic path's loader and the fast path's for a level's last, partial vector.
__device__ __forceinline__ uint4 fd1_load_edge(const uint8_t *a, const uint8_t *lo, const uint8_t *hi)
{
    if (a >= hi) return make_uint4(0u, 0u, 0u, 0u);
    const uintptr_t A = (uintptr_t)a, LO = (uintptr_t)lo, HI = (uintptr_t)hi;
    const uint32_t sh = (uint32_t)(A & 3u);
    const uintptr_t a0 = A - sh;
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uintptr_t q = a0 + 4u * (uint32_t)k;
        w[k] = 0u;
        if (k == 4 && sh == 0u) continue;                        // an aligned vector is four dwords
        if (q >= LO && q + 4u <= HI) {
            w[k] = *reinterpret_cast<const uint32_t *>(q);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (q + (uint32_t)b >= LO && q + (uint32_t)b < HI) w[k] |= (uint32_t)*reinterpret_cast<const uint8_t *>(q + (uint32_t)b) << (8 * b);
        }
    }
    // (v_alignbyte_b32: the low dword of {w[k+1], w[k]} >> 8 sh)
    return make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], sh), __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                      __builtin_amdgcn_alignbyte(w[3], w[2], sh), __builtin_amdgcn_alignbyte(w[4], w[3], sh));
}

struct Fd1Block { uint4 v[FD1_ROWS]; };

// Lane `lane`'s four vectors of block j of the level [p, p + len).  ALIGNED (p a multiple of 16): a block that lies inside the level
// whole is four 16-byte loads, straight line; the level's last block tests every vector.
template <bool ALIGNED>
__device__ __forceinline__ void fd1_load_block(Fd1Block &b, const uint8_t *p, uint64_t len, uint64_t j, uint32_t lane)
{
    const uint64_t base = j * FD1_BLOCK_BYTES + 16u * lane;
    if (ALIGNED && (j + 1) * FD1_BLOCK_BYTES <= len) {
#pragma unroll
        for (uint32_t r = 0; r < FD1_ROWS; ++r) {
            const uint4 *q = reinterpret_cast<const uint4 *>(p + base + r * FD1_ROW_BYTES);
            b.v[r] = RBF_DIGEST_NT ? load_stream(q) : *q;
        }
        return;
    }
#pragma unroll
    for (uint32_t r = 0; r < FD1_ROWS; ++r) {
        const uint64_t o = base + r * FD1_ROW_BYTES;
        if (ALIGNED && o + 16u <= len) b.v[r] = *reinterpret_cast<const uint4 *>(p + o);
        else b.v[r] = o < len ? fd1_load_edge(p + o, p, p + len) : make_uint4(0u, 0u, 0u, 0u);
    }
}

// Level [src + y * src_stride, + len) of frame y = blockIdx.y, nblocks = fd1_blocks(len) blocks: dst[y * dst_stride + j] = hash of block
// j, seeded with j -- or, for the final block of a digest (top: nblocks == 1), with top_seed = the frame's length in bytes.
// Wave g of the grid's x dimension takes the blocks g, g + waves, g + 2 waves ...; the next block's four loads are issued before the
// current block's rounds.  ALIGNED: src and src_stride are multiples of 16 (fd1_load_block); <false> takes any layout, and the upper
// levels, whose arrays of block hashes are 8-byte aligned.
template <bool ALIGNED>
__global__ __launch_bounds__(WG_THREADS) void k_frame_digest(const uint8_t *__restrict__ src, uint64_t src_stride, uint64_t len, uint64_t nblocks,
                                                             uint32_t top, uint64_t top_seed, uint64_t *__restrict__ dst, uint64_t dst_stride)
{
    const uint32_t lane = threadIdx.x & 63u, waves_wg = blockDim.x >> 6;
    const uint64_t step = (uint64_t)gridDim.x * waves_wg;
    uint64_t j = (uint64_t)blockIdx.x * waves_wg + (threadIdx.x >> 6);
    if (j >= nblocks) return;
    const uint8_t *const p = src + (uint64_t)blockIdx.y * src_stride;
    uint64_t *const out = dst + (uint64_t)blockIdx.y * dst_stride;
    Fd1Block cur, nxt;
    fd1_load_block<ALIGNED>(cur, p, len, j, lane);
    for (; j < nblocks; j += step) {
        const bool more = j + step < nblocks;                    // (wave-uniform)
        if (more) fd1_load_block<ALIGNED>(nxt, p, len, j + step, lane);
        uint64_t acc = fd1_lane_seed(top ? top_seed : j, lane);
#pragma unroll
        for (uint32_t r = 0; r < FD1_ROWS; ++r) {
            acc = fd1_round(acc, (uint64_t)cur.v[r].x | ((uint64_t)cur.v[r].y << 32));
            acc = fd1_round(acc, (uint64_t)cur.v[r].z | ((uint64_t)cur.v[r].w << 32));
        }
#pragma unroll
        for (uint32_t d = 1; d < FD1_LANES; d *= 2)              // only the lanes that are multiples of 2d carry a meaningful value on
            acc = fd1_merge(acc, (uint64_t)__shfl_down((unsigned long long)acc, d));
        if (lane == 0) out[j] = fd1_aval(acc);
        if (more) cur = nxt;
    }
}

}  // namespace rbf
