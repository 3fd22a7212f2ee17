// rbf_lds_dma.h -- how the LDS kernels move data without registers or cache pollution: non-temporal accesses for one-shot streams
// (the cache-policy note below), the wave-level LDS fence, and LDS-DMA (global_load_lds_*) of a filter, a tile or an image row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rbf {

// Cache policy for data that is read or written ONCE.  A step of several GOPs moves ~750 MB through 32 MB of L2 and the 256 MB Infinity
// Cache, next to two things that must stay cached: the pixel-index hash table the insert gathers from (54 MB) and the probe images every
// query workgroup restages.  Non-temporal loads / stores keep the one-shot streams from evicting them.  Measured (profiles/r05_cache_policy.txt,
// four pipelines): the mask kernel's frame loads alone +2.6 % at one GOP per call and +1.6 % at four; with the witness-row clears (since
// removed altogether), the reduce kernel's partial loads and filter stores and the compaction's pass-word and mask loads +5.4 % at four GOPs
// per call, +3.8 % at three, nothing at two, -1 % at one (so those follow the batch size: STREAM).  The query kernel's pass-byte stores and the compaction's
// witness stores must NOT stream (-2 ... -3 %: their consumers follow at once), nor the table gathers (insert 33 -> 55 us).
typedef uint32_t nt_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_stream(uint4 *p, uint4 v) { const nt_u32x4 x = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(x, reinterpret_cast<nt_u32x4 *>(p)); }
__device__ __forceinline__ uint4 load_stream(const uint4 *p) { const nt_u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4 *>(p)); return make_uint4(x.x, x.y, x.z, x.w); }

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- LDS-DMA ---------------------------------------------------------------------------------------------------------
// Filter staging by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, no VGPRs, no
// ds_write pass).  LDS destination = M0 (wave-uniform base) + lane*16; the global source is per lane.
//
// The DMA is issued from inline asm ON PURPOSE: when hipcc sees the builtin it cannot tell the DMA's
// LDS destination (the *other* buffer) from the probes' source, so it drains vmcnt(0) in front of
// every LDS access of the compute phase and the double buffering buys nothing (measured: 35 us of
// a 183 us launch).  Asm DMAs are invisible to its scoreboard; completion is waited for explicitly
// with dma_wait_all() right before the workgroup barrier that hands the buffer over.
__device__ __forceinline__ void dma16(const uint32_t *gsrc, uint32_t lds_byte_addr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
__device__ __forceinline__ void dma4(const uint32_t *gsrc, uint32_t lds_byte_addr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dword %1, off\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t lds_addr_of(const uint32_t *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t *)p;
}

__device__ __forceinline__ void dma_filter(uint32_t *lds_dst, const uint32_t *src, uint32_t words, uint32_t wave,
                                           uint32_t lane, uint32_t nwaves)
{
    const uint32_t base = __builtin_amdgcn_readfirstlane(lds_addr_of(lds_dst));
    const uint32_t npieces = words >> 2;                      // whole 16-byte pieces
    const uint32_t nchunks = (npieces + 63u) >> 6;
    for (uint32_t c = wave; c < nchunks; c += nwaves) {
        const uint32_t piece = (c << 6) + lane;
        if (piece < npieces) dma16(src + (piece << 2), __builtin_amdgcn_readfirstlane(base + (c << 10)));
    }
    const uint32_t tail = words & 3u;                         // 0..3 dwords left: 4-byte DMA
    if (wave == 0 && lane < tail) dma4(src + (npieces << 2) + lane, __builtin_amdgcn_readfirstlane(base + (npieces << 4)));
}

// An image row (the FP64 kernels):
// `words` dwords of `row` -> LDS at lds_byte_addr, 1 KiB (one 16-byte piece per lane) per wave and step, the row pointer in an SGPR
// pair (saddr addressing: the VGPR holds a 32-bit byte offset), bounds tested only on the row's last piece.  M0 is saved and
// restored inside the asm block (a reserved register: the compiler rejects it as a clobber).  Completion: dma_wait_all().
__device__ __forceinline__ void dma_row(uint32_t lds_byte_addr /* uniform */, const uint32_t *row /* uniform */, uint32_t words, uint32_t wave, uint32_t lane, uint32_t nwaves)
{
    const uint32_t npieces = words >> 2;                          // whole 16-byte pieces
    const uint32_t lane_off = lane << 4;
    for (uint32_t c = wave; (c << 6) < npieces; c += nwaves) {
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr + (c << 10));
        const uint32_t off = lane_off + (c << 10);
        if ((c << 6) + 64u <= npieces || (c << 6) + lane < npieces) {
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(off), "s"(row) : "memory");
        }
    }
    const uint32_t tail = words & 3u;                             // 0..3 dwords left: 4-byte DMA by wave 0
    if (wave == 0 && lane < tail) {
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr + (npieces << 4));
        const uint32_t off = (npieces << 4) + (lane << 2);
        uint32_t keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, %3\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(dst), "v"(off), "s"(row) : "memory");
    }
}

}  // namespace rbf
