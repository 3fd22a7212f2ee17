// rbf_kernels_mask.h -- the GOP mask stage (A1): residual masks of a whole GOP with every frame read once (k_residual_mask_gop, its
// all-channel twin k_residual_mask_any_gop; one body, rbf_kernels_mask_body.h), the per-lane bit extraction they are built on, the
// chunk table and fused finish they take as arguments, and the two small kernels around them (k_store_thresholds, k_finish_ones).
#pragma once
#include "rbf_kernels.h"
#include "rbf_mask_plan.h"

namespace rbf {

// ------------------------------------------------------------------------------------------
// A1 fast path: residual masks of a whole GOP, every frame read from HBM exactly once.
// ------------------------------------------------------------------------------------------
// Frames must be flat (row pitch == width * pixel stride), so a frame is an array of n pixels of
// PIXEL_BYTES each whose first sample is the luma.  A lane owns 16 consecutive pixels for the
// whole GOP: it keeps the previous frame's 16*PIXEL_BYTES bytes in registers, streams the next
// frame's with 16-byte loads (two frames of prefetch in flight), and emits its 16 mask bits as one
// MSB-first uint16, so a wave writes 128 contiguous bytes per frame and needs no ballot.
template <typename SAMPLE, int PIXEL_BYTES>
struct LanePixels {
    static constexpr int DW = 16 * PIXEL_BYTES / 4;            // dwords per lane per frame
    uint32_t d[DW];
    template <bool NT>
    __device__ __forceinline__ void load(const uint8_t *p)
    {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int i = 0; i < DW / 4; ++i) {
            const u32x4 v = NT ? __builtin_nontemporal_load(q + i) : q[i];
            d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
        }
    }
    __device__ __forceinline__ uint32_t luma(int k) const     // sample 0 of pixel k
    {
        const int byte = k * PIXEL_BYTES;
        const uint32_t w = d[byte >> 2];
        if (sizeof(SAMPLE) == 1) return (w >> (8 * (byte & 3))) & 0xFFu;
        return (w >> (8 * (byte & 3))) & 0xFFFFu;              // 2-byte samples are 2-byte aligned
    }
};

// Threshold 0 (the lossless setting, verify_true_lossless.py:244-246): the bit is "luma changed", which needs no
// per-pixel extraction.  8-bit: XOR whole dwords, pull the luma bytes of four pixels into one dword (v_perm), turn
// "byte != 0" into the byte's top bit with the carry trick and squeeze the four flags into a nibble with one
// multiply: ~3 instructions per pixel instead of ~10.  16-bit: numpy's int16 arithmetic makes abs(a - b) > 0 false for
// a - b == 0 AND for a - b == 0x8000 (abs(-32768) stays negative, :801), i.e. exactly when a and b agree in their LOW 15 BITS -- so
// the bit is ((a ^ b) & 0x7FFF) != 0 and no subtraction is needed.  Planar 16-bit luma (BASELINE config 5): per dword (two pixels) one
// v_bitop3 ((a ^ b) & 0x7FFF7FFF), one v_pk_min_u16 against 0x00010001 (the two flags at bits 0 and 16) and one v_lshl_or into an
// accumulator whose halves interleave at the end: 26 vector instructions per 16 pixels (round 5's v_pk_sub / carry / shift chain: 62).
// `count_src`: a value with the same population count as the returned bits (the 16-bit path's accumulator: no masking needed).
// `one2`: 1 in both halves, made by the caller ONCE with an asm v_mov -- the compiler turns a visible min(t, 1) into v_cmp + v_cndmask
// through VCC (21 cycles a pair, profiles/r04_opbench2.txt), hence also the asm v_pk_min_u16.
template <typename SAMPLE, int PIXEL_BYTES>
__device__ __forceinline__ uint32_t lane_bits_thr0(const LanePixels<SAMPLE, PIXEL_BYTES> &a, const LanePixels<SAMPLE, PIXEL_BYTES> &b, uint32_t one2, uint32_t &count_src)
{
    uint32_t bits = 0;
    if (sizeof(SAMPLE) == 1) {
        constexpr int shift_of_group[4] = {4, 0, 12, 8};       // pixels 4g..4g+3 -> bits (k ^ 7), MSB-first per byte
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t z;
            if (PIXEL_BYTES == 1) z = a.d[g] ^ b.d[g];
            else {                                              // 3-byte pixels: lumas at bytes 0, 3, 6, 9 of three dwords
                const uint32_t x0 = a.d[3 * g] ^ b.d[3 * g], x1 = a.d[3 * g + 1] ^ b.d[3 * g + 1], x2 = a.d[3 * g + 2] ^ b.d[3 * g + 2];
                const uint32_t y = __builtin_amdgcn_perm(x1, x0, 0x00060300u);   // {x0.b0, x0.b3, x1.b2, -}
                z = __builtin_amdgcn_perm(x2, y, 0x05020100u);                   // {.., .., .., x2.b1}
            }
            const uint32_t f = (((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;   // top bit of every non-zero byte
            bits |= (((f >> 7) * 0x08040201u) >> 24) << shift_of_group[g];            // flags at 0,8,16,24 -> 27,26,25,24
        }
        count_src = bits;
    } else if (PIXEL_BYTES == 2) {
        const uint32_t k7 = 0x7FFF7FFFu;
        // dword j's flags: pixel 2j at bit 2 (j ^ 3), pixel 2j+1 16 bits above (one2: 0x00010001 in a VGPR the compiler cannot see through: see the kernel)
        uint32_t acc = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int j = s ^ 4;                                // order 4,5,6,7,0,1,2,3: the first dword ends up highest
            const uint32_t t = (a.d[j] ^ b.d[j]) & k7;
            uint32_t g;
            asm("v_pk_min_u16 %0, %1, %2" : "=v"(g) : "v"(t), "v"(one2));
            acc = (acc << 2) | g;
        }
        bits = (acc >> 16) | (acc << 1);                        // pixel 2j -> odd bit (2j) ^ 7, pixel 2j+1 -> the bit below; bits 16.. are never stored
        count_src = acc;
    } else {
        typedef unsigned short h2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int j = 0; j < 8; ++j) {                           // pixels 2j, 2j+1; 6-byte pixels: luma = low half of dword 3j, high half of dword 3j+1
            const h2 t0 = __builtin_bit_cast(h2, a.d[3 * j]) - __builtin_bit_cast(h2, b.d[3 * j]);
            const h2 t1 = __builtin_bit_cast(h2, a.d[3 * j + 1]) - __builtin_bit_cast(h2, b.d[3 * j + 1]);
            const uint32_t d = (__builtin_bit_cast(uint32_t, t0) & 0x0000FFFFu) | (__builtin_bit_cast(uint32_t, t1) & 0xFFFF0000u);
            const uint32_t f = ((d & 0x7FFF7FFFu) + 0x7FFF7FFFu) & 0x80008000u;          // top bit of every half with (d & 0x7FFF) != 0
            const uint32_t two = ((f >> 14) & 2u) | (f >> 31);                          // pixel 2j -> bit 1, pixel 2j+1 -> bit 0
            bits |= two << (((2 * j + 1) ^ 7));
        }
        count_src = bits;
    }
    return bits;
}

// All-channel mode (rbf_residual_mask_batch_ex with mask_channels = the pixel's sample count; threshold 0 only): the bit is "some byte of
// the pixel changed", an exact comparison of every sample -- a 16-bit change of 0x8000, which the int16 rule above ignores, IS marked.  The
// pixel's bytes are XOR-ed as whole dwords and reduced to one flag without extracting a sample.  3-byte pixels: the three bytes of each
// of four pixels are gathered into three dwords (v_perm) whose OR goes through the carry trick above.  4- and 8-byte pixels: a pixel is
// one or two whole dwords, its flag one v_min_u32 against 1 (asm: the compiler turns a visible min(t, 1) into v_cmp + v_cndmask).
// 6-byte pixels: the three halves of each of two pixels are gathered into three dwords (one half per pixel each), OR-ed, and from there on
// it is the planar 16-bit path above (v_pk_min_u16, accumulator, interleave).
template <typename SAMPLE, int PIXEL_BYTES>
__device__ __forceinline__ uint32_t lane_bits_any(const LanePixels<SAMPLE, PIXEL_BYTES> &a, const LanePixels<SAMPLE, PIXEL_BYTES> &b, uint32_t one2, uint32_t &count_src)
{
    static_assert(PIXEL_BYTES == 3 || PIXEL_BYTES == 4 || PIXEL_BYTES == 6 || PIXEL_BYTES == 8, "all-channel masks: 3 or 4 samples of 1 or 2 bytes");
    uint32_t bits = 0;
    if (PIXEL_BYTES == 3) {
        constexpr int shift_of_group[4] = {4, 0, 12, 8};       // as lane_bits_thr0
#pragma unroll
        for (int g = 0; g < 4; ++g) {                           // pixels 4g..4g+3 = bytes 0-2 | 3-5 | 6-8 | 9-11 of three dwords
            const uint32_t x0 = a.d[3 * g] ^ b.d[3 * g], x1 = a.d[3 * g + 1] ^ b.d[3 * g + 1], x2 = a.d[3 * g + 2] ^ b.d[3 * g + 2];
            const uint32_t s0 = __builtin_amdgcn_perm(x2, __builtin_amdgcn_perm(x1, x0, 0x00060300u), 0x05020100u);   // bytes 0, 3, 6, 9
            const uint32_t s1 = __builtin_amdgcn_perm(x2, __builtin_amdgcn_perm(x1, x0, 0x00070401u), 0x06020100u);   // bytes 1, 4, 7, 10
            const uint32_t s2 = __builtin_amdgcn_perm(x2, __builtin_amdgcn_perm(x1, x0, 0x00000502u), 0x07040100u);   // bytes 2, 5, 8, 11
            const uint32_t z = s0 | s1 | s2;
            const uint32_t f = (((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
            bits |= (((f >> 7) * 0x08040201u) >> 24) << shift_of_group[g];
        }
        count_src = bits;
    } else if (PIXEL_BYTES == 4 || PIXEL_BYTES == 8) {
        constexpr int DPP = PIXEL_BYTES / 4;                    // dwords per pixel
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uint32_t t = a.d[DPP * k] ^ b.d[DPP * k];
            if (DPP == 2) t |= a.d[DPP * k + 1] ^ b.d[DPP * k + 1];
            uint32_t g;
            asm("v_min_u32 %0, 1, %1" : "=v"(g) : "v"(t));
            bits |= g << (k ^ 7);                               // MSB-first within each byte
        }
        count_src = bits;
    } else {
        uint32_t acc = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int j = s ^ 4;                                // pixels 2j, 2j+1 = halves 0-2 | 3-5 of dwords 3j..3j+2
            const uint32_t x0 = a.d[3 * j] ^ b.d[3 * j], x1 = a.d[3 * j + 1] ^ b.d[3 * j + 1], x2 = a.d[3 * j + 2] ^ b.d[3 * j + 2];
            const uint32_t h0 = __builtin_amdgcn_perm(x1, x0, 0x07060100u);       // {half 0, half 3}
            const uint32_t h1 = __builtin_amdgcn_perm(x2, x0, 0x05040302u);       // {half 1, half 4}
            const uint32_t h2 = __builtin_amdgcn_perm(x2, x1, 0x07060100u);       // {half 2, half 5}
            const uint32_t t = h0 | h1 | h2;
            uint32_t g;
            asm("v_pk_min_u16 %0, %1, %2" : "=v"(g) : "v"(t), "v"(one2));
            acc = (acc << 2) | g;
        }
        bits = (acc >> 16) | (acc << 1);
        count_src = acc;
    }
    return bits;
}

// What used to be k_finish_ones' job, folded into the mask kernel when it covers the whole frame (rbf_encode_gop on frames of whole
// 1024-pixel segments): every workgroup clears its share of up to two output regions (round 5: only the stats of the batch -- the
// witness rows are no longer cleared, k_chunk_offsets zeroes the few words compaction ORs into; region a is null), and
// the LAST workgroup to finish (a ticket) hands the counts out -- to the caller's array and into the device-visible pinned block
// whose token the host spins on -- and re-zeroes the accumulator and the ticket.  One launch less per step, and the publish no
// longer queues behind whatever else occupies the GPU (round 2's overlap profile, git history: the 5 us k_finish_ones took 61 us
// under overlap).
constexpr uint32_t MASK_TICKETS = 64;           // first-level ticket counters; one more dword for the second level
struct MaskFinish {
    uint32_t enabled;              // 0: the caller runs k_finish_ones
    uint32_t count;                // pairs
    uint32_t *ticket;              // context-owned: MASK_TICKETS + 1 counters, zero between launches
    uint64_t *ones_out;            // caller's device array
    uint64_t *host_block;          // nullable: [token | ones...] in pinned host memory
    uint64_t token;
    uint4 *clear_a; uint64_t quads_a;
    uint4 *clear_b; uint64_t quads_b;
};

// The temporal chunks of one launch (blockIdx.y) -- MaskChunks, MASK_MAX_CHUNKS, MASK_CHUNK_SKIP -- and the host planner that fills them
// live in rbf_mask_plan.h, which a plain host compiler takes.

template <typename SAMPLE, int PIXEL_BYTES, bool NT = false, bool THR0 = false>
__global__ __launch_bounds__(WG_THREADS) void k_residual_mask_gop(
    const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t nframes, uint64_t nsegs /* of 1024 px */,
    int32_t thr_all, const int32_t *__restrict__ thr_tab /* nullable: per pair */,
    uint16_t *__restrict__ masks, uint64_t mask_stride_u16, uint64_t *__restrict__ ones,
    const MaskChunks chunks, const MaskFinish fin)
{
    constexpr bool ANY = false;
#include "rbf_kernels_mask_body.h"
}

// All-channel twin of k_residual_mask_gop (rbf_residual_mask_batch_ex / rbf_encode_runs_begin_ex with mask_channels >= 2): the same
// chunks, skipped pairs, packed-count tally and fused finish; the bit is "any sample of the pixel changed" (lane_bits_any).  thr_tab:
// nullable, 0 = code the pair, > 0 = a skipped pair (a block with more runs than the chunk table holds).
template <typename SAMPLE, int PIXEL_BYTES, bool NT = false>
__global__ __launch_bounds__(WG_THREADS) void k_residual_mask_any_gop(
    const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t nframes, uint64_t nsegs /* of 1024 px */,
    const int32_t *__restrict__ thr_tab /* nullable: per pair */,
    uint16_t *__restrict__ masks, uint64_t mask_stride_u16, uint64_t *__restrict__ ones,
    const MaskChunks chunks, const MaskFinish fin)
{
    constexpr bool ANY = true, THR0 = false;
    constexpr int32_t thr_all = 0;
#include "rbf_kernels_mask_body.h"
}

// per-pair thresholds travel as kernel arguments (captured at launch) into a device table
struct ThrChunk {
    static constexpr uint32_t N = 256;
    int32_t v[N];
};
__global__ void k_store_thresholds(const ThrChunk c, int32_t *__restrict__ dst, uint32_t count)
{
    if (threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

// The tail of a residual-mask pass, ONE launch instead of a memset in front of the mask kernels, a copy kernel behind
// them and two more memsets (rocprofv3: the four small launches were ~25 us of a ~215 us step).  The mask kernels count
// into a context-owned accumulator that is zero whenever they start; block 0 hands the counts to the caller's array (and,
// for rbf_encode_gop, into the device-visible pinned block whose flag word the host spins on) and zeroes the accumulator
// again; every block clears its share of up to two output regions (the witness rows and the stats of the batch).
__global__ __launch_bounds__(256) void k_finish_ones(uint64_t *__restrict__ acc, uint64_t *__restrict__ ones, uint32_t count,
                                                     uint64_t *host_block /* nullable */, uint64_t token,
                                                     uint4 *__restrict__ clear_a, uint64_t quads_a, uint4 *__restrict__ clear_b, uint64_t quads_b)
{
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < count; i += blockDim.x) {
            const uint64_t v = acc[i];
            ones[i] = v;
            acc[i] = 0;
            if (host_block) __hip_atomic_store(&host_block[1 + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (host_block) {
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(&host_block[0], token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads_a; i += (uint64_t)gridDim.x * blockDim.x) clear_a[i] = z;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads_b; i += (uint64_t)gridDim.x * blockDim.x) clear_b[i] = z;
}

}  // namespace rbf
