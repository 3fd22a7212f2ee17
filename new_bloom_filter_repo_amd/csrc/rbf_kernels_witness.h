// rbf_kernels_witness.h -- between the query's pass words and the packed witness: k_chunk_offsets (where every workgroup's bits start),
// k_compact_witness (A5: witness = mask bits at the passing positions) and k_expand_mask (A6: the way back), with the software pext / pdep
// tables the two share.
#pragma once
#include "rbf_kernels.h"

namespace rbf {

// ------------------------------------------------------------------------------------------
// witness compaction (A5): witness = mask bits at the passing positions, in position order.
// One lane per 64-pixel word: its bits are pext(mask word, pass word) placed at
// seg_off[segment] + (passes of the segment's earlier words) in the pre-zeroed packed witness.
// ------------------------------------------------------------------------------------------
// Where the witness bits of every chunk of WG_THREADS words (= chunk_segs whole segments: the compaction's and the expansion's
// workgroups) start: off[f][c] = passes of all earlier segments of frame f.  One workgroup per frame scans the frame's segment counts once
// -- until round 5 every compaction workgroup summed all the counts in front of it by itself (a third of its instructions, and 1 MB of L2
// reads per 1080p frame).  total < 2^32 (n < 2^32).
constexpr int CO_THREADS = 1024;
__global__ __launch_bounds__(CO_THREADS) void k_chunk_offsets(const uint32_t *__restrict__ seg_cnt, uint64_t nseg, uint32_t chunk_segs, uint32_t nchunks,
                                                              uint32_t *__restrict__ off, uint32_t *__restrict__ witnesses /* nullable (decode) */, uint64_t witness_stride_words32)
{
    // Encode: this kernel also ZEROES the few witness dwords the compaction's workgroups share -- the 64-bit word around every chunk's
    // first bit and around the witness's end (whose pad bits must read 0) -- so that nobody has to clear whole witness rows (until round 5
    // the mask kernel cleared 259 KB per 1080p frame for them: a tenth of its HBM traffic).  Everything else the compaction overwrites.
    // a thread sums `per` consecutive counts (4 when a chunk has that many segments), the workgroup scans the sums, and the thread that
    // holds a chunk's first segments writes the chunk's offset; frames of more than 1024 * per segments take several rounds with a carry
    __shared__ uint32_t wtot[CO_THREADS / WAVE];
    __shared__ uint32_t carry_s;
    const uint32_t f = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t *cnt = seg_cnt + (uint64_t)f * nseg;
    uint32_t *out = off + (uint64_t)f * nchunks;
    uint32_t *wit = witnesses ? witnesses + (uint64_t)f * witness_stride_words32 : nullptr;
    auto zero_word_at = [&](uint32_t bit) {
        const uint64_t d = (bit >> 5) & ~1u;
        if (d < witness_stride_words32) wit[d] = 0;
        if (d + 1 < witness_stride_words32) wit[d + 1] = 0;
    };
    const uint32_t per = (chunk_segs & 3u) == 0 ? 4u : (chunk_segs & 1u) == 0 ? 2u : 1u;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < nseg; base += (uint64_t)CO_THREADS * per) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * per;
        uint32_t sum = 0;
        for (uint32_t k = 0; k < per; ++k) sum += i0 + k < nseg ? cnt[i0 + k] : 0u;
        const uint32_t incl = wave_inclusive_scan(sum);
        if (lane == WAVE - 1) wtot[wave] = incl;
        const uint32_t carry = carry_s;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t k = 0; k < wave; ++k) before += wtot[k];
        if (i0 < nseg && i0 % chunk_segs == 0) {
            out[i0 / chunk_segs] = before + incl - sum;
            if (wit) zero_word_at(before + incl - sum);
        }
        __syncthreads();
        if (threadIdx.x == CO_THREADS - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (wit && threadIdx.x == 0) zero_word_at(carry_s);          // the end of the witness
}

// Software pext / pdep through a 256-byte LDS table of their 4-bit forms, entry [p4 << 4 | x4] (thread t of a 256-thread workgroup
// writes entry t): pext4 = the bits of x4 at the set positions of p4, packed low; pdep4 = the low popc(p4) bits of x4 dealt out to the
// set positions of p4.  A 64-bit word is sixteen independent look-ups -- a lane reads one byte, lanes reading the same dword are served
// by one broadcast and the table covers each of the 64 banks once, so there are no bank conflicts -- against a loop that ran as long as
// the busiest lane of the wave (~9 rounds of 19 instructions for the compaction, ~22 of 14 for the expansion).
static_assert(WG_THREADS == 256, "one table entry per thread");
__host__ __device__ constexpr uint32_t pext4_entry(uint32_t t)
{
    const uint32_t p4 = t >> 4, x4 = t & 15u;
    uint32_t r = 0, k = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if ((p4 >> b) & 1u) { r |= ((x4 >> b) & 1u) << k; ++k; }
    return r;
}
__host__ __device__ constexpr uint32_t pdep4_entry(uint32_t t)
{
    const uint32_t p4 = t >> 4, x4 = t & 15u;
    uint32_t r = 0, k = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if ((p4 >> b) & 1u) { r |= ((x4 >> k) & 1u) << b; ++k; }
    return r;
}
// The two tables, built at compile time (until round 5 every workgroup computed its own: ~25 instructions per thread), 64 dwords each in
// constant memory; wave 0 of a workgroup copies one into LDS.
struct Lut256 { uint32_t w[64]; };
template <bool PDEP>
constexpr Lut256 make_lut4()
{
    Lut256 t{};
    for (uint32_t i = 0; i < 256; ++i) t.w[i >> 2] |= (PDEP ? pdep4_entry(i) : pext4_entry(i)) << (8u * (i & 3u));
    return t;
}
static __constant__ Lut256 LUT_PEXT4 = make_lut4<false>();
static __constant__ Lut256 LUT_PDEP4 = make_lut4<true>();
__device__ __forceinline__ void lut_to_lds(uint8_t *lut, const Lut256 &src)
{
    if (threadIdx.x < 64u) reinterpret_cast<uint32_t *>(lut)[threadIdx.x] = src.w[threadIdx.x];
}

// pext(x, p) of a 32-bit half: <= popc(p) <= 32 bits, LSB = the first set position of p
__device__ __forceinline__ uint32_t pext32_lut(const uint8_t *lut, uint32_t x, uint32_t p)
{
    uint32_t out = 0, off = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t p4 = __builtin_amdgcn_ubfe(p, 4u * j, 4u), x4 = __builtin_amdgcn_ubfe(x, 4u * j, 4u);
        out |= (uint32_t)lut[(p4 << 4) | x4] << (off & 31u);       // (off + popc(p4) <= 32, the entry has popc(p4) bits; off = 32 only with nothing left)
        off += __popc(p4);
    }
    return out;
}
// pdep(w, p) of a 32-bit half: the low popc(p) bits of w (stream order, LSB first) dealt out to the set positions of p
__device__ __forceinline__ uint32_t pdep32_lut(const uint8_t *lut, uint32_t w, uint32_t p)
{
    uint32_t out = 0, off = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t p4 = __builtin_amdgcn_ubfe(p, 4u * j, 4u), w4 = __builtin_amdgcn_ubfe(w, off, 4u);     // (off = 32 only when nothing is left to deal out)
        out |= (uint32_t)lut[(p4 << 4) | w4] << (4u * j);
        off += __popc(p4);
    }
    return out;
}

template <bool STREAM>
__global__ __launch_bounds__(WG_THREADS) void k_compact_witness(
    const uint64_t *__restrict__ pass_words, const uint32_t *__restrict__ seg_cnt, uint64_t nseg, uint32_t words_per_seg,
    const uint64_t *__restrict__ masks, uint64_t mask_stride_words64, uint64_t n,
    uint32_t *__restrict__ witnesses, uint64_t witness_stride_words32, uint64_t *__restrict__ stats,
    const uint32_t *__restrict__ chunk_off /* k_chunk_offsets: [frame][workgroup] */)
{
    // A workgroup owns WG_THREADS consecutive words (= whole segments).  Their witness bits form one contiguous bit range starting at
    // (passes of all earlier segments, from k_chunk_offsets): the range is assembled in LDS with LDS atomics and written with plain
    // coalesced stores; only its first and last dword may be shared with the neighbouring workgroups (atomicOr onto zeroed dwords).  The offsets inside the
    // chunk are a block scan.
    //
    // The step is bound by instruction issue, so this kernel is written for a short instruction stream (round 3: ~415
    // VALU wave-instructions per 64 words, now ~230): the earlier counts are read four to a load, all loads of a thread are in flight
    // before the first wait, both block-wide sums cross ONE barrier, the wave scans are DPP adds, and the pext is sixteen look-ups.
    __shared__ uint32_t buf[WG_THREADS * 2 + 2];
    __shared__ uint32_t wsum[WG_WAVES];
    __shared__ __attribute__((aligned(4))) uint8_t lut[256];
    const uint32_t f = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (uint32_t)((n + 63) >> 6);                        // n < 2^32 (rbf_plan_batch)
    const uint32_t total = (uint32_t)nseg * words_per_seg;
    const uint64_t *pwf = pass_words + (uint64_t)f * total;
    const uint32_t start32 = chunk_off[(uint64_t)f * gridDim.x + blockIdx.x];      // (uniform: a scalar load)
    uint32_t *wit = witnesses + (uint64_t)f * witness_stride_words32;
    const uint32_t wbeg = blockIdx.x * WG_THREADS;
    const uint32_t w = wbeg + threadIdx.x;
    // my word (packed -> bit b = position 64w + b) and its mask word: requested before anything waits
    const bool have = w < total && w < nwords;
    const uint64_t *mkp = masks + (uint64_t)f * mask_stride_words64 + w;
    const uint64_t pw_raw = have ? (STREAM ? __builtin_nontemporal_load(pwf + w) : pwf[w]) : 0ull;        // read once: see the cache-policy note in rbf_lds_dma.h
    const uint64_t mk_raw = have ? (STREAM ? __builtin_nontemporal_load(mkp) : *mkp) : 0ull;
    lut_to_lds(lut, LUT_PEXT4);
    buf[threadIdx.x] = 0;
    buf[threadIdx.x + WG_THREADS] = 0;
    if (threadIdx.x < 2) buf[threadIdx.x + 2 * WG_THREADS] = 0;
    const uint64_t pw = flip_bytes64(pw_raw);
    const uint32_t pw_lo = (uint32_t)pw, pw_hi = (uint32_t)(pw >> 32);
    const uint32_t c_lo = __popc(pw_lo), c = c_lo + __popc(pw_hi);
    const uint32_t incl = wave_inclusive_scan(c);
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, chunk_total = 0;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k) {
        if ((uint32_t)k < wave) before += wsum[k];
        chunk_total += wsum[k];
    }
    const uint32_t obase = start32 & ~31u;                                    // dword-aligned start of my LDS image
    const uint32_t o = start32 + before + incl - c;
    // pext(mask, pw), LSB = first passing position, as two 32-bit halves; the high half's result is shifted up by the low half's pass count
    const uint64_t mk = flip_bytes64(mk_raw);
    const uint32_t o_lo = pext32_lut(lut, (uint32_t)mk, pw_lo), o_hi = pext32_lut(lut, (uint32_t)(mk >> 32), pw_hi);
    const uint64_t out = (uint64_t)o_lo | ((uint64_t)o_hi << c_lo);
    if (out) {
        const uint32_t rel = o - obase;
        const uint32_t sh = rel & 31u, word = rel >> 5;
        const uint32_t lo = (uint32_t)out, hi = (uint32_t)(out >> 32);
        const uint32_t d0 = lo << sh;
        const uint32_t d1 = sh ? ((lo >> (32u - sh)) | (hi << sh)) : hi;
        const uint32_t d2 = sh ? (hi >> (32u - sh)) : 0u;
        if (d0) atomicOr(&buf[word], d0);
        if (d1) atomicOr(&buf[word + 1], d1);
        if (d2) atomicOr(&buf[word + 2], d2);
    }
    __syncthreads();
    const uint32_t oend = start32 + chunk_total;
    const uint32_t ndw = ((oend - obase) + 31u) >> 5;
    // a dword this workgroup shares with a neighbour (its first one when it does not start on a dword, its last one when it does not end on
    // one) was zeroed by k_chunk_offsets and is OR-ed into; every other dword of the range is written whole, zero or not
    for (uint32_t i = threadIdx.x; i < ndw; i += WG_THREADS) {
        const uint32_t v = buf[i];
        const bool shared = (i == 0 && (start32 & 31u)) || (i + 1 == ndw && (oend & 31u));
        if (shared) { if (v) atomicOr(&wit[(obase >> 5) + i], flip_bytes32(v)); }
        else wit[(obase >> 5) + i] = flip_bytes32(v);
    }
    if (threadIdx.x == 0 && wbeg + WG_THREADS >= total) stats[(uint64_t)f * 4 + 0] = oend;   // len(witness)
}

// A6 expand: out[i] = witness[rank(i)] where position i passes, else 0 (:299-304).  One lane per 64-position word, a workgroup per
// WG_THREADS consecutive words (= whole segments), offsets as in k_compact_witness: the start comes from k_chunk_offsets, the offsets
// inside the chunk are a block scan.  The lane's popc(pass) stream bits are fetched
// as one 64-bit window and dealt out to the set bits of the pass word through the pdep table.  Reads never leave the row.
__global__ __launch_bounds__(WG_THREADS) void k_expand_mask(
    const uint64_t *__restrict__ pass_words, const uint32_t *__restrict__ seg_cnt, uint64_t nseg, uint32_t words_per_seg,
    const uint32_t *__restrict__ witnesses, uint64_t witness_stride_words32,
    uint64_t *__restrict__ masks, uint64_t mask_stride_words64, uint64_t n, const uint32_t *__restrict__ chunk_off /* k_chunk_offsets */)
{
    __shared__ uint32_t wsum[WG_WAVES];
    __shared__ __attribute__((aligned(4))) uint8_t lut[256];
    const uint32_t f = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (uint32_t)((n + 63) >> 6);
    const uint32_t total = (uint32_t)nseg * words_per_seg;
    const uint32_t start32 = chunk_off[(uint64_t)f * gridDim.x + blockIdx.x];
    const uint32_t *wit = witnesses + (uint64_t)f * witness_stride_words32;
    const uint32_t wbeg = blockIdx.x * WG_THREADS;
    const uint32_t w = wbeg + threadIdx.x;
    const bool have = w < total && w < nwords;
    const uint64_t pw_raw = have ? pass_words[(uint64_t)f * total + w] : 0ull;
    lut_to_lds(lut, LUT_PDEP4);
    const uint64_t p = flip_bytes64(pw_raw);                      // packed -> bit b = position 64w + b
    const uint32_t p_lo = (uint32_t)p, p_hi = (uint32_t)(p >> 32);
    const uint32_t c_lo = __popc(p_lo), c = c_lo + __popc(p_hi);
    const uint32_t incl = wave_inclusive_scan(c);
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t o = start32 + incl - c;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k)
        if ((uint32_t)k < wave) o += wsum[k];
    if (w >= nwords) return;
    uint64_t out = 0;
    if (c) {
        // stream bits o ... o + c - 1 as a window with bit t = stream bit o + t (flip_bytes32: packed dword -> stream bit b at bit b)
        const uint32_t d0 = o >> 5, dl = (o + c - 1u) >> 5, r = o & 31u;
        const uint64_t x0 = d0 < witness_stride_words32 ? flip_bytes32(wit[d0]) : 0u;
        const uint64_t x1 = (d0 + 1 <= dl && d0 + 1 < witness_stride_words32) ? flip_bytes32(wit[d0 + 1]) : 0u;
        const uint64_t x2 = (d0 + 2 <= dl && d0 + 2 < witness_stride_words32) ? flip_bytes32(wit[d0 + 2]) : 0u;
        uint64_t win = (x0 | (x1 << 32)) >> r;
        win |= r ? x2 << (64u - r) : 0ull;
        out = (uint64_t)pdep32_lut(lut, (uint32_t)win, p_lo) | ((uint64_t)pdep32_lut(lut, (uint32_t)(win >> c_lo), p_hi) << 32);
    }
    masks[(uint64_t)f * mask_stride_words64 + w] = flip_bytes64(out);
}

}  // namespace rbf
