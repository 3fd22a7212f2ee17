// rbf_kernels_barrett.h -- the LDS-resident insert and query kernels with Barrett reductions: every filter size the FP64 kernels
// do not take (m outside 2^15 ... 2^23, or a test knob), whole in LDS or tile by tile.
//
// Measured on MI355X (round 1's microbenchmark: git history): random dword probes run at ~430 G/s from a 76 KB
// global region and ~260 G/s from an L2-resident 2 MB one, random global atomicOr at ~25 G/s --
// while LDS probes / LDS atomics run at >1600 G/s.  So both the filter build (insert) and the
// filter test (query) keep the whole filter of one frame in LDS:
//
//   k_insert_lds   grid (S, F): workgroup (s, f) builds a PARTIAL filter of frame f in LDS from slice
//                  s of the mask (set positions are compacted through a per-wave LDS queue so the
//                  hashing always runs with full waves) and stores it; k_filter_reduce ORs the S
//                  partials -- no global atomics anywhere.
//   k_query_lds    "frames-inner": a wave owns a segment of P*64 consecutive pixels for the whole
//                  batch.  The three XXH64 of each pixel index depend only on the index, so they are
//                  computed ONCE and kept in registers; then for every frame of the batch the
//                  workgroup stages that frame's filter into LDS and each lane does the per-frame
//                  part only: two Barrett reductions mod m_f, the LDS probes, ballot + compaction.
//   k_query_tiled  the same for filters larger than LDS, staged tile by tile.
#pragma once
#include "rbf_kernels.h"
#include "rbf_lds_dma.h"

namespace rbf {

// h mod m for 2 <= m <= 2^30 (m2 = 2m), three 32x32 multiplies for the quotient estimate:
// q' = hh*Mh + hi32(hh*Ml) + hi32(hl*Mh) >= floor(h*M/2^64) - 2 >= floor(h/m) - 3, so
// r' = h - q'*m < 4m <= 2^32 and everything is carried modulo 2^32; two conditional subtracts
// (2m, then m) finish the reduction.
__device__ __forceinline__ uint32_t mod_m_small(uint64_t h, uint32_t m, uint32_t m2, uint32_t Mh, uint32_t Ml)
{
    const uint32_t hh = (uint32_t)(h >> 32), hl = (uint32_t)h;
    const uint32_t q = hh * Mh + __umulhi(hh, Ml) + __umulhi(hl, Mh);
    uint32_t r = hl - q * m;
    r = min(r, r - m2);
    r = min(r, r - m);
    return r;
}

// ------------------------------------------------------------------------------------------
// insert
// ------------------------------------------------------------------------------------------
template <bool SMALL_M>
__global__ __launch_bounds__(IL_THREADS) void k_insert_lds(
    const uint8_t *__restrict__ masks, uint64_t mask_stride_bytes, uint64_t n,
    const FrameTable tab, Seeds seeds,
    uint32_t *__restrict__ partials, uint64_t part_stride_words32, uint32_t tile_words /* even */,
    const SliceTable slices, uint32_t per_tile /* sum of slices.n */, uint32_t Smax /* max of slices.n: row pitch of the partials */)
{
    // 1-D grid of tiles * per_tile workgroups: frame f is cut into slices.n[f] mask slices (0 for a frame that is
    // not Bloom-coded), chosen on the host so that the workgroups fill the 256 CUs whatever the frame count is
    // (29 frames: 24 x 9 + 5 x 8).  The grid is one-dimensional on purpose: consecutive workgroup ids go to
    // consecutive XCDs, and a 2-D grid whose x extent is not a multiple of 8 left some XCDs with more workgroups
    // than CUs (measured: grid (9, 29) -> 114 us instead of 70 us for the same 242 workgroups).
    // The tile index is the slowest coordinate: this workgroup keeps words [tile0, tile0 + tile_words) of the
    // partial filter in LDS and sets only the positions that fall into them.  Filters that fit LDS whole
    // (1080p: 76 KB) have one tile; a 4K filter (306 KB) is built in 3 tiles (keys re-hashed per tile).
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *filt = lds;                                         // [tile_words]
    uint32_t *queues = lds + tile_words;                          // [IL_WAVES][IL_QUEUE]
    const uint32_t tile = blockIdx.x / per_tile;
    uint32_t s = blockIdx.x - tile * per_tile, f = 0;
    while (s >= slices.n[f]) { s -= slices.n[f]; ++f; }          // workgroup-uniform walk over <= 128 bytes
    const uint32_t S = slices.n[f];
    const FrameDev fd = tab.f[f];
    if (fd.m == 0) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t fwords = filter_words(fd.m);
    const uint32_t tile0 = tile * tile_words;                     // first word of my tile
    if (tile0 >= fwords) return;
    const uint32_t tile_bit0 = tile0 << 5, tile_bits = tile_words << 5;
    for (uint32_t i = threadIdx.x; i < tile_words; i += IL_THREADS) filt[i] = 0;
    __syncthreads();

    const uint8_t *mask = masks + (uint64_t)f * mask_stride_bytes;
    const uint64_t nbytes = (n + 7) >> 3;
    const uint64_t groups = (nbytes + 63) >> 6;                    // 64-byte wave steps
    const uint64_t gper = (groups + S - 1) / S;
    const uint64_t g0 = (uint64_t)s * gper;
    const uint64_t g1 = g0 + gper < groups ? g0 + gper : groups;
    uint32_t *q = queues + wave * IL_QUEUE;
    uint32_t qn = 0;                                               // wave-uniform queue length

    const uint32_t m = fd.m, m2 = fd.m << 1, Mh = (uint32_t)(fd.M >> 32), Ml = (uint32_t)fd.M;
    auto drain_at = [&](uint32_t first, uint32_t count) {          // hash `count` (<= 64) queued positions
        const bool act = lane < count;                             // (wave-uniform call: hash3_index votes)
        const uint32_t idx = act ? q[first + lane] : 0u;
        const Hash3 h = hash3_index(idx, act, seeds);
        if (act) {
            uint32_t pos, step;
            if (SMALL_M) { pos = mod_m_small(h.h1, m, m2, Mh, Ml); step = mod_m_small(h.h2, m, m2, Mh, Ml); }
            else         { pos = mod_m(h.h1, m, fd.M);             step = mod_m(h.h2, m, fd.M); }
            for (uint32_t j = 0; j < fd.floor_k; ++j) {
                const uint32_t rel = pos - tile_bit0;              // unsigned: out-of-tile positions wrap high
                if (rel < tile_bits) atomicOr(&filt[rel >> 5], msb_bit(pos));
                const uint64_t s2 = (uint64_t)pos + step;
                pos = (uint32_t)(s2 >= m ? s2 - m : s2);
            }
            const uint32_t rel = pos - tile_bit0;
            if (h.ha < fd.T && rel < tile_bits) atomicOr(&filt[rel >> 5], msb_bit(pos));
        }
    };

    auto load_bits = [&](uint64_t g) -> uint32_t {                 // my byte of wave step g in natural bit order
        const uint64_t byte = g * 64 + lane;
        if (g >= g1 || byte >= nbytes) return 0u;
        uint32_t b = __builtin_bitreverse32((uint32_t)mask[byte]) >> 24;
        const uint64_t rem = n - byte * 8;
        if (rem < 8) b &= (1u << rem) - 1u;                        // ignore pad bits
        return b;
    };
    uint32_t nxt = load_bits(g0 + wave);
    for (uint64_t g = g0 + wave; g < g1; g += IL_WAVES) {
        uint32_t bits = nxt;
        nxt = load_bits(g + IL_WAVES);                             // prefetch: the load flies while we hash
        // exclusive prefix of the per-lane counts (0..8) without a cross-lane scan: one ballot per bit
        // of the count, rank of the ballot below my lane (mbcnt), weighted sum -- no LDS round trips
        const uint32_t c = __popc(bits);
        const uint64_t b0 = __ballot((c & 1u) != 0), b1 = __ballot((c & 2u) != 0);
        const uint64_t b2 = __ballot((c & 4u) != 0), b3 = __ballot((c & 8u) != 0);
        const uint32_t excl = rank_below(b0) + 2u * rank_below(b1) + 4u * rank_below(b2) + 8u * rank_below(b3);
        const uint32_t total = __popcll(b0) + 2u * __popcll(b1) + 4u * __popcll(b2) + 8u * __popcll(b3);
        uint32_t off = qn + excl;
        const uint32_t base = (uint32_t)((g * 64 + lane) << 3);
        while (bits) {
            q[off++] = base + __builtin_ctz(bits);
            bits &= bits - 1u;
        }
        qn += total;
        wave_lds_fence();
        while (qn >= WAVE) {                                       // full waves only; order is irrelevant (OR)
            qn -= WAVE;
            drain_at(qn, WAVE);
        }
        wave_lds_fence();                                          // queue reads done before it is refilled
    }
    drain_at(0, qn);
    __syncthreads();
    uint32_t *part = partials + ((uint64_t)f * Smax + s) * part_stride_words32 + tile0;
    const uint32_t mine = fwords - tile0 < tile_words ? fwords - tile0 : tile_words;
    const uint32_t pairs = (mine + 1) >> 1;                       // tile0 is even: 8-byte aligned
    for (uint32_t i = threadIdx.x; i < pairs; i += IL_THREADS)
        reinterpret_cast<uint2 *>(part)[i] = reinterpret_cast<const uint2 *>(filt)[i];
}

// ------------------------------------------------------------------------------------------
// query, frames-inner
// ------------------------------------------------------------------------------------------
// LDS dword holding filter bit `pos`: (pos >> 5) * 4 + base in two instructions (v_bfe_u32 +
// v_lshl_add_u32); written plainly the compiler folds it to shift / and / add.
__device__ __forceinline__ uint32_t probe_word(const uint32_t *filt, uint32_t pos)
{
    const uint32_t w = __builtin_amdgcn_ubfe(pos, 5, 27);
    return filt[w];
}

// One frame's pass over a lane's QL_P consecutive pixels: reductions mod m, LDS probes, verdict.
// FK >= 0: floor(k*) known at compile time (fully unrolled probes); FK < 0: runtime fk.
// The verdict of pixel j is the sign bit of `acc`; it is shifted into `pb` (one v_alignbit), so after
// the loop pb holds the lane's QL_P verdicts MSB-first -- exactly one byte of the packed pass vector.
// Returns the wave's number of passing positions.  Branch-free for FK >= 0 so the QL_P dependency
// chains interleave.
template <bool SMALL_M, int FK>
__device__ __forceinline__ uint32_t frame_pass(
    const uint64_t (&h1)[QL_P], const uint64_t (&h2)[QL_P], const uint64_t (&ha)[QL_P], uint32_t validmask,
    const uint32_t *filt, uint32_t m, uint64_t M, uint64_t T, uint32_t fk_rt, uint32_t &pb)
{
    const uint32_t Mh = (uint32_t)(M >> 32), Ml = (uint32_t)M;
    const uint32_t fk = FK >= 0 ? (uint32_t)FK : fk_rt;
    const uint32_t m2 = m << 1;
    uint32_t npass = 0;
    pb = 0;
#pragma unroll
    for (int it = 0; it < QL_P; ++it) {
        uint32_t pos, step;
        if (SMALL_M) { pos = mod_m_small(h1[it], m, m2, Mh, Ml); step = mod_m_small(h2[it], m, m2, Mh, Ml); }
        else         { pos = mod_m(h1[it], m, M);            step = mod_m(h2[it], m, M); }
        // Each probe shifts its word LEFT so that the probed bit lands in bit 31: the verdict is the
        // sign bit of the AND of all probes.  MSB-first bit (pos & 31) ^ 7 -> shift (pos ^ 24) & 31.
        uint32_t acc = validmask << (31 - it);                // only the sign bit is ever looked at: bit `it` -> bit 31
#pragma unroll
        for (uint32_t j = 0; j < fk; ++j) {
            acc &= probe_word(filt, pos) << ((pos ^ 24u) & 31u);
            if (SMALL_M) { const uint32_t s2 = pos + step; pos = min(s2, s2 - m); }
            else { const uint64_t s2 = (uint64_t)pos + step; pos = (uint32_t)(s2 >= m ? s2 - m : s2); }
        }
        const uint32_t x = probe_word(filt, pos) << ((pos ^ 24u) & 31u);
        acc &= (ha[it] < T) ? x : 0x80000000u;
        pb = __builtin_amdgcn_alignbit(pb, acc, 31);          // (pb << 1) | (acc >> 31)
        npass += __popcll(__ballot((int32_t)acc < 0));
    }
    return npass;
}

// Query, frames-inner (A5 for encode, A6 for decode: both need the pass word of every 64 pixels).
//   pass_words, as bytes: [(f*nseg + seg)*QL_SEG_PIXELS/8 + b]  bit 7-r = position seg*QL_SEG_PIXELS + 8b + r passes
//                                          filter f, i.e. the packed (numpy.packbits) order of masks and witnesses
// A lane owns QL_P = 8 CONSECUTIVE pixels (its verdicts are one byte of that vector, and their keys share all
// but the last character, see hash3_run8); a wave owns 512 consecutive pixels.
//   seg_cnt[f*nseg + seg]                  passing positions of the segment (= witness bits it owns)
// SMALL_M: every filter of the batch has 2 <= m <= 2^30 (host-checked) -> cheap reductions.
template <bool DOUBLE_BUFFER, bool SMALL_M>
__global__ __launch_bounds__(QL_THREADS) void k_query_lds(
    uint64_t n, uint32_t nframes, const FrameTable tab, Seeds seeds,
    const uint32_t *__restrict__ filters, uint64_t filter_stride_words32, uint32_t fwords_max,
    uint32_t *__restrict__ seg_cnt, uint64_t nseg, uint64_t *__restrict__ pass_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t bufwords = (fwords_max + 3u) & ~3u;            // 16-byte multiple
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nwaves = blockDim.x >> 6;
    const uint64_t seg = (uint64_t)blockIdx.x * nwaves + wave;
    const bool live = seg < nseg;
    const uint64_t base = seg * QL_SEG_PIXELS;

    // ---- frame-independent part: the three hashes of my P consecutive pixel indices ------
    // (the 8-pixel hash block below has twins in query_u64_body, rbf_kernels_query_f64.h, which also stores the hash table, and in
    // k_query_s64t, rbf_kernels_query_f64_tiled.h, which pins hd1 / hd2 with an empty asm.  Kept apart: sharing them changes the ISA.)
    static_assert(QL_P == 8, "a lane's verdicts fill one byte; hash3_run8 hashes runs of 8");
    uint64_t h1[QL_P], h2[QL_P], ha[QL_P];
    uint32_t validmask = 0;
    const uint64_t i0 = base + (uint64_t)lane * QL_P;
#pragma unroll
    for (int it = 0; it < QL_P; ++it) {
        h1[it] = 0; h2[it] = 0; ha[it] = ~0ull;
        if (live && i0 + it < n) validmask |= 1u << it;
    }
    if (!hash3_run8((uint32_t)i0, validmask, seeds, h1, h2, ha)) {
#pragma unroll
        for (int it = 0; it < QL_P; ++it) {                      // mixed key lengths in this wave: index by index
            const bool act = (validmask >> it) & 1u;
            const Hash3 h = hash3_index((uint32_t)(i0 + it), act, seeds);
            h1[it] = h.h1; h2[it] = h.h2; ha[it] = h.ha;
        }
    }
    uint8_t *pass_bytes = reinterpret_cast<uint8_t *>(pass_words);

    // passthrough frames (m == 0): nothing passes (twins, driven by the `empty` bits: query_u64_body and k_query_s64t)
    for (uint32_t g = 0; g < nframes; ++g) {
        if (tab.f[g].m == 0) {
            if (live && lane == 0) seg_cnt[(uint64_t)g * nseg + seg] = 0;
            if (live) pass_bytes[((uint64_t)g * nseg + seg) * (QL_SEG_PIXELS / 8) + lane] = 0;
        }
    }
    // Every workgroup walks the frames in the same order: all CUs then pull the same 76 KB filter at
    // about the same time, which the L2 serves best (measured in round 1: rotating the start frame per workgroup, so that
    // ~29 different filters are in flight, costs +11 us per launch).
    auto frame_at = [&](uint32_t k) -> uint32_t { return k; };
    auto next_active = [&](uint32_t k) -> uint32_t { while (k < nframes && tab.f[frame_at(k)].m == 0) ++k; return k; };
    uint32_t k = next_active(0);
    uint32_t cur = 0;
    if (DOUBLE_BUFFER && k < nframes) {
        const uint32_t f0 = frame_at(k);
        dma_filter(lds, filters + (uint64_t)f0 * filter_stride_words32, filter_words(tab.f[f0].m), wave, lane, nwaves);
    }
    while (k < nframes) {
        k = __builtin_amdgcn_readfirstlane(k);                    // frame indices are wave-uniform: scalar table loads
        const uint32_t kn = __builtin_amdgcn_readfirstlane(next_active(k + 1));
        const uint32_t f = __builtin_amdgcn_readfirstlane(frame_at(k));
        const uint32_t fn = __builtin_amdgcn_readfirstlane(kn < nframes ? frame_at(kn) : 0u);
        const FrameDev fd = tab.f[f];
        const uint32_t *filt;
        if (DOUBLE_BUFFER) {
            dma_wait_all();           // my share of DMA(f) has landed ...
            __syncthreads();          // ... and everyone's; buffer cur^1 is free again
            filt = lds + cur * bufwords;
            if (kn < nframes)
                dma_filter(lds + (cur ^ 1u) * bufwords, filters + (uint64_t)fn * filter_stride_words32, filter_words(tab.f[fn].m), wave, lane, nwaves);
            cur ^= 1u;
        } else {
            __syncthreads();          // previous frame's probes are done
            dma_filter(lds, filters + (uint64_t)f * filter_stride_words32, filter_words(fd.m), wave, lane, nwaves);
            dma_wait_all();
            __syncthreads();
            filt = lds;
        }
        // frame geometry is wave-uniform: keep it in SGPRs so every branch below is scalar
        // (the builtin returns int: go through uint32_t or the low half sign-extends)
        const uint32_t m = __builtin_amdgcn_readfirstlane(fd.m);
        const uint32_t fk = __builtin_amdgcn_readfirstlane(fd.floor_k);
        const uint32_t Mh = __builtin_amdgcn_readfirstlane((uint32_t)(fd.M >> 32));
        const uint32_t Ml = __builtin_amdgcn_readfirstlane((uint32_t)fd.M);
        const uint32_t Thi = __builtin_amdgcn_readfirstlane((uint32_t)(fd.T >> 32));
        const uint32_t Tlo = __builtin_amdgcn_readfirstlane((uint32_t)fd.T);
        const uint64_t T = ((uint64_t)Thi << 32) | Tlo;
        const uint64_t M = ((uint64_t)Mh << 32) | Ml;

        uint32_t pb = 0, npass;
        // floor(k*) is a small integer: straight-line code for the common values lets the compiler
        // issue every LDS probe of all QL_P pixels back to back instead of one round trip at a time.
        switch (fk) {
        case 1: npass = frame_pass<SMALL_M, 1>(h1, h2, ha, validmask, filt, m, M, T, fk, pb); break;
        case 2: npass = frame_pass<SMALL_M, 2>(h1, h2, ha, validmask, filt, m, M, T, fk, pb); break;
        case 3: npass = frame_pass<SMALL_M, 3>(h1, h2, ha, validmask, filt, m, M, T, fk, pb); break;
        case 4: npass = frame_pass<SMALL_M, 4>(h1, h2, ha, validmask, filt, m, M, T, fk, pb); break;
        default: npass = frame_pass<SMALL_M, -1>(h1, h2, ha, validmask, filt, m, M, T, fk, pb); break;
        }
        if (live) {
            pass_bytes[((uint64_t)f * nseg + seg) * (QL_SEG_PIXELS / 8) + lane] = (uint8_t)pb;
            if (lane == 0) seg_cnt[(uint64_t)f * nseg + seg] = npass;
        }
        k = kn;
    }
}

// ------------------------------------------------------------------------------------------
// query for filters larger than LDS (4K frames: 306 KB): the filter is staged tile by tile; every
// (pixel, frame) computes its probe positions once and tests, per tile, the probes that land in it.
// Same outputs as k_query_lds with TQ_P pass words per segment.
// ------------------------------------------------------------------------------------------
template <bool SMALL_M>
__global__ __launch_bounds__(QL_THREADS) void k_query_tiled(
    uint64_t n, uint32_t nframes, const FrameTable tab, Seeds seeds,
    const uint32_t *__restrict__ filters, uint64_t filter_stride_words32, uint32_t tile_words /* multiple of 4 */,
    uint32_t *__restrict__ seg_cnt, uint64_t nseg, uint64_t *__restrict__ pass_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nwaves = blockDim.x >> 6;
    const uint64_t seg = (uint64_t)blockIdx.x * nwaves + wave;
    const bool live = seg < nseg;
    const uint64_t base = seg * TQ_SEG_PIXELS;
    uint64_t h1[TQ_P], h2[TQ_P], ha[TQ_P];
    uint32_t validmask = 0;
#pragma unroll
    for (int it = 0; it < TQ_P; ++it) {
        const uint64_t i = base + (uint64_t)it * WAVE + lane;
        const bool act = live && i < n;
        const Hash3 h = hash3_index((uint32_t)i, act, seeds);
        h1[it] = act ? h.h1 : 0; h2[it] = act ? h.h2 : 0; ha[it] = act ? h.ha : ~0ull;
        validmask |= act ? 1u << it : 0u;
    }
    for (uint32_t f = 0; f < nframes; ++f) {
        const FrameDev fd = tab.f[f];
        if (fd.m == 0) {                                          // passthrough frame (block-uniform)
            if (live && lane == 0) seg_cnt[(uint64_t)f * nseg + seg] = 0;
            if (live && lane < TQ_P) pass_words[((uint64_t)f * nseg + seg) * TQ_P + lane] = 0;
            continue;
        }
        const uint32_t m = __builtin_amdgcn_readfirstlane(fd.m);
        const uint32_t fk = __builtin_amdgcn_readfirstlane(fd.floor_k);
        const uint32_t Mh = __builtin_amdgcn_readfirstlane((uint32_t)(fd.M >> 32));
        const uint32_t Ml = __builtin_amdgcn_readfirstlane((uint32_t)fd.M);
        const uint32_t Thi = __builtin_amdgcn_readfirstlane((uint32_t)(fd.T >> 32));
        const uint32_t Tlo = __builtin_amdgcn_readfirstlane((uint32_t)fd.T);
        const uint64_t T = ((uint64_t)Thi << 32) | Tlo, M = ((uint64_t)Mh << 32) | Ml;
        const uint32_t fwords = filter_words(m);
        uint32_t pos0[TQ_P], step[TQ_P], acc[TQ_P];
#pragma unroll
        for (int it = 0; it < TQ_P; ++it) {
            if (SMALL_M) { pos0[it] = mod_m_small(h1[it], m, m << 1, Mh, Ml); step[it] = mod_m_small(h2[it], m, m << 1, Mh, Ml); }
            else         { pos0[it] = mod_m(h1[it], m, M);                     step[it] = mod_m(h2[it], m, M); }
            acc[it] = (validmask >> it) << 31;
        }
        for (uint32_t tile0 = 0; tile0 < fwords; tile0 += tile_words) {
            const uint32_t words = fwords - tile0 < tile_words ? fwords - tile0 : tile_words;
            __syncthreads();                                      // previous tile's probes are done
            dma_filter(lds, filters + (uint64_t)f * filter_stride_words32 + tile0, words, wave, lane, nwaves);
            dma_wait_all();
            __syncthreads();
            const uint32_t bit0 = tile0 << 5, nbits = words << 5;
#pragma unroll
            for (int it = 0; it < TQ_P; ++it) {
                uint32_t pos = pos0[it];
                for (uint32_t j = 0; j <= fk; ++j) {               // j == fk: the activated extra probe
                    const uint32_t rel = pos - bit0;
                    const bool in = rel < nbits && (j < fk || ha[it] < T);
                    const uint32_t w = lds[in ? rel >> 5 : 0u];
                    acc[it] &= in ? w << ((pos ^ 24u) & 31u) : 0x80000000u;
                    const uint64_t s2 = (uint64_t)pos + step[it];
                    pos = (uint32_t)(s2 >= m ? s2 - m : s2);
                }
            }
        }
        uint32_t npass = 0, pw_lo = 0, pw_hi = 0;
#pragma unroll
        for (int it = 0; it < TQ_P; ++it) {
            const uint64_t pw = __ballot((int32_t)acc[it] < 0);
            if (lane == (uint32_t)it) { pw_lo = (uint32_t)pw; pw_hi = (uint32_t)(pw >> 32); }
            npass += __popcll(pw);
        }
        if (live) {
            if (lane < TQ_P) pass_words[((uint64_t)f * nseg + seg) * TQ_P + lane] = flip_bytes64(((uint64_t)pw_hi << 32) | pw_lo);
            if (lane == 0) seg_cnt[(uint64_t)f * nseg + seg] = npass;
        }
    }
}

}  // namespace rbf
