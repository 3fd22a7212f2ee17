// rbf_query_f64_pass.h -- one frame's pass of the frames-inner FP64 query kernel (k_query_u64, rbf_kernels_query_f64.h): the probes
// of a lane's 8 pixels against a probe image in LDS, in rows of four independent chains (frame_pass_rows, on rows_reduce4) or pixel by
// pixel (frame_pass_plain: any floor(k*), partial waves).  Not a kernel header: the kernel supplies the staging hook and the outputs.
// Arithmetic: hashes as (RN(h), low dword), h mod m through one v_fma_f64, probe image, activation ranks (rbf_f64_common.h).  (Round 3's
// k_query_s64 / k_query_s64w, the first kernels built on these passes, are in the git history.)
#pragma once
#include "rbf_f64_common.h"

namespace rbf {

#define RBF_ROW() __builtin_amdgcn_sched_barrier(0)

// The two reductions of the two pixels of pair g, as rows of four: x = {pos0, step} of pixel 2g, {pos0, step} of pixel 2g + 1.
// Needs no filter image, so the kernels run pair 0's IN FRONT of the frame's barrier.
__device__ __forceinline__ void rows_reduce4(int g, const double (&hd1)[QL_P], const uint32_t (&hl1)[QL_P], const double (&hd2)[QL_P], const uint32_t (&hl2)[QL_P],
                                             uint32_t m /* VGPR */, double ninv, uint32_t (&x)[4])
{
    const int i0 = 2 * g, i1 = 2 * g + 1;
    const double t0 = __builtin_fma(hd1[i0], ninv, 0x1.8p52), t1 = __builtin_fma(hd2[i0], ninv, 0x1.8p52);
    const double t2 = __builtin_fma(hd1[i1], ninv, 0x1.8p52), t3 = __builtin_fma(hd2[i1], ninv, 0x1.8p52);
    RBF_ROW();
    // r_est = h - q_est * m as an exact SIGNED 32-bit number (mod_m_f64, rbf_f64_common.h, derives the same value modulo 2^24 and
    // sign-extends it): the low dword of t is -q_est mod 2^32 (1.5 * 2^52 has no low bits), hl is h mod 2^32, and
    // |r_est| <= 0.75 m < 2^23.  One multiply-add; then the same fold of a negative r_est back into [0, m).
    const uint32_t s0 = (uint32_t)__builtin_bit_cast(uint64_t, t0) * m + hl1[i0], s1 = (uint32_t)__builtin_bit_cast(uint64_t, t1) * m + hl2[i0];
    const uint32_t s2 = (uint32_t)__builtin_bit_cast(uint64_t, t2) * m + hl1[i1], s3 = (uint32_t)__builtin_bit_cast(uint64_t, t3) * m + hl2[i1];
    RBF_ROW();
    const uint32_t q0 = s0 + m, q1 = s1 + m, q2 = s2 + m, q3 = s3 + m;
    RBF_ROW();
    x[0] = min(s0, q0); x[1] = min(s1, q1); x[2] = min(s2, q2); x[3] = min(s3, q3);
    RBF_ROW();
}

// One frame's pass over a lane's 8 pixels, in pixel PAIRS, written in ROWS: a row holds the same instruction of up to four independent
// chains (the two reductions of the two pixels; for the steps: two chains + the address arithmetic of the probes they feed), rows
// are pinned with sched_barrier.  Per pair g:  reductions(g) | combine(g - 1) | steps + addresses + reads(g) | stager(g): the reads
// of pair g - 1 fly under the reductions of pair g.  `x` arrives holding pair 0's reductions (computed in front of the barrier);
// `after_first_reads()` runs once pair 0's reads are in flight (the kernel puts the previous frame's outputs there); `st.at(g)` is
// the kernel's staging hook (k_query_u64 issues the next image's LDS-DMA at g = 0).
// PRIO: wave priority falls as the wave advances (3, 2, 1, 0 over the four pairs; 0 until the next barrier).  The SIMD's arbiter
// serves the highest priority first and, among equals, the OLDEST wave: left alone the four waves of a SIMD run their passes almost
// one after the other and the youngest finishes alone while fifteen waves stand at the barrier (round 3's query ablation, git history).
template <int FK, bool OVERLAP = true, bool PRIO = true, typename STAGER, typename HOOK>
__device__ __forceinline__ void frame_pass_rows(
    const double (&hd1)[QL_P], const uint32_t (&hl1)[QL_P], const double (&hd2)[QL_P], const uint32_t (&hl2)[QL_P],
    uint32_t rank_lo, uint32_t rank_hi, uint32_t c /* VGPR */, uint32_t lds_base_bytes /* VGPR */, uint32_t safe_pos /* VGPR */, uint32_t m /* VGPR */, double ninv,
    uint32_t (&x)[4], uint32_t &pbf, STAGER &st, HOOK &&after_first_reads)
{
    static_assert(FK >= 1, "at least one deterministic probe");
    constexpr int NP = FK + 1, NG = QL_P / 2;
    // OVERLAP = false (floor(k*) = 5: nearly static frames; 6 would spill): one pair's positions and words at a time -- they are 2 x 2 x 7 registers
    // each otherwise -- and the pair's reads are waited for right behind their issue; the other waves of the SIMD cover them.
    uint32_t pos[OVERLAP ? 2 : 1][2][NP], wrd[OVERLAP ? 2 : 1][2][NP];       // [pair parity][pixel of the pair][probe]
    uint32_t five = 5u;                                            // opaque: written with a literal 5 the compiler folds shift, shift, add into shift, and, add
    asm volatile("" : "+s"(five));
    auto lds_word = [&](uint32_t addr) -> uint32_t { return *reinterpret_cast<const __attribute__((address_space(3))) uint32_t *>((uintptr_t)addr); };
    auto steps_and_reads = [&](int g, const uint32_t (&x)[4]) {    // positions of the pair's probes; every read is issued as soon as its address exists
        const int par = OVERLAP ? g & 1 : 0;
        uint32_t pa = x[0], pb_ = x[2];
        const uint32_t sa = x[1], sb = x[3];
#pragma unroll
        for (int j = 0; j < FK; ++j) {
            pos[par][0][j] = pa; pos[par][1][j] = pb_;
            const uint32_t wa = pa >> five, wb = pb_ >> five;
            const uint32_t ua = pa + sa, ub = pb_ + sb;
            RBF_ROW();
            const uint32_t aa = (wa << 2) + lds_base_bytes, ab = (wb << 2) + lds_base_bytes;
            const uint32_t va = ua - m, vb = ub - m;
            RBF_ROW();
            wrd[par][0][j] = lds_word(aa); wrd[par][1][j] = lds_word(ab);
            pa = min(ua, va); pb_ = min(ub, vb);
            RBF_ROW();
        }
        const int i0 = 2 * g, i1 = 2 * g + 1;
        const uint32_t rk0 = i0 < 4 ? rank_lo : rank_hi, rk1 = i1 < 4 ? rank_lo : rank_hi;
        uint64_t k0, k1;                                           // the pair's activation masks: rank byte <= c
        if ((i0 & 3) == 0) { k0 = rank_le<0>(rk0, c); k1 = rank_le<1>(rk1, c); }
        else { k0 = rank_le<2>(rk0, c); k1 = rank_le<3>(rk1, c); }
        RBF_ROW();
        pos[par][0][FK] = select_by(k0, safe_pos, pa); pos[par][1][FK] = select_by(k1, safe_pos, pb_);   // the activated extra probe, or SAFE
        RBF_ROW();
        const uint32_t wa = pos[par][0][FK] >> five, wb = pos[par][1][FK] >> five;
        RBF_ROW();
        const uint32_t aa = (wa << 2) + lds_base_bytes, ab = (wb << 2) + lds_base_bytes;
        RBF_ROW();
        wrd[par][0][FK] = lds_word(aa); wrd[par][1][FK] = lds_word(ab);
        RBF_ROW();
    };
    auto combine2 = [&](int g) {                                   // verdicts of pair g: the sign bit of `fail` says "some probed filter bit is 0"
        const int par = OVERLAP ? g & 1 : 0;
        uint32_t f0 = 0u, f1 = 0u;
        __builtin_amdgcn_s_waitcnt(0xC07F);                       // lgkmcnt(0), once: left alone the compiler waits in front of each of the six words
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f0 = (wrd[par][0][j] << (pos[par][0][j] & 31u)) | f0;
            f1 = (wrd[par][1][j] << (pos[par][1][j] & 31u)) | f1;
            RBF_ROW();
        }
        pbf = __builtin_amdgcn_alignbit(pbf, f0, 31);             // (pbf << 1) | (fail >> 31)
        RBF_ROW();
        pbf = __builtin_amdgcn_alignbit(pbf, f1, 31);
        RBF_ROW();
    };
    if (PRIO) __builtin_amdgcn_s_setprio(3);
    steps_and_reads(0, x);
    st.at(0);
    RBF_ROW();
    after_first_reads();
    RBF_ROW();
#pragma unroll
    for (int g = 1; g < NG; ++g) {
        if (PRIO) { if (g == 1) __builtin_amdgcn_s_setprio(2); else if (g == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        rows_reduce4(g, hd1, hl1, hd2, hl2, m, ninv, x);          // the reads of pair g - 1 fly under these rows
        combine2(g - 1);
        steps_and_reads(g, x);
        st.at(g);
        RBF_ROW();
    }
    combine2(NG - 1);
    st.at(4);
}

// Any floor(k*) and partial waves (positions past the end of the frame must fail): pixel by pixel, probes in a loop.
template <typename STAGER>
__device__ __forceinline__ void frame_pass_plain(
    const double (&hd1)[QL_P], const uint32_t (&hl1)[QL_P], const double (&hd2)[QL_P], const uint32_t (&hl2)[QL_P],
    uint32_t rank_lo, uint32_t rank_hi, uint32_t c, uint32_t validmask, uint32_t lds_base_bytes, uint32_t safe_pos, uint32_t m, double ninv,
    uint32_t fk, uint32_t &pbf, STAGER &st)
{
#pragma unroll
    for (int it = 0; it < QL_P; ++it) {
        if ((it & 1) == 0) st.at(it >> 1);
        uint32_t pos = mod_m_f64(hd1[it], hl1[it], ninv, m);
        const uint32_t step = mod_m_f64(hd2[it], hl2[it], ninv, m);
        uint32_t fail = ~(validmask << (31 - it)) & 0x80000000u;
        for (uint32_t j = 0; j < fk; ++j) {
            fail = (probe_image_word(lds_base_bytes, pos) << (pos & 31u)) | fail;
            const uint32_t s2 = pos + step;
            pos = min(s2, s2 - m);
        }
        const uint32_t rk = ((it < 4 ? rank_lo : rank_hi) >> (8 * (it & 3))) & 0xFFu;
        const uint32_t pc = rk <= c ? pos : safe_pos;
        fail = (probe_image_word(lds_base_bytes, pc) << (pc & 31u)) | fail;
        pbf = __builtin_amdgcn_alignbit(pbf, fail, 31);
    }
    st.at(4);
}

#undef RBF_ROW

}  // namespace rbf
