// rbf_mask_plan.h -- the temporal chunks of the GOP mask kernels (rbf_kernels_mask.h): the table they take as a kernel argument and the
// host arithmetic that fills it.  Pure host code over rbf_plan.h's Knobs: no HIP header, so tests/c/mask_plan_cases.cpp is built with a
// plain host compiler and runs on a machine without a GPU (tests/test_mask_stage_cpu.py).
#pragma once
#include "rbf_plan.h"

#include <algorithm>
#include <cstdint>

namespace rbf {

// The temporal chunks of one launch (blockIdx.y).  count == 0: uniform chunks of `ppc` pairs over the whole block (one run).  Otherwise
// chunk y reads frames first[y] .. first[y] + pairs[y] and writes the mask rows first[y] .. first[y] + pairs[y] - 1 -- so a block that
// holds SEVERAL keyframe-delimited runs (rbf_encode_runs) is cut at the keyframes: no chunk reads across one, the pair in front of a
// keyframe is never diffed.  pairs[y] & MASK_CHUNK_SKIP: those pairs are NOT coded; their rows are written as zeros, nothing is counted.
constexpr uint32_t MASK_MAX_CHUNKS = 256, MASK_CHUNK_SKIP = 0x8000u;
struct MaskChunks {
    uint32_t count, ppc;
    uint16_t first[MASK_MAX_CHUNKS], pairs[MASK_MAX_CHUNKS];
};

}  // namespace rbf

// Temporal chunks of the fast mask kernel: enough waves to fill the chip (>= ~32 per CU) without re-reading much.  Returns the chunk
// count (blockIdx.y).  *skip_in_table: the chunk table cuts the block at its keyframes, so the fast kernel needs no threshold trick.
static uint32_t plan_mask_chunks(const Knobs &k, uint32_t nframes, uint64_t fast_segs, const uint8_t *skip, MaskChunks *mc, bool *skip_in_table)
{
    const uint32_t pairs = nframes - 1;
    const uint32_t wanted = k.mask_chunks ? k.mask_chunks : (uint32_t)((6500 + fast_segs - 1) / fast_segs);   // 4 at 1080p (measured best)
    *mc = MaskChunks{};
    *skip_in_table = false;
    uint32_t coded = pairs;
    if (skip) { coded = 0; for (uint32_t i = 0; i < pairs; ++i) coded += skip[i] ? 0u : 1u; }
    uint32_t chunks = std::max(1u, std::min(wanted, coded));
    uint32_t ppc = std::max(1u, (coded + chunks - 1) / chunks);
    if (skip && nframes < MASK_CHUNK_SKIP) {
        uint32_t cnt = 0;
        bool fits = true;
        for (uint32_t a = 0; a < pairs && fits;) {
            uint32_t b = a;
            while (b < pairs && (skip[b] != 0) == (skip[a] != 0)) ++b;
            const uint32_t len = b - a;
            if (skip[a]) {
                if (cnt >= MASK_MAX_CHUNKS) { fits = false; break; }
                mc->first[cnt] = (uint16_t)a; mc->pairs[cnt] = (uint16_t)(len | MASK_CHUNK_SKIP); ++cnt;
            } else {
                const uint32_t c = (len + ppc - 1) / ppc, per = (len + c - 1) / c;     // this run in c chunks of about ppc pairs
                for (uint32_t x = a; x < b; x += per) {
                    if (cnt >= MASK_MAX_CHUNKS) { fits = false; break; }
                    mc->first[cnt] = (uint16_t)x; mc->pairs[cnt] = (uint16_t)(b - x < per ? b - x : per); ++cnt;
                }
            }
            a = b;
        }
        if (fits && cnt) { mc->count = cnt; *skip_in_table = true; return cnt; }
        *mc = MaskChunks{};
    }
    if (skip) {         // (a block of more runs than the table holds) uniform chunks over everything, the skipped pairs through their thresholds
        chunks = std::min(wanted, pairs);
        ppc = (pairs + chunks - 1) / chunks;
    }
    mc->ppc = ppc;
    return (pairs + ppc - 1) / ppc;
}
