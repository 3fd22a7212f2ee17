// rbf_geometry.h -- what host planning (rbf_plan.h) and the kernels must agree on: launch constants, LDS layout sizes and the plain
// structs that travel as kernel arguments.  No HIP header, no device code: any C++17 host compiler takes it.  Each group names the
// header whose kernels it sizes; the reasons for the values are there, next to the code.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rbf {

constexpr int WAVE = 64;

// Per-frame filter geometry as the kernels see it.
struct FrameDev {
    uint32_t m;        // filter bits
    uint32_t floor_k;  // deterministic probes
    uint64_t T;        // activation threshold: extra probe iff h_act < T
    uint64_t M;        // floor(2^64 / m) for m >= 2 (Barrett reciprocal); unused when m == 1
};

struct Seeds { uint64_t h1, h2, act; };

// A batch's geometry travels BY VALUE in the kernel-argument segment (3 KiB of the 4 KiB limit):
// no upload, no device buffer, and the per-frame fields arrive through scalar loads.
constexpr int MAX_BATCH = 128;
struct FrameTable { FrameDev f[MAX_BATCH]; };
struct SliceTable { uint8_t n[MAX_BATCH]; };     // insert: partial filters (mask slices) per frame, 0 = frame not coded

// ---- generic path (rbf_kernels.h) and the stages that work in workgroups of 256 threads
constexpr int SEG_PIXELS = 1024;                 // pixels per segment (one wave)
constexpr int WG_THREADS = 256;

// ---- Barrett kernels (rbf_kernels_barrett.h); the FP64 query kernels share the query's workgroup and segment shape
constexpr int QL_THREADS = 1024;                   // 16 waves, one workgroup per CU, filter double-buffered in LDS
constexpr int QL_WAVES = QL_THREADS / WAVE;
constexpr int QL_P = 8;                            // pixels per lane
constexpr int QL_SEG_PIXELS = QL_P * WAVE;         // 512

constexpr int IL_THREADS = 1024;                   // insert: one workgroup per CU
constexpr int IL_WAVES = IL_THREADS / WAVE;
constexpr int IL_QUEUE = 64 + 512;                 // carry (<64) + one wave-step of 64 mask bytes

constexpr int TQ_P = 8;                            // k_query_tiled: pixels per lane
constexpr int TQ_SEG_PIXELS = TQ_P * WAVE;         // 512

// ---- table-driven insert (rbf_kernels_insert_f64.h)
constexpr int IT_STEP_BYTES = 128;                 // mask bytes per wave step: a lane owns 16 pixels (two bytes)
constexpr int IT_CHUNK_STEPS = 16;                 // wave steps whose mask bytes are staged in LDS at a time
constexpr int IT_QUEUE = 64 + IT_STEP_BYTES * 8;   // queue entries (16 bits each): carry (< 64) + one wave step
constexpr int IT_STAGE_BYTES = IT_CHUNK_STEPS * IT_STEP_BYTES;
constexpr int IT_WAVE_LDS_BYTES = IT_QUEUE * 2 + IT_STAGE_BYTES;      // per wave: the queue, then the staged mask bytes (4224)

// ---- FP64 kernels: eligible filter sizes (rbf_f64_common.h: mod_m_f64), LDS behind the image buffers of k_query_u64
// (rbf_kernels_query_f64.h) and of k_query_s64t (rbf_kernels_query_f64_tiled.h)
constexpr uint32_t F64MOD_M_MIN = 1u << 15, F64MOD_M_MAX = (1u << 23) - 1u;      // eligible filter sizes (host: make_plan, rbf_plan.h)
constexpr uint32_t U64_REC_BYTES = 32;
constexpr uint32_t u64_geo_bytes(uint32_t nactive) { return (nactive + 1u) * U64_REC_BYTES; }   // LDS behind the two image buffers: one record per coded frame + 1
constexpr int U64_CLASSES = 6;                                    // floor(k*) = 1, 2, 3, 4, 5 in rows, then everything else (plain pass)
struct U64Classes { uint32_t n[U64_CLASSES]; };                  // coded frames per class, in the order of the compacted table

constexpr uint32_t S64_GEO_BYTES = MAX_BATCH * 16;                 // k_query_s64t: 16 bytes of geometry per coded frame
constexpr uint32_t s64t_geo_word(uint32_t tile_words) { return tile_words + 4u > 4u * MAX_BATCH ? tile_words + 4u : 4u * MAX_BATCH; }
constexpr size_t s64t_lds_bytes(uint32_t tile_words) { return (size_t)s64t_geo_word(tile_words) * 4 + S64_GEO_BYTES; }

}  // namespace rbf
