/*
 * rbf.h -- C ABI of librbf_hip.so: the MI355X (gfx950) rational-Bloom-filter residual coder.
 *
 * The reference (ross39/new_bloom_filter_repo) is pure Python and has no FFI layer; its
 * boundary for this path is a Python class surface.  Each entry point below names the
 * reference code whose BODY it replaces (file:line under the reference tree); the Python
 * classes in new_bloom_filter_repo_amd/ keep the reference's names and call these through
 * ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - Every function returns 0 (RBF_OK) or a negative errno-style code; it never throws and
 *    never aborts.  rbf_last_error() returns a thread-local, library-owned description of
 *    the most recent failure on the calling thread.
 *  - Pointers named *_dev are DEVICE pointers (HIP global memory); everything else is host
 *    memory owned by the caller.  The library owns what it allocates (context scratch,
 *    rbf_malloc blocks until rbf_free) and nothing it returns outlives the context.
 *  - Bit vectors (masks, filters, witnesses) are packed MSB-first per byte, i.e. exactly
 *    numpy.packbits order: stream bit i lives in byte i>>3 at bit 7-(i&7).  Buffers holding
 *    them must be padded to a multiple of 8 bytes; pad bits are written as 0.
 *  - All work of one context is enqueued on ONE HIP stream (the caller's, or one the library
 *    creates); calls on one context are serialised, different contexts are independent.
 *    One context per thread.  Calls return after ENQUEUEING unless stated otherwise.
 *  - Limits: 1 <= n < 2^32 pixels per frame; 1 <= m <= 2^32-1 filter bits; floor_k <= 64.
 */
#ifndef RBF_H
#define RBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBF_OK        0
#define RBF_EINVAL  (-22)
#define RBF_ENOMEM  (-12)
#define RBF_EIO      (-5)   /* a HIP runtime call failed; see rbf_last_error() */
#define RBF_ERANGE  (-34)

#define RBF_ABI_VERSION 4

typedef struct rbf_ctx rbf_ctx;

/* One filter's geometry, computed on the HOST (float64 via libm must match CPython's `math`
 * to the last ulp -- improved_video_compressor.py:181-196 -- so it never runs on the device).
 *   m          filter length in bits            (l,         improved_video_compressor.py:193)
 *   floor_k    deterministic hash count         (floor(k*), :57)
 *   threshold  activate the extra hash iff XXH64(str(i), act_seed) < threshold
 *              (integer form of `h / (2**64-1) < k* - floor(k*)`, :94-97)                  */
typedef struct {
    uint32_t m;
    uint32_t floor_k;
    uint64_t threshold;
} rbf_filter_params;

/* Hash seeds: (0x12345678, 0x87654321, 999) improved_video_compressor.py:62-63,94;
 * (0, 1, 999) bloom_compress.py:163-164,195; (0, 1, ceil(k*)) rational_bloom_filter.py:100-101,134. */
typedef struct {
    uint64_t h1;
    uint64_t h2;
    uint64_t act;
} rbf_seeds;

/* Per-frame results written by encode (device memory, 4 x uint64 per frame). */
#define RBF_STAT_WITNESS_BITS 0   /* len(witness),            improved_video_compressor.py:253 */
#define RBF_STAT_FILTER_ONES  1   /* popcount of the filter */
#define RBF_STAT_RESERVED0    2
#define RBF_STAT_RESERVED1    3
#define RBF_STATS_PER_FRAME   4

/* ---- library / context ------------------------------------------------------------------ */
int rbf_version(void);
const char *rbf_last_error(void);
int rbf_device_count(int *count);

/* hip_stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream),
 * or NULL to let the library create and own a stream. */
int rbf_ctx_create(int device, void *hip_stream, rbf_ctx **out);
int rbf_ctx_destroy(rbf_ctx *ctx);
int rbf_ctx_sync(rbf_ctx *ctx);                       /* blocks until the stream is idle */

/* Device-memory helpers so host code needs no other GPU runtime. */
int rbf_malloc(rbf_ctx *ctx, size_t bytes, void **out_dev);
int rbf_free(rbf_ctx *ctx, void *ptr_dev);
int rbf_memset(rbf_ctx *ctx, void *dst_dev, int value, size_t bytes);            /* async */
int rbf_memcpy_h2d(rbf_ctx *ctx, void *dst_dev, const void *src, size_t bytes);  /* blocks */
int rbf_memcpy_d2h(rbf_ctx *ctx, void *dst, const void *src_dev, size_t bytes);  /* blocks */
int rbf_memcpy_d2d(rbf_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);   /* async, on the context's stream */

/* Per-kernel HIP-event timing (bench.py): launches of the selected kernels are bracketed by
 * events on the context's stream.  `on`: 0 = off, 1 = every kernel, otherwise a bit mask with
 * bit RBF_K_* set for each kernel to time.  rbf_timing_read blocks until the stream is idle. */
#define RBF_K_MASK    0
#define RBF_K_INSERT  1
#define RBF_K_QUERY   2
#define RBF_K_STITCH  3
#define RBF_K_EXPAND  4
#define RBF_K_GATHER  5
#define RBF_K_SCATTER 6
#define RBF_K_INDEX   7
#define RBF_K_REDUCE  8
#define RBF_K_SCAN    9
#define RBF_K_NOISE   10
#define RBF_K_PACK    11
#define RBF_K_HASHTAB 12      /* k_hash_table: the per-batch table of the pixel indices' three hashes */
#define RBF_K_HOLD    13      /* k_temporal_hold (+ _px): the near-lossless stage in front of the mask stage */
#define RBF_K_COUNT   14
int rbf_timing_enable(rbf_ctx *ctx, int on);
/* Testing / tuning knob (bit mask).  0 (default) = pick the fastest variant that fits.  Only LIVE alternatives are selectable (ABI 3
 * dropped the bits that picked superseded kernels: 6 and 13 are ignored).
 *   bit 0       always the generic (global-memory filter) kernels
 *   bit 1       LDS fast path without double-buffering the filter (the integer Barrett kernels)
 *   bit 2       per-pixel threshold compare in the GOP mask kernel even for threshold 0
 *   bit 3       Barrett reductions only (never the FP64 h mod m, which is taken when every filter of a batch has 2^15 <= m < 2^23)
 *   bit 4       run k_hash_table (the pixel-index hash table the insert kernel gathers from, 26 bytes per pixel in an allocation of 32, shared by the
 *               contexts of a process) for every batch instead of once per (device, frame size, seeds).
 *               FOOTPRINT: the table is process-global device memory -- 32 * (width*height + 512) bytes per (device, frame size,
 *               seeds) in use, e.g. 66 MB at 1080p (54 MB used) -- allocated by the first encode of a geometry and released when the last
 *               context holding it is destroyed or moves to another geometry (including one that never uses a table).  Geometries
 *               whose table would exceed 96 MB (2560x1440 and up) never get one: their insert kernels hash the set positions instead.
 *   bit 5       never use that table: the insert kernel hashes the set positions itself
 *   bit 7       filters of several LDS tiles are inserted by the tiled k_insert_tab even inside rbf_encode_gop (default there:
 *               k_insert_positions + k_insert_records)
 *   bits 8..12  temporal chunks of the GOP mask kernel (0 = auto)
 *   bit 14      k_insert_positions hashes the set positions itself whatever the frame size (default: only when the table would
 *               exceed 96 MB)
 *   bit 15      the query kernel never rewrites the hash table (default: a context that is the table's only holder has it
 *               rewritten in every batch, which keeps it in the Infinity Cache)
 *   bits 16..31 LDS tile cap in units of 64 dwords (0 = all of LDS): forces the tiled kernels */
int rbf_ctx_force_generic(rbf_ctx *ctx, int on);
/* Further testing / tuning knobs.  RBF_OPT_SEPARATE_FINISH (0 / 1): 1 = rbf_encode_gop always hands the ones counts out through the
 * separate k_finish_ones launch (default: inside the GOP mask kernel whenever that kernel covers the whole frame).  (Option 1 of ABI 2,
 * the round-2 query kernel, is gone with that kernel: RBF_EINVAL.) */
#define RBF_OPT_SEPARATE_FINISH 2
/* RBF_OPT_INSERT_SLICES (tuning): mask slices (= partial filters) per frame of the single-tile insert kernel; 0 = auto (about one
 * workgroup per CU for the whole batch).  (Options 3, 5 and 99 of ABI 3 / early ABI 4 -- the side-stream compaction, the grouped insert
 * and the kernel-skipping diagnostic -- are gone: RBF_EINVAL.) */
#define RBF_OPT_INSERT_SLICES 4
int rbf_ctx_option(rbf_ctx *ctx, int option, int64_t value);
int rbf_timing_reset(rbf_ctx *ctx);
int rbf_timing_read(rbf_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches);

/* ---- host-side scalar helpers (no GPU) --------------------------------------------------- */
/* BloomFilterCompressor._calculate_optimal_params with p = ones/n (improved_video_compressor.py:161-196,
 * :211-212).  Returns k=0,l=0 for the reference's "(0, 0)" cases. */
int rbf_optimal_params(uint64_t n, uint64_t ones, double *k, uint64_t *l);
/* floor(k*) and the integer activation threshold T = min{h : RN(h/(2^64-1)) >= k*-floor(k*)}
 * (improved_video_compressor.py:57-58,94-97). */
int rbf_activation_threshold(double k_star, uint32_t *floor_k, uint64_t *threshold);

/* The host step of BloomFilterCompressor.compress for a batch (:211-225): for frame f with
 * ones[f] set bits out of n, fill params[f] (and k[f] if k != NULL).  A frame the reference would
 * NOT Bloom-code (p >= P_STAR, l == 0, or l >= n when guard_l_ge_n != 0) gets params[f].m = 0,
 * which every batch entry point treats as "skip this frame": an empty witness, and a filter row WITHOUT DEFINED CONTENT (the LDS
 * insert kernels leave it alone, the generic path clears every row of the batch). */
int rbf_plan_batch(uint64_t n, const uint64_t *ones, uint32_t nframes, int guard_l_ge_n,
                   rbf_filter_params *params, double *k);

/* ---- A1: residual mask  (VideoFrameCompressor._calculate_frame_diff, :784-808,845) ------- */
/* mask bit = abs_int16(prev - curr) > thr, with numpy's int16 wrap for 16-bit samples; thr is
 * thr_floors[f] for pair f when thr_floors (HOST array of nframes-1 entries) is not NULL -- the
 * adaptive per-frame thresholds of :804-805 -- else thr_floor for every pair.
 * Sample (x, y) of a frame is at base + y*row_pitch_bytes + x*pixel_stride_bytes (so the luma
 * of interleaved YUV444 or a planar plane are both addressable); sample_bytes is 1 or 2.
 * Frame f of the batch is at frames_dev + f*frame_stride_bytes; mask f (f = 0..nframes-2) is the
 * mask between frame f and f+1, written at masks_dev + f*mask_stride_bytes; ones_dev[f] gets
 * np.sum(mask).  mask_stride_bytes must be a multiple of 8 and >= ceil(n/64)*8. */
int rbf_residual_mask_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                            uint32_t nframes, uint32_t width, uint32_t height,
                            uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                            void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev);

/* ---- A1, all-channel mask ------------------------------------------------------------------- */
/* rbf_residual_mask_batch with one more argument.  mask_channels = 1: exactly rbf_residual_mask_batch (the luma rule above).
 * mask_channels >= 2: mask bit = 1 when ANY of the pixel's first mask_channels samples differs between frame f and f+1 -- an exact
 * comparison of the whole sample, not the int16 rule (a 16-bit change of 0x8000 IS marked).  The reference's inter-frame record is
 * (mask, every channel of the masked pixels) (improved_video_compressor.py:811-842) and its _apply_frame_diff writes every channel
 * wherever the mask is 1 (:849-909), so a record built on this mask reconstructs frame f+1 bit for bit even where chroma changed and
 * luma did not -- the luma mask then has to give up the frame.  Lossless only: RBF_EINVAL (before the stream is touched) for
 * mask_channels >= 2 with thr_floor != 0, with thr_floors != NULL, or with mask_channels * sample_bytes > pixel_stride_bytes; and for
 * mask_channels == 0. */
int rbf_residual_mask_batch_ex(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                               uint32_t nframes, uint32_t width, uint32_t height,
                               uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                               uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                               void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev, uint32_t mask_channels);

/* ---- A1, near-lossless: bounded-error temporal hold --------------------------------------------- */
/* In place, on nframes dense interleaved frames (frame f at frames_dev + f*frame_stride_bytes; a frame is width*height pixels of
 * `channels` samples of sample_bytes, no row padding).  Per pixel and run -- run_starts (HOST array of nframes bytes, NULL = one run):
 * frame 0 and every frame f with run_starts[f] != 0 start a run, exactly the keyframes rbf_encode_runs_begin takes --
 *     y_0 = x_0;   y_t = y_{t-1} if |x_t[c] - y_{t-1}[c]| <= max_error for EVERY sample c of the pixel, else y_t = x_t (whole pixel)
 * and frame t is overwritten with y_t; a run's first frame is never written.  The difference is the true unsigned one (16-bit 0 and
 * 0x8000 are 32768 apart; no int16 wrap).  The comparison is against the HELD pixel, so the loop is closed: |y_t - x_t| <= max_error
 * for every sample of every frame, however slowly x drifts, and y_t differs from y_{t-1} exactly where the hold let a pixel through.
 * Coding the held block with the exact all-channel mask (rbf_encode_runs_begin_ex, mask_channels = channels, the same run_starts) is
 * therefore a near-lossless codec with a per-sample bound -- what JPEG-LS calls NEAR.  The reference's knob for sensor noise
 * (noise_tolerance / min_diff_threshold / max_diff_threshold and the thresholded _calculate_frame_diff, improved_video_compressor.py:
 * 768-847) compares luma only, against the previous INPUT frame (open loop: a drift of one level per frame is never coded), and bounds
 * nothing.  Idempotent: holding y gives y.  Deterministic (no atomics).  Asynchronous on the context's stream.
 * Frames whose base and stride are multiples of 16 go through 16-byte accesses, any other sample-aligned layout and the last
 * (width*height) % 16 pixels of a frame through a per-pixel kernel.
 * max_error == 0 or nframes < 2: RBF_OK, nothing is launched.  RBF_EINVAL: channels outside 1..4, sample_bytes not 1 or 2,
 * frames_dev or frame_stride_bytes not a multiple of sample_bytes, frame_stride_bytes < width*height*channels*sample_bytes (with
 * nframes >= 2).  RBF_ERANGE: max_error >= 2^(8*sample_bytes). */
int rbf_temporal_hold_runs(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                           uint32_t max_error, const uint8_t *run_starts);

/* ---- A1, near-lossless: look-ahead temporal hold -------------------------------------------------- */
/* rbf_temporal_hold_runs with another decision rule; the same arguments, layout, runs, checks, error codes and no-op cases.  The hold
 * above keeps a pixel while its samples stay within e = max_error of the segment's FIRST value, so sensor noise of +-a needs e >= 2a.
 * The bound only asks that a segment's samples fit one window of width 2e, so this rule lets a segment run for as long as the windows
 * [x_t - e, x_t + e] of its frames still intersect (greedy interval stabbing: the fewest updates for a fixed first value), and noise of
 * +-a needs e >= a.  Per pixel and run, M = 2^(8*sample_bytes) - 1, true integer differences (no wrap):
 *     y_0 = x_0; a run's first frame is never written.
 *     Anchored segment: while |x_t[c] - x_0[c]| <= e for EVERY sample c, y_t = x_0 (the keyframe is coded exactly).
 *     At the first frame t that breaks this a free segment opens with lo[c] = max(0, x_t[c] - e), hi[c] = min(M, x_t[c] + e).
 *     A following frame u gives lo' = max(lo, max(0, x_u - e)), hi' = min(hi, min(M, x_u + e)); if lo'[c] > hi'[c] for ANY sample the
 *     segment ends at u - 1 and a new free segment opens at u, else lo, hi = lo', hi'.  The end of the run ends the last segment.
 *     A free segment's value is v[c] = clamp(prev[c], lo[c], hi[c]) with prev the previous segment's value (x_0 after the anchored one);
 *     every frame of the segment becomes v, the whole pixel.
 * So |y_t - x_t| <= max_error everywhere, y_t differs from y_{t-1} exactly at the frames where a segment opens (the exact all-channel
 * mask of the result is the set of segment starts), and the samples of a breaking pixel that can keep their value do.  No pixel is
 * updated more often than by rbf_temporal_hold_runs.  NOT idempotent: applied to its own output it can merge segments and double the
 * error -- call it once per uploaded block.  Deterministic (no atomics).  Asynchronous on the context's stream.  Two sweeps over the
 * block and a scratch bitmap of nframes * ceil(width*height/8) bytes that the context keeps.  Frames whose base and stride are
 * multiples of 8 go through 8-byte accesses, any other sample-aligned layout and the last (width*height) % 8 pixels of a frame through
 * a per-pixel kernel.  Timed under RBF_K_HOLD. */
int rbf_temporal_lookahead_runs(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                                uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                                uint32_t max_error, const uint8_t *run_starts);

/* ---- A1, near-lossless: a bound per sample ---------------------------------------------------------- */
/* The two calls above with a BOUND FRAME in place of max_error: bounds_dev is one dense frame of width*height*channels samples of
 * sample_bytes on the device, E[p][c] = the bound of sample c of pixel p, in the frames' own layout and sample type (so every bound
 * fits the sample width by construction).  The same arguments, layout, runs and checks otherwise; the rules are the scalar ones with
 * max_error replaced by E[p][c]:
 *     Hold:       y_t = y_{t-1} if |x_t[c] - y_{t-1}[c]| <= E[p][c] for EVERY sample c of pixel p, else y_t = x_t (the whole pixel).
 *     Look-ahead: the windows are [max(0, x - E[p][c]), min(M, x + E[p][c])]; the anchored segment, the greedy stabbing,
 *                 v[c] = clamp(prev[c], lo[c], hi[c]) and the segment starts are unchanged.
 * What carries over: true unsigned differences (16-bit 0 and 0x8000 are 32768 apart); a run's first frame is never written;
 * |y_t - x_t| <= E[p][c] for every sample of every frame; a pixel whose bounds are all 0 is coded exactly, whatever its neighbours'
 * bounds; the hold is idempotent, the look-ahead is NOT (once per uploaded block) and never updates a pixel more often than the hold;
 * deterministic (no atomics); asynchronous on the context's stream; timed under RBF_K_HOLD.  The bound frame is only read: a lane loads
 * its tile of it once per run, 1 / (run length) of the frames' traffic.
 * bounds_dev's alignment rules are the frames' own: when the frames' base and stride AND bounds_dev are multiples of 16 (look-ahead: 8)
 * the lane tiles run, anything sample-aligned goes through the per-pixel kernels.
 * An all-zero bound frame is legal and leaves the block as it is (the kernels run).  nframes < 2: RBF_OK, nothing is launched.
 * The error codes are those of the scalar calls; a NULL bounds_dev, or one that is not a multiple of sample_bytes, is RBF_EINVAL. */
int rbf_temporal_hold_runs_map(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                               uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                               const void *bounds_dev, const uint8_t *run_starts);
int rbf_temporal_lookahead_runs_map(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                                    uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                                    const void *bounds_dev, const uint8_t *run_starts);

/* ---- A1, BGR input  (cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY), :794-795) --------------------- */
/* gray = (B*3735 + G*19235 + R*9798 + 2^14) >> 15 per pixel -- OpenCV 4.x's integer path for 8- and
 * 16-bit samples; samples 0,1,2 of a pixel are B,G,R (further channels are ignored).  gray_dev receives
 * nframes dense planes of height*width samples, ready for rbf_residual_mask_batch with
 * pixel_stride_bytes = sample_bytes. */
int rbf_bgr_to_gray_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                          uint32_t sample_bytes, void *gray_dev);

/* ---- A1, planar luma -------------------------------------------------------------------------- */
/* luma_dev[f][y*width + x] = sample 0 of pixel (x, y) of frame f: the dense Y planes of a YUV GOP (the reference reads
 * frame[:, :, 0], improved_video_compressor.py:788-791; its YUVFrame wrapper keeps the same plane as a contiguous copy,
 * fixed_video_compressor.py:292-296).  The residual masks only ever look at luma, so a coder that keeps this block resident
 * (rbf_encode_gop / rbf_residual_mask_batch with pixel_stride_bytes = sample_bytes, frame_stride_bytes = width*height*sample_bytes)
 * moves one third of the bytes of the interleaved frames through the mask stage; the interleaved frames are then only touched
 * by the changed-value gather.  One-time pass at upload. */
int rbf_extract_luma_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                           uint32_t sample_bytes, void *luma_dev);

/* ---- A1, adaptive threshold  (VideoFrameCompressor._estimate_noise_level, :727-744) -------- */
/* For each of nframes luma planes (addressed as above): smoothed = 5x5 median with replicated
 * borders (cv2.medianBlur(frame, 5), :738), noise = frame - smoothed (:741).
 *   moments_dev  out: nframes x 2 int64 -- exact sum(noise) and sum(noise^2)
 *   noise_dev    out, nullable: nframes planes of height*width float32, the array whose float32
 *                np.std the reference takes (:744); every value is an exact integer.
 * The standard deviation, the clamp to [min, max] and the floor that turns it into thr_floors
 * (:756-760) are host float work: engine.py does them from the moments, and falls back to the
 * noise plane when rounding could matter. */
int rbf_noise_moments_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                            uint32_t nframes, uint32_t width, uint32_t height,
                            uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, int64_t *moments_dev, float *noise_dev);

/* ---- rows of the Bloom entries: what is read, what is written, what is left alone ------------------------------------------------ */
/* For rbf_bloom_encode_batch, rbf_bloom_decode_batch, rbf_pack_records and rbf_encode_runs_begin(_ex) / rbf_encode_gop_begin +
 * rbf_encode_gop_finish (tests/test_gpu_bloom_row_sweep.py holds every sentence, byte for byte, under poisoned blocks):
 *  - Row f of masks, filters or witnesses lies at base + f * stride_bytes, a 64-bit product: rows may be gigabytes apart.  Every stride is
 *    a multiple of 8 and at least the minimum its entry states.  Every base -- masks_dev, filters_dev, witnesses_dev, stats_dev,
 *    ones_dev, record_dev -- is a multiple of 8: the kernels address them as 64-bit words and add to stats_dev atomically.  Any other base
 *    is RBF_EINVAL ("masks_dev must be 8-byte aligned", ...) before anything is enqueued, and nothing is written.  Nothing needs more than
 *    8: rows that are not 16-byte aligned, or a stride that is no multiple of 16, take the kernels' 4- and 8-byte paths.
 *  - Nothing is written outside [base, base + nframes * stride_bytes) of an output role, and input rows are never written.
 *  - Mask rows as INPUT (encode, pack): the first ceil(n/64)*8 bytes of a row are the mask, the pad bits of its last word must be 0 (the
 *    mask stage writes them so; the record of an m == 0 frame carries the word as it is).  Nothing behind them is read.
 *  - Filter rows as OUTPUT: a coded row (m != 0) is written over its WHOLE STRIDE -- the filter's ceil(m/64)*8 bytes, bits past m zero,
 *    followed by zeros up to filter_stride_bytes.  So filters_dev must be a block of nframes * filter_stride_bytes bytes: one sized for
 *    the filters alone is overrun, and rows a stride of gigabytes apart cost gigabytes of stores.  The row of an m == 0 frame or of a
 *    skipped pair has NO DEFINED CONTENT (the LDS insert kernels leave it alone, the generic path clears it).
 *  - Witness rows as OUTPUT: the first stats[f][RBF_STAT_WITNESS_BITS] bits, zero-padded to a whole 64-bit word, are defined; what lies
 *    behind that word in the row is unspecified (left alone or zeroed; nothing is written from byte ceil(n/64)*8 + 8 of a row on).  An
 *    m == 0 frame or a skipped pair has zero bits: nothing of its row is defined.
 *  - stats_dev as OUTPUT: all RBF_STATS_PER_FRAME words of every row; the reserved ones, and every word of an m == 0 frame or a skipped
 *    pair, are 0.
 *  - Mask rows as OUTPUT (decode; the mask stage of the runs entries): the first ceil(n/64)*8 bytes, pad bits 0; the rest of the row is
 *    left alone.  A frame with m == 0 decodes to an all-zero mask (its filter and witness rows are not read); a skipped pair's row is zero.
 *  - Filter and witness rows as INPUT (decode, pack): of a filter row the ceil(m/64)*8 bytes of the filter count -- what else the row
 *    holds up to its stride may be read and is ignored; of a witness row only the words that hold the frame's witness_bits bits are
 *    read, so decode takes any witness stride >= the largest ceil(witness_bits/64)*8 of the batch, below ceil(n/64)*8.
 *  - record_dev: the header and the record's used bytes (word [2]) are written, nothing behind them. */

/* ---- A4 + A5: insert + query/witness  (BloomFilterCompressor.compress loops, :232-253) --- */
/* For each frame f: zero filter f, insert every '1' position of mask f
 * (RationalBloomFilter.add_index, :99-114), then test every position 0..n-1 in order
 * (check_index, :116-138) and append mask bit i to the witness when it passes.
 *   masks_dev     nframes packed masks, stride mask_stride_bytes
 *   params        nframes host structs
 *   filters_dev   out: nframes packed filters, stride filter_stride_bytes >= ceil(m/64)*8 for every m of the batch; a coded row is written
 *                 over its whole stride, so the block is nframes * filter_stride_bytes bytes (rows of the Bloom entries, above)
 *   witnesses_dev out: nframes packed witnesses, stride witness_stride_bytes >= ceil(n/64)*8; the first stats[f][RBF_STAT_WITNESS_BITS]
 *                 bits of row f are the witness, zero-padded to whole 64-bit words -- what lies behind them in the row is unspecified
 *   stats_dev     out: nframes x RBF_STATS_PER_FRAME uint64
 * More than 128 frames are coded in chunks of 128 rows, each at its place in the caller's strides. */
int rbf_bloom_encode_batch(rbf_ctx *ctx, const void *masks_dev, uint64_t mask_stride_bytes,
                           uint64_t n, uint32_t nframes, const rbf_filter_params *params,
                           const rbf_seeds *seeds,
                           void *filters_dev, uint64_t filter_stride_bytes,
                           void *witnesses_dev, uint64_t witness_stride_bytes,
                           uint64_t *stats_dev);

/* ---- A1 + A3 + A4 + A5 for a whole GOP in one call ----------------------------------------- */
/* residual masks of the nframes-1 consecutive pairs -> ones to the host -> rbf_plan_batch ->
 * insert + query.  Blocks once in the middle (the parameter math needs the ones counts on the
 * host); the Bloom kernels are enqueued when it returns.  params_out / k_out (host, nframes-1
 * entries, nullable) receive the per-frame geometry so the caller can size and label the output.
 * filter_stride_bytes must cover every planned filter (0.32*n bits always suffices). */
int rbf_encode_gop(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                   uint32_t nframes, uint32_t width, uint32_t height,
                   uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                   uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                   const rbf_seeds *seeds,
                   void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                   void *filters_dev, uint64_t filter_stride_bytes,
                   void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev,
                   rbf_filter_params *params_out, double *k_out);

/* The same in two phases (`..._masks()` -> host parameter math -> `..._blooms()`; the reference does these steps one
 * after the other per frame, improved_video_compressor.py:198-266 -- mask, :211-215 parameters, :235-237 insert, :245-253 query).
 *   rbf_encode_gop_begin   checks EVERY argument first (a bad call touches neither the stream nor the caller's buffers), enqueues the
 *                          mask stage (its last workgroup publishes the set-bit counts into pinned host memory and the
 *                          stats rows are cleared on the way) and returns without waiting.
 *   rbf_encode_gop_poll    *ready = 1 once the counts have arrived (never blocks).
 *   rbf_encode_gop_finish  waits for the counts, runs rbf_plan_batch, enqueues insert / reduce / query / compaction; params_out /
 *                          k_out as for rbf_encode_gop.  Clears the pending state even when it fails.
 * One GOP per context may be between begin and finish (a second begin returns RBF_EINVAL); the buffers named in begin must stay
 * valid until the kernels enqueued by finish have run.  A thread that feeds several contexts issues begin(k+1) before finish(k) and
 * never stands still while a mask kernel runs; rbf_encode_gop is begin + finish. */
int rbf_encode_gop_begin(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                         uint32_t nframes, uint32_t width, uint32_t height,
                         uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                         uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                         const rbf_seeds *seeds,
                         void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                         void *filters_dev, uint64_t filter_stride_bytes,
                         void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev);
int rbf_encode_gop_poll(rbf_ctx *ctx, int *ready);

/* SEVERAL keyframe-delimited runs of one clip in ONE launch sequence (SURVEY.md 8b `rbf_encode_batch ... GOP batching`).  The reference
 * codes frame by frame (improved_video_compressor.py:198-266) and has no GOP loop (:1236-1268); a caller that holds a clip whose frame t
 * is a keyframe iff t % keyframe_interval == 0 hands over up to a few hundred consecutive frames at once and every fixed cost of the
 * launch sequence -- the query kernel's hashing prologue, the mask kernel's ramp and tail, five launches -- is paid once per block
 * instead of once per GOP.
 *   run_starts   HOST array of nframes bytes, nullable (= one run, rbf_encode_gop_begin).  run_starts[t] != 0 for t >= 1: frame t is a
 *                keyframe of the caller's stream, it starts a new run, and PAIR t-1 (frame t against frame t-1) IS NOT CODED: its mask
 *                row is written as zeros, ones_dev[t-1] = 0, its stats are zero (an empty witness), its filter row holds NO DEFINED CONTENT afterwards (the
 *                LDS insert kernels never write it, the generic path clears every row of the batch: read nothing from it),
 *                params_out[t-1] = {m = 0, floor_k = RBF_PAIR_SKIPPED, 0}, k_out[t-1] = 0, and rbf_pack_records gives it a header row
 *                with no payload.  run_starts[0] is ignored.  No frame of a run is read by the mask stage of another run.
 * Everything else as rbf_encode_gop_begin / rbf_encode_gop; rbf_encode_gop_poll / rbf_encode_gop_finish complete either kind of begin.
 * Both begins check EVERY argument before they touch the stream or the caller's buffers.
 * PRECONDITION SINCE ABI 4 (a caller written against ABI 3 that sized the filter rows from its own density bound gets RBF_EINVAL now):
 *   filter_stride_bytes >= rbf_filter_stride_min(width * height), a multiple of 8.
 * The filters are planned in the second half, from counts the first half has not seen yet, so the stride must cover the largest filter
 * the planner can produce for the frame size (l <= 0.31606 n for every density, :181-193) -- ask rbf_filter_stride_min, do not guess. */
#define RBF_PAIR_SKIPPED 0xFFFFFFFFu
uint64_t rbf_filter_stride_min(uint64_t n);
int rbf_encode_runs_begin(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                          uint32_t nframes, uint32_t width, uint32_t height,
                          uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                          uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                          const uint8_t *run_starts, const rbf_seeds *seeds,
                          void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                          void *filters_dev, uint64_t filter_stride_bytes,
                          void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev);
/* rbf_encode_runs_begin with the mask rule of rbf_residual_mask_batch_ex (mask_channels: 1 = luma, exactly rbf_encode_runs_begin;
 * >= 2 = all-channel, same argument checks).  Runs, skipped pairs, counts and filters as rbf_encode_runs_begin; rbf_encode_gop_poll /
 * rbf_encode_gop_finish complete it. */
int rbf_encode_runs_begin_ex(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                             uint32_t nframes, uint32_t width, uint32_t height,
                             uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                             uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                             const uint8_t *run_starts, const rbf_seeds *seeds,
                             void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                             void *filters_dev, uint64_t filter_stride_bytes,
                             void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev, uint32_t mask_channels);
int rbf_encode_runs(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                    uint32_t nframes, uint32_t width, uint32_t height,
                    uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                    uint32_t sample_bytes, int32_t thr_floor, const int32_t *thr_floors,
                    const uint8_t *run_starts, const rbf_seeds *seeds,
                    void *masks_dev, uint64_t mask_stride_bytes, uint64_t *ones_dev,
                    void *filters_dev, uint64_t filter_stride_bytes,
                    void *witnesses_dev, uint64_t witness_stride_bytes, uint64_t *stats_dev,
                    rbf_filter_params *params_out, double *k_out);
int rbf_encode_gop_finish(rbf_ctx *ctx, rbf_filter_params *params_out, double *k_out);

/* ---- exact-size record of a batch (what the gather to rank 0 moves) ------------- */
/* Compacts the padded output rows of an encode into ONE contiguous self-describing block on the
 * device, without the host learning the witness lengths.  Little-endian uint64 words:
 *   [0] "RBFREC01"  [1] nframes  [2] used bytes  [3] 1 if capacity_bytes was too small (payload incomplete)
 *   per frame 8 words: m, floor_k, threshold, k (float64 bits), witness_bits, filter_ones,
 *                      filter_offset, witness_offset (bytes from the start of the block)
 *   payload, 8-byte aligned rows: filter ceil(m/64)*8 bytes -- or, for a frame the reference does
 *   not Bloom-code (m == 0; :215-225 returns the input itself), its packed mask ceil(n/64)*8 bytes --
 *   and witness ceil(witness_bits/64)*8 bytes.
 * params / k: the host arrays rbf_encode_gop or rbf_plan_batch filled (k nullable -> 0.0).
 * rbf_record_max_bytes: a capacity that can never overflow. */
uint64_t rbf_record_max_bytes(uint32_t nframes, uint64_t n);
int rbf_pack_records(rbf_ctx *ctx, uint32_t nframes, uint64_t n, const rbf_filter_params *params, const double *k,
                     const void *masks_dev, uint64_t mask_stride_bytes,
                     const void *filters_dev, uint64_t filter_stride_bytes,
                     const void *witnesses_dev, uint64_t witness_stride_bytes,
                     const uint64_t *stats_dev, void *record_dev, uint64_t capacity_bytes);

/* ---- A6: decode  (BloomFilterCompressor.decompress loop, :286-307) ------------------------ */
/* out mask bit i = witness[w++] if position i passes the filter, else 0.  filter_stride_bytes >= ceil(m/64)*8 for every m of the batch;
 * witness_stride_bytes: any multiple of 8 (it may be smaller than ceil(n/64)*8); a caller who wants every witness bit read gives one
 * that holds every frame's witness bits.  The filter decides how many positions pass, not the caller: where a frame passes more positions
 * than its row holds bits -- a damaged or foreign filter --, a witness bit at or past witness_stride_bytes * 8 reads as 0, and nothing
 * outside row f is read (tests/test_gpu_foreign_decode.py).  mask_stride_bytes >= ceil(n/64)*8.  What is read and written in a row: rows
 * of the Bloom entries, above. */
int rbf_bloom_decode_batch(rbf_ctx *ctx, const void *filters_dev, uint64_t filter_stride_bytes,
                           const void *witnesses_dev, uint64_t witness_stride_bytes,
                           uint64_t n, uint32_t nframes, const rbf_filter_params *params,
                           const rbf_seeds *seeds,
                           void *masks_dev, uint64_t mask_stride_bytes);

/* ---- per-index surface  (RationalBloomFilter.add_index / check_index, :99-138) ----------- */
/* filter_dev is a packed filter of params->m bits.  indices_dev: count uint32 indices. */
int rbf_filter_insert_indices(rbf_ctx *ctx, void *filter_dev, const rbf_filter_params *params,
                              const rbf_seeds *seeds, const uint32_t *indices_dev, uint64_t count);
/* out_dev[i] = 1 if indices_dev[i] passes, else 0 (one byte per index). */
int rbf_filter_query_indices(rbf_ctx *ctx, const void *filter_dev, const rbf_filter_params *params,
                             const rbf_seeds *seeds, const uint32_t *indices_dev, uint64_t count,
                             uint8_t *out_dev);

/* ---- string-keyed twins  (rational_bloom_filter.py) ----------------------------------------- */
/* Keys are arbitrary byte strings: key i = keys_dev[offsets_dev[i] .. offsets_dev[i+1]) (count+1
 * uint32 offsets).  standard_k == 0: RationalBloomFilter.add / contains (rational_bloom_filter.py:
 * 139-182; seeds (0, 1, ceil(k*))); standard_k > 0: StandardBloomFilter.add / contains (:29-41), k
 * independent hashes XXH64(key, seed=j) % m (params->m; floor_k / threshold / seeds unused). */
int rbf_filter_insert_keys(rbf_ctx *ctx, void *filter_dev, const rbf_filter_params *params,
                           const rbf_seeds *seeds, uint32_t standard_k,
                           const uint8_t *keys_dev, const uint32_t *offsets_dev, uint64_t count);
int rbf_filter_query_keys(rbf_ctx *ctx, const void *filter_dev, const rbf_filter_params *params,
                          const rbf_seeds *seeds, uint32_t standard_k,
                          const uint8_t *keys_dev, const uint32_t *offsets_dev, uint64_t count,
                          uint8_t *out_dev);

/* ---- A2 / A8: changed-value gather / scatter  (:811-842, :886-903) ------------------------ */
/* Gather, in raster order, the `channels` samples of every pixel whose mask bit is 1 out of
 * an interleaved frame (sample c of pixel (x,y) at base + y*row_pitch + x*pixel_stride + c*sample_bytes)
 * into values_dev (count*channels samples); count_dev gets the number of pixels. */
int rbf_gather_values(rbf_ctx *ctx, const void *frame_dev, uint32_t width, uint32_t height,
                      uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes, uint32_t sample_bytes,
                      uint32_t channels, const void *mask_dev, void *values_dev, uint64_t *count_dev);
/* The same for every pair of a GOP in one call: pair f (f = 0..nframes-2) gathers from frame f+1
 * under mask f; the blocks are concatenated in frame order, pair f starting at pixel offsets_dev[f]
 * (offsets_dev: nframes entries, the last one = total changed pixels), i.e. at sample
 * offsets_dev[f]*channels of values_dev.  Nothing is written past capacity_pixels pixels.
 * uncovered_dev (nullable, nframes-1 entries): pixels whose mask bit is 0 although some channel
 * differs between frame f and f+1 -- changes a luma-only mask cannot carry (:849-909 applies the
 * mask to all channels), which a lossless caller must route to a keyframe. */
int rbf_gather_values_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                            uint32_t width, uint32_t height, uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes,
                            uint32_t sample_bytes, uint32_t channels, const void *masks_dev, uint64_t mask_stride_bytes,
                            void *values_dev, uint64_t capacity_pixels, uint64_t *offsets_dev, uint64_t *uncovered_dev);
/* Inverse: write values back at the mask's '1' pixels (frame_dev is updated in place). */
int rbf_scatter_values(rbf_ctx *ctx, void *frame_dev, uint32_t width, uint32_t height,
                       uint64_t row_pitch_bytes, uint32_t pixel_stride_bytes, uint32_t sample_bytes,
                       uint32_t channels, const void *mask_dev, const void *values_dev);

/* ---- sample codec: prediction residuals in a chunked Rice code (no reference counterpart) ---------- */
/* The opt-in replacement of the record formats' zlib-9 for keyframes and changed values.  A SAMPLE STREAM codes N samples of B = 8 or 16
 * bits: '<I' N | '<B' B | 3 zero bytes | k[C] | '<H' words[C] | zero padding to 4 bytes | the payload as '<I' words, C = ceil(N / 1024).
 * Sample x with prediction pred: s = (x - pred) mod 2^B read as B-bit two's complement, u = 2s (s >= 0) or -2s - 1.  Chunk c codes samples
 * [1024c, 1024c + 1024) from payload word words[0] + ... + words[c-1]; bit j of a chunk is bit (j & 31) of its word j >> 5; k[c] in [0, B] is
 * the parameter of fewest bits (the smallest on a tie): k == B stores the B bits of u; otherwise q = u >> k < 16 is q one-bits, a zero-bit and
 * the k low bits of u, and q >= 16 is 16 one-bits and the B bits of u (bits least significant first).  words[c] = ceil(chunk bits / 32).
 * Frames are DENSE: height x width pixels of `channels` (1..4) interleaved samples, sample_bytes 1 or 2 (B = 8 * sample_bytes).
 * Every entry checks its arguments -- B, channels, capacities, and a stream's header and table against its length -- before it launches
 * anything: RBF_EINVAL with rbf_last_error().
 *
 * Keyframes: pred = the same channel of the pixel to the left; in column 0 of the pixel above; 0 for the first pixel.
 *   rbf_rice_encode_intra  the streams of nframes frames (frame f at frames_dev + f * frame_stride_bytes), back to back at out_dev;
 *                          stream_bytes (host, nframes) receives their sizes.  capacity_bytes must hold every stream stored raw:
 *                          sum over streams of 4 * (ceil((8 + 3C) / 4) + sum over chunks ceil(chunk samples * B / 32)).  Blocks.
 *   rbf_rice_decode_intra  one stream (HOST memory) of width * height * channels samples back into the dense frame at frame_dev.  Waits for the
 *                          decode: a chunk whose codes do not end inside its declared words gives RBF_EINVAL and frame_dev is not written.
 * Inter-frames: pred = the same sample of frame t-1, at the pixels whose mask bit is 1 (raster order, channels interleaved).
 *   rbf_rice_encode_inter  pair f (f = 0..nframes-2: frame f+1 against frame f under mask f, rows as in rbf_gather_values_batch) gets the stream
 *                          of its ones[f] * channels residuals; ones (host, nframes-1 entries) are the masks' set-bit counts (RBF_EINVAL after the
 *                          run when a mask disagrees); a pair with ones[f] = 0 gets the 8-byte empty stream.  Layout, capacity and
 *                          stream_bytes as for the keyframes.  Blocks.
 *   rbf_rice_apply_inter   count streams (HOST memory, back to back, sizes in stream_bytes) against count masks: frames_dev holds count + 1
 *                          dense frames, slot 0 = the frame in front of the run; slot j + 1 becomes slot j with pred + s written at mask j's '1'
 *                          pixels.  Decodes every stream and checks every mask's count first: on any failure no frame slot is written. */
int rbf_rice_encode_intra(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                          void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes);
int rbf_rice_decode_intra(rbf_ctx *ctx, const void *stream, uint64_t stream_bytes, uint32_t width, uint32_t height,
                          uint32_t channels, uint32_t sample_bytes, void *frame_dev);
int rbf_rice_encode_inter(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                          const void *masks_dev, uint64_t mask_stride_bytes, const uint64_t *ones,
                          void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes);
int rbf_rice_apply_inter(rbf_ctx *ctx, const void *streams, const uint64_t *stream_bytes, uint32_t count,
                         uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                         const void *masks_dev, uint64_t mask_stride_bytes, void *frames_dev);

/* ---- bounded-error keyframes: the quantiser inside the keyframe predictor (no reference counterpart) ---------- */
/* A keyframe within a bound per channel instead of exact (record type 7 of 'BFV2' containers: the type-3 head '<IIIBB' height, width,
 * itemsize, channels, yuv | '<B' version = 1 | '<B' n = max(1, channels) | n x '<H' d_c | zero padding to 4 bytes | a sample stream of
 * height * width * n samples).  THE RULE (normative).  Frame X is (H, W, C) with B-bit samples, channel c has bound d_c and step
 * t_c = 2 d_c + 1, S is an integer state per sample, the order is raster order:
 *     P(y, x, c) = S(y, x-1, c) for x > 0;  P(y, 0, c) = S(y-1, 0, c) for y > 0;  P(0, 0, c) = 0      (the type-3 neighbours)
 *     d_c >= 1:  e = X - P;  q = sgn(e) * floor((|e| + d_c) / t_c);  S = P + q t_c;  Y = clamp(S, 0, 2^B - 1)
 *     d_c == 0:  q = (X - P) mod 2^B read as B-bit two's complement;  S = X;  Y = X                    (the type-3 rule)
 *     stream sample u = 2q for q >= 0, -2q - 1 otherwise
 * So |X - Y| <= |X - S| <= d_c, S stays in [-d_c, 2^B - 1 + d_c], |q| <= (2^B + 1) / 3 and u < 2^B.  The stream is an unchanged sample
 * stream: N = H W C, chunks of 1024, the same rule for k, channels interleaved.  A decoder sums q t_c down column 0 and along every row
 * (32-bit wrap-around arithmetic is exact: every true partial sum is in range), then Y = clamp(sum) where d_c >= 1 and sum mod 2^B where
 * d_c == 0.  Y is a pure function of (X, d): two blocks that hold the same keyframe get the same Y.  The loop has a closed form: it
 * starts at 0 and moves in multiples of t_c, so S = t_c * floor((X + d_c) / t_c) whatever the neighbours are -- S is never negative, the
 * upper clamp binds where a multiple of t_c lies just above 2^B - 1, and quantising Y again gives Y.
 *   the encode entry  quantises the `count` frames frame_index[0] < frame_index[1] < ... (host; frame i of the block lies at frames_dev +
 *                     i * frame_stride_bytes, dense as above; an index is < 65535) IN PLACE -- each becomes its Y -- and writes their
 *                     streams back to back at out_dev; stream_bytes (host, count) receives their sizes, capacity_bytes as for
 *                     rbf_rice_encode_intra.  No other frame of the block is touched.  Blocks.
 *   the decode entry  one stream (HOST memory) back into the dense frame Y at frame_dev, as rbf_rice_decode_intra does for type 3.
 * bounds: `channels` host entries, each <= 65535.  Arguments, capacities and stream headers are checked before anything is launched:
 * RBF_EINVAL with rbf_last_error(), and a refused call writes neither frames nor output.  Not timed: there is no RBF_K_ id for them. */
int rbf_rice_encode_intra_near(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, const uint32_t *frame_index, uint32_t count,
                               uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes, const uint32_t *bounds,
                               void *out_dev, uint64_t capacity_bytes, uint64_t *stream_bytes);
int rbf_rice_decode_intra_near(rbf_ctx *ctx, const void *stream, uint64_t stream_bytes, uint32_t width, uint32_t height,
                               uint32_t channels, uint32_t sample_bytes, const uint32_t *bounds, void *frame_dev);

/* ---- integrity: frame digests (no reference counterpart) ------------------------------------------ */
/* FD1, the digest a container stores per frame so that a decoder can prove, without the originals, that it rebuilt the frames the
 * encoder coded (record type 5 of 'BFV2' containers: '<B' version = 1 | '<B' algo = 1 | '<H' 0 | '<I' count | count x '<Q' digest |
 * '<Q' FD1 of all preceding body bytes; only as the last record, count = the frame records in front of it).  A frame's bytes are its dense
 * C-order (height, width, channels) samples, little-endian.  Arithmetic mod 2^64; P1..P5 are the XXH64 primes:
 *     round(acc, x) = rotl64(acc + x*P2, 31) * P1
 *     merge(a, b)   = (a ^ round(0, b)) * P1 + P4
 *     aval(h)       : h ^= h>>33; h *= P2; h ^= h>>29; h *= P3; h ^= h>>32
 *     block(w[0..511], seed)          one 4096-byte block, zero-padded, as 512 little-endian u64
 *       for lane l in 0..63:  acc[l] = seed + P5 + l*P1
 *       for row r in 0..3, half h in 0..1, every lane l:  acc[l] = round(acc[l], w[128*r + 2*l + h])
 *       for d in 1,2,4,8,16,32:  for every l that is a multiple of 2d:  acc[l] = merge(acc[l], acc[l+d])
 *       the block's hash is aval(acc[0])
 *     FD1(bytes b, L = len(b)):
 *       while len(b) > 4096:  b = the hashes of b's blocks, block j zero-padded and seeded with j, as '<Q' each
 *       FD1 = block(b zero-padded to 4096, seed = L)
 * The layout is a wave's: one wave hashes one block, lane l reads the 16 bytes at 1024*r + 16*l of each row (four coalesced 16-byte
 * loads), the 64 accumulators fold in six cross-lane steps.  merge is not commutative (swapped lanes, rows, halves and blocks all change
 * the result) and L in the last seed separates a frame from its zero-extended twin.  FD1 of the empty string is 0x19044D0607DE195D.
 *
 * rbf_frame_digest_batch: FD1 of nframes byte ranges [frames_dev + f*frame_stride_bytes, +frame_bytes); digests_dev: nframes uint64
 * (device), asynchronous on the context's stream; 1 + (number of levels) launches whatever nframes is.  Base and stride multiples of 16:
 * 16-byte loads; any other layout: a generic path.  Nothing outside the byte ranges is read.  frame_bytes >= 1, frame_stride_bytes >=
 * frame_bytes unless nframes <= 1 (RBF_EINVAL otherwise); nframes == 0 is a no-op.
 * rbf_frame_digest_host: the same digest of host memory in plain C++: no GPU, no context. */
int rbf_frame_digest_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                           uint64_t frame_bytes, uint64_t *digests_dev);
uint64_t rbf_frame_digest_host(const void *bytes, uint64_t nbytes);

/* ---- scene cuts: is a frame cheaper as a keyframe than as an inter-frame? -------------------------------------------------------- */
/* Read-only, on nframes dense interleaved frames (the layout of rbf_temporal_hold_runs: frame f at frames_dev + f*frame_stride_bytes, a
 * frame is width*height pixels of `channels` (1..4) samples of B = 8*sample_bytes bits, no row padding).  For a sample x with
 * prediction pred:
 *     u = rice_map((x - pred) mod 2^B)         the sample codec's mapping: 2d for d < 2^(B-1), else 2(2^B - d) - 1
 *     glen(u) = 2*floor(log2(u + 1)) + 1       the Elias-gamma length of u + 1 (u + 1 formed in 32 bits): an integer proxy for code
 *                                              length that needs no Rice parameter.  glen(0) = 1, glen(1) = glen(2) = 3,
 *                                              glen(255) = 17, glen(65535) = 33.
 * For every pair t = 1 .. nframes-1, stats_dev[3*(t-1) ..] receives three uint64:
 *     moving      the pixels with at least one sample where |x_t[c] - x_{t-1}[c]| > tolerance -- the true unsigned difference, as in the
 *                 hold: 16-bit samples 0 and 0x8000 are 32768 apart
 *     inter_bits  the sum over the moving pixels, and over all their samples, of glen(u) with pred = x_{t-1}
 *     intra_bits  the sum over all samples of frame t of glen(u) with the type-3 predictor: the same channel of the pixel to the left,
 *                 of the pixel above in column 0, and 0 for the first pixel
 * Frame t is a CUT iff inter_bits + moving > intra_bits (one bit per moving pixel for the mask): an integer rule without a tunable
 * constant, applied by the caller (container.cut_frames).  Deterministic: the kernels write per-wave partial sums into scratch the
 * context keeps and a second kernel folds them; no atomics.  Asynchronous on the context's stream; every frame is read once.  Frames
 * whose base and stride are multiples of 16 go through 16-byte loads, any other sample-aligned layout, the last (width*height) % 16
 * pixels and frames of fewer than 16 pixels through a per-pixel kernel.
 * nframes < 2: RBF_OK, nothing is launched.  RBF_EINVAL: channels outside 1..4, sample_bytes not 1 or 2, a null pointer, frames_dev or
 * frame_stride_bytes not a multiple of sample_bytes, stats_dev not a multiple of 8, frame_stride_bytes < width*height*channels*
 * sample_bytes.  RBF_ERANGE: tolerance >= 2^B.  Everything is checked before anything is launched. */
int rbf_cut_stats(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                  uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                  uint32_t tolerance, uint64_t *stats_dev);   /* 3 * (nframes - 1) uint64, device */

/* ---- quality report: what does a coded block differ from its originals by? ------------------------------------------------------- */
/* Read-only, on two resident blocks of nframes dense interleaved frames of one geometry (the layout of rbf_temporal_hold_runs): A, the
 * originals, frame f at a_dev + f*a_stride_bytes, and B, the coded frames, at b_dev + f*b_stride_bytes.  rows_host (HOST, nframes rows)
 * receives for frame f, over all its width*height*channels samples, with the true unsigned difference of the hold:
 *     sse         the sum of (a - b)^2, exact (64-bit integers)
 *     differing   the samples with a != b
 *     over_bound  the samples with |a - b| > their bound: E[p][c] when bounds_dev is a bound frame (the bound frame of
 *                 rbf_temporal_hold_runs_map), the scalar `bound` for every sample when bounds_dev is NULL
 *     max_abs     the largest |a - b|
 * so that MSE = sse / samples and PSNR = 10 log10((2^B - 1)^2 / MSE) are the caller's to form.  Deterministic: the kernels write
 * per-wave partial sums into scratch the context keeps and a second kernel folds them; no atomics.  BLOCKS until the rows are on the
 * host.  Blocks and bounds whose bases and strides are multiples of 16 go through 16-byte loads, any other sample-aligned layout and the
 * last (width*height) % 16 pixels of a frame through a per-pixel kernel.  Not timed: there is no RBF_K_ id for it, as for rbf_cut_stats.
 * nframes == 0: RBF_OK, nothing is launched.  RBF_EINVAL: channels outside 1..4, sample_bytes not 1 or 2, a null a_dev, b_dev or
 * rows_host, a base, stride or bounds_dev that is not a multiple of sample_bytes, a stride < width*height*channels*sample_bytes (with
 * nframes >= 2).  RBF_ERANGE: bound >= 2^B with bounds_dev NULL; more than 2^31 samples per frame.  Everything is checked before anything
 * is launched. */
typedef struct { uint64_t sse, differing, over_bound; uint32_t max_abs, reserved; } rbf_error_row;
int rbf_error_stats(rbf_ctx *ctx, const void *a_dev, uint64_t a_stride_bytes, const void *b_dev, uint64_t b_stride_bytes,
                    uint32_t nframes, uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                    const void *bounds_dev, uint32_t bound, rbf_error_row *rows_host);

/* ---- hold sweep: what would every candidate bound do to every run of a block? ---------------------------------------------------- */
/* Read-only, on a resident block in the layout of rbf_temporal_hold_runs, with runs as there: frame 0 and every frame f with
 * run_starts[f] != 0 (HOST, nframes bytes, NULL: one run) start one.  candidates (HOST) are ncandidates = 1..8 strictly ascending
 * bounds, each <= 255 (0 is legal as the first).  rows_host (HOST, runs * ncandidates rows; runs counted in frame order, a run of one
 * frame included) receives in row r * ncandidates + i, for run r and Y = the block that rbf_temporal_hold_runs (lookahead == 0) or
 * rbf_temporal_lookahead_runs (lookahead != 0) would leave with max_error = candidates[i] -- neither is run, nothing is written --
 * over the run's frames, with the true unsigned difference of the hold:
 *     sse      the sum of (X - Y)^2 over every sample, exact (the run's first frame contributes 0)
 *     updates  the (pixel, frame) pairs with Y_t(p) != Y_{t-1}(p): the sum of the run's all-channel mask counts
 *     max_abs  the largest |X - Y|
 * A run of one frame has all fields 0; with candidate 0, Y = X: sse = 0 and updates is the exact mask count.  ONE read of the block
 * serves every candidate: a lane owns a pixel of a run and walks the run's frames once with the state of four candidates in registers
 * (more than four: two halves of a workgroup share a tile staged in LDS).  Under the look-ahead rule a segment's value is known only
 * when it closes; the kernel keeps the segment's length n and, per sample, the first and second moments S1, S2 of d = x - (the segment's
 * first sample), their min and max, and adds S2 - 2 w S1 + n w^2 on close (w = value - first sample).  Deterministic: per-wave partial
 * sums go into scratch the context keeps and a second kernel folds them; no atomics.  BLOCKS until the rows are on the host.  A block
 * whose base and stride are multiples of 16 goes through 16-byte loads in tiles of 256 pixels (128 with more than four candidates), any
 * other sample-aligned layout and the pixels behind the last whole tile through a per-pixel kernel.  Not timed: there is no RBF_K_ id
 * for it, as for rbf_cut_stats.  nframes == 0: RBF_OK, nothing is launched or written.
 * RBF_EINVAL: channels outside 1..4, sample_bytes not 1 or 2, a null frames_dev, candidates or rows_host, a base or stride that is not
 * a multiple of sample_bytes, a stride < width*height*channels*sample_bytes, ncandidates outside 1..8, candidates that do not strictly
 * ascend.  RBF_ERANGE: a candidate > 255 (or >= 2^B); more than 128 runs; a run of more than 128 frames.  Everything is checked before
 * anything is launched, and rows_host is untouched by a refused call. */
typedef struct { uint64_t sse, updates; uint32_t max_abs, reserved; } rbf_sweep_row;
int rbf_hold_sweep(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                   uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                   const uint8_t *run_starts, int lookahead,
                   const uint32_t *candidates, uint32_t ncandidates, rbf_sweep_row *rows_host);

/* ---- pan alignment: the global integer shift of a pair, and the roll that makes a block still ------------------------------------ */
/* During a camera pan every pixel differs from the pixel at the same position one frame earlier; shifted by the pan it does not.  Let
 * F_f(p)[c] be sample c of pixel p = (x, y) of frame f, Y_f(p) = F_f(p)[0]; a pair is frame f against frame f-1; R is the range
 * (1..32) and G = 8 a fixed grid step.  Frames are W x H, with W > 2R and H > 2R.
 *     grid          the points (x, y) with x in {R, R+G, ...} < W-R and y in {R, R+G, ...} < H-R.  Interior addressing only: no wrap.
 *     SAD_f(dx,dy)  = sum over the grid of |Y_f(x+dx, y+dy) - Y_{f-1}(x, y)| for |dx|, |dy| <= R: an unsigned 64-bit sum of true
 *                   absolute differences (16-bit samples 0 and 0x8000 are 32768 apart: no int16 wrap).
 *     best shift    the candidate that minimises the tuple (SAD, |dx|+|dy|, |dy|, dy, dx) lexicographically: (0, 0) wins every tie.
 *     moving_f(v)   the number of pixels p of the WHOLE frame for which some sample c of the first `channels` samples has
 *                   |F_f((p+v) mod (W,H))[c] - F_{f-1}(p)[c]| > tolerance.  Cyclic addressing: exactly what the mask of the rolled
 *                   block will mark.
 *     rule          (host, integers, no tunable constant: container.pan_offsets) the pair adopts v_f = best iff
 *                   moving_f(best) < moving_f(0), else v_f = 0.
 *     offsets       c_f = 0 at frame 0 and at every run start, else c_f = c_{f-1} + v_f, stored reduced to 0 <= ox < W, 0 <= oy < H.
 *     stabilised    S_f(p) = F_f((p + c_f) mod (W,H)).  Pair f of the stabilised block differs in exactly moving_f(v_f) pixels.
 * The model is integer translation: a sub-pixel pan leaves edge residue, and nothing is interpolated.  A cyclic shift is a bijection:
 * it loses nothing and needs no border side information; the pixels that wrap around are the newly revealed picture content and get
 * coded as changed pixels.
 *
 * rbf_pan_search: frames dense and interleaved as for rbf_cut_stats.  out (HOST, nframes-1 rows) receives for pair f = 1..nframes-1 row
 * f-1 = {dx, dy of the best shift; sad_zero = SAD(0,0); sad_best; moving_zero = moving(0); moving_best = moving(best)} (moving_best =
 * moving_zero when best = (0,0)); the row of a pair in front of a run start (run_starts: HOST, nframes bytes, nullable; entry t != 0 =
 * frame t starts a run) is all zeros.  A workgroup stages a tile of frame f plus a halo of R in LDS and walks the (2R+1)^2 candidates
 * over it; per-workgroup partial sums are folded and the tie-break applied on the device, where the moving kernel reads the shift: no
 * atomics, deterministic.  BLOCKS until the rows are on the host.  Not timed: there is no RBF_K_ id for it, as for rbf_cut_stats.
 * nframes < 2: RBF_OK, nothing is launched.  RBF_EINVAL, with `out` untouched and before anything is launched: range outside 1..32,
 * width or height <= 2*range, channels outside 1..4, sample_bytes not 1 or 2, tolerance >= 2^B, a null pointer, a base or stride that is
 * not a multiple of sample_bytes, a stride smaller than a frame.
 *
 * rbf_roll_frames: in place on nframes frames of width x height pixels of pixel_bytes (1..8) bytes, no row padding, frame f at
 * frames_dev + f*frame_stride_bytes:  new_f(x, y) = old_f((x + ox_f) mod W, (y + oy_f) mod H), (ox_f, oy_f) = offsets[2f], offsets[2f+1]
 * (HOST; any int32, reduced mod W / H).  A frame whose reduced offsets are zero is neither read nor written; bytes between a frame's end
 * and the next frame's start are never written.  Frames are rolled, a few at a time, into scratch the context keeps and copied back: the
 * source is never the destination.  Rows of a multiple of 16 bytes move as 16-byte vectors, others byte by byte.  Asynchronous on the
 * context's stream.  A decoder calls it with the negated offsets.  RBF_EINVAL: pixel_bytes outside 1..8, an empty frame, a null
 * pointer, a stride smaller than a frame. */
typedef struct { int32_t dx, dy; uint64_t sad_zero, sad_best, moving_zero, moving_best; } rbf_pan_stat;
int rbf_pan_search(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                   uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                   uint32_t range, uint32_t tolerance, const uint8_t *run_starts, rbf_pan_stat *out);
int rbf_roll_frames(rbf_ctx *ctx, void *frames_dev, uint64_t frame_stride_bytes, uint32_t nframes,
                    uint32_t width, uint32_t height, uint32_t pixel_bytes, const int32_t *offsets);

/* ---- views: a region of a frame, reduced by a box mean (no reference counterpart) ---------------------------------------------- */
/* A reader that wants part of a clip -- a frame range, a region, a reduced preview -- takes it where the rebuilt frames lie, so that
 * only the view crosses to the host.  A VIEW of a dense (H, W, C) frame of B-bit samples is given by a region (x0, y0, w, h) and a
 * scale s in {1, 2, 4, 8}:
 *     region     w, h >= 1, x0 + w <= W, y0 + h <= H.
 *     output     dense (ceil(h/s), ceil(w/s), C), of the same sample type.
 *     blocks     output pixel (Y, X) covers the source pixels x0 + sX .. min(x0 + sX + s, x0 + w) - 1 by
 *                y0 + sY .. min(y0 + sY + s, y0 + h) - 1: the block grid hangs off the region's corner, and a ragged last block
 *                averages over the cnt pixels it has.
 *     rule       per channel, out = floor((2*sum + cnt) / (2*cnt)) with sum the sum of the block's cnt samples of that channel.  For
 *                a full block that is (sum + s*s/2) >> 2*log2(s); with s = 1 it is a plain crop.
 * All values are integers and the rule rounds half up (a 2x2 block that sums to 4q + 2 gives q + 1, one that sums to 4q + 1 gives q).
 * The largest numerator is 2*64*65535 + 64: 32 bits are enough.  No other filter: a box mean, nothing is interpolated.
 *
 * rbf_frame_view_batch: the views of `count` frames of a resident block, written back to back at out_dev (view j at out_dev +
 * j * ceil(h/s)*ceil(w/s)*channels*sample_bytes).  frame_index (HOST, count entries, ascending): frame i lies at frames_dev +
 * i*frame_stride_bytes -- the slot addressing of a chain block, the convention of rbf_rice_encode_intra_near; every offset is formed in
 * 64 bits.  Read-only on the frames; asynchronous on the context's stream.  Where every source row the region touches starts on a
 * 16-byte boundary (frames_dev, frame_stride_bytes, width*channels*sample_bytes and x0*channels*sample_bytes multiples of 16) the full
 * blocks go through 16-byte loads in whole lane tiles of 16 / gcd(16, s*channels*sample_bytes) output pixels; what that leaves -- the
 * columns behind the last whole tile, the ragged last rows -- and the whole view of tiny frames and of every other layout go through a
 * kernel with one lane per output sample, launched over those output pixels only.  Not timed: there is no RBF_K_ id for it, as for
 * rbf_cut_stats.
 * count == 0: RBF_OK, nothing is launched.  RBF_EINVAL, before anything is launched and with out_dev untouched: a scale outside
 * {1, 2, 4, 8}, an empty region or one that leaves the frame, channels outside 1..4, sample_bytes not 1 or 2, a null pointer, a base or
 * stride that is not a multiple of sample_bytes, frame_stride_bytes < width*height*channels*sample_bytes, indices that do not ascend,
 * capacity_bytes smaller than the count views, out_dev's range overlapping the source span [frames_dev, frames_dev +
 * last index * frame_stride_bytes + a frame). */
int rbf_frame_view_batch(rbf_ctx *ctx, const void *frames_dev, uint64_t frame_stride_bytes,
                         const uint32_t *frame_index, uint32_t count,
                         uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes,
                         uint32_t x0, uint32_t y0, uint32_t roi_w, uint32_t roi_h, uint32_t scale,
                         void *out_dev, uint64_t capacity_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RBF_H */
