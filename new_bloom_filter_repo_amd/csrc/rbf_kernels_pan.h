// rbf_kernels_pan.h -- pan alignment of a block of dense interleaved frames: the global integer shift of every pair (k_pan_sad, k_pan_pick),
// how many pixels still move with and without it (k_pan_moving, k_pan_moving_reduce) and the cyclic roll that makes the block still
// (k_roll_frames, its byte-wise twin k_roll_frames_bytes).  include/rbf.h (rbf_pan_search, rbf_roll_frames) has the normative text:
//   grid        the points (x, y), x in {R, R+8, ...} < W-R, y in {R, R+8, ...} < H-R: interior only, no wrap
//   SAD(dx,dy)  = sum over the grid of |Y_f(x+dx, y+dy) - Y_{f-1}(x, y)|, |dx|, |dy| <= R, Y = sample 0, the true unsigned difference
//   best        the candidate with the smallest (SAD, |dx|+|dy|, |dy|, dy, dx)
//   moving(v)   pixels p of the whole frame with a sample c where |F_f((p+v) mod (W,H))[c] - F_{f-1}(p)[c]| > tolerance (cyclic)
// The search kernels only read the frames.  No atomics: a workgroup of k_pan_sad writes its (2R+1)^2 sums to a row of its own, a wave of
// k_pan_moving its two counts; k_pan_pick and k_pan_moving_reduce fold a pair's rows into its rbf_pan_stat row ON THE DEVICE, so that
// k_pan_moving reads the shift it has to test without a host round trip.  Integer sums: the result is deterministic.
#pragma once
#include "rbf_kernels.h"

namespace rbf {

constexpr int PAN_GRID = 8, PAN_TX = 16, PAN_TY = 8;              // the grid step; a workgroup's tile of grid points
constexpr int PAN_MAX_RANGE = 32;

// The row of a pair as the ABI declares it (rbf_pan_stat).
struct PanRow {
    int32_t dx, dy;
    uint64_t sad_zero, sad_best, moving_zero, moving_best;
};

// Samples of an LDS tile row of k_pan_sad: (8 TX - 7 + 2R) used, the pitch rounded up to an ODD number of dwords so that lanes on
// different rows (different dy) fall on different banks.
__host__ __device__ __forceinline__ constexpr uint32_t pan_tile_pitch_bytes(uint32_t range, uint32_t sample_bytes)
{
    const uint32_t dwords = ((PAN_GRID * PAN_TX + 2 * range) * sample_bytes + 3) / 4;
    return 4 * (dwords | 1u);
}
__host__ __device__ __forceinline__ constexpr uint32_t pan_tile_rows(uint32_t range) { return PAN_GRID * PAN_TY + 2 * range; }
__host__ __device__ __forceinline__ constexpr uint32_t pan_sad_lds_bytes(uint32_t range, uint32_t sample_bytes)
{
    return pan_tile_pitch_bytes(range, sample_bytes) * pan_tile_rows(range) + PAN_TX * PAN_TY * 4;
}
// The candidates a lane of k_pan_sad owns: one dy and `chunk` consecutive dx -- with nd = 2R + 1 rows of candidates and floor(256 / nd)
// lanes per row, chunk = ceil(nd / lanes per row).  CH(RMAX) bounds it for every R <= RMAX (chunk grows with nd).
__host__ __device__ __forceinline__ constexpr uint32_t pan_chunk(uint32_t range)
{
    const uint32_t nd = 2 * range + 1, per_row = WG_THREADS / nd;
    return (nd + per_row - 1) / per_row;
}

// k_pan_sad: workgroup (blockIdx.x = tile, blockIdx.y = pair) owns the PAN_TX x PAN_TY grid points of its tile of pair (f-1, f),
// f = blockIdx.y + 1.  It stages the channel-0 samples of frame f under the tile plus a halo of R into LDS -- tile row r, column c is
// frame pixel (8 TX tx + c, 8 TY ty + r): grid point (i, j) of the tile with candidate (dx, dy) is tile entry (8 i + R + dx, 8 j + R + dy) --
// and the tile's grid samples of frame f-1.  A lane keeps ONE dy and a chunk of consecutive dx in registers and walks the tile's grid
// points: per grid point it reads its chunk of one LDS row once.  Frames that are not whole tiles go through the same code: an entry
// outside the frame is staged as 0 and belongs to no valid grid point's window (x < W-R, y < H-R), and the walk stops at the tile's last
// valid grid point (nx, ny).  The sums of a tile are at most 128 * 65535: they fit 32 bits.
// partials[((pair * tiles + tile) * nd + (dy + R)) * nd + (dx + R)].  A pair in front of a run start is not looked at (k_pan_pick zeroes
// its row).  RMAX: the largest range of this instantiation (it sizes the lane's registers).
template <typename SAMPLE, int RMAX>
__global__ __launch_bounds__(WG_THREADS) void k_pan_sad(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t width, uint32_t height,
                                                        uint32_t channels, uint32_t range, uint32_t ngx, uint32_t ngy, uint32_t tiles_x,
                                                        const uint8_t *__restrict__ run_starts, uint32_t *__restrict__ partials)
{
    constexpr int CH = (int)pan_chunk(RMAX);
    extern __shared__ __align__(16) uint8_t pan_lds[];
    const uint32_t pair = blockIdx.y, tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    if (run_starts[pair + 1]) return;                             // (the same for the whole workgroup)
    const uint32_t pitch = pan_tile_pitch_bytes(range, sizeof(SAMPLE)), rows = pan_tile_rows(range);
    const uint32_t cols = PAN_GRID * (PAN_TX - 1) + 1 + 2 * range;                  // the columns some window can reach
    uint32_t *const pg = reinterpret_cast<uint32_t *>(pan_lds + (size_t)pitch * rows);     // the grid samples of frame f-1
    const SAMPLE *const cur = reinterpret_cast<const SAMPLE *>(frames + (uint64_t)(pair + 1) * frame_stride);
    const SAMPLE *const prev = reinterpret_cast<const SAMPLE *>(frames + (uint64_t)pair * frame_stride);
    const uint32_t x0 = PAN_GRID * PAN_TX * tx, y0 = PAN_GRID * PAN_TY * ty;
    for (uint32_t r = threadIdx.x >> 6; r < rows; r += WG_WAVES) {
        const uint32_t y = y0 + r;
        SAMPLE *const row = reinterpret_cast<SAMPLE *>(pan_lds + (size_t)pitch * r);
        for (uint32_t c = threadIdx.x & 63u; c < cols; c += 64) {
            const uint32_t x = x0 + c;
            row[c] = (x < width && y < height) ? cur[((uint64_t)y * width + x) * channels] : (SAMPLE)0;
        }
    }
    const uint32_t gx0 = PAN_TX * tx, gy0 = PAN_TY * ty;
    const uint32_t nx = ngx - gx0 < (uint32_t)PAN_TX ? ngx - gx0 : (uint32_t)PAN_TX, ny = ngy - gy0 < (uint32_t)PAN_TY ? ngy - gy0 : (uint32_t)PAN_TY;
    if (threadIdx.x < PAN_TX * PAN_TY) {
        const uint32_t i = threadIdx.x % PAN_TX, j = threadIdx.x / PAN_TX;
        uint32_t v = 0;
        if (i < nx && j < ny) {
            const uint64_t x = range + PAN_GRID * (gx0 + i), y = range + PAN_GRID * (gy0 + j);
            v = prev[(y * width + x) * channels];
        }
        pg[threadIdx.x] = v;
    }
    __syncthreads();
    const uint32_t nd = 2 * range + 1, per_row = WG_THREADS / nd, chunk = (nd + per_row - 1) / per_row;
    const uint32_t a = threadIdx.x / per_row, b0 = (threadIdx.x % per_row) * chunk;      // dy + R, the first dx + R
    if (a >= nd || b0 >= nd) return;                              // (behind the last barrier)
    // Every lane walks CH candidates without a branch: those behind its chunk, or behind the last dx, read on in the tile row (at most
    // CH - 1 samples past the last window: still inside the tile, whose last row no window reaches) and are not stored.
    uint32_t acc[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) acc[q] = 0;
    for (uint32_t j = 0; j < ny; ++j) {
        const SAMPLE *const row = reinterpret_cast<const SAMPLE *>(pan_lds + (size_t)pitch * (PAN_GRID * j + a)) + b0;
        for (uint32_t i = 0; i < nx; ++i) {
            const uint32_t p = pg[j * PAN_TX + i];
            const SAMPLE *const win = row + PAN_GRID * i;
#pragma unroll
            for (int q = 0; q < CH; ++q) acc[q] = __usad((uint32_t)win[q], p, acc[q]);
        }
    }
    uint32_t *const out = partials + (((uint64_t)pair * gridDim.x + tile) * nd + a) * nd;
#pragma unroll
    for (int q = 0; q < CH; ++q)
        if ((uint32_t)q < chunk && b0 + q < nd) out[b0 + q] = acc[q];
}

// The order of the best shift: (SAD, |dx| + |dy|, |dy|, dy, dx), smallest first -- (0, 0) wins every tie.  Behind the SAD the order is
// that of ONE integer: the four fields, each below 256, packed most significant first (dy and dx offset by R: ascending all the same).
__device__ __forceinline__ uint32_t pan_rank(int32_t dx, int32_t dy, uint32_t range)
{
    const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
    return ((ax + ay) << 24) | (ay << 16) | ((uint32_t)(dy + (int32_t)range) << 8) | (uint32_t)(dx + (int32_t)range);
}

// One workgroup per pair: folds the pair's `tiles` rows of k_pan_sad per candidate (uint64), picks the best and writes dx, dy, sad_zero
// and sad_best of the pair's row; the row of a pair in front of a run start becomes all zeros (moving counts included: k_pan_moving_reduce
// leaves such a row alone).
__global__ __launch_bounds__(WG_THREADS) void k_pan_pick(const uint32_t *__restrict__ partials, uint32_t tiles, uint32_t range,
                                                         const uint8_t *__restrict__ run_starts, PanRow *__restrict__ rows)
{
    __shared__ uint64_t best_sad[WG_THREADS];
    __shared__ uint32_t best_rank[WG_THREADS];
    __shared__ uint64_t zero_sad;
    const uint32_t pair = blockIdx.x, nd = 2 * range + 1, nc = nd * nd;
    if (run_starts[pair + 1]) {
        if (threadIdx.x == 0) rows[pair] = PanRow{0, 0, 0, 0, 0, 0};
        return;
    }
    const uint32_t *const in = partials + (uint64_t)pair * tiles * nc;
    uint64_t my_sad = ~0ull;
    uint32_t my_rank = ~0u;                                        // (no candidate: loses against every real one)
    for (uint32_t c = threadIdx.x; c < nc; c += WG_THREADS) {
        uint64_t s = 0;
        for (uint32_t t = 0; t < tiles; ++t) s += in[(uint64_t)t * nc + c];
        const int32_t dx = (int32_t)(c % nd) - (int32_t)range, dy = (int32_t)(c / nd) - (int32_t)range;
        const uint32_t rank = pan_rank(dx, dy, range);
        if (dx == 0 && dy == 0) zero_sad = s;
        if (s < my_sad || (s == my_sad && rank < my_rank)) { my_sad = s; my_rank = rank; }
    }
    best_sad[threadIdx.x] = my_sad;
    best_rank[threadIdx.x] = my_rank;
    __syncthreads();
    for (uint32_t step = WG_THREADS / 2; step > 0; step >>= 1) {
        if (threadIdx.x < step) {
            const uint64_t s = best_sad[threadIdx.x + step];
            const uint32_t rank = best_rank[threadIdx.x + step];
            if (s < best_sad[threadIdx.x] || (s == best_sad[threadIdx.x] && rank < best_rank[threadIdx.x])) {
                best_sad[threadIdx.x] = s;
                best_rank[threadIdx.x] = rank;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        PanRow r = rows[pair];                                     // (the moving counts are k_pan_moving_reduce's)
        r.dx = (int32_t)(best_rank[0] & 0xFFu) - (int32_t)range; r.dy = (int32_t)((best_rank[0] >> 8) & 0xFFu) - (int32_t)range;
        r.sad_zero = zero_sad; r.sad_best = best_sad[0];
        rows[pair] = r;
    }
}

constexpr uint32_t PAN_COUNTS = 2;                                // moving(0), moving(best)

// k_pan_moving: a thread owns ONE pixel p of pair blockIdx.y and compares F_{f-1}(p) with F_f(p) and, where the pick chose a shift, with
// F_f((p + best) mod (W, H)) -- all C samples, the true unsigned difference against the tolerance.  A wave writes its two counts to a row
// of its own: partials[(pair * rows + row) * 2 + j]; every row of every coded pair is written by every call.  Any sample-aligned layout.
template <typename SAMPLE, int C>
__global__ __launch_bounds__(WG_THREADS) void k_pan_moving(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t width, uint32_t height,
                                                           uint32_t tolerance, const uint8_t *__restrict__ run_starts,
                                                           const PanRow *__restrict__ picks, uint32_t *__restrict__ partials, uint64_t rows)
{
    const uint32_t pair = blockIdx.y;
    if (run_starts[pair + 1]) return;
    const uint64_t n = (uint64_t)width * height, px = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    const int32_t dx = picks[pair].dx, dy = picks[pair].dy;       // (uniform: scalar loads)
    const bool shifted = dx != 0 || dy != 0;
    uint32_t m0 = 0, m1 = 0;
    if (px < n) {
        const uint32_t y = (uint32_t)(px / width), x = (uint32_t)(px - (uint64_t)y * width);
        const SAMPLE *const a = reinterpret_cast<const SAMPLE *>(frames + (uint64_t)pair * frame_stride) + px * C;
        const SAMPLE *const cur = reinterpret_cast<const SAMPLE *>(frames + (uint64_t)(pair + 1) * frame_stride);
        const SAMPLE *const b = cur + px * C;
        uint32_t pa[C], worst = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            pa[c] = a[c];
            const uint32_t d = __usad(pa[c], (uint32_t)b[c], 0u);
            worst = d > worst ? d : worst;
        }
        m0 = worst > tolerance ? 1u : 0u;
        m1 = m0;
        if (shifted) {
            int32_t sx = (int32_t)x + dx, sy = (int32_t)y + dy;  // |dx|, |dy| <= R < W, H: one step brings them back
            sx = sx < 0 ? sx + (int32_t)width : (sx >= (int32_t)width ? sx - (int32_t)width : sx);
            sy = sy < 0 ? sy + (int32_t)height : (sy >= (int32_t)height ? sy - (int32_t)height : sy);
            const SAMPLE *const s = cur + ((uint64_t)sy * width + (uint32_t)sx) * C;
            worst = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint32_t d = __usad(pa[c], (uint32_t)s[c], 0u);
                worst = d > worst ? d : worst;
            }
            m1 = worst > tolerance ? 1u : 0u;
        }
    }
    m0 = wave_sum_to_lane63(m0 | (m1 << 16));                     // (two counts of at most 64)
    if ((threadIdx.x & 63u) == 63u) {
        uint32_t *const out = partials + ((uint64_t)pair * rows + (uint64_t)blockIdx.x * WG_WAVES + (threadIdx.x >> 6)) * PAN_COUNTS;
        out[0] = m0 & 0xFFFFu; out[1] = m0 >> 16;
    }
}

// moving_zero and moving_best of pair blockIdx.x = the sums of the pair's rows.
__global__ __launch_bounds__(WG_THREADS) void k_pan_moving_reduce(const uint32_t *__restrict__ partials, uint64_t rows,
                                                                  const uint8_t *__restrict__ run_starts, PanRow *__restrict__ out)
{
    __shared__ uint64_t part[PAN_COUNTS][WG_THREADS];
    const uint32_t pair = blockIdx.x;
    if (run_starts[pair + 1]) return;
    const uint32_t *const in = partials + (uint64_t)pair * rows * PAN_COUNTS;
    uint64_t acc[PAN_COUNTS] = {0, 0};
    for (uint64_t r = threadIdx.x; r < rows; r += WG_THREADS)
#pragma unroll
        for (uint32_t j = 0; j < PAN_COUNTS; ++j) acc[j] += in[r * PAN_COUNTS + j];
#pragma unroll
    for (uint32_t j = 0; j < PAN_COUNTS; ++j) part[j][threadIdx.x] = acc[j];
    __syncthreads();
    if (threadIdx.x < PAN_COUNTS) {
        uint64_t s = 0;
        for (uint32_t i = 0; i < WG_THREADS; ++i) s += part[threadIdx.x][i];
        if (threadIdx.x == 0) out[pair].moving_zero = s; else out[pair].moving_best = s;
    }
}

// ---- the roll ----
// The frames of one launch (blockIdx.y): frame `frame[y]` of the block, rolled by (ox[y], oy[y]) pixels, 0 <= ox < W, 0 <= oy < H, into
// slot y of the scratch (dense, frame_bytes apart).
constexpr uint32_t ROLL_CHUNK = 8;
struct RollJobs {
    uint32_t frame[ROLL_CHUNK], ox[ROLL_CHUNK], oy[ROLL_CHUNK];
};

struct __attribute__((packed, aligned(1))) roll_vec_u { uint32_t x, y, z, w; };      // 16 bytes of any alignment

// k_roll_frames: rows whose byte length is a multiple of 16.  A lane owns 16 destination bytes of the scratch slot -- they lie in ONE row,
// and the slot is 16-byte aligned: one aligned 16-byte store -- and reads the same row of the source frame ox * pixel_bytes bytes further,
// wrapping at the row end: one 16-byte load of whatever alignment the shift leaves, or, for the one vector of a row that straddles the
// wrap point, sixteen byte loads.  new(x, y) = old((x + ox) mod W, (y + oy) mod H).  Plain loads and stores: the stages behind the roll read
// the block again at once (the reasoning of rbf_kernels_hold.h).  The source is never the destination.
__global__ __launch_bounds__(WG_THREADS) void k_roll_frames(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t row_bytes,
                                                            uint32_t height, uint32_t pixel_bytes, const RollJobs jobs,
                                                            uint8_t *__restrict__ scratch, uint64_t frame_bytes)
{
    const uint64_t at = ((uint64_t)blockIdx.x * WG_THREADS + threadIdx.x) * 16;
    if (at >= frame_bytes) return;
    const uint32_t y = (uint32_t)(at / row_bytes), xb = (uint32_t)(at - (uint64_t)y * row_bytes);
    uint32_t sy = y + jobs.oy[blockIdx.y], sxb = xb + jobs.ox[blockIdx.y] * pixel_bytes;
    sy = sy >= height ? sy - height : sy;
    sxb = sxb >= row_bytes ? sxb - row_bytes : sxb;
    const uint8_t *const src = frames + (uint64_t)jobs.frame[blockIdx.y] * frame_stride + (uint64_t)sy * row_bytes;
    uint4 v;
    if (sxb + 16 <= row_bytes) {
        const roll_vec_u u = *reinterpret_cast<const roll_vec_u *>(src + sxb);
        v = make_uint4(u.x, u.y, u.z, u.w);
    } else {
        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uint32_t s = sxb + k;
            s = s >= row_bytes ? s - row_bytes : s;
            d[k >> 2] |= (uint32_t)src[s] << (8 * (k & 3));
        }
        v = make_uint4(d[0], d[1], d[2], d[3]);
    }
    *reinterpret_cast<uint4 *>(scratch + (uint64_t)blockIdx.y * frame_bytes + at) = v;
}

// The byte-wise path: a thread owns ONE destination byte.  Rows of any byte length.
__global__ __launch_bounds__(WG_THREADS) void k_roll_frames_bytes(const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t row_bytes,
                                                                  uint32_t height, uint32_t pixel_bytes, const RollJobs jobs,
                                                                  uint8_t *__restrict__ scratch, uint64_t frame_bytes)
{
    const uint64_t at = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (at >= frame_bytes) return;
    const uint32_t y = (uint32_t)(at / row_bytes), xb = (uint32_t)(at - (uint64_t)y * row_bytes);
    uint32_t sy = y + jobs.oy[blockIdx.y], sxb = xb + jobs.ox[blockIdx.y] * pixel_bytes;
    sy = sy >= height ? sy - height : sy;
    sxb = sxb >= row_bytes ? sxb - row_bytes : sxb;
    scratch[(uint64_t)blockIdx.y * frame_bytes + at] = frames[(uint64_t)jobs.frame[blockIdx.y] * frame_stride + (uint64_t)sy * row_bytes + sxb];
}

}  // namespace rbf
