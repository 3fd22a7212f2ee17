// rbf_kernels_rice.h -- the opt-in sample codec (ImprovedVideoCompressor(sample_codec="rice")): every stored sample is predicted, the
// prediction error is mapped to an unsigned value u and written with a chunked Rice code.  The format is normative (the tests
// pin it):
//   s = (x - pred) mod 2^B read as a B-bit two's-complement value; u = 2s for s >= 0, -2s - 1 otherwise;
//   chunk c codes samples [1024c, 1024c + 1024) with ONE parameter k[c] in [0, B] (the k of fewest bits, the smallest on a tie);
//   k == B: the B bits of u; k < B, q = u >> k: q < 16 -> q one-bits, a zero-bit, the k low bits of u; else 16 one-bits, the B bits of u;
//   bit j of a chunk is bit (j & 31) of its word j >> 5, and every chunk starts on a word of its own -- a chunk's writer owns its words.
// Stream: <I N | <B B | 3 zero bytes | k[C] | <H words[C] | zero pad to 4 bytes | payload words.
//
// Encode, many streams in one launch sequence: a producer writes the u values of every stream into one dense buffer (keyframes: the
// left / above predictor; inter-frames: frame t-1 at the mask's pixels), k_rice_cost picks k and counts words per chunk (one wave per
// chunk), k_rice_scan turns the word counts into offsets (one 1024-thread workgroup), k_rice_headers and k_rice_write lay the streams
// out back to back.  Decode: k_rice_decode (one wave per chunk: the chunk's words staged in LDS, one lane walks them) writes s, then the
// keyframe rebuild (prefix sums down column 0 and along every row) or the inter-frame add at the mask's pixels.
#pragma once
#include "rbf_kernels.h"

namespace rbf {

constexpr int RICE_CHUNK = 1024;                       // samples per chunk
constexpr int RICE_PER_LANE = RICE_CHUNK / WAVE;       // 16
constexpr uint32_t RICE_ESC = 16;                      // unary length of an escaped value
constexpr int RICE_WMAX = RICE_CHUNK * 16 / 32;        // words of a chunk: never more than its raw 16-bit samples

struct RiceStream {            // one stream of an encode call (host-built; a sentinel entry follows the last)
    uint64_t u_off;            // its first u value in the dense buffer
    uint64_t hdr_word;         // header words of the streams in front of it
    uint32_t n;                // samples
    uint32_t chunk0;           // its first chunk among all chunks of the call
};

struct RiceChunk {             // one chunk of a decode call (host-built from a table checked against its stream's length)
    uint64_t word_off;         // its first payload word in the uploaded streams
    uint64_t out_off;          // its first sample in the output
    uint32_t words;            // 1 .. ceil(nsamp * bits / 32)
    uint16_t nsamp;            // 1 .. 1024
    uint8_t k, bits;
};

__device__ __forceinline__ uint32_t rice_map(uint32_t d, uint32_t bits)
{
    const uint32_t full = 1u << bits;
    d &= full - 1u;
    return d < (full >> 1) ? 2u * d : 2u * (full - d) - 1u;
}

__device__ __forceinline__ uint32_t rice_unmap(uint32_t u, uint32_t bits)
{
    return ((u >> 1) ^ (0u - (u & 1u))) & ((1u << bits) - 1u);
}

template <int B>
__device__ __forceinline__ uint32_t rice_code(uint32_t u, uint32_t k, uint32_t *len)
{
    if (k >= (uint32_t)B) { *len = B; return u; }
    const uint32_t q = u >> k;
    if (q < RICE_ESC) { *len = q + 1u + k; return ((1u << q) - 1u) | ((u & ((1u << k) - 1u)) << (q + 1u)); }
    *len = RICE_ESC + B;
    return 0xFFFFu | (u << RICE_ESC);
}

// the stream that owns chunk c: the last one whose first chunk is <= c (a stream without chunks shares its successor's chunk0)
__device__ __forceinline__ uint32_t rice_stream_of(const RiceStream *__restrict__ st, uint32_t nstreams, uint32_t c)
{
    uint32_t lo = 0, hi = nstreams;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (st[mid].chunk0 <= c) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t rice_chunk_samples(const RiceStream &st, uint32_t c)
{
    const uint64_t left = (uint64_t)st.n - (uint64_t)(c - st.chunk0) * RICE_CHUNK;
    return left < (uint64_t)RICE_CHUNK ? (uint32_t)left : (uint32_t)RICE_CHUNK;
}

// ---- producers -----------------------------------------------------------------------------------------------------------------
// Keyframes: u of every sample of nframes dense (H, W, C) frames; pred = the same channel of the pixel to the left, of the pixel above
// in column 0, 0 for the first pixel.  grid (ceil(W*C / 256), H, nframes).
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_rice_intra_u(
    const uint8_t *__restrict__ frames, uint64_t frame_stride, uint32_t width, uint32_t channels, uint32_t bits, uint16_t *__restrict__ u)
{
    const uint64_t row = (uint64_t)width * channels;
    const uint64_t col = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (col >= row) return;
    const uint32_t y = blockIdx.y, f = blockIdx.z;
    const SAMPLE *x = (const SAMPLE *)(frames + (uint64_t)f * frame_stride);
    const uint64_t i = (uint64_t)y * row + col;
    uint32_t pred = 0;
    if (col >= channels) pred = x[i - channels];
    else if (y > 0) pred = x[i - row];
    u[(uint64_t)f * row * gridDim.y + i] = (uint16_t)rice_map((uint32_t)x[i] - pred, bits);
}

// Inter-frames, every pair of a block at once (the k_gather_words indexing): pair f = blockIdx.y reads frame f+1 and frame f at the
// '1' pixels of mask f and writes the u values of its stream in raster order, channels interleaved.  Nothing is written past the
// stream's n samples (the caller checks the mask counts against them).
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_rice_inter_u(
    const uint8_t *__restrict__ frames, uint64_t frame_stride, uint64_t n, uint32_t channels, const uint64_t *__restrict__ masks,
    uint64_t mask_stride_words64, const uint64_t *__restrict__ seg_off, uint64_t nseg, const RiceStream *__restrict__ streams,
    uint32_t bits, uint16_t *__restrict__ u)
{
    const uint32_t f = blockIdx.y;
    const uint64_t nwords = (n + 63) >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (w >= nwords) return;
    const uint64_t *mask = masks + (uint64_t)f * mask_stride_words64;
    uint64_t p = flip_bytes64(mask[w]);
    if (!p) return;
    const uint64_t seg = w / SEG_ITERS;
    uint64_t o = seg_off[(uint64_t)f * nseg + seg];
    for (uint64_t j = seg * SEG_ITERS; j < w; ++j) o += __popcll(mask[j]);
    const RiceStream st = streams[f];
    const uint64_t npix = st.n / channels;
    const SAMPLE *prev = (const SAMPLE *)(frames + (uint64_t)f * frame_stride);
    const SAMPLE *cur = (const SAMPLE *)(frames + (uint64_t)(f + 1) * frame_stride);
    while (p) {
        const uint32_t b = __builtin_ctzll(p);
        p &= p - 1;
        const uint64_t i = w * 64 + b;
        if (i < n && o < npix) {
            for (uint32_t c = 0; c < channels; ++c)
                u[st.u_off + o * channels + c] = (uint16_t)rice_map((uint32_t)cur[i * channels + c] - (uint32_t)prev[i * channels + c], bits);
        }
        ++o;
    }
}

// ---- encode ----------------------------------------------------------------------------------------------------------------------
// One wave per chunk: the chunk's bits for every k in [0, B], the cheapest k (the smallest on a tie) and its word count:
// kw[c] = k | words << 8.
template <int B>
__global__ __launch_bounds__(WG_THREADS) void k_rice_cost(
    const uint16_t *__restrict__ u, const RiceStream *__restrict__ streams, uint32_t nstreams, uint32_t nchunks, uint32_t *__restrict__ kw)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    if (c >= nchunks) return;
    const RiceStream st = streams[rice_stream_of(streams, nstreams, c)];
    const uint32_t ns = rice_chunk_samples(st, c);
    const uint16_t *src = u + st.u_off + (uint64_t)(c - st.chunk0) * RICE_CHUNK;
    uint32_t cost[B];
#pragma unroll
    for (int k = 0; k < B; ++k) cost[k] = 0;
    for (int t = 0; t < RICE_PER_LANE; ++t) {
        const uint32_t i = (uint32_t)t * WAVE + lane;              // (the cost does not depend on the order: coalesced loads)
        if (i < ns) {
            const uint32_t v = src[i];
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const uint32_t q = v >> k;
                cost[k] += q < RICE_ESC ? q + 1u + (uint32_t)k : RICE_ESC + (uint32_t)B;
            }
        }
    }
    uint32_t best = ns * (uint32_t)B, bk = B;                      // k == B: the samples stored raw
#pragma unroll
    for (int k = B - 1; k >= 0; --k) {                             // downwards with <=: the smallest k wins a tie
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_lane63(cost[k]), 63);
        if (tot <= best) { best = tot; bk = (uint32_t)k; }
    }
    if (lane == 0) kw[c] = bk | (((best + 31u) >> 5) << 8);
}

// Payload word offsets: goff[c] = the words of the chunks in front of chunk c over the whole call (goff[nchunks] = all of them), and
// stream_words[s] = goff[streams[s].chunk0] for s in [0, nstreams] -- stream s starts at word streams[s].hdr_word + stream_words[s].
// One 1024-thread workgroup.
__global__ __launch_bounds__(1024) void k_rice_scan(
    const uint32_t *__restrict__ kw, uint32_t nchunks, uint64_t *__restrict__ goff, const RiceStream *__restrict__ streams, uint32_t nstreams,
    uint64_t *__restrict__ stream_words)
{
    __shared__ uint32_t smem[16];
    uint64_t carry = 0;
    for (uint32_t s0 = 0; s0 < nchunks; s0 += 1024) {
        const uint32_t s = s0 + threadIdx.x;
        const uint32_t v = s < nchunks ? kw[s] >> 8 : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_1024(v, smem, &tot);
        if (s < nchunks) goff[s] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) goff[nchunks] = carry;
    __threadfence();
    __syncthreads();
    for (uint32_t s = threadIdx.x; s <= nstreams; s += 1024) stream_words[s] = goff[streams[s].chunk0];
}

// Header and table of every stream, one thread per 32-bit word (streams[nstreams].hdr_word = the header words of the call).
__global__ __launch_bounds__(WG_THREADS) void k_rice_headers(
    const uint32_t *__restrict__ kw, const RiceStream *__restrict__ streams, uint32_t nstreams, const uint64_t *__restrict__ stream_words,
    uint32_t bits, uint32_t *__restrict__ out)
{
    const uint64_t total = streams[nstreams].hdr_word;
    for (uint64_t hw = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x; hw < total; hw += (uint64_t)gridDim.x * WG_THREADS) {
        uint32_t lo = 0, hi = nstreams;                            // every header has >= 2 words: hdr_word strictly increases
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (streams[mid].hdr_word <= hw) lo = mid; else hi = mid;
        }
        const RiceStream st = streams[lo];
        const uint32_t nch = streams[lo + 1].chunk0 - st.chunk0;
        const uint32_t w = (uint32_t)(hw - st.hdr_word);
        uint32_t word = 0;
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t b = 4u * w + j;
            uint32_t v = 0;
            if (b < 4) v = (st.n >> (8 * b)) & 0xFFu;
            else if (b == 4) v = bits;
            else if (b < 8) v = 0;
            else if (b < 8 + nch) v = kw[st.chunk0 + (b - 8)] & 0xFFu;
            else if (b < 8 + 3 * nch) {
                const uint32_t t = b - 8 - nch;
                const uint32_t words = kw[st.chunk0 + (t >> 1)] >> 8;
                v = (t & 1u) ? (words >> 8) & 0xFFu : words & 0xFFu;
            }
            word |= v << (8 * j);
        }
        out[st.hdr_word + stream_words[lo] + w] = word;
    }
}

// One wave per chunk: lane l codes samples 16l .. 16l+15 at its bit offset (a wave prefix sum) into the chunk's words in LDS, then the
// wave writes the words out.  Chunk c's payload starts at word hdr_word(s) + header words(s) + goff[c] = hdr_word(s+1) + goff[c].
template <int B>
__global__ __launch_bounds__(WG_THREADS) void k_rice_write(
    const uint16_t *__restrict__ u, const RiceStream *__restrict__ streams, uint32_t nstreams, uint32_t nchunks, const uint32_t *__restrict__ kw,
    const uint64_t *__restrict__ goff, uint32_t *__restrict__ out)
{
    constexpr uint32_t WMAX = RICE_CHUNK * B / 32;
    __shared__ uint32_t buf[WG_WAVES][WMAX];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * WG_WAVES + wv;
    uint32_t k = 0, words = 0, ns = 0;
    const uint16_t *src = u;
    uint64_t dst = 0;
    if (c < nchunks) {
        const uint32_t s = rice_stream_of(streams, nstreams, c);
        const RiceStream st = streams[s];
        ns = rice_chunk_samples(st, c);
        src = u + st.u_off + (uint64_t)(c - st.chunk0) * RICE_CHUNK;
        k = kw[c] & 0xFFu;
        words = min(kw[c] >> 8, WMAX);
        dst = streams[s + 1].hdr_word + goff[c];
    }
    for (uint32_t i = lane; i < words; i += WAVE) buf[wv][i] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int t = 0; t < RICE_PER_LANE; ++t) {
        const uint32_t i = lane * RICE_PER_LANE + (uint32_t)t;
        uint32_t len = 0;
        if (i < ns) (void)rice_code<B>(src[i], k, &len);
        mine += len;
    }
    uint32_t pos = wave_inclusive_scan(mine) - mine;
    for (int t = 0; t < RICE_PER_LANE; ++t) {
        const uint32_t i = lane * RICE_PER_LANE + (uint32_t)t;
        if (i < ns) {
            uint32_t len;
            const uint32_t code = rice_code<B>(src[i], k, &len);
            const uint32_t wi = pos >> 5, sh = pos & 31u;
            if (wi < words) atomicOr(&buf[wv][wi], code << sh);
            if (sh + len > 32u && wi + 1 < words) atomicOr(&buf[wv][wi + 1], code >> (32u - sh));
            pos += len;
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < words; i += WAVE) out[dst + i] = buf[wv][i];
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------
// One wave per chunk: the chunk's declared words are staged in LDS, lane 0 decodes the chunk from there (its reads never leave the
// declared words), the wave writes the s values out.  A code that runs past the words, words left over, or set bits behind the last code
// set *err.
__global__ __launch_bounds__(WG_THREADS) void k_rice_decode(
    const uint32_t *__restrict__ blob, const RiceChunk *__restrict__ chunks, uint32_t nchunks, uint16_t *__restrict__ s_out, uint32_t *__restrict__ err)
{
    __shared__ uint32_t wbuf[WG_WAVES][RICE_WMAX];
    __shared__ uint16_t sbuf[WG_WAVES][RICE_CHUNK];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * WG_WAVES + wv;
    const bool live = c < nchunks;
    RiceChunk ch{};
    if (live) ch = chunks[c];
    const uint32_t words = min(ch.words, (uint32_t)RICE_WMAX), ns = min((uint32_t)ch.nsamp, (uint32_t)RICE_CHUNK);
    for (uint32_t i = lane; i < words; i += WAVE) wbuf[wv][i] = blob[ch.word_off + i];
    __syncthreads();
    if (live && lane == 0) {
        const uint32_t B = ch.bits, k = ch.k, bmask = (1u << B) - 1u, kmask = (1u << k) - 1u;
        uint64_t buf = 0;
        uint32_t avail = 0, widx = 0;
        bool bad = words != ch.words || B > 16u;
        for (uint32_t i = 0; i < ns && !bad; ++i) {
            if (avail <= 32u && widx < words) { buf |= (uint64_t)wbuf[wv][widx++] << avail; avail += 32u; }
            uint32_t v, used;
            if (k >= B) { used = B; v = (uint32_t)buf & bmask; }
            else {
                const uint32_t q = (uint32_t)__builtin_ctzll(~buf | (1ull << RICE_ESC));
                if (q < RICE_ESC) { used = q + 1u + k; v = (q << k) | ((uint32_t)(buf >> (q + 1u)) & kmask); }
                else { used = RICE_ESC + B; v = (uint32_t)(buf >> RICE_ESC) & bmask; }
            }
            if (used > avail) { bad = true; break; }
            buf >>= used;
            avail -= used;
            sbuf[wv][i] = (uint16_t)rice_unmap(v, B);
        }
        if (bad || widx != words || avail >= 32u || buf != 0) err[0] = 1u;
    }
    __syncthreads();
    for (uint32_t i = lane; i < ns; i += WAVE) s_out[ch.out_off + i] = sbuf[wv][i];
}

// Keyframe rebuild, one wave per row: X(y, 0) = the sum of s down column 0 over rows 0..y (the wave sums them itself), then
// X(y, x) = X(y, 0) + s(y, 1) + ... + s(y, x) as a running inclusive scan over 64-pixel tiles; per channel, mod 2^B.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_rice_intra_rebuild(
    const uint16_t *__restrict__ s, uint32_t width, uint32_t height, uint32_t channels, uint32_t bits, SAMPLE *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t y = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    if (y >= height) return;
    const uint64_t row = (uint64_t)width * channels;
    const uint32_t bmask = (1u << bits) - 1u;
    uint32_t col0[4] = {0, 0, 0, 0}, carry[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        if (c < channels) {
            uint32_t acc = 0;
            for (uint32_t r = lane; r <= y; r += WAVE) acc += s[(uint64_t)r * row + c];
            col0[c] = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_lane63(acc), 63);
        }
    }
    const uint16_t *srow = s + (uint64_t)y * row;
    SAMPLE *orow = out + (uint64_t)y * row;
    for (uint32_t x0 = 0; x0 < width; x0 += WAVE) {
        const uint32_t x = x0 + lane;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            if (c < channels) {
                const uint32_t v = x == 0 ? col0[c] : (x < width ? (uint32_t)srow[(uint64_t)x * channels + c] : 0u);
                const uint32_t incl = wave_inclusive_scan(v) + carry[c];
                if (x < width) orow[(uint64_t)x * channels + c] = (SAMPLE)(incl & bmask);
                carry[c] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        }
    }
}

// Inter-frame apply: frame t (a copy of frame t-1) gets pred + s at the '1' pixels of its mask -- the add-variant of k_values<..., true>,
// one lane per 64-pixel mask word (seg_off: the mask's segment offsets).  A pixel past npix sets *err and is left alone.
template <typename SAMPLE>
__global__ __launch_bounds__(WG_THREADS) void k_rice_inter_add(
    SAMPLE *__restrict__ frame, uint64_t n, uint32_t channels, const uint64_t *__restrict__ mask, const uint64_t *__restrict__ seg_off,
    const uint16_t *__restrict__ s, uint64_t npix, uint32_t *__restrict__ err)
{
    const uint64_t nwords = (n + 63) >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (w >= nwords) return;
    uint64_t p = flip_bytes64(mask[w]);
    if (!p) return;
    const uint64_t seg = w / SEG_ITERS;
    uint64_t o = seg_off[seg];
    for (uint64_t j = seg * SEG_ITERS; j < w; ++j) o += __popcll(mask[j]);
    bool bad = false;
    while (p) {
        const uint32_t b = __builtin_ctzll(p);
        p &= p - 1;
        const uint64_t i = w * 64 + b;
        if (i < n && o < npix) {
            for (uint32_t c = 0; c < channels; ++c) {
                SAMPLE *px = frame + i * channels + c;
                *px = (SAMPLE)((uint32_t)*px + (uint32_t)s[o * channels + c]);
            }
        } else {
            bad = true;
        }
        ++o;
    }
    if (bad) err[0] = 2u;
}

}  // namespace rbf
