// rbf_rice_host.h -- host side of the sample codec (rbf_kernels_rice.h): prediction residuals in a chunked Rice code.  The stream
// tables of a call, the checks of an uploaded stream, and the launch sequences the four rbf_rice_* entry points of rbf_api.hip share.
#pragma once
#include "rbf_host.h"
#include "rbf_kernels_rice.h"

static inline uint64_t rice_nchunks(uint64_t n) { return (n + RICE_CHUNK - 1) / RICE_CHUNK; }
static inline uint64_t rice_header_words(uint64_t n) { return (8 + 3 * rice_nchunks(n) + 3) / 4; }

// the longest stream of n samples of `bits` bits: every chunk stored raw
static uint64_t rice_max_bytes(uint64_t n, uint32_t bits)
{
    const uint64_t full = n / RICE_CHUNK, tail = n % RICE_CHUNK;
    return 4 * (rice_header_words(n) + full * (RICE_CHUNK * bits / 32) + (tail * bits + 31) / 32);
}

// a dense frame of `channels` samples per pixel
static int rice_check_frame(uint32_t width, uint32_t height, uint32_t channels, uint32_t sample_bytes)
{
    LayoutRules rules;
    rules.samples = channels; rules.channels = true; rules.max_height = 65535;
    const uint32_t pixel = channels * sample_bytes;
    if (int r = check_layout(FrameLayout{width, height, (uint64_t)width * pixel, pixel, sample_bytes, 0}, 1, rules)) return r;
    if ((uint64_t)width * height * channels > 0xFFFFFFFFull) return fail(RBF_ERANGE, "a stream holds at most 2^32-1 samples");
    return RBF_OK;
}

static int rice_check_dense(uint64_t frame_stride_bytes, uint64_t samples, uint32_t sample_bytes)
{
    if (frame_stride_bytes < samples * sample_bytes || frame_stride_bytes % sample_bytes)
        return fail(RBF_EINVAL, "frame stride %llu cannot hold a dense frame of %llu bytes", (unsigned long long)frame_stride_bytes,
                    (unsigned long long)(samples * sample_bytes));
    return RBF_OK;
}

struct RicePlan { std::vector<RiceStream> st; uint32_t nchunks = 0; uint64_t samples = 0; };

// The stream table of an encode call (nstreams streams of n[s] samples, a sentinel behind them) and the capacity check.
static int rice_plan(const uint64_t *n, uint32_t nstreams, uint32_t bits, uint64_t capacity_bytes, RicePlan *p)
{
    try { p->st.resize((size_t)nstreams + 1); } catch (...) { return fail(RBF_ENOMEM, "out of host memory"); }
    uint64_t hdr = 0, chunks = 0, samples = 0, need = 0;
    for (uint32_t s = 0; s < nstreams; ++s) {
        if (n[s] > 0xFFFFFFFFull) return fail(RBF_ERANGE, "stream %u: %llu samples, a stream holds at most 2^32-1", s, (unsigned long long)n[s]);
        p->st[s] = RiceStream{samples, hdr, (uint32_t)n[s], (uint32_t)chunks};
        hdr += rice_header_words(n[s]);
        chunks += rice_nchunks(n[s]);
        samples += n[s];
        need += rice_max_bytes(n[s], bits);
    }
    if (chunks > 0xFFFFFFFFull) return fail(RBF_ERANGE, "too many chunks in one call");
    p->st[nstreams] = RiceStream{samples, hdr, 0, (uint32_t)chunks};
    p->nchunks = (uint32_t)chunks;
    p->samples = samples;
    if (capacity_bytes < need)
        return fail(RBF_EINVAL, "output capacity %llu bytes < %llu, the longest these streams can be", (unsigned long long)capacity_bytes,
                    (unsigned long long)need);
    return RBF_OK;
}

static int rice_stage(rbf_ctx *ctx, const RicePlan &p)
{
    if (int r = ctx->rice_u.reserve((size_t)std::max<uint64_t>(p.samples, 1) * 2)) return r;
    if (int r = ctx->rice_kw.reserve(((size_t)p.nchunks + 1) * 4)) return r;
    if (int r = ctx->rice_off.reserve(((size_t)p.nchunks + 1 + p.st.size()) * 8)) return r;
    if (int r = ctx->rice_tab.reserve(p.st.size() * sizeof(RiceStream))) return r;
    HIP_TRY(hipMemcpyAsync(ctx->rice_tab.p, p.st.data(), p.st.size() * sizeof(RiceStream), hipMemcpyHostToDevice, ctx->stream));
    return RBF_OK;
}

// cost -> scan -> headers + payload words, then the stream sizes to the host (blocks)
template <int B>
static int rice_encode_streams(rbf_ctx *ctx, const RicePlan &p, void *out_dev, uint64_t *stream_bytes)
{
    const uint32_t nstreams = (uint32_t)p.st.size() - 1;
    const RiceStream *st = (const RiceStream *)ctx->rice_tab.p;
    uint64_t *goff = ctx->rice_off.p, *swords = ctx->rice_off.p + p.nchunks + 1;
    const uint32_t bx = (p.nchunks + WG_WAVES - 1) / WG_WAVES;
    if (p.nchunks)
        hipLaunchKernelGGL(k_rice_cost<B>, dim3(bx), dim3(WG_THREADS), 0, ctx->stream, ctx->rice_u.p, st, nstreams, p.nchunks,
                           ctx->rice_kw.p);
    hipLaunchKernelGGL(k_rice_scan, dim3(1), dim3(1024), 0, ctx->stream, ctx->rice_kw.p, p.nchunks, goff, st, nstreams, swords);
    const uint64_t hw = p.st[nstreams].hdr_word;
    hipLaunchKernelGGL(k_rice_headers, dim3((uint32_t)std::min<uint64_t>((hw + WG_THREADS - 1) / WG_THREADS, 4096)), dim3(WG_THREADS), 0, ctx->stream,
                       ctx->rice_kw.p, st, nstreams, swords, (uint32_t)B, (uint32_t *)out_dev);
    if (p.nchunks)
        hipLaunchKernelGGL(k_rice_write<B>, dim3(bx), dim3(WG_THREADS), 0, ctx->stream, ctx->rice_u.p, st, nstreams, p.nchunks,
                           ctx->rice_kw.p, goff, (uint32_t *)out_dev);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> sw;
    try { sw.resize(p.st.size()); } catch (...) { (void)hipStreamSynchronize(ctx->stream); return fail(RBF_ENOMEM, "out of host memory"); }
    HIP_TRY(hipMemcpyAsync(sw.data(), swords, sw.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t s = 0; s < nstreams; ++s)
        stream_bytes[s] = 4 * ((p.st[s + 1].hdr_word + sw[s + 1]) - (p.st[s].hdr_word + sw[s]));
    return RBF_OK;
}

static inline uint32_t rice_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// Checks stream `idx` (len bytes at p) before anything is launched -- its bit width, the reserved and padding bytes, every k <= B, every
// word count in 1 .. ceil(chunk samples * B / 32), the table against the stream's length -- and appends its chunks.  word0: the stream's
// first word among the uploaded streams; out0: its first sample in the output.
static int rice_parse(const uint8_t *p, uint64_t len, uint32_t idx, uint32_t bits, uint64_t word0, uint64_t out0,
                      std::vector<RiceChunk> *chunks, uint64_t *n_out)
{
    if (len < 8 || len % 4) return fail(RBF_EINVAL, "sample stream %u: %llu bytes (a stream is >= 8 bytes, a multiple of 4)", idx, (unsigned long long)len);
    const uint64_t n = rice_le32(p);
    if (p[4] != bits) return fail(RBF_EINVAL, "sample stream %u codes %u-bit samples, the frame has %u", idx, (unsigned)p[4], bits);
    if (p[5] | p[6] | p[7]) return fail(RBF_EINVAL, "sample stream %u: reserved header bytes are not zero", idx);
    const uint64_t nch = rice_nchunks(n), hdr = 4 * rice_header_words(n);
    if (hdr > len)
        return fail(RBF_EINVAL, "sample stream %u: the table of %llu chunks runs past its %llu bytes", idx, (unsigned long long)nch, (unsigned long long)len);
    for (uint64_t b = 8 + 3 * nch; b < hdr; ++b)
        if (p[b]) return fail(RBF_EINVAL, "sample stream %u: padding bytes are not zero", idx);
    uint64_t w = 0;
    try {
        for (uint64_t c = 0; c < nch; ++c) {
            const uint32_t k = p[8 + c], words = (uint32_t)p[8 + nch + 2 * c] | (uint32_t)p[9 + nch + 2 * c] << 8;
            const uint64_t nc = std::min<uint64_t>(RICE_CHUNK, n - c * RICE_CHUNK);
            if (k > bits) return fail(RBF_EINVAL, "sample stream %u, chunk %llu: k = %u > %u", idx, (unsigned long long)c, k, bits);
            if (words == 0 || words > (nc * bits + 31) / 32)
                return fail(RBF_EINVAL, "sample stream %u, chunk %llu: %u words, a chunk of %llu samples has 1..%llu", idx, (unsigned long long)c, words,
                            (unsigned long long)nc, (unsigned long long)((nc * bits + 31) / 32));
            chunks->push_back(RiceChunk{word0 + hdr / 4 + w, out0 + c * RICE_CHUNK, words, (uint16_t)nc, (uint8_t)k, (uint8_t)bits});
            w += words;
        }
    } catch (...) {
        return fail(RBF_ENOMEM, "out of host memory");
    }
    if (hdr + 4 * w != len)
        return fail(RBF_EINVAL, "sample stream %u: its table declares %llu bytes, the stream has %llu", idx, (unsigned long long)(hdr + 4 * w),
                    (unsigned long long)len);
    *n_out = n;
    return RBF_OK;
}

// Uploads the streams and their chunk table, decodes every chunk into ctx->rice_u and waits: RBF_EINVAL when a chunk's codes do not end
// inside its declared words.
static int rice_decode(rbf_ctx *ctx, const void *streams, uint64_t nbytes, const std::vector<RiceChunk> &ch, uint64_t samples)
{
    if (int r = ctx->rice_blob.reserve((size_t)std::max<uint64_t>(nbytes, 8))) return r;
    if (int r = ctx->rice_tab.reserve(std::max<size_t>(ch.size(), 1) * sizeof(RiceChunk))) return r;
    if (int r = ctx->rice_u.reserve((size_t)std::max<uint64_t>(samples, 1) * 2)) return r;
    if (int r = ctx->rice_err.reserve(8)) return r;
    HIP_TRY(hipMemcpyAsync(ctx->rice_blob.p, streams, nbytes, hipMemcpyHostToDevice, ctx->stream));
    if (!ch.empty()) HIP_TRY(hipMemcpyAsync(ctx->rice_tab.p, ch.data(), ch.size() * sizeof(RiceChunk), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->rice_err.p, 0, 8, ctx->stream));
    if (!ch.empty())
        hipLaunchKernelGGL(k_rice_decode, dim3((uint32_t)((ch.size() + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, ctx->stream,
                           (const uint32_t *)ctx->rice_blob.p, (const RiceChunk *)ctx->rice_tab.p, (uint32_t)ch.size(), ctx->rice_u.p,
                           ctx->rice_err.p);
    HIP_TRY(hipGetLastError());
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, ctx->rice_err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (err) return fail(RBF_EINVAL, "corrupt sample stream: a chunk's codes do not end inside its declared words");
    return RBF_OK;
}
