// rbf_digest.h -- the arithmetic of the frame digest FD1 (include/rbf.h has the normative text), shared by the kernel
// (rbf_kernels_digest.h), the host twin below and the CPU check (tests/c/digest_cases.cpp).  No HIP header: any C++17 host compiler takes
// it; under hipcc the small functions are __host__ __device__, so the device runs the very lines the CPU check pins.
//
//   round(acc, x) = rotl64(acc + x*P2, 31) * P1          merge(a, b) = (a ^ round(0, b)) * P1 + P4
//   aval(h): h ^= h>>33; h *= P2; h ^= h>>29; h *= P3; h ^= h>>32
//   block(w[0..511], seed): one 4096-byte block, zero-padded, as 512 little-endian u64
//     lane l in 0..63: acc[l] = seed + P5 + l*P1;  row r in 0..3, half h in 0..1: acc[l] = round(acc[l], w[128 r + 2 l + h])
//     d in 1,2,4,8,16,32: every l that is a multiple of 2d: acc[l] = merge(acc[l], acc[l+d]);  the block's hash is aval(acc[0])
//   FD1(b, L = len(b)): while len(b) > 4096: b = the hashes of b's blocks (block j with seed j) as little-endian u64;
//                       FD1 = block(b, seed L)
// P1..P5 are the XXH64 primes (rbf_device.h has the same values for the key hashes).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define RBF_FD1_HD __host__ __device__ inline
#else
#define RBF_FD1_HD inline
#endif

namespace rbf {

constexpr uint64_t FD1_P1 = 0x9E3779B185EBCA87ULL, FD1_P2 = 0xC2B2AE3D27D4EB4FULL, FD1_P3 = 0x165667B19E3779F9ULL,
                   FD1_P4 = 0x85EBCA77C2B2AE63ULL, FD1_P5 = 0x27D4EB2F165667C5ULL;
constexpr uint32_t FD1_BLOCK_BYTES = 4096, FD1_LANES = 64, FD1_ROWS = 4, FD1_ROW_BYTES = 1024, FD1_BLOCK_WORDS = 512;

RBF_FD1_HD uint64_t fd1_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
RBF_FD1_HD uint64_t fd1_round(uint64_t acc, uint64_t x) { return fd1_rotl(acc + x * FD1_P2, 31) * FD1_P1; }
RBF_FD1_HD uint64_t fd1_merge(uint64_t a, uint64_t b) { return (a ^ fd1_round(0, b)) * FD1_P1 + FD1_P4; }
RBF_FD1_HD uint64_t fd1_aval(uint64_t h)
{
    h ^= h >> 33; h *= FD1_P2;
    h ^= h >> 29; h *= FD1_P3;
    h ^= h >> 32;
    return h;
}
RBF_FD1_HD uint64_t fd1_lane_seed(uint64_t seed, uint32_t lane) { return seed + FD1_P5 + (uint64_t)lane * FD1_P1; }

// ---- the levels.  Level 0 is the frame's bytes; while a level is longer than one block, the next one is its block hashes (8 bytes each).
// fd1_levels(L): how many levels are hashed block by block with the block index as seed, in front of the final block (seed L).
RBF_FD1_HD uint64_t fd1_blocks(uint64_t bytes) { return (bytes + FD1_BLOCK_BYTES - 1) / FD1_BLOCK_BYTES; }
RBF_FD1_HD uint64_t fd1_level_bytes(uint64_t L, uint32_t level)
{
    uint64_t b = L;
    for (uint32_t k = 0; k < level; ++k) b = 8 * fd1_blocks(b);
    return b;
}
RBF_FD1_HD uint32_t fd1_levels(uint64_t L)
{
    uint32_t k = 0;
    for (uint64_t b = L; b > FD1_BLOCK_BYTES; b = 8 * fd1_blocks(b)) ++k;
    return k;
}
// u64 words of scratch a frame of L bytes needs for the block hashes of all its levels
RBF_FD1_HD uint64_t fd1_scratch_words(uint64_t L)
{
    uint64_t words = 0;
    for (uint64_t b = L; b > FD1_BLOCK_BYTES; b = 8 * fd1_blocks(b)) words += fd1_blocks(b);
    return words;
}

// ---- the host twin (a little-endian host, as everything at this ABI)
// One block: `bytes` (<= 4096) bytes at p, zero-padded.
inline uint64_t fd1_block_host(const uint8_t *p, size_t bytes, uint64_t seed)
{
    uint64_t w[FD1_BLOCK_WORDS];
    if (bytes < FD1_BLOCK_BYTES) memset(w, 0, sizeof w);
    if (bytes) memcpy(w, p, bytes);
    uint64_t acc[FD1_LANES];
    for (uint32_t l = 0; l < FD1_LANES; ++l) acc[l] = fd1_lane_seed(seed, l);
    for (uint32_t r = 0; r < FD1_ROWS; ++r)
        for (uint32_t h = 0; h < 2; ++h)
            for (uint32_t l = 0; l < FD1_LANES; ++l) acc[l] = fd1_round(acc[l], w[128 * r + 2 * l + h]);
    for (uint32_t d = 1; d < FD1_LANES; d *= 2)
        for (uint32_t l = 0; l < FD1_LANES; l += 2 * d) acc[l] = fd1_merge(acc[l], acc[l + d]);
    return fd1_aval(acc[0]);
}

inline uint64_t fd1_host(const void *data, size_t nbytes)
{
    const uint8_t *p = (const uint8_t *)data;
    size_t len = nbytes;
    std::vector<uint64_t> cur, nxt;
    while (len > FD1_BLOCK_BYTES) {
        const size_t nb = (size_t)fd1_blocks(len);
        nxt.resize(nb);
        for (size_t j = 0; j < nb; ++j) {
            const size_t off = j * FD1_BLOCK_BYTES;
            nxt[j] = fd1_block_host(p + off, len - off < FD1_BLOCK_BYTES ? len - off : FD1_BLOCK_BYTES, j);
        }
        cur.swap(nxt);
        p = (const uint8_t *)cur.data();
        len = nb * 8;
    }
    return fd1_block_host(p, len, nbytes);
}

}  // namespace rbf
