// median_net_cases.cpp -- csrc/rbf_median_net.h under a plain host compiler (tests/test_median_net_cpu.py builds it with g++: no HIP, no GPU).
// Replays the comparator list exactly as median25 (csrc/rbf_kernels_noise.h) does -- for comparator c the minimum goes to wire a[c], the
// maximum to wire b[c], the output is wire 12 -- over 0/1 inputs, bit-sliced: wire w is one 64-bit word, bit i of it is input i of the batch,
// min is AND and max is OR.  Every 25-bit input with exactly 12 ones must give 0 and every input with exactly 13 ones must give 1.
// `median_net_cases drop <c>` runs the same proof with comparator c left out (the test's check that the proof can fail).
// Prints the comparator count, the min/max operations that can reach wire 12, the inputs checked per layer and `ok`, or the first failure.
#include "../../new_bloom_filter_repo_amd/csrc/rbf_median_net.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static constexpr rbf::MedianNet NET = rbf::make_median_net();
static_assert(NET.n > 0 && NET.n <= 192, "the comparator list fits MedianNet's arrays");

static int g_drop = -1;             // `median_net_cases drop <c>`: comparator c is left out -- the proof has to notice (or c is redundant)

static uint64_t run(uint64_t (&w)[25])
{
    for (int c = 0; c < NET.n; ++c) {
        if (c == g_drop) continue;
        const uint64_t lo = w[NET.a[c]] & w[NET.b[c]], hi = w[NET.a[c]] | w[NET.b[c]];
        w[NET.a[c]] = lo;
        w[NET.b[c]] = hi;
    }
    return w[12];
}

// every 25-bit word of `ones` set bits (Gosper's walk), 64 to a batch; returns the number checked, or -1 after printing the failure
static long long layer(int ones, uint64_t want_bit)
{
    long long checked = 0;
    uint32_t x = (1u << ones) - 1, batch[64];
    const uint32_t end = 1u << 25;
    while (x < end) {
        int cnt = 0;
        while (cnt < 64 && x < end) {
            batch[cnt++] = x;
            const uint32_t c = x & -x, r = x + c;
            x = (((r ^ x) >> 2) / c) | r;
        }
        uint64_t w[25] = {};
        for (int i = 0; i < cnt; ++i)
            for (int b = 0; b < 25; ++b) w[b] |= (uint64_t)((batch[i] >> b) & 1u) << i;
        const uint64_t valid = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
        const uint64_t bad = (run(w) ^ (want_bit ? ~0ull : 0ull)) & valid;
        if (bad) {
            const int i = __builtin_ctzll(bad);
            printf("FAIL input=0x%07x ones=%d median=%d want=%d\n", batch[i], ones, (int)!want_bit, (int)want_bit);
            return -1;
        }
        checked += cnt;
    }
    return checked;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "drop")) g_drop = atoi(argv[2]);
    else if (argc != 1) { fprintf(stderr, "usage: median_net_cases [drop <comparator>]\n"); return 2; }
    for (int c = 0; c < NET.n; ++c)
        if (NET.a[c] >= NET.b[c] || NET.b[c] >= 25) { printf("FAIL comparator %d joins wires %d and %d\n", c, NET.a[c], NET.b[c]); return 1; }
    // the operations whose result can reach wire 12: what the compiler keeps of median25 after dead-code elimination
    bool live[25] = {};
    live[12] = true;
    int live_ops = 0;
    for (int c = NET.n - 1; c >= 0; --c) {
        const bool la = live[NET.a[c]], lb = live[NET.b[c]];
        live_ops += la + lb;
        if (la || lb) live[NET.a[c]] = live[NET.b[c]] = true;
    }
    printf("comparators %d\noperations %d live %d\n", NET.n, 2 * NET.n, live_ops);
    const long long n12 = layer(12, 0);
    if (n12 < 0) return 1;
    const long long n13 = layer(13, 1);
    if (n13 < 0) return 1;
    printf("ones12 %lld\nones13 %lld\n", n12, n13);
    if (n12 != 5200300 || n13 != 5200300) { printf("FAIL the walk visited %lld and %lld inputs, not 5200300 each\n", n12, n13); return 1; }
    printf("ok\n");
    return 0;
}
