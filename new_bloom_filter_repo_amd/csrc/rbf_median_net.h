// The comparator list of the 5x5 median (k_noise_moments, rbf_kernels_noise.h).  Host-only: no HIP header, so that
// tests/c/median_net_cases.cpp replays the same list with a plain host compiler and proves it over every input.
#pragma once
#include <cstdint>

namespace rbf {

// Batcher's odd-even merge sort on 32 wires, restricted to the 25 wires that carry data (the other
// seven would hold +inf and never move).  Only wire 12 -- the median -- is consumed, so the compiler
// drops every min/max that cannot reach it (202 packed min/max remain out of 280).
struct MedianNet {
    int n;
    unsigned char a[192], b[192];
};
constexpr MedianNet make_median_net()
{
    MedianNet net{};
    for (int p = 1; p < 32; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j + k < 32; j += 2 * k)
                for (int i = 0; i < (k < 32 - j - k ? k : 32 - j - k); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < 25) {
                        net.a[net.n] = (unsigned char)(i + j);
                        net.b[net.n] = (unsigned char)(i + j + k);
                        ++net.n;
                    }
    return net;
}

}  // namespace rbf
