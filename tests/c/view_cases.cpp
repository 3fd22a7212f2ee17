// view_cases.cpp -- the arithmetic of a frame view (csrc/rbf_view.h, the header the kernels include) under a plain host compiler: no HIP,
// no GPU.  tests/test_view_cpu.py builds it (g++ -std=c++17; it may be built with -fsanitize=address,undefined) and runs
//   view_cases check                                   the rounding pins, the block lengths, the lane tiles and the launch plan's
//                                                      coverage, swept; prints "ok <checks>" or the first failure
//   view_cases view FILE B W H C x0 y0 w h s           the host twin's view of the dense frame in FILE (B = sample bytes), as
//                                                      whitespace-separated decimal samples in output order
//   view_cases plan W PB x0 w h s aligned              the plan: out_w out_h tile tiles_x wide_cols wide_rows
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../new_bloom_filter_repo_amd/csrc/rbf_view.h"

using namespace rbf;

static long checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++checks;                                                        \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int check()
{
    // the rounding, both directions
    for (uint32_t q = 0; q < 65535; q += 257) {
        CHECK(view_round(4 * q + 2, 4) == q + 1 && view_round(4 * q + 1, 4) == q);
        CHECK(view_round_full(4 * q + 2, 1) == q + 1 && view_round_full(4 * q + 1, 1) == q);
        CHECK(view_round(3 * q + 1, 3) == q && view_round(3 * q + 2, 3) == q + 1);
        CHECK(view_round(q, 1) == q && view_round_full(q, 0) == q);
    }
    CHECK(view_round(64u * 65535u, 64) == 65535 && view_round_full(64u * 65535u, 3) == 65535);      // a 16-bit sum would have wrapped
    // a full block: the shift is the division
    for (uint32_t s : {1u, 2u, 4u, 8u})
        for (uint32_t sum = 0; sum <= s * s * 65535u; sum += 997) CHECK(view_round(sum, s * s) == view_round_full(sum, view_log2(s)));
    // every count of a ragged block against the rule in 64 bits
    for (uint32_t cnt = 1; cnt <= 64; ++cnt)
        for (uint32_t sum = 0; sum <= cnt * 65535u; sum += 1009 + cnt)
            CHECK(view_round(sum, cnt) == (uint32_t)((2ull * sum + cnt) / (2ull * cnt)));
    CHECK(view_scale_ok(1) && view_scale_ok(2) && view_scale_ok(4) && view_scale_ok(8));
    for (uint32_t s : {0u, 3u, 5u, 6u, 7u, 9u, 16u, 0xFFFFFFFFu}) CHECK(!view_scale_ok(s));
    // block lengths tile a side exactly
    for (uint32_t s : {1u, 2u, 4u, 8u})
        for (uint32_t len = 1; len <= 70; ++len) {
            const uint32_t out = view_out_dim(len, s);
            uint32_t covered = 0;
            for (uint32_t X = 0; X < out; ++X) {
                const uint32_t b = view_block_len(len, s, X);
                CHECK(b >= 1 && b <= s && (X + 1 < out ? b == s : true));
                covered += b;
            }
            CHECK(covered == len);
        }
    CHECK(view_out_dim(0xFFFFFFFFu, 8) == 0x20000000u && view_out_dim(0xFFFFFFFFu, 1) == 0xFFFFFFFFu);
    // the lane tiles: whole 16-byte vectors, at most four per row
    for (uint32_t s : {1u, 2u, 4u, 8u})
        for (uint32_t pb : {1u, 2u, 3u, 4u, 6u, 8u}) {
            const uint32_t t = view_tile_pixels(s, pb), v = view_tile_vectors(s, pb);
            CHECK(t >= 1 && t <= 16 && (t * s * pb) % 16 == 0 && v * 16 == t * s * pb && v >= 1 && v <= 4);
            for (uint32_t smaller = 1; smaller < t; ++smaller) CHECK((smaller * s * pb) % 16 != 0);
        }
    // the plan: the wide kernel never leaves the region, takes full blocks only, and needs every alignment it is given
    for (uint32_t s : {1u, 2u, 4u, 8u})
        for (uint32_t pb : {1u, 2u, 3u, 4u, 6u, 8u})
            for (uint32_t W : {1u, 15u, 16u, 37u, 64u, 67u, 96u, 1030u})
                for (uint32_t x0 : {0u, 1u, 8u, 16u})
                    for (uint32_t w : {1u, 7u, 16u, 33u, 64u, 80u}) {
                        if (x0 + w > W) continue;
                        for (uint32_t h : {1u, 7u, 8u, 33u}) {
                            const ViewPlan p = view_plan(W, pb, x0, w, h, s, true), g = view_plan(W, pb, x0, w, h, s, false);
                            CHECK(p.out_w == view_out_dim(w, s) && p.out_h == view_out_dim(h, s));
                            CHECK(g.tiles_x == 0 && g.wide_cols == 0 && g.wide_rows == 0);
                            CHECK(p.wide_cols == p.tiles_x * p.tile && (uint64_t)p.wide_cols * s <= w && (uint64_t)p.wide_rows * s <= h);
                            CHECK((p.tiles_x == 0) == (p.wide_rows == 0));
                            if (p.tiles_x) CHECK((W * pb) % 16 == 0 && (x0 * pb) % 16 == 0 && p.wide_rows == h / s && p.tiles_x == (w / s) / p.tile);
                        }
                    }
    printf("ok %ld\n", checks);
    return 0;
}

template <typename S>
static int view_of(const char *path, uint32_t W, uint32_t H, uint32_t C, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t s)
{
    std::vector<S> src((size_t)W * H * C);
    FILE *f = fopen(path, "rb");
    if (!f || fread(src.data(), sizeof(S), src.size(), f) != src.size()) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    fclose(f);
    std::vector<S> dst((size_t)view_out_dim(w, s) * view_out_dim(h, s) * C);
    view_frame_host<S>(src.data(), W, C, x0, y0, w, h, s, dst.data());
    for (S v : dst) printf("%u\n", (unsigned)v);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 12 && !strcmp(argv[1], "view")) {
        uint32_t a[9];
        for (int i = 0; i < 9; ++i) a[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
        const uint32_t B = a[0], W = a[1], H = a[2], C = a[3], x0 = a[4], y0 = a[5], w = a[6], h = a[7], s = a[8];
        if (!view_scale_ok(s) || !w || !h || x0 + w > W || y0 + h > H || C < 1 || C > 4 || (B != 1 && B != 2)) { fprintf(stderr, "bad view\n"); return 2; }
        return B == 1 ? view_of<uint8_t>(argv[2], W, H, C, x0, y0, w, h, s) : view_of<uint16_t>(argv[2], W, H, C, x0, y0, w, h, s);
    }
    if (argc == 9 && !strcmp(argv[1], "plan")) {
        uint32_t a[7];
        for (int i = 0; i < 7; ++i) a[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
        const ViewPlan p = view_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6] != 0);
        printf("%u %u %u %u %u %u\n", p.out_w, p.out_h, p.tile, p.tiles_x, p.wide_cols, p.wide_rows);
        return 0;
    }
    fprintf(stderr, "usage: view_cases check | view FILE B W H C x0 y0 w h s | plan W PB x0 w h s aligned\n");
    return 2;
}
