// block_plan_cases.cpp -- the dense-block stages' host arithmetic (csrc/rbf_block_plan.h, the header rbf_api.hip's entry points stand on)
// under a plain host compiler: no HIP, no GPU.  tests/test_block_plan_cpu.py builds it (g++ -std=c++17; it may be built with
// -fsanitize=address,undefined) and runs
//   block_plan_cases check                                   the lane split's identities over every n of 1..4200, both sides of the grid
//                                                            limit, the alignment predicate; prints "ok <checks>" or the first failure
//   block_plan_cases splits UNIT PER_WG TAIL_PER_WG ROWS_PER_WG VEC NMAX
//                                                            a line per n of 1..NMAX: units first_px bx_vec bx_px rows tail_row_base
//   block_plan_cases block W,H,C,SB,STRIDE,NFRAMES,BASE,WAIVE ...
//                                                            a line per argument: the code of check_block_shape, then of check_block_at
//                                                            ("-" if the shape was refused), then 1 if a refusal left a text
//   block_plan_cases runs NFRAMES MARKS ...                  a line per MARKS (NFRAMES digits 0/1, or "null"): first:len of every run
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../new_bloom_filter_repo_amd/csrc/rbf_block_plan.h"

static char g_text[256] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof g_text, fmt, ap);
    va_end(ap);
    return code;
}

static long checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++checks;                                                        \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int check_split(uint64_t n, uint32_t unit, uint32_t per_wg, uint32_t tail_per_wg, uint32_t rows_per_wg, bool vec)
{
    const LaneSplit s = split_lanes(n, unit, per_wg, tail_per_wg, rows_per_wg, vec);
    const uint64_t tail = n - s.first_px;
    CHECK(s.first_px <= n && s.first_px % unit == 0 && s.first_px == s.units * unit);
    CHECK(vec ? tail < unit : (s.units == 0 && tail == n));
    CHECK(s.bx_vec * per_wg >= s.units && (s.bx_vec == 0 ? s.units == 0 : (s.bx_vec - 1) * per_wg < s.units));
    CHECK(s.bx_px * tail_per_wg >= tail && (s.bx_px == 0 ? tail == 0 : (s.bx_px - 1) * tail_per_wg < tail));
    CHECK(s.rows == (s.bx_vec + s.bx_px) * rows_per_wg && s.tail_row_base == s.bx_vec * rows_per_wg);
    CHECK(s.bx_vec + s.bx_px >= 1 && s.fits());
    return 0;
}

static int check()
{
    for (uint64_t n = 1; n <= 4200; ++n)
        for (int vec = 0; vec < 2; ++vec) {
            for (uint32_t unit : {8u, 16u})                           // the lane kernels: 256 lanes and four rows to a workgroup
                if (check_split(n, unit, 256, 256, 4, vec)) return 1;
            for (uint32_t tile : {128u, 256u})                        // the sweep: a tile to a workgroup, a row per wave of the tile
                if (check_split(n, tile, 1, tile, tile / 64, vec)) return 1;
        }
    // the grid limit, both sides: 0x7FFFFFFF workgroups fit a grid's x, one more does not -- in the lane kernel, and in the per-pixel kernel
    const uint64_t top = 0x7FFFFFFFull;
    CHECK(split_lanes(top * 256 * 16, 16, 256, 256, 4, true).fits() && split_lanes(top * 256 * 16, 16, 256, 256, 4, true).bx_vec == top);
    CHECK(!split_lanes(top * 256 * 16 + 16, 16, 256, 256, 4, true).fits());
    CHECK(split_lanes(top * 256 * 16 + 15, 16, 256, 256, 4, true).fits() && split_lanes(top * 256 * 16 + 15, 16, 256, 256, 4, true).bx_px == 1);
    CHECK(split_lanes(top * 256, 16, 256, 256, 4, false).fits() && split_lanes(top * 256, 16, 256, 256, 4, false).bx_px == top);
    CHECK(!split_lanes(top * 256 + 1, 16, 256, 256, 4, false).fits());
    CHECK(split_lanes(top * 128, 128, 1, 128, 2, true).fits() && !split_lanes((top + 1) * 128, 128, 1, 128, 2, true).fits());
    CHECK(split_lanes((top + 1) * 128, 128, 1, 128, 2, true).rows == (top + 1) * 2);                  // (64-bit throughout)
    // the alignment predicate
    const uintptr_t a16 = 0x7f0000001000, a8 = 0x7f0000001008, a1 = 0x7f0000001001;
    const uint64_t s32 = 32, s24 = 24, far = (1ull << 32) + 16, far8 = (1ull << 32) + 8;
    CHECK(lanes_aligned(16, a16, s32) && !lanes_aligned(16, a8, s32) && lanes_aligned(8, a8, s32) && !lanes_aligned(8, a1, s32));
    CHECK(!lanes_aligned(16, a16, s24) && lanes_aligned(8, a16, s24) && !lanes_aligned(16, a16, a8, s32) && !lanes_aligned(16, a16, s32, s24));
    CHECK(lanes_aligned(16, a16, (uintptr_t) nullptr, s32));                                          // (a bound frame that is not given)
    CHECK(lanes_aligned(16, a16, far) && !lanes_aligned(16, a16, far8) && lanes_aligned(8, a16, far8));      // (all 64 bits of a stride count)
    CHECK(lanes_aligned(16, a16, a16, (uint64_t)0) && !lanes_aligned(16, a16, a8, (uint64_t)0));     // (a single frame: 0 for the strides)
    printf("ok %ld\n", checks);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 8 && !strcmp(argv[1], "splits")) {
        const uint32_t unit = (uint32_t)atol(argv[2]), per_wg = (uint32_t)atol(argv[3]), tail_per_wg = (uint32_t)atol(argv[4]), rows_per_wg = (uint32_t)atol(argv[5]);
        for (uint64_t n = 1; n <= (uint64_t)atoll(argv[7]); ++n) {
            const LaneSplit s = split_lanes(n, unit, per_wg, tail_per_wg, rows_per_wg, atoi(argv[6]) != 0);
            printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.units, (unsigned long long)s.first_px, (unsigned long long)s.bx_vec,
                   (unsigned long long)s.bx_px, (unsigned long long)s.rows, (unsigned long long)s.tail_row_base);
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "block")) {
        for (int i = 2; i < argc; ++i) {
            unsigned long long v[8];
            if (sscanf(argv[i], "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) != 8) return 2;
            const PackedBlock b{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], v[4]};
            g_text[0] = 0;
            const int shape = check_block_shape(b, (uint32_t)v[5]);
            const int at = shape ? 0 : check_block_at(b, (uint32_t)v[5], (const void *)(uintptr_t)v[6], v[7] != 0);
            if (shape) printf("%d - %d\n", shape, g_text[0] != 0);
            else printf("%d %d %d\n", shape, at, g_text[0] != 0);
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "runs")) {
        const uint32_t nframes = (uint32_t)atol(argv[2]);
        for (int i = 3; i < argc; ++i) {
            std::vector<uint8_t> marks;
            const bool null = !strcmp(argv[i], "null");
            if (!null) {
                if (strlen(argv[i]) != nframes) return 2;
                for (uint32_t t = 0; t < nframes; ++t) marks.push_back(argv[i][t] == '1' ? 0x80 : 0);       // (any non-zero byte marks)
            }
            uint32_t next = 0;
            const int r = for_each_run(null ? nullptr : marks.data(), nframes, [&](uint32_t first, uint32_t len) {
                if (first != next || len == 0) return 7;                   // the runs tile the frames in order
                next = first + len;
                printf("%u:%u ", first, len);
                return 0;
            });
            if (r || next != nframes) return 3;
            printf("\n");
        }
        // the first non-zero return ends the walk and is handed back
        int calls = 0;
        if (for_each_run(nullptr, 0, [&](uint32_t, uint32_t) { return ++calls; }) != 0 || calls) return 4;
        std::vector<uint8_t> every(nframes, 1);
        if (nframes >= 3 && (for_each_run(every.data(), nframes, [&](uint32_t first, uint32_t) { ++calls; return first == 1 ? -34 : 0; }) != -34 || calls != 2)) return 4;
        return 0;
    }
    fprintf(stderr, "usage: block_plan_cases check | splits ... | block ... | runs ...\n");
    return 2;
}
