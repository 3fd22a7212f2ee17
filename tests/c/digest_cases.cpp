// digest_cases.cpp -- csrc/rbf_digest.h under a plain host compiler (tests/test_frame_digest_cpu.py builds it with g++: no HIP, no GPU).
//   digest_cases prefixes <file> <len>...   fd1_host of the first <len> bytes of <file>, one hex digest per line
//   digest_cases levels <L>...              per L one line: L, fd1_levels(L), the blocks of every level in front of the final block,
//                                           fd1_scratch_words(L)
#include "../../new_bloom_filter_repo_amd/csrc/rbf_digest.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "prefixes")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { perror(argv[2]); return 2; }
        std::vector<unsigned char> data;
        unsigned char buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
        fclose(f);
        for (int i = 3; i < argc; ++i) {
            const unsigned long long len = strtoull(argv[i], nullptr, 10);
            if (len > data.size()) { fprintf(stderr, "length %llu past the file's %zu bytes\n", len, data.size()); return 2; }
            // an exact-size copy, so that a host sanitizer sees any read past byte len-1
            std::vector<unsigned char> exact(data.begin(), data.begin() + (size_t)len);
            printf("%016llX\n", (unsigned long long)rbf::fd1_host(exact.data(), exact.size()));
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "levels")) {
        for (int i = 2; i < argc; ++i) {
            const uint64_t L = strtoull(argv[i], nullptr, 10);
            const uint32_t levels = rbf::fd1_levels(L);
            printf("%llu %u", (unsigned long long)L, levels);
            for (uint32_t k = 0; k < levels; ++k) printf(" %llu", (unsigned long long)rbf::fd1_blocks(rbf::fd1_level_bytes(L, k)));
            printf(" %llu\n", (unsigned long long)rbf::fd1_scratch_words(L));
        }
        return 0;
    }
    fprintf(stderr, "usage: digest_cases prefixes <file> <len>... | levels <L>...\n");
    return 2;
}
