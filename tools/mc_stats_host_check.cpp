// mc_stats_host_check.cpp -- the host bookkeeping of ldpc_mc_stats_read
// (csrc/mc_stats_host.h: buffer sizes, record clipping, sorting) in a program of
// its own, so that it can run under a sanitizer on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ldpc-simulator_amd/csrc \
//       tools/mc_stats_host_check.cpp -o /tmp/mc_stats_host_check && /tmp/mc_stats_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mc_stats_host.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    using namespace ldpc;
    CHECK(mc_stats_point_words(20) == 3 + 21);
    CHECK(mc_stats_words(2, 20, 0) == 2 * 24);
    CHECK(mc_stats_words(3, 1, 8) == 3 * (5 + 16));
    CHECK(mc_stats_stored(0, 8) == 0);
    CHECK(mc_stats_stored(5, 8) == 5);
    CHECK(mc_stats_stored(8, 8) == 8);
    CHECK(mc_stats_stored(1000, 8) == 8);
    CHECK(mc_stats_stored(7, 0) == 0);
    CHECK(mc_stats_stored(7, -1) == 0);
    CHECK(mc_stats_stored(~0ull, 8) == 8);
    // records in the order the workgroups reserved them -> sorted by frame index
    uint64_t x = 88172645463325252ull;
    for (int64_t n : {0, 1, 2, 7, 64, 1000}) {
        std::vector<int64_t> rec(2 * (size_t)n), out(2 * (size_t)n, -1);
        for (int64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            rec[2 * i] = (int64_t)(x % 100000) * 1000 + i;  // distinct
            rec[2 * i + 1] = rec[2 * i] % 97;
        }
        mc_stats_sort_records(rec.data(), n, out.data());
        for (int64_t i = 0; i < n; ++i) {
            CHECK(out[2 * i + 1] == out[2 * i] % 97);  // a record's count stays with its index
            if (i) CHECK(out[2 * i - 2] < out[2 * i]);
        }
    }
    std::puts("mc_stats_host_check: OK");
    return 0;
}
