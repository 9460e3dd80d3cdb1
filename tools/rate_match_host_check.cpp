// rate_match_host_check.cpp -- the host side of ldpc_rate_match_set
// (csrc/rate_match_host.h: the pattern's validation and the kernels' tables) in a
// program of its own, so that it can run under a sanitizer on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ldpc-simulator_amd/csrc
//       tools/rate_match_host_check.cpp -o /tmp/rate_match_host_check && /tmp/rate_match_host_check
// (one command line)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rate_match_host.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

namespace {
using V = std::vector<int32_t>;
std::string check(int n, int k, const V &p, const V &s) {
    return ldpc::rate_match_validate(n, k, (int32_t)p.size(), p.empty() ? nullptr : p.data(), (int32_t)s.size(),
                                     s.empty() ? nullptr : s.data());
}
bool has(const std::string &s, const char *needle) { return s.find(needle) != std::string::npos; }
}  // namespace

int main() {
    using namespace ldpc;
    // n = 66, k = 46 (the tests' tiny graph)
    CHECK(check(66, 46, {}, {}).empty());
    CHECK(check(66, 46, {0, 7, 45, 46, 47, 65}, {1, 33, 44}).empty());
    CHECK(has(rate_match_validate(66, 46, -1, nullptr, 0, nullptr), "negative"));
    CHECK(has(rate_match_validate(66, 46, 0, nullptr, -3, nullptr), "negative"));
    CHECK(has(rate_match_validate(66, 46, 2, nullptr, 0, nullptr), "NULL"));
    CHECK(has(rate_match_validate(66, 46, 0, nullptr, 1, nullptr), "NULL"));
    CHECK(has(check(66, 46, {66}, {}), "outside"));
    CHECK(has(check(66, 46, {-1}, {}), "outside"));
    CHECK(has(check(66, 46, {3}, {-7}), "outside"));
    CHECK(has(check(66, 46, {5, 9, 5}, {}), "twice"));
    CHECK(has(check(66, 46, {}, {2, 2}), "twice"));
    CHECK(has(check(66, 46, {5}, {5}), "twice"));
    CHECK(has(check(66, 46, {}, {46}), "information column"));
    CHECK(check(66, 46, {46}, {45}).empty());
    {
        V p, s;
        for (int j = 21; j < 66; ++j) p.push_back(j);
        for (int j = 0; j < 21; ++j) s.push_back(j);
        CHECK(has(check(66, 46, p, s), "E < 1"));
        p.pop_back();
        CHECK(check(66, 46, p, s).empty());  // E = 1
        V all;
        for (int j = 0; j < 46; ++j) all.push_back(j);
        CHECK(has(check(66, 46, {}, all), "information bit"));
        V many(67, 0);
        CHECK(!check(66, 46, many, {}).empty());  // more entries than columns: refused before any table is sized by it
    }
    // tables: E = 57, 9 columns not sent, kw = 2
    {
        const V p = {0, 7, 45, 46, 47, 65}, s = {1, 33, 44};
        const RateMatchTables t = rate_match_build(66, 46, p, s);
        CHECK(t.E == 57 && t.n_fill == 9 && t.kw == 2);
        CHECK(t.words.size() == 57 + 9 + 9 + 2 && t.words.size() <= rate_match_max_words(66, 46));
        std::vector<int> kind(66, -1);
        for (int i = 0; i < t.E; ++i) {
            const int j = (int)t.words[t.tx_off() + i];
            CHECK(j >= 0 && j < 66 && kind[j] == -1);
            if (i) CHECK((int)t.words[t.tx_off() + i - 1] < j);  // ascending
            kind[j] = 0;
        }
        CHECK(t.words[t.tx_off()] == 2 && t.words[t.tx_off() + 56] == 64);
        for (int i = 0; i < t.n_fill; ++i) {
            const int j = (int)t.words[t.fill_off() + i];
            CHECK(j >= 0 && j < 66 && kind[j] == -1);
            float v;
            std::memcpy(&v, &t.words[t.llr_off() + i], sizeof v);
            const bool shortened = j == 1 || j == 33 || j == 44;
            CHECK(v == (shortened ? -1.0e4f : 0.0f));
            if (!shortened) CHECK(t.words[t.llr_off() + i] == 0u);  // +0.0, not -0.0
            kind[j] = shortened ? 2 : 1;
        }
        for (int j = 0; j < 66; ++j) CHECK(kind[j] >= 0);  // every column is in exactly one list
        CHECK(t.words[t.mask_off()] == ~(1u << 1));
        CHECK(t.words[t.mask_off() + 1] == ~((1u << (33 - 32)) | (1u << (44 - 32))));
    }
    // nothing shortened: the mask is all ones; the largest pattern fits the allocation
    {
        const RateMatchTables t = rate_match_build(64, 32, {63}, {});
        CHECK(t.E == 63 && t.kw == 1 && t.words[t.mask_off()] == 0xFFFFFFFFu);
        V p;
        for (int j = 1; j < 64; ++j) p.push_back(j);
        const RateMatchTables big = rate_match_build(64, 32, p, {});
        CHECK(big.E == 1 && big.words.size() <= rate_match_max_words(64, 32));
    }
    std::puts("rate_match_host_check: OK");
    return 0;
}
