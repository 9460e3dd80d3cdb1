// rate_match_host.h -- host side of the frame source's rate-matching pattern
// (include/ldpc_hip.h "rate matching"): the validation of ldpc_rate_match_set
// and the tables the kernels of frame_rate_match.hip read; and of its bit
// interleaver ("bit interleaver and block fading"): the validation of
// ldpc_interleaver_set and the composite table col[t] = tx[perm[t]].  No HIP
// here, so a stand-alone program can run it under a sanitizer
// (tools/rate_match_host_check.cpp, tools/interleave_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ldpc {

constexpr float kRateMatchKnownLlr = 1.0e4f;  // LDPC_RM_KNOWN_LLR: exact in fp32 and fp64

// Empty when {punct, shrt} is a pattern a code with n columns, k of them
// information columns, can carry; else what is wrong with it (the contract's
// list, in its order).
inline std::string rate_match_validate(int n, int k, int32_t n_punct, const int32_t *punct, int32_t n_short,
                                       const int32_t *shrt) {
    if (n_punct < 0 || n_short < 0)
        return "negative count (n_punct = " + std::to_string(n_punct) + ", n_short = " + std::to_string(n_short) + ")";
    if ((n_punct > 0 && !punct) || (n_short > 0 && !shrt)) return "NULL column list with a positive count";
    if (n_punct > n || n_short > n) return "more columns listed than the code has (n = " + std::to_string(n) + ")";
    std::vector<uint8_t> seen((size_t)std::max(n, 0), 0);
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *cols = pass ? shrt : punct;
        const int32_t cnt = pass ? n_short : n_punct;
        const char *what = pass ? "shortened" : "punctured";
        for (int32_t i = 0; i < cnt; ++i) {
            const int32_t c = cols[i];
            if (c < 0 || c >= n)
                return std::string(what) + " column " + std::to_string(c) + " is outside [0, " + std::to_string(n) + ")";
            if (seen[(size_t)c]) return std::string("column ") + std::to_string(c) + " is listed twice (duplicate)";
            seen[(size_t)c] = 1;
        }
    }
    for (int32_t i = 0; i < n_short; ++i)
        if (shrt[i] >= k)
            return "shortened column " + std::to_string(shrt[i]) + " is not an information column (k = " +
                   std::to_string(k) + ")";
    if (n - n_punct - n_short < 1) return "no transmitted column is left (E < 1)";
    if (k - n_short < 1) return "no information bit is left (k - n_short < 1)";
    return std::string();
}

// What the kernels read, as one block of 32-bit words: tx_col [E] (the
// transmitted columns, ascending), fill_col [n_fill] (the others, ascending),
// fill_llr [n_fill] (fp32: +0.0 punctured, -kRateMatchKnownLlr shortened),
// umask [kw] (bit j%32 of word j/32 clear for a shortened column j).
struct RateMatchTables {
    int E = 0, n_fill = 0, kw = 0;
    std::vector<uint32_t> words;
    size_t tx_off() const { return 0; }
    size_t fill_off() const { return (size_t)E; }
    size_t llr_off() const { return (size_t)E + (size_t)n_fill; }
    size_t mask_off() const { return (size_t)E + 2 * (size_t)n_fill; }
};

// Words the tables of any pattern of an (n, k) code fit in.
inline size_t rate_match_max_words(int n, int k) { return 2 * (size_t)n + (size_t)((k + 31) >> 5); }

// The tables of a validated pattern.
inline RateMatchTables rate_match_build(int n, int k, const std::vector<int32_t> &punct,
                                        const std::vector<int32_t> &shrt) {
    std::vector<uint8_t> kind((size_t)n, 0);  // 0 transmitted, 1 punctured, 2 shortened
    for (int32_t c : punct) kind[(size_t)c] = 1;
    for (int32_t c : shrt) kind[(size_t)c] = 2;
    RateMatchTables t;
    t.n_fill = (int)(punct.size() + shrt.size());
    t.E = n - t.n_fill;
    t.kw = (k + 31) >> 5;
    t.words.assign(t.mask_off() + (size_t)t.kw, 0u);
    size_t it = t.tx_off(), jf = 0;
    for (int j = 0; j < n; ++j) {
        if (kind[(size_t)j] == 0) {
            t.words[it++] = (uint32_t)j;
            continue;
        }
        const float v = kind[(size_t)j] == 2 ? -kRateMatchKnownLlr : 0.0f;
        t.words[t.fill_off() + jf] = (uint32_t)j;
        std::memcpy(&t.words[t.llr_off() + jf], &v, sizeof v);
        ++jf;
    }
    for (int w = 0; w < t.kw; ++w) t.words[t.mask_off() + (size_t)w] = 0xFFFFFFFFu;
    for (int32_t c : shrt) t.words[t.mask_off() + (size_t)(c >> 5)] &= ~(1u << (c & 31));
    return t;
}

// ------------------------------------------------------------ interleaver
// (include/ldpc_hip.h "bit interleaver and block fading")  Empty when perm is a
// permutation of 0 .. len-1 (len == 0: none), else what is wrong with it.
inline std::string interleaver_validate(int32_t len, const int32_t *perm) {
    if (len < 0) return "negative length (len = " + std::to_string(len) + ")";
    if (len > 0 && !perm) return "NULL perm with a positive length";
    std::vector<uint8_t> seen((size_t)len, 0);
    for (int32_t t = 0; t < len; ++t) {
        const int32_t v = perm[t];
        if (v < 0 || v >= len)
            return "entry " + std::to_string(v) + " (position " + std::to_string(t) + ") is outside [0, " +
                   std::to_string(len) + ")";
        if (seen[(size_t)v]) return "entry " + std::to_string(v) + " is listed twice (duplicate)";
        seen[(size_t)v] = 1;
    }
    return std::string();
}

// The composite table: tx_col[t] = tx[perm[t]] in place, so that transmitted
// position t carries column tx[perm[t]].  perm must have passed
// interleaver_validate; false (tables untouched) unless its length is t.E.
inline bool interleaver_apply(RateMatchTables &t, const std::vector<int32_t> &perm) {
    if ((int)perm.size() != t.E) return false;
    std::vector<uint32_t> tx(t.words.begin() + (std::ptrdiff_t)t.tx_off(),
                             t.words.begin() + (std::ptrdiff_t)(t.tx_off() + (size_t)t.E));
    for (int i = 0; i < t.E; ++i) {
        const int32_t p = perm[(size_t)i];
        if (p < 0 || p >= t.E) return false;
        t.words[t.tx_off() + (size_t)i] = tx[(size_t)p];
    }
    return true;
}

// ------------------------------------------------------------------- HARQ
// (include/ldpc_hip.h "HARQ")  Empty when {tx_len, cols} is a plan of n_tx
// transmissions a code with n columns can carry (n_tx == 0: none), else what is
// wrong with it (the contract's list, in its order).  cols is read only as far
// as the lengths checked so far say.
constexpr int kHarqMaxTxHost = 8;  // LDPC_HARQ_MAX_TX
inline std::string harq_validate(int n, int32_t n_tx, const int32_t *tx_len, const int32_t *cols) {
    if (n_tx < 0 || n_tx > kHarqMaxTxHost)
        return "n_tx = " + std::to_string(n_tx) + " is outside [0, " + std::to_string(kHarqMaxTxHost) +
               "] (LDPC_HARQ_MAX_TX)";
    if (n_tx > 0 && (!tx_len || !cols)) return "NULL tx_len or cols with n_tx > 0";
    for (int32_t r = 0; r < n_tx; ++r)
        if (tx_len[r] < 1 || tx_len[r] > n)
            return "tx_len[" + std::to_string(r) + "] = " + std::to_string(tx_len[r]) +
                   (tx_len[r] < 1 ? " < 1" : " > n = " + std::to_string(n) + " (a duplicate column within the transmission)");
    std::vector<int32_t> seen((size_t)std::max(n, 0), -1);  // the last transmission that carried the column
    size_t off = 0;
    for (int32_t r = 0; r < n_tx; ++r) {
        for (int32_t t = 0; t < tx_len[r]; ++t) {
            const int32_t c = cols[off + (size_t)t];
            if (c < 0 || c >= n)
                return "column " + std::to_string(c) + " (transmission " + std::to_string(r) + ", position " +
                       std::to_string(t) + ") is outside [0, " + std::to_string(n) + ")";
            if (seen[(size_t)c] == r)
                return "column " + std::to_string(c) + " is listed twice in transmission " + std::to_string(r) +
                       " (duplicate)";
            seen[(size_t)c] = r;
        }
        off += (size_t)tx_len[r];
    }
    return std::string();
}

// The last gate before an upload: every index a kernel gathers or scatters with
// lies in [0, n), tx_col and fill_col together name every column exactly once,
// and the block fits the device allocation.
inline bool rate_match_tables_ok(const RateMatchTables &t, int n, int k) {
    if (t.E < 1 || t.n_fill < 0 || t.E + t.n_fill != n || t.kw != ((k + 31) >> 5)) return false;
    if (t.words.size() != t.mask_off() + (size_t)t.kw || t.words.size() > rate_match_max_words(n, k)) return false;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (size_t i = 0; i < (size_t)t.E + (size_t)t.n_fill; ++i) {
        const uint32_t c = t.words[i];  // tx_col, then fill_col
        if (c >= (uint32_t)n || seen[c]) return false;
        seen[c] = 1;
    }
    return true;
}

}  // namespace ldpc
