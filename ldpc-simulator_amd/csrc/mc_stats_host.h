// mc_stats_host.h -- host bookkeeping of the Monte-Carlo statistics
// (ldpc_mc_stats_read): no HIP here, so a stand-alone program can run it under
// a sanitizer (tools/mc_stats_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ldpc {

// Words of one point's header on the device: undetected frames, their info-bit
// errors, failed frames seen (the record reservations), then hist[max_iter + 1].
constexpr int kMcStatsHead = 3;
inline size_t mc_stats_point_words(int max_iter) { return (size_t)kMcStatsHead + (size_t)max_iter + 1; }
// Words of a whole run: the points' headers, then their record arrays [max_failed][2].
inline size_t mc_stats_words(int n_points, int max_iter, int max_failed) {
    return (size_t)n_points * (mc_stats_point_words(max_iter) + 2 * (size_t)max_failed);
}

// Records a point stored: the kernels reserved `seen` records and wrote those
// with an index below max_failed.
inline int64_t mc_stats_stored(uint64_t seen, int max_failed) {
    return (int64_t)std::min<uint64_t>(seen, (uint64_t)std::max(max_failed, 0));
}

// The stored records [stored][2] (frame index, info-bit errors) as read from the
// device, sorted by frame index into out [stored][2].
inline void mc_stats_sort_records(const int64_t *rec, int64_t stored, int64_t *out) {
    std::vector<std::pair<int64_t, int64_t>> v;
    v.reserve((size_t)std::max<int64_t>(stored, 0));
    for (int64_t i = 0; i < stored; ++i) v.emplace_back(rec[2 * i], rec[2 * i + 1]);
    std::sort(v.begin(), v.end());
    for (int64_t i = 0; i < stored; ++i) {
        out[2 * i] = v[(size_t)i].first;
        out[2 * i + 1] = v[(size_t)i].second;
    }
}

}  // namespace ldpc
