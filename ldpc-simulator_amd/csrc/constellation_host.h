// constellation_host.h -- host bookkeeping of the frame source's constellation
// table (ldpc_constellation_set / _get; contract: include/ldpc_hip.h
// "constellations"): no HIP here, so a stand-alone program can run it under a
// sanitizer (tools/constellation_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ldpc {

constexpr int kConstMaxBps = 6;          // LDPC_CONST_MAX_BPS
constexpr double kConstEnergyTol = 1e-9;  // |mean |x|^2 - 1| a table may have

// Empty if `points` (2^bps pairs re, im, indexed by label) is a table
// ldpc_constellation_set takes, else what is wrong with it.  bps == 0 (clear)
// reads nothing; nothing past 2 * 2^bps doubles is read.
inline std::string constellation_validate(int32_t bps, const double *points) {
    char buf[192];
    if (bps < 0 || bps > kConstMaxBps) {
        std::snprintf(buf, sizeof buf, "bps %d is outside 0 (clear) .. LDPC_CONST_MAX_BPS = %d", bps, kConstMaxBps);
        return buf;
    }
    if (bps == 0) return "";
    if (!points) return "NULL points with bps > 0";
    const int np = 1 << bps;
    double energy = 0.0;
    for (int i = 0; i < np; ++i) {
        const double re = points[2 * i], im = points[2 * i + 1];
        if (!std::isfinite(re) || !std::isfinite(im)) {
            std::snprintf(buf, sizeof buf, "point %d has a coordinate that is not finite", i);
            return buf;
        }
        energy += re * re + im * im;
    }
    energy /= (double)np;
    if (!(std::fabs(energy - 1.0) <= kConstEnergyTol)) {
        std::snprintf(buf, sizeof buf, "the mean energy of the %d points is %.12g, not 1 to within 1e-9 (sigma means "
                                       "Es/N0 = 1 / (2 sigma^2) only at unit energy)", np, energy);
        return buf;
    }
    for (int i = 0; i < np; ++i)
        for (int j = i + 1; j < np; ++j)
            if (points[2 * i] == points[2 * j] && points[2 * i + 1] == points[2 * j + 1]) {
                std::snprintf(buf, sizeof buf, "points %d and %d are equal: their labels could not be told apart", i, j);
                return buf;
            }
    return "";
}

// A decoder's table: bps == 0 is none.
struct ConstellationTable {
    int bps = 0;
    std::vector<double> xy;  // 2 * 2^bps: re, im of label 0, 1, ...

    // points validated by constellation_validate
    void assign(int32_t new_bps, const double *points) {
        bps = new_bps;
        if (bps > 0)
            xy.assign(points, points + ((size_t)2 << bps));
        else
            xy.clear();
    }
    // 0: copied (out may be null: nothing copied), else the doubles out needs
    int copy_to(double *out, int32_t cap) const {
        if (!out) return 0;
        if (cap < 0 || (size_t)cap < xy.size()) return (int)xy.size();
        for (size_t i = 0; i < xy.size(); ++i) out[i] = xy[i];
        return 0;
    }
};

}  // namespace ldpc
