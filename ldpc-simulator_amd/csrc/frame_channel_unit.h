// frame_channel_unit.h -- the arithmetic of one channel-model "unit" (what one
// Philox noise block serves: a symbol, or for BPSK the two bits 2i, 2i+1),
// shared by the frame source's channel kernels (frame_channel_models.hip) and
// its HARQ kernels (frame_harq.hip), so that a transmission of a HARQ plan is
// the frame the single-transmission kernels make, operation for operation.
// The formulas are at the head of frame_channel_models.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frame_source.h"
#include "spa_device.h"

namespace ldpc {
namespace {

constexpr int kChRayleigh = 2;  // LDPC_CH_RAYLEIGH
constexpr int kDemapMaxlog = 1;  // LDPC_DEMAP_MAXLOG

// LLRs of the M Gray-labelled bits of one axis with 2^M levels, a_0 first.
template <int M, int DEMAP>
__device__ __forceinline__ void axis_llr(double r, double h, double s2, double *out) {
    constexpr int L = 1 << M;
    constexpr double d = M == 1 ? 0.70710678118654752440 : M == 2 ? 0.31622776601683793320 : 0.15430334996209191026;
    if constexpr (M == 1) {
        out[0] = 2.0 * h * d * r / s2;
    } else {
        double mu[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const double t = r - h * ((double)(2 * i - (L - 1)) * d);
            mu[i] = t * t / (2.0 * s2);
        }
#pragma unroll
        for (int t = 0; t < M; ++t) {
            double min0 = INFINITY, min1 = INFINITY;
#pragma unroll
            for (int i = 0; i < L; ++i) {
                if (((i ^ (i >> 1)) >> (M - 1 - t)) & 1)
                    min1 = fmin(min1, mu[i]);
                else
                    min0 = fmin(min0, mu[i]);
            }
            if constexpr (DEMAP == kDemapMaxlog) {
                out[t] = min0 - min1;
            } else {
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    if (((i ^ (i >> 1)) >> (M - 1 - t)) & 1)
                        s1 += exp(-(mu[i] - min1));
                    else
                        s0 += exp(-(mu[i] - min0));
                }
                out[t] = (log(s1) - min1) - (log(s0) - min0);
            }
        }
    }
}

template <int BPS>
struct Unit {
    static constexpr int kAxisBits = BPS == 1 ? 1 : BPS / 2;
    static constexpr int kBits = 2 * kAxisBits;       // BPSK: the two bits of a noise block
    static constexpr int kPerBlock = 128 / kBits;     // units a block of the tile form walks
    __host__ __device__ static int count(int n) { return BPS == 1 ? (n + 1) >> 1 : n / BPS; }
};

// llr[0 .. kBits) of unit i of frame F; a BPSK bit past n - 1 (odd n) gets 0.
// BPSK is one real dimension with the levels +-1: the one-bit expression with d = 1.
// RM (a rate-matching pattern, a bit interleaver or a HARQ transmission): n is
// the number of transmitted bits E and position t of the sequence is column
// tx[t]; else position t is column t and tx is not read.
// BF (block fading, Rayleigh): the two axes (BPSK: two bits) fade by hb[0],
// hb[1], the caller's; else a fade of its own per symbol (BPSK: per bit).
template <int BPS, int MODEL, int DEMAP, bool RM = false, bool BF = false>
__device__ __forceinline__ void unit_llr(const uint32_t *Ut, const uint32_t *Pt, const uint32_t *Wt, int k, int n,
                                         uint64_t seed, int64_t F, int snr_point, int i, double sigma, double *llr,
                                         const int32_t *__restrict__ tx = nullptr, const double *hb = nullptr) {
    constexpr int M = Unit<BPS>::kAxisBits;
    constexpr int L = 1 << M;
    constexpr double d = BPS == 1   ? 1.0
                         : M == 1 ? 0.70710678118654752440
                         : M == 2 ? 0.31622776601683793320
                                  : 0.15430334996209191026;
    const double s2 = sigma * sigma;
    double g[2];
    noise_pair(seed, F, snr_point, i, g);
    double h[2] = {1.0, 1.0};
    if constexpr (MODEL == kChRayleigh) {
        double u[2];
        if constexpr (BF) {
            h[0] = hb[0];
            h[1] = hb[1];
        } else if constexpr (BPS == 1) {
            fade_uniforms(seed, F, snr_point, i, u);
            h[0] = sqrt(-log(u[0]));
            h[1] = sqrt(-log(u[1]));
        } else {
            fade_uniforms(seed, F, snr_point, i >> 1, u);
            h[0] = h[1] = sqrt(-log((i & 1) ? u[1] : u[0]));
        }
    }
    const int j0 = i * Unit<BPS>::kBits;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (BPS == 1 && j0 + q >= n) {
            llr[q] = 0.0;
            continue;
        }
        uint32_t a = 0u;  // the axis's Gray label, a_0 the most significant bit
#pragma unroll
        for (int t = 0; t < M; ++t) {
            const int tb = j0 + q * M + t;
            a = (a << 1) | frame_bit(Ut, Pt, Wt, k, RM ? tx[tb] : tb);
        }
        const int B = (int)(a ^ (a >> 1) ^ (a >> 2));  // b_i = b_(i-1) xor a_i (M <= 3)
        const double x = (double)(2 * B - (L - 1)) * d;
        const double r = h[q] * x + sigma * g[q];
        if constexpr (BPS == 1)
            llr[q] = 2.0 * h[q] * d * r / s2;
        else
            axis_llr<M, DEMAP>(r, h[q], s2, llr + q * M);
    }
}

// Block fading (ldpc_fading_set, Rayleigh): the fade of index B, the draw a
// symbol of that index has without it.
__device__ __forceinline__ double block_fade(uint64_t seed, int64_t F, int snr_point, int B) {
    double u[2];
    fade_uniforms(seed, F, snr_point, B >> 1, u);
    return sqrt(-log((B & 1) ? u[1] : u[0]));
}

// h[0], h[1] of unit i when block_len symbols (BPSK: transmitted positions)
// share a fade: a symbol's two axes have index i / block_len, the two BPSK
// positions 2i and 2i + 1 an index each.  {*Bc, *hc} is the caller's last
// index and its fade (start with *Bc = -1): a caller that walks consecutive
// units pays the log and sqrt once per fading block.
template <int BPS>
__device__ __forceinline__ void block_fades(uint64_t seed, int64_t F, int snr_point, int i, int block_len, int *Bc,
                                            double *hc, double h[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int B = BPS == 1 ? (2 * i + q) / block_len : i / block_len;
        if (B != *Bc) {
            *Bc = B;
            *hc = block_fade(seed, F, snr_point, B);
        }
        h[q] = *hc;
    }
}

// ------------------------------------------------------ constellation table
// The second unit kind (include/ldpc_hip.h "constellations"): one symbol of a
// table of 2^BPS complex points, for every BPS one noise pair of its own.
// The table travels as a kernel argument, so the loops over its points, which
// are uniform across the wavefront in both kernel forms, read it with scalar
// loads; every array below has static indices after unrolling.
template <int BPS>
struct TablePoints {
    double xy[2 << BPS];  // re, im of label 0, 1, ...
};

template <int BPS>
struct TableUnit {
    static constexpr int kPoints = 1 << BPS;
    static constexpr int kPerBlock = 128 / BPS;  // symbols a block of the tile form walks
};

// At most this far below the nearest point's class does the other class of a
// bit share the nearest point's exponentials; exp(-500) is still a normal number.
constexpr double kTableShareMax = 500.0;

// llr[0 .. BPS) of the symbol with label a, fade h and noise g: r = h x_a +
// sigma g, mu_i = |r - h x_i|^2 / (2 sigma^2).
// Exact: e_i = exp(-(mu_i - m)) with m the smallest mu, once per point.  The
// class of bit t that holds the nearest point has its own maximum m, so its
// sum is the contract's.  The other class (smallest metric m') takes the same
// e_i while m' - m <= kTableShareMax: log(sum e_i) - m is its LSE with a
// relative error of (m' - m) 2^-53 in each term; beyond that it takes its own
// exp(-(mu_i - m')).  2^BPS exponentials a symbol, plus 2^BPS (half of them of
// -inf) for each bit whose classes are more than kTableShareMax apart.
template <int BPS, int DEMAP>
__device__ __forceinline__ void table_llr(const TablePoints<BPS> &tab, uint32_t a, double h, double sigma,
                                          const double g[2], double *llr) {
    constexpr int P = 1 << BPS;
    double xr = 0.0, xq = 0.0;  // the one per-lane lookup, as selects over the uniform loop
#pragma unroll
    for (int i = 0; i < P; ++i) {
        xr = a == (uint32_t)i ? tab.xy[2 * i] : xr;
        xq = a == (uint32_t)i ? tab.xy[2 * i + 1] : xq;
    }
    const double rr = h * xr + sigma * g[0];
    const double rq = h * xq + sigma * g[1];
    const double two_s2 = 2.0 * (sigma * sigma);
    double mu[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const double dr = rr - h * tab.xy[2 * i];
        const double dq = rq - h * tab.xy[2 * i + 1];
        mu[i] = (dr * dr + dq * dq) / two_s2;
    }
    if constexpr (DEMAP == kDemapMaxlog) {
#pragma unroll
        for (int t = 0; t < BPS; ++t) {
            double mn[2] = {INFINITY, INFINITY};
#pragma unroll
            for (int i = 0; i < P; ++i) mn[(i >> (BPS - 1 - t)) & 1] = fmin(mn[(i >> (BPS - 1 - t)) & 1], mu[i]);
            llr[t] = mn[0] - mn[1];
        }
    } else {
        double m = mu[0];
#pragma unroll
        for (int i = 1; i < P; ++i) m = fmin(m, mu[i]);
        double e[P];
#pragma unroll
        for (int i = 0; i < P; ++i) e[i] = exp(-(mu[i] - m));
        // the near path of every bit with static class tests: one fmin and one
        // add per point and bit
        uint32_t far_bits = 0u;
#pragma unroll
        for (int t = 0; t < BPS; ++t) {
            double mn[2] = {INFINITY, INFINITY}, s[2] = {0.0, 0.0};
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int c = (i >> (BPS - 1 - t)) & 1;
                mn[c] = fmin(mn[c], mu[i]);
                s[c] += e[i];
            }
            llr[t] = (log(s[1]) - m) - (log(s[0]) - m);
            if (fmax(mn[0], mn[1]) - m > kTableShareMax) far_bits |= 1u << t;
        }
        // the far path: t is a run-time value here, so that the kernel holds
        // its exponentials once, not once per bit; mu and llr keep their
        // static indices (the class tests become selects)
        if (far_bits != 0u) {
#pragma unroll 1
            for (int t = 0; t < BPS; ++t) {
                if (!((far_bits >> t) & 1u)) continue;
                const int sh = BPS - 1 - t;
                double mn0 = INFINITY, mn1 = INFINITY, s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const bool one = (i >> sh) & 1;
                    mn0 = one ? mn0 : fmin(mn0, mu[i]);
                    mn1 = one ? fmin(mn1, mu[i]) : mn1;
                    s0 += one ? 0.0 : e[i];
                    s1 += one ? e[i] : 0.0;
                }
                // the class that does not hold the nearest point, and its smallest metric
                const bool far1 = mn1 > mn0;
                const double mo = far1 ? mn1 : mn0;
                double so = 0.0;
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const bool one = (i >> sh) & 1;
                    // a point of the near class has no weight: exp(-inf) = +0
                    so += exp(-(one == far1 ? mu[i] - mo : INFINITY));
                }
                const double lse_far = log(so) - mo;
                const double lse_near = log(far1 ? s0 : s1) - m;
                const double v = far1 ? lse_far - lse_near : lse_near - lse_far;
#pragma unroll
                for (int tt = 0; tt < BPS; ++tt) llr[tt] = tt == t ? v : llr[tt];
            }
        }
    }
}

// The label of symbol i of frame F's transmitted sequence (first bit most
// significant); position t is column tx[t], or column t without tx.
template <int BPS>
__device__ __forceinline__ uint32_t table_label(const uint32_t *Ut, const uint32_t *Pt, const uint32_t *Wt, int k, int i,
                                                const int32_t *__restrict__ tx) {
    uint32_t a = 0u;
#pragma unroll
    for (int t = 0; t < BPS; ++t) {
        const int tb = i * BPS + t;
        a = (a << 1) | frame_bit(Ut, Pt, Wt, k, tx ? tx[tb] : tb);
    }
    return a;
}

}  // namespace
}  // namespace ldpc
