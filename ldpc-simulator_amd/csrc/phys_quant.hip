// phys_quant.hip -- physical mode, fixed-point min-sum with q-bit messages
// (q = 4..8), flooding and layered schedules, gfx950.
//
// What a hardware decoder computes: saturating integer messages, no float after
// the load.  The contract (DESIGN.md "Physical mode: fixed-point min-sum";
// tests/qminsum_ref.py restates it in numpy int32, and every output equals it):
//   Qmax = 2^(q-1) - 1,  Pmax = 2^(q+1) - 1  (511 at q = 8: posteriors fit int16)
//   load (the only fp32 operations, each rounds once):
//     x = (-(float)llr[j]) * llr_scale   (lam[j] * llr_scale for on-device frames)
//     Lam[j] = (int)clamp(rintf(x), -Qmax, Qmax)   rintf: half to even
//              (v_rndne_f32); the clamp is in float, before the conversion
//     L = Lam, E = 0
//   check row r, edges in CSR order:
//     Q_e = clamp(L[c_e] - E_e, -Qmax, Qmax),  a_e = |Q_e|,  s_e = (Q_e < 0)
//     min1 = smallest a, min2 = smallest over the other edges (= min1 on a tie)
//     mag_e = (e is the argmin) ? min2 : min1
//     NMS: mag_e = (alpha_q * mag_e + 8) >> 4      alpha_q in 1..16 (sixteenths)
//     OMS: mag_e = max(mag_e - beta_q, 0)          beta_q in 0..Qmax (steps)
//     R_e = (parity(all s) ^ s_e) ? -mag_e : mag_e
//   flooding: every row from the same L and E, E = R, then
//     L[j] = clamp(Lam[j] + sum E, -Pmax, Pmax)   an int32 sum clamped once:
//                                                 the order of the adds is immaterial
//   layered (ldpc_layers_build's layers, in order): L[c_e] = Q_e + R_e, E_e = R_e.
//     |L| <= 2 Qmax < Pmax by construction: this schedule has no posterior clamp.
//   exit: after each full iteration b = (L < 0) (L == 0 is bit 0); conv = the
//   first iteration with H b = 0.  post_out is the integer posterior, int16, in
//   units of 1 / llr_scale.
// Worked values:  q = 6 (Qmax 31), NMS alpha_q = 12, a row with L - E = [5, -3, 40, 0]:
//   Q = [5, -3, 31, 0], min1 = 0 (edge 3), min2 = 3, magnitudes [0, 0, 0, (36+8)>>4 = 2],
//   parity 1, R = [0, 0, 0, -2].   llr_scale = 4: llr 0.625 -> Lam -2 (x = -2.5),
//   llr 0.875 -> Lam -4 (x = -3.5): both ties round to even.
//
// One workgroup per frame, frames grid-strided.  LDS holds E as int8, L as
// int16 and (flooding only) Lam as int8: 16 KB for wimax_2304_0.5 where the
// fp32 kernels hold 48 KB, so registers and the 32-wave limit, not LDS, set
// the frames per CU (7 workgroups of 4 wavefronts).  A row's messages start at a 4-byte
// aligned, padded offset (the per-graph table QuantTab, built by ldpc_api.cpp
// on first use), so a row is read and written as ceil(deg / 4) dwords, and its
// column indices -- 16 bit, in the same padded order -- as one 8-byte load per
// dword of messages.  A row takes two sweeps: the first forms Q, finds the two
// smallest |Q| and the sign parity and leaves Q in the row's own message bytes
// (nobody else reads them before the row's R replaces them); the second reads
// Q back, so it needs neither L nor, in the flooding schedule, the columns.
// min2 equals min1 on a tie, so "e is the argmin" is a_e == min1.
//
// Flooding folds the syndrome into the next iteration's first sweep, which
// reads every L[c_e] of every row anyway: the frame leaves with conv = it - 1
// when that sweep finds H b = 0 (L is untouched by a check sweep; E is dead by
// then).  That costs a converged frame one check sweep too many, which is most
// of the work where frames converge at once, so the first kQEarlySyn
// iterations (and the last, which has no next) get a syndrome sweep of their
// own right after the variable nodes.  Two barriers per iteration after those.
// The layered schedule changes L inside an iteration and keeps the syndrome
// sweep after its last layer.
//
// phys_quant_kernel covers any row and column degree with byte-addressed
// generic loops and index loads in the loop; phys_quant_reg_kernel (below) is
// the flooding decoder with the indices in registers, for the graphs whose
// shape it has (LDPC_PHYS_Q_REG=0 forces the generic one).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "phys_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

// Flooding: iterations whose posterior gets a syndrome sweep of its own, right
// after the variable nodes (see the header): the frames of a clean channel
// stop there and skip a whole check sweep.
constexpr int kQEarlySyn = 2;
// LDS a workgroup may take (ldpc_api.cpp's kLdsLimit)
constexpr size_t kQLdsLimit = 160 * 1024 - 1024;

struct QuantArgs {
    DevGraph g;
    const double *llr;        // layout 0: [count][n] channel LLRs
    const float *lam;         // layout 2: [count][n] fp32 Lambda (on-device frames), else null
    int count;
    int max_iter;
    uint8_t *z_out;           // [count][n] or null: z = (bit estimate) ^ 1
    int *conv_out;            // [count] or null
    int *status_out;          // [count] or null
    int *iters_out;           // [count] or null
    int16_t *post_out;        // [count][n] or null: integer posteriors
    const uint32_t *ubits;    // MC: info bits [tile][kw][64], else null
    unsigned long long *ctr;  // MC: counters [7] or null
    QuantTab t;
    int qmax, pmax, param_q;
    float scale;
    const int *layer_ptr;     // layered: as PhysArgs
    const int *layer_rows;
    int n_layers;
};

__device__ __forceinline__ int q_clamp(int v, int lim) { return min(max(v, -lim), lim); }

// Frame f's Lam[j] (the contract's load).
__device__ __forceinline__ int q_lambda(const QuantArgs &a, int f, int j) {
    const size_t i = (size_t)f * a.g.n + j;
    const float x = (a.lam ? a.lam[i] : -(float)a.llr[i]) * a.scale;
    const float lim = (float)a.qmax;
    return (int)fminf(fmaxf(rintf(x), -lim), lim);
}

template <int CN>
__device__ __forceinline__ int q_scale(int mag, int param_q) {
    static_assert(CN == kCnNms || CN == kCnOms, "min-sum rules only");
    if constexpr (CN == kCnNms) return (param_q * mag + 8) >> 4;
    else return max(mag - param_q, 0);
}

__device__ __forceinline__ int q_col(const uint2 &c, int b) {
    return (int)(((b < 2 ? c.x : c.y) >> ((b & 1) * 16)) & 0xffffu);
}

// One check row (the contract's check rule).  E: the row's message dwords in
// LDS; cw: its columns, four to a uint2.  Returns the parity of (L[c_e] < 0)
// over the row as it stood before the update (the syndrome bit of the posterior
// the row read).  LAYERED also writes L[c_e] = Q_e + R_e.
template <int CN, bool LAYERED>
__device__ __forceinline__ unsigned q_check_row(const QuantArgs &a, uint32_t *E, int16_t *L, const uint2 *cw,
                                                int deg) {
    int min1 = 0x7fff, min2 = 0x7fff;
    unsigned neg = 0u, par = 0u;
    const int full = deg >> 2, tail = deg & 3;
    auto first = [&](int w, int nv) {
        const uint32_t ew = E[w];
        const uint2 c = cw[w];
        uint32_t qw = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nv) {
                const int l = L[q_col(c, b)];
                const int q = q_clamp(l - (int)(int8_t)(ew >> (8 * b)), a.qmax);
                const int aq = abs(q);
                min2 = min(min2, max(min1, aq));
                min1 = min(min1, aq);
                neg ^= (unsigned)q >> 31;
                par ^= (unsigned)l >> 31;
                qw |= ((uint32_t)q & 0xffu) << (8 * b);
            }
        }
        E[w] = qw;
    };
    for (int w = 0; w < full; ++w) first(w, 4);
    if (tail) first(full, tail);
    const int m1 = q_scale<CN>(min1, a.param_q), m2 = q_scale<CN>(min2, a.param_q);
    auto second = [&](int w, int nv) {
        const uint32_t qw = E[w];
        uint2 c = {0u, 0u};
        if constexpr (LAYERED) c = cw[w];
        uint32_t rw = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nv) {
                const int q = (int)(int8_t)(qw >> (8 * b));
                const int mag = abs(q) == min1 ? m2 : m1;
                const int R = ((neg ^ ((unsigned)q >> 31)) & 1u) ? -mag : mag;
                rw |= ((uint32_t)R & 0xffu) << (8 * b);
                if constexpr (LAYERED) L[q_col(c, b)] = (int16_t)(q + R);
            }
        }
        E[w] = rw;
    };
    for (int w = 0; w < full; ++w) second(w, 4);
    if (tail) second(full, tail);
    return par;
}

// Whether some row of H has odd parity in b = (L < 0) (this thread's rows).
__device__ __forceinline__ int q_syndrome(const QuantArgs &a, const int16_t *L, int tid, int nt) {
    unsigned bad = 0u;
    for (int r = tid; r < a.g.m && !bad; r += nt) {
        const int2 rw = a.t.row[r];
        const uint2 *cw = reinterpret_cast<const uint2 *>(a.t.col + rw.x);
        unsigned par = 0u;
        for (int w = 0; 4 * w < rw.y; ++w) {
            const uint2 c = cw[w];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * w + b < rw.y) par ^= (unsigned)(int)L[q_col(c, b)] >> 31;
        }
        bad = par;
    }
    return (int)bad;
}

// Outputs and Monte-Carlo counters of frame f: frame_finish (phys_common.h) on
// integer posteriors.  cnt: thread 0's running counts, FrameCounts::v or (to
// spare 14 registers) a copy of it in LDS.
template <bool STATS>
__device__ __forceinline__ void q_frame_finish(const QuantArgs &a, const McStats &ms, int f, int conv, const int16_t *L, int *s_err,
                                               unsigned *s_bins, int tid, int nt, unsigned long long *cnt) {
    const DevGraph &g = a.g;
    const int iters = conv >= 0 ? conv + 1 : a.max_iter;
    for (int j = tid; j < g.n; j += nt) {
        if (a.z_out) a.z_out[(size_t)f * g.n + j] = L[j] < 0 ? 0 : 1;
        if (a.post_out) a.post_out[(size_t)f * g.n + j] = L[j];
    }
    if (tid == 0) {
        if (a.conv_out) a.conv_out[f] = conv;
        if (a.status_out) a.status_out[f] = conv >= 0 ? 0 : 1;
        if (a.iters_out) a.iters_out[f] = iters;
        *s_err = 0;
    }
    if (a.ctr) {
        __syncthreads();
        constexpr bool stats = STATS;  // the statistics compare the converged frames too
        if (conv < 0 || stats) {  // BER counts failed frames only
            const int kw = (g.k + 31) >> 5;
            int my = 0;
            for (int j = tid; j < g.k; j += nt) {
                const uint32_t w = a.ubits[((size_t)(f >> 6) * kw + (j >> 5)) * kTile + (f & 63)];
                my += (((w >> (j & 31)) & 1u) != (L[j] < 0 ? 1u : 0u)) ? 1 : 0;
            }
            atomicAdd(s_err, my);
        }
        __syncthreads();
        if (tid == 0) {
            cnt[0] += 1ull;
            if (conv < 0) {
                cnt[1] += 1ull;
                cnt[2] += (unsigned long long)*s_err;
            } else {
                cnt[3] += (unsigned long long)conv;
                cnt[4] += 1ull;
            }
            cnt[6] += (unsigned long long)iters;
            if constexpr (stats) mc_stats_frame(ms, ms.frame_base + f, conv, *s_err, s_bins);
        }
    }
    __syncthreads();  // LDS reused by the next frame
}

template <int CN, int SCHED, bool STATS>
__global__ __launch_bounds__(512) void phys_quant_kernel(QuantArgs a, McStats ms) {
    constexpr bool kLayered = SCHED == 1;
    extern __shared__ __attribute__((aligned(16))) uint32_t qlds[];
    const DevGraph &g = a.g;
    uint32_t *E = qlds;                                                  // [epad / 4]: int8 messages, rows padded
    int16_t *L = reinterpret_cast<int16_t *>(E + (a.t.epad >> 2));       // [n + 1] (the last: phys_quant_reg_kernel)
    int8_t *Lam = reinterpret_cast<int8_t *>(L + ((g.n + 2) & ~1));      // [n], flooding only
    const int8_t *Eb = reinterpret_cast<const int8_t *>(E);
    __shared__ int s_err;
    unsigned *s_bins = nullptr;
    if constexpr (STATS) {  // static LDS of the statistics instantiation only
        __shared__ unsigned bins[kMcBins];
        s_bins = bins;
    }
    FrameCounts fc;
    const int tid = threadIdx.x, nt = blockDim.x;
    if constexpr (STATS) mc_stats_begin(s_bins, tid);
    for (int f = blockIdx.x; f < a.count; f += gridDim.x) {
        for (int j = tid; j < g.n; j += nt) {
            const int v = q_lambda(a, f, j);
            L[j] = (int16_t)v;
            if constexpr (!kLayered) Lam[j] = (int8_t)v;
        }
        for (int w = tid; w < (a.t.epad >> 2); w += nt) E[w] = 0u;
        __syncthreads();
        int conv = -1;
        if constexpr (kLayered) {
            for (int it = 0; it < a.max_iter; ++it) {
                for (int l = 0; l < a.n_layers; ++l) {
                    const int i1 = a.layer_ptr[l + 1];
                    for (int i = a.layer_ptr[l] + tid; i < i1; i += nt) {
                        const int2 rw = a.t.row[a.layer_rows[i]];
                        q_check_row<CN, true>(a, E + (rw.x >> 2), L, reinterpret_cast<const uint2 *>(a.t.col + rw.x),
                                              rw.y);
                    }
                    __syncthreads();
                }
                if (!__syncthreads_or(q_syndrome(a, L, tid, nt))) {
                    conv = it;
                    break;
                }
            }
        } else {
            for (int it = 0; it < a.max_iter; ++it) {
                // --- check nodes, and the syndrome of the posterior they read
                unsigned bad = 0u;
                for (int r = tid; r < g.m; r += nt) {
                    const int2 rw = a.t.row[r];
                    bad |= q_check_row<CN, false>(a, E + (rw.x >> 2), L,
                                                  reinterpret_cast<const uint2 *>(a.t.col + rw.x), rw.y);
                }
                if (!__syncthreads_or((int)bad) && it > 0) {  // iteration it - 1 left H b = 0
                    conv = it - 1;
                    break;
                }
                // --- variable nodes
                for (int j = tid; j < g.n; j += nt) {
                    int s = Lam[j];
                    for (int p = g.csc_ptr[j]; p < g.csc_ptr[j + 1]; ++p) s += Eb[a.t.csc[p]];
                    L[j] = (int16_t)q_clamp(s, a.pmax);
                }
                __syncthreads();
                // the first iterations and the last check their own posterior
                if ((it < kQEarlySyn || it + 1 == a.max_iter) && !__syncthreads_or(q_syndrome(a, L, tid, nt))) {
                    conv = it;
                    break;
                }
            }
        }
        q_frame_finish<STATS>(a, ms, f, conv, L, &s_err, s_bins, tid, nt, fc.v);
    }
    if (tid == 0) fc.flush(a.ctr);
    if constexpr (STATS) mc_stats_flush(ms, s_bins, tid);
}

// The flooding decoder with every thread's rows and columns fixed for the whole
// launch (row r = tid + k*NT, column j = tid + k*NT) and their LDS addresses
// held in registers as 16-bit pairs, loaded once and reused for every frame:
// no index load in the iteration loop (phys_reg_kernel does the same for
// fp32).  A row's Q words stay in registers between its two sweeps.  The
// padded slots of a row's last dword need no predicate: their column is the
// dummy posterior L[n] = +Qmax and their message byte is kept 0, so their
// Q = Qmax can be neither min1 nor lower min2 (a row has two real edges, each
// |Q| <= Qmax), and their sign is +.  Same integers as phys_quant_kernel.
// RW: dwords of a row (row degree <= 4 RW); CDEG: column degree bound.
constexpr int kQRegNT = 512;

template <int CN, int RPT, int RW, int CPT, int CDEG, bool STATS>
__global__ __launch_bounds__(kQRegNT, 6) void phys_quant_reg_kernel(QuantArgs a, McStats ms) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qlds[];
    const DevGraph &g = a.g;
    char *base = reinterpret_cast<char *>(qlds);  // E at 0, as phys_quant_kernel
    const uint32_t Lb = (uint32_t)a.t.epad;        // L's byte offset
    int16_t *L = reinterpret_cast<int16_t *>(base + Lb);
    int8_t *Lam = reinterpret_cast<int8_t *>(L + ((g.n + 2) & ~1));
    __shared__ int s_err;
    __shared__ unsigned long long s_cnt[7];  // thread 0's FrameCounts
    unsigned *s_bins = nullptr;
    if constexpr (STATS) {  // static LDS of the statistics instantiation only
        __shared__ unsigned bins[kMcBins];
        s_bins = bins;
    }
    const int tid = threadIdx.x;
    if constexpr (STATS) mc_stats_begin(s_bins, tid);
    constexpr int NT = kQRegNT;
    if (tid < 7) s_cnt[tid] = 0ull;
    uint32_t rinfo[RPT];        // byte offset of the row's messages | degree << 16
    uint32_t rc[RPT][2 * RW];   // byte offsets of L[c_e], two to a register
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = tid + k * NT;
        int2 rw = {0, 0};
        if (r < g.m) rw = a.t.row[r];
        rinfo[k] = (uint32_t)rw.x | ((uint32_t)rw.y << 16);
        const uint2 *cw = reinterpret_cast<const uint2 *>(a.t.col + rw.x);
#pragma unroll
        for (int w = 0; w < RW; ++w) {
            uint2 c = {(uint32_t)g.n * 0x10001u, (uint32_t)g.n * 0x10001u};
            if (4 * w < rw.y) c = cw[w];
            rc[k][2 * w] = (Lb * 0x10001u) + 2u * c.x;  // both halves: Lb + 2 col < 65536
            rc[k][2 * w + 1] = (Lb * 0x10001u) + 2u * c.y;
        }
    }
    static_assert(CPT <= 8 && CDEG <= 15, "column degrees are packed four bits each");
    uint32_t cdegs = 0u;         // column k's degree in bits 4k..4k+3
    uint32_t ce[CPT][CDEG / 2];  // byte offsets of the column's messages
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * NT;
        const int p0 = j < g.n ? g.csc_ptr[j] : 0;
        const int cd = j < g.n ? g.csc_ptr[j + 1] - p0 : 0;
        cdegs |= (uint32_t)cd << (4 * k);
#pragma unroll
        for (int i = 0; i < CDEG / 2; ++i) {
            const uint32_t lo = 2 * i < cd ? (uint32_t)a.t.csc[p0 + 2 * i] : 0u;
            const uint32_t hi = 2 * i + 1 < cd ? (uint32_t)a.t.csc[p0 + 2 * i + 1] : 0u;
            ce[k][i] = lo | (hi << 16);
        }
    }
    auto half = [](uint32_t v, int i) -> uint32_t { return (i & 1) ? v >> 16 : v & 0xffffu; };

    for (int f = blockIdx.x; f < a.count; f += gridDim.x) {
        for (int j = tid; j < g.n; j += NT) {
            const int v = q_lambda(a, f, j);
            L[j] = (int16_t)v;
            Lam[j] = (int8_t)v;
        }
        if (tid == 0) L[g.n] = (int16_t)a.qmax;
        for (int w = tid; w < (a.t.epad >> 2); w += NT) qlds[w] = 0u;
        __syncthreads();
        int conv = -1;
        for (int it = 0; it < a.max_iter; ++it) {
            // --- check nodes, and the syndrome of the posterior they read
            uint32_t bad = 0u;
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
                const int deg = (int)(rinfo[k] >> 16);
                if (deg == 0) continue;
                const uint32_t eoff = rinfo[k] & 0xffffu;
                uint32_t qw[RW];
                int min1 = 0x7fff, min2 = 0x7fff;
                uint32_t sx = 0u, lx = 0u;
#pragma unroll
                for (int w = 0; w < RW; ++w) {
                    qw[w] = 0u;
                    if (w == 0 || 4 * w < deg) {
                        const uint32_t ew = *reinterpret_cast<const uint32_t *>(base + eoff + 4 * w);
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int l = *reinterpret_cast<const int16_t *>(base + half(rc[k][2 * w + (b >> 1)], b));
                            const int q = q_clamp(l - (int)(int8_t)(ew >> (8 * b)), a.qmax);
                            const int aq = abs(q);
                            min2 = min(min2, max(min1, aq));
                            min1 = min(min1, aq);
                            sx ^= (uint32_t)q;
                            lx ^= (uint32_t)l;
                            qw[w] |= ((uint32_t)q & 0xffu) << (8 * b);
                        }
                    }
                }
                bad |= lx >> 31;
                const uint32_t neg = sx >> 31;
                const int m1 = q_scale<CN>(min1, a.param_q), m2 = q_scale<CN>(min2, a.param_q);
#pragma unroll
                for (int w = 0; w < RW; ++w) {
                    if (w == 0 || 4 * w < deg) {
                        uint32_t rw = 0u;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int q = (int)(int8_t)(qw[w] >> (8 * b));
                            const int mag = abs(q) == min1 ? m2 : m1;
                            const int R = ((neg ^ ((uint32_t)q >> 31)) & 1u) ? -mag : mag;
                            rw |= ((uint32_t)R & 0xffu) << (8 * b);
                        }
                        const int rem = deg - 4 * w;  // the padded slots keep 0
                        if (rem < 4) rw &= (1u << (8 * rem)) - 1u;
                        *reinterpret_cast<uint32_t *>(base + eoff + 4 * w) = rw;
                    }
                }
            }
            if (!__syncthreads_or((int)bad) && it > 0) {  // iteration it - 1 left H b = 0
                conv = it - 1;
                break;
            }
            // --- variable nodes
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int j = tid + k * NT;
                const int cd = (int)((cdegs >> (4 * k)) & 15u);
                if (j >= g.n) continue;
                int s = Lam[j];
#pragma unroll
                for (int i = 0; i < CDEG; ++i)
                    if (i < cd) s += *reinterpret_cast<const int8_t *>(base + half(ce[k][i >> 1], i));
                L[j] = (int16_t)q_clamp(s, a.pmax);
            }
            __syncthreads();
            // the first iterations and the last check their own posterior (the
            // padded slots read L[n] > 0)
            if (it < kQEarlySyn || it + 1 == a.max_iter) {
                uint32_t lx = 0u;
#pragma unroll
                for (int k = 0; k < RPT; ++k) {
                    const int deg = (int)(rinfo[k] >> 16);
                    uint32_t rx = 0u;
#pragma unroll
                    for (int i = 0; i < 4 * RW; ++i)
                        if (i < 4 || (i & ~3) < deg)
                            rx ^= (uint32_t)(int)*reinterpret_cast<const int16_t *>(base + half(rc[k][i >> 1], i));
                    lx |= rx;
                }
                if (!__syncthreads_or((int)(lx >> 31))) {
                    conv = it;
                    break;
                }
            }
        }
        q_frame_finish<STATS>(a, ms, f, conv, L, &s_err, s_bins, tid, NT, s_cnt);
    }
    if (tid == 0 && a.ctr) {
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (s_cnt[i]) atomicAdd(&a.ctr[i], s_cnt[i]);
    }
    if constexpr (STATS) mc_stats_flush(ms, s_bins, tid);
}

}  // namespace

size_t phys_quant_lds_bytes(const DevGraph &g, int epad, bool layered) {
    return (size_t)epad + (((size_t)g.n * 2 + 2 + 3) & ~(size_t)3) + (layered ? 0 : ((size_t)g.n + 3) & ~(size_t)3);
}

namespace {

// Shapes of phys_quant_reg_kernel: rows per thread, dwords per row, columns
// per thread, column degree bound (512 threads).
struct QRegShape {
    int rpt, rw, cpt, cdeg;
};
// Rows of up to 8 edges only: a {2, 4, 5, 6} shape for the rate-3/4 codes
// (14-15 edges) spilled 51 registers and lost to the generic kernel
// (DESIGN.md).
constexpr QRegShape kQRegShapes[] = {{1, 2, 2, 6}, {3, 2, 5, 6}};

}  // namespace

// The shape phys_quant_reg_kernel runs this graph with, or -1: the generic
// phys_quant_kernel (the layered schedule; a graph no shape covers; addresses
// past 16 bits).  LDPC_PHYS_Q_REG=0 (read per launch) forces the generic
// kernel (tests, A/B).
int phys_quant_reg_shape(const DevGraph &g, int epad, bool layered) {
    if (layered || phys_quant_lds_bytes(g, epad, false) > 65536) return -1;
    if (const char *e = getenv("LDPC_PHYS_Q_REG"))
        if (atoi(e) == 0) return -1;
    int best = -1;
    for (int i = 0; i < (int)(sizeof(kQRegShapes) / sizeof(kQRegShapes[0])); ++i) {
        const QRegShape &q = kQRegShapes[i];
        if (q.rpt * kQRegNT >= g.m && q.cpt * kQRegNT >= g.n && 4 * q.rw >= g.max_row_deg && q.cdeg >= g.max_col_deg &&
            (best < 0 || q.rpt * q.rw * 2 + q.cpt * q.cdeg <
                             kQRegShapes[best].rpt * kQRegShapes[best].rw * 2 + kQRegShapes[best].cpt * kQRegShapes[best].cdeg))
            best = i;
    }
    return best;
}

// LDPC_PHYS_Q_NT=64..512 (a multiple of 64, read per launch) overrides the
// generic kernel's block size (A/B)
int phys_quant_threads(const DevGraph &g, const QuantRule &rule) {
    if (phys_quant_reg_shape(g, rule.tab.epad, rule.layer_ptr != nullptr) >= 0) return kQRegNT;
    if (const char *e = getenv("LDPC_PHYS_Q_NT")) {
        const int nt = atoi(e);
        if (nt >= 64 && nt <= 512 && nt % 64 == 0) return nt;
    }
    if (!rule.layer_ptr) return 256;
    return std::min(256, std::max(64, (rule.max_layer + 63) & ~63));
}

namespace {

// Launch on min(max_grid, CUs x workgroups per CU) workgroups.  Per CU:
// min(32 / waves, LDS limit / frame bytes), as the fp32 kernels' grids.  With
// `resident` no more than the runtime says are resident for this kernel, block
// and LDS size, which counts registers too: the register kernel holds 6 waves
// per SIMD, three workgroups per CU where the rule above says four, and it
// pays its index loads once per workgroup; the fourth bought nothing but a
// second round (wimax_2304_0.5, 1.0 dB: 16.2 -> 14.8 ns per frame-iteration
// without it).  The generic kernel is the other way round: one workgroup more
// than the seven resident evens out frames of unequal length (12.5 against
// 13.3 ns at -2.5 dB), so it keeps the plain rule.
template <typename K>
void launch_quant(K kernel, const QuantArgs &a, const McStats &ms, int nt, size_t lds, int max_grid, bool resident, hipStream_t s) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    int per_cu = (int)std::min<size_t>(32 / (nt / 64), kQLdsLimit / (lds + 64));
    if (resident) {
        int fit = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, nt, lds) == hipSuccess && fit > 0)
            per_cu = std::min(per_cu, fit);
        (void)hipGetLastError();
    }
    const int grid = std::max(1, std::min(max_grid, cus * std::max(1, per_cu)));
    kernel<<<grid, nt, lds, s>>>(a, ms);
}

template <int CN, bool STATS>
void launch_quant_reg(const QuantArgs &a, const McStats &ms, int shape, int max_grid, size_t lds, hipStream_t s) {
    switch (shape) {
    case 0: launch_quant(phys_quant_reg_kernel<CN, 1, 2, 2, 6, STATS>, a, ms, kQRegNT, lds, max_grid, true, s); break;
    default: launch_quant(phys_quant_reg_kernel<CN, 3, 2, 5, 6, STATS>, a, ms, kQRegNT, lds, max_grid, true, s); break;
    }
}

}  // namespace

hipError_t launch_phys_quant(const DevGraph &g, const double *llr, const float *lam, int count, int max_iter,
                             uint8_t *z, int *conv, int *status, int *iters, int16_t *post, const uint32_t *ubits,
                             unsigned long long *ctr, int max_grid, hipStream_t s, const QuantRule &rule,
                             const McStats &ms_in) {
    if (!rule.tab.row || !rule.tab.col || !rule.tab.csc || rule.qbits < 4 || rule.qbits > 8)
        return hipErrorInvalidValue;
    if (rule.cn != kCnNms && rule.cn != kCnOms) return hipErrorInvalidValue;
    const int qmax = (1 << (rule.qbits - 1)) - 1, pmax = (1 << (rule.qbits + 1)) - 1;
    QuantArgs a{g, llr, lam, count, max_iter, z, conv, status, iters, post, ubits, ctr, rule.tab, qmax, pmax,
                rule.param_q, rule.scale, rule.layer_ptr, rule.layer_rows, rule.n_layers};
    const McStats ms = ctr ? ms_in : McStats{};  // ms.hist set: the kernels' statistics instantiations
    if (count <= 0) return hipSuccess;
    const bool layered = rule.layer_ptr != nullptr;
    const size_t lds = phys_quant_lds_bytes(g, rule.tab.epad, layered);
    const int shape = phys_quant_reg_shape(g, rule.tab.epad, layered);
    const int nt = phys_quant_threads(g, rule);
    max_grid = std::min(max_grid, count);
    const bool nms = rule.cn == kCnNms;
    auto go = [&](auto stats) {  // stats: std::true_type for the kernels' statistics instantiations
        constexpr bool S = decltype(stats)::value;
        if (shape >= 0 && nms) launch_quant_reg<kCnNms, S>(a, ms, shape, max_grid, lds, s);
        else if (shape >= 0) launch_quant_reg<kCnOms, S>(a, ms, shape, max_grid, lds, s);
        else if (nms && !layered) launch_quant(phys_quant_kernel<kCnNms, 0, S>, a, ms, nt, lds, max_grid, false, s);
        else if (nms) launch_quant(phys_quant_kernel<kCnNms, 1, S>, a, ms, nt, lds, max_grid, false, s);
        else if (!layered) launch_quant(phys_quant_kernel<kCnOms, 0, S>, a, ms, nt, lds, max_grid, false, s);
        else launch_quant(phys_quant_kernel<kCnOms, 1, S>, a, ms, nt, lds, max_grid, false, s);
    };
    if (ms.hist) go(std::true_type{});
    else go(std::false_type{});
    return hipGetLastError();
}

}  // namespace ldpc
