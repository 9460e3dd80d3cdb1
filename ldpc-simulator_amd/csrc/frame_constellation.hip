// frame_constellation.hip -- the frame source's channel models over a
// constellation table (physical mode only; contract: include/ldpc_hip.h
// "constellations"), gfx950.  What frame_channel_models.hip and frame_harq.hip
// launch in place of their per-axis kernels when ldpc_constellation_set has set
// a table: the codeword bits, the noise pairs and the fades are the same, the
// symbol is one of 2^bps complex points and the demapper runs over all of them.
//
//   symbol s   positions s bps .. s bps + bps - 1 of the transmitted sequence,
//              label a = the bits, first bit most significant, x = points[a]
//   r          h x + sigma (g0 + i g1), noise_pair(s) = (g0, g1); Rayleigh:
//              h = block_fade(s / block_len) (block_len 1: a fade per symbol)
//   mu_i       |r - h x_i|^2 / (2 sigma^2) over all 2^bps points
//   exact, max-log   as frame_channel_models.hip's, over the points (table_llr,
//              frame_channel_unit.h)
//
// The same two forms as frame_channel_models.hip, 64 threads a block:
//   frame_table_kernel      lane = frame, a block walks floor(128 / bps) symbols
//                           of one tile; every store is 64 consecutive frames.
//                           Writes st.ch, or pt.Lam and pt.L, or adds into a
//                           HARQ accumulator (frame_harq_acc_kernel's step).
//   frame_table_row_kernel  one wavefront per (frame, 64 symbols), lane = symbol
// A kernel is templated on bps and the demapper only.  The channel model, the
// column list of a pattern, an interleaver or a HARQ transmission (tx) and the
// coherence length are arguments: they are uniform across the grid, and next
// to a symbol's 2^bps fp64 exponentials and its Philox block a scalar branch
// costs nothing, while each as a template parameter would multiply the 24
// kernels here by twelve.  The table is a kernel argument of 2^(bps+4) bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "frame_channel_unit.h"
#include "frame_source.h"
#include "spa_device.h"

namespace ldpc {
namespace {

enum TableSink { kSinkCh = 0, kSinkLambda = 1, kSinkAcc = 2 };

// llr[0 .. BPS) of symbol i of frame F.  {*Bc, *hc}: the caller's last fading
// index and its fade, as block_fades'.
template <int BPS, int DEMAP>
__device__ __forceinline__ void table_symbol(const TablePoints<BPS> &tab, const uint32_t *Ut, const uint32_t *Pt,
                                             const uint32_t *Wt, int k, const int32_t *__restrict__ tx, int model,
                                             int block_len, uint64_t seed, int64_t F, int snr_point, int i,
                                             double sigma, int *Bc, double *hc, double *llr) {
    double g[2];
    noise_pair(seed, F, snr_point, i, g);
    double h = 1.0;
    if (model == kChRayleigh) {
        const int B = i / block_len;
        if (B != *Bc) {
            *Bc = B;
            *hc = block_fade(seed, F, snr_point, B);
        }
        h = *hc;
    }
    table_llr<BPS, DEMAP>(tab, table_label<BPS>(Ut, Pt, Wt, k, i, tx), h, sigma, g, llr);
}

// E positions (tx: their columns; null: E = n columns in order).  sink kSinkCh /
// kSinkLambda: lanes past st.count write zeros; kSinkAcc: acc[col] += llr.
template <int BPS, int DEMAP>
__global__ __launch_bounds__(64) void frame_table_kernel(DevGraph g, DevState st, PhysTile pt, TablePoints<BPS> tab,
                                                       const int32_t *__restrict__ tx, int E, int model,
                                                       int block_len, uint64_t seed, int snr_point, double sigma,
                                                       int64_t frame0, int sink, double *__restrict__ acc) {
    using U = TableUnit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = E / BPS;
    const int per_tile = (units + U::kPerBlock - 1) / U::kPerBlock;
    const int tile = blockIdx.x / per_tile;
    const int i0 = (blockIdx.x % per_tile) * U::kPerBlock;
    const int i1 = min(units, i0 + U::kPerBlock);
    const int lane = threadIdx.x;
    const int f = tile * kTile + lane;
    const bool valid = f < st.count;
    const int64_t F = frame0 + f;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lane;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lane;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lane;
    const size_t base = (size_t)tile * g.n * kTile + lane;
    int Bc = -1;
    double hc = 1.0;
    for (int i = i0; i < i1; ++i) {
        double llr[BPS];
        table_symbol<BPS, DEMAP>(tab, Ut, Pt, Wt, g.k, tx, model, block_len, seed, F, snr_point, i, sigma, &Bc, &hc,
                                 llr);
#pragma unroll
        for (int t = 0; t < BPS; ++t) {
            const int tb = i * BPS + t;
            const size_t o = base + (size_t)(tx ? tx[tb] : tb) * kTile;
            const double v = valid ? llr[t] : 0.0;
            if (sink == kSinkAcc) {
                acc[o] = acc[o] + llr[t];
            } else if (sink == kSinkLambda) {
                pt.Lam[o] = -(float)v;
                pt.L[o] = -(float)v;
            } else {
                st.ch[o] = v;
            }
        }
    }
}

// Row-major fp32 Lambda = -llr, [count][n] (kFramesRowLambda).
template <int BPS, int DEMAP>
__global__ __launch_bounds__(64) void frame_table_row_kernel(DevGraph g, DevState st, PhysTile pt, TablePoints<BPS> tab,
                                                           const int32_t *__restrict__ tx, int E, int model,
                                                           int block_len, uint64_t seed, int snr_point, double sigma,
                                                           int64_t frame0, float *__restrict__ row_out) {
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = E / BPS;
    const int per_frame = (units + 63) >> 6;
    const int f = blockIdx.x / per_frame;
    const int i = (blockIdx.x % per_frame) * 64 + threadIdx.x;
    if (f >= st.count || i >= units) return;
    const int tile = f >> 6, lf = f & 63;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lf;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lf;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lf;
    int Bc = -1;
    double hc = 1.0, llr[BPS];
    table_symbol<BPS, DEMAP>(tab, Ut, Pt, Wt, g.k, tx, model, block_len, seed, frame0 + f, snr_point, i, sigma, &Bc,
                             &hc, llr);
    float *row = row_out + (size_t)f * g.n;
#pragma unroll
    for (int t = 0; t < BPS; ++t) {
        const int tb = i * BPS + t;
        row[tx ? tx[tb] : tb] = -(float)llr[t];
    }
}

template <int BPS, int DEMAP>
hipError_t launch_table(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                        double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                        const int32_t *tx, int E, double *acc, hipStream_t s) {
    TablePoints<BPS> tab;
    std::copy(ch.table, ch.table + (2 << BPS), tab.xy);
    const int units = E / BPS;
    if (!acc && out == kFramesRowLambda) {
        frame_table_row_kernel<BPS, DEMAP><<<st.count * ((units + 63) >> 6), 64, 0, s>>>(
            g, st, pt, tab, tx, E, ch.model, ch.fade_block, seed, snr_point, sigma, frame0, row_out);
    } else {
        constexpr int per = TableUnit<BPS>::kPerBlock;
        const int sink = acc ? kSinkAcc : out == kFramesTileLambda ? kSinkLambda : kSinkCh;
        frame_table_kernel<BPS, DEMAP><<<st.ntiles * ((units + per - 1) / per), 64, 0, s>>>(
            g, st, pt, tab, tx, E, ch.model, ch.fade_block, seed, snr_point, sigma, frame0, sink, acc);
    }
    return hipGetLastError();
}

template <int BPS>
hipError_t launch_table_of(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                           double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                           const int32_t *tx, int E, double *acc, hipStream_t s) {
    return ch.demap == kDemapMaxlog
               ? launch_table<BPS, 1>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s)
               : launch_table<BPS, 0>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
}

}  // namespace

hipError_t launch_frame_table(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                              double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                              const int32_t *tx, int E, double *acc, hipStream_t s) {
    if (!ch.table || ch.bps < 1 || ch.bps > 6 || st.count <= 0 || st.ntiles <= 0) return hipErrorInvalidValue;
    if (ch.model != 1 && ch.model != kChRayleigh) return hipErrorInvalidValue;  // LDPC_CH_AWGN
    if (ch.fade_block < 1 || (ch.fade_block > 1 && ch.model != kChRayleigh)) return hipErrorInvalidValue;
    if (!tx) E = g.n;
    if (E < 1 || E > g.n || E % ch.bps != 0) return hipErrorInvalidValue;
    if (!acc && out == kFramesRowLambda && !row_out) return hipErrorInvalidValue;
    switch (ch.bps) {
        case 1: return launch_table_of<1>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
        case 2: return launch_table_of<2>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
        case 3: return launch_table_of<3>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
        case 4: return launch_table_of<4>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
        case 5: return launch_table_of<5>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
        default: return launch_table_of<6>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, tx, E, acc, s);
    }
}

}  // namespace ldpc
