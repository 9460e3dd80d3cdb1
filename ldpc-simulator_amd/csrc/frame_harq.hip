// frame_harq.hip -- the frame source under a HARQ plan (physical mode only;
// contract: include/ldpc_hip.h "HARQ"), gfx950.  The last stage of
// launch_frames (frame_kernels.hip) when ldpc_harq_set has set a plan: the
// codeword bits are the same (st.ubits, pt.pbits / pt.wpar), sent n_tx times.
//
//   transmission r  the interleaver contract's frame over the E_r positions of
//                   its own column list, with the Philox key seed_r = seed +
//                   r 0x9E3779B97F4A7C15 (mod 2^64) for its noise and fades
//   llr[j]          +0.0, then + llr_r[j] for r ascending over the
//                   transmissions that carry column j: one fp64 addition each
//   never sent      +0.0; shortened (rm.umask): -LDPC_RM_KNOWN_LLR
//
// Three steps in stream order on the fp64 accumulator hq.acc, which has
// DevState::ch's tile layout [tile][n][64]:
//   hipMemsetAsync        every column +0.0
//   frame_harq_acc_kernel one launch per transmission: lane = frame, a block
//                         walks 128 positions' worth of units of one tile as
//                         frame_model_rm_kernel / frame_model_bf_kernel do
//                         (unit_llr: frame_channel_unit.h) and adds each LLR
//                         into its column: a 512-byte load and a 512-byte store
//                         of 64 consecutive frames, whatever order the plan
//                         sends the columns in
//   frame_harq_out_kernel / frame_harq_rows_kernel
//                         every column of the requested form from acc
// A transmission's columns are distinct and the launches are serialised by the
// stream, so the read-modify-write is plain loads and stores: no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "frame_channel_unit.h"
#include "frame_source.h"
#include "spa_device.h"

namespace ldpc {
namespace {

constexpr uint64_t kHarqSeedStep = 0x9E3779B97F4A7C15ull;
constexpr float kKnownLlr = 1.0e4f;  // LDPC_RM_KNOWN_LLR

// acc[col(t)] += llr_r[col(t)] for the E positions of tx; seed is seed_r.
// BF: block fading (MODEL is Rayleigh), block_len positions (BPSK) or symbols a fade.
template <int BPS, int MODEL, int DEMAP, bool BF>
__global__ __launch_bounds__(64) void frame_harq_acc_kernel(DevGraph g, DevState st, PhysTile pt,
                                                          const int32_t *__restrict__ tx, int E,
                                                          double *__restrict__ acc, uint64_t seed, int snr_point,
                                                          double sigma, int64_t frame0, int block_len) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = U::count(E);
    const int per_tile = (units + U::kPerBlock - 1) / U::kPerBlock;
    const int tile = blockIdx.x / per_tile;
    const int i0 = (blockIdx.x % per_tile) * U::kPerBlock;
    const int i1 = min(units, i0 + U::kPerBlock);
    const int lane = threadIdx.x;
    const int64_t F = frame0 + tile * kTile + lane;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lane;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lane;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lane;
    double *At = acc + (size_t)tile * g.n * kTile + lane;
    int Bc = -1;
    double hc = 1.0;
    for (int i = i0; i < i1; ++i) {
        double h[2] = {1.0, 1.0}, llr[U::kBits];
        if constexpr (BF) block_fades<BPS>(seed, F, snr_point, i, block_len, &Bc, &hc, h);
        unit_llr<BPS, MODEL, DEMAP, true, BF>(Ut, Pt, Wt, g.k, E, seed, F, snr_point, i, sigma, llr, tx, h);
#pragma unroll
        for (int t = 0; t < U::kBits; ++t) {
            const int tb = i * U::kBits + t;
            if (tb >= E) break;
            const int j = tx[tb];
            At[j * kTile] = At[j * kTile] + llr[t];
        }
    }
}

// bit j of the info mask clear: a shortened column
__device__ __forceinline__ bool harq_shortened(const uint32_t *__restrict__ umask, int k, int j) {
    return umask && j < k && !((umask[j >> 5] >> (j & 31)) & 1u);
}

// The tile forms from acc: lane = frame, a block walks 128 columns of one tile.
// to_lambda and the lanes past st.count as frame_model_kernel's.
constexpr int kHarqColsPerBlock = 128;
__global__ __launch_bounds__(64) void frame_harq_out_kernel(DevGraph g, DevState st, PhysTile pt,
                                                          const double *__restrict__ acc,
                                                          const uint32_t *__restrict__ umask, int to_lambda) {
    const int per_tile = (g.n + kHarqColsPerBlock - 1) / kHarqColsPerBlock;
    const int tile = blockIdx.x / per_tile;
    const int j0 = (blockIdx.x % per_tile) * kHarqColsPerBlock;
    const int j1 = min(g.n, j0 + kHarqColsPerBlock);
    const int lane = threadIdx.x;
    const bool valid = tile * kTile + lane < st.count;
    const double *At = acc + (size_t)tile * g.n * kTile + lane;
    double *Ct = st.ch + (size_t)tile * g.n * kTile + lane;
    float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    for (int j = j0; j < j1; ++j) {
        const double a = harq_shortened(umask, g.k, j) ? -(double)kKnownLlr : At[j * kTile];
        const double v = valid ? a : 0.0;
        if (to_lambda) {
            Lamt[j * kTile] = -(float)v;
            Lt[j * kTile] = -(float)v;
        } else {
            Ct[j * kTile] = v;
        }
    }
}

// Row-major fp32 Lambda = -llr, [count][n], from acc: a block transposes 64
// columns of one tile through LDS, so that the loads are 64 consecutive frames
// of a column and the stores 64 consecutive columns of a frame.  256 threads:
// wavefront w loads columns j0 + w, j0 + w + 4, ... and stores frames w, w + 4, ...
__global__ __launch_bounds__(256) void frame_harq_rows_kernel(DevGraph g, DevState st, const double *__restrict__ acc,
                                                            const uint32_t *__restrict__ umask,
                                                            float *__restrict__ row_out) {
    __shared__ float sm[kTile][kTile + 1];  // [column][frame], padded: the transposed read is conflict-free
    const int per_tile = (g.n + kTile - 1) / kTile;
    const int tile = blockIdx.x / per_tile;
    const int j0 = (blockIdx.x % per_tile) * kTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *At = acc + (size_t)tile * g.n * kTile + lane;
    for (int c = w; c < kTile; c += 4) {
        const int j = j0 + c;
        if (j >= g.n) break;
        const double a = harq_shortened(umask, g.k, j) ? -(double)kKnownLlr : At[j * kTile];
        sm[c][lane] = -(float)a;
    }
    __syncthreads();
    const int j = j0 + lane;
    if (j >= g.n) return;
    for (int fl = w; fl < kTile; fl += 4) {
        const int f = tile * kTile + fl;
        if (f >= st.count) break;
        row_out[(size_t)f * g.n + j] = sm[lane][fl];
    }
}

template <int BPS, int MODEL, int DEMAP, bool BF>
hipError_t launch_harq_acc(const DevGraph &g, const DevState &st, const PhysTile &pt, const HarqDev &hq, uint64_t seed,
                           int snr_point, double sigma, int64_t frame0, int block_len, hipStream_t s) {
    using U = Unit<BPS>;
    for (int r = 0; r < hq.n_tx; ++r) {
        const int units = U::count(hq.tx_len[r]);
        frame_harq_acc_kernel<BPS, MODEL, DEMAP, BF>
            <<<st.ntiles * ((units + U::kPerBlock - 1) / U::kPerBlock), 64, 0, s>>>(
                g, st, pt, hq.cols + hq.tx_off[r], hq.tx_len[r], hq.acc, seed + (uint64_t)r * kHarqSeedStep, snr_point,
                sigma, frame0, block_len);
    }
    return hipGetLastError();
}

// One bit per axis has one LLR expression: a single instantiation serves both demappers.
template <int MODEL, bool BF>
hipError_t launch_harq_acc_of(const DevGraph &g, const DevState &st, const PhysTile &pt, const HarqDev &hq,
                              uint64_t seed, int snr_point, double sigma, int64_t frame0, const FrameChannel &ch,
                              hipStream_t s) {
    const bool maxlog = ch.demap == kDemapMaxlog;
    const int bl = ch.fade_block;
    switch (ch.bps) {
        case 1: return launch_harq_acc<1, MODEL, 0, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s);
        case 2: return launch_harq_acc<2, MODEL, 0, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s);
        case 4:
            return maxlog ? launch_harq_acc<4, MODEL, 1, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s)
                          : launch_harq_acc<4, MODEL, 0, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s);
        case 6:
            return maxlog ? launch_harq_acc<6, MODEL, 1, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s)
                          : launch_harq_acc<6, MODEL, 0, BF>(g, st, pt, hq, seed, snr_point, sigma, frame0, bl, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_frame_harq(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                             double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                             const RateMatchDev &rm, const HarqDev &hq, hipStream_t s) {
    if (ch.bps < 1 || st.count <= 0 || st.ntiles <= 0) return hipErrorInvalidValue;
    if (hq.n_tx < 1 || hq.n_tx > kHarqMaxTx || !hq.cols || !hq.acc) return hipErrorInvalidValue;
    for (int r = 0; r < hq.n_tx; ++r)
        if (hq.tx_len[r] < 1 || hq.tx_len[r] > g.n || hq.tx_len[r] % ch.bps != 0 || hq.tx_off[r] < 0)
            return hipErrorInvalidValue;
    if (rm.n_short > 0 && !rm.umask) return hipErrorInvalidValue;
    if (out == kFramesRowLambda && !row_out) return hipErrorInvalidValue;
    if (ch.fade_block < 1 || (ch.fade_block > 1 && ch.model != kChRayleigh)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(hq.acc, 0, sizeof(double) * (size_t)st.ntiles * g.n * kTile, s);  // +0.0
    if (e != hipSuccess) return e;
    if (ch.table) {  // a constellation table: frame_constellation.hip's tile form adds into acc
        for (int r = 0; r < hq.n_tx && e == hipSuccess; ++r)
            e = launch_frame_table(g, st, pt, seed + (uint64_t)r * kHarqSeedStep, snr_point, sigma, frame0, out, row_out,
                                   ch, hq.cols + hq.tx_off[r], hq.tx_len[r], hq.acc, s);
    } else if (ch.fade_block > 1)
        e = launch_harq_acc_of<kChRayleigh, true>(g, st, pt, hq, seed, snr_point, sigma, frame0, ch, s);
    else if (ch.model == kChRayleigh)
        e = launch_harq_acc_of<kChRayleigh, false>(g, st, pt, hq, seed, snr_point, sigma, frame0, ch, s);
    else if (ch.model == 1)  // LDPC_CH_AWGN
        e = launch_harq_acc_of<1, false>(g, st, pt, hq, seed, snr_point, sigma, frame0, ch, s);
    else
        e = hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    const uint32_t *umask = rm.n_short > 0 ? rm.umask : nullptr;
    if (out == kFramesRowLambda)
        frame_harq_rows_kernel<<<st.ntiles * ((g.n + kTile - 1) / kTile), 256, 0, s>>>(g, st, hq.acc, umask, row_out);
    else
        frame_harq_out_kernel<<<st.ntiles * ((g.n + kHarqColsPerBlock - 1) / kHarqColsPerBlock), 64, 0, s>>>(
            g, st, pt, hq.acc, umask, out == kFramesTileLambda ? 1 : 0);
    return hipGetLastError();
}

}  // namespace ldpc
