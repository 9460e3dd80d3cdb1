// frame_channel_models.hip -- the frame source's channel models (physical mode
// only; contract: include/ldpc_hip.h "channel models"), gfx950.  The last stage
// of launch_frames (frame_kernels.hip) when a channel other than the reference's
// is set: the codeword bits are the same (st.ubits, pt.pbits / pt.wpar), the
// symbols, the noise scale and the LLRs are the textbook ones.
//
//   sigma     noise standard deviation per real dimension at unit average symbol
//             energy: N0 = 2 sigma^2, Es/N0 = 1 / (2 sigma^2)
//   BPSK      real, x = +-1, bit j takes noise_pair(j >> 1)[j & 1] as the
//             reference channel does
//   QPSK, 16-QAM, 64-QAM   square, Gray mapped per axis: symbol s carries bits
//             s bps .. s bps + bps - 1, the first half on I, the rest on Q;
//             noise_pair(s) = (I, Q)
//   Rayleigh  h = sqrt(-log u), u from fade_uniforms (frame_source.h), one fade
//             per symbol (BPSK: per bit), known to the receiver; AWGN: h = 1
//   per axis  r = h x + sigma g,  mu_i = (r - h x_i)^2 / (2 sigma^2) over the
//             2^(bps/2) levels x_i = (2 i - (2^m - 1)) d, Gray label i ^ (i >> 1)
//   exact     llr_t = LSE_{a_t(i) = 1}(-mu_i) - LSE_{a_t(i) = 0}(-mu_i), each LSE
//             with its own maximum taken out first
//   max-log   llr_t = min_{a_t = 0} mu_i - min_{a_t = 1} mu_i
//   one bit per axis (BPSK, QPSK): 2 h d r / sigma^2 for either demapper
// All fp64; llr > 0 means bit 1; the decoders get Lambda = -(float)llr.
//
// A "unit" is what one Philox noise block serves: a symbol, or for BPSK the two
// bits 2i, 2i+1.  Two forms, as frame_kernels.hip's:
//   frame_model_kernel      lane = frame, a block walks 128 bits' worth of units
//                           of one tile; every store is 64 consecutive frames
//   frame_model_row_kernel  one wavefront per (frame, 64 units), lane = unit,
//                           each lane writes its unit's consecutive fp32 Lambda
// Both are bound by the fp64 log / sincospi / exp of a unit, not by their
// stores; 64 threads per block as the reference kernels, so that a small chunk
// still spreads over the chip.
//
// Under a rate-matching pattern (ldpc_rate_match_set) the same two forms run as
// frame_model_rm_kernel / frame_model_rm_row_kernel over the E transmitted bits,
// frame_fill_kernel / frame_fill_row_kernel write the columns not sent, and
// frame_shorten_kernel clears the shortened info bits ahead of the parity stage.
// A bit interleaver (ldpc_interleaver_set) is those kernels with a permuted
// tx_col; alone it has nothing to fill.  Rayleigh with a coherence length
// (ldpc_fading_set) is frame_model_bf_kernel / frame_model_bf_row_kernel.
// Under a constellation table (ldpc_constellation_set, ch.table) none of these
// runs: the launchers at the end hand over to frame_constellation.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "frame_channel_unit.h"
#include "frame_source.h"
#include "spa_device.h"

namespace ldpc {
namespace {

// axis_llr, Unit, unit_llr, block_fade and block_fades: frame_channel_unit.h
// (frame_harq.hip runs the same arithmetic per transmission).

// to_lambda: the tile decoders' fp32 Lambda = L = -llr (kFramesTileLambda), else
// the fp64 channel LLRs ch (kFramesCh).  Lanes past st.count write zeros.
template <int BPS, int MODEL, int DEMAP>
__global__ __launch_bounds__(64) void frame_model_kernel(DevGraph g, DevState st, PhysTile pt, uint64_t seed,
                                                       int snr_point, double sigma, int64_t frame0, int to_lambda) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = U::count(g.n);
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
    double *Ct = st.ch + (size_t)tile * g.n * kTile + lane;
    float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    for (int i = i0; i < i1; ++i) {
        double llr[U::kBits];
        unit_llr<BPS, MODEL, DEMAP>(Ut, Pt, Wt, g.k, g.n, seed, F, snr_point, i, sigma, llr);
#pragma unroll
        for (int t = 0; t < U::kBits; ++t) {
            const int j = i * U::kBits + t;
            if (j >= g.n) break;
            const double v = valid ? llr[t] : 0.0;
            if (to_lambda) {
                Lamt[j * kTile] = -(float)v;
                Lt[j * kTile] = -(float)v;
            } else {
                Ct[j * kTile] = v;
            }
        }
    }
}

// Row-major fp32 Lambda = -llr, [count][n] (kFramesRowLambda).
template <int BPS, int MODEL, int DEMAP>
__global__ __launch_bounds__(64) void frame_model_row_kernel(DevGraph g, DevState st, PhysTile pt, uint64_t seed,
                                                           int snr_point, double sigma, int64_t frame0,
                                                           float *__restrict__ row_out) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = U::count(g.n);
    const int per_frame = (units + 63) >> 6;
    const int f = blockIdx.x / per_frame;
    const int i = (blockIdx.x % per_frame) * 64 + threadIdx.x;
    if (f >= st.count || i >= units) return;
    const int tile = f >> 6, lf = f & 63;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lf;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lf;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lf;
    double llr[U::kBits];
    unit_llr<BPS, MODEL, DEMAP>(Ut, Pt, Wt, g.k, g.n, seed, frame0 + f, snr_point, i, sigma, llr);
    float *row = row_out + (size_t)f * g.n;
#pragma unroll
    for (int t = 0; t < U::kBits; ++t) {
        const int j = i * U::kBits + t;
        if (j >= g.n) break;
        row[j] = -(float)llr[t];
    }
}

// ------------------------------------------------------------ rate matching
// The two forms above under a rate-matching pattern (include/ldpc_hip.h "rate
// matching"): instantiations of their own, so that without a pattern the
// kernels above run exactly as they always did.  Units run over the E
// transmitted bits; bit t of the sequence is column rm.tx_col[t] (a wave-uniform
// load in the tile form, a per-lane gather in the row form), read from and
// written to that column.  The columns not sent are frame_fill_*_kernel's.
template <int BPS, int MODEL, int DEMAP>
__global__ __launch_bounds__(64) void frame_model_rm_kernel(DevGraph g, DevState st, PhysTile pt, RateMatchDev rm,
                                                          uint64_t seed, int snr_point, double sigma, int64_t frame0,
                                                          int to_lambda) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = U::count(rm.E);
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
    double *Ct = st.ch + (size_t)tile * g.n * kTile + lane;
    float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    for (int i = i0; i < i1; ++i) {
        double llr[U::kBits];
        unit_llr<BPS, MODEL, DEMAP, true>(Ut, Pt, Wt, g.k, rm.E, seed, F, snr_point, i, sigma, llr, rm.tx_col);
#pragma unroll
        for (int t = 0; t < U::kBits; ++t) {
            const int tb = i * U::kBits + t;
            if (tb >= rm.E) break;
            const int j = rm.tx_col[tb];
            const double v = valid ? llr[t] : 0.0;
            if (to_lambda) {
                Lamt[j * kTile] = -(float)v;
                Lt[j * kTile] = -(float)v;
            } else {
                Ct[j * kTile] = v;
            }
        }
    }
}

template <int BPS, int MODEL, int DEMAP>
__global__ __launch_bounds__(64) void frame_model_rm_row_kernel(DevGraph g, DevState st, PhysTile pt, RateMatchDev rm,
                                                              uint64_t seed, int snr_point, double sigma,
                                                              int64_t frame0, float *__restrict__ row_out) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int units = U::count(rm.E);
    const int per_frame = (units + 63) >> 6;
    const int f = blockIdx.x / per_frame;
    const int i = (blockIdx.x % per_frame) * 64 + threadIdx.x;
    if (f >= st.count || i >= units) return;
    const int tile = f >> 6, lf = f & 63;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lf;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lf;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lf;
    double llr[U::kBits];
    unit_llr<BPS, MODEL, DEMAP, true>(Ut, Pt, Wt, g.k, rm.E, seed, frame0 + f, snr_point, i, sigma, llr, rm.tx_col);
    float *row = row_out + (size_t)f * g.n;
#pragma unroll
    for (int t = 0; t < U::kBits; ++t) {
        const int tb = i * U::kBits + t;
        if (tb >= rm.E) break;
        row[rm.tx_col[tb]] = -(float)llr[t];
    }
}

// ------------------------------------------------------------ block fading
// Rayleigh with a coherence length (include/ldpc_hip.h "bit interleaver and
// block fading", ch.fade_block > 1): instantiations of their own again, so that
// with a fade per symbol the kernels above run exactly as they always did.  RM
// as unit_llr's: the E positions of rm.tx_col, else the n columns in
// order (rm is not read).  The tile form's workgroup walks consecutive units,
// so it takes log and sqrt once per fading block it meets (a wave-uniform
// branch: lanes are frames); a lane of the row form has one unit and one or
// two fades.
template <int BPS, int DEMAP, bool RM>
__global__ __launch_bounds__(64) void frame_model_bf_kernel(DevGraph g, DevState st, PhysTile pt, RateMatchDev rm,
                                                          uint64_t seed, int snr_point, double sigma, int64_t frame0,
                                                          int to_lambda, int block_len) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int nbits = RM ? rm.E : g.n;
    const int units = U::count(nbits);
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
    double *Ct = st.ch + (size_t)tile * g.n * kTile + lane;
    float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    int Bc = -1;
    double hc = 1.0;
    for (int i = i0; i < i1; ++i) {
        double h[2], llr[U::kBits];
        block_fades<BPS>(seed, F, snr_point, i, block_len, &Bc, &hc, h);
        unit_llr<BPS, kChRayleigh, DEMAP, RM, true>(Ut, Pt, Wt, g.k, nbits, seed, F, snr_point, i, sigma, llr, rm.tx_col,
                                                    h);
#pragma unroll
        for (int t = 0; t < U::kBits; ++t) {
            const int tb = i * U::kBits + t;
            if (tb >= nbits) break;
            const int j = RM ? rm.tx_col[tb] : tb;
            const double v = valid ? llr[t] : 0.0;
            if (to_lambda) {
                Lamt[j * kTile] = -(float)v;
                Lt[j * kTile] = -(float)v;
            } else {
                Ct[j * kTile] = v;
            }
        }
    }
}

template <int BPS, int DEMAP, bool RM>
__global__ __launch_bounds__(64) void frame_model_bf_row_kernel(DevGraph g, DevState st, PhysTile pt, RateMatchDev rm,
                                                              uint64_t seed, int snr_point, double sigma,
                                                              int64_t frame0, float *__restrict__ row_out,
                                                              int block_len) {
    using U = Unit<BPS>;
    const int kw = (g.k + 31) >> 5;
    const int mw = (g.m + 31) >> 5;
    const int mw32 = (mw + 31) >> 5;
    const int nbits = RM ? rm.E : g.n;
    const int units = U::count(nbits);
    const int per_frame = (units + 63) >> 6;
    const int f = blockIdx.x / per_frame;
    const int i = (blockIdx.x % per_frame) * 64 + threadIdx.x;
    if (f >= st.count || i >= units) return;
    const int tile = f >> 6, lf = f & 63;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lf;
    const uint32_t *Pt = pt.pbits + (size_t)tile * mw * kTile + lf;
    const uint32_t *Wt = pt.wpar + (size_t)tile * mw32 * kTile + lf;
    int Bc = -1;
    double hc = 1.0;
    double h[2], llr[U::kBits];
    block_fades<BPS>(seed, frame0 + f, snr_point, i, block_len, &Bc, &hc, h);
    unit_llr<BPS, kChRayleigh, DEMAP, RM, true>(Ut, Pt, Wt, g.k, nbits, seed, frame0 + f, snr_point, i, sigma, llr,
                                                rm.tx_col, h);
    float *row = row_out + (size_t)f * g.n;
#pragma unroll
    for (int t = 0; t < U::kBits; ++t) {
        const int tb = i * U::kBits + t;
        if (tb >= nbits) break;
        row[RM ? rm.tx_col[tb] : tb] = -(float)llr[t];
    }
}

// The columns a pattern does not send, tile forms: lane = frame, a block walks
// up to 128 of them; every store is 64 consecutive frames.  The value is the
// column's LLR (+0.0 punctured, -LDPC_RM_KNOWN_LLR shortened), through the same
// expressions as a transmitted column's; lanes past st.count write zeros.
constexpr int kFillPerBlock = 128;
__global__ __launch_bounds__(64) void frame_fill_kernel(DevGraph g, DevState st, PhysTile pt, RateMatchDev rm,
                                                      int to_lambda) {
    const int per_tile = (rm.n_fill + kFillPerBlock - 1) / kFillPerBlock;
    const int tile = blockIdx.x / per_tile;
    const int c0 = (blockIdx.x % per_tile) * kFillPerBlock;
    const int c1 = min(rm.n_fill, c0 + kFillPerBlock);
    const int lane = threadIdx.x;
    const bool valid = tile * kTile + lane < st.count;
    double *Ct = st.ch + (size_t)tile * g.n * kTile + lane;
    float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    for (int c = c0; c < c1; ++c) {
        const int j = rm.fill_col[c];
        const double v = valid ? (double)rm.fill_llr[c] : 0.0;
        if (to_lambda) {
            Lamt[j * kTile] = -(float)v;
            Lt[j * kTile] = -(float)v;
        } else {
            Ct[j * kTile] = v;
        }
    }
}

// The same for the rows: one thread per (frame, column not sent).
__global__ __launch_bounds__(64) void frame_fill_row_kernel(DevGraph g, DevState st, RateMatchDev rm,
                                                          float *__restrict__ row_out) {
    const int per_frame = (rm.n_fill + 63) >> 6;
    const int f = blockIdx.x / per_frame;
    const int c = (blockIdx.x % per_frame) * 64 + threadIdx.x;
    if (f >= st.count || c >= rm.n_fill) return;
    row_out[(size_t)f * g.n + rm.fill_col[c]] = -(float)(double)rm.fill_llr[c];
}

// st.ubits &= umask: lane = frame, a block takes up to 16 of the kw words.
constexpr int kShortenWords = 16;
__global__ __launch_bounds__(64) void frame_shorten_kernel(DevGraph g, DevState st, RateMatchDev rm) {
    const int kw = (g.k + 31) >> 5;
    const int per_tile = (kw + kShortenWords - 1) / kShortenWords;
    const int tile = blockIdx.x / per_tile;
    const int w0 = (blockIdx.x % per_tile) * kShortenWords;
    const int w1 = min(kw, w0 + kShortenWords);
    uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + threadIdx.x;
    for (int w = w0; w < w1; ++w) {
        const uint32_t mask = rm.umask[w];
        if (mask != 0xFFFFFFFFu) Ut[w * kTile] &= mask;
    }
}

// The columns not sent, after the transmitted ones; an interleaver without a
// pattern has none (n_fill == 0) and launches nothing.
hipError_t launch_fill(const DevGraph &g, const DevState &st, const PhysTile &pt, const RateMatchDev &rm, FramesOut out,
                       float *row_out, hipStream_t s) {
    if (rm.n_fill > 0) {
        if (out == kFramesRowLambda)
            frame_fill_row_kernel<<<st.count * ((rm.n_fill + 63) >> 6), 64, 0, s>>>(g, st, rm, row_out);
        else
            frame_fill_kernel<<<st.ntiles * ((rm.n_fill + kFillPerBlock - 1) / kFillPerBlock), 64, 0, s>>>(
                g, st, pt, rm, out == kFramesTileLambda ? 1 : 0);
    }
    return hipGetLastError();
}

template <int BPS, int MODEL, int DEMAP>
hipError_t launch_model_rm(const DevGraph &g, const DevState &st, const PhysTile &pt, const RateMatchDev &rm,
                           uint64_t seed, int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                           hipStream_t s) {
    using U = Unit<BPS>;
    const int units = U::count(rm.E);
    if (out == kFramesRowLambda) {
        frame_model_rm_row_kernel<BPS, MODEL, DEMAP><<<st.count * ((units + 63) >> 6), 64, 0, s>>>(
            g, st, pt, rm, seed, snr_point, sigma, frame0, row_out);
    } else {
        const int to_lambda = out == kFramesTileLambda ? 1 : 0;
        frame_model_rm_kernel<BPS, MODEL, DEMAP>
            <<<st.ntiles * ((units + U::kPerBlock - 1) / U::kPerBlock), 64, 0, s>>>(g, st, pt, rm, seed, snr_point,
                                                                                  sigma, frame0, to_lambda);
    }
    return launch_fill(g, st, pt, rm, out, row_out, s);
}

// Rayleigh with ch.fade_block > 1; rm.E > 0: under a pattern and / or an interleaver.
template <int BPS, int DEMAP, bool RM>
hipError_t launch_model_bf(const DevGraph &g, const DevState &st, const PhysTile &pt, const RateMatchDev &rm,
                           uint64_t seed, int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                           int block_len, hipStream_t s) {
    using U = Unit<BPS>;
    const int units = U::count(RM ? rm.E : g.n);
    if (out == kFramesRowLambda)
        frame_model_bf_row_kernel<BPS, DEMAP, RM><<<st.count * ((units + 63) >> 6), 64, 0, s>>>(
            g, st, pt, rm, seed, snr_point, sigma, frame0, row_out, block_len);
    else
        frame_model_bf_kernel<BPS, DEMAP, RM><<<st.ntiles * ((units + U::kPerBlock - 1) / U::kPerBlock), 64, 0, s>>>(
            g, st, pt, rm, seed, snr_point, sigma, frame0, out == kFramesTileLambda ? 1 : 0, block_len);
    return RM ? launch_fill(g, st, pt, rm, out, row_out, s) : hipGetLastError();
}

template <bool RM>
hipError_t launch_model_bf_of(const DevGraph &g, const DevState &st, const PhysTile &pt, const RateMatchDev &rm,
                              uint64_t seed, int snr_point, double sigma, int64_t frame0, FramesOut out,
                              float *row_out, const FrameChannel &ch, hipStream_t s) {
    const bool maxlog = ch.demap == kDemapMaxlog;
    const int bl = ch.fade_block;
    switch (ch.bps) {
        case 1: return launch_model_bf<1, 0, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s);
        case 2: return launch_model_bf<2, 0, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s);
        case 4:
            return maxlog ? launch_model_bf<4, 1, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s)
                          : launch_model_bf<4, 0, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s);
        case 6:
            return maxlog ? launch_model_bf<6, 1, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s)
                          : launch_model_bf<6, 0, RM>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, bl, s);
        default: return hipErrorInvalidValue;
    }
}

template <int MODEL>
hipError_t launch_model_rm_of(const DevGraph &g, const DevState &st, const PhysTile &pt, const RateMatchDev &rm,
                              uint64_t seed, int snr_point, double sigma, int64_t frame0, FramesOut out,
                              float *row_out, const FrameChannel &ch, hipStream_t s) {
    const bool maxlog = ch.demap == kDemapMaxlog;
    switch (ch.bps) {
        case 1: return launch_model_rm<1, MODEL, 0>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s);
        case 2: return launch_model_rm<2, MODEL, 0>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s);
        case 4:
            return maxlog ? launch_model_rm<4, MODEL, 1>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s)
                          : launch_model_rm<4, MODEL, 0>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s);
        case 6:
            return maxlog ? launch_model_rm<6, MODEL, 1>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s)
                          : launch_model_rm<6, MODEL, 0>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, s);
        default: return hipErrorInvalidValue;
    }
}

template <int BPS, int MODEL, int DEMAP>
hipError_t launch_model(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                        double sigma, int64_t frame0, FramesOut out, float *row_out, hipStream_t s) {
    using U = Unit<BPS>;
    const int units = U::count(g.n);
    if (out == kFramesRowLambda)
        frame_model_row_kernel<BPS, MODEL, DEMAP><<<st.count * ((units + 63) >> 6), 64, 0, s>>>(
            g, st, pt, seed, snr_point, sigma, frame0, row_out);
    else
        frame_model_kernel<BPS, MODEL, DEMAP><<<st.ntiles * ((units + U::kPerBlock - 1) / U::kPerBlock), 64, 0, s>>>(
            g, st, pt, seed, snr_point, sigma, frame0, out == kFramesTileLambda ? 1 : 0);
    return hipGetLastError();
}

// One bit per axis has one LLR expression: a single instantiation serves both demappers.
template <int MODEL>
hipError_t launch_model_of(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                           double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                           hipStream_t s) {
    const bool maxlog = ch.demap == kDemapMaxlog;
    switch (ch.bps) {
        case 1: return launch_model<1, MODEL, 0>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s);
        case 2: return launch_model<2, MODEL, 0>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s);
        case 4:
            return maxlog ? launch_model<4, MODEL, 1>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s)
                          : launch_model<4, MODEL, 0>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s);
        case 6:
            return maxlog ? launch_model<6, MODEL, 1>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s)
                          : launch_model<6, MODEL, 0>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_frame_channel_model(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed,
                                      int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                                      const FrameChannel &ch, hipStream_t s) {
    if (ch.bps < 1 || g.n % ch.bps != 0 || st.count <= 0) return hipErrorInvalidValue;
    if (ch.fade_block < 1 || (ch.fade_block > 1 && ch.model != kChRayleigh)) return hipErrorInvalidValue;
    if (ch.table)  // a constellation table: frame_constellation.hip
        return launch_frame_table(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, nullptr, g.n, nullptr, s);
    if (ch.fade_block > 1)
        return launch_model_bf_of<false>(g, st, pt, RateMatchDev{}, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    if (ch.model == kChRayleigh)
        return launch_model_of<kChRayleigh>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    if (ch.model == 1)  // LDPC_CH_AWGN
        return launch_model_of<1>(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    return hipErrorInvalidValue;
}

hipError_t launch_frame_channel_model_rm(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed,
                                         int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                                         const FrameChannel &ch, const RateMatchDev &rm, hipStream_t s) {
    if (ch.bps < 1 || st.count <= 0) return hipErrorInvalidValue;
    // n_fill == 0: a bit interleaver without a pattern (no fill kernel runs)
    if (rm.n_fill < 0 || rm.E < 1 || rm.E + rm.n_fill != g.n || rm.E % ch.bps != 0 || !rm.tx_col ||
        (rm.n_fill > 0 && (!rm.fill_col || !rm.fill_llr)))
        return hipErrorInvalidValue;
    if (ch.fade_block < 1 || (ch.fade_block > 1 && ch.model != kChRayleigh)) return hipErrorInvalidValue;
    if (ch.table) {  // a constellation table: frame_constellation.hip
        const hipError_t e =
            launch_frame_table(g, st, pt, seed, snr_point, sigma, frame0, out, row_out, ch, rm.tx_col, rm.E, nullptr, s);
        return e != hipSuccess ? e : launch_fill(g, st, pt, rm, out, row_out, s);
    }
    if (ch.fade_block > 1)
        return launch_model_bf_of<true>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    if (ch.model == kChRayleigh)
        return launch_model_rm_of<kChRayleigh>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    if (ch.model == 1)  // LDPC_CH_AWGN
        return launch_model_rm_of<1>(g, st, pt, rm, seed, snr_point, sigma, frame0, out, row_out, ch, s);
    return hipErrorInvalidValue;
}

hipError_t launch_frame_shorten(const DevGraph &g, const DevState &st, const RateMatchDev &rm, hipStream_t s) {
    const int kw = (g.k + 31) >> 5;
    if (kw < 1 || !rm.umask || st.ntiles <= 0) return hipErrorInvalidValue;
    frame_shorten_kernel<<<st.ntiles * ((kw + kShortenWords - 1) / kShortenWords), 64, 0, s>>>(g, st, rm);
    return hipGetLastError();
}

}  // namespace ldpc
