// phys_common.h -- what the LDS-resident physical-mode kernels share
// (phys_kernels.hip: flooding; phys_layered.hip: layered min-sum;
// phys_bitflip.hip: bit flipping): the kernel
// arguments, a frame's load into LDS, its outputs and Monte-Carlo counters, and
// the min-sum check rule (also used by phys_tile.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spa_device.h"

namespace ldpc {

struct PhysArgs {
    DevGraph g;               // H[:, perm] (sparse)
    const double *llr;        // [count][n] (layout 0) or ch tile layout (layout 1)
    const float *lam;         // layout 2: [count][n] fp32 Lambda (on-device frames, frame_kernels.hip)
    int layout;               // 0: row per frame; 1: [tile][n][64]; 2: lam
    int count;
    int max_iter;
    uint8_t *z_out;           // [count][n] or null: z = (bit estimate) ^ 1
    int *conv_out;            // [count] or null
    int *status_out;          // [count] or null
    int *iters_out;           // [count] or null
    float *post_out;          // [count][n] or null
    const uint32_t *ubits;    // MC: info bits [tile][kw][64] (layout 1), else null
    unsigned long long *ctr;  // MC: counters [7] or null
    float param;              // min-sum: alpha (kCnNms) or beta (kCnOms)
    const int *layer_ptr;     // layered: [n_layers + 1] offsets into layer_rows
    const int *layer_rows;    // layered: [m] rows, layer after layer
    int n_layers;
};

// Frame f's Lambda = -channel LLR (input layouts as PhysArgs::layout).
__device__ __forceinline__ float frame_lambda(const PhysArgs &a, int f, int j) {
    const DevGraph &g = a.g;
    if (a.layout == 2) return a.lam[(size_t)f * g.n + j];  // contiguous per frame
    const double ch = a.layout == 0 ? a.llr[(size_t)f * g.n + j]
                                    : a.llr[((size_t)(f >> 6) * g.n + j) * kTile + (f & 63)];
    return -(float)ch;
}

// Frame f into LDS: Lambda = -channel LLR, L = Lambda, E = 0.
__device__ __forceinline__ void frame_load(const PhysArgs &a, int f, float *E, float *L, float *Lam, int tid,
                                           int nt) {
    const DevGraph &g = a.g;
    for (int j = tid; j < g.n; j += nt) {
        Lam[j] = frame_lambda(a, f, j);
        L[j] = Lam[j];
    }
    for (int e = tid; e < g.nnz; e += nt) E[e] = 0.0f;
}

// Monte-Carlo counters of the frames one workgroup decodes (thread 0's
// registers), added to the device counters once, when the workgroup is done:
// one atomic per counter per frame on the same 7 addresses serialised every
// frame of a launch in L2.
struct FrameCounts {
    unsigned long long v[7] = {0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void flush(unsigned long long *ctr) const {
        if (!ctr) return;
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (v[i]) atomicAdd(&ctr[i], v[i]);
    }
};

// Monte-Carlo statistics (McStats) of the frames one workgroup decodes.  At a
// clean channel every frame lands in the first bins, so thread 0 keeps those,
// and the failed frames' bin, in a small static LDS array (registers would
// cost the decoders occupancy; dynamic LDS a frame per CU) and adds them to the
// point's histogram once, as FrameCounts::flush does.  Later bins, undetected
// errors and failure records are rare per unit of work: one atomic each.
constexpr int kMcHotBins = 4;
constexpr int kMcBins = kMcHotBins + 1;  // s_bins: bins 0 .. kMcHotBins - 1, then the failed frames

__device__ __forceinline__ void mc_stats_begin(unsigned *s_bins, int tid) {
    if (tid != 0) return;
#pragma unroll
    for (int i = 0; i < kMcBins; ++i) s_bins[i] = 0u;
}

// thread 0, once per frame: err = the frame's info-bit errors
__device__ __forceinline__ void mc_stats_frame(const McStats &ms, long long frame, int conv, int err,
                                               unsigned *s_bins) {
    if (conv < 0) {
        ++s_bins[kMcHotBins];
        const unsigned long long i = atomicAdd(&ms.und[2], 1ull);
        if (i < (unsigned long long)ms.max_failed) {
            ms.failed[2 * i] = frame;
            ms.failed[2 * i + 1] = err;
        }
        return;
    }
    if (conv < kMcHotBins) ++s_bins[conv];
    else atomicAdd(&ms.hist[min(conv, ms.max_iter - 1)], 1ull);
    if (err) {  // converged to another codeword
        atomicAdd(&ms.und[0], 1ull);
        atomicAdd(&ms.und[1], (unsigned long long)err);
    }
}

__device__ __forceinline__ void mc_stats_flush(const McStats &ms, const unsigned *s_bins, int tid) {
    if (tid != 0) return;
#pragma unroll
    for (int i = 0; i < kMcHotBins; ++i)
        if (s_bins[i] && i < ms.max_iter) atomicAdd(&ms.hist[i], (unsigned long long)s_bins[i]);
    if (s_bins[kMcHotBins]) atomicAdd(&ms.hist[ms.max_iter], (unsigned long long)s_bins[kMcHotBins]);
}

// Outputs and Monte-Carlo counters of frame f (conv = -1: not converged).
// STATS: the kernel's statistics instantiation (the host launches it when the
// point's McStats is set: ms, and s_bins, the workgroup's kMcBins bins of
// mc_stats_begin / _flush); the other one is the code without statistics,
// nothing added (ms unused, s_bins null).
template <bool STATS>
__device__ __forceinline__ void frame_finish(const PhysArgs &a, const McStats &ms, int f, int conv, const float *L,
                                             int *s_err, unsigned *s_bins, int tid, int nt, FrameCounts &fc) {
    const DevGraph &g = a.g;
    const int iters = conv >= 0 ? conv + 1 : a.max_iter;
    for (int j = tid; j < g.n; j += nt) {
        const bool bit = L[j] < 0.0f;
        if (a.z_out) a.z_out[(size_t)f * g.n + j] = bit ? 0 : 1;
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
        // BER counts failed frames only (main.py:130-138); the statistics look
        // at the converged ones too (undetected errors)
        constexpr bool stats = STATS;
        if (conv < 0 || stats) {
            const int kw = (g.k + 31) >> 5;
            int my = 0;
            for (int j = tid; j < g.k; j += nt) {
                const uint32_t w = a.ubits[((size_t)(f >> 6) * kw + (j >> 5)) * kTile + (f & 63)];
                my += (((w >> (j & 31)) & 1u) != (L[j] < 0.0f ? 1u : 0u)) ? 1 : 0;
            }
            atomicAdd(s_err, my);
        }
        __syncthreads();
        if (tid == 0) {
            fc.v[0] += 1ull;
            if (conv < 0) {
                fc.v[1] += 1ull;
                fc.v[2] += (unsigned long long)*s_err;
            } else {
                fc.v[3] += (unsigned long long)conv;
                fc.v[4] += 1ull;
            }
            fc.v[6] += (unsigned long long)iters;
            if constexpr (stats) mc_stats_frame(ms, ms.frame_base + f, conv, *s_err, s_bins);
        }
    }
    __syncthreads();  // LDS reused by the next frame
}

// frame_finish for a decoder whose state is the hard decisions themselves
// (phys_bitflip.hip): bits[j] = frame f's bit estimate b_j (0 / 1), no posterior.
// Same outputs, counters and statistics; synw_out[f] (or null) = synw, the
// syndrome weight the caller counted at exit.
template <bool STATS>
__device__ __forceinline__ void frame_finish_bits(const PhysArgs &a, const McStats &ms, int f, int conv,
                                                  const uint8_t *bits, int synw, int *synw_out, int *s_err,
                                                  unsigned *s_bins, int tid, int nt, FrameCounts &fc) {
    const DevGraph &g = a.g;
    const int iters = conv >= 0 ? conv + 1 : a.max_iter;
    if (a.z_out)
        for (int j = tid; j < g.n; j += nt) a.z_out[(size_t)f * g.n + j] = bits[j] ^ 1;
    if (tid == 0) {
        if (a.conv_out) a.conv_out[f] = conv;
        if (a.status_out) a.status_out[f] = conv >= 0 ? 0 : 1;
        if (a.iters_out) a.iters_out[f] = iters;
        if (synw_out) synw_out[f] = synw;
        *s_err = 0;
    }
    if (a.ctr) {
        __syncthreads();
        constexpr bool stats = STATS;
        if (conv < 0 || stats) {  // as frame_finish: failed frames, and every frame for the statistics
            const int kw = (g.k + 31) >> 5;
            int my = 0;
            for (int j = tid; j < g.k; j += nt) {
                const uint32_t w = a.ubits[((size_t)(f >> 6) * kw + (j >> 5)) * kTile + (f & 63)];
                my += (((w >> (j & 31)) & 1u) != (uint32_t)bits[j]) ? 1 : 0;
            }
            atomicAdd(s_err, my);
        }
        __syncthreads();
        if (tid == 0) {
            fc.v[0] += 1ull;
            if (conv < 0) {
                fc.v[1] += 1ull;
                fc.v[2] += (unsigned long long)*s_err;
            } else {
                fc.v[3] += (unsigned long long)conv;
                fc.v[4] += 1ull;
            }
            fc.v[6] += (unsigned long long)iters;
            if constexpr (stats) mc_stats_frame(ms, ms.frame_base + f, conv, *s_err, s_bins);
        }
    }
    __syncthreads();  // LDS reused by the next frame
}

// ---- min-sum check rule (fp32, every operation rounds once).
// The two smallest |Q| of a row and where the smallest sits.  min2 equals
// min1 on a tie, so which of the tied edges is called the argmin is immaterial.
struct MinPair {
    float min1 = __builtin_inff(), min2 = __builtin_inff();
    int arg = -1;
    __device__ __forceinline__ void add(float a, int i) {
        if (a < min1) {
            min2 = min1;
            min1 = a;
            arg = i;
        } else if (a < min2) {
            min2 = a;
        }
    }
    __device__ __forceinline__ float other(int i) const { return i == arg ? min2 : min1; }
};

// Magnitude correction: normalized (alpha * mag) or offset (max(mag - beta, 0)).
template <int CN>
__device__ __forceinline__ float ms_scale(float mag, float param) {
    static_assert(CN == kCnNms || CN == kCnOms, "min-sum rules only");
    if constexpr (CN == kCnNms) return param * mag;
    else return fmaxf(mag - param, 0.0f);
}

}  // namespace ldpc
