// phys_layered.hip -- physical mode, min-sum check rule, layered (row-serial)
// schedule, gfx950.
//
// The rows of the sparse graph are split into layers whose rows share no column
// (first-fit, ldpc_layers_build).  An iteration visits the layers in order; a
// row's update reads the posteriors the earlier layers of the same iteration
// already improved:
//   Q_e = L[c_e] - E_e            (fp32, every operation rounds once)
//   R_e = sign * scale(min over the other edges of |Q|)
//   L[c_e] = Q_e + R_e,  E_e = R_e
// scale = alpha * mag (normalized) or max(mag - beta, 0) (offset).  After the
// last layer, b = (L < 0) and the frame stops when H b = 0 -- the exit of
// phys_kernels.hip, as are the outputs and counters (phys_common.h).
//
// One workgroup per frame, frames grid-strided; LDS holds E[nnz] and L[n]
// (Lambda is not needed after the load: 38 KB for wimax_2304_0.5 against the
// flooding kernel's 48 KB, four frames per CU instead of three).  A
// thread takes one row of the current layer; rows of a layer touch disjoint
// columns and edges, so a layer needs no ordering inside and one workgroup
// barrier after it.  The block is the largest layer rounded up to a wavefront,
// at most 256 threads (WiMAX layers have 24-192 rows).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "phys_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

template <int CN, bool STATS>
__global__ __launch_bounds__(256) void phys_layered_kernel(PhysArgs a, McStats ms) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DevGraph &g = a.g;
    float *E = lds;                     // [nnz]
    float *L = E + ((g.nnz + 3) & ~3);  // [n]
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
        for (int j = tid; j < g.n; j += nt) L[j] = frame_lambda(a, f, j);
        for (int e = tid; e < g.nnz; e += nt) E[e] = 0.0f;
        __syncthreads();
        int conv = -1;
        for (int it = 0; it < a.max_iter; ++it) {
            for (int l = 0; l < a.n_layers; ++l) {
                const int i1 = a.layer_ptr[l + 1];
                for (int i = a.layer_ptr[l] + tid; i < i1; i += nt) {
                    const int r = a.layer_rows[i];
                    const int b = g.row_ptr[r], e1 = g.row_ptr[r + 1];
                    MinPair mp;
                    unsigned neg = 0u;
                    for (int e = b; e < e1; ++e) {
                        const float Q = L[g.col_idx[e]] - E[e];
                        mp.add(fabsf(Q), e);
                        neg ^= (Q < 0.0f) ? 1u : 0u;
                    }
                    // a row's columns are distinct: L[c_e] is still the value
                    // the first sweep read when edge e is rewritten
                    for (int e = b; e < e1; ++e) {
                        const int c = g.col_idx[e];
                        const float Q = L[c] - E[e];
                        const float mag = ms_scale<CN>(mp.other(e), a.param);
                        const float R = ((neg ^ ((Q < 0.0f) ? 1u : 0u)) != 0u) ? -mag : mag;
                        L[c] = Q + R;
                        E[e] = R;
                    }
                }
                __syncthreads();
            }
            // --- syndrome of b = (L < 0)
            int bad = 0;
            for (int r = tid; r < g.m && !bad; r += nt) {
                unsigned par = 0u;
                for (int e = g.row_ptr[r]; e < g.row_ptr[r + 1]; ++e) par ^= (L[g.col_idx[e]] < 0.0f) ? 1u : 0u;
                bad = (int)par;
            }
            if (!__syncthreads_or(bad)) {
                conv = it;
                break;
            }
        }
        frame_finish<STATS>(a, ms, f, conv, L, &s_err, s_bins, tid, nt, fc);
    }
    if (tid == 0) fc.flush(a.ctr);
    if constexpr (STATS) mc_stats_flush(ms, s_bins, tid);
}

}  // namespace

size_t phys_layered_lds_bytes(const DevGraph &g) {
    return sizeof(float) * (size_t)(((g.nnz + 3) & ~3) + ((g.n + 3) & ~3));
}

// LDPC_LAYERED_NT=64|128|256 (read per launch) overrides the block size (A/B)
int phys_layered_threads(const PhysRule &rule) {
    if (const char *e = getenv("LDPC_LAYERED_NT")) {
        const int nt = atoi(e);
        if (nt == 64 || nt == 128 || nt == 256) return nt;
    }
    return std::min(256, std::max(64, (rule.max_layer + 63) & ~63));
}

hipError_t launch_phys_layered(const DevGraph &g, const double *llr, const float *lam, int layout, int count,
                               int max_iter, uint8_t *z, int *conv, int *status, int *iters, float *post,
                               const uint32_t *ubits, unsigned long long *ctr, int grid, hipStream_t s,
                               const PhysRule &rule, const McStats &ms_in) {
    if (!rule.layer_ptr || !rule.layer_rows || rule.n_layers <= 0) return hipErrorInvalidValue;
    PhysArgs a{g, llr, lam, layout, count, max_iter, z, conv, status, iters, post, ubits, ctr, rule.param,
               rule.layer_ptr, rule.layer_rows, rule.n_layers};
    const McStats ms = ctr ? ms_in : McStats{};  // ms.hist set: the kernel's statistics instantiation
    if (count <= 0) return hipSuccess;
    const size_t lds = phys_layered_lds_bytes(g);
    const int nt = phys_layered_threads(rule);
    switch (rule.cn) {
    case kCnNms:
        if (ms.hist) phys_layered_kernel<kCnNms, true><<<grid, nt, lds, s>>>(a, ms);
        else phys_layered_kernel<kCnNms, false><<<grid, nt, lds, s>>>(a, ms);
        break;
    case kCnOms:
        if (ms.hist) phys_layered_kernel<kCnOms, true><<<grid, nt, lds, s>>>(a, ms);
        else phys_layered_kernel<kCnOms, false><<<grid, nt, lds, s>>>(a, ms);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ldpc
