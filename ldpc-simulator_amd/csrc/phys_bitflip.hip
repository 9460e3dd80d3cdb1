// phys_bitflip.hip -- physical mode's hard-decision baseline: parallel
// gradient-descent bit flipping (Wadayama et al.) on the sparse graph, gfx950.
//
// One family, weight w >= 0 and threshold theta (include/ldpc_hip.h
// "bit-flipping decoders"; w = 0 is plain bit flipping, with theta = 0 the
// majority rule).  fp32, every operation rounds once:
//   Lam = -(float)llr, b = (Lam < 0); per iteration, while any s_r = XOR of b
//   over row r is 1: u_j = sum of s over column j's rows, c_j = b_j ? -Lam_j : Lam_j,
//   Delta_j = fl(fl(w c_j) + (float)(d_j - 2 u_j))  ((float)(d_j - 2 u_j) alone
//   when w == 0), every j with Delta_j < theta flips from the same s, s is
//   recomputed; conv = the first iteration that ends with s = 0.
// No messages: the state of a frame is n bits (and Lam when w > 0).
//
// bitflip_kernel (any w): one workgroup per frame, frames grid-strided, Lam[n]
// fp32 and b[n], s[m] as bytes in LDS; a thread per row forms the syndrome, a
// thread per column u_j through the CSC lists and the flip.
//
// bitflip_sliced_kernel (w == 0, column degrees <= 63): one workgroup per
// 64-frame tile, one 64-bit word per column (bit f = frame f of the tile) and
// per row in LDS.  A row's syndrome of 64 frames is the XOR of its columns'
// words.  With w == 0 the flip rule is u_j >= t(d_j), t(d) the smallest u with
// (float)(d - 2u) < theta (d + 1 if none: never) -- the same fp32 comparison,
// made once per degree.  u_j of 64 frames is counted in bit planes (a ripple
// half-adder per row word) and compared with the constant t from the top plane
// down.  Both kernels give the same outputs and counters.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phys_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

typedef unsigned long long u64;

struct BfArgs {
    PhysArgs p;     // post_out, param and the layer table unused
    float weight, theta;
    int *synw_out;  // [count] or null: syndrome weight at exit
};

constexpr int kBfThreads = 256;
constexpr int kBfWaves = kBfThreads / 64;

template <bool W, bool STATS>
__global__ __launch_bounds__(kBfThreads) void bitflip_kernel(BfArgs a, McStats ms) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DevGraph &g = a.p.g;
    float *Lam = lds;                                           // [n] (read when w > 0 only)
    uint8_t *b = reinterpret_cast<uint8_t *>(Lam + ((g.n + 3) & ~3));  // [n] bit estimates
    uint8_t *sy = b + ((g.n + 3) & ~3);                         // [m] row syndromes
    __shared__ int s_err, s_synw;
    unsigned *s_bins = nullptr;
    if constexpr (STATS) {  // static LDS of the statistics instantiation only
        __shared__ unsigned bins[kMcBins];
        s_bins = bins;
    }
    FrameCounts fc;
    const int tid = threadIdx.x, nt = blockDim.x;
    if constexpr (STATS) mc_stats_begin(s_bins, tid);
    // s = H b of the frame in LDS; nonzero iff any row fails (with a barrier)
    auto syndrome = [&]() -> int {
        int bad = 0;
        for (int r = tid; r < g.m; r += nt) {
            unsigned par = 0u;
            for (int e = g.row_ptr[r]; e < g.row_ptr[r + 1]; ++e) par ^= b[g.col_idx[e]];
            sy[r] = (uint8_t)par;
            bad |= (int)par;
        }
        return __syncthreads_or(bad);
    };
    for (int f = blockIdx.x; f < a.p.count; f += gridDim.x) {
        for (int j = tid; j < g.n; j += nt) {
            const float lam = frame_lambda(a.p, f, j);
            if constexpr (W) Lam[j] = lam;
            b[j] = lam < 0.0f ? 1 : 0;
        }
        __syncthreads();
        int bad = syndrome();
        int conv = -1;
        for (int it = 0; it < a.p.max_iter; ++it) {
            if (bad) {
                for (int j = tid; j < g.n; j += nt) {
                    const int p0 = g.csc_ptr[j], p1 = g.csc_ptr[j + 1];
                    int u = 0;
                    for (int p = p0; p < p1; ++p) u += sy[g.csc_row[p]];
                    float delta = (float)(p1 - p0 - 2 * u);
                    if constexpr (W) {
                        const float c = b[j] ? -Lam[j] : Lam[j];
                        const float wc = a.weight * c;
                        delta = wc + delta;
                    }
                    if (delta < a.theta) b[j] ^= 1;
                }
                __syncthreads();
                bad = syndrome();
            }
            if (!bad) {
                conv = it;
                break;
            }
        }
        int synw = 0;
        if (a.synw_out && conv < 0) {  // conv is uniform
            if (tid == 0) s_synw = 0;
            __syncthreads();
            int my = 0;
            for (int r = tid; r < g.m; r += nt) my += sy[r];
            if (my) atomicAdd(&s_synw, my);
            __syncthreads();
            synw = s_synw;
        }
        frame_finish_bits<STATS>(a.p, ms, f, conv, b, synw, a.synw_out, &s_err, s_bins, tid, nt, fc);
    }
    if (tid == 0) fc.flush(a.p.ctr);
    if constexpr (STATS) mc_stats_flush(ms, s_bins, tid);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// NP bit planes count u_j: 2^NP > the graph's largest column degree.
template <int NP>
__global__ __launch_bounds__(kBfThreads) void bitflip_sliced_kernel(BfArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds64[];
    const DevGraph &g = a.p.g;
    u64 *bw = lds64;     // [n] bit f = frame f's estimate of the column
    u64 *sw = bw + g.n;  // [m] bit f = frame f's syndrome of the row
    __shared__ u64 s_wbad[kBfWaves];
    __shared__ int s_err[kTile], s_syn[kTile];
    __shared__ uint8_t s_thr[kTile];  // t(d), d = 0 .. 63
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    FrameCounts fc;
    if (tid < kTile) {
        const int d = tid;
        int t = d + 1;
        for (int u = d; u >= 0; --u)  // (float)(d - 2u) falls as u grows: the smallest u that flips
            if ((float)(d - 2 * u) < a.theta) t = u;
        s_thr[d] = (uint8_t)t;
    }
    // sw = H bw; the OR of all rows' words: bit f set iff frame f has a failing row (with a barrier)
    auto syndrome = [&]() -> u64 {
        u64 any = 0;
        for (int r = tid; r < g.m; r += nt) {
            u64 x = 0;
            for (int e = g.row_ptr[r]; e < g.row_ptr[r + 1]; ++e) x ^= bw[g.col_idx[e]];
            sw[r] = x;
            any |= x;
        }
        unsigned lo = (unsigned)any, hi = (unsigned)(any >> 32);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo |= __shfl_xor(lo, off);
            hi |= __shfl_xor(hi, off);
        }
        if (lane == 0) s_wbad[wave] = ((u64)hi << 32) | lo;
        __syncthreads();
        u64 bad = 0;
        for (int w = 0; w < nw; ++w) bad |= s_wbad[w];
        return bad;
    };
    const int ntiles = (a.p.count + kTile - 1) / kTile;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int f0 = tile * kTile;
        const int cnt = min(kTile, a.p.count - f0);
        for (int j = tid; j < g.n; j += nt) {
            u64 w = 0;
            if (cnt == kTile && a.p.layout == 2) {
                // a full tile of the frame source's rows: the loads of 16 frames in flight (a loop of
                // dependent-looking loads left the pack bound by memory latency)
                const float *src = a.p.lam + (size_t)f0 * g.n + j;
#pragma unroll 16
                for (int f = 0; f < kTile; ++f) w |= (u64)(src[(size_t)f * g.n] < 0.0f ? 1 : 0) << f;
            } else {
                for (int f = 0; f < cnt; ++f) w |= (u64)(frame_lambda(a.p, f0 + f, j) < 0.0f ? 1 : 0) << f;
            }
            bw[j] = w;
        }
        if (tid < kTile) {
            s_err[tid] = 0;
            s_syn[tid] = 0;
        }
        __syncthreads();
        u64 bad = syndrome();
        u64 active = cnt == kTile ? ~0ull : ((1ull << cnt) - 1ull);  // frames not yet converged
        int conv = -1;                                               // thread f < 64: frame f's
        for (int it = 0; it < a.p.max_iter; ++it) {
            const u64 run = active & bad;
            if (run) {
                for (int j = tid; j < g.n; j += nt) {
                    const int p0 = g.csc_ptr[j], p1 = g.csc_ptr[j + 1];
                    const int t = s_thr[p1 - p0];
                    if (t > p1 - p0) continue;  // never flips
                    u64 c[NP];
#pragma unroll
                    for (int i = 0; i < NP; ++i) c[i] = 0;
                    for (int p = p0; p < p1; ++p) {
                        u64 carry = sw[g.csc_row[p]];
#pragma unroll
                        for (int i = 0; i < NP; ++i) {
                            const u64 up = c[i] & carry;
                            c[i] ^= carry;
                            carry = up;
                        }
                    }
                    // u >= t, from the top plane down: ge = decided greater, eq = equal so far
                    u64 ge = 0, eq = ~0ull;
#pragma unroll
                    for (int i = NP - 1; i >= 0; --i) {
                        const u64 tm = ((t >> i) & 1) ? ~0ull : 0ull;
                        ge |= eq & c[i] & ~tm;
                        eq &= ~(c[i] ^ tm);
                    }
                    ge |= eq;
                    bw[j] ^= ge & run;
                }
                __syncthreads();
                bad = syndrome();
            }
            const u64 done = active & ~bad;
            if (tid < kTile && ((done >> tid) & 1ull)) conv = it;
            active &= bad;
            if (!active) break;
        }
        // --- outputs: the frames left in `active` did not converge
        if (a.p.z_out)
            for (int j = tid; j < g.n; j += nt) {
                const u64 w = ~bw[j];
                for (int f = 0; f < cnt; ++f) a.p.z_out[(size_t)(f0 + f) * g.n + j] = (uint8_t)((w >> f) & 1ull);
            }
        const int iters = conv >= 0 ? conv + 1 : a.p.max_iter;
        if (tid < cnt) {
            if (a.p.conv_out) a.p.conv_out[f0 + tid] = conv;
            if (a.p.status_out) a.p.status_out[f0 + tid] = conv >= 0 ? 0 : 1;
            if (a.p.iters_out) a.p.iters_out[f0 + tid] = iters;
        }
        const bool failed = (active >> lane) & 1ull;  // this lane's frame
        if (a.p.ctr && active) {
            // info-bit errors of the failed frames (main.py:130-138): lane f, the waves share the words
            const int kw = (g.k + 31) >> 5;
            int e = 0;
            if (failed)
                for (int w = wave; w < kw; w += nw) {
                    const uint32_t word = a.p.ubits[((size_t)tile * kw + w) * kTile + lane];
                    const int nb = min(32, g.k - 32 * w);
                    for (int i = 0; i < nb; ++i)
                        e += (((word >> i) & 1u) != (uint32_t)((bw[32 * w + i] >> lane) & 1ull)) ? 1 : 0;
                }
            if (e) atomicAdd(&s_err[lane], e);
        }
        if (a.synw_out && active) {
            int sy = 0;
            if (failed)
                for (int r = wave; r < g.m; r += nw) sy += (int)((sw[r] >> lane) & 1ull);
            if (sy) atomicAdd(&s_syn[lane], sy);
        }
        __syncthreads();
        if (a.synw_out && tid < cnt) a.synw_out[f0 + tid] = s_syn[tid];
        if (a.p.ctr && tid < kTile) {  // wave 0, whole
            const int err = wave_sum(failed ? s_err[tid] : 0);
            const int csum = wave_sum(tid < cnt && conv >= 0 ? conv : 0);
            const int isum = wave_sum(tid < cnt ? iters : 0);
            if (tid == 0) {
                const int nfail = __popcll(active);
                fc.v[0] += (unsigned long long)cnt;
                fc.v[1] += (unsigned long long)nfail;
                fc.v[2] += (unsigned long long)err;
                fc.v[3] += (unsigned long long)csum;
                fc.v[4] += (unsigned long long)(cnt - nfail);
                fc.v[6] += (unsigned long long)isum;
            }
        }
        __syncthreads();  // LDS reused by the next tile
    }
    if (tid == 0) fc.flush(a.p.ctr);
}

}  // namespace

size_t bitflip_lds_bytes(const DevGraph &g) {
    return sizeof(float) * (size_t)((g.n + 3) & ~3) + (size_t)((g.n + 3) & ~3) + (size_t)((g.m + 3) & ~3);
}

size_t bitflip_sliced_lds_bytes(const DevGraph &g) { return sizeof(u64) * ((size_t)g.n + (size_t)g.m); }

bool bitflip_sliced_applies(const DevGraph &g) { return g.max_col_deg <= 63; }

int bitflip_threads() { return kBfThreads; }

hipError_t launch_bitflip(const DevGraph &g, const double *llr, const float *lam, int layout, int count, int max_iter,
                          uint8_t *z, int *conv, int *status, int *iters, int *synw, const uint32_t *ubits,
                          unsigned long long *ctr, int grid, hipStream_t s, const BitflipRule &rule,
                          const McStats &ms_in) {
    if (count <= 0) return hipSuccess;
    BfArgs a{};
    a.p = PhysArgs{g, llr, lam, layout, count, max_iter, z, conv, status, iters, nullptr, ubits, ctr, 0.0f,
                   nullptr, nullptr, 0};
    a.weight = rule.weight;
    a.theta = rule.theta;
    a.synw_out = synw;
    const McStats ms = ctr ? ms_in : McStats{};
    if (rule.sliced) {
        if (rule.weight != 0.0f || ms.hist || !bitflip_sliced_applies(g)) return hipErrorInvalidValue;
        const size_t lds = bitflip_sliced_lds_bytes(g);
        if (g.max_col_deg <= 7) bitflip_sliced_kernel<3><<<grid, kBfThreads, lds, s>>>(a);
        else if (g.max_col_deg <= 15) bitflip_sliced_kernel<4><<<grid, kBfThreads, lds, s>>>(a);
        else bitflip_sliced_kernel<6><<<grid, kBfThreads, lds, s>>>(a);
        return hipGetLastError();
    }
    const size_t lds = bitflip_lds_bytes(g);
    if (rule.weight != 0.0f) {
        if (ms.hist) bitflip_kernel<true, true><<<grid, kBfThreads, lds, s>>>(a, ms);
        else bitflip_kernel<true, false><<<grid, kBfThreads, lds, s>>>(a, ms);
    } else {
        if (ms.hist) bitflip_kernel<false, true><<<grid, kBfThreads, lds, s>>>(a, ms);
        else bitflip_kernel<false, false><<<grid, kBfThreads, lds, s>>>(a, ms);
    }
    return hipGetLastError();
}

}  // namespace ldpc
