// phys_qtile.hip -- physical mode, fixed-point min-sum with the decoder state
// in HBM, flooding and layered schedules, gfx950.
//
// The integers of phys_quant.hip (its header states the contract; DESIGN.md
// "Physical mode: fixed-point min-sum"; tests/qminsum_ref.py restates it), for
// codes whose int8 / int16 state does not fit LDS (DVB-S2 profile n = 64800:
// 227 KB of messages + 130 KB of posteriors per frame), on the tiles and with
// the machinery of phys_tile.hip: 64 frames per tile, lane = frame,
//   E8 [tile][nnz][64] int8 (CSR edge order)   L16 [tile][n][64] int16
//   Lam8 [tile][n][64] int8 (flooding only)
// so a wavefront's message access is 64 B contiguous and a posterior access
// 128 B; DevState's done / conv / status / iters / tile_active, the bad flags,
// xcd_item placement and the host's poll-and-compact loop are phys_tile.hip's.
// This file keeps the load and the sweeps; the exits, the syndrome, out, count
// and the compaction are phys_tile_state.hip's, shared with the fp32 family.
// There is no padded table and no 16-bit column index here: any n.
//
//   phys_qlayer_tile  one launch per layer and iteration (stream order is the
//                     order of the layers), a wavefront per kRowsPerWave rows
//                     of the layer: L[c_e] and E_e gathered first, Q, the sign
//                     word and the two smallest |Q| in registers, then E_e =
//                     R_e and L[c_e] = Q_e + R_e: 6 B per edge.
//   phys_qcn_tile     flooding check sweep: reads L16 and E8, writes E8 (4 B
//                     per edge) and flags the row parities of the posterior it
//                     read -> bad[it&1][frame], as phys_cn_tile.
//   phys_qvn_tile     L = clamp(Lam + sum E, +-Pmax), an int32 sum clamped
//                     once (1 B per edge + 3 B per column); a frame whose
//                     syndrome was zero stops, converged at it - 1.
//   phys_lsyn_tile    (phys_tile_state.hip) row parities of b = (L < 0) read
//                     from L16 itself: the layered exit of every iteration, the
//                     flooding early exit (iterations 1 and 2) and the sweep
//                     after the last one.
// Iteration 0 takes E = 0 from `first` and every edge of a running frame is
// written once per sweep, so E needs no memset.  Only the lanes of running
// frames load or store: a stopped frame's L16 is its posterior, and the lanes
// past `count` of a ragged last tile never touch memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "phys_tile_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

// The message bytes are streamed once per sweep in each direction: loaded and
// stored non-temporally, as phys_tile.hip's E32.  The load sign-extends.
__device__ __forceinline__ int ld_e8(const int8_t *p) { return (int)(int8_t)__builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_e8(int8_t *p, int v) { __builtin_nontemporal_store((int8_t)v, p); }

__device__ __forceinline__ int q_clamp(int v, int lim) { return min(max(v, -lim), lim); }

template <int CN>
__device__ __forceinline__ int q_scale(int mag, int param_q) {
    static_assert(CN == kCnNms || CN == kCnOms, "min-sum rules only");
    if constexpr (CN == kCnNms) return (param_q * mag + 8) >> 4;
    else return max(mag - param_q, 0);
}

// The two smallest |Q| of a row; min2 = min1 on a tie, so "e is the argmin" is
// a_e == min1.
struct QMin {
    int min1 = 0x7fff, min2 = 0x7fff;
    __device__ __forceinline__ void add(int a) {
        min2 = min(min2, max(min1, a));
        min1 = min(min1, a);
    }
};

__device__ __forceinline__ int q_msg(int q, int min1, int m1, int m2, uint32_t neg) {
    const int mag = abs(q) == min1 ? m2 : m1;
    return ((neg ^ ((uint32_t)q >> 31)) & 1u) ? -mag : mag;
}

// ------------------------------------------------------------------ load
__global__ void phys_qtile_init_kernel(DevGraph g, DevState st, QTile qt, const float *lam32, int flooding) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)st.ntiles * g.n * kTile;
    if (i < total) {
        const size_t f = (i / ((size_t)g.n * kTile)) * kTile + (i & (kTile - 1));
        if (f < (size_t)st.count) {
            const float x = (lam32 ? lam32[i] : -(float)st.ch[i]) * qt.scale;
            const float lim = (float)qt.qmax;
            const int v = (int)fminf(fmaxf(rintf(x), -lim), lim);
            qt.L[i] = (int16_t)v;
            if (flooding) qt.Lam[i] = (int8_t)v;
        }
    }
    if (i < (size_t)st.ntiles * kTile) {
        const int f = (int)i;
        const bool valid = f < st.count;
        frame_reset(st, qt.bad, qt.cap, f, valid);
        if ((f & 63) == 0) st.tile_active[f >> 6] = valid ? 1 : 0;
    }
}

// --------------------------------------------------------------- layered
// Rows of one layer share no column, so no two wavefronts of a launch touch
// the same L or E element.  Longer rows than kDeg take two sweeps, Q recomputed
// in the second from the L and E the first one read (a row's columns are
// distinct, and nothing is stored before the second sweep).
template <int kDeg, int CN>
__global__ __launch_bounds__(256) void phys_qlayer_tile_kernel(DevGraph g, DevState st, QTile qt, int it, int lbeg,
                                                               int lrows, int per_tile, int items,
                                                               const int *__restrict__ row_ptr,
                                                               const int *__restrict__ col_idx,
                                                               const int *__restrict__ layer_rows) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    const bool first = it == 0;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        int tile, part;
        xcd_item(item, per_tile, tile, part);
        if (tile >= st.ntiles || !st.tile_active[tile]) continue;
        const int f = tile * kTile + lane;
        const bool live = st.done[f] == 0;
        if (__ballot(live) == 0ull) continue;
        int16_t *Lt = qt.L + (size_t)tile * g.n * kTile + lane;
        int8_t *Et = qt.E + (size_t)tile * g.nnz * kTile + lane;
        const int i0 = (part * 4 + wave) * kRowsPerWave;
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            if (i0 + rr >= lrows) break;
            const int r = uniform(layer_rows[lbeg + i0 + rr]);
            const int beg = row_ptr[r], deg = row_ptr[r + 1] - beg;
            if (deg <= kDeg) {
                int Q[kDeg], Eo[kDeg];
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    Q[i] = 0;
                    Eo[i] = 0;
                    if (i < deg && live) {
                        Q[i] = Lt[col_idx[beg + i] * kTile];
                        if (!first) Eo[i] = ld_e8(&Et[(beg + i) * kTile]);
                    }
                }
                QMin mp;
                uint32_t sx = 0u;
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    if (i < deg) {
                        Q[i] = q_clamp(Q[i] - Eo[i], qt.qmax);
                        mp.add(abs(Q[i]));
                        sx ^= (uint32_t)Q[i];
                    }
                }
                if (live) {
                    const uint32_t neg = sx >> 31;
                    const int m1 = q_scale<CN>(mp.min1, qt.param_q), m2 = q_scale<CN>(mp.min2, qt.param_q);
#pragma unroll
                    for (int i = 0; i < kDeg; ++i) {
                        if (i < deg) {
                            const int R = q_msg(Q[i], mp.min1, m1, m2, neg);
                            st_e8(&Et[(beg + i) * kTile], R);
                            Lt[col_idx[beg + i] * kTile] = (int16_t)(Q[i] + R);
                        }
                    }
                }
            } else if (live) {
                const int end = beg + deg;
                QMin mp;
                uint32_t sx = 0u;
                for (int e = beg; e < end; ++e) {
                    const int Lc = Lt[col_idx[e] * kTile];
                    const int q = q_clamp(first ? Lc : Lc - ld_e8(&Et[e * kTile]), qt.qmax);
                    mp.add(abs(q));
                    sx ^= (uint32_t)q;
                }
                const uint32_t neg = sx >> 31;
                const int m1 = q_scale<CN>(mp.min1, qt.param_q), m2 = q_scale<CN>(mp.min2, qt.param_q);
                for (int e = beg; e < end; ++e) {
                    const int c = col_idx[e];
                    const int Lc = Lt[c * kTile];
                    const int q = q_clamp(first ? Lc : Lc - ld_e8(&Et[e * kTile]), qt.qmax);
                    const int R = q_msg(q, mp.min1, m1, m2, neg);
                    st_e8(&Et[e * kTile], R);
                    Lt[c * kTile] = (int16_t)(q + R);
                }
            }
        }
    }
}

// -------------------------------------------------------------- flooding
// A wavefront takes kRowsPerWave rows of one tile (as phys_cn_tile): E = R
// from the L and E every row reads, and the row parity of the posterior it
// read (the syndrome of iteration it - 1; none before iteration 0).
template <int kDeg, int CN>
__global__ __launch_bounds__(256) void phys_qcn_tile_kernel(DevGraph g, DevState st, QTile qt, int it, int per_tile,
                                                            int items, const int *__restrict__ row_ptr,
                                                            const int *__restrict__ col_idx) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    const bool first = it == 0;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        int tile, part;
        xcd_item(item, per_tile, tile, part);
        if (tile >= st.ntiles || !st.tile_active[tile]) continue;
        const int f = tile * kTile + lane;
        const bool live = st.done[f] == 0;
        if (__ballot(live) == 0ull) continue;
        const int16_t *Lt = qt.L + (size_t)tile * g.n * kTile + lane;
        int8_t *Et = qt.E + (size_t)tile * g.nnz * kTile + lane;
        uint32_t bad = 0u;
        const int r0 = (part * 4 + wave) * kRowsPerWave;
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            const int r = r0 + rr;
            if (r >= g.m) break;
            const int beg = row_ptr[r], deg = row_ptr[r + 1] - beg;
            if (deg <= kDeg) {
                int Q[kDeg], Eo[kDeg];
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    Q[i] = 0;
                    Eo[i] = 0;
                    if (i < deg && live) {
                        Q[i] = Lt[col_idx[beg + i] * kTile];
                        if (!first) Eo[i] = ld_e8(&Et[(beg + i) * kTile]);
                    }
                }
                QMin mp;
                uint32_t sx = 0u, lx = 0u;
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    if (i < deg) {
                        lx ^= (uint32_t)Q[i];
                        Q[i] = q_clamp(Q[i] - Eo[i], qt.qmax);
                        mp.add(abs(Q[i]));
                        sx ^= (uint32_t)Q[i];
                    }
                }
                bad |= lx >> 31;
                if (live) {
                    const uint32_t neg = sx >> 31;
                    const int m1 = q_scale<CN>(mp.min1, qt.param_q), m2 = q_scale<CN>(mp.min2, qt.param_q);
#pragma unroll
                    for (int i = 0; i < kDeg; ++i)
                        if (i < deg) st_e8(&Et[(beg + i) * kTile], q_msg(Q[i], mp.min1, m1, m2, neg));
                }
            } else if (live) {
                const int end = beg + deg;
                QMin mp;
                uint32_t sx = 0u, lx = 0u;
                for (int e = beg; e < end; ++e) {
                    const int Lc = Lt[col_idx[e] * kTile];
                    const int q = q_clamp(first ? Lc : Lc - ld_e8(&Et[e * kTile]), qt.qmax);
                    lx ^= (uint32_t)Lc;
                    mp.add(abs(q));
                    sx ^= (uint32_t)q;
                }
                bad |= lx >> 31;
                const uint32_t neg = sx >> 31;
                const int m1 = q_scale<CN>(mp.min1, qt.param_q), m2 = q_scale<CN>(mp.min2, qt.param_q);
                for (int e = beg; e < end; ++e) {
                    const int Lc = Lt[col_idx[e] * kTile];
                    const int q = q_clamp(first ? Lc : Lc - ld_e8(&Et[e * kTile]), qt.qmax);
                    st_e8(&Et[e * kTile], q_msg(q, mp.min1, m1, m2, neg));
                }
            }
        }
        if (it >= 1 && live && bad) qt.bad[(it & 1) * qt.cap + f] = 1;
    }
}

// A wavefront takes kColsPerWave columns of one tile: L = clamp(Lam + E_0 +
// E_1 + ..., +-Pmax) in int32.  With every column of degree <= kCD (0 = the
// plain loop for any degree) a batch of kQVnBatch columns issues all its
// message loads before the first sum, as phys_vn_tile.  The exits and the
// running counts are phys_vn_tile's.
constexpr int kQVnBatch = 4;

template <int kCD>
__global__ __launch_bounds__(256) void phys_qvn_tile_kernel(DevGraph g, DevState st, QTile qt, int it, int per_tile,
                                                            int items, const int *__restrict__ csc_ptr,
                                                            const int *__restrict__ csc_edge, int *active_count,
                                                            int max_iter) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        int tile, part;
        xcd_item(item, per_tile, tile, part);
        if (tile >= st.ntiles || !st.tile_active[tile]) continue;
        const int f = tile * kTile + lane;
        // done[f] may flip to 1 under us (the wave below): either value gives upd = 0
        const bool live = st.done[f] == 0;
        const bool conv_now = live && it >= 1 && qt.bad[(it & 1) * qt.cap + f] == 0;
        const bool upd = live && !conv_now;
        const int8_t *Et = qt.E + (size_t)tile * g.nnz * kTile + lane;
        int16_t *Lt = qt.L + (size_t)tile * g.n * kTile + lane;
        const int8_t *Lamt = qt.Lam + (size_t)tile * g.n * kTile + lane;
        if (__ballot(upd) != 0ull) {
            const int j0 = (part * 4 + wave) * kColsPerWave;
            const int j1 = min(g.n, j0 + kColsPerWave);
            if constexpr (kCD > 0) {
                constexpr int CB = kQVnBatch;
#pragma unroll
                for (int b = 0; b < kColsPerWave / CB; ++b) {
                    int Ev[CB][kCD], La[CB];
                    int p0[CB], cd[CB];
#pragma unroll
                    for (int q = 0; q < CB; ++q) {
                        const int j = j0 + b * CB + q;
                        p0[q] = j < j1 ? csc_ptr[j] : 0;
                        cd[q] = j < j1 ? csc_ptr[j + 1] - p0[q] : 0;
                    }
#pragma unroll
                    for (int q = 0; q < CB; ++q) {
                        La[q] = 0;
                        if (upd && j0 + b * CB + q < j1) La[q] = (int)Lamt[(j0 + b * CB + q) * kTile];
#pragma unroll
                        for (int i = 0; i < kCD; ++i) {
                            Ev[q][i] = 0;
                            if (upd && i < cd[q]) Ev[q][i] = ld_e8(&Et[csc_edge[p0[q] + i] * kTile]);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < CB; ++q) {
                        int sum = La[q];
#pragma unroll
                        for (int i = 0; i < kCD; ++i)
                            if (i < cd[q]) sum += Ev[q][i];
                        if (upd && j0 + b * CB + q < j1)
                            Lt[(j0 + b * CB + q) * kTile] = (int16_t)q_clamp(sum, qt.pmax);
                    }
                }
            } else {
                for (int j = j0; j < j1; ++j) {
                    if (upd) {
                        int sum = (int)Lamt[j * kTile];
                        for (int p = csc_ptr[j]; p < csc_ptr[j + 1]; ++p) sum += ld_e8(&Et[csc_edge[p] * kTile]);
                        Lt[j * kTile] = (int16_t)q_clamp(sum, qt.pmax);
                    }
                }
            }
        }
        if (part == 0 && wave == 0) {
            if (conv_now) {  // syndrome of iteration it-1 was zero
                st.done[f] = 1;
                st.conv[f] = it - 1;
                st.status[f] = 0;
                st.iters[f] = it;
            }
            qt.bad[((it + 1) & 1) * qt.cap + f] = 0;  // for the next CN sweep
            const unsigned long long any = __ballot(upd);
            if (lane == 0) {
                st.tile_active[tile] = any != 0ull ? 1 : 0;
                if (any) {
                    atomicAdd(&active_count[it], 1);  // host polls: 0 -> every frame has stopped
                    atomicAdd(&active_count[max_iter + it], (int)__popcll(any));  // running frames (compaction)
                }
            }
        }
    }
}

template <int CN>
void launch_qlayer_rule(const DevGraph &g, const DevState &st, const QTile &qt, int it, int lbeg, int lrows,
                        const int *layer_rows, hipStream_t s) {
    const int per_tile = rows_per_tile(lrows);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    for_row_deg(g.max_row_deg, [&](auto deg) {
        phys_qlayer_tile_kernel<decltype(deg)::value, CN><<<stride_grid(items), 256, 0, s>>>(
            g, st, qt, it, lbeg, lrows, per_tile, items, g.row_ptr, g.col_idx, layer_rows);
    });
}

template <int CN>
void launch_qcn_rule(const DevGraph &g, const DevState &st, const QTile &qt, int it, hipStream_t s) {
    const int per_tile = rows_per_tile(g.m);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    for_row_deg(g.max_row_deg, [&](auto deg) {
        phys_qcn_tile_kernel<decltype(deg)::value, CN><<<stride_grid(items), 256, 0, s>>>(
            g, st, qt, it, per_tile, items, g.row_ptr, g.col_idx);
    });
}

}  // namespace

hipError_t launch_phys_qtile_init(const DevGraph &g, const DevState &st, const QTile &qt, const float *lam32,
                                  bool flooding, hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    const size_t total = std::max((size_t)st.ntiles * g.n * kTile, (size_t)st.ntiles * kTile);
    phys_qtile_init_kernel<<<grid_for(total, 256), 256, 0, s>>>(g, st, qt, lam32, flooding ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_phys_qlayer_tile(const DevGraph &g, const DevState &st, const QTile &qt, int cn, int it, int lbeg,
                                   int lrows, const int *layer_rows, hipStream_t s) {
    if (!layer_rows || lbeg < 0 || lrows < 0 || lbeg + lrows > g.m) return hipErrorInvalidValue;
    if (lrows == 0 || st.ntiles <= 0) return hipSuccess;
    switch (cn) {
    case kCnNms: launch_qlayer_rule<kCnNms>(g, st, qt, it, lbeg, lrows, layer_rows, s); break;
    case kCnOms: launch_qlayer_rule<kCnOms>(g, st, qt, it, lbeg, lrows, layer_rows, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_phys_qtile_cn(const DevGraph &g, const DevState &st, const QTile &qt, int cn, int it,
                                hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    switch (cn) {
    case kCnNms: launch_qcn_rule<kCnNms>(g, st, qt, it, s); break;
    case kCnOms: launch_qcn_rule<kCnOms>(g, st, qt, it, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_phys_qtile_vn(const DevGraph &g, const DevState &st, const QTile &qt, int it, int *active_count,
                                int max_iter, hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    const int per_tile = (g.n + 4 * kColsPerWave - 1) / (4 * kColsPerWave);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    if (g.max_col_deg <= 8)
        phys_qvn_tile_kernel<8><<<stride_grid(items), 256, 0, s>>>(g, st, qt, it, per_tile, items, g.csc_ptr,
                                                                   g.csc_edge, active_count, max_iter);
    else
        phys_qvn_tile_kernel<0><<<stride_grid(items), 256, 0, s>>>(g, st, qt, it, per_tile, items, g.csc_ptr,
                                                                   g.csc_edge, active_count, max_iter);
    return hipGetLastError();
}

}  // namespace ldpc
