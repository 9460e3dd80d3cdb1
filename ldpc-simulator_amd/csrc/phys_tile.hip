// phys_tile.hip -- physical mode with the decoder state in HBM (SURVEY.md
// §8 f4, BASELINE config 5), gfx950.
//
// Same arithmetic as phys_kernels.hip (phys_math.h, identical operation
// order, so both paths give bit-identical results), for codes whose per-frame
// state does not fit in LDS (DVB-S2-profile n=64800: E 0.9 MB + L 0.26 MB per
// frame).  Layout as the parity decoder: 64 frames per tile, lane = frame,
//   E32 [tile][nnz][64] fp32   L32 [tile][n][64] fp32   ch [tile][n][64] fp64
// so every load/store of a wavefront is 256 B contiguous.
//
//   phys_cn_tile  one wavefront per (tile, 4 check rows): per row, gather
//                 L[col] and E_old, keep phi(|M|) and the signs of M in
//                 registers (rows of degree <= kDeg), write E_new: 12 B/edge.
//                 The same sweep forms the row parity of the hard decisions
//                 (L < 0) -> bad[it&1][frame]: the syndrome of the previous
//                 iteration's posterior, for free.
//   phys_vn_tile  one wavefront per (tile, 8 columns): L = Lambda + sum E
//                 (Lambda = -channel LLR) in CSC order: 4 B/edge + 12 B/col.
//                 A frame whose syndrome was zero stops here, converged at
//                 the previous iteration (exactly the LDS kernel's exit).
// After the last iteration a syndrome-only CN sweep and phys_tile_final give
// the frames that converge on it.
// The bookkeeping around the sweeps -- the exits, phys_tile_final, the
// syndrome read from L, out, count and the compaction -- is shared with the
// fixed-point family and lives in phys_tile_state.hip; this file keeps the
// load, the sweeps and the early syndrome from the VN sweep's bytes.
// Monte-Carlo runs (counters only) compact: once at most a quarter of the
// launched slots still run, the finished frames are counted and the running
// ones move into the first tiles (phys_compact_*), so the last sweeps launch
// those tiles only -- at 1 dB on the DVB-S2 profile the fourth CN sweep ran
// for ~5 % of the frames, scattered over every tile, at the cost of a full
// sweep (profiles/r5s_c5).  Each (tile, row block) and (tile, column block) is
// placed XCD-aware like cn_kernel.
// The layered min-sum schedule runs on the same tiles (phys_layer_tile: one
// launch per layer, then phys_tile_state.hip's syndrome and exit; further down).
// Frames come from frame_kernels.hip (directly as fp32 Lambda/L for IRA
// codes, else as fp64 ch converted by phys_tile_init).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phys_common.h"
#include "phys_math.h"
#include "phys_tile_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

// The fp32 message array (streamed once per pass in each direction, far
// larger than L2) is loaded / stored non-temporally, so the gathers of L keep
// L2 to themselves (as the parity kernels' E stream; +2-3 %,
// profiles/r1u_nt/ab_phys_nt.txt).
__device__ __forceinline__ float ld_e32(const float *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_e32(float *p, float v) { __builtin_nontemporal_store(v, p); }


constexpr int kVnBatch = 4;  // columns per batch of phys_vn_tile's batched loads (2 / 8: same or slower)

// ------------------------------------------------------- tile decoder
__global__ void phys_tile_init_kernel(DevGraph g, DevState st, PhysTile pt, int convert) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)st.ntiles * g.n * kTile;
    if (convert && i < total) pt.L[i] = pt.Lam[i] = -(float)st.ch[i];  // Lambda = log P0/P1 = -channel LLR
    if (i < (size_t)st.ntiles * kTile) {
        const int f = (int)i;
        const bool valid = f < st.count;
        frame_reset(st, pt.bad, pt.cap, f, valid);
        if ((f & 63) == 0) st.tile_active[f >> 6] = valid ? 1 : 0;
    }
}

// One row's update from its gathered posteriors Lc and messages Eo (E_old;
// unused on iteration 0, for a stopped frame or in the syndrome-only sweep):
// phi(|M|) and the signs in registers, E_new = sign * phi(S - phi(|M_i|)).
// Returns the row parity of the hard decisions (L < 0).
// CN = kCnNms / kCnOms: the min-sum rule instead (the two smallest |M| and the
// argmin in registers; param = alpha / beta).
template <int kDeg, int CN>
__device__ __forceinline__ uint32_t phys_row(float *__restrict__ Et, int beg, int deg, const float (&Lc)[kDeg],
                                             const float (&Eo)[kDeg], bool first, bool live, bool syn_only,
                                             float param) {
    uint32_t hp = 0u, sg = 0u;
    if constexpr (CN != kCnSpa) {
        MinPair mp;
#pragma unroll
        for (int i = 0; i < kDeg; ++i) {
            if (i < deg) {
                hp ^= Lc[i] < 0.0f ? 1u : 0u;
                if (!syn_only) {
                    const float M = (first || !live) ? Lc[i] : Lc[i] - Eo[i];
                    mp.add(fabsf(M), i);
                    sg |= (M < 0.0f ? 1u : 0u) << i;
                }
            }
        }
        if (!syn_only && live) {
            const uint32_t neg = __popc(sg) & 1u;
            const float m1 = ms_scale<CN>(mp.min1, param), m2 = ms_scale<CN>(mp.min2, param);
#pragma unroll
            for (int i = 0; i < kDeg; ++i) {
                if (i < deg) {
                    const float mag = i == mp.arg ? m2 : m1;
                    st_e32(&Et[(beg + i) * kTile], ((neg ^ (sg >> i)) & 1u) ? -mag : mag);
                }
            }
        }
        return hp;
    }
    float ph[kDeg];
    float S = 0.0f;
#pragma unroll
    for (int i = 0; i < kDeg; ++i) {
        if (i < deg) {
            hp ^= Lc[i] < 0.0f ? 1u : 0u;
            if (!syn_only) {
                const float M = (first || !live) ? Lc[i] : Lc[i] - Eo[i];
                ph[i] = phi(fabsf(M));
                S += ph[i];
                sg |= (M < 0.0f ? 1u : 0u) << i;
            }
        }
    }
    if (!syn_only && live) {
        const uint32_t neg = __popc(sg) & 1u;
#pragma unroll
        for (int i = 0; i < kDeg; ++i) {
            if (i < deg) {
                const float mag = phi(fmaxf(S - ph[i], 0.0f));
                st_e32(&Et[(beg + i) * kTile], ((neg ^ (sg >> i)) & 1u) ? -mag : mag);
            }
        }
    }
    return hp;
}

// A wavefront takes kRowsPerWave rows of one tile, one after the other: rows
// of degree <= kDeg with their gathers and E_old loads issued together
// (phys_row), longer rows in two sweeps with M recomputed (same values).
// (Batching the loads of 2 or 4 rows before any row's math measured 1.5-3 %
// slower once phi was cheap: the extra registers cost occupancy,
// profiles/r6_ab/r6e_c5.)
template <int kDeg, int CN>
__global__ __launch_bounds__(256) void phys_cn_tile_kernel(DevGraph g, DevState st, PhysTile pt, int it,
                                                           int syn_only, int per_tile, int items,
                                                           const int *__restrict__ row_ptr,
                                                           const int *__restrict__ col_idx, float param) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
    int tile, part;
    xcd_item(item, per_tile, tile, part);
    if (tile >= st.ntiles || !st.tile_active[tile]) continue;
    const int f = tile * kTile + lane;
    const bool live = st.done[f] == 0;
    const float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    float *Et = pt.E + (size_t)tile * g.nnz * kTile + lane;
    const bool first = it == 0;
    const bool readE = !first && !syn_only && live;
    uint32_t bad = 0u;
    const int r0 = (part * 4 + wave) * kRowsPerWave;
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
        const int r = r0 + rr;
        if (r >= g.m) break;
        const int beg = row_ptr[r], deg = row_ptr[r + 1] - beg;
        if (deg <= kDeg) {
            float Lc[kDeg], Eo[kDeg];
            // lane-masked loads: a tile with few running frames moves only
            // their sectors, not 256 B per wavefront access
#pragma unroll
            for (int i = 0; i < kDeg; ++i) {
                Lc[i] = 0.0f;
                Eo[i] = 0.0f;
                if (i < deg) {
                    if (live) Lc[i] = Lt[col_idx[beg + i] * kTile];
                    if (readE) Eo[i] = ld_e32(&Et[(beg + i) * kTile]);
                }
            }
            bad |= phys_row<kDeg, CN>(Et, beg, deg, Lc, Eo, first, live, syn_only != 0, param);
        } else {
            const int end = beg + deg;
            uint32_t hp = 0u;
            [[maybe_unused]] float S = 0.0f;
            uint32_t neg = 0u;
            [[maybe_unused]] MinPair mp;
            for (int e = beg; e < end; ++e) {
                const float Lc = live ? Lt[col_idx[e] * kTile] : 0.0f;
                hp ^= Lc < 0.0f ? 1u : 0u;
                if (!syn_only) {
                    const float M = (first || !live) ? Lc : Lc - Et[e * kTile];
                    if constexpr (CN == kCnSpa) S += phi(fabsf(M));
                    else mp.add(fabsf(M), e);
                    neg ^= (M < 0.0f) ? 1u : 0u;
                }
            }
            if (!syn_only && live) {
                for (int e = beg; e < end; ++e) {
                    const float Lc = Lt[col_idx[e] * kTile];
                    const float M = first ? Lc : Lc - ld_e32(&Et[e * kTile]);
                    float mag;
                    if constexpr (CN == kCnSpa) mag = phi(fmaxf(S - phi(fabsf(M)), 0.0f));
                    else mag = ms_scale<CN>(mp.other(e), param);
                    st_e32(&Et[e * kTile], ((neg ^ ((M < 0.0f) ? 1u : 0u)) != 0u) ? -mag : mag);
                }
            }
            bad |= hp;
        }
    }
    // syndrome of the posterior of iteration it-1 (none before iteration 0)
    if (it >= 1 && live && bad) pt.bad[(it & 1) * pt.cap + f] = 1;
    }
}

// A wavefront takes kColsPerWave columns of one tile: L = Lambda + E_0 + E_1
// + ... in CSC order.  With every column of degree <= kCD (template; 0 = the
// plain loop for any degree), all the wavefront's message loads -- up to
// 8 x kCD -- are issued before the first sum (the per-column loop waited one
// memory latency per message: each add needs its load).
template <int kCD>
__global__ __launch_bounds__(256) void phys_vn_tile_kernel(DevGraph g, DevState st, PhysTile pt, int it,
                                                           int per_tile, int items, const int *__restrict__ csc_ptr,
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
    const bool conv_now = live && it >= 1 && pt.bad[(it & 1) * pt.cap + f] == 0;
    const bool upd = live && !conv_now;
    const float *Et = pt.E + (size_t)tile * g.nnz * kTile + lane;
    float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
    const float *Lamt = pt.Lam + (size_t)tile * g.n * kTile + lane;
    if (__ballot(upd) != 0ull) {
        const int j0 = (part * 4 + wave) * kColsPerWave;
        const int j1 = min(g.n, j0 + kColsPerWave);
        uint32_t hb = 0u;  // this lane's hard decisions of the 8 columns (early syndrome)
        if constexpr (kCD > 0) {
            // batches of CB columns (CB x kCD loads in flight; more batch
            // columns spill the uniform edge indices)
            constexpr int CB = kVnBatch;
#pragma unroll
            for (int b = 0; b < kColsPerWave / CB; ++b) {
                float Ev[CB][kCD], La[CB];
                int p0[CB], cd[CB];
#pragma unroll
                for (int q = 0; q < CB; ++q) {
                    const int j = j0 + b * CB + q;
                    p0[q] = j < j1 ? csc_ptr[j] : 0;
                    cd[q] = j < j1 ? csc_ptr[j + 1] - p0[q] : 0;
                }
                // lane-masked: converged / finished frames move no data.  Lambda
                // for every column below n: one without edges keeps L = Lambda
#pragma unroll
                for (int q = 0; q < CB; ++q) {
                    La[q] = 0.0f;
                    if (upd && j0 + b * CB + q < j1) La[q] = Lamt[(j0 + b * CB + q) * kTile];
#pragma unroll
                    for (int i = 0; i < kCD; ++i) {
                        Ev[q][i] = 0.0f;
                        if (upd && i < cd[q]) Ev[q][i] = ld_e32(&Et[csc_edge[p0[q] + i] * kTile]);
                    }
                }
#pragma unroll
                for (int q = 0; q < CB; ++q) {
                    float sum = La[q];
#pragma unroll
                    for (int i = 0; i < kCD; ++i)
                        if (i < cd[q]) sum += Ev[q][i];
                    if (upd && j0 + b * CB + q < j1) Lt[(j0 + b * CB + q) * kTile] = sum;
                    hb |= (sum < 0.0f ? 1u : 0u) << (b * CB + q);
                }
            }
        } else {
            for (int j = j0; j < j1; ++j) {
                if (upd) {
                    float sum = Lamt[j * kTile];
                    for (int p = csc_ptr[j]; p < csc_ptr[j + 1]; ++p) sum += ld_e32(&Et[csc_edge[p] * kTile]);
                    Lt[j * kTile] = sum;
                    hb |= (sum < 0.0f ? 1u : 0u) << (j - j0);
                }
            }
        }
        if (j0 < g.n && upd) pt.zb[((size_t)tile * ((g.n + 7) >> 3) + (j0 >> 3)) * kTile + lane] = (uint8_t)hb;
    }
    if (part == 0 && wave == 0) {
        if (conv_now) {  // syndrome of iteration it-1 was zero
            st.done[f] = 1;
            st.conv[f] = it - 1;
            st.status[f] = 0;
            st.iters[f] = it;
        }
        pt.bad[((it + 1) & 1) * pt.cap + f] = 0;  // for the next CN sweep
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

// Early syndrome: the row parities of the hard decisions VN(it) just wrote
// (pt.zb: one byte per 8 columns, kColsPerWave == 8), one wavefront per
// (tile, 4 rows) like phys_cn_tile, into bad[(it+1)&1] -- the flag CN(it+1)
// would set from the same posterior.  Then phys_tile_exit stops the frames
// whose flag stayed 0: converged at iteration it (the exit VN(it+1) would have
// taken, one CN sweep earlier).  Only the running frames' bytes are current.
static_assert(kColsPerWave == 8, "one hard-decision byte per VN wavefront");
__global__ __launch_bounds__(256) void phys_tile_syn_kernel(DevGraph g, DevState st, PhysTile pt, int it,
                                                            int per_tile, int items, const int *__restrict__ row_ptr,
                                                            const int *__restrict__ col_idx) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    const size_t nb = (size_t)(g.n + 7) >> 3;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        int tile, part;
        xcd_item(item, per_tile, tile, part);
        if (tile >= st.ntiles || !st.tile_active[tile]) continue;
        const int f = tile * kTile + lane;
        const bool live = st.done[f] == 0;
        if (__ballot(live) == 0ull) continue;
        const uint8_t *zt = pt.zb + (size_t)tile * nb * kTile + lane;
        uint32_t bad = 0u;
        const int r0 = (part * 4 + wave) * kRowsPerWave;
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            const int r = r0 + rr;
            if (r >= g.m) break;
            uint32_t hp = 0u;
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                const int c = col_idx[e];
                hp ^= ((uint32_t)zt[(size_t)(c >> 3) * kTile] >> (c & 7)) & 1u;
            }
            bad |= hp;
        }
        if (live && bad) pt.bad[((it + 1) & 1) * pt.cap + f] = 1;
    }
}

// ------------------------------------------- layered min-sum on the tiles
// The layered schedule (phys_layered.hip's arithmetic, operation for
// operation: bit-identical) with E32 / L32 in HBM.  One launch per layer and
// iteration; stream order is the ordering between layers.  A wavefront takes
// kRowsPerWave rows of the layer, layer_rows[lbeg + ...]: rows of one layer
// share no column, so no two wavefronts of a launch touch the same L or E
// element.  Per row of degree <= kDeg every gather of L[c_e] and every E_e
// load is issued first, Q = L[c_e] - E_e stays in registers with the sign
// word and the two smallest |Q|, then E_e = R_e and L[c_e] = Q_e + R_e are
// stored: 16 B/edge.  Longer rows take two sweeps, Q recomputed in the second
// from the L and E the first one read (a row's columns are distinct).
// Iteration 0 does not read E (Q = L), and every edge of a running frame is
// written once per iteration: E needs no memset, and a compaction move (after
// a poll, so after a whole iteration) copies written messages only.  Only the
// lanes of running frames load or store: a stopped frame's L is its posterior.
template <int kDeg, int CN>
__global__ __launch_bounds__(256) void phys_layer_tile_kernel(DevGraph g, DevState st, PhysTile pt, int it, int lbeg,
                                                              int lrows, int per_tile, int items,
                                                              const int *__restrict__ row_ptr,
                                                              const int *__restrict__ col_idx,
                                                              const int *__restrict__ layer_rows, float param) {
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
        float *Lt = pt.L + (size_t)tile * g.n * kTile + lane;
        float *Et = pt.E + (size_t)tile * g.nnz * kTile + lane;
        const int i0 = (part * 4 + wave) * kRowsPerWave;
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            if (i0 + rr >= lrows) break;
            const int r = uniform(layer_rows[lbeg + i0 + rr]);
            const int beg = row_ptr[r], deg = row_ptr[r + 1] - beg;
            if (deg <= kDeg) {
                float Q[kDeg], Eo[kDeg];
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    Q[i] = 0.0f;
                    Eo[i] = 0.0f;
                    if (i < deg && live) {
                        Q[i] = Lt[col_idx[beg + i] * kTile];
                        if (!first) Eo[i] = ld_e32(&Et[(beg + i) * kTile]);
                    }
                }
                MinPair mp;
                uint32_t sg = 0u;
#pragma unroll
                for (int i = 0; i < kDeg; ++i) {
                    if (i < deg) {
                        if (!first) Q[i] = Q[i] - Eo[i];
                        mp.add(fabsf(Q[i]), i);
                        sg |= (Q[i] < 0.0f ? 1u : 0u) << i;
                    }
                }
                if (live) {
                    const uint32_t neg = __popc(sg) & 1u;
                    const float m1 = ms_scale<CN>(mp.min1, param), m2 = ms_scale<CN>(mp.min2, param);
#pragma unroll
                    for (int i = 0; i < kDeg; ++i) {
                        if (i < deg) {
                            const float mag = i == mp.arg ? m2 : m1;
                            const float R = ((neg ^ (sg >> i)) & 1u) ? -mag : mag;
                            st_e32(&Et[(beg + i) * kTile], R);
                            Lt[col_idx[beg + i] * kTile] = Q[i] + R;
                        }
                    }
                }
            } else if (live) {
                const int end = beg + deg;
                MinPair mp;
                uint32_t neg = 0u;
                for (int e = beg; e < end; ++e) {
                    const float Lc = Lt[col_idx[e] * kTile];
                    const float Qe = first ? Lc : Lc - Et[e * kTile];
                    mp.add(fabsf(Qe), e);
                    neg ^= (Qe < 0.0f) ? 1u : 0u;
                }
                for (int e = beg; e < end; ++e) {
                    const int c = col_idx[e];
                    const float Lc = Lt[c * kTile];
                    const float Qe = first ? Lc : Lc - ld_e32(&Et[e * kTile]);
                    const float mag = ms_scale<CN>(mp.other(e), param);
                    const float R = ((neg ^ ((Qe < 0.0f) ? 1u : 0u)) != 0u) ? -mag : mag;
                    st_e32(&Et[e * kTile], R);
                    Lt[c * kTile] = Qe + R;
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_phys_tile_init(const DevGraph &g, const DevState &st, const PhysTile &pt, bool convert,
                                 hipStream_t s) {
    const size_t total = convert ? std::max((size_t)st.ntiles * g.n * kTile, (size_t)st.ntiles * kTile)
                                 : (size_t)st.ntiles * kTile;
    phys_tile_init_kernel<<<grid_for(total, 256), 256, 0, s>>>(g, st, pt, convert ? 1 : 0);
    return hipGetLastError();
}

namespace {

template <int CN>
void launch_cn_tile_rule(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, bool syn_only,
                         float param, hipStream_t s) {
    const int per_tile = rows_per_tile(g.m);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    for_row_deg(g.max_row_deg, [&](auto deg) {
        phys_cn_tile_kernel<decltype(deg)::value, CN><<<stride_grid(items), 256, 0, s>>>(
            g, st, pt, it, syn_only ? 1 : 0, per_tile, items, g.row_ptr, g.col_idx, param);
    });
}

}  // namespace

hipError_t launch_phys_tile_cn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, bool syn_only,
                               hipStream_t s, const PhysRule &rule) {
    switch (rule.cn) {
    case kCnSpa: launch_cn_tile_rule<kCnSpa>(g, st, pt, it, syn_only, rule.param, s); break;
    case kCnNms: launch_cn_tile_rule<kCnNms>(g, st, pt, it, syn_only, rule.param, s); break;
    case kCnOms: launch_cn_tile_rule<kCnOms>(g, st, pt, it, syn_only, rule.param, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_phys_tile_vn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, int *active_count,
                               int max_iter, hipStream_t s) {
    const int per_tile = (g.n + 4 * kColsPerWave - 1) / (4 * kColsPerWave);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    if (g.max_col_deg <= 8)
        phys_vn_tile_kernel<8><<<stride_grid(items), 256, 0, s>>>(g, st, pt, it, per_tile, items, g.csc_ptr,
                                                                  g.csc_edge, active_count, max_iter);
    else
        phys_vn_tile_kernel<0><<<stride_grid(items), 256, 0, s>>>(g, st, pt, it, per_tile, items, g.csc_ptr,
                                                                  g.csc_edge, active_count, max_iter);
    return hipGetLastError();
}

hipError_t launch_phys_tile_syn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    const int per_tile = rows_per_tile(g.m);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    phys_tile_syn_kernel<<<stride_grid(items), 256, 0, s>>>(g, st, pt, it, per_tile, items, g.row_ptr, g.col_idx);
    return hipGetLastError();
}

namespace {

template <int CN>
void launch_layer_tile_rule(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, int lbeg, int lrows,
                            const PhysRule &rule, hipStream_t s) {
    const int per_tile = rows_per_tile(lrows);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    for_row_deg(g.max_row_deg, [&](auto deg) {
        phys_layer_tile_kernel<decltype(deg)::value, CN><<<stride_grid(items), 256, 0, s>>>(
            g, st, pt, it, lbeg, lrows, per_tile, items, g.row_ptr, g.col_idx, rule.layer_rows, rule.param);
    });
}

}  // namespace

hipError_t launch_phys_layer_tile(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, int lbeg,
                                  int lrows, hipStream_t s, const PhysRule &rule) {
    if (!rule.layer_rows || lbeg < 0 || lrows < 0 || lbeg + lrows > g.m) return hipErrorInvalidValue;
    if (lrows == 0 || st.ntiles <= 0) return hipSuccess;
    switch (rule.cn) {
    case kCnNms: launch_layer_tile_rule<kCnNms>(g, st, pt, it, lbeg, lrows, rule, s); break;
    case kCnOms: launch_layer_tile_rule<kCnOms>(g, st, pt, it, lbeg, lrows, rule, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ldpc
