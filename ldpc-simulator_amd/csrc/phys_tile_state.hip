// phys_tile_state.hip -- the bookkeeping of physical mode's HBM tile decoders,
// gfx950: everything the fp32 family (phys_tile.hip) and the fixed-point one
// (phys_qtile.hip) do around their sweeps, once.
//
// Both keep a frame's state on 64-frame tiles, lane = frame: E [tile][nnz][64],
// L [tile][n][64], Lam [tile][n][64] (float / float / float or int8 / int16 /
// int8), with DevState's done / conv / status / iters / tile_active and the bad
// flags [2][cap].  done[]: 0 running, 1 finished (to be counted), 2 counted,
// moved away, or no frame.
//
//   exits       phys_tile_exit (flooding, after an early syndrome), phys_tile_final
//               (flooding, after the last one), phys_layer_exit (layered, every
//               iteration): DevState, bad and cap only.
//   syndrome    phys_lsyn_tile: the row parities of b = (L < 0) read from L
//               itself -> bad[slot][frame].  The layered exit of both families;
//               fixed-point flooding's early and last syndrome (the fp32
//               flooding sweeps form theirs on the way, phys_tile.hip).
//   out, count  the tiles to row-major z / post; main.py's counters and McStats.
//   compaction  (Monte-Carlo runs) after the finished frames were counted, mark
//               them counted; then move each running frame of the plan
//               (spa_kernels' compact plan: sources = running slots in tiles
//               >= nt, destinations = finished slots below) -- its lanes of E,
//               L, Lam and the u bits -- and reset the destination's per-frame
//               state.  Sources and destinations are disjoint, so the moves
//               need no ordering.
// The kernels that read the arrays are templates on the element types, both
// instances at the end of the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "phys_tile_common.h"
#include "spa_device.h"

namespace ldpc {
namespace {

// bit 31 = (x < 0): the hard decision, XOR-able over a row
__device__ __forceinline__ uint32_t sign_word(float x) { return x < 0.0f ? 0x80000000u : 0u; }
__device__ __forceinline__ uint32_t sign_word(int16_t x) { return (uint32_t)(int)x; }

// One wavefront per (tile, kRowsPerWave rows), placed as the check sweeps.
// Only the running frames' lanes load.
template <class TL>
__global__ __launch_bounds__(256) void phys_lsyn_tile_kernel(DevGraph g, DevState st, const TL *L, int *flags,
                                                             int cap, int slot, int per_tile, int items,
                                                             const int *__restrict__ row_ptr,
                                                             const int *__restrict__ col_idx) {
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        int tile, part;
        xcd_item(item, per_tile, tile, part);
        if (tile >= st.ntiles || !st.tile_active[tile]) continue;
        const int f = tile * kTile + lane;
        const bool live = st.done[f] == 0;
        if (__ballot(live) == 0ull) continue;
        const TL *Lt = L + (size_t)tile * g.n * kTile + lane;
        uint32_t bad = 0u;
        const int r0 = (part * 4 + wave) * kRowsPerWave;
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            const int r = r0 + rr;
            if (r >= g.m) break;
            uint32_t lx = 0u;
            if (live)
                for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) lx ^= sign_word(Lt[col_idx[e] * kTile]);
            bad |= lx >> 31;
        }
        if (live && bad) flags[slot * cap + f] = 1;
    }
}

// Flooding, after a syndrome into bad[(it+1)&1]: the running frames whose flag
// stayed 0 stop, converged at iteration it.
__global__ __launch_bounds__(64) void phys_tile_exit_kernel(DevState st, int *bad, int cap, int it,
                                                            int *active_count, int max_iter) {
    const int tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int f = tile * kTile + lane;
    const bool live = st.tile_active[tile] && st.done[f] == 0;
    const bool conv_now = live && bad[((it + 1) & 1) * cap + f] == 0;
    if (conv_now) {  // the syndrome of iteration it is zero
        st.done[f] = 1;
        st.conv[f] = it;
        st.status[f] = 0;
        st.iters[f] = it + 1;
    }
    const unsigned long long still = __ballot(live && !conv_now);
    if (lane == 0) {
        if (st.tile_active[tile]) st.tile_active[tile] = still != 0ull ? 1 : 0;
        if (still) {
            atomicAdd(&active_count[it], 1);
            atomicAdd(&active_count[max_iter + it], (int)__popcll(still));
        }
    }
}

// Flooding, after the syndrome of the last iteration's posterior ("iteration" max_iter)
__global__ void phys_tile_final_kernel(DevState st, int *bad, int cap, int max_iter) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= st.ntiles * kTile || st.done[f]) return;
    const bool ok = bad[(max_iter & 1) * cap + f] == 0;
    st.done[f] = 1;
    st.conv[f] = ok ? max_iter - 1 : -1;
    st.status[f] = ok ? 0 : 1;
    st.iters[f] = max_iter;
}

// Layered, after the syndrome into bad[0]: a running frame with no bad row
// stops, converged at it; after the last iteration the frames still running
// stop unconverged.  Runs every iteration, so the results never depend on when
// the host polls the running counts.
__global__ __launch_bounds__(64) void phys_layer_exit_kernel(DevState st, int *bad, int it, int *active_count,
                                                             int max_iter) {
    const int tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int f = tile * kTile + lane;
    const bool active = st.tile_active[tile] != 0;
    const bool live = active && st.done[f] == 0;
    const bool conv_now = live && bad[f] == 0;
    bad[f] = 0;  // for the next iteration's syndrome
    const bool last = it + 1 >= max_iter;
    if (conv_now) {
        st.done[f] = 1;
        st.conv[f] = it;
        st.status[f] = 0;
        st.iters[f] = it + 1;
    } else if (live && last) {
        st.done[f] = 1;
        st.conv[f] = -1;
        st.status[f] = 1;
        st.iters[f] = max_iter;
    }
    const unsigned long long still = __ballot(live && !conv_now && !last);
    if (lane == 0) {
        if (active) st.tile_active[tile] = still != 0ull ? 1 : 0;
        if (still) {
            atomicAdd(&active_count[it], 1);
            atomicAdd(&active_count[max_iter + it], (int)__popcll(still));
        }
    }
}

// L tiles -> row-major z = (L < 0 ? 0 : 1) (bit estimate ^ 1) and post
template <class TL>
__global__ void phys_tile_out_kernel(DevGraph g, DevState st, const TL *Lp, uint8_t *z, TL *post) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)st.count * g.n) return;
    const int f = (int)(i / g.n);
    const int j = (int)(i % g.n);
    const TL L = Lp[((size_t)(f >> 6) * g.n + j) * kTile + (f & 63)];
    if (z) z[i] = L < 0 ? 0 : 1;
    if (post) post[i] = L;
}

// main.py counters; block = one wavefront x (tile, 1024 info columns)
template <class TL>
__global__ __launch_bounds__(64) void phys_tile_count_kernel(DevGraph g, DevState st, const TL *L,
                                                             unsigned long long *ctr, McStats ms) {
    const int kw = (g.k + 31) >> 5;
    const int per_tile = (g.k + 1023) >> 10 > 0 ? (g.k + 1023) >> 10 : 1;
    const int tile = blockIdx.x / per_tile, part = blockIdx.x % per_tile;
    const int lane = threadIdx.x;
    const int f = tile * kTile + lane;
    const bool valid = st.done[f] == 1;  // finished and not counted yet (frame_reset, the compaction)
    const bool failed = valid && st.status[f] != 0;
    unsigned long long err = 0;
    // BER counts failed frames only (main.py:130-138); the statistics need the converged ones too
    const bool cmp = ms.hist ? valid : failed;
    if (__ballot(cmp) != 0ull) {
        const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lane;
        const TL *Lt = L + (size_t)tile * g.n * kTile + lane;
        const int j1 = min(g.k, (part + 1) * 1024);
        for (int j = part * 1024; j < j1; ++j) {
            const uint32_t u = (Ut[(j >> 5) * kTile] >> (j & 31)) & 1u;
            err += (u != (Lt[j * kTile] < 0 ? 1u : 0u)) ? 1 : 0;
        }
        if (!cmp) err = 0;
    }
    const unsigned long long e = wave_sum(failed ? err : 0ull);
    if (lane == 0 && e) atomicAdd(&ctr[2], e);
    if (ms.hist) mc_stats_tile(ms, st, tile, per_tile, lane, valid, failed, (int)err);
    if (part != 0) return;
    const int cv = valid ? st.conv[f] : -1;
    unsigned long long v[7] = {valid ? 1ull : 0ull, failed ? 1ull : 0ull, 0, cv >= 0 ? (unsigned long long)cv : 0,
                               cv >= 0 ? 1ull : 0ull, 0, valid ? (unsigned long long)st.iters[f] : 0};
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        if (i == 2 || i == 5) continue;
        const unsigned long long s = wave_sum(v[i]);
        if (lane == 0 && s) atomicAdd(&ctr[i], s);
    }
}

// McStats::slot_frame of a fresh chunk
__global__ void mc_stats_slots_kernel(long long *slot_frame, long long base, int count) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < count) slot_frame[f] = base + f;
}

__global__ void phys_mark_counted_kernel(DevState st) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < st.ntiles * kTile && st.done[f] == 1) st.done[f] = 2;
}
// Lam null: the family keeps no Lambda plane (fixed-point layered)
template <class TE, class TL, class TLam>
__global__ void phys_compact_move_kernel(DevGraph g, DevState st, TE *E, TL *L, TLam *Lam, int cap,
                                         const int *pairs) {
    const int P = pairs[0];
    const int kw = (g.k + 31) >> 5;
    const int64_t nlam = Lam ? g.n : 0;
    const int64_t items = (int64_t)g.nnz + g.n + nlam + kw;
    const int64_t total = (int64_t)P * items;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % P);  // pair-fastest: neighbouring lanes of one item
        int64_t it = i / P;
        const int src = pairs[1 + p], dst = pairs[1 + cap + p];
        const size_t sT = src >> 6, sl = src & 63, dT = dst >> 6, dl = dst & 63;
        if (it < g.nnz) {
            E[(dT * g.nnz + it) * kTile + dl] = E[(sT * g.nnz + it) * kTile + sl];
            continue;
        }
        it -= g.nnz;
        if (it < g.n) {
            L[(dT * g.n + it) * kTile + dl] = L[(sT * g.n + it) * kTile + sl];
            continue;
        }
        it -= g.n;
        if (it < nlam) {
            Lam[(dT * g.n + it) * kTile + dl] = Lam[(sT * g.n + it) * kTile + sl];
            continue;
        }
        it -= nlam;
        st.ubits[(dT * kw + it) * kTile + dl] = st.ubits[(sT * kw + it) * kTile + sl];
    }
}
__global__ void phys_compact_flags_kernel(DevState st, int *bad, int cap, const int *pairs, long long *slot_frame) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pairs[0]) return;
    const int src = pairs[1 + p], dst = pairs[1 + cap + p];
    if (slot_frame) slot_frame[dst] = slot_frame[src];  // the frame's global index moves with it
    frame_reset(st, bad, cap, dst, true);
    st.tile_active[dst >> 6] = 1;
    st.done[src] = 2;  // moved: nothing to count here
}

}  // namespace

template <class TL>
hipError_t launch_phys_tile_lsyn(const DevGraph &g, const DevState &st, const TL *L, int *bad, int cap, int slot,
                                 hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    const int per_tile = rows_per_tile(g.m);
    const int items = (int)xcd_items(st.ntiles, per_tile);
    phys_lsyn_tile_kernel<<<stride_grid(items), 256, 0, s>>>(g, st, L, bad, cap, slot, per_tile, items, g.row_ptr,
                                                             g.col_idx);
    return hipGetLastError();
}

hipError_t launch_phys_tile_exit(const DevState &st, int *bad, int cap, int it, int *active_count, int max_iter,
                                 hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(active_count + it, 0, sizeof(int), s)) return e;
    if (hipError_t e = hipMemsetAsync(active_count + max_iter + it, 0, sizeof(int), s)) return e;
    phys_tile_exit_kernel<<<st.ntiles, kTile, 0, s>>>(st, bad, cap, it, active_count, max_iter);
    return hipGetLastError();
}

hipError_t launch_phys_tile_final(const DevState &st, int *bad, int cap, int max_iter, hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    phys_tile_final_kernel<<<grid_for((size_t)st.ntiles * kTile, 256), 256, 0, s>>>(st, bad, cap, max_iter);
    return hipGetLastError();
}

template <class TL>
hipError_t launch_phys_layer_exit(const DevGraph &g, const DevState &st, const TL *L, int *bad, int cap, int it,
                                  int *active_count, int max_iter, hipStream_t s) {
    if (st.ntiles <= 0) return hipSuccess;
    if (hipError_t e = launch_phys_tile_lsyn(g, st, L, bad, cap, 0, s)) return e;
    phys_layer_exit_kernel<<<st.ntiles, kTile, 0, s>>>(st, bad, it, active_count, max_iter);
    return hipGetLastError();
}

template <class TL>
hipError_t launch_phys_tile_out(const DevGraph &g, const DevState &st, const TL *L, uint8_t *z, TL *post,
                                hipStream_t s) {
    const size_t total = (size_t)st.count * g.n;
    if (total && (z || post)) phys_tile_out_kernel<<<grid_for(total, 256), 256, 0, s>>>(g, st, L, z, post);
    return hipGetLastError();
}

template <class TL>
hipError_t launch_phys_tile_count(const DevGraph &g, const DevState &st, const TL *L, unsigned long long *ctr,
                                  hipStream_t s, const McStats &ms) {
    if (st.ntiles <= 0) return hipSuccess;
    const int per_tile = std::max(1, (g.k + 1023) >> 10);
    phys_tile_count_kernel<<<st.ntiles * per_tile, 64, 0, s>>>(g, st, L, ctr, ms);
    return hipGetLastError();
}

template <class TE, class TL, class TLam>
hipError_t launch_phys_compact(const DevGraph &g, const DevState &st, TE *E, TL *L, TLam *Lam, int *bad, int nt,
                               int cap, int *pairs, hipStream_t s, long long *slot_frame) {
    phys_mark_counted_kernel<<<grid_for((size_t)st.ntiles * kTile, 256), 256, 0, s>>>(st);
    if (hipError_t e = launch_compact_plan(st, nt, cap, pairs, s)) return e;
    phys_compact_move_kernel<<<2048, 256, 0, s>>>(g, st, E, L, Lam, cap, pairs);
    phys_compact_flags_kernel<<<grid_for((size_t)cap, 256), 256, 0, s>>>(st, bad, cap, pairs, slot_frame);
    return hipGetLastError();
}

hipError_t launch_mc_stats_slots(long long *slot_frame, long long base, int count, hipStream_t s) {
    if (!slot_frame || count <= 0) return hipSuccess;
    mc_stats_slots_kernel<<<grid_for((size_t)count, 256), 256, 0, s>>>(slot_frame, base, count);
    return hipGetLastError();
}

// the two families: fp32 (PhysTile) and fixed point (QTile)
#define LDPC_TILE_STATE(TE, TL, TLam)                                                                                 \
    template hipError_t launch_phys_tile_lsyn(const DevGraph &, const DevState &, const TL *, int *, int, int,        \
                                              hipStream_t);                                                           \
    template hipError_t launch_phys_layer_exit(const DevGraph &, const DevState &, const TL *, int *, int, int,       \
                                               int *, int, hipStream_t);                                              \
    template hipError_t launch_phys_tile_out(const DevGraph &, const DevState &, const TL *, uint8_t *, TL *,         \
                                             hipStream_t);                                                            \
    template hipError_t launch_phys_tile_count(const DevGraph &, const DevState &, const TL *, unsigned long long *,  \
                                               hipStream_t, const McStats &);                                         \
    template hipError_t launch_phys_compact(const DevGraph &, const DevState &, TE *, TL *, TLam *, int *, int, int,  \
                                            int *, hipStream_t, long long *);
LDPC_TILE_STATE(float, float, float)
LDPC_TILE_STATE(int8_t, int16_t, int8_t)
#undef LDPC_TILE_STATE

}  // namespace ldpc
