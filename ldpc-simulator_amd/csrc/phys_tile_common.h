// phys_tile_common.h -- what the HBM tile kernels of physical mode share
// (phys_tile.hip: fp32; phys_qtile.hip: fixed point): the work split of a
// wavefront, the XCD-aware placement of the work items, the launch sizes, the
// kDeg dispatch of the row kernels and the reset of a slot's per-frame state.
// The bookkeeping kernels of both families -- exits, final, syndrome from L,
// out, count, compaction -- are in phys_tile_state.hip, once.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "spa_device.h"

namespace ldpc {

constexpr int kRowsPerWave = 4;
constexpr int kColsPerWave = 8;

__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Work item i = (tile, part).  Blocks b and b+8 run on the same XCD; the grid
// is a multiple of 8 and block b takes items b, b+G, b+2G, ... so every item
// of a block -- and every part of one tile -- has the same i%8 = tile%8: a
// tile's L rows stay in one XCD's L2.  A grid of a few thousand blocks makes
// a launch over finished tiles cost a few microseconds, not one block per item.
__device__ __forceinline__ void xcd_item(int i, int per_tile, int &tile, int &part) {
    const int slot = i >> 3;
    tile = (slot / per_tile) * 8 + (i & 7);
    part = slot % per_tile;
}

// Monte-Carlo statistics (McStats) of the frames a count kernel counts: one
// wavefront per (tile, 1024 info columns), lane = slot of `tile`.  `valid`:
// the slot's frame is finished and not counted yet (the same in every block of
// the tile), so a frame is binned exactly once, at the end of its chunk or
// before a compaction.  `err`: the info-bit errors of the lane's frame in this
// block's columns -- with statistics on the count kernels compare every valid
// lane, not only the failed ones: a converged frame that differs is an
// undetected error.  The blocks of a tile add their shares to slot_err; the
// one that arrives last (tile_arrive) takes the sums, leaves both arrays zero
// and bins the tile's frames, each distinct bin with one atomic.
__device__ __forceinline__ void mc_stats_tile(const McStats &ms, const DevState &st, int tile, int per_tile, int lane,
                                              bool valid, bool failed, int err) {
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) return;
    const int f = tile * kTile + lane;
    long long total = valid ? err : 0;
    if (per_tile > 1) {
        if (valid && err) atomicAdd(&ms.slot_err[f], err);
        __threadfence();
        int seen = 0;
        if (lane == 0) seen = atomicAdd(&ms.tile_arrive[tile], 1);
        if (__shfl(seen, 0) != per_tile - 1) return;
        __threadfence();
        if (lane == 0) atomicExch(&ms.tile_arrive[tile], 0);
        total = valid ? atomicExch(&ms.slot_err[f], 0) : 0;
    }
    const int cv = valid && !failed ? st.conv[f] : ms.max_iter;
    const int bin = min(max(cv, 0), ms.max_iter);
    unsigned long long todo = vmask;
    while (todo) {
        const int b = __shfl(bin, __ffsll(todo) - 1);
        const unsigned long long same = __ballot(valid && bin == b);
        if (lane == 0) atomicAdd(&ms.hist[b], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
    const bool und = valid && !failed && total != 0;
    const unsigned long long uf = wave_sum(und ? 1ull : 0ull), ub = wave_sum(und ? (unsigned long long)total : 0ull);
    if (lane == 0 && uf) {
        atomicAdd(&ms.und[0], uf);
        atomicAdd(&ms.und[1], ub);
    }
    if (failed) {
        const unsigned long long i = atomicAdd(&ms.und[2], 1ull);
        if (i < (unsigned long long)ms.max_failed) {
            ms.failed[2 * i] = ms.slot_frame[f];
            ms.failed[2 * i + 1] = total;
        }
    }
}

// Slot f before its frame's first sweep (the init kernels; the destination of
// a compaction move): running, or without a frame (done = 2: never counted).
// The caller sets tile_active.
__device__ __forceinline__ void frame_reset(const DevState &st, int *bad, int cap, int f, bool valid) {
    st.done[f] = valid ? 0 : 2;
    st.conv[f] = -1;
    st.status[f] = 1;
    st.iters[f] = 0;
    bad[f] = 0;
    bad[cap + f] = 0;
}

inline unsigned grid_for(size_t total, int block) { return (unsigned)((total + block - 1) / block); }
inline unsigned xcd_items(int ntiles, int per_tile) { return (unsigned)(((ntiles + 7) / 8) * 8 * per_tile); }
// 256 CUs x 16 blocks of 4 waves (a multiple of 8, see xcd_item)
inline unsigned stride_grid(int items) { return (unsigned)std::min(items, 4096); }
// work items of a tile in a row sweep: a block of 4 wavefronts takes 4 kRowsPerWave rows
inline int rows_per_tile(int rows) { return (rows + 4 * kRowsPerWave - 1) / (4 * kRowsPerWave); }

// f(std::integral_constant<int, kDeg>) for the row kernels' kDeg of a graph:
// the smallest of 8 / 16 / 32 that holds max_row_deg, 32 for any longer row
template <class F>
void for_row_deg(int max_row_deg, F &&f) {
    if (max_row_deg <= 8) f(std::integral_constant<int, 8>{});
    else if (max_row_deg <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}

}  // namespace ldpc
