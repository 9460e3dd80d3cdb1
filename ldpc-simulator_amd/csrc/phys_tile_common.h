// phys_tile_common.h -- what the HBM tile kernels of physical mode share
// (phys_tile.hip: fp32; phys_qtile.hip: fixed point): the work split of a
// wavefront, the XCD-aware placement of the work items and the launch sizes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

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

inline unsigned grid_for(size_t total, int block) { return (unsigned)((total + block - 1) / block); }
inline unsigned xcd_items(int ntiles, int per_tile) { return (unsigned)(((ntiles + 7) / 8) * 8 * per_tile); }
// 256 CUs x 16 blocks of 4 waves (a multiple of 8, see xcd_item)
inline unsigned stride_grid(int items) { return (unsigned)std::min(items, 4096); }

}  // namespace ldpc
