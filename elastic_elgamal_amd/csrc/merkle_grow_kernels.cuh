// merkle_grow_kernels.cuh -- the grow entry of the receipt log (eg_merkle_grow, eg_hip.hip): the node store and the root of N leaves out
// of the node store of the first m, hashing only what an append can have changed.  The rule is in include/eg_hip.h, the plan (which
// tiles are copied, which are reduced, the rows of the copy) in merkle_grow_host.hpp.
//
//   k_merkle_grow_copy     ONE launch for every level: the nodes of the tiles that lie wholly inside the old tree, from their offset in the
//                          old store to their offset in the new one.  The rows come by value (at most 31); a lane moves 16 bytes when both
//                          stores are 16-byte aligned and one word otherwise, and walks on by the width of the grid
//   k_merkle_grow_tile<T>  k_merkle_tile with tile = tile0 + blockIdx.x: merkle_tile_step and MerkleTileDev as they are, the same launch
//                          shape; only the tiles from the first one that holds a changed node on
// Order on the one stream: the copy, then the tile launches bottom-up (a launch reads nodes of its input level that the copy moved and
// that the launch below made), then k_merkle_root.  Nothing is read below tile0 of a launch, nothing of the old store outside the rows.
// The lane body of the copy is a plain function over its memory, so that the host check build (tests/hostcheck/merklegrowcheck.cpp) runs
// the same code serially on arrays; the tiles are merkle_tile_step.  Everything is variable time: the log is public data.
#pragma once
#include "merkle_grow_host.hpp"
#include "merkle_kernels.cuh"

namespace eg {

// unit u of the copy: wide = the 16-byte half `u & 1` of node u >> 1, else word `u & 7` of node u >> 3, nodes counted through the rows in
// order.  Mem: move16(src_node, dst_node, half), move4(src_node, dst_node, word).  The row index is the same in every lane
template <class Mem>
EG_HD void merkle_lane_grow_copy(Mem& m, const egm::GrowTable& tab, uint64_t u, bool wide) {
  uint64_t rem = wide ? u >> 1 : u >> 3;
  if (rem >= tab.total) return;
  uint64_t src = 0, dst = 0;
  bool placed = false;
#pragma unroll 1
  for (uint32_t r = 0; r < tab.n_rows; ++r) {
    const uint64_t count = tab.row[r].count;
    if (!placed && rem < count) {
      src = tab.row[r].src + rem;
      dst = tab.row[r].dst + rem;
      placed = true;
    }
    if (!placed) rem -= count;
  }
  if (!placed) return;
  if (wide) m.move16(src, dst, (u32)(u & 1u));
  else m.move4(src, dst, (u32)(u & 7u));
}

}  // namespace eg

#if defined(__HIPCC__)

namespace eg {

constexpr unsigned MERKLE_GROW_COPY_BLOCKS = 1u << 16;      // the grid of the copy at the most: lanes walk on by its width

struct MerkleGrowCopyDev {
  const u32* src;                 // the old store
  u32* dst;                       // the new store
  __device__ __forceinline__ void move16(uint64_t s, uint64_t d, u32 half) {
    reinterpret_cast<uint4*>(dst)[d * 2 + half] = reinterpret_cast<const uint4*>(src)[s * 2 + half];
  }
  __device__ __forceinline__ void move4(uint64_t s, uint64_t d, u32 word) { dst[d * 8 + word] = src[s * 8 + word]; }
};
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_grow_copy(MerkleGrowCopyDev mem, egm::GrowTable tab, uint64_t units, int wide) {
  const uint64_t step = (uint64_t)gridDim.x * MERKLE_NT;
  for (uint64_t u = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x; u < units; u += step) merkle_lane_grow_copy(mem, tab, u, wide != 0);
}

// k_merkle_tile from tile0 on (merkle_kernels.cuh has the reasons for the launch shape).  tile0 comes FIRST: behind the tile arguments the
// same body takes 172 VGPR instead of k_merkle_tile's 156, and a third workgroup no longer fits a CU
template <int TL>
__global__ void __launch_bounds__(1 << (TL - 2)) k_merkle_grow_tile(u32 tile0, MerkleTileArgs a) {
  __shared__ u32 odd[8 << (TL - 1)];
  __shared__ u32 even[8 << (TL - 2)];
  MerkleTileDev<TL> mem{a, odd, even};
  const u32 tile = tile0 + blockIdx.x;             // below 2^21: a level has fewer than 2^31 nodes
  for (int s = 1; s <= a.steps; ++s) {
#pragma unroll 1
    for (u32 t = threadIdx.x; t < (1u << (TL - s)); t += 1u << (TL - 2)) merkle_tile_step<TL>(mem, tile, s, t, a.n_in);
    __syncthreads();
  }
}

}  // namespace eg
#endif
