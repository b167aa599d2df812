// scan.cuh -- the exclusive prefix sum of SEQ sequences of 32-bit words at once, in three launches; every pass that ranks or compacts
// (pippenger.cuh, group_tally_kernels.cuh, weed_kernels.cuh, roll_kernels.cuh, merkle_kernels.cuh) wraps these bodies in kernels of its own:
//   scan_tile_sums   <<<tiles, SCAN_NT>>>     the sums of every tile of SCAN_TILE elements -> tile_sums[tile * SEQ + k]
//   scan_tops        <<<1, 64 * SEQ>>>        wavefront k turns the tile sums of sequence k into exclusive offsets, in place, and returns
//                                             the total to all its lanes; what becomes of the total is the caller's epilogue
//   scan_apply       <<<tiles, SCAN_NT>>>     the scan inside every tile: a lane gets the words of its SCAN_PER_LANE elements and the sums
//                                             of every sequence over the elements before its first one
// An element's contribution comes from a loader, load(v, i): the SEQ words of element i, zeros for i beyond the end (the loader knows the
// end).  It is called twice per element (sums, apply) and must answer the same both times.  What is written back is the caller's loop over
// its elements scan_element(0 .. SCAN_PER_LANE - 1), which adds v[e] to run as it goes.  (A writer functor in its place costs the kernels
// whose outputs are a struct of pointers some twenty scalar registers: the struct's address is taken, so it is copied whole at the start.)
#pragma once
#include <hip/hip_runtime.h>
#include "scan_host.hpp"

namespace eg {

constexpr int SCAN_NT = 256;           // lanes per block
constexpr int SCAN_PER_LANE = 4;       // consecutive elements of one lane
static_assert(SCAN_NT * SCAN_PER_LANE == egscan::SCAN_TILE, "a block scans one tile");
static_assert(SCAN_NT == 4 * 64, "four wavefronts: the tile sum adds four partials");

__device__ __forceinline__ uint32_t scan_element(int e) { return blockIdx.x * egscan::SCAN_TILE + threadIdx.x * SCAN_PER_LANE + e; }

template <int SEQ, class Load>
__device__ __forceinline__ void scan_tile_sums(uint32_t* tile_sums, Load load) {
  __shared__ uint32_t red[SEQ][SCAN_NT / 64];
  uint32_t sum[SEQ];
#pragma unroll
  for (int k = 0; k < SEQ; ++k) sum[k] = 0u;
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    uint32_t v[SEQ];
    load(v, scan_element(e));
#pragma unroll
    for (int k = 0; k < SEQ; ++k) sum[k] += v[k];
  }
#pragma unroll
  for (int k = 0; k < SEQ; ++k) {
    uint32_t x = sum[k];
    for (int off = 32; off >= 1; off >>= 1) x += (uint32_t)__shfl_down((int)x, off, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if (threadIdx.x < SEQ) tile_sums[blockIdx.x * SEQ + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

template <int SEQ>
__device__ __forceinline__ uint32_t scan_tops(uint32_t n_tiles, uint32_t* tile_sums) {
  const int k = SEQ > 1 ? threadIdx.x >> 6 : 0, lane = threadIdx.x & 63;
  uint32_t run = 0;
  for (uint32_t b0 = 0; b0 < n_tiles; b0 += 64) {
    const uint32_t b = b0 + lane;
    const uint32_t v = b < n_tiles ? tile_sums[b * SEQ + k] : 0u;
    uint32_t x = v;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64); if (lane >= off) x += y; }
    if (b < n_tiles) tile_sums[b * SEQ + k] = run + x - v;
    run += (uint32_t)__shfl((int)x, 63, 64);
  }
  return run;
}

template <int SEQ, class Load>
__device__ __forceinline__ void scan_apply(const uint32_t* tile_sums, Load load, uint32_t (&v)[SCAN_PER_LANE][SEQ], uint32_t (&run)[SEQ]) {
  __shared__ uint32_t part[SEQ][SCAN_NT];
  uint32_t sum[SEQ];
#pragma unroll
  for (int k = 0; k < SEQ; ++k) sum[k] = 0u;
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    load(v[e], scan_element(e));
#pragma unroll
    for (int k = 0; k < SEQ; ++k) sum[k] += v[e][k];
  }
#pragma unroll
  for (int k = 0; k < SEQ; ++k) part[k][threadIdx.x] = sum[k];
  __syncthreads();
  for (int d = 1; d < SCAN_NT; d <<= 1) {         // Hillis-Steele inclusive scan over the 256 lanes, all sequences together
    uint32_t add[SEQ];
#pragma unroll
    for (int k = 0; k < SEQ; ++k) add[k] = (int)threadIdx.x >= d ? part[k][threadIdx.x - d] : 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SEQ; ++k) part[k][threadIdx.x] += add[k];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < SEQ; ++k) run[k] = tile_sums[blockIdx.x * SEQ + k] + (threadIdx.x ? part[k][threadIdx.x - 1] : 0u);
}

}  // namespace eg
