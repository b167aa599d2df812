// merkle_audit_kernels.cuh -- the audit entries of the receipt log (eg_merkle_heads / _consistency / _consistency_check, eg_hip.hip):
// the heads the log had at earlier sizes, consistency proofs between an earlier size and the present one, and the check of many such
// proofs.  The rule is in include/eg_hip.h, the arithmetic in merkle_audit_host.hpp.  Nothing is added to the tree: every node that is
// needed is in the node store that k_merkle_tile writes (merkle_kernels.cuh).
//
//   k_merkle_heads         one lane = one earlier size: the complete subtrees that the bits of the size name, folded on the left; at most
//                          depth(N) node hashes
//   k_merkle_consistency   one lane = one earlier size: a gather out of the log and the node store, as k_merkle_paths
//   k_merkle_cons_check    one lane = one proof: two hash chains (the old root fr, the new root sr) that share every sibling; the new
//                          root's chain runs at every step and the old root's beside it where the sibling lies on the left
// The lane bodies are plain functions over their memory, so that the host check build (tests/hostcheck/merkleauditcheck.cpp) runs the same
// code serially on arrays.  Every loop is bounded by MAX_DEPTH + 1.  Everything is variable time: the log is public data.
#pragma once
#include "merkle_audit_host.hpp"
#include "merkle_kernels.cuh"

namespace eg {

// Mem: size(j), node(level, off, idx, w) as for the paths, head_put(j, w), head_zero(j).  Returns whether the size lies above N
template <class Mem>
EG_HD bool merkle_lane_head(Mem& m, uint64_t j, uint64_t n_leaves) {
  uint64_t x = m.size(j);
  if (x > n_leaves) { m.head_zero(j); return true; }
  u32 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (x == 0) merkle_empty_root(acc);
  bool first = true;
  uint64_t off = 0, n = n_leaves;
  for (int level = 0; level <= egm::MAX_DEPTH && x; ++level) {
    if (x & 1u) {                                  // node (level, x - 1): a complete subtree that lies wholly inside the first size leaves
      u32 w[8];
      m.node(level, off, x - 1u, w);
      if (first) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = w[q];
      } else {
        merkle_node(acc, w, acc);
      }
      first = false;
    }
    if (level >= 1) off += n;
    x >>= 1;
    n = (n + 1) >> 1;
  }
  m.head_put(j, acc);
  return false;
}

// Mem: node(level, off, idx, w), proof_put(j, k, w), proof_zero(j, k).  `row` = depth(N) + 1 entries.  Returns proof_len
template <class Mem>
EG_HD uint32_t merkle_lane_consistency(Mem& m, uint64_t j, uint64_t old, uint64_t n_leaves, int row) {
  uint32_t len = 0;
  const bool known = old >= 1 && old <= n_leaves;
  if (known && old < n_leaves) {
    const int first = egm::seed_level(old);
    uint64_t node = (old >> first) - 1u;            // old = (node + 1) 2^first
    uint64_t off = 0, n = n_leaves;
    for (int level = 0; level <= egm::MAX_DEPTH && n > 1; ++level) {
      if (level >= first) {
        u32 w[8];
        if (level == first && node) {              // the seed: the last complete piece of the old tree
          m.node(level, off, node, w);
          m.proof_put(j, len++, w);
        }
        if ((node ^ 1u) < n) {
          m.node(level, off, node ^ 1u, w);
          m.proof_put(j, len++, w);
        }
        node >>= 1;
      }
      if (level >= 1) off += n;
      n = (n + 1) >> 1;
    }
  }
  for (uint32_t k = len; k < (uint32_t)row; ++k) m.proof_zero(j, k);
  return known ? len : egm::NO_PATH;
}

// Mem: old_size(j), proof_len(j), old_root(j, w), proof(j, k, w), root(w).  The verdict: the first failure in the order index, length,
// old root, new root; no proof byte is read unless the length is the one that (old_size, N) demands
template <class Mem>
EG_HD uint32_t merkle_lane_cons_check(const Mem& m, uint64_t j, uint64_t n_leaves) {
  const uint64_t old = m.old_size(j);
  if (old == 0 || old > n_leaves) return egm::MERKLE_BAD_INDEX;
  if (m.proof_len(j) != egm::consistency_len(old, n_leaves)) return egm::MERKLE_BAD_LENGTH;
  u32 fr[8], sr[8], c[8];
  m.old_root(j, fr);
  if (old < n_leaves) {
    const int first = egm::seed_level(old);
    uint64_t node = (old >> first) - 1u;
    uint32_t k = 0;
    if (node) m.proof(j, k++, fr);                  // the seed; without one the old tree is node (first, 0): the old root itself
#pragma unroll
    for (int q = 0; q < 8; ++q) sr[q] = fr[q];
    uint64_t n = egm::level_count(n_leaves, first);
    for (int level = first; level <= egm::MAX_DEPTH && n > 1; ++level, n = (n + 1) >> 1, node >>= 1) {
      if ((node ^ 1u) >= n) continue;
      m.proof(j, k++, c);
      const bool left = (node & 1u) != 0;          // the sibling lies on the left: it belongs to the old tree as well
      u32 l[8], r[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { l[q] = left ? c[q] : sr[q]; r[q] = left ? sr[q] : c[q]; }
      merkle_node(sr, l, r);
      if (left) merkle_node(fr, c, fr);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) sr[q] = fr[q];
  }
  m.old_root(j, c);
  u32 diff = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) diff |= fr[q] ^ c[q];
  if (diff) return egm::MERKLE_MISMATCH_OLD;
  m.root(c);
#pragma unroll
  for (int q = 0; q < 8; ++q) diff |= sr[q] ^ c[q];
  return diff ? egm::MERKLE_MISMATCH : 0u;
}

}  // namespace eg

#if defined(__HIPCC__)

namespace eg {

struct MerkleHeadDev {
  const unsigned long long* size_;
  const u32* log;
  const u32* store;
  u32* heads;
  __device__ __forceinline__ uint64_t size(uint64_t j) const { return size_[j]; }
  __device__ __forceinline__ void node(int level, uint64_t off, uint64_t idx, u32 w[8]) const {
    merkle_ld8(w, level ? store + (off + idx) * 8 : log + idx * 8);
  }
  __device__ __forceinline__ void head_put(uint64_t j, const u32 w[8]) { merkle_st8(heads + j * 8, w); }
  __device__ __forceinline__ void head_zero(uint64_t j) {
#pragma unroll
    for (int i = 0; i < 8; ++i) heads[j * 8 + i] = 0u;
  }
};
// whole blocks: every lane stays for the wave-level atomic
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_heads(MerkleHeadDev mem, uint64_t m, uint64_t n_leaves, u32* found) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  const bool above = j < m && merkle_lane_head(mem, j, n_leaves);
  merkle_wave_tally(found, above);
}

struct MerkleConsDev {
  const u32* log;
  const u32* store;
  u32* proofs;
  size_t stride_words;            // 8 (depth(N) + 1)
  __device__ __forceinline__ void node(int level, uint64_t off, uint64_t idx, u32 w[8]) const {
    merkle_ld8(w, level ? store + (off + idx) * 8 : log + idx * 8);
  }
  __device__ __forceinline__ void proof_put(uint64_t j, u32 k, const u32 w[8]) { merkle_st8(proofs + j * stride_words + k * 8, w); }
  __device__ __forceinline__ void proof_zero(uint64_t j, u32 k) {
#pragma unroll
    for (int i = 0; i < 8; ++i) proofs[j * stride_words + k * 8 + i] = 0u;
  }
};
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_consistency(MerkleConsDev mem, const unsigned long long* old_size, uint64_t m,
                                                                  uint64_t n_leaves, int row, u32* proof_len) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  if (j >= m) return;
  proof_len[j] = merkle_lane_consistency(mem, j, old_size[j], n_leaves, row);
}

struct MerkleConsCheckDev {
  const unsigned long long* old_size_;
  const u32* old_roots;
  const u32* proofs;
  size_t stride_words;
  const u32* proof_len_;
  const u32* root_;
  __device__ __forceinline__ uint64_t old_size(uint64_t j) const { return old_size_[j]; }
  __device__ __forceinline__ u32 proof_len(uint64_t j) const { return proof_len_[j]; }
  __device__ __forceinline__ void old_root(uint64_t j, u32 w[8]) const { merkle_ld8(w, old_roots + j * 8); }
  __device__ __forceinline__ void proof(uint64_t j, u32 k, u32 w[8]) const { merkle_ld8(w, proofs + j * stride_words + k * 8); }
  __device__ __forceinline__ void root(u32 w[8]) const { merkle_ld8(w, root_); }
};
// whole blocks: every lane stays for the wave-level atomics
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_cons_check(MerkleConsCheckDev mem, uint64_t m, uint64_t n_leaves, u32* verdict, u32* found) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  const bool live = j < m;
  const u32 v = live ? merkle_lane_cons_check(mem, j, n_leaves) : 0u;
  if (live) verdict[j] = v;
  merkle_wave_tally(found, v == egm::MERKLE_BAD_INDEX);
  merkle_wave_tally(found + 1, v == egm::MERKLE_BAD_LENGTH);
  merkle_wave_tally(found + 2, v == egm::MERKLE_MISMATCH);
  merkle_wave_tally(found + 3, v == egm::MERKLE_MISMATCH_OLD);
}

}  // namespace eg
#endif
