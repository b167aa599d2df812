// merkle_audit_host.hpp -- arithmetic and argument rules of the receipt log's audit entries (eg_merkle_heads / _consistency /
// _consistency_check, eg_hip.hip; kernels: merkle_audit_kernels.cuh): pure host code, no HIP.  tests/hostcheck/merkleauditcheck.cpp
// compiles it under ASan + UBSan together with the lane functions of the kernels.
//
// Everything is read out of the node store of merkle_host.hpp: node j of level L is the tree hash of leaves [j 2^L, min((j + 1) 2^L, N)),
// the promoted ragged last node included.  For an old size 1 <= m <= N:
//   m = (node + 1) 2^L with L = the number of trailing zero bits of m: store node (L, node) is the last complete piece of the old tree
//   (THE SEED); node == 0: m is a power of two and the old tree is that one node.
//   PROOF(m, D[N]) of RFC 9162 2.1.4.1 = the seed (if node != 0), then the audit path of node (L, node) inside the N-tree.
#pragma once
#include "merkle_host.hpp"

namespace egm {

constexpr uint32_t MERKLE_MISMATCH_OLD = 4;       // EG_MERKLE_MISMATCH_OLD

// the level of the seed of old size m >= 1: the trailing zero bits of m (= the trailing one bits of m - 1)
EGM_HD int seed_level(uint64_t m) {
  int level = 0;
  for (; level < 63 && !((m >> level) & 1u); ++level) {}
  return level;
}
// the length of the consistency proof of (m, N); NO_PATH for m == 0 or m > N
EGM_HD uint32_t consistency_len(uint64_t m, uint64_t n_leaves) {
  if (m == 0 || m > n_leaves) return NO_PATH;
  if (m == n_leaves) return 0;
  const int first = seed_level(m);
  uint64_t node = (m >> first) - 1u;
  uint32_t len = node ? 1u : 0u;
  uint64_t n = level_count(n_leaves, first);
  for (int level = first; level < 64 && n > 1; ++level, n = (n + 1) >> 1, node >>= 1)
    if ((node ^ 1u) < n) ++len;
  return len;
}
// entries of a row of proofs: depth(N) + 1
EGM_HD size_t consistency_row(uint64_t n_leaves) { return (size_t)depth(n_leaves) + 1; }

// argument rules that need no context: nullptr = fine, else what is wrong
inline const char* refuse_heads(uint64_t m, uint64_t n_leaves, bool have_size, bool have_log, bool have_nodes, bool have_heads, bool have_found) {
  if (m >= LEAVES_MAX) return "m is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (m && !(have_size && have_heads && have_found)) return "null size, heads or found";
  if (m && ((n_leaves > 0 && !have_log) || (n_leaves > 1 && !have_nodes))) return "null log or nodes";
  return nullptr;
}
inline const char* refuse_consistency(uint64_t m, uint64_t n_leaves, bool have_old_size, bool have_log, bool have_nodes, bool have_proofs,
                                      bool have_len) {
  if (m >= LEAVES_MAX) return "m is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (m && !(have_old_size && have_proofs && have_len)) return "null old_size, proofs or proof_len";
  if (m && ((n_leaves > 0 && !have_log) || (n_leaves > 1 && !have_nodes))) return "null log or nodes";
  return nullptr;
}
inline const char* refuse_consistency_check(uint64_t m, uint64_t n_leaves, bool have_old_size, bool have_old_root, bool have_proofs,
                                            uint64_t proof_stride, bool have_len, bool have_root, bool have_verdict, bool have_found) {
  if (m >= LEAVES_MAX) return "m is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (proof_stride < HASH_BYTES * (uint64_t)consistency_row(n_leaves)) return "proof_stride is below 32 * (depth(N) + 1)";
  if (proof_stride & 3u) return "proof_stride is no multiple of 4";
  if (m && !(have_old_size && have_old_root && have_len && have_root && have_verdict && have_found))
    return "null old_size, old_root, proof_len, root, verdict or found";
  if (m && n_leaves > 1 && !have_proofs) return "null proofs";
  return nullptr;
}

}  // namespace egm
