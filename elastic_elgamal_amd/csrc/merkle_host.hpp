// merkle_host.hpp -- arithmetic and layout of the receipt log (eg_merkle_*, eg_hip.hip; kernels: merkle_kernels.cuh): pure host code, no
// HIP.  tests/hostcheck/merklecheck.cpp compiles it under ASan + UBSan together with the lane functions of the kernels.
//
// The log is the caller's array of 32-byte leaf hashes; the tree above it is RFC 6962 2.1 with H = the first 32 bytes of SHA-512:
//   leaf = H(0x00 || prefix || msg || extra)      node(l, r) = H(0x01 || l || r)      the empty tree = H("")
// in the bottom-up form that equals the RFC's split at the largest power of two below N: level L + 1 has ceil(n_L / 2) nodes, node i =
// node(a[2i], a[2i + 1]), and an odd last node is promoted unchanged.  So level L has ceil(N / 2^L) nodes and depth(N) = ceil(log2 N).
// THE NODE STORE holds levels 1 .. depth back to back, level 0 is the log itself.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "scan_host.hpp"

#if defined(__HIPCC__)
#define EGM_HD __host__ __device__ inline
#else
#define EGM_HD inline
#endif

namespace egm {

constexpr uint32_t MERKLE_BAD_INDEX = 1;          // EG_MERKLE_BAD_INDEX
constexpr uint32_t MERKLE_BAD_LENGTH = 2;         // EG_MERKLE_BAD_LENGTH
constexpr uint32_t MERKLE_MISMATCH = 3;           // EG_MERKLE_MISMATCH
constexpr uint64_t LEAF_NONE = ~0ull;             // EG_LEAF_NONE
constexpr uint32_t NO_PATH = 0xffffffffu;         // EG_MERKLE_NO_PATH
constexpr uint64_t LEAVES_MAX = 1ull << 31;       // EG_MERKLE_LEAVES_MAX: n, m and N stay below
constexpr size_t HASH_BYTES = 32;                 // EG_MERKLE_HASH_BYTES
constexpr size_t HASH_WORDS = 8;
constexpr size_t PREFIX_MAX = 255;
constexpr int T_LOG = 10;                         // levels per launch of the tree: a tile of 2^T_LOG nodes per workgroup
constexpr int MAX_DEPTH = 31;

EGM_HD int depth(uint64_t n_leaves) {
  int d = 0;
  while (d < 64 && ((uint64_t)1 << d) < n_leaves) ++d;
  return d;
}
// nodes of level L (0 = the leaves)
EGM_HD uint64_t level_count(uint64_t n_leaves, int level) {
  if (level >= 64) return n_leaves ? 1u : 0u;
  return (n_leaves >> level) + ((n_leaves & (((uint64_t)1 << level) - 1u)) ? 1u : 0u);
}
// where level L >= 1 starts in the node store, in nodes
EGM_HD uint64_t level_offset(uint64_t n_leaves, int level) {
  uint64_t off = 0;
  for (int l = 1; l < level; ++l) off += level_count(n_leaves, l);
  return off;
}
EGM_HD uint64_t nodes_total(uint64_t n_leaves) { return level_offset(n_leaves, depth(n_leaves) + 1); }
// the length of the audit path of leaf i < N: bottom-up, one entry per level at which the sibling i ^ 1 exists
EGM_HD uint32_t path_len(uint64_t i, uint64_t n_leaves) {
  uint32_t len = 0;
  for (uint64_t n = n_leaves; n > 1; n = (n + 1) >> 1, i >>= 1)
    if ((i ^ 1u) < n) ++len;
  return len;
}
// the append of `total` leaves behind n_prior entries of a log with room for log_cap
EGM_HD bool append_fits(uint64_t n_prior, uint64_t total, uint64_t log_cap) { return n_prior <= log_cap && total <= log_cap - n_prior; }

// argument rules that need no context: nullptr = fine, else what is wrong
inline const char* refuse_messages(uint64_t n, bool have_msgs, uint64_t msg_stride, uint64_t msg_len, bool have_prefix, uint64_t prefix_len,
                                   bool have_extra, uint64_t extra_stride, uint64_t extra_len) {
  if (n >= LEAVES_MAX) return "n is 2^31 or more";
  if (prefix_len > PREFIX_MAX) return "prefix_len is above 255";
  if (prefix_len && !have_prefix) return "null prefix with a length";
  if (msg_stride < msg_len) return "msg_stride is below msg_len";
  if (extra_stride < extra_len) return "extra_stride is below extra_len";
  if (n && msg_len && !have_msgs) return "null msgs";
  if (n && extra_len && !have_extra) return "null extra with a length";
  return nullptr;
}
inline const char* refuse_leaves(uint64_t n, uint64_t n_prior, bool have_leaf_index, bool have_found, bool have_log, bool have_log_count,
                                 uint64_t log_cap) {
  if (n_prior >= LEAVES_MAX) return "n_prior is 2^31 or more";
  if (n && !(have_leaf_index && have_found)) return "null leaf_index or found";
  if (have_log_count && n_prior > log_cap) return "n_prior is above log_cap";
  if (have_log_count && !have_log) return "null log with an append requested";
  return nullptr;
}
inline const char* refuse_tree(uint64_t n_leaves, bool have_log, bool have_root) {
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (!have_root) return "null root";
  if (n_leaves && !have_log) return "null log";
  return nullptr;
}
inline const char* refuse_paths(uint64_t m, uint64_t n_leaves, bool have_index, bool have_log, bool have_nodes, bool have_paths, bool have_len) {
  if (m >= LEAVES_MAX) return "m is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (m && !(have_index && have_len)) return "null index or path_len";
  if (m && n_leaves > 1 && !(have_log && have_nodes && have_paths)) return "null log, nodes or paths";
  return nullptr;
}
inline const char* refuse_check(uint64_t m, uint64_t n_leaves, bool have_index, bool have_leaves, bool have_paths, uint64_t path_stride,
                                bool have_len, bool have_root, bool have_verdict, bool have_found) {
  if (m >= LEAVES_MAX) return "m is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (path_stride < HASH_BYTES * (uint64_t)depth(n_leaves)) return "path_stride is below 32 * depth(N)";
  if (path_stride & 3u) return "path_stride is no multiple of 4";
  if (m && !(have_index && have_leaves && have_len && have_root && have_verdict && have_found)) return "null index, leaves, path_len, root, verdict or found";
  if (m && n_leaves > 1 && !have_paths) return "null paths";
  return nullptr;
}

// the caller's scratch of the leaf pass, in bytes from its start (every part 256-byte aligned); n == 0 needs none
struct LeafLayout {
  uint32_t n_tiles;            // of the scan over the ballots
  size_t head, pos, tiles, total_word, leaves, total;
};
inline LeafLayout leaf_layout(size_t n) {
  LeafLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.n_tiles = egscan::scan_tiles(n);
  L.head = take(n ? 1 + PREFIX_MAX : 0);                  // the domain byte 0x00 and the prefix
  L.pos = take(n * sizeof(uint32_t));                     // 1 = ballot b has a leaf, then its rank
  L.tiles = take((size_t)L.n_tiles * sizeof(uint32_t));
  L.total_word = take(n ? 2 * sizeof(uint32_t) : 0);      // the number of leaves, whether the append fits
  L.leaves = take(n * HASH_BYTES);                        // the leaves, where the caller takes no leaves_out
  L.total = off;
  return L;
}
// the caller's scratch of a tree WITHOUT a node store: the top level of every launch, two buffers in turn
struct TreeLayout {
  size_t ping, pong, total;
};
inline TreeLayout tree_layout(uint64_t n_leaves) {
  TreeLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  const bool more = n_leaves > ((uint64_t)1 << T_LOG);    // more than one launch
  L.ping = take(more ? (size_t)level_count(n_leaves, T_LOG) * HASH_BYTES : 0);
  L.pong = take(more ? (size_t)level_count(n_leaves, 2 * T_LOG) * HASH_BYTES : 0);
  L.total = off;
  return L;
}

}  // namespace egm
