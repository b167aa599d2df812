// merkle_grow_host.hpp -- arithmetic and argument rules of the receipt log's grow entry (eg_merkle_grow, eg_hip.hip; kernels:
// merkle_grow_kernels.cuh): pure host code, no HIP.  tests/hostcheck/merklegrowcheck.cpp compiles it under ASan + UBSan together with the
// lane functions of the kernels.
//
// The node store of N leaves out of the node store of its first m: node j of level L is the tree hash of leaves [j 2^L, min((j + 1) 2^L,
// N)), so an append from m to N leaves it unchanged exactly when (j + 1) 2^L <= m: level L keeps its first m >> L nodes.  The levels lie
// back to back with counts ceil(N / 2^L), so every level above the first MOVES when N grows: a copy, not a hash.
//   The launches are those of eg_merkle_tree: launch k reduces input level L0 = k T through up to T levels in tiles of 2^T input nodes.
//   tile0 = (m >> L0) >> T tiles of the launch lie wholly inside the old tree: on every level L0 + s of the launch their tile0 << (T - s)
//   nodes are COPIED from the old store (one row of the table per level), and the tiles from tile0 on are reduced as the tree reduces them.
//   Those read input nodes from tile0 << T on: leaves from (m >> T) << T on at the first launch, and above it nodes that the launch below
//   copied (index < m >> L0) or made.  The old tree's ragged and promoted nodes are in no row.
#pragma once
#include "merkle_host.hpp"

namespace egm {

constexpr int GROW_ROWS_MAX = MAX_DEPTH;          // one row per level 1 .. depth at the most
constexpr int GROW_LAUNCHES_MAX = 16;             // ceil(31 / 2): the host check runs tiles of 4

// the copy: row r moves `count` nodes from node `src` of the old store to node `dst` of the new one; rows by rising level
struct GrowRow {
  uint64_t src, dst, count;
};
struct GrowTable {
  uint32_t n_rows;
  uint64_t total;                                 // the sum of the counts
  GrowRow row[GROW_ROWS_MAX];
};
struct GrowLaunch {
  int level;                                      // L0, the input level (0: the log)
  int steps;
  uint64_t n_in, tiles, tile0;                    // tiles tile0 .. tiles - 1 are reduced; none if tile0 == tiles
  uint64_t off[T_LOG];                            // off[s - 1]: where level L0 + s starts in the NEW store, in nodes
};
struct GrowPlan {
  int n_launches;
  GrowLaunch launch[GROW_LAUNCHES_MAX];
  GrowTable table;
};
// old size m <= N < LEAVES_MAX, tiles of 2^t_log nodes (the library: T_LOG)
inline GrowPlan grow_plan(uint64_t m, uint64_t n_leaves, int t_log = T_LOG) {
  GrowPlan P;
  P.n_launches = 0;
  P.table.n_rows = 0;
  P.table.total = 0;
  const int d = depth(n_leaves);
  uint64_t n_in = n_leaves;
  for (int level = 0; level < d;) {
    GrowLaunch& a = P.launch[P.n_launches++];
    a.level = level;
    a.steps = d - level < t_log ? d - level : t_log;
    a.n_in = n_in;
    a.tiles = (n_in + (((uint64_t)1 << t_log) - 1u)) >> t_log;
    a.tile0 = (m >> level) >> t_log;
    for (int k = 0; k < T_LOG; ++k) a.off[k] = k < a.steps ? level_offset(n_leaves, level + k + 1) : 0u;
    // a whole tile inside the old tree: m >= 2^(level + t_log), so the old and the new tree both have every level of this launch
    for (int s = 1; a.tile0 && s <= a.steps; ++s) {
      GrowRow& r = P.table.row[P.table.n_rows++];
      r.src = level_offset(m, level + s);
      r.dst = a.off[s - 1];
      r.count = a.tile0 << (t_log - s);
      P.table.total += r.count;
    }
    n_in = level_count(n_in, a.steps);
    level += a.steps;
  }
  return P;
}

// byte ranges [a, a + a_bytes) and [b, b + b_bytes); an empty range overlaps nothing
inline bool ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes) {
  return a_bytes && b_bytes && a < b + b_bytes && b < a + a_bytes;
}
// argument rules that need no context: nullptr = fine, else what is wrong.  The addresses are looked at, never followed
inline const char* refuse_grow(uint64_t old_size, uint64_t n_leaves, const void* nodes_old, bool have_log, const void* nodes, bool have_root) {
  if (old_size >= LEAVES_MAX) return "old_size is 2^31 or more";
  if (n_leaves >= LEAVES_MAX) return "N is 2^31 or more";
  if (old_size > n_leaves) return "old_size is above N";
  if (!have_root) return "null root";
  if (n_leaves && !have_log) return "null log";
  if (n_leaves > 1 && !nodes) return "null nodes";
  if (old_size > 1 && !nodes_old) return "null nodes_old";
  if (nodes_old && nodes &&
      ranges_overlap((uint64_t)(uintptr_t)nodes_old, nodes_total(old_size) * HASH_BYTES, (uint64_t)(uintptr_t)nodes, nodes_total(n_leaves) * HASH_BYTES))
    return "nodes_old and nodes overlap";
  return nullptr;
}

}  // namespace egm
