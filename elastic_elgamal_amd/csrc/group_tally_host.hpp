// group_tally_host.hpp -- arithmetic of the per-group tally (eg_*_tally_grouped*, eg_hip.hip; kernels: group_tally_kernels.cuh): pure host
// code, no HIP.  tests/hostcheck/grouptallycheck.cpp and weightedtallycheck.cpp compile it under ASan + UBSan together with the lane
// functions of the kernels.
//
// The pass is a keyed sum of points: ballot b, if accepted, adds its 2 n_options ciphertext points to the tally of group groups[b].
//   level 0      a group's list of accepted ballots is cut into PIECES of <= S1 ballots; one lane sums one tally slot of one piece
//                straight from the wire bytes (S1 decodings on one chain);
//   level l >= 1 the partial sums of a group at level l - 1 are cut into pieces of <= S2; one lane sums one slot of one piece.
// A group is as long as the electorate makes it - one precinct may hold every ballot - so no lane ever sums a whole group: the number of
// levels is fixed by n alone (levels()), and at the last level every group has at most one entry.
//   S1 = S2 = 32: S1 S2^2 = 2^15, so 2^15 + 1 ballots in one group already need four levels (a test below 10^5 ballots walks every kind
//   of level), and n < 2^31 needs seven.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "plan.h"
#include "scan_host.hpp"

#if defined(__HIPCC__)
#define EGGT_HD __host__ __device__ inline
#else
#define EGGT_HD inline
#endif

namespace eggt {

constexpr uint32_t S1 = 32;                       // ballots per piece at level 0 (production; the lane functions take it as an argument)
constexpr uint32_t S2 = 32;                       // partial sums per piece at the following levels
constexpr uint32_t GROUP_NONE = 0xffffffffu;      // EG_GROUP_NONE
constexpr uint32_t GROUPS_MAX = 1u << 24;         // EG_TALLY_GROUPS_MAX
constexpr uint64_t N_LIMIT = 1ull << 31;          // n must stay below: ballot indices and list offsets are 32-bit
constexpr int MAX_LEVELS = 7;                     // ceil(2^31 / 32) = 2^26 pieces -> 2^21 -> 2^16 -> 2^11 -> 2^6 -> 2 -> 1
constexpr int SEQ = MAX_LEVELS + 1;               // sequences of the scan: list offsets + pieces of every level
constexpr size_t POINT_BYTES = 144;               // a partial sum: 36 limbs (device_io.cuh: PT_WORDS)

EGGT_HD uint32_t ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b ? 1u : 0u); }

// levels that n ballots need whatever their groups: 1 + the number of times ceil(n / S1) must be cut by S2 to reach one entry
inline int levels(uint64_t n, uint32_t s1, uint32_t s2) {
  int l = 1;
  for (uint64_t m = (n + s1 - 1) / s1; m > 1; m = (m + s2 - 1) / s2) ++l;
  return l;
}

// v[0] = the group's count; v[l + 1] = its pieces at level l (0 beyond the last level)
EGGT_HD void pieces_tuple(uint32_t v[SEQ], uint32_t cnt, int n_levels, uint32_t s1, uint32_t s2) {
  v[0] = cnt;
  uint32_t m = ceil_div(cnt, s1);
  for (int l = 0; l < MAX_LEVELS; ++l) { v[l + 1] = l < n_levels ? m : 0u; m = ceil_div(m, s2); }
}

// what the scan kernels compute, serially: list offsets, and pieces / first piece of every group at every level
struct Scan {
  std::vector<uint32_t> offsets;
  std::vector<uint32_t> pieces[MAX_LEVELS], piece0[MAX_LEVELS];
  uint32_t totals[MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0};
};
inline Scan scan(const std::vector<uint32_t>& counts, int n_levels, uint32_t s1, uint32_t s2) {
  Scan S;
  const size_t g = counts.size();
  S.offsets.resize(g);
  for (int l = 0; l < n_levels; ++l) { S.pieces[l].resize(g); S.piece0[l].resize(g); }
  uint32_t run[SEQ] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t q = 0; q < g; ++q) {
    uint32_t v[SEQ];
    pieces_tuple(v, counts[q], n_levels, s1, s2);
    S.offsets[q] = run[0];
    for (int l = 0; l < n_levels; ++l) { S.pieces[l][q] = v[l + 1]; S.piece0[l][q] = run[l + 1]; }
    for (int k = 0; k < SEQ; ++k) run[k] += v[k];
  }
  for (int l = 0; l < n_levels; ++l) S.totals[l] = run[l + 1];
  return S;
}

// most pieces that level 0 and level 1 can have: floor(entries / S) whole pieces and one ragged piece per non-empty group.  Later
// levels never have more than the level two before them, so two buffers of these sizes serve every level in turn.
inline size_t pieces_bound(size_t entries, size_t n, uint32_t n_groups, uint32_t s) { return entries / s + (n < n_groups ? n : (size_t)n_groups); }

// the caller's scratch, in bytes from its start (every part 256-byte aligned)
struct Layout {
  size_t counts, cursors, offsets, pieces[MAX_LEVELS], piece0[MAX_LEVELS], totals, tiles, idx, psum[2], total;
  size_t psum_points[2];       // capacity of the two partial-sum buffers, in pieces
  int n_levels;
  uint32_t n_tiles;
};
inline Layout layout(size_t n, uint32_t n_groups, uint32_t n_slots, uint32_t s1 = S1, uint32_t s2 = S2) {
  Layout L;
  L.n_levels = levels(n, s1, s2);
  L.n_tiles = egscan::scan_tiles(n_groups);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  const size_t g = (size_t)n_groups * sizeof(uint32_t);
  L.counts = take(g);
  L.cursors = take(g);          // directly behind the counts: one memset clears both
  L.offsets = take(g);
  for (int l = 0; l < MAX_LEVELS; ++l) { L.pieces[l] = l < L.n_levels ? take(g) : 0; L.piece0[l] = l < L.n_levels ? take(g) : 0; }
  L.totals = take(SEQ * sizeof(uint32_t));
  L.tiles = take((size_t)L.n_tiles * SEQ * sizeof(uint32_t));
  L.idx = take(n * sizeof(uint32_t));
  L.psum_points[0] = pieces_bound(n, n, n_groups, s1);
  L.psum_points[1] = L.n_levels > 1 ? pieces_bound(L.psum_points[0], n, n_groups, s2) : 0;
  L.psum[0] = take(L.psum_points[0] * n_slots * POINT_BYTES);
  L.psum[1] = take(L.psum_points[1] * n_slots * POINT_BYTES);
  L.total = off;
  return L;
}

// the 32-byte wire item behind every tally slot: pt_items[i].item with pt_items[i].slot == tally_slots[t] (0xffffffff: none - a plan
// whose tally slot is not a wire point, which check_flat_plan's callers treat as an internal error)
inline std::vector<uint32_t> tally_items(const std::vector<egplan::WireItem>& pt_items, const std::vector<uint32_t>& tally_slots) {
  std::vector<uint32_t> items(tally_slots.size(), 0xffffffffu);
  for (size_t t = 0; t < tally_slots.size(); ++t)
    for (const egplan::WireItem& w : pt_items)
      if (w.slot == tally_slots[t]) { items[t] = w.item; break; }
  return items;
}

// argument rules of eg_*_tally_grouped*: nullptr = fine, else what is wrong
inline const char* refuse(size_t n, uint32_t n_groups) {
  if (n_groups == 0) return "n_groups is 0";
  if (n_groups > GROUPS_MAX) return "n_groups is above EG_TALLY_GROUPS_MAX";
  if ((uint64_t)n >= N_LIMIT) return "n is 2^31 or more";
  return nullptr;
}

// ---- the weighted pass (eg_*_tally_weighted*): ballot b adds [w_b] x its ciphertext points, w_b < 2^weight_bits ---------------------------
// The same lists, pieces and levels; beside every partial sum of slot 0 travels the piece's sum of weights, a 128-bit number in two
// 64-bit words (low, high): n < 2^31 weights below 2^64 stay below 2^95.
constexpr size_t WSUM_BYTES = 16;

// the grouped layout, and behind it one weight sum per piece for the same two alternating levels
struct WeightedLayout {
  Layout base;
  size_t wsum[2], total;
};
inline WeightedLayout layout_weighted(size_t n, uint32_t n_groups, uint32_t n_slots, uint32_t s1 = S1, uint32_t s2 = S2) {
  WeightedLayout W;
  W.base = layout(n, n_groups, n_slots, s1, s2);
  size_t off = W.base.total;
  for (int k = 0; k < 2; ++k) { W.wsum[k] = off; off += (W.base.psum_points[k] * WSUM_BYTES + 255) / 256 * 256; }
  W.total = off;
  return W;
}

// does weight w fit weight_bits (1..64) bits
EGGT_HD bool weight_fits(uint64_t w, int weight_bits) { return weight_bits >= 64 || (w >> weight_bits) == 0u; }

// argument rules of eg_*_tally_weighted* beyond refuse()
inline const char* refuse_weight_bits(int weight_bits) {
  return weight_bits < 1 || weight_bits > 64 ? "weight_bits is outside 1..64" : nullptr;
}

}  // namespace eggt
