// weed_index_host.hpp -- arithmetic of the persistent board index (eg_weed_index_*, eg_*_weed_indexed*, eg_hip.hip; kernels:
// weed_index_kernels.cuh): pure host code, no HIP.  tests/hostcheck/weedindexcheck.cpp compiles it under ASan + UBSan together with the
// lane functions of the kernels.
//
// The stateless pass (weed_host.hpp) puts the board and the batch into ONE table that it clears and fills in every call.  The indexed
// pass keeps TWO:
//   the board index   the caller's, in device memory between calls: 32-bit slots, a slot holds a board position (< 2^31) or INDEX_EMPTY.
//                     egw::table_slots(board_cap) slots, so an append that fits the board keeps the load at or below 0.5.  One seed for
//                     the life of the index.
//   the batch table   in the call's scratch: 64-bit batch references of the n K keys of the batch alone, a fresh seed per call.
// A key is flagged EG_DUP_PRIOR iff the index holds it; otherwise its owner is the batch table's.  That is the stateless rule: a board
// reference is below every batch reference, so the minimum over one table is "the board if it is there, else the batch".
#pragma once
#include "weed_host.hpp"

namespace egw {

constexpr uint32_t INDEX_EMPTY = 0xffffffffu;

// bytes of an index over a board of board_cap entries (0: refused)
inline size_t index_bytes(uint64_t board_cap) { return board_cap >= N_LIMIT ? 0 : (size_t)table_slots(board_cap) * sizeof(uint32_t); }

// 32-bit slots behind the 64-bit Table interface of weed_lane_insert / weed_lane_owner: INDEX_EMPTY <-> EMPTY, a position as it is
EGW_HD uint64_t index_widen(uint32_t v) { return v == INDEX_EMPTY ? EMPTY : (uint64_t)v; }

// argument rules of the indexed pass that need no plan: the board no longer counts against KEYS_MAX
inline const char* refuse_indexed(uint64_t n, uint64_t n_prior, uint64_t board_cap) {
  if (const char* why = refuse(n, n_prior, board_cap)) return why;
  if (board_cap >= N_LIMIT) return "board_cap is 2^31 or more";
  return nullptr;
}
inline const char* refuse_indexed_keys(uint64_t n, uint32_t keys_per_ballot) {
  return n * keys_per_ballot > KEYS_MAX ? "n * keys_per_ballot is above EG_WEED_KEYS_MAX" : nullptr;
}

// the scratch of an indexed call: the stateless layout of a batch beside an empty board - a function of n alone
inline Layout layout_indexed(size_t n, uint32_t keys_per_ballot) { return layout(n, 0, keys_per_ballot); }

}  // namespace egw
