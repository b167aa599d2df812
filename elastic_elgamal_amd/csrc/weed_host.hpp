// weed_host.hpp -- arithmetic of ballot weeding (eg_*_weed*, eg_hip.hip; kernels: weed_kernels.cuh): pure host code, no HIP.
// tests/hostcheck/weedcheck.cpp compiles it under ASan + UBSan together with the lane functions of the kernels.
//
// The pass flags every participating ballot that carries a tally ciphertext (64 wire bytes R || B, a KEY) which is already on the
// caller's board or in an earlier participating ballot of the batch.  Keys are never copied or decoded: an open-addressing table of
// 64-bit REFERENCES says where a key's bytes live, and the smallest reference of a key is its earliest owner:
//   board entry j                  -> j                              (j < 2^31: below every batch reference)
//   key k of ballot b (K a ballot) -> BATCH_BASE + b K + k           (ordered by ballot, then option)
//   an empty slot                  -> EMPTY, all ones
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "scan_host.hpp"

#if defined(__HIPCC__)
#define EGW_HD __host__ __device__ inline
#else
#define EGW_HD inline
#endif

namespace egw {

constexpr uint32_t DUP_NONE = 0xffffffffu;        // EG_DUP_NONE
constexpr uint32_t DUP_PRIOR = 0xfffffffeu;       // EG_DUP_PRIOR
constexpr uint32_t ST_DUPLICATE = 14;             // EG_ST_DUPLICATE
constexpr uint64_t N_LIMIT = 1ull << 31;          // n and n_prior must stay below
constexpr uint64_t KEYS_MAX = 1ull << 30;         // EG_WEED_KEYS_MAX: n K + n_prior
constexpr uint64_t EMPTY = ~0ull;
constexpr uint64_t BATCH_BASE = 1ull << 32;
constexpr uint64_t MIN_SLOTS = 1024;
constexpr size_t KEY_BYTES = 64;

EGW_HD uint64_t board_ref(uint64_t j) { return j; }
EGW_HD uint64_t batch_ref(uint64_t b, uint32_t keys_per_ballot, uint32_t k) { return BATCH_BASE + b * keys_per_ballot + k; }
EGW_HD bool is_board_ref(uint64_t r) { return r < BATCH_BASE; }
EGW_HD uint64_t ref_ballot(uint64_t r, uint32_t keys_per_ballot) { return (r - BATCH_BASE) / keys_per_ballot; }
EGW_HD uint32_t ref_key(uint64_t r, uint32_t keys_per_ballot) { return (uint32_t)((r - BATCH_BASE) % keys_per_ballot); }

// where the 64 bytes of key k of ballot b begin, in bytes from the start of the batch: 64-bit throughout (a batch above 4 GB)
EGW_HD uint64_t key_offset(uint64_t b, uint64_t stride, uint32_t r_item) { return b * stride + (uint64_t)r_item * 32u; }

// the table: the smallest power of two >= 2 x keys, at least MIN_SLOTS (a load of at most 0.5)
inline uint64_t table_slots(uint64_t keys) {
  uint64_t c = MIN_SLOTS;
  while (c < 2 * keys) c <<= 1;
  return c;
}

// the R items of the keys: tally item 2k of the plan, whose B item must be the next wire item (the 64 bytes are then contiguous).
// false: a plan whose tally ciphertexts are not laid out that way - no weeding arguments are made for it
inline bool key_items(std::vector<uint32_t>& r_items, const std::vector<uint32_t>& tally_items) {
  r_items.clear();
  if (tally_items.empty() || tally_items.size() % 2) return false;
  for (size_t t = 0; t < tally_items.size(); t += 2) {
    if (tally_items[t] == 0xffffffffu || tally_items[t + 1] != tally_items[t] + 1u) return false;
    r_items.push_back(tally_items[t]);
  }
  return true;
}

// argument rules that need no plan: nullptr = fine, else what is wrong
inline const char* refuse(uint64_t n, uint64_t n_prior, uint64_t board_cap) {
  if (n >= N_LIMIT) return "n is 2^31 or more";
  if (n_prior >= N_LIMIT) return "n_prior is 2^31 or more";
  if (n_prior > board_cap) return "n_prior is above board_cap";
  return nullptr;
}
inline const char* refuse_keys(uint64_t n, uint64_t n_prior, uint32_t keys_per_ballot) {
  return n * keys_per_ballot + n_prior > KEYS_MAX ? "n * keys_per_ballot + n_prior is above EG_WEED_KEYS_MAX" : nullptr;
}

// the caller's scratch, in bytes from its start (every part 256-byte aligned); n == 0 needs none
struct Layout {
  uint64_t slots;              // of the table
  uint32_t n_tiles;            // of the scan over the ballots
  size_t table, pos, tiles, total_word, total;
};
inline Layout layout(size_t n, size_t n_prior, uint32_t keys_per_ballot) {
  Layout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.slots = n ? table_slots((uint64_t)n * keys_per_ballot + n_prior) : 0;
  L.n_tiles = egscan::scan_tiles(n);
  L.table = take((size_t)L.slots * sizeof(uint64_t));
  L.pos = take(n * sizeof(uint32_t));                     // keep flag of every ballot, then its rank among the kept ones
  L.tiles = take((size_t)L.n_tiles * sizeof(uint32_t));
  L.total_word = take(n ? 2 * sizeof(uint32_t) : 0);      // kept ballots, and whether their keys fit the board
  L.total = off;
  return L;
}

}  // namespace egw
