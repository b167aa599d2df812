// roll_host.hpp -- arithmetic of the voter-roll pass (eg_roll_*, eg_hip.hip; kernels: roll_kernels.cuh): pure host code, no HIP.
// tests/hostcheck/rollcheck.cpp compiles it under ASan + UBSan together with the lane functions of the kernels.
//
// The pass says, per ballot, whether it is the one ballot of its voter that counts.  The ROLL is one 64-bit word per roster key: 0 = no
// counted ballot yet, else a PRIORITY that encodes the sequence number of the counted ballot so that the larger word wins under either
// policy (the rule is a maximum: commutative, idempotent, mergeable by an element-wise maximum):
//   ROLL_LAST   word = seq + 1              the last ballot of a voter counts
//   ROLL_FIRST  word = 2^63 - 1 - seq       the first one does
// seq <= 2^63 - 2, so every word is in [1, 2^63 - 1]: signed and unsigned order agree.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "scan_host.hpp"

#if defined(__HIPCC__)
#define EGR_HD __host__ __device__ inline
#else
#define EGR_HD inline
#endif

namespace egr {

constexpr uint32_t ST_SUPERSEDED = 16;            // EG_ST_SUPERSEDED
constexpr int ROLL_FIRST = 1;                     // EG_ROLL_FIRST
constexpr int ROLL_LAST = 2;                      // EG_ROLL_LAST
constexpr uint32_t ROLL_SUPERSEDED = 1;           // EG_ROLL_SUPERSEDED
constexpr uint32_t ROLL_OFF_ROLL = 2;             // EG_ROLL_OFF_ROLL
constexpr uint32_t ROLL_NOT_CAST = 3;             // EG_ROLL_NOT_CAST
constexpr uint64_t SEQ_NONE = ~0ull;              // EG_SEQ_NONE
constexpr uint32_t GROUP_NONE = 0xffffffffu;      // EG_GROUP_NONE
constexpr uint64_t N_LIMIT = 1ull << 31;          // n must stay below
constexpr uint64_t KEYS_MAX = 1ull << 31;         // EG_ROLL_KEYS_MAX
constexpr uint64_t SEQ_END_MAX = (1ull << 63) - 1; // seq_base + n may reach it

EGR_HD uint64_t word_of(uint64_t seq, int policy) { return policy == ROLL_LAST ? seq + 1u : SEQ_END_MAX - seq; }
EGR_HD uint64_t seq_of(uint64_t word, int policy) { return policy == ROLL_LAST ? word - 1u : SEQ_END_MAX - word; }
EGR_HD uint32_t status_word(uint32_t detail) { return ST_SUPERSEDED | detail << 8; }
// the claim of ballot b on its voter inside a batch of n: the batch's sequence order is its ballot order, so 32 bits carry it
EGR_HD uint32_t claim_of(uint64_t b, uint64_t n, int policy) { return (uint32_t)(policy == ROLL_LAST ? b + 1u : n - b); }
EGR_HD uint64_t claimant(uint32_t claim, uint64_t n, int policy) { return policy == ROLL_LAST ? (uint64_t)claim - 1u : n - claim; }

// argument rules that need no context: nullptr = fine, else what is wrong
struct Have {
  bool key_index, roll, superseded_by, found, roster_groups, roster_weights, groups_out, weights_out, displaced, displaced_count;
};
inline const char* refuse_sizes(uint64_t n, uint64_t n_keys) {
  if (n >= N_LIMIT) return "n is 2^31 or more";
  if (n && n_keys == 0) return "n_keys is 0";
  if (n_keys > KEYS_MAX) return "n_keys is above EG_ROLL_KEYS_MAX";
  return nullptr;
}
inline const char* refuse(uint64_t n, uint64_t n_keys, uint64_t seq_base, int policy, const Have& h) {
  if (const char* why = refuse_sizes(n, n_keys)) return why;
  if (seq_base > SEQ_END_MAX || n > SEQ_END_MAX - seq_base) return "seq_base + n is above 2^63 - 1";
  if (policy != ROLL_FIRST && policy != ROLL_LAST) return "policy is neither EG_ROLL_FIRST nor EG_ROLL_LAST";
  if (n && !(h.key_index && h.roll && h.superseded_by && h.found)) return "null key_index, roll, superseded_by or found";
  if (h.groups_out && !h.roster_groups) return "groups_out without roster_groups";
  if (h.weights_out && !h.roster_weights) return "weights_out without roster_weights";
  if (h.displaced != h.displaced_count) return "displaced and displaced_count come together";
  return nullptr;
}

// the caller's scratch of a cast, in bytes from its start (every part 256-byte aligned); n == 0 needs none
struct Layout {
  uint32_t n_tiles;            // of the scan over the ballots
  size_t best, flag, tiles, total;
};
inline Layout layout(size_t n, size_t n_keys) {
  Layout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.n_tiles = egscan::scan_tiles(n);
  L.best = take(n ? n_keys * sizeof(uint32_t) : 0);       // the largest claim on every voter, 0 = none
  L.flag = take(n * sizeof(uint32_t));                    // what the commit does for ballot b: FLAG_*, then FLAG_DISPLACED + rank
  L.tiles = take((size_t)L.n_tiles * sizeof(uint32_t));
  L.total = off;
  return L;
}

}  // namespace egr
