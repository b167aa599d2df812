// open_host.hpp -- arithmetic of the ballot-audit pass (eg_*_open_check*, eg_*_open_batch*, eg_hip.hip; kernels: open_kernels.cuh and, for
// the opener, open_gen_kernels.cuh): pure host code, no HIP.  tests/hostcheck/opencheck.cpp compiles it under ASan + UBSan together with
// the lane functions of the kernels.
//
// An OPENING of a ballot gives, per tally ciphertext (slot) t, the value v and the encryption randomness r the voting device used (the
// Benaloh challenge).  The pass re-encrypts and compares bytes: R = [r]G, B = [v]G + [r]K.  Per (ballot, slot) one verdict word, 0 or
// status_word(slot, check); the first non-zero word of a ballot, in slot order, is its status.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EGO_HD __host__ __device__ inline
#else
#define EGO_HD inline
#endif

namespace ego {

constexpr uint32_t ST_BAD_OPENING = 17;           // EG_ST_BAD_OPENING
constexpr uint32_t OPEN_BAD_SCALAR = 1;           // EG_OPEN_BAD_SCALAR: r is not below l
constexpr uint32_t OPEN_R = 2;                    // EG_OPEN_R: encode([r]G) is not the wire R
constexpr uint32_t OPEN_B = 3;                    // EG_OPEN_B: encode([v]G + [r]K) is not the wire B
constexpr uint64_t N_LIMIT = 1ull << 31;          // n must stay below
constexpr uint64_t ITEMS_MAX = 1ull << 31;        // EG_OPEN_ITEMS_MAX: n x n_slots may reach it
constexpr size_t RAND_BYTES = 32, WIRE_BYTES = 64;

// EG_OPEN_DETAIL(slot, check) in the detail field of the status word; slot < 2^22 always (a ballot has at most 4000 options)
EGO_HD uint32_t status_word(uint32_t slot, uint32_t check) { return ST_BAD_OPENING | (slot * 4u + check) << 8; }

// ---- where the generators draw the encryption randomness (prover_kernels.cuh), in 64-byte draws of the ballot's ChaCha stream --------------
// Choice (k_choice_encrypt): option j draws r, x and, where it is NOT chosen, a simulated response; the responses of the chosen options
// come after all of these.  `not_chosen_before` = #{j < k : option j not chosen}.
EGO_HD uint64_t choice_r_draw(uint64_t rng_skip, uint32_t k, uint32_t not_chosen_before) { return rng_skip + 2ull * k + not_chosen_before; }
// One range proof (gen_range_proof): r, n_rings - 1 partial randomnesses, n_rings x, and size - 1 responses per ring wherever the value
// sits in it - the same number whatever the value.
EGO_HD uint64_t range_draws(uint32_t n_rings, uint64_t ring_sizes_sum) { return (uint64_t)n_rings + ring_sizes_sum; }
// Quadratic voting (k_qv_encrypt): vote k's r is the first draw of the k-th range proof over the vote range
EGO_HD uint64_t qv_r_draw(uint64_t rng_skip, uint32_t k, uint64_t draws_per_vote) { return rng_skip + (uint64_t)k * draws_per_vote; }

// argument rules that need no params object: nullptr = fine, else what is wrong
struct Have { bool ballots, values, rand, status_out, found; };
inline const char* refuse(uint64_t n, const Have& h) {
  if (n >= N_LIMIT) return "n is 2^31 or more";
  if (n && !(h.ballots && h.values && h.rand && h.status_out && h.found)) return "null ballots, values, rand, status_out or found";
  return nullptr;
}
inline const char* refuse_items(uint64_t n, uint32_t n_slots) {
  if (n_slots == 0) return "internal: the plan has no tally ciphertexts";
  if (n * (uint64_t)n_slots > ITEMS_MAX) return "n x n_slots is above EG_OPEN_ITEMS_MAX";
  return nullptr;
}
// or-ed addresses: 16 bytes for the ballots (and the scratch), 8 for the values, 4 for rand and the status and found words
inline const char* refuse_alignment(uintptr_t quads, uintptr_t words64, uintptr_t words32) {
  if (quads & 15u) return "ballots and scratch must be 16-byte aligned";
  if (words64 & 7u) return "values must be 8-byte aligned";
  if (words32 & 3u) return "rand, status_in, status_out and found must be 4-byte aligned";
  return nullptr;
}

// the caller's scratch, in bytes from its start (every part 256-byte aligned); n == 0 needs none
struct Layout { size_t words, total; };
inline Layout layout(size_t n, uint32_t n_slots) {
  Layout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.words = take(n * (size_t)n_slots * sizeof(uint32_t));      // the verdict word of every (ballot, slot); written for participating ballots only
  L.total = off;
  return L;
}

}  // namespace ego
