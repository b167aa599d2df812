// shuffle_host.hpp -- sizes, argument rules and scratch layout of the shuffle verifier (eg_shuffle_*; eg_hip.hip; kernels and lane
// functions: shuffle_kernels.cuh; the rule: include/eg_hip.h): pure host code, no HIP.  tests/hostcheck/shufflecheck.cpp compiles it under
// ASan + UBSan beside the lane functions and counts the layout against a sum of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace egsh {

constexpr uint64_t ROWS_MAX = 1ull << 23;         // 2N terms of a product stay within the 2^24 of the product entry
constexpr size_t PREFIX_MAX = 255;
constexpr size_t HEAD_BYTES = 288;                // t1 t2 t3 t41 t42 s1 s2 s3 s4
constexpr size_t ROW_BYTES = 160;                 // c, c^, t^, s^, s' of a row (planar in the blob)
constexpr uint32_t KEY_TRIES = 4096;              // tries of a generator before its lane gives up
constexpr unsigned NT = 256;                      // lanes per block
constexpr unsigned WAVE_ROWS = 63;                // rows of a wavefront of the chain kernel: lane 0 decodes the row before them
constexpr unsigned CHAIN_BLOCKS_PER_CU = 4;       // grid of the chain kernel, each wavefront striding over its tiles
constexpr size_t TABLE_BYTES = 8 * 9 * 16;        // a radix-16 table: WS_QUADS uint4 (device_io.cuh); a chain lane has two
constexpr size_t BIG_PRODUCTS = 4, SMALL_PRODUCTS = 2, SMALL_TERMS = 2;
// words of the state block (one 32-bit word each; the kernels' names for them are in shuffle_kernels.cuh)
constexpr size_t STATE_BYTES = 512;

inline size_t key_bytes(uint64_t cap) { return cap <= ROWS_MAX ? (size_t)(cap + 1) * 32 : 0; }
inline size_t proof_bytes(uint64_t n) { return n <= ROWS_MAX ? HEAD_BYTES + ROW_BYTES * (size_t)n : 0; }

// what is wrong with the arguments of a verification (nullptr = fine); the pointers are looked at only with rows to verify
inline const char* refuse_verify(uint64_t n, uint64_t key_cap, bool have_in, bool have_out, bool have_K, bool have_prefix, uint64_t prefix_len,
                                 bool have_key, bool have_proof, bool have_verdict, bool have_found) {
  if (n > ROWS_MAX) return "N is above EG_SHUFFLE_ROWS_MAX";
  if (key_cap > ROWS_MAX) return "key_cap is above EG_SHUFFLE_ROWS_MAX";
  if (n > key_cap) return "the commitment key is shorter than N + 1 generators (N > key_cap)";
  if (prefix_len > PREFIX_MAX) return "prefix_len is above 255";
  if (prefix_len && !have_prefix) return "null prefix with prefix_len > 0";
  if (!have_verdict || !have_found) return "null verdict or found";
  if (n && (!have_in || !have_out || !have_K || !have_key || !have_proof)) return "null in, out, K, key or proof";
  return nullptr;
}
inline const char* refuse_key(uint64_t cap, bool have_seed, uint64_t seed_len, bool have_key) {
  if (cap > ROWS_MAX) return "cap is above EG_SHUFFLE_ROWS_MAX";
  if (seed_len > PREFIX_MAX) return "seed_len is above 255";
  if (seed_len && !have_seed) return "null seed with seed_len > 0";
  if (!have_key) return "null key";
  return nullptr;
}

constexpr unsigned chain_tiles(uint64_t n) { return (unsigned)((n + WAVE_ROWS - 1) / WAVE_ROWS); }
inline unsigned chain_blocks(uint64_t n, unsigned cus) {
  const size_t want = ((size_t)chain_tiles(n) * 64 + NT - 1) / NT, cap = (size_t)(cus ? cus : 1) * CHAIN_BLOCKS_PER_CU;
  return (unsigned)(want < cap ? want : cap);
}
inline unsigned row_blocks(uint64_t n) { return (unsigned)((n + NT - 1) / NT); }

// the caller's scratch of a verification, in bytes from its start (every part 256-byte aligned); N == 0 needs none.  tree, msm_big and
// msm_small are what eg_merkle_tree_scratch_bytes(N) and the product entry's scratch for (4, 2N) and (2, 2) say.
struct Layout {
  unsigned chain_grid;
  size_t prefix, state, leaves, rowbad, tree, upart, big_scalars, big_points, big_r, big_out, big_ok, small_scalars, small_points, small_r,
      small_out, small_ok, tables, msm, total;
};
inline Layout layout(uint64_t n, unsigned cus, size_t tree_bytes, size_t msm_big, size_t msm_small) {
  Layout L{};
  if (n == 0 || n > ROWS_MAX) return L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.chain_grid = chain_blocks(n, cus);
  L.prefix = take(PREFIX_MAX + 1);
  L.state = take(STATE_BYTES);
  L.leaves = take((size_t)n * 32);
  L.rowbad = take((size_t)n);
  L.tree = take(tree_bytes);
  L.upart = take((size_t)row_blocks(n) * 32);
  L.big_scalars = take(BIG_PRODUCTS * 2 * (size_t)n * 32);
  L.big_points = take(BIG_PRODUCTS * 2 * (size_t)n * 32);
  L.big_r = take(BIG_PRODUCTS * 32);
  L.big_out = take(BIG_PRODUCTS * 32);
  L.big_ok = take(BIG_PRODUCTS);
  L.small_scalars = take(SMALL_PRODUCTS * SMALL_TERMS * 32);
  L.small_points = take(SMALL_PRODUCTS * SMALL_TERMS * 32);
  L.small_r = take(SMALL_PRODUCTS * 32);
  L.small_out = take(SMALL_PRODUCTS * 32);
  L.small_ok = take(SMALL_PRODUCTS);
  L.tables = take((size_t)L.chain_grid * NT * 2 * TABLE_BYTES);
  L.msm = take(msm_big > msm_small ? msm_big : msm_small);
  L.total = off;
  return L;
}

}  // namespace egsh
