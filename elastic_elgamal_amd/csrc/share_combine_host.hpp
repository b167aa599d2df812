// share_combine_host.hpp -- arithmetic of the batched share combination (eg_combine_shares_batch*, eg_hip.hip; kernels:
// share_combine_kernels.cuh): pure host code, no HIP.  tests/hostcheck/sharecombinecheck.cpp compiles it under ASan + UBSan together with
// the lane functions of the kernels.
//
// The pass opens m ciphertexts at once: for ciphertext c the columns (participants) of the caller's order are walked, the first
// `threshold` usable ones are the shares (Params::combine_shares, src/sharing/mod.rs:302-325: `.take(self.threshold)`), their Lagrange
// coefficients come from the chosen participant indexes (lagrange_coefficients, :139-170) and D = sum [coefficient_j] dh_j is the
// decryption [x]R.  One lane owns one ciphertext in every stage; the stages exchange a column mask (8 bytes), the coefficients
// (threshold x 32 bytes) and the radix-16 tables of one chunk of shares (CHUNK x 1152 bytes) per lane through the caller's scratch.
// Long vectors are cut into SLABS of at most SLAB ciphertexts that reuse the same scratch one after the other on the stream, so the
// scratch does not grow with m beyond a slab.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace egsc {

constexpr uint64_t MAX_SHARES = 64;        // EG_COMBINE_SHARES_MAX: a column mask and a `used` mask are one 64-bit word
constexpr int CHUNK = 8;                   // shares on one doubling chain (k_prim_msm's MSM_CHUNK)
constexpr size_t SLAB = (size_t)1 << 17;   // ciphertexts per round of launches: two blocks of 256 lanes on each of 256 compute units
constexpr size_t BLOCK = 256;              // lanes per block: a slab is a whole number of blocks
constexpr size_t TABLE_BYTES = 8 * 144;    // {1..8}P in cached form, 36 words each (WsTable)

struct Layout {
  size_t lanes;                            // lanes of a slab: m rounded up to whole blocks, at most SLAB
  size_t mask, coef, tables, total;        // byte offsets: mask[lanes] (uint64), coef[threshold][8][lanes] (uint32), tables[lanes][chunk]
  int chunk;                               // tables per lane: min(threshold, CHUNK)
};
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
inline Layout layout(uint64_t threshold, size_t m) {
  Layout L;
  const size_t blocks = (m + BLOCK - 1) / BLOCK * BLOCK;
  L.lanes = blocks < SLAB ? blocks : SLAB;
  L.chunk = (int)(threshold < (uint64_t)CHUNK ? threshold : (uint64_t)CHUNK);
  L.mask = 0;
  L.coef = up256(L.lanes * 8);
  L.tables = L.coef + up256(L.lanes * (size_t)threshold * 32);
  L.total = L.tables + up256(L.lanes * (size_t)L.chunk * TABLE_BYTES);
  return L;
}

// what the size function and both entries refuse about the numbers alone
inline const char* refuse_sizes(uint64_t shares, uint64_t threshold, size_t m) {
  if (shares == 0 || shares > MAX_SHARES) return "shares is outside 1..EG_COMBINE_SHARES_MAX";
  if (threshold < 1 || threshold > shares) return "threshold is outside 1..shares";
  if (m >= ((size_t)1 << 31)) return "m is 2^31 or more";
  return nullptr;
}
// ... and about the columns: k of them with the zero-based participant indexes of the caller's order
inline const char* refuse_columns(uint64_t shares, int k, const uint64_t* indexes) {
  if (k < 0 || (uint64_t)k > shares) return "k is outside 0..shares";
  if (k && !indexes) return "null indexes";
  uint64_t seen = 0;
  for (int j = 0; j < k; ++j) {
    if (indexes[j] >= shares) return "a share index exceeds the number of participants";
    if ((seen >> indexes[j]) & 1u) return "duplicate share index";
    seen |= (uint64_t)1 << indexes[j];
  }
  return nullptr;
}
inline size_t scratch_bytes(uint64_t threshold, size_t m) {
  if (threshold < 1 || threshold > MAX_SHARES || m == 0 || m >= ((size_t)1 << 31)) return 0;
  return layout(threshold, m).total;
}

}  // namespace egsc
