// share_combine_kernels.cuh -- decryption shares of MANY ciphertexts combined in one pass (eg_combine_shares_batch*, eg_hip.hip):
// for every ciphertext c, D_c = [scale] sum [denominator_j^-1] dh_j over the first `threshold` usable shares (Params::combine_shares,
// src/sharing/mod.rs:302-325 with lagrange_coefficients :139-170) and B_c - D_c, the element the discrete-log solver takes
// (VerifiableDecryption::decrypt_to_element, src/decryption.rs:129-131).  eg_combine_shares opens ONE ciphertext in about a dozen
// synchronised primitive calls; per-precinct tallies are 10^4 .. 10^5 ciphertexts.
//
// One lane owns one ciphertext in each of three kernels (share_combine_host.hpp has the layout of what they exchange):
//   k_sc_select     walks the k columns in the caller's order: a column is usable when its status word is 0 (or no status is given) and
//                   the first 32 bytes of its item - the R the share was proven for - are the ciphertext's R.  Accepted shares of another
//                   R count in bad[0] and are skipped.  The walk ends with the threshold-th usable column (`.take(threshold)`): later
//                   columns are not looked at.  Leaves the column mask, or 0 when there are too few.
//   k_sc_coeffs     the lane's `threshold` scalars scale / denominator_i from the participant indexes of its mask.  Small factors (at
//                   most 64) are multiplied ten at a time in a 64-bit word before they meet a scalar; ONE sc_invert per lane by
//                   Montgomery's trick: prefix products forward, each denominator made a second time on the way back.
//                   Masks mostly agree across a wavefront, but one rejected share changes one lane's set, so every lane computes its own.
//   k_sc_combine    Straus: the chosen shares in chunks of up to 8 on one chain of 252 doublings each (per-lane radix-16 tables in the
//                   caller's scratch, signed digits in LDS: k_prim_msm's form with its device functions), the chunks of a ciphertext one
//                   after the other in the same lane; then B is decoded and D and B - D are encoded (two encodings: the encoder's
//                   inverse square roots are exponentiations, which do not batch).  A chosen dh that does not decode counts in bad[1],
//                   a B that does not in bad[2]; both leave combined = 0 and zero bytes.  Shares that were not chosen are never decoded.
// The lane bodies are plain functions over IO policies, so that the host check build (tests/hostcheck/sharecombinecheck.cpp,
// -DEG_BOUNDCHECK) runs the same code serially on arrays.
#pragma once
#include "ge25519.cuh"
#include "sc25519.cuh"
#include "share_combine_host.hpp"

namespace eg {

constexpr int SC_CHUNK = egsc::CHUNK;

EG_HD int sc_low_bit(u64 x) { return __builtin_ctzll(x); }
EG_HD int sc_high_bit(u64 x) { return 63 - __builtin_clzll(x); }
// a mask the later stages act on: exactly t of the k columns (the scratch is the caller's memory: what it holds is checked, not trusted)
EG_HD bool sc_mask_valid(u64 mask, int k, u32 t) { return (u32)__builtin_popcountll(mask) == t && (k >= 64 || (mask >> k) == 0u); }

// ---- select ----------------------------------------------------------------------------------------------------------------------------
// the column mask of ciphertext c: the first t usable columns, or 0 when the k columns hold fewer
template <class StatusIO, class ItemIO, class CtIO>
EG_HD u64 sc_lane_select(u32& bad0, u32 c, int k, u32 t, const StatusIO& status, const ItemIO& items, const CtIO& cts) {
  u32 r[8];
  cts.load(r, c, 0);
  u64 mask = 0;
  u32 count = 0;
  for (int j = 0; j < k && count < t; ++j) {
    if (!status.accepted(j, c)) continue;                 // items of columns that are not accepted are never read
    u32 w[8];
    items.load(w, j, c, 0);
    u32 diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= w[i] ^ r[i];
    if (diff) { ++bad0; continue; }                       // a share proven for another ciphertext
    mask |= (u64)1 << j;
    ++count;
  }
  return count == t ? mask : 0u;
}
// bit indexes[j] for every column j of the mask
EG_HD u64 sc_used_of(u64 mask, int k, const unsigned char* idx) {
  u64 used = 0;
  for (int j = 0; j < k; ++j) used |= ((mask >> j) & 1u) ? (u64)1 << idx[j] : (u64)0;
  return used;
}

// ---- coefficients ------------------------------------------------------------------------------------------------------------------------
// out = out * acc, acc a product of small factors
EG_HD void sc_mul_small(u32 out[8], u64 acc) {
  u32 f[8];
  sc_from_u64(f, acc);
  sc_mul(out, out, f);
}
// the signed denominator of the participant with index a among the indexes of the mask: prod_b (a == b ? a + 1 : |a - b|), negated when
// an odd number of them lies below a.  Factors are at most 64: ten of them fit a 64-bit word.
EG_HD void sc_denominator(u32 out[8], u64 mask, const unsigned char* idx, u32 a) {
  sc_from_u64(out, 1);
  u64 acc = 1;
  int held = 0;
  bool negative = false;
  for (u64 mm = mask; mm; mm &= mm - 1) {
    const u32 b = idx[sc_low_bit(mm)];
    negative ^= a > b;
    acc *= a == b ? a + 1u : (a > b ? a - b : b - a);
    if (++held == 10) { sc_mul_small(out, acc); acc = 1; held = 0; }
  }
  if (held) sc_mul_small(out, acc);
  u32 n[8];
  sc_neg(n, out);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = negative ? n[i] : out[i];
}
// the scale: prod_b (b + 1)
EG_HD void sc_scale(u32 out[8], u64 mask, const unsigned char* idx) {
  sc_from_u64(out, 1);
  u64 acc = 1;
  int held = 0;
  for (u64 mm = mask; mm; mm &= mm - 1) {
    acc *= idx[sc_low_bit(mm)] + 1u;
    if (++held == 10) { sc_mul_small(out, acc); acc = 1; held = 0; }
  }
  if (held) sc_mul_small(out, acc);
}
// coef[i] = scale / denominator_i for the i-th column of the mask, i in the caller's column order
template <class CoefIO>
EG_HD void sc_lane_coeffs(u64 mask, const unsigned char* idx, CoefIO& coef) {
  u32 run[8], d[8];
  sc_from_u64(run, 1);
  int i = 0;
  for (u64 mm = mask; mm; mm &= mm - 1, ++i) {            // coef[i] = denominator_0 ... denominator_i
    sc_denominator(d, mask, idx, idx[sc_low_bit(mm)]);
    sc_mul(run, run, d);
    coef.store(i, run);
  }
  u32 inv[8], scale[8];
  sc_invert(inv, run);                                     // the lane's only inversion; no denominator is 0 mod l (factors 1..64)
  sc_scale(scale, mask, idx);
  sc_mul(inv, inv, scale);                                 // inv = scale / (denominator_0 ... denominator_i) from here on
  for (u64 mm = mask; mm;) {
    const int j = sc_high_bit(mm);
    mm &= ~((u64)1 << j);
    --i;
    u32 before[8], c[8];
    sc_from_u64(before, 1);
    if (i > 0) coef.load(before, i - 1);
    sc_mul(c, inv, before);
    coef.store(i, c);
    sc_denominator(d, mask, idx, idx[j]);
    sc_mul(inv, inv, d);
  }
}

// ---- combine -----------------------------------------------------------------------------------------------------------------------------
// acc = sum_n [scalar_n] P_n over the n tables and digit rows of a chunk: one chain of 252 doublings (k_prim_msm's loop)
template <class Tables, class Digits>
EG_HD void sc_chain(ge& acc, int n, const Tables& tabs, const Digits& dig) {
  ge_identity(acc);
  ge_cached ident; ge_cached_identity(ident);
#pragma unroll 1
  for (int d = 63; d >= 0; --d) {
    ge_p1p1 tt;
    if (d != 63) {
      ge_p2 q; q.X = acc.X; q.Y = acc.Y; q.Z = acc.Z;
#pragma unroll 1
      for (int r = 0; r < 3; ++r) { ge_dbl(tt, q.X, q.Y, q.Z); ge_dbl_to_p2(q, tt); }
      ge_dbl(tt, q.X, q.Y, q.Z);
      ge_dbl_to_p3(acc, tt);
    }
#pragma unroll 1
    for (int t = 0; t < n; ++t) {
      const int dv = dig.digit(t, d), ad = dv < 0 ? -dv : dv;
      const auto tab = tabs.at(t);
      ge_cached c; tab.load(c, ad == 0 ? 0 : ad - 1);
      fe_cmov(c.YpX, ident.YpX, ad == 0); fe_cmov(c.YmX, ident.YmX, ad == 0);
      fe_cmov(c.Z2, ident.Z2, ad == 0); fe_cmov(c.T2d, ident.T2d, ad == 0);
      ge_cached_cneg(c, dv < 0);
      ge_add(tt, acc, c);
      if (t + 1 == n && d > 0) {              // a doubling follows: T is not needed
        ge_p2 q; ge_add_to_p2(q, tt);
        acc.X = q.X; acc.Y = q.Y; acc.Z = q.Z;
      } else {
        ge_add_to_p3(acc, tt);
      }
    }
  }
}
// D = sum [coef_i] dh_i over the columns of the mask, SC_CHUNK at a time; bad1 counts the chosen dh that do not decode (they add nothing)
template <class ItemIO, class CoefIO, class Tables, class Digits>
EG_HD void sc_lane_combine(ge& D, u32& bad1, u64 mask, u32 c, const ItemIO& items, const CoefIO& coef, Tables& tabs, Digits& dig) {
  ge_identity(D);
  int i = 0;
  u64 mm = mask;
#pragma unroll 1
  while (mm) {
    int n = 0;
#pragma unroll 1
    for (; mm && n < SC_CHUNK; mm &= mm - 1, ++n, ++i) {
      u32 w[8], s[8], dg[8];
      items.load(w, sc_low_bit(mm), c, 1);
      ge p;
      if (!ristretto_decode(p, w)) ++bad1;                // p is then the identity
      coef.load(s, i);
      sc_recode_radix16(dg, s);
#pragma unroll
      for (int q = 0; q < 8; ++q) dig.store(n, q, dg[q]);
      auto tab = tabs.at(n);
      ge_var_table_build(tab, p);
    }
    ge acc, sum;
    sc_chain(acc, n, tabs, dig);
    ge_add_full(sum, D, acc);
    D = sum;
  }
}
// dh = serialize(D) and, when asked for, plain = serialize(B - D); false (bad2 counted) when B does not decode
template <class CtIO>
EG_HD bool sc_lane_finish(u32 dh[8], u32 plain[8], bool want_plain, u32& bad2, u32 c, const ge& D, const CtIO& cts) {
  ristretto_encode(dh, D);
  if (!want_plain) return true;
  u32 w[8];
  cts.load(w, c, 1);
  ge B, P;
  if (!ristretto_decode(B, w)) { ++bad2; return false; }
  ge_sub_full(P, B, D);
  ristretto_encode(plain, P);
  return true;
}

}  // namespace eg

#if defined(__HIPCC__)
#include "device_io.cuh"

namespace eg {

struct ScIndexes { unsigned char v[egsc::MAX_SHARES]; };   // zero-based participant index of every column, by value in the kernel arguments

struct ScStatusDev {
  const u32* st;         // [k][m], or null: every share accepted
  size_t m;
  __device__ __forceinline__ bool accepted(int j, u32 c) const { return !st || st[(size_t)j * m + c] == 0u; }
};
struct ScItemsDev {
  const uint4* items;    // [k][m] items of 128 bytes: R || dh || challenge || response
  size_t m;
  __device__ __forceinline__ void load(u32 w[8], int j, u32 c, int part) const {
    const uint4* p = items + ((size_t)j * m + c) * 8 + (size_t)part * 2;
    const uint4 a = p[0], b = p[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
};
struct ScCtDev {
  const uint4* cts;      // [m] ciphertexts of 64 bytes: R || B
  __device__ __forceinline__ void load(u32 w[8], u32 c, int part) const {
    const uint4* p = cts + (size_t)c * 4 + (size_t)part * 2;
    const uint4 a = p[0], b = p[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
};
struct ScCoefDev {       // [i][word][lane]: a wavefront's access is one row
  u32* base;             // coef + lane
  size_t lanes;
  __device__ __forceinline__ void store(int i, const u32 w[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) base[(size_t)(i * 8 + q) * lanes] = w[q];
  }
  __device__ __forceinline__ void load(u32 w[8], int i) const {
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = base[(size_t)(i * 8 + q) * lanes];
  }
};
struct ScTablesDev {
  uint4* base;           // the lane's `chunk` tables
  __device__ __forceinline__ WsTable at(int n) const { WsTable t; t.base = base + (size_t)n * WS_QUADS; return t; }
};
struct ScDigitsDev {     // [table][word][NT] in LDS
  u32* dig;
  __device__ __forceinline__ void store(int n, int q, u32 v) { dig[(n * 8 + q) * NT + threadIdx.x] = v; }
  __device__ __forceinline__ int digit(int n, int i) const {
    const u32 w = dig[(n * 8 + (i >> 3)) * NT + threadIdx.x];
    const int nib = (int)((w >> (4 * (i & 7))) & 15u);
    return nib >= 8 ? nib - 16 : nib;
  }
};
__device__ __forceinline__ void sc_store8(void* dst, size_t c, const u32 w[8]) {
  uint4* p = static_cast<uint4*>(dst) + c * 2;
  p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// lanes of a slab: ciphertexts first .. first + count - 1; masks[lane]
__global__ void __launch_bounds__(NT) k_sc_select(u32 first, u32 count, int k, u32 t, ScStatusDev status, ScItemsDev items, ScCtDev cts,
                                                  u64* masks, u32* bad) {
  const u32 lane = blockIdx.x * NT + threadIdx.x;
  if (lane >= count) return;
  u32 bad0 = 0;
  masks[lane] = sc_lane_select(bad0, first + lane, k, t, status, items, cts);
  if (bad0) atomicAdd(bad, bad0);
}
__global__ void __launch_bounds__(NT, 2) k_sc_coeffs(u32 count, int k, u32 t, ScIndexes idx, const u64* masks, u32* coef, size_t lanes) {
  __shared__ unsigned char s_idx[egsc::MAX_SHARES];          // the lanes look indexes up by their own column numbers
  if (threadIdx.x < egsc::MAX_SHARES) s_idx[threadIdx.x] = idx.v[threadIdx.x];
  __syncthreads();
  const u32 lane = blockIdx.x * NT + threadIdx.x;
  if (lane >= count) return;
  const u64 mask = masks[lane];
  if (!sc_mask_valid(mask, k, t)) return;
  ScCoefDev io{coef + lane, lanes};
  sc_lane_coeffs(mask, s_idx, io);
}
__global__ void __launch_bounds__(NT, 2) k_sc_combine(u32 first, u32 count, int k, u32 t, int chunk, ScIndexes idx, ScItemsDev items, ScCtDev cts,
                                                      const u64* masks, const u32* coef, size_t lanes, uint4* tables, void* dh, void* plain,
                                                      unsigned char* combined, u64* used, u32* bad) {
  __shared__ u32 s_dig[SC_CHUNK * 8 * NT];                   // radix-16 digits of the chunk's scalars
  const u32 lane = blockIdx.x * NT + threadIdx.x;
  if (lane >= count) return;
  const u32 c = first + lane;
  u64 mask = masks[lane];
  if (!sc_mask_valid(mask, k, t)) mask = 0;
  u32 o_dh[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o_plain[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = mask != 0u;
  if (ok) {
    const ScCoefDev cf{const_cast<u32*>(coef) + lane, lanes};
    ScTablesDev tabs{tables + (size_t)lane * chunk * WS_QUADS};
    ScDigitsDev dig{s_dig};
    ge D;
    u32 bad1 = 0, bad2 = 0;
    sc_lane_combine(D, bad1, mask, c, items, cf, tabs, dig);
    ok = bad1 == 0u;
    if (ok) ok = sc_lane_finish(o_dh, o_plain, plain != nullptr, bad2, c, D, cts);
    if (bad1) atomicAdd(bad + 1, bad1);
    if (bad2) atomicAdd(bad + 2, bad2);
    if (!ok) {
#pragma unroll
      for (int q = 0; q < 8; ++q) { o_dh[q] = 0u; o_plain[q] = 0u; }
    }
  }
  if (dh) sc_store8(dh, c, o_dh);
  if (plain) sc_store8(plain, c, o_plain);
  combined[c] = ok ? 1 : 0;
  if (used) used[c] = ok ? sc_used_of(mask, k, idx.v) : (u64)0;
}

}  // namespace eg
#endif
