// ed25519.cuh -- Ed25519 (RFC 8032, pure EdDSA: no context, no prehash) on the engine's curve: the Edwards point codec and the lane
// functions of the verifier and of the signer.  Host and device: tests/hostcheck/ed25519check.cpp runs the same code serially.
//
// The Ristretto generator IS the Ed25519 base point B, so the generator's comb table (ge_fixed_mul_add) serves unchanged, and
// R' = [S]B - [h]A is one variable-base product over a per-lane radix-16 table of -A plus one comb - a double-base product of one term.
//
// THE RULE of a verification (include/eg_hip.h has it in full), first failure wins, detail in status >> 8:
//   1  S >= l (not canonical)
//   2  A does not decode.  The decoding is STRICT: y >= p refused, x = 0 with the sign bit set refused, no square root refused.
//   3  [8]A is the identity (A has small order)
//   4  the RFC 8032 5.1.2 encoding of R' = [S]B - [h]A, h = SHA-512(R || A || M) mod l, differs from the 32 bytes R.
// R is never decoded: a non-canonical R can never match, and a small-order R is not separately refused.  This is the COFACTORLESS
// byte comparison, the check OpenSSL makes.
//
// TIMING: everything here is variable time - verification sees public data only, and the signer is a maker of test and benchmark items
// (branches and table lookups depend on the secret scalar): it must not sign for a voter.
#pragma once
#include "ge25519.cuh"
#include "sc25519.cuh"
#include "sha512.cuh"

namespace eg {

constexpr u32 ED_ST_BAD_SIGNATURE = 15;           // EG_ST_BAD_SIGNATURE
enum : u32 { ED_OK = 0, ED_BAD_S = 1, ED_BAD_KEY = 2, ED_SMALL_ORDER = 3, ED_MISMATCH = 4, ED_BAD_INDEX = 5 };
EG_HD u32 ed_status(u32 detail) { return detail ? (ED_ST_BAD_SIGNATURE | (detail << 8)) : 0u; }

// RFC 8032 5.1.3, strict.  w = little-endian words of the encoding: y in bits 0..254, the sign of x in bit 255.
EG_HD bool ed_decode(ge& p, const u32 w[8]) {
  const fe d = EG_FE_D;
  u32 yw[8], chk[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) yw[i] = w[i];
  yw[7] &= 0x7fffffffu;
  const bool sign = (w[7] >> 31) != 0;
  fe y, one, yy, u, v, x;
  fe_1(one);
  fe_from_words(y, yw);
  fe_to_words(chk, y);
  u32 diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= chk[i] ^ yw[i];
  if (diff) return false;                              // y >= p
  fe_sq(yy, y);
  fe_sub(u, yy, one); fe_carry(u);                     // y^2 - 1
  fe_mul(v, yy, d);
  fe_add(v, v, one); fe_carry(v);                      // d y^2 + 1 (never 0: -1/d is no square)
  if (!fe_sqrt_ratio_m1(x, u, v)) return false;        // x = the even root of u / v
  if (fe_iszero(x) && sign) return false;
  fe n; fe_neg(n, x); fe_carry(n);
  fe_cmov(x, n, sign);
  p.X = x; p.Y = y; fe_1(p.Z);
  fe_mul(p.T, x, y);
  return true;
}
// RFC 8032 5.1.2: one inversion
EG_HD void ed_encode(u32 w[8], const ge& p) {
  fe zi, x, y;
  fe_invert(zi, p.Z);
  fe_mul(x, p.X, zi);
  fe_mul(y, p.Y, zi);
  fe_to_words(w, y);
  w[7] |= fe_isnegative(x) ? 0x80000000u : 0u;
}
// [8]P = the identity (0 : z : z)
EG_HD bool ed_is_small_order(const ge& p) {
  ge_p1p1 t; ge_p2 q;
  q.X = p.X; q.Y = p.Y; q.Z = p.Z;
#pragma unroll 1
  for (int k = 0; k < 3; ++k) { ge_dbl(t, q.X, q.Y, q.Z); ge_dbl_to_p2(q, t); }
  return fe_iszero(q.X) && fe_eq(q.Y, q.Z);
}

// h = the 64 digest bytes mod l
EG_HD void ed_hash_mod_l(u32 h[8], const ShaRanges& r) {
  u32 dg[16];
  sha512_ranges(dg, r);
  sc_from_wide(h, dg);
}

// checks 1 .. 4 of the rule given h: the detail (0 = accepted).  tab: the lane's radix-16 table (ge_var_table_build), tg: the comb of B.
template <class TableIO, class FixedIO>
EG_HD u32 ed_verify_lane(TableIO& tab, FixedIO& tg, const u32 Rw[8], const u32 Sw[8], const u32 Aw[8], const u32 hw[8]) {
  if (!sc_is_canonical(Sw)) return ED_BAD_S;
  ge A;
  if (!ed_decode(A, Aw)) return ED_BAD_KEY;
  if (ed_is_small_order(A)) return ED_SMALL_ORDER;
  ge negA; ge_neg(negA, A);
  ge_var_table_build(tab, negA);
  u32 dg[8], sk[EG_COMB_WORDS], enc[8];
  sc_recode_radix16(dg, hw);
  ge acc;
  ge_var_mul(acc, tab, dg);                            // [h](-A): one chain of 252 doublings
  sc_recode_comb(sk, Sw);
  ge_fixed_mul_add(acc, tg, sk);                       // + [S]B
  ed_encode(enc, acc);
  u32 diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= enc[i] ^ Rw[i];
  return diff ? ED_MISMATCH : ED_OK;
}

// ---- the signer (RFC 8032 5.1.5 / 5.1.6): VARIABLE TIME, a maker of test and benchmark items ----------------------------------------
EG_HD void ed_words_to_bytes(unsigned char* out, const u32* w, int words) {
  for (int i = 0; i < words; ++i) { out[4 * i] = (unsigned char)w[i]; out[4 * i + 1] = (unsigned char)(w[i] >> 8); out[4 * i + 2] = (unsigned char)(w[i] >> 16); out[4 * i + 3] = (unsigned char)(w[i] >> 24); }
}
template <class FixedIO>
EG_HD void ed_mul_base_encode(u32 enc[8], FixedIO& tg, const u32 k[8]) {
  u32 sk[EG_COMB_WORDS];
  sc_recode_comb(sk, k);
  ge acc; ge_identity(acc);
  ge_fixed_mul_add(acc, tg, sk);
  ed_encode(enc, acc);
}
// seed -> a mod l (the clamped scalar is below 2^255; the comb wants it below 2^254, and B has order l), the hash prefix, A = [a]B
template <class FixedIO>
EG_HD void ed_expand_seed(u32 a[8], u32 hash_prefix[8], u32 Aw[8], FixedIO& tg, const unsigned char* seed) {
  u32 dg[16], wide[16];
  sha512_ranges(dg, sha_ranges(seed, 32));
#pragma unroll
  for (int i = 0; i < 8; ++i) { wide[i] = dg[i]; wide[8 + i] = 0; hash_prefix[i] = dg[8 + i]; }
  wide[0] &= 0xfffffff8u;
  wide[7] = (wide[7] & 0x7fffffffu) | 0x40000000u;
  sc_from_wide(a, wide);
  ed_mul_base_encode(Aw, tg, a);
}
template <class FixedIO>
EG_HD void ed_keypair_lane(u32 Aw[8], FixedIO& tg, const unsigned char* seed) {
  u32 a[8], hp[8];
  ed_expand_seed(a, hp, Aw, tg, seed);
}
// sig = R || S over M = prefix || msg
template <class FixedIO>
EG_HD void ed_sign_lane(u32 sig[16], FixedIO& tg, const unsigned char* seed, const unsigned char* prefix, size_t prefix_len,
                        const unsigned char* msg, size_t msg_len) {
  u32 a[8], hp[8], Aw[8], r[8], h[8];
  ed_expand_seed(a, hp, Aw, tg, seed);
  unsigned char b0[32], b1[32];
  ed_words_to_bytes(b0, hp, 8);
  ed_hash_mod_l(r, sha_ranges(b0, 32, prefix, prefix_len, msg, msg_len));
  ed_mul_base_encode(sig, tg, r);
  ed_words_to_bytes(b0, sig, 8);
  ed_words_to_bytes(b1, Aw, 8);
  ed_hash_mod_l(h, sha_ranges(b0, 32, b1, 32, prefix, prefix_len, msg, msg_len));
  sc_muladd(sig + 8, h, a, r);
}

}  // namespace eg
