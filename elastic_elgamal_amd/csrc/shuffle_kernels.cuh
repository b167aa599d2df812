// shuffle_kernels.cuh -- verification of a re-encryption shuffle of the board (eg_shuffle_*: eg_hip.hip; the rule: include/eg_hip.h,
// "re-encryption shuffles"; sizes, argument rules and the scratch layout: shuffle_host.hpp; the model: tests/shuffle_ref.py).
//
// The lane functions in the first half are host and device code: tests/hostcheck/shufflecheck.cpp runs them serially on arrays.
// THE PASS, every stage a kernel boundary on the caller's stream (no lane waits on another workgroup):
//   k_shuffle_begin    one lane: the found words
//   k_shuffle_leaf1    one lane per row: leaf1_i, the row's points copied into the products' point arrays, the five decodings that say
//                      whether the row's in, out and c are elements (a byte per row)
//   (tree)             root1 = eg_merkle_tree_device over the leaves, as it is
//   k_shuffle_seed     one lane: seed1
//   k_shuffle_leaf2    one lane per row: leaf2_i; (tree) root2
//   k_shuffle_x        one lane: x and -x
//   k_shuffle_scalars  one lane per row: u_i, then -x u_i and s'_i into the products' scalar arrays; the workgroup multiplies its u_i
//   k_shuffle_fold     one workgroup: u = the product of the workgroups' products; the scalars and points of the two small products
//   k_shuffle_chain    the hot row kernel: CHAIN of every row, 63 rows a wavefront (below)
//   (products)         eg_vartime_multi_mul_batch_device twice: four products of 2N terms (T1, T3, T41 without K, T42), two of two
//                      terms (T2 and [-s4]K)
//   k_shuffle_close    one lane: compares with the head, masks, writes the verdict
// THE CHAIN KERNEL.  Row i needs the decoded c^_i and c^_(i-1).  A wavefront takes 63 consecutive rows: lane l decodes chain element
// 63 w + l - 1 (lane 0 of the first tile: H_0), so every element is decoded once by the wavefront that needs it twice, and lanes 1 .. 63
// fetch their predecessor's point from lane l - 1 with wavefront shuffles (36 limbs and the flag).  Each of those lanes then runs
// [-x]c^_i + [s'_i]c^_(i-1) on ONE chain of 252 doublings over two radix-16 tables of its own (the primitive tier's lane with two terms),
// adds [s^_i]G from the generator's comb, encodes and compares with t^_i: a bit per row leaves the kernel, not a point.
// Everything is variable time: a shuffle proof is public data.
#pragma once
#include "ge25519.cuh"
#include "sc25519.cuh"
#include "sha512.cuh"
#include "shuffle_host.hpp"
#if defined(__HIPCC__)
#include "device_io.cuh"
#endif

namespace eg {

enum : u32 { SHUF_BAD_ENCODING = 1, SHUF_T1 = 2, SHUF_T2 = 4, SHUF_T3 = 8, SHUF_T41 = 16, SHUF_T42 = 32, SHUF_CHAIN = 64 };
enum : u32 { SHUF_ROW_BAD = 1, SHUF_ROW_CHAIN = 2 };
// words of the state block
enum : int { SHUF_ST_SEED1 = 0, SHUF_ST_ROOT1 = 16, SHUF_ST_ROOT2 = 24, SHUF_ST_X = 32, SHUF_ST_NEGX = 40, SHUF_ST_K = 48, SHUF_ST_HEADBAD = 56 };

// a hash input assembled in private memory: the inputs here are short, of many parts and hashed once
struct ShufMsg {
  unsigned char b[384];
  u32 len;
  EG_HD void open() { len = 0; }
  EG_HD void bytes(const void* p, u32 n) {
    const unsigned char* s = static_cast<const unsigned char*>(p);
    for (u32 i = 0; i < n; ++i) b[len + i] = s[i];
    len += n;
  }
  EG_HD void byte(u32 v) { b[len++] = (unsigned char)v; }
  EG_HD void words(const u32* w, int n) {
    for (int i = 0; i < n; ++i) { b[len] = (unsigned char)w[i]; b[len + 1] = (unsigned char)(w[i] >> 8); b[len + 2] = (unsigned char)(w[i] >> 16); b[len + 3] = (unsigned char)(w[i] >> 24); len += 4; }
  }
  EG_HD void le64(u64 v) { for (int i = 0; i < 8; ++i) b[len++] = (unsigned char)(v >> (8 * i)); }
  EG_HD void digest(u32 dg[16]) const { sha512_ranges(dg, sha_ranges(b, len)); }
};
EG_HD void shuf_ld8(u32 w[8], const u32* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
}
EG_HD void shuf_st8(u32* p, const u32 w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = w[i];
}
EG_HD void shuf_zero8(u32 w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0;
}

// ---- lane functions ----------------------------------------------------------------------------------------------------------------------
// H_j: the first candidate that is a non-identity element; returns the tries it took, 0 when `tries` candidates gave none (out zeroed)
EG_HD u32 shuffle_key_lane(u32 out[8], const unsigned char* seed, u32 seed_len, u64 j, u32 tries) {
  ShufMsg m; m.open();
  m.bytes("eg-shuffle-v1/generator", 23); m.byte(seed_len); m.bytes(seed, seed_len); m.le64(j);
  const u32 at = m.len;
  m.len += 4;
  for (u32 ctr = 0; ctr < tries; ++ctr) {
    m.b[at] = (unsigned char)ctr; m.b[at + 1] = (unsigned char)(ctr >> 8); m.b[at + 2] = (unsigned char)(ctr >> 16); m.b[at + 3] = (unsigned char)(ctr >> 24);
    u32 dg[16];
    m.digest(dg);
    dg[7] &= 0x7fffffffu;
    u32 any = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= dg[i];
    ge p;
    if (any && ristretto_decode(p, dg)) { shuf_st8(out, dg); return ctr + 1; }
  }
  shuf_zero8(out);
  return 0;
}
// leaf1_i = H32(0x00 || in_i || out_i || c_i || H_(i+1))
EG_HD void shuffle_leaf1_lane(u32 leaf[8], const u32 in[16], const u32 out[16], const u32 c[8], const u32 h[8]) {
  ShufMsg m; m.open();
  m.byte(0); m.words(in, 16); m.words(out, 16); m.words(c, 8); m.words(h, 8);
  u32 dg[16];
  m.digest(dg);
  shuf_st8(leaf, dg);
}
// leaf2_i = H32(0x00 || c^_i || t^_i)
EG_HD void shuffle_leaf2_lane(u32 leaf[8], const u32 chat[8], const u32 that[8]) {
  ShufMsg m; m.open();
  m.byte(0); m.words(chat, 8); m.words(that, 8);
  u32 dg[16];
  m.digest(dg);
  shuf_st8(leaf, dg);
}
EG_HD void shuffle_seed_lane(u32 seed1[16], const unsigned char* prefix, u32 prefix_len, u64 n, const u32 K[8], const u32 h0[8], const u32 root1[8]) {
  ShufMsg m; m.open();
  m.bytes("eg-shuffle-v1/seed", 18); m.byte(prefix_len); m.bytes(prefix, prefix_len); m.le64(n); m.words(K, 8); m.words(h0, 8); m.words(root1, 8);
  m.digest(seed1);
}
EG_HD void shuffle_u_lane(u32 u[8], const u32 seed1[16], u64 i) {
  ShufMsg m; m.open();
  m.bytes("eg-shuffle-v1/u", 15); m.words(seed1, 16); m.le64(i);
  u32 dg[16];
  m.digest(dg);
  sc_from_wide(u, dg);
}
// head = the proof's head: t1 t2 t3 t41 t42 are its first 40 words
EG_HD void shuffle_x_lane(u32 x[8], const u32 seed1[16], const u32 root2[8], const u32* head) {
  ShufMsg m; m.open();
  m.bytes("eg-shuffle-v1/c", 15); m.words(seed1, 16); m.words(root2, 8); m.words(head, 40);
  u32 dg[16];
  m.digest(dg);
  sc_from_wide(x, dg);
}
// CHAIN of one row given both decoded chain elements and canonical scalars: true when enc([-x]cur + [s^]G + [s']prev) differs from t^
template <class TableIO, class FixedIO>
EG_HD bool shuffle_chain_row(TableIO& tab_cur, TableIO& tab_prev, FixedIO& tg, const ge& cur, const ge& prev, const u32 negx[8], const u32 shat[8],
                             const u32 sprime[8], const u32 that[8]) {
  ge_var_table_build(tab_cur, cur);
  ge_var_table_build(tab_prev, prev);
  u32 d0[8], d1[8];
  sc_recode_radix16(d0, negx);
  sc_recode_radix16(d1, sprime);
  ge acc; ge_identity(acc);
  ge_cached ident; ge_cached_identity(ident);
#pragma unroll 1
  for (int d = 63; d >= 0; --d) {
    ge_p1p1 tt;
    if (d != 63) {
      ge_p2 q; q.X = acc.X; q.Y = acc.Y; q.Z = acc.Z;
#pragma unroll 1
      for (int k = 0; k < 3; ++k) { ge_dbl(tt, q.X, q.Y, q.Z); ge_dbl_to_p2(q, tt); }
      ge_dbl(tt, q.X, q.Y, q.Z);
      ge_dbl_to_p3(acc, tt);
    }
    // the two terms, written out: a rolled loop over them makes the compiler index the digit arrays in private memory
    {
      const int dv = sc_digit16(d0, d), ad = dv < 0 ? -dv : dv;
      ge_cached c; tab_cur.load(c, ad == 0 ? 0 : ad - 1);
      fe_cmov(c.YpX, ident.YpX, ad == 0); fe_cmov(c.YmX, ident.YmX, ad == 0);
      fe_cmov(c.Z2, ident.Z2, ad == 0); fe_cmov(c.T2d, ident.T2d, ad == 0);
      ge_cached_cneg(c, dv < 0);
      ge_add(tt, acc, c);
      ge_add_to_p3(acc, tt);
    }
    {
      const int dv = sc_digit16(d1, d), ad = dv < 0 ? -dv : dv;
      ge_cached c; tab_prev.load(c, ad == 0 ? 0 : ad - 1);
      fe_cmov(c.YpX, ident.YpX, ad == 0); fe_cmov(c.YmX, ident.YmX, ad == 0);
      fe_cmov(c.Z2, ident.Z2, ad == 0); fe_cmov(c.T2d, ident.T2d, ad == 0);
      ge_cached_cneg(c, dv < 0);
      ge_add(tt, acc, c);
      if (d > 0) {                              // a doubling follows: T is not needed
        ge_p2 q; ge_add_to_p2(q, tt);
        acc.X = q.X; acc.Y = q.Y; acc.Z = q.Z;
      } else {
        ge_add_to_p3(acc, tt);
      }
    }
  }
  u32 sk[EG_COMB_WORDS], enc[8];
  sc_recode_comb(sk, shat);
  ge_fixed_mul_add(acc, tg, sk);
  ristretto_encode(enc, acc);
  u32 diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= enc[i] ^ that[i];
  return diff != 0;
}
// the word of a row: rowbad = the leaf pass's byte; ok_cur / ok_prev = whether c^_i / c^_(i-1) decoded.  The chain is evaluated only
// where both decoded and both scalars are canonical.
EG_HD bool shuffle_row_evaluates(bool ok_cur, bool ok_prev, const u32 shat[8], const u32 sprime[8]) {
  return ok_cur && ok_prev && sc_is_canonical(shat) && sc_is_canonical(sprime);
}
EG_HD u32 shuffle_row_word(bool rowbad, bool ok_cur, const u32 shat[8], const u32 sprime[8], bool chain_fails) {
  const bool bad = rowbad || !ok_cur || !sc_is_canonical(shat) || !sc_is_canonical(sprime);
  return (bad ? SHUF_ROW_BAD : 0u) | (chain_fails ? SHUF_ROW_CHAIN : 0u);
}
// the closing lane: out_big = T1, T3, T41 without K, T42; out_small = T2, [-s4]K; ok = the products' flags; found = the row counts
EG_HD u32 shuffle_close_lane(const u32* head, const u32* out_big, const unsigned char* ok_big, const u32* out_small, const unsigned char* ok_small,
                             const u32* found, u32 headbad) {
  bool bad = headbad != 0 || found[0] != 0;
  for (int k = 0; k < (int)egsh::BIG_PRODUCTS; ++k) bad = bad || !ok_big[k];
  for (int k = 0; k < (int)egsh::SMALL_PRODUCTS; ++k) bad = bad || !ok_small[k];
  if (bad) return SHUF_BAD_ENCODING;
  u32 t41[8];
  {
    ge a, b, s;
    ristretto_decode(a, out_big + 16);
    ristretto_decode(b, out_small + 8);
    ge_add_full(s, a, b);
    ristretto_encode(t41, s);
  }
  u32 mask = found[1] ? (u32)SHUF_CHAIN : 0u;
  u32 d1 = 0, d2 = 0, d3 = 0, d41 = 0, d42 = 0;
  for (int i = 0; i < 8; ++i) {
    d1 |= out_big[i] ^ head[i]; d2 |= out_small[i] ^ head[8 + i]; d3 |= out_big[8 + i] ^ head[16 + i];
    d41 |= t41[i] ^ head[24 + i]; d42 |= out_big[24 + i] ^ head[32 + i];
  }
  return mask | (d1 ? (u32)SHUF_T1 : 0u) | (d2 ? (u32)SHUF_T2 : 0u) | (d3 ? (u32)SHUF_T3 : 0u) | (d41 ? (u32)SHUF_T41 : 0u) | (d42 ? (u32)SHUF_T42 : 0u);
}

#if defined(__HIPCC__)
// ---- kernels -------------------------------------------------------------------------------------------------------------------------------
struct ShufKeyArgs { unsigned char seed[256]; u32 seed_len; u64 cap; u32 tries; };
__global__ void __launch_bounds__(NT) k_shuffle_key(ShufKeyArgs a, u32* key, u32* exhausted) {
  const u64 j = (u64)blockIdx.x * NT + threadIdx.x;
  if (j > a.cap) return;
  u32 h[8];
  if (!shuffle_key_lane(h, a.seed, a.seed_len, j, a.tries)) atomicAdd(exhausted, 1u);
  shuf_st8(key + j * 8, h);
}

// the device arrays of a verification
struct ShufDev {
  u64 n;
  const u32 *in, *out, *key, *proof;         // rows of 16 words; H_0 .. ; head, then c, c^, t^, s^, s' planar
  const unsigned char* prefix; u32 prefix_len;
  u32* state;
  u32* leaves;
  unsigned char* rowbad;
  u32* upart;
  u32 *big_scalars, *big_points, *big_r;      // [4][2N][8], [4][2N][8], [4][8]
  u32 *small_scalars, *small_points, *small_r;
  u32* rows;                                  // or null
  u32* found;
  __device__ __forceinline__ const u32* c(u64 i) const { return proof + 72 + i * 8; }
  __device__ __forceinline__ const u32* chat(u64 i) const { return proof + 72 + (n + i) * 8; }
  __device__ __forceinline__ const u32* that(u64 i) const { return proof + 72 + (2 * n + i) * 8; }
  __device__ __forceinline__ const u32* shat(u64 i) const { return proof + 72 + (3 * n + i) * 8; }
  __device__ __forceinline__ const u32* sprime(u64 i) const { return proof + 72 + (4 * n + i) * 8; }
};

__global__ void __launch_bounds__(64) k_shuffle_begin(u32* found, u32* verdict) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { found[0] = 0; found[1] = 0; found[2] = 0xffffffffu; found[3] = 0xffffffffu; *verdict = 0; }
}

__global__ void __launch_bounds__(NT) k_shuffle_leaf1(ShufDev D) {
  const u64 i = (u64)blockIdx.x * NT + threadIdx.x;
  if (i >= D.n) return;
  u32 in[16], out[16], c[8], h[8], leaf[8];
  shuf_ld8(in, D.in + i * 16); shuf_ld8(in + 8, D.in + i * 16 + 8);
  shuf_ld8(out, D.out + i * 16); shuf_ld8(out + 8, D.out + i * 16 + 8);
  shuf_ld8(c, D.c(i)); shuf_ld8(h, D.key + (i + 1) * 8);
  shuffle_leaf1_lane(leaf, in, out, c, h);
  shuf_st8(D.leaves + i * 8, leaf);
  // the products' points: problem 0 and 1 (c, H), 2 (B, B'), 3 (R, R'); term i and term N + i
  const u64 two_n = 2 * D.n;
  shuf_st8(D.big_points + (0 * two_n + i) * 8, c); shuf_st8(D.big_points + (0 * two_n + D.n + i) * 8, h);
  shuf_st8(D.big_points + (1 * two_n + i) * 8, c); shuf_st8(D.big_points + (1 * two_n + D.n + i) * 8, h);
  shuf_st8(D.big_points + (2 * two_n + i) * 8, in + 8); shuf_st8(D.big_points + (2 * two_n + D.n + i) * 8, out + 8);
  shuf_st8(D.big_points + (3 * two_n + i) * 8, in); shuf_st8(D.big_points + (3 * two_n + D.n + i) * 8, out);
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < 5; ++k) {
    u32 w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = k == 0 ? in[q] : k == 1 ? in[8 + q] : k == 2 ? out[q] : k == 3 ? out[8 + q] : c[q];
    ge p;
    ok = ristretto_decode(p, w) && ok;
  }
  D.rowbad[i] = ok ? 0 : 1;
}

__global__ void __launch_bounds__(NT) k_shuffle_leaf2(ShufDev D) {
  const u64 i = (u64)blockIdx.x * NT + threadIdx.x;
  if (i >= D.n) return;
  u32 a[8], b[8], leaf[8];
  shuf_ld8(a, D.chat(i)); shuf_ld8(b, D.that(i));
  shuffle_leaf2_lane(leaf, a, b);
  shuf_st8(D.leaves + i * 8, leaf);
}

__global__ void __launch_bounds__(64) k_shuffle_seed(ShufDev D) {
  if (blockIdx.x || threadIdx.x) return;
  u32 K[8], h0[8], r1[8], seed1[16];
  shuf_ld8(K, D.state + SHUF_ST_K); shuf_ld8(h0, D.key); shuf_ld8(r1, D.state + SHUF_ST_ROOT1);
  shuffle_seed_lane(seed1, D.prefix, D.prefix_len, D.n, K, h0, r1);
  shuf_st8(D.state + SHUF_ST_SEED1, seed1); shuf_st8(D.state + SHUF_ST_SEED1 + 8, seed1 + 8);
}

__global__ void __launch_bounds__(64) k_shuffle_x(ShufDev D) {
  if (blockIdx.x || threadIdx.x) return;
  u32 seed1[16], r2[8], x[8], nx[8];
  shuf_ld8(seed1, D.state + SHUF_ST_SEED1); shuf_ld8(seed1 + 8, D.state + SHUF_ST_SEED1 + 8); shuf_ld8(r2, D.state + SHUF_ST_ROOT2);
  shuffle_x_lane(x, seed1, r2, D.proof);
  sc_neg(nx, x);
  shuf_st8(D.state + SHUF_ST_X, x); shuf_st8(D.state + SHUF_ST_NEGX, nx);
}

// the product of the workgroup's scalars (every lane hands one in); valid in lane 0
__device__ __forceinline__ void shuf_block_product(u32 v[8], u32* sh /* [NT][8] */) {
  shuf_st8(sh + threadIdx.x * 8, v);
  __syncthreads();
#pragma unroll 1
  for (int step = NT / 2; step >= 1; step >>= 1) {
    if ((int)threadIdx.x < step) {
      u32 a[8], b[8], p[8];
      shuf_ld8(a, sh + threadIdx.x * 8); shuf_ld8(b, sh + (threadIdx.x + step) * 8);
      sc_mul(p, a, b);
      shuf_st8(sh + threadIdx.x * 8, p);
    }
    __syncthreads();
  }
  shuf_ld8(v, sh);
}

__global__ void __launch_bounds__(NT) k_shuffle_scalars(ShufDev D) {
  __shared__ u32 sh[NT * 8];
  const u64 i = (u64)blockIdx.x * NT + threadIdx.x;
  u32 u[8];
  shuf_zero8(u); u[0] = 1;
  if (i < D.n) {
    u32 seed1[16], x[8], nx[8], xu[8], sp[8];
    shuf_ld8(seed1, D.state + SHUF_ST_SEED1); shuf_ld8(seed1 + 8, D.state + SHUF_ST_SEED1 + 8);
    shuf_ld8(x, D.state + SHUF_ST_X); shuf_ld8(nx, D.state + SHUF_ST_NEGX);
    shuffle_u_lane(u, seed1, i);
    sc_mul(xu, nx, u);
    shuf_ld8(sp, D.sprime(i));
    if (!sc_is_canonical(sp)) shuf_zero8(sp);           // the row is flagged by the chain kernel; the products stay below l
    const u64 two_n = 2 * D.n;
    shuf_st8(D.big_scalars + (0 * two_n + i) * 8, nx); shuf_st8(D.big_scalars + (0 * two_n + D.n + i) * 8, x);
#pragma unroll 1
    for (u64 k = 1; k < 4; ++k) { shuf_st8(D.big_scalars + (k * two_n + i) * 8, xu); shuf_st8(D.big_scalars + (k * two_n + D.n + i) * 8, sp); }
  }
  shuf_block_product(u, sh);
  if (threadIdx.x == 0) shuf_st8(D.upart + (u64)blockIdx.x * 8, u);
}

__global__ void __launch_bounds__(NT) k_shuffle_fold(ShufDev D, u32 n_parts) {
  __shared__ u32 sh[NT * 8];
  u32 u[8];
  shuf_zero8(u); u[0] = 1;
#pragma unroll 1
  for (u32 k = threadIdx.x; k < n_parts; k += NT) {
    u32 a[8], p[8];
    shuf_ld8(a, D.upart + (u64)k * 8);
    sc_mul(p, u, a);
    shuf_st8(u, p);
  }
  shuf_block_product(u, sh);
  if (threadIdx.x) return;
  u32 x[8], nx[8], s[4][8], zero[8], w[8];
  shuf_zero8(zero);
  shuf_ld8(x, D.state + SHUF_ST_X); shuf_ld8(nx, D.state + SHUF_ST_NEGX);
  u32 headbad = 0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    shuf_ld8(s[k], D.proof + 40 + k * 8);
    if (!sc_is_canonical(s[k])) { headbad = 1; shuf_zero8(s[k]); }
  }
  D.state[SHUF_ST_HEADBAD] = headbad;
  u32 ns4[8];
  sc_neg(ns4, s[3]);
  // big: T1 + [s1]G, T3 + [s3]G, T41 (K apart), T42 - [s4]G
  shuf_st8(D.big_r, s[0]); shuf_st8(D.big_r + 8, s[2]); shuf_st8(D.big_r + 16, zero); shuf_st8(D.big_r + 24, ns4);
  // small 0: [-x]c^_(N-1) + [x u]H_0 + [s2]G; small 1: [-s4]K + [0]H_0
  sc_mul(w, x, u);
  shuf_st8(D.small_scalars, nx); shuf_st8(D.small_scalars + 8, w); shuf_st8(D.small_scalars + 16, ns4); shuf_st8(D.small_scalars + 24, zero);
  shuf_st8(D.small_r, s[1]); shuf_st8(D.small_r + 8, zero);
  shuf_ld8(w, D.chat(D.n - 1)); shuf_st8(D.small_points, w);
  shuf_ld8(w, D.key); shuf_st8(D.small_points + 8, w); shuf_st8(D.small_points + 24, w);
  shuf_ld8(w, D.state + SHUF_ST_K); shuf_st8(D.small_points + 16, w);
}

__global__ void __launch_bounds__(NT, 2) k_shuffle_chain(ShufDev D, const uint4* tabG, uint4* ws) {
  const FixedTable tg(tabG);
  uint4* mine = ws + ((size_t)blockIdx.x * NT + threadIdx.x) * 2 * WS_QUADS;
  WsTable tab_cur, tab_prev;
  tab_cur.base = mine; tab_prev.base = mine + WS_QUADS;
  const int lane = threadIdx.x & 63;
  const u64 waves = (u64)gridDim.x * (NT / 64), tiles = egsh::chain_tiles(D.n);
  u32 negx[8];
  shuf_ld8(negx, D.state + SHUF_ST_NEGX);
#pragma unroll 1
  for (u64 tile = (u64)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); tile < tiles; tile += waves) {      // wavefront-uniform
    // lane l decodes element 63 tile + l - 1 (H_0 in front of row 0); lanes past the end decode the identity's zeros
    const u64 e = tile * egsh::WAVE_ROWS + (u64)lane;        // element index + 1
    u32 w[8];
    shuf_zero8(w);
    if (e == 0) shuf_ld8(w, D.key);
    else if (e <= D.n) shuf_ld8(w, D.chat(e - 1));
    ge cur, prev;
    const bool ok_cur = ristretto_decode(cur, w);
    u32 pw[PT_WORDS];
    ge_to_words(pw, cur);
#pragma unroll
    for (int q = 0; q < PT_WORDS; ++q) pw[q] = __shfl_up(pw[q], 1);
    words_to_ge(prev, pw);
    const bool ok_prev = __shfl_up((int)ok_cur, 1) != 0;
    const u64 row = e - 1;
    const bool have = lane >= 1 && e <= D.n;
    if (have) {                                  // no lane leaves the loop body early: the next tile shuffles again
      u32 shat[8], sprime[8], that[8];
      shuf_ld8(shat, D.shat(row)); shuf_ld8(sprime, D.sprime(row));
      bool fails = false;
      if (shuffle_row_evaluates(ok_cur, ok_prev, shat, sprime)) {
        shuf_ld8(that, D.that(row));
        fails = shuffle_chain_row(tab_cur, tab_prev, tg, cur, prev, negx, shat, sprime, that);
      }
      const u32 word = shuffle_row_word(D.rowbad[row] != 0, ok_cur, shat, sprime, fails);
      if (D.rows) D.rows[row] = word;
      if (word & SHUF_ROW_BAD) { atomicAdd(D.found, 1u); atomicMin(D.found + 2, (u32)row); }
      if (word & SHUF_ROW_CHAIN) { atomicAdd(D.found + 1, 1u); atomicMin(D.found + 3, (u32)row); }
    }
  }
}

__global__ void __launch_bounds__(64) k_shuffle_close(ShufDev D, const u32* out_big, const unsigned char* ok_big, const u32* out_small, const unsigned char* ok_small,
                                u32* verdict) {
  if (blockIdx.x || threadIdx.x) return;
  *verdict = shuffle_close_lane(D.proof, out_big, ok_big, out_small, ok_small, D.found, D.state[SHUF_ST_HEADBAD]);
}
#endif  // __HIPCC__

}  // namespace eg
