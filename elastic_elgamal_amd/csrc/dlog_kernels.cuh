// dlog_kernels.cuh -- bounded discrete logarithms by baby-step/giant-step (eg_dlog_solver_*, eg_hip.hip): the count m behind a
// decrypted element [m]G, for intervals that no table of [v]G can hold (DiscreteLogTable, src/encryption.rs:260-298, makes one entry
// per admissible value).
//
// Torsion-free key.  A decoded Ristretto element is P = [m]B + T with T in E[4]; two doublings give Q = [4m]B in the prime-order
// subgroup, where a point has ONE pair of affine coordinates.  The key of a point is taken from its canonical affine y, so no
// inverse square root (an encoding) is paid per step; every point that is walked is a multiple of [4]B.
//   baby table:  for i in [0, W), W = 2^baby_bits: (tag of y([4i]B), i) in an open-addressing table of 8-byte slots in HBM
//                (2 W slots: load 0.5; linear probing; slot = tag << 32 | (i + 1), 0 = empty).
//   giant step:  S_j = Q - [4 (lo + j W)]B; if y(S_j) is the key of entry i then m = lo + j W + i is a CANDIDATE.
// y is the same for S and -S, and a tag is shorter than y, so a candidate may be false: the host confirms every candidate with
// [m]G encoded and compared with the element's bytes, and a false candidate ends nothing - the lane goes on probing and walking.
// (S_j = -[4i]B means m = lo + j W - i, which step j - 1 reports as lo + (j - 1) W + (W - i) when it is in range: nothing is lost
// by reporting the '+' reading only.)  The unified addition is complete on this curve, so Z is never 0 and the identity
// (m = lo + j W, entry 0) needs no special case.
//
// Both walks are runs of DLOG_RUN consecutive points per lane, as k_build_fixed_table's: start from the G comb, ge_madd by a constant
// affine-Niels point, running product of the Z's into scratch, ONE inversion per run, then per point 1/Z, y = Y/Z, the key and the
// insertion / probe.  Per giant step: 11 multiplications for the addition, 4 for the batched inversion, 1/64 of an inversion.
// Limb classes: every coordinate that is stored or multiplied is the output of a multiplication (class 1); the host check build
// (tests/hostcheck/dlogcheck.cpp, -DEG_BOUNDCHECK) runs these same lane functions and asserts it over whole runs.
//
// The lane functions are templates over their memory (table, run scratch, candidate list) so that the host check runs them on arrays;
// the tag width is a template parameter too: the product uses 32 bits, the host check 4, where false candidates are certain.
#pragma once
#include "ge25519.cuh"
#include "sc25519.cuh"
#include "dlog_host.hpp"

namespace eg {

constexpr int DLOG_RUN = egdlog::RUN;
constexpr u32 DLOG_MAX_PROBE = 1024;      // longest probe sequence an insertion may need (checked: the build fails beyond it)
constexpr int DLOG_TAG_BITS = 32;
constexpr int DLOG_RUN_WORDS = 3 * EG_NL; // Y, Z and the product of the Z's before the point

// 4 (lo + off) as a scalar: < 2^67, no wrap at lo + off >= 2^64
EG_HD void dlog_scalar4(u32 k[8], u64 lo, u64 off) {
  const u64 s = lo + off;
  const u32 c = s < lo ? 1u : 0u;
  k[0] = (u32)s << 2;
  k[1] = (u32)(s >> 30);
  k[2] = (u32)(s >> 62) | (c << 2);
#pragma unroll
  for (int i = 3; i < 8; ++i) k[i] = 0;
}

template <int TAG_BITS>
EG_HD void dlog_key(u32& pos, u32& tag, const fe& y, u32 slot_mask) {
  static_assert(TAG_BITS >= 1 && TAG_BITS <= 32, "a tag is 1..32 bits");
  u32 w[8];
  fe_to_words(w, y);
  pos = w[0] & slot_mask;
  tag = TAG_BITS == 32 ? w[1] : (w[1] & ((1u << (TAG_BITS & 31)) - 1u));
}

template <int TAG_BITS, class Slots>
EG_HD void dlog_insert(Slots& slots, const fe& y, u32 idx, u32 slot_mask, u32 max_probe) {
  u32 pos, tag;
  dlog_key<TAG_BITS>(pos, tag, y, slot_mask);
  const u64 v = ((u64)tag << 32) | (u64)(idx + 1u);
  for (u32 t = 0; t < max_probe; ++t) {
    if (slots.cas(pos, v) == 0) return;
    pos = (pos + 1u) & slot_mask;
  }
  slots.overflow();
}

// the rest of a probe sequence whose first slot `v` was read ahead: every slot up to the first empty one whose tag matches is a candidate
template <int TAG_BITS, class Slots, class Sink>
EG_HD void dlog_probe(const Slots& slots, u64 v, u32 pos, u32 tag, u32 elem, u64 lo, u64 span, u64 j, int baby_bits, u32 slot_mask,
                      u32 max_probe, Sink& sink) {
  for (u32 t = 0; v != 0 && t < max_probe; ++t) {
    if ((u32)(v >> 32) == tag) {
      u64 m;
      if (egdlog::candidate_value(lo, span, j, (u32)v - 1u, baby_bits, &m)) sink.push(elem, m);
    }
    pos = (pos + 1u) & slot_mask;
    v = slots.get(pos);
  }
}

// forward half of a run: `steps` points q, q + step, .. with (Y, Z, product of the earlier Z's) parked in io; returns the product of all Z's
template <class RunIO>
EG_HD void dlog_run_forward(fe& prod, ge& q, const ge_niels& step, int steps, RunIO& io) {
  fe_1(prod);
#pragma unroll 1
  for (int i = 0; i < steps; ++i) {
    io.store(i, q.Y, q.Z, prod);
    fe_mul(prod, prod, q.Z);
    if (i + 1 < steps) { ge_p1p1 t; ge_madd(t, q, step); ge_add_to_p3(q, t); }
  }
}
// backward half, point i: y = Y_i / Z_i; inv = 1 / (Z_0 .. Z_i) on entry, 1 / (Z_0 .. Z_(i-1)) on return
template <class RunIO>
EG_HD void dlog_run_affine_y(fe& y, fe& inv, int i, const RunIO& io) {
  fe Y, Z, pre, zi;
  io.load(i, Y, Z, pre);
  fe_mul(zi, inv, pre);
  fe_mul(inv, inv, Z);
  fe_mul(y, Y, zi);
}

// one lane of the table build: entries [run * DLOG_RUN, (run + 1) * DLOG_RUN) of the baby table; step = niels([4]B)
template <int TAG_BITS, class NielsIO, class RunIO, class Slots>
EG_HD void dlog_baby_lane(u32 run, u32 n_entries, NielsIO& tg, const ge_niels& step, RunIO& io, Slots& slots, u32 slot_mask, u32 max_probe) {
  const u32 i0 = run * (u32)DLOG_RUN;
  u32 k[8], dg[EG_COMB_WORDS];
  dlog_scalar4(k, 0, i0);
  sc_recode_comb(dg, k);
  ge q; ge_identity(q);
  ge_fixed_mul_add(q, tg, dg);
  fe prod, inv;
  dlog_run_forward(prod, q, step, DLOG_RUN, io);
  fe_invert(inv, prod);
#pragma unroll 1
  for (int i = DLOG_RUN - 1; i >= 0; --i) {
    fe y;
    dlog_run_affine_y(y, inv, i, io);
    if (i0 + (u32)i < n_entries) {
      slots.note(i0 + (u32)i, y);
      dlog_insert<TAG_BITS>(slots, y, i0 + (u32)i, slot_mask, max_probe);
    }
  }
}

// one lane of the search: giant steps [j0, j0 + steps) of element `elem`, steps <= DLOG_RUN; p = the decoded element (any representative
// of its coset), gstep = niels(-[4 W]B).  The first slot of a probe is read one step ahead of its use.
template <int TAG_BITS, class NielsIO, class RunIO, class Slots, class Sink>
EG_HD void dlog_giant_lane(u32 elem, const ge& p, u64 lo, u64 span, u64 j0, int steps, int baby_bits, NielsIO& tg, const ge_niels& gstep,
                           RunIO& io, const Slots& slots, u32 slot_mask, u32 max_probe, Sink& sink) {
  u32 k[8], nk[8], dg[EG_COMB_WORDS];
  dlog_scalar4(k, lo, j0 << baby_bits);
  sc_neg(nk, k);                                  // l - 4 (lo + j0 W): canonical
  sc_recode_comb(dg, nk);
  ge q, d;
  ge_dbl_full(d, p);
  ge_dbl_full(q, d);                              // Q = [4]P
  ge_fixed_mul_add(q, tg, dg);
  fe prod, inv;
  dlog_run_forward(prod, q, gstep, steps, io);
  fe_invert(inv, prod);
  u64 ahead_v = 0, ahead_j = 0;
  u32 ahead_pos = 0, ahead_tag = 0;
  bool ahead = false;
#pragma unroll 1
  for (int i = steps - 1; i >= 0; --i) {
    fe y;
    dlog_run_affine_y(y, inv, i, io);
    u32 pos, tag;
    dlog_key<TAG_BITS>(pos, tag, y, slot_mask);
    const u64 v = slots.get(pos);
    if (ahead) dlog_probe<TAG_BITS>(slots, ahead_v, ahead_pos, ahead_tag, elem, lo, span, ahead_j, baby_bits, slot_mask, max_probe, sink);
    ahead = true; ahead_v = v; ahead_pos = pos; ahead_tag = tag; ahead_j = j0 + (u64)i;
  }
  if (ahead) dlog_probe<TAG_BITS>(slots, ahead_v, ahead_pos, ahead_tag, elem, lo, span, ahead_j, baby_bits, slot_mask, max_probe, sink);
}

}  // namespace eg

#if defined(__HIPCC__)
#include "kernels.cuh"       // FixedTable (device_io.cuh), prepared_load

namespace eg {

// run scratch, word-interleaved across the lanes of a launch: [point][word][lane]
struct DlogRunDev {
  u32* base;         // scratch + lane
  size_t stride;     // lanes the scratch is laid out for
  __device__ __forceinline__ void store(int i, const fe& Y, const fe& Z, const fe& pre) {
    u32* p = base + (size_t)i * DLOG_RUN_WORDS * stride;
#pragma unroll
    for (int j = 0; j < EG_NL; ++j) { p[(size_t)j * stride] = Y.v[j]; p[(size_t)(EG_NL + j) * stride] = Z.v[j]; p[(size_t)(2 * EG_NL + j) * stride] = pre.v[j]; }
  }
  __device__ __forceinline__ void load(int i, fe& Y, fe& Z, fe& pre) const {
    const u32* p = base + (size_t)i * DLOG_RUN_WORDS * stride;
#pragma unroll
    for (int j = 0; j < EG_NL; ++j) { Y.v[j] = p[(size_t)j * stride]; Z.v[j] = p[(size_t)(EG_NL + j) * stride]; pre.v[j] = p[(size_t)(2 * EG_NL + j) * stride]; }
  }
};
struct DlogSlotsDev {
  unsigned long long* tab;
  u32* overflowed;
  __device__ __forceinline__ u64 cas(u32 pos, u64 v) { return (u64)atomicCAS(tab + pos, 0ull, (unsigned long long)v); }
  __device__ __forceinline__ u64 get(u32 pos) const { return (u64)tab[pos]; }
  __device__ __forceinline__ void note(u32, const fe&) {}
  __device__ __forceinline__ void overflow() { atomicAdd(overflowed, 1u); }
};
struct DlogSinkDev {
  u32* count;
  u32 cap;
  unsigned long long* list;      // [cap][2]: element, value
  __device__ __forceinline__ void push(u32 elem, u64 m) {
    const u32 at = atomicAdd(count, 1u);
    if (at < cap) { list[2 * (size_t)at] = elem; list[2 * (size_t)at + 1] = m; }
  }
};
__device__ __forceinline__ void dlog_load_niels(ge_niels& n, const u32* w /* 3 * EG_NL */) {
#pragma unroll
  for (int j = 0; j < EG_NL; ++j) { n.ypx.v[j] = w[j]; n.ymx.v[j] = w[EG_NL + j]; n.xy2d.v[j] = w[2 * EG_NL + j]; }
}

// lanes [0, n_runs): runs run0 .. of the baby table.  consts = niels([4]B), niels(-[4 W]B) as limbs (made on the host at creation).
__global__ void __launch_bounds__(NT, 2) k_dlog_baby(u32 run0, u32 n_runs, u32 n_entries, const uint4* tabG, const u32* consts, u32* scratch,
                                                      size_t stride, unsigned long long* slots, u32 slot_mask, u32 max_probe, u32* overflowed) {
  const size_t lane = (size_t)blockIdx.x * NT + threadIdx.x;
  if (lane >= n_runs || lane >= stride) return;
  ge_niels step; dlog_load_niels(step, consts);
  const FixedTable tg(tabG);
  DlogRunDev io{scratch + lane, stride};
  DlogSlotsDev sl{slots, overflowed};
  dlog_baby_lane<DLOG_TAG_BITS>(run0 + (u32)lane, n_entries, tg, step, io, sl, slot_mask, max_probe);
}

// lanes [0, n_elems * n_runs): lane = e * n_runs + r walks giant steps [(run0 + r) DLOG_RUN, ..) of element elem0 + e (prepared: the
// decoded elements of this block as k_prim_points_prepare leaves them; done[e] != 0: answered, undecodable or the identity - skipped)
__global__ void __launch_bounds__(NT, 2) k_dlog_giant(u32 elem0, u32 n_elems, const u32* prepared, const unsigned char* done, u64 lo, u64 span,
                                                       u64 run0, u32 n_runs, u64 total_steps, int baby_bits, const uint4* tabG, const u32* consts,
                                                       u32* scratch, size_t stride, const unsigned long long* slots, u32 slot_mask, u32 max_probe,
                                                       u32* count, u32 cap, unsigned long long* list) {
  const size_t lane = (size_t)blockIdx.x * NT + threadIdx.x;
  if (lane >= (size_t)n_elems * n_runs || lane >= stride) return;
  const u32 e = (u32)(lane / n_runs);
  const u64 j0 = (run0 + (u64)(lane % n_runs)) * (u64)DLOG_RUN;
  if (done[e] || j0 >= total_steps) return;
  const int steps = (int)(total_steps - j0 < (u64)DLOG_RUN ? total_steps - j0 : (u64)DLOG_RUN);
  ge p; prepared_load(p, prepared + (size_t)e * PREP_WORDS);
  ge_niels gstep; dlog_load_niels(gstep, consts + DLOG_RUN_WORDS);
  const FixedTable tg(tabG);
  DlogRunDev io{scratch + lane, stride};
  const DlogSlotsDev sl{const_cast<unsigned long long*>(slots), nullptr};
  DlogSinkDev sink{count, cap, list};
  dlog_giant_lane<DLOG_TAG_BITS>(elem0 + e, p, lo, span, j0, steps, baby_bits, tg, gstep, io, sl, slot_mask, max_probe, sink);
}

}  // namespace eg
#endif
