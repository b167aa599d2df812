// limb_ops.cuh -- TEST-ONLY: every field / point / scalar operation of fe25519.cuh, ge25519.cuh and sc25519.cuh behind one
// raw-limb calling convention, shared by the host bound-check build (tests/hostcheck/hostcheck.cpp: hc_limb_ops) and the
// device build (tests/devcheck/devcheck.hip: dc_limb_ops), so that both compilations of the headers run the same calls on the
// same records (tests/limb_cases.py makes the records and holds the reference).  Never part of the product.
//
// One case = LIMB_WORDS input words, LIMB_SLOTS classes, LIMB_WORDS output words.  A field element occupies a slot of 9 words
// (slot s = words 9 s .. 9 s + 8); words 72..79 are extra (flags and counts in, canonical words out).  The class of every input
// element is passed in: the bound-check build asserts it against the limbs (fe_check_values) and carries it through the
// operation, so a case outside a precondition aborts instead of running.  The device build ignores the classes.
#pragma once
#include "../../elastic_elgamal_amd/csrc/ge25519.cuh"
#include "../../elastic_elgamal_amd/csrc/sc25519.cuh"

#define LIMB_SLOTS 8
#define LIMB_WORDS 80
#define LIMB_EXTRA 72

namespace eg {

enum LimbOp {
  // field: f = slot 0, g = slot 1 -> h = slot 0, h aliasing f = slot 1, h aliasing g = slot 2, canonical words of h = extra
  LOP_MUL = 0, LOP_SQ, LOP_SQN /* extra[0] = n */, LOP_ADD, LOP_SUB, LOP_SUB4, LOP_NEG, LOP_CARRY,
  // canonical form: f = slot 0, g = slot 1 -> word 0 isnegative(f), 1 iszero(f), 2 eq(f, g), 3 eq(g, f); extra = to_words(f);
  // with extra[0] != 0 (class-1 f) also words 9..16 = pack8(f) and slot 2 = unpack8 of them
  LOP_CANON = 8,
  LOP_FROM_WORDS,            // words 0..7 -> slot 0 = fe_from_words, extra = its canonical words
  // chains: slot 0 -> slot 0, extra = canonical words
  LOP_INVERT = 10, LOP_POW22523,
  LOP_SQRT_RATIO,            // u = slot 0, v = slot 1 -> slot 0 = r, word 9 = was_square, extra = canonical words of r
  // completed -> extended: p1p1 (X, Y, Z, T) = slots 0..3 -> slots 0..3 (0..2 for p2)
  LOP_ADD_TO_P3 = 13, LOP_ADD_TO_P2, LOP_DBL_TO_P3, LOP_DBL_TO_P2,
  // point formulas: p (X, Y, Z, T) = slots 0..3, addend = slots 4..; extra[0]: 0 = addend as it is, 1 = cneg(false), 2 = cneg(true)
  // -> p1p1 = slots 0..3, its _to_p3 conversion = slots 4..7
  LOP_GE_ADD = 17, LOP_GE_MADD,
  LOP_GE_DBL,                // X, Y, Z = slots 0..2 -> p1p1 = slots 0..3, ge_dbl_to_p3 = slots 4..7
  LOP_TO_CACHED, LOP_TO_CACHED_LAZY,          // p = slots 0..3 -> (YpX, YmX, Z2, T2d) = slots 0..3
  LOP_CACHED_CNEG, LOP_NIELS_CNEG,            // entry = slots 0..3 / 0..2, extra[0] = flag -> the same slots
  // scalars: a = words 0..7, b = 9..16, c = 18..25 (wide input: words 0..15) -> words 0..7 (flag: word 0)
  LOP_SC_MULADD = 24, LOP_SC_MUL, LOP_SC_ADD, LOP_SC_FROM_WIDE, LOP_SC_IS_CANONICAL, LOP_SC_NEG, LOP_SC_HALVE,
  LOP_COUNT
};

EG_HD void lo_load(fe& f, const u32* in, const float* cls, int slot) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) f.v[i] = in[EG_NL * slot + i];
  (void)cls;
  EG_SETCLS(f, cls[slot]);
  fe_check_values(f);
}
EG_HD void lo_store(u32* out, int slot, const fe& f) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) out[EG_NL * slot + i] = f.v[i];
}
EG_HD void lo_store_words(u32* out, const fe& f) {
  u32 w[8]; fe_to_words(w, f);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[LIMB_EXTRA + i] = w[i];
}

EG_HD void limb_field_op(int op, const u32* in, const float* cls, u32* out) {
  fe f, g, h, a, b;
  lo_load(f, in, cls, 0); lo_load(g, in, cls, 1);
  a = f; b = g; h = f;
  switch (op) {
    case LOP_MUL: fe_mul(h, f, g); fe_mul(a, a, g); fe_mul(b, f, b); break;
    case LOP_SQ: fe_sq(h, f); fe_sq(a, a); b = h; break;
    case LOP_SQN: fe_sqn(h, f, (int)in[LIMB_EXTRA]); fe_sqn(a, a, (int)in[LIMB_EXTRA]); b = h; break;
    case LOP_ADD: fe_add(h, f, g); fe_add(a, a, g); fe_add(b, f, b); break;
    case LOP_SUB: fe_sub(h, f, g); fe_sub(a, a, g); fe_sub(b, f, b); break;
    case LOP_SUB4: fe_sub4(h, f, g); fe_sub4(a, a, g); fe_sub4(b, f, b); break;
    case LOP_NEG: fe_neg(h, f); fe_neg(a, a); b = h; break;
    default: fe_carry(h); a = h; b = h; break;          // LOP_CARRY
  }
  lo_store(out, 0, h); lo_store(out, 1, a); lo_store(out, 2, b);
  lo_store_words(out, h);
}

EG_HD void limb_canon_op(int op, const u32* in, const float* cls, u32* out) {
  if (op == LOP_FROM_WORDS) {
    u32 w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = in[i];
    fe h; fe_from_words(h, w);
    lo_store(out, 0, h);
    lo_store_words(out, h);
    return;
  }
  fe f, g;
  lo_load(f, in, cls, 0); lo_load(g, in, cls, 1);
  out[0] = fe_isnegative(f) ? 1u : 0u;
  out[1] = fe_iszero(f) ? 1u : 0u;
  out[2] = fe_eq(f, g) ? 1u : 0u;
  out[3] = fe_eq(g, f) ? 1u : 0u;
  lo_store_words(out, f);
  if (in[LIMB_EXTRA] != 0) {
    u32 w[8]; fe_pack8(w, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[EG_NL + i] = w[i];
    fe u; fe_unpack8(u, w);
    lo_store(out, 2, u);
  }
}

EG_HD void limb_chain_op(int op, const u32* in, const float* cls, u32* out) {
  fe f, g, h;
  lo_load(f, in, cls, 0); lo_load(g, in, cls, 1);
  if (op == LOP_INVERT) fe_invert(h, f);
  else if (op == LOP_POW22523) fe_pow22523(h, f);
  else out[EG_NL] = fe_sqrt_ratio_m1(h, f, g) ? 1u : 0u;
  lo_store(out, 0, h);
  lo_store_words(out, h);
}

EG_HD void limb_p1p1_op(int op, const u32* in, const float* cls, u32* out) {
  ge_p1p1 p;
  lo_load(p.X, in, cls, 0); lo_load(p.Y, in, cls, 1); lo_load(p.Z, in, cls, 2); lo_load(p.T, in, cls, 3);
  if (op == LOP_ADD_TO_P3 || op == LOP_DBL_TO_P3) {
    ge r;
    if (op == LOP_ADD_TO_P3) ge_add_to_p3(r, p); else ge_dbl_to_p3(r, p);
    lo_store(out, 0, r.X); lo_store(out, 1, r.Y); lo_store(out, 2, r.Z); lo_store(out, 3, r.T);
  } else {
    ge_p2 r;
    if (op == LOP_ADD_TO_P2) ge_add_to_p2(r, p); else ge_dbl_to_p2(r, p);
    lo_store(out, 0, r.X); lo_store(out, 1, r.Y); lo_store(out, 2, r.Z);
  }
}

EG_HD void limb_point_op(int op, const u32* in, const float* cls, u32* out) {
  ge p;
  lo_load(p.X, in, cls, 0); lo_load(p.Y, in, cls, 1); lo_load(p.Z, in, cls, 2); lo_load(p.T, in, cls, 3);
  const u32 flag = in[LIMB_EXTRA];
  if (op == LOP_GE_ADD || op == LOP_GE_MADD || op == LOP_GE_DBL) {
    ge_p1p1 t; ge r;
    if (op == LOP_GE_ADD) {
      ge_cached q;
      lo_load(q.YpX, in, cls, 4); lo_load(q.YmX, in, cls, 5); lo_load(q.Z2, in, cls, 6); lo_load(q.T2d, in, cls, 7);
      if (flag != 0) ge_cached_cneg(q, flag == 2);
      ge_add(t, p, q);
      ge_add_to_p3(r, t);
    } else if (op == LOP_GE_MADD) {
      ge_niels q;
      lo_load(q.ypx, in, cls, 4); lo_load(q.ymx, in, cls, 5); lo_load(q.xy2d, in, cls, 6);
      if (flag != 0) ge_niels_cneg(q, flag == 2);
      ge_madd(t, p, q);
      ge_add_to_p3(r, t);
    } else {
      ge_dbl(t, p.X, p.Y, p.Z);
      ge_dbl_to_p3(r, t);
    }
    lo_store(out, 0, t.X); lo_store(out, 1, t.Y); lo_store(out, 2, t.Z); lo_store(out, 3, t.T);
    lo_store(out, 4, r.X); lo_store(out, 5, r.Y); lo_store(out, 6, r.Z); lo_store(out, 7, r.T);
  } else if (op == LOP_TO_CACHED || op == LOP_TO_CACHED_LAZY) {
    ge_cached c;
    if (op == LOP_TO_CACHED) ge_to_cached(c, p); else ge_to_cached_lazy(c, p);
    lo_store(out, 0, c.YpX); lo_store(out, 1, c.YmX); lo_store(out, 2, c.Z2); lo_store(out, 3, c.T2d);
  } else if (op == LOP_CACHED_CNEG) {
    ge_cached c; c.YpX = p.X; c.YmX = p.Y; c.Z2 = p.Z; c.T2d = p.T;
    ge_cached_cneg(c, flag != 0);
    lo_store(out, 0, c.YpX); lo_store(out, 1, c.YmX); lo_store(out, 2, c.Z2); lo_store(out, 3, c.T2d);
  } else {                                              // LOP_NIELS_CNEG
    ge_niels c; c.ypx = p.X; c.ymx = p.Y; c.xy2d = p.Z;
    ge_niels_cneg(c, flag != 0);
    lo_store(out, 0, c.ypx); lo_store(out, 1, c.ymx); lo_store(out, 2, c.xy2d);
  }
}

EG_HD void limb_scalar_op(int op, const u32* in, u32* out) {
  u32 a[16], b[8], c[8], o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = in[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) { b[i] = in[9 + i]; c[i] = in[18 + i]; }
  switch (op) {
    case LOP_SC_MULADD: sc_muladd(o, a, b, c); break;
    case LOP_SC_MUL: sc_mul(o, a, b); break;
    case LOP_SC_ADD: sc_add(o, a, b); break;
    case LOP_SC_FROM_WIDE: sc_from_wide(o, a); break;
    case LOP_SC_IS_CANONICAL: o[0] = sc_is_canonical(a) ? 1u : 0u; break;
    case LOP_SC_NEG: sc_neg(o, a); break;
    default: sc_halve(o, a); break;                     // LOP_SC_HALVE
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = o[i];
}

// group of an operation: one kernel (device) / one branch (host) per group
EG_HD int limb_op_group(int op) {
  return op < LOP_CANON ? 0 : op < LOP_INVERT ? 1 : op < LOP_ADD_TO_P3 ? 2 : op < LOP_GE_ADD ? 3 : op < LOP_SC_MULADD ? 4 : 5;
}

}  // namespace eg
