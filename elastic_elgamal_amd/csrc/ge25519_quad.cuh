// ge25519_quad.cuh -- quad-lane point arithmetic: FOUR adjacent lanes hold one point and cooperate on every point operation.
//
// The extended-coordinate formulas of ge25519.cuh have four-way parallelism that one lane cannot use: a doubling is four independent
// products followed by four more, an addition the same.  Here lane r (0..3) of a quad holds coordinate r of (X, Y, Z, T) and computes ONE
// fe_mul of each half-step with the unchanged 9-limb routine of fe25519.cuh; between the half-steps the lanes exchange operands with
// DPP quad permutes (full-rate VALU, no LDS).  A doubling then has the latency of two multiplications instead of 4 S + 4 M, an
// addition two instead of eight.  Used by the small-batch verifier (latency_kernels.cuh), where a ballot offers a dozen equations
// to a 256-CU chip and the dependent chain of each is what the caller waits for.
//
// Layout of a quad:            lane 0   lane 1   lane 2   lane 3
//   point  (qpoint)            X        Y        Z        T          all [1] (products); the doubling accepts up to [3]
//   addend (qcached)           Y+X      Y-X      2dT      2Z         all <= [3]  (NOTE lanes 2 / 3: T2d before Z2, the order the
//                                                                     first half-step of the addition wants them in)
// Half-step products:          doubling  X*X      Y*Y      Z*Z      X*Y       (lane 3 multiplies instead of squaring X+Y: the lanes run
//                                                                              in lockstep, so a squaring would save nothing, and
//                                                                              E = 2XY comes out [2] instead of [5])
//                              addition  (Y+X)*q0 (Y-X)*q1 T*q2     Z*q3
//                              finish    E*F      G*H      G*F      E*H       (both operations; E H G F as in ge25519.cuh)
// Limb classes ([n] of fe25519.cuh) of every intermediate, worst case over the lanes (the bound-check host build sees a select as the
// larger class of its two sides):
//   doubling   operands [<=3] x [<=3] = 9 <= 12.5;  E = 2XY [2], H = YY+XX [2], G = YY-XX [3], F = 2ZZ-G [6] carried to [1];
//              finish a = E|G [3], b = F|H [2]: 6.
//   addition   a = Y+X [2] | Y-X [3] | T | Z [1] times the addend [<=3]: 9;  E = PP-MM [3], H = PP+MM [2], G = D+TT [2], F = D-TT [3];
//              finish a = E|G [3], b = F|H [3]: 9.  The point must be [1] (fe_sub wants a class-1 subtrahend): every quad
//              operation returns products, so a chain of them stays inside the preconditions without a single carry.
//
// The exchange is behind a small policy (class Q): QuadDev is the device form (a value per lane, DPP); QuadHost emulates a quad as an
// array of four lanes so that the bound-check build (tests/hostcheck/quadcheck.cpp, -DEG_BOUNDCHECK under UBSan) compiles the SAME
// operations.  An operation is written as  q.perm / q.gather  (exchanges) and  q.each([&](int r) { .. })  (the per-lane code).
#pragma once
#include "ge25519.cuh"

namespace eg {

struct fe4 { fe v[4]; };

// ---- the two quad policies -------------------------------------------------------------------------------------------------------
struct QuadHost {
  template <class V> struct var { V v[4]; V& at(int r) { return v[r]; } const V& at(int r) const { return v[r]; } };
  template <class F> void each(F f) { for (int r = 0; r < 4; ++r) f(r); }
  // out(lane r) = in(lane P_r)
  template <int P0, int P1, int P2, int P3> void perm(var<fe>& out, const var<fe>& in) {
    const int p[4] = {P0, P1, P2, P3};
    var<fe> t = in;
    for (int r = 0; r < 4; ++r) out.v[r] = t.v[p[r]];
  }
  // every lane receives all four values
  void gather(var<fe4>& out, const var<fe>& in) {
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) out.v[r].v[k] = in.v[k];
  }
};

#if defined(__HIPCC__)
struct QuadDev {
  template <class V> struct var { V v; __device__ __forceinline__ V& at(int) { return v; } __device__ __forceinline__ const V& at(int) const { return v; } };
  int r;                       // lane within the quad
  __device__ __forceinline__ explicit QuadDev(int lane) : r(lane & 3) {}
  template <class F> __device__ __forceinline__ void each(F f) { f(r); }
  template <int CTRL> static __device__ __forceinline__ u32 dpp(u32 x) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);      // v_mov_b32_dpp quad_perm:[..]
  }
  template <int P0, int P1, int P2, int P3> __device__ __forceinline__ void perm(var<fe>& out, const var<fe>& in) {
#pragma unroll
    for (int i = 0; i < EG_NL; ++i) out.v.v[i] = dpp<P0 | (P1 << 2) | (P2 << 4) | (P3 << 6)>(in.v.v[i]);
  }
  __device__ __forceinline__ void gather(var<fe4>& out, const var<fe>& in) {
#pragma unroll
    for (int i = 0; i < EG_NL; ++i) {
      out.v.v[0].v[i] = dpp<0x00>(in.v.v[i]);
      out.v.v[1].v[i] = dpp<0x55>(in.v.v[i]);
      out.v.v[2].v[i] = dpp<0xaa>(in.v.v[i]);
      out.v.v[3].v[i] = dpp<0xff>(in.v.v[i]);
    }
  }
};
#endif

template <class Q> using qfe = typename Q::template var<fe>;

// ---- constants and trivial operations --------------------------------------------------------------------------------------------
template <class Q> EG_HD void quad_identity(Q& q, qfe<Q>& c) {                 // (0 : 1 : 1 : 0)
  q.each([&](int r) { fe one; fe_1(one); fe_0(c.at(r)); fe_cmov(c.at(r), one, r == 1 || r == 2); });
}
template <class Q> EG_HD void quad_cached_identity(Q& q, qfe<Q>& c) {          // (1, 1, 0, 2): the neutral addend, also of the Niels form
  q.each([&](int r) { fe one, two; fe_1(one); fe_0(two); two.v[0] = 2; fe_0(c.at(r)); fe_cmov(c.at(r), one, r < 2); fe_cmov(c.at(r), two, r == 3); });
}
// c = flag ? d : c, the flag being the same in the four lanes
template <class Q> EG_HD void quad_select(Q& q, qfe<Q>& c, const qfe<Q>& d, bool flag) {
  q.each([&](int r) { fe_cmov(c.at(r), d.at(r), flag); });
}
// split a one-lane value over the quad and back (the host form copies; the device form keeps what its lane is for)
template <class Q> EG_HD void quad_from_ge(Q& q, qfe<Q>& c, const ge& p) {
  q.each([&](int r) { c.at(r) = p.X; fe_cmov(c.at(r), p.Y, r == 1); fe_cmov(c.at(r), p.Z, r == 2); fe_cmov(c.at(r), p.T, r == 3); });
}
template <class Q> EG_HD void quad_from_cached(Q& q, qfe<Q>& c, const ge_cached& p) {
  q.each([&](int r) { c.at(r) = p.YpX; fe_cmov(c.at(r), p.YmX, r == 1); fe_cmov(c.at(r), p.T2d, r == 2); fe_cmov(c.at(r), p.Z2, r == 3); });
}
// negation of a point: (-X, Y, Z, -T), carried back to [1]
template <class Q> EG_HD void quad_neg(Q& q, qfe<Q>& c, bool neg) {
  q.each([&](int r) { fe n; fe_neg(n, c.at(r)); fe_carry(n); fe_cmov(c.at(r), n, neg && (r == 0 || r == 3)); });
}
// conditional negation of an addend: Y+X and Y-X change places, 2dT changes sign ([1] -> [3])
template <class Q> EG_HD void quad_cached_cneg(Q& q, qfe<Q>& c, bool neg) {
  qfe<Q> sw;
  q.template perm<1, 0, 2, 3>(sw, c);
  q.each([&](int r) { fe n; fe_neg(n, c.at(r)); fe_cmov(c.at(r), sw.at(r), neg && r < 2); fe_cmov(c.at(r), n, neg && r == 2); });
}
// the same for an addend that a table load has already swapped (QuadTable::load(.., neg)): only the sign of 2dT is left
template <class Q> EG_HD void quad_cached_neg_t(Q& q, qfe<Q>& c, bool neg) {
  q.each([&](int r) { fe n; fe_neg(n, c.at(r)); fe_cmov(c.at(r), n, neg && r == 2); });
}

// ---- the second half-step of both operations: (X, Y, Z, T) = (E F, G H, G F, E H) -----------------------------------------------
template <class Q> EG_HD void quad_finish_lane(fe& out, int r, const fe& E, const fe& H, const fe& G, const fe& F) {
  fe a = G, b = H;
  fe_cmov(a, E, r == 0 || r == 3);
  fe_cmov(b, F, r == 0 || r == 2);
  fe_mul(out, a, b);
}

// c = 2 c.  Needs X, Y, Z of class <= 3 (lane 3 is not read); returns all four coordinates [1].
template <class Q> EG_HD void quad_dbl(Q& q, qfe<Q>& c) {
  qfe<Q> a, b, s;
  q.template perm<0, 1, 2, 0>(a, c);
  q.template perm<0, 1, 2, 1>(b, c);
  q.each([&](int r) { fe_mul(s.at(r), a.at(r), b.at(r)); });          // XX YY ZZ XY
  typename Q::template var<fe4> g;
  q.gather(g, s);
  q.each([&](int r) {
    const fe4& v = g.at(r);
    fe E, H, G, F, zz2;
    fe_add(E, v.v[3], v.v[3]);        // 2XY [2]
    fe_add(H, v.v[1], v.v[0]);        // [2]
    fe_sub(G, v.v[1], v.v[0]);        // [3]
    fe_add(zz2, v.v[2], v.v[2]);      // [2]
    fe_sub4(F, zz2, G);               // [6]
    fe_carry(F);                      // [1]
    quad_finish_lane<Q>(c.at(r), r, E, H, G, F);
  });
}

// c = c + d, d an addend (qcached layout, classes <= 3); c must be [1]; returns [1]
template <class Q> EG_HD void quad_add(Q& q, qfe<Q>& c, const qfe<Q>& d) {
  qfe<Q> u, s;
  q.template perm<1, 0, 3, 2>(u, c);                                    // Y X T Z
  q.each([&](int r) {
    fe sum, dif, a = u.at(r);                                           // lanes 2, 3: T, Z
    fe_add(sum, u.at(r), c.at(r));                                      // lane 0: Y + X [2]
    fe_sub(dif, c.at(r), u.at(r));                                      // lane 1: Y - X [3]
    fe_cmov(a, sum, r == 0);
    fe_cmov(a, dif, r == 1);
    fe_mul(s.at(r), a, d.at(r));                                        // PP MM TT D
  });
  typename Q::template var<fe4> g;
  q.gather(g, s);
  q.each([&](int r) {
    const fe4& v = g.at(r);
    fe E, H, G, F;
    fe_sub(E, v.v[0], v.v[1]);        // [3]
    fe_add(H, v.v[0], v.v[1]);        // [2]
    fe_add(G, v.v[3], v.v[2]);        // [2]
    fe_sub(F, v.v[3], v.v[2]);        // [3]
    quad_finish_lane<Q>(c.at(r), r, E, H, G, F);
  });
}

// d = the addend form of the point c ([1]): (Y+X, Y-X, 2dT, 2Z), every lane through ONE multiplication (by 1, 1, 2d, 2), so that the
// result is [1] in every lane and packs into a table entry as it is
template <class Q> EG_HD void quad_to_cached(Q& q, qfe<Q>& d, const qfe<Q>& c) {
  qfe<Q> u;
  q.template perm<1, 0, 3, 2>(u, c);
  q.each([&](int r) {
    const fe d2 = EG_FE_2D;
    fe sum, dif, a = u.at(r), k;
    fe_add(sum, u.at(r), c.at(r));
    fe_sub(dif, c.at(r), u.at(r));
    fe_cmov(a, sum, r == 0);
    fe_cmov(a, dif, r == 1);
    fe_1(k);
    fe two; fe_0(two); two.v[0] = 2;
    fe_cmov(k, d2, r == 2);
    fe_cmov(k, two, r == 3);
    fe_mul(d.at(r), a, k);
  });
}
// c = the projective point (2X : 2Y : 2Z) that an addend IS (lane 3 is left undefined-but-bounded: a doubling follows, which does not
// read T).  Classes: X, Y carried to [1], Z as stored.
template <class Q> EG_HD void quad_cached_to_p2(Q& q, qfe<Q>& c, const qfe<Q>& d) {
  qfe<Q> u;
  q.template perm<1, 0, 3, 2>(u, d);                                    // Y-X  Y+X  2Z  2dT
  q.each([&](int r) {
    fe sum, dif, x = u.at(r);                                           // lane 2: 2Z
    fe_sub4(dif, d.at(r), u.at(r));                                     // lane 0: 2X
    fe_add(sum, d.at(r), u.at(r));                                      // lane 1: 2Y
    fe_cmov(x, dif, r == 0);
    fe_cmov(x, sum, r == 1);
    fe_carry(x);
    c.at(r) = x;
  });
}

// c = the point (2X : 2Y : 2Z : 2T) that an addend IS, with T (one multiplication: by 1, 1, 1, 1/d); accepts the lazily stored classes
// (<= 3); returns [1]
template <class Q> EG_HD void quad_cached_to_p3(Q& q, qfe<Q>& c, const qfe<Q>& d) {
  qfe<Q> u;
  q.template perm<1, 0, 3, 2>(u, d);                                    // Y-X  Y+X  2Z  2dT
  q.each([&](int r) {
    const fe dinv = EG_FE_DINV;
    fe sum, dif, a = u.at(r), k;                                        // lane 2: 2Z, lane 3: 2dT
    fe_sub4(dif, d.at(r), u.at(r));                                     // lane 0: 2X [<= 7]
    fe_add(sum, d.at(r), u.at(r));                                      // lane 1: 2Y [<= 6]
    fe_cmov(a, dif, r == 0);
    fe_cmov(a, sum, r == 1);
    fe_1(k);
    fe_cmov(k, dinv, r == 3);
    fe_mul(c.at(r), a, k);
  });
}

// ---- products -----------------------------------------------------------------------------------------------------------------------------
// acc = [k]P from the comb table of P (ge_teeth_mul on a quad); io.load(d, idx, neg) delivers entry idx as an addend with Y+X / Y-X
// already swapped when neg.  50 (42) doublings + 50 (42) additions for 5 (6) teeth.
template <int T, class Q, class TableIO>
EG_HD void quad_teeth_mul(Q& q, qfe<Q>& acc, TableIO& io, u64 rows[T]) {
  {
    int idx; bool neg;
    sc_teeth_next<T>(rows, idx, neg);
    qfe<Q> cur;
    io.load(q, cur, idx, neg);
    quad_cached_to_p2(q, acc, cur);
  }
#pragma unroll 1
  for (int c = Teeth<T>::COLS - 2; c >= 0; --c) {
    int idx; bool neg;
    sc_teeth_next<T>(rows, idx, neg);
    qfe<Q> cur;
    io.load(q, cur, idx, neg);
    quad_dbl(q, acc);
    quad_cached_neg_t(q, cur, neg);
    quad_add(q, acc, cur);
  }
}

// acc += [k]Base over a fixed-base comb table (ge_fixed_mul_add on a quad); io.load(d, idx, neg) delivers a Niels entry as an addend
// with 2Z = 2 in lane 3; io.bits = the table's window width.  One addition per window, entries requested one addition ahead.
template <class Q, class NielsIO>
EG_HD void quad_fixed_mul_add(Q& q, qfe<Q>& acc, NielsIO& io, const u32 k[EG_COMB_WORDS]) {
  qfe<Q> ident, nxt;
  quad_cached_identity(q, ident);
  const int bits = io.bits, windows = comb_windows(bits);
  u32 carry = 0;
  int d_nxt = sc_comb_digit(k, 0, carry, bits);
  io.load(q, nxt, ge_fixed_index(0, d_nxt, bits), d_nxt < 0);
#pragma unroll 1
  for (int i = 0; i < windows; ++i) {
    qfe<Q> c = nxt;
    const int d = d_nxt;
    if (i + 1 < windows) {
      d_nxt = sc_comb_digit(k, i + 1, carry, bits);
      io.load(q, nxt, ge_fixed_index(i + 1, d_nxt, bits), d_nxt < 0);
    }
    quad_select(q, c, ident, d == 0);
    quad_cached_neg_t(q, c, d < 0);
    quad_add(q, acc, c);
  }
}

// the comb table of P (ge_teeth_tables_build on a quad): the same entries in the same slots, so that one-lane code can read a table a
// quad has built.  The T - 1 steps 2 P_j of the Gray-code walk stay in registers (one field element per lane and step).
template <int T, class Q, class TableIO>
EG_HD void quad_teeth_tables_build(Q& q, TableIO& io, const qfe<Q>& p) {
  qfe<Q> cur = p, sum, steps[T - 1];
  quad_identity(q, sum);
#pragma unroll
  for (int j = 0; j < T - 1; ++j) {
    {
      qfe<Q> pc;
      quad_to_cached(q, pc, cur);
      quad_cached_cneg(q, pc, true);
      quad_add(q, sum, pc);                   // sum -= P_j
    }
    quad_dbl(q, cur);                         // 2 P_j
    quad_to_cached(q, steps[j], cur);
#pragma unroll 1
    for (int r = 0; r < Teeth<T>::COLS - 1; ++r) quad_dbl(q, cur);      // P_(j+1)
  }
  {
    qfe<Q> pc, e;
    quad_to_cached(q, pc, cur);
    quad_add(q, sum, pc);                     // entry 0 = P_(T-1) - .. - P_0
    quad_to_cached(q, e, sum);
    io.store(q, 0, e);
  }
#pragma unroll 1
  for (int i = 1; i < Teeth<T>::ENTRIES; ++i) {
    int j = 0;
    while (((i >> j) & 1) == 0) ++j;          // Gray code: step i flips tooth ctz(i)
    const int g = i ^ (i >> 1);
    qfe<Q> qc = steps[0], e;
#pragma unroll
    for (int k = 1; k < T - 1; ++k) quad_select(q, qc, steps[k], j == k);
    quad_cached_cneg(q, qc, ((g >> j) & 1) == 0);
    quad_add(q, sum, qc);
    quad_to_cached(q, e, sum);
    io.store(q, g, e);
  }
}

// the comb table of S = B_1 + .. + B_m from the members' tables (ge_teeth_tables_sum on a quad): no doublings; src(k, g, d) loads entry g
// of member k as an addend.  The T - 1 steps of the walk stay in registers.
template <int T, class Q, class TableIO, class SrcFn>
EG_HD void quad_teeth_tables_sum(Q& q, TableIO& io, int m, SrcFn src) {
  qfe<Q> sum, steps[T - 1];
  quad_identity(q, sum);
#pragma unroll
  for (int k = 0; k < T - 1; ++k) steps[k] = sum;
#pragma unroll 1
  for (int i = 0; i < Teeth<T>::ENTRIES; ++i) {
    const int g = i ^ (i >> 1);
    int j = 0;
    while (i != 0 && ((i >> j) & 1) == 0) ++j;      // Gray code: step i flips tooth ctz(i)
    if ((i & (i - 1)) == 0) {                       // first flip of tooth j (or the start): entry g summed over the members
      qfe<Q> acc, c;
      src(0, g, c);
      quad_cached_to_p3(q, acc, c);
#pragma unroll 1
      for (int k = 1; k < m; ++k) {
        src(k, g, c);
        quad_add(q, acc, c);
      }
      if (i != 0) {                                 // step of tooth j: 2 P_j(S) = entry g - previous entry
        qfe<Q> pc, d = acc, dc;
        quad_to_cached(q, pc, sum);
        quad_cached_cneg(q, pc, true);
        quad_add(q, d, pc);
        quad_to_cached(q, dc, d);
#pragma unroll
        for (int k = 0; k < T - 1; ++k) quad_select(q, steps[k], dc, j == k);
      }
      sum = acc;
    } else {
      qfe<Q> qc = steps[0];
#pragma unroll
      for (int k = 1; k < T - 1; ++k) quad_select(q, qc, steps[k], j == k);
      quad_cached_cneg(q, qc, ((g >> j) & 1) == 0);
      quad_add(q, sum, qc);
    }
    qfe<Q> e;
    quad_to_cached(q, e, sum);
    io.store(q, g, e);
  }
}

}  // namespace eg
