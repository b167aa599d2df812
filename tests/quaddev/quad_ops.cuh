// quad_ops.cuh -- TEST-ONLY: the quad operations of csrc/ge25519_quad.cuh behind one raw-limb calling convention, shared by the
// bound-check host build (tests/hostcheck/quadcheck.cpp, a quad emulated as four lanes) and the device build next to this file
// (quaddev.hip, a quad = four adjacent lanes), so that both run the same case code and can be compared limb for limb.
//
// A case has two operands of four field elements each, in the ONE-LANE order: a point (X, Y, Z, T) or an addend (Y+X, Y-X, 2Z, 2dT).
// a_pt / a_cd are operand a distributed over the quad as a point (lane r = element r) and as an addend (lane r = element
// QUAD_CACHED_ORDER[r]); b_cd is operand b as an addend.  The result comes back distributed; *cached says in which of the two orders.
#pragma once
#include "../../elastic_elgamal_amd/csrc/ge25519_quad.cuh"

namespace eg {

enum { QOP_DBL = 0, QOP_ADD, QOP_MADD, QOP_TO_CACHED, QOP_CACHED_CNEG, QOP_NEG, QOP_CACHED_TO_P2, QOP_IDENTITY, QOP_DBL_WIDE,
       QOP_CACHED_TO_P3, QOP_CACHED_NEG_T, QOP_CACHED_IDENTITY, QOP_FROM_CACHED, QOP_COUNT };
// lane r of an addend holds element QUAD_CACHED_ORDER[r] of (Y+X, Y-X, 2Z, 2dT)
EG_HD int quad_cached_order(int r) { return r < 2 ? r : (r == 2 ? 3 : 2); }

template <class Q>
EG_HD void quad_case(Q& q, int op, const qfe<Q>& a_pt, const qfe<Q>& a_cd, const qfe<Q>& b_cd, qfe<Q>& out, bool& cached) {
  cached = false;
  switch (op) {
    case QOP_DBL: case QOP_DBL_WIDE:
      out = a_pt;
      quad_dbl(q, out);
      break;
    case QOP_ADD:
      out = a_pt;
      quad_add(q, out, b_cd);
      break;
    case QOP_MADD: {
      qfe<Q> d = b_cd, ident;
      quad_cached_identity(q, ident);                        // lane 3 of the neutral addend is the Niels form's 2Z = 2
      q.each([&](int r) { fe_cmov(d.at(r), ident.at(r), r == 3); });
      out = a_pt;
      quad_add(q, out, d);
      break;
    }
    case QOP_TO_CACHED:
      quad_to_cached(q, out, a_pt);
      cached = true;
      break;
    case QOP_CACHED_CNEG:
      out = a_cd;
      quad_cached_cneg(q, out, true);
      cached = true;
      break;
    case QOP_NEG:
      out = a_pt;
      quad_neg(q, out, true);
      break;
    case QOP_CACHED_TO_P2:
      quad_cached_to_p2(q, out, a_cd);
      break;
    case QOP_IDENTITY: {
      qfe<Q> id;
      quad_identity(q, id);
      out = a_pt;
      quad_select(q, out, id, true);
      break;
    }
    case QOP_CACHED_TO_P3:
      quad_cached_to_p3(q, out, a_cd);
      break;
    case QOP_CACHED_NEG_T:
      out = a_cd;
      quad_cached_neg_t(q, out, true);
      cached = true;
      break;
    case QOP_CACHED_IDENTITY: {
      qfe<Q> id;
      quad_cached_identity(q, id);
      out = a_cd;
      quad_select(q, out, id, true);
      cached = true;
      break;
    }
    case QOP_FROM_CACHED: {                                  // every lane is handed the whole one-lane addend and keeps its own part
      typename Q::template var<fe4> g;
      q.gather(g, a_pt);
      const fe4& w = g.at(0);
      const ge_cached c{w.v[0], w.v[1], w.v[2], w.v[3]};
      quad_from_cached(q, out, c);
      cached = true;
      break;
    }
    default: break;
  }
}

}  // namespace eg
