// chain_ops.cuh -- TEST-ONLY: the fused square-and-subtract and the chain doubling of fe25519.cuh / ge25519.cuh behind the raw-limb
// calling convention of tests/devcheck/limb_ops.cuh (80 input words = 8 slots of 9 limbs + 8 extra words, 8 classes, 80 output
// words), shared by the stand-alone host program (tests/hostcheck/dblchaincheck.cpp, bound-check build) and the device build
// (tests/dblchaindev/dblchaindev.hip), so that both compilations of the headers run the same calls on the same records
// (tests/dbl_chain_cases.py makes the records and holds the reference).  Never part of the product.
#pragma once
#include "../../elastic_elgamal_amd/csrc/ge25519.cuh"

#define CHAIN_SLOTS 8
#define CHAIN_WORDS 80
#define CHAIN_EXTRA 72

namespace eg {

enum ChainOp {
  // f = slot 0, g = slot 1 -> h = slot 0, h aliasing f = slot 1, h aliasing g = slot 2, canonical words of h = extra
  COP_SQ2_SUB = 0,
  // X, Y, Z = slots 0..2, extra[0]: 0 = ge_dbl_chain_sgn(.., false), 1 = ge_dbl_chain_sgn(.., true) (the negated point), 2 = ge_dbl_chain
  // -> its p1p1 (E, H, G, F) = slots 0..3, that of ge_dbl on the same (X, Y, Z) = slots 4..7
  COP_DBL_CHAIN,
  COP_COUNT
};

EG_HD void co_load(fe& f, const u32* in, const float* cls, int slot) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) f.v[i] = in[EG_NL * slot + i];
  (void)cls;
  EG_SETCLS(f, cls[slot]);
  fe_check_values(f);
}
EG_HD void co_store(u32* out, int slot, const fe& f) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) out[EG_NL * slot + i] = f.v[i];
}

EG_HD void chain_op(int op, const u32* in, const float* cls, u32* out) {
  if (op == COP_SQ2_SUB) {
    fe f, g, h, a, b;
    co_load(f, in, cls, 0); co_load(g, in, cls, 1);
    a = f; b = g;
    fe_sq2_sub(h, f, g); fe_sq2_sub(a, a, g); fe_sq2_sub(b, f, b);
    co_store(out, 0, h); co_store(out, 1, a); co_store(out, 2, b);
    u32 w[8]; fe_to_words(w, h);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[CHAIN_EXTRA + i] = w[i];
  } else {
    fe X, Y, Z;
    co_load(X, in, cls, 0); co_load(Y, in, cls, 1); co_load(Z, in, cls, 2);
    const u32 flag = in[CHAIN_EXTRA];
    ge_p1p1 t, u;
    if (flag == 2) ge_dbl_chain(t, X, Y, Z);
    else ge_dbl_chain_sgn(t, X, Y, Z, flag == 1);
    ge_dbl(u, X, Y, Z);
    co_store(out, 0, t.X); co_store(out, 1, t.Y); co_store(out, 2, t.Z); co_store(out, 3, t.T);
    co_store(out, 4, u.X); co_store(out, 5, u.Y); co_store(out, 6, u.Z); co_store(out, 7, u.T);
  }
}

}  // namespace eg
