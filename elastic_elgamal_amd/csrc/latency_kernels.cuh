// latency_kernels.cuh -- the small-batch verifier: ONE workgroup verifies ONE ballot from wire bytes to status word in ONE launch.
//
// The batch engine (kernels.cuh) maps one lane to one group equation of one ballot and chains about twenty kernels per call; for a
// handful of ballots the chip is empty and the caller waits for the dependent chain of one lane.  k_ballot_small walks
// the same plan - wire items, derive classes, table builds, job classes per stage, deferred encodings, hash programs, status rules - with
// __syncthreads() where the batch engine has kernel boundaries, and gives the long chains (the comb table of a ring base, the ring
// equations over it, the fixed-base combs) a QUAD of lanes each (ge25519_quad.cuh).  The cold phases call the per-ballot step bodies
// of kernels.cuh, the very ones the batch kernels wrap, one lane per item: this file adds the assignment of threads, quads and lanes
// and the barriers, no second copy of a rule.  Intermediate values live in the engine's work-set buffers, as in the batch path: the
// tables a quad builds have the layout of BaseTable, so the one-lane families (several bases on one chain, sums of tables) read them.
//
// What stays separate from the batch path, on purpose:
//   - quad_eq_fixed_terms against eq_fixed_terms, and the quad evaluation of the one-table equations (FAM_TABLE1): other table types
//     (QuadFixedTable, QuadBaseTable) and another multiply (one field element a lane); a shared body would have to branch on its caller;
//   - the deferred-commitment encode: one inverse a lane here, one batched inversion in k_encode_batch / k_encode_hash (the comment at
//     the loop says why);
//   - the comb-table builds on quads (quad_teeth_tables_build / quad_teeth_tables_sum).
//
// Block size: 4 lanes per quad of the widest stage, a multiple of 64, at most 256 (one wavefront per SIMD: the kernel is sized for
// latency, and a block that wide leaves every lane the whole register file, so nothing spills); wider stages loop.
#pragma once
#include "host_plan.hpp"
#include "kernels.cuh"
#include "ge25519_quad.cuh"

namespace eg {

constexpr int SM_MAX_THREADS = 256;
constexpr int SM_LANES = 64;                          // lanes of the one-lane phases that need LDS or workspace per lane
constexpr int SM_LDS_WORDS = eghost::EG_MULTI_GROUP * 9 * SM_LANES;  // the largest user: sign vectors of a shared doubling chain

struct SmallPlanDev {
  const egplan::WireItem *pt_items, *sc_items;
  int n_pt, n_sc;
  const egplan::DeriveClass* dclasses;
  const egplan::DeriveTerm* dterms;
  const eghost::LevelDev* levels;
  int n_levels;
  const eghost::StageDev* stages;
  int n_stages;
  const egplan::JobClass* jobs;
  const egplan::VarTerm* vterms;
  const egplan::HashInst* insts;
  const egplan::HashOp* ops;
  const egplan::StatusRule* rules;
  int n_rules;
  const unsigned short* base_slots;
  const egplan::SumBase* sums;
  const unsigned short* sum_members;
  int n_sums;
  const egplan::SumBase* acc_sums;
  const unsigned short* acc_members;
  const unsigned short* defer_slots;
  uint4* ws;                 // [block][SM_LANES][WS_QUADS]: radix-16 tables of the equations without a comb table; null if the plan has none
};

// ---- quad I/O ---------------------------------------------------------------------------------------------------------------------------
// coordinate r of a point row ([slot][PT_QUADS][cap] uint4, 9 words per coordinate)
__device__ __forceinline__ void quad_load_pt(const QuadDev& q, QuadDev::var<fe>& c, const uint4* pts, u32 cap, u32 slot, u32 b) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) {
    const int w = q.r * EG_NL + i;
    c.v.v[i] = reinterpret_cast<const u32*>(&pts[((size_t)slot * PT_QUADS + (w >> 2)) * cap + b])[w & 3];
  }
}
__device__ __forceinline__ void quad_store_pt(const QuadDev& q, uint4* pts, u32 cap, u32 slot, u32 b, const QuadDev::var<fe>& c) {
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) {
    const int w = q.r * EG_NL + i;
    reinterpret_cast<u32*>(&pts[((size_t)slot * PT_QUADS + (w >> 2)) * cap + b])[w & 3] = c.v.v[i];
  }
}
// a BaseTable seen by a quad: lane r reads / writes its own 32 bytes of the 128-byte entry (Y+X, Y-X, 2Z, 2dT: lanes 0, 1, 3, 2)
struct QuadBaseTable {
  uint4* base;
  __device__ __forceinline__ void load(const QuadDev& q, QuadDev::var<fe>& d, int e, bool neg) const {
    const int el = q.r < 2 ? (q.r ^ (neg ? 1 : 0)) : (q.r == 2 ? 3 : 2);
    const uint4 a = base[e * BTAB_ENTRY_QUADS + 2 * el], c = base[e * BTAB_ENTRY_QUADS + 2 * el + 1];
    const u32 w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    fe_unpack8(d.v, w);
  }
  __device__ __forceinline__ void store(const QuadDev& q, int e, const QuadDev::var<fe>& d) {
    const int el = q.r < 2 ? q.r : (q.r == 2 ? 3 : 2);
    u32 w[8];
    fe_pack8(w, d.v);
    base[e * BTAB_ENTRY_QUADS + 2 * el] = make_uint4(w[0], w[1], w[2], w[3]);
    base[e * BTAB_ENTRY_QUADS + 2 * el + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
};
// a FixedTable seen by a quad: lanes 0..2 read (y+x, y-x, 2dxy), lane 3 holds 2Z = 2
struct QuadFixedTable {
  const u32* tab;
  int bits;
  __device__ __forceinline__ explicit QuadFixedTable(const uint4* t) : tab(reinterpret_cast<const u32*>(t)), bits((int)reinterpret_cast<const u32*>(t)[-4]) {}
  __device__ __forceinline__ void load(const QuadDev& q, QuadDev::var<fe>& d, int idx, bool neg) const {
    const int el = q.r < 2 ? (q.r ^ (neg ? 1 : 0)) : 2;
    const u32* p = tab + (size_t)idx * 32 + el * EG_NL;
#pragma unroll
    for (int i = 0; i < EG_NL; ++i) d.v.v[i] = p[i];
    fe two; fe_0(two); two.v[0] = 2;
    fe_cmov(d.v, two, q.r == 3);
  }
};

// the fixed-base terms of an equation on a quad (eq_fixed_terms)
__device__ __forceinline__ void quad_eq_fixed_terms(QuadDev& q, QuadDev::var<fe>& acc, const EngineBufs& B, u32 b, const egplan::JobClass& jc) {
  if (jc.g.kind != egplan::SRC_NONE) {
    const QuadFixedTable tg(B.tabG);
    u32 s[8], dg[EG_COMB_WORDS];
    load_scalar(s, B, b, jc.g, true);
    sc_recode_comb(dg, s);
    quad_fixed_mul_add(q, acc, tg, dg);
  }
  if (jc.k.kind != egplan::SRC_NONE) {
    const QuadFixedTable tk(B.tabK);
    u32 s[8], dg[EG_COMB_WORDS];
    load_scalar(s, B, b, jc.k, true);
    sc_recode_comb(dg, s);
    quad_fixed_mul_add(q, acc, tk, dg);
  }
}

// ---- the kernel: block b = ballot b ---------------------------------------------------------------------------------------------------
template <int T>
__global__ void __launch_bounds__(SM_MAX_THREADS) k_ballot_small(EngineBufs B, SmallPlanDev P) {
  __shared__ u32 lds[SM_LDS_WORDS];
  const u32 b = blockIdx.x;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int qid = tid >> 2, nq = nt >> 2;
  QuadDev q(tid);

  // wire items: decode every point, check every scalar
  if (tid == 0) B.bad_item[b] = 0xffffffffu;
  __syncthreads();
  for (int k = tid; k < P.n_pt; k += nt) wire_point_decode(B, b, P.pt_items[k]);
  for (int k = tid; k < P.n_sc; k += nt) wire_scalar_check(B, b, P.sc_items[k]);
  __syncthreads();

  // derived points, level by level
  for (int l = 0; l < P.n_levels; ++l) {
    const eghost::LevelDev lv = P.levels[l];
    for (int k = tid; k < lv.count; k += nt) point_derive(B, b, P.dclasses[lv.first + k], P.dterms);
    if (lv.count) __syncthreads();
  }

  for (int si = 0; si < P.n_stages; ++si) {
    const eghost::StageDev st = P.stages[si];
    // comb tables this stage starts with: one QUAD per base
    if (st.build_count) {
      for (int k = qid; k < st.build_count; k += nq) {
        QuadDev::var<fe> p;
        quad_load_pt(q, p, B.pts, B.cap, P.base_slots[st.build_first + k], b);
        QuadBaseTable bt{B.btab + ((size_t)k * B.cap + b) * btab_quads<T>()};
        quad_teeth_tables_build<T>(q, bt, p);
      }
      __syncthreads();
    }
    if (st.sums_direct) {                   // tables of the sums of bases from the members' tables: a quad per sum
      for (int k = qid; k < P.n_sums; k += nq) {
        const egplan::SumBase sb = P.sums[k];
        QuadBaseTable out{B.btab + ((size_t)sb.out_base * B.cap + b) * btab_quads<T>()};
        quad_teeth_tables_sum<T>(q, out, (int)sb.count, [&](int t, int g, QuadDev::var<fe>& e) {
          const QuadBaseTable bt{B.btab + ((size_t)P.sum_members[sb.first + t] * B.cap + b) * btab_quads<T>()};
          bt.load(q, e, g, false);
        });
      }
      __syncthreads();
    }
    if (st.acc_count) {
      for (int j = tid; j < st.acc_count * T; j += nt) {
        const egplan::SumBase rec = P.acc_sums[st.acc_first + j / T];
        BaseTable acc{B.sacc + ((size_t)rec.out_base * B.cap + b) * (T * BTAB_ENTRY_QUADS)};
        ge_teeth_sum_accumulate<T>(acc, j % T, rec.pad != 0, (int)rec.count, [&](int t, int g, ge_cached& e) {
          const BaseTable bt{B.btab + ((size_t)P.acc_members[rec.first + t] * B.cap + b) * btab_quads<T>()};
          bt.load(e, g);
        });
      }
      __syncthreads();
    }
    if (st.sum_finish) {
      for (int k = qid; k < P.n_sums; k += nq) {
        QuadBaseTable out{B.btab + ((size_t)P.sums[k].out_base * B.cap + b) * btab_quads<T>()};
        const QuadBaseTable acc{B.sacc + ((size_t)k * B.cap + b) * (T * BTAB_ENTRY_QUADS)};
        quad_teeth_tables_sum<T>(q, out, 1, [&](int, int g, QuadDev::var<fe>& e) { acc.load(q, e, teeth_first_flip_index<T>(g), false); });
      }
      __syncthreads();
    }

    // the group equations of the stage.  One table-backed base (every ring equation): a quad each
    for (int j = qid; j < st.fam_count[eghost::FAM_TABLE1]; j += nq) {
      const egplan::JobClass jc = P.jobs[st.fam_first[eghost::FAM_TABLE1] + j];
      const egplan::VarTerm vt = P.vterms[jc.term_first];
      u32 s[8];
      load_scalar(s, B, b, vt.s, true);
      u64 rows[T];
      sc_recode_teeth<T>(rows, s);
      QuadBaseTable bt{B.btab + ((size_t)vt.base * B.cap + b) * btab_quads<T>()};
      QuadDev::var<fe> acc;
      quad_teeth_mul<T>(q, acc, bt, rows);
      quad_eq_fixed_terms(q, acc, B, b, jc);
      quad_store_pt(q, B.dpt, B.cap, jc.out_slot, b, acc);
    }
    // several table-backed bases on shared doubling chains: one lane each, sign vectors in LDS
    for (int j0 = 0; j0 < st.fam_count[eghost::FAM_TABLEN]; j0 += SM_LANES) {
      const int j = j0 + tid;
      if (tid < SM_LANES && j < st.fam_count[eghost::FAM_TABLEN]) {
        const egplan::JobClass jc = P.jobs[st.fam_first[eghost::FAM_TABLEN] + j];
        ge acc;
        eq_shared_chains<T>(acc, B, b, jc, P.vterms, eghost::EG_MULTI_GROUP, [&](int t, int w) -> u32& { return lds[(t * 9 + w) * SM_LANES + tid]; });
        eq_fixed_terms(acc, B, b, jc);
        store_pt(B.dpt, B.cap, jc.out_slot, b, acc);
      }
    }
    // everything else: one lane each over a radix-16 table in the block's workspace slice.  JobClass::h (a term over the third fixed
    // base, k_eq_direct_h) is NOT evaluated here: no ballot plan has one, and engine_small_prepare refuses a plan that does
    {
      const int first = st.fam_first[eghost::FAM_DIRECT1];
      const int count = st.fam_count[eghost::FAM_DIRECT1] + st.fam_count[eghost::FAM_GENERIC];
      for (int j0 = 0; j0 < count; j0 += SM_LANES) {
        const int j = j0 + tid;
        if (tid < SM_LANES && j < count) {
          const int ci = j < st.fam_count[eghost::FAM_DIRECT1] ? first + j : st.fam_first[eghost::FAM_GENERIC] + (j - st.fam_count[eghost::FAM_DIRECT1]);
          WsTable tab{P.ws + ((size_t)b * SM_LANES + tid) * WS_QUADS};
          eq_term_by_term<T>(B, b, P.jobs[ci], P.vterms, tab);
        }
      }
    }
    for (int j = tid; j < st.fam_count[eghost::FAM_ENCODE]; j += nt) point_encode_plain(B, b, P.jobs[st.fam_first[eghost::FAM_ENCODE] + j]);
    __syncthreads();

    // deferred commitments, out = encode(2P): one lane each.  The batch path encodes a ballot's commitments with ONE inversion in ONE
    // lane (k_encode_batch), which is the cheapest in total and the longest to wait for; here every lane pays its own inverse square
    // root and they all finish together (encodings are canonical, so the bytes are the same)
    for (int k = tid; k < st.defer_count; k += nt) {
      const u32 slot = P.defer_slots[st.defer_first + k];
      ge p, p2;
      load_pt(p, B.dpt, B.cap, slot, b);
      ge_dbl_full(p2, p);
      u32 out[8];
      ristretto_encode(out, p2);
      store32(B.cmp, B.cap, slot, b, out);
    }
    __syncthreads();

    // transcripts: the stage's Merlin programs, SM_LANES at a time
    for (int i0 = 0; i0 < st.inst_count; i0 += SM_LANES) {
      const int i = i0 + tid;
      if (tid < SM_LANES && i < st.inst_count) hash_program<LdsStateT<SM_LANES>, false>(B, b, P.insts[st.inst_first + i], P.ops, lds + tid);
    }
    __syncthreads();
  }

  if (tid == 0) ballot_status(B, b, P.rules, P.n_rules);
}

}  // namespace eg
