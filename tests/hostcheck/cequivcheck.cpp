// cequivcheck.cpp -- TEST-ONLY build of the commitment-equivalence plan (csrc/host_plan.hpp: build_commit_equiv_plan, its flattening
// and the index check of the third fixed base's scalar sources) under AddressSanitizer + UBSan.  The product never loads this library.
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../elastic_elgamal_amd/csrc/host_plan.hpp"

using namespace eghost;

static int check(Plan& P, char* why_out, int cap) {
  uint8_t pk[32]; memset(pk, 7, 32);
  if (P.pk_off >= 0) memcpy(P.blob.data() + P.pk_off, pk, 32);
  const FlatPlan F = flatten_plan(P);
  const std::string why = check_flat_plan(P, F);
  if (why_out && cap > 0) { strncpy(why_out, why.c_str(), cap - 1); why_out[cap - 1] = 0; }
  if (!why.empty()) return -1;
  // what the engine relies on beyond the index check: the three equations are of the direct family, and exactly one names H
  int with_h = 0;
  for (auto& j : F.jobs) {
    if (job_family(j, P.vterms) != FAM_DIRECT1) return -3;
    with_h += j.h != 0;
  }
  if (with_h != 1 || P.h_srcs.size() != 1 || F.stages.size() != 1 || F.stages[0].fam_count[FAM_DIRECT1] != 3) return -4;
  return (int)F.jobs.size();
}

extern "C" {
// the plan for a label of any length the ABI admits; returns its number of equations, -1 if the index check refuses it
int ce_plan(const char* label, int label_len, char* why_out, int cap) {
  Plan P = build_commit_equiv_plan(std::string(label, (size_t)label_len));
  return check(P, why_out, cap);
}
unsigned long long ce_stride(void) { return build_commit_equiv_plan("test").stride; }
// the plan with its H scalar source bent on purpose: 1 = wire item beyond the item, 2 = job names a source beyond the side array,
// 3 = the source is SRC_NONE, 4 = a challenge slot the plan does not have, 5 = an H term on an equation WITHOUT a variable base (not
// the direct family: no kernel would add it).  Returns 0 if check_flat_plan accepts, 1 if it refuses (why_out says why).
int ce_plan_mutated(int mutation, char* why_out, int cap) {
  Plan P = build_commit_equiv_plan("test");
  JobClass* with_h = nullptr;
  for (auto& j : P.stages[0].jobs) if (j.h) with_h = &j;
  if (!with_h) return -2;
  switch (mutation) {
    case 0: break;
    case 1: P.h_srcs[with_h->h - 1].idx = (uint16_t)(P.stride / 32); break;
    case 2: with_h->h = (uint16_t)(P.h_srcs.size() + 1); break;
    case 3: P.h_srcs[with_h->h - 1].kind = SRC_NONE; break;
    case 4: P.h_srcs[with_h->h - 1] = ScalarSrc{SRC_CHAL, 0, 0, 0}; break;
    case 5: with_h->term_count = 0; break;
    default: return -2;
  }
  const int r = check(P, why_out, cap);
  return r == -1 ? 1 : (r > 0 ? 0 : r);
}
// the existing plans carry no H term and an empty side array
int ce_others_have_no_h(void) {
  size_t item = 0;
  uint8_t pk[32]; memset(pk, 7, 32);
  Plan plans[] = {build_choice_plan(5, true), build_choice_plan(16, false), build_qv_plan(5, 20), build_zero_plan(), build_bool_plan(),
                  build_range_plan(100, &item), build_sumsq_plan(3, "test", &item), build_share_plan(10, 7, pk, 2)};
  for (auto& P : plans) {
    if (P.has_h()) return 0;
    for (auto& st : P.stages) for (auto& j : st.jobs) if (j.h) return 0;
  }
  return 1;
}
}
