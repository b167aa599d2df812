// provecheck.cpp -- TEST-ONLY build of the host logic behind the single-item provers (csrc/host_plan.hpp: check_prove_inputs,
// prove_inputs_per_item, scalar_bytes_canonical; csrc/plan.h: the per-lane workspace counts) under AddressSanitizer + UBSan.  The
// product never loads this library.
#include <stdint.h>
#include <string.h>
#include "../../elastic_elgamal_amd/csrc/host_plan.hpp"

using namespace eghost;

extern "C" {
int pc_inputs_per_item(int kind, int n_values) { return prove_inputs_per_item(kind, n_values); }
// 0 = admissible; 1 = refused (why_out says why)
int pc_check(int kind, unsigned long long upper_bound, int n_values, const unsigned long long* inputs, unsigned long long n, char* why_out,
             int cap) {
  const char* why = check_prove_inputs(kind, upper_bound, n_values, reinterpret_cast<const uint64_t*>(inputs), (size_t)n);
  if (why_out && cap > 0) { strncpy(why_out, why ? why : "", cap - 1); why_out[cap - 1] = 0; }
  return why ? 1 : 0;
}
int pc_scalar_canonical(const unsigned char s[32]) { return scalar_bytes_canonical(s) ? 1 : 0; }
// the workspace of a range proof over RangeDecomposition::optimal(upper_bound), and the decomposition's shape for the test's own count
unsigned pc_range_ws_words(unsigned long long upper_bound, unsigned* n_rings, unsigned* responses) {
  const RangeDecomposition d = optimal_range(upper_bound);
  *n_rings = (unsigned)d.rings.size();
  *responses = (unsigned)d.rings_size();
  return egplan::gen_range_ws_words((uint32_t)d.rings.size(), (uint32_t)d.rings_size());
}
unsigned pc_sumsq_ws_words(unsigned n_values) { return egplan::gen_sumsq_ws_words(n_values); }
unsigned pc_share_ws_words(void) { return egplan::gen_share_ws_words(); }
// the prefixes the provers import are the ones the plans hoist: index inside the plan's prefixes, or -1
int pc_gen_prefix(int kind, int which) {
  size_t item = 0;
  uint8_t pk[32]; memset(pk, 7, 32);
  Plan P;
  switch (kind) {
    case PROVE_ZERO: P = build_zero_plan(); break;
    case PROVE_BOOL: P = build_bool_plan(); break;
    case PROVE_RANGE: P = build_range_plan(100, &item); break;
    case PROVE_SHARE: P = build_share_plan(10, 7, pk, 2); break;
    case PROVE_SUMSQ: P = build_sumsq_plan(5, "test", &item); break;
    default: return -2;
  }
  const int v[] = {P.gen_pre_main, P.gen_pre_ring, P.gen_pre_logeq, P.gen_pre_sumsq};
  return which >= 0 && which < 4 && v[which] < P.n_prefixes ? v[which] : -2;
}
}
