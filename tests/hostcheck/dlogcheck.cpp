// Host build of the discrete-log lanes (elastic_elgamal_amd/csrc/dlog_kernels.cuh) with -DEG_BOUNDCHECK: the baby build and the giant
// walk run as lanes over arrays, with 4-bit tags (false candidates are certain) and baby tables of 2^4 and 2^6 entries.  Every field
// operation asserts its limb-class precondition, so a clean run proves the bound discipline of the new chain over whole runs.
// Stand-alone program (tests/test_dlog_solver_cpu.py builds it under UBSan and reads its report): exit code 0 and "PASS" = every check held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <vector>
#include "../../elastic_elgamal_amd/csrc/dlog_kernels.cuh"

using namespace eg;

constexpr int TAG = 4;

// comb table of G with entries made on demand (the product's has millions; a comb touches one per window)
struct NielsOnDemand {
  int bits = 8;
  mutable std::map<int, ge_niels> cache;
  void load(ge_niels& c, int idx) const {
    auto it = cache.find(idx);
    if (it == cache.end()) {
      const int w = idx / comb_entries(bits), k = idx % comb_entries(bits) + 1;
      ge p; ge_generator(p);
      for (int i = 0; i < bits * w; ++i) { ge d; ge_dbl_full(d, p); p = d; }
      ge q; ge_identity(q);
      for (int bit = bits - 1; bit >= 0; --bit) {
        ge d; ge_dbl_full(d, q); q = d;
        if ((k >> bit) & 1) { ge t; ge_add_full(t, q, p); q = t; }
      }
      ge_niels n; ge_to_niels(n, q);
      it = cache.emplace(idx, n).first;
    }
    c = it->second;
  }
};
struct RunArr {
  fe Y[DLOG_RUN], Z[DLOG_RUN], P[DLOG_RUN];
  void store(int i, const fe& y, const fe& z, const fe& pre) { Y[i] = y; Z[i] = z; P[i] = pre; }
  void load(int i, fe& y, fe& z, fe& pre) const { y = Y[i]; z = Z[i]; pre = P[i]; }
};
struct SlotsArr {
  std::vector<u64> tab;
  unsigned overflowed = 0;
  std::map<u32, fe> ys;          // canonical y of every inserted entry
  u64 cas(u32 pos, u64 v) { const u64 old = tab[pos]; if (old == 0) tab[pos] = v; return old; }
  u64 get(u32 pos) const { return tab[pos]; }
  void note(u32 idx, const fe& y) { ys[idx] = y; }
  void overflow() { ++overflowed; }
};
struct SinkVec {
  std::vector<std::pair<u32, u64>> c;
  void push(u32 elem, u64 m) { c.push_back({elem, m}); }
};

static NielsOnDemand g_tab;
static unsigned long long g_fail = 0, g_false_candidates = 0, g_found = 0, g_lanes = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void mul_generator(ge& out, const u32 k[8]) {
  u32 dg[EG_COMB_WORDS];
  sc_recode_comb(dg, k);
  ge_identity(out);
  ge_fixed_mul_add(out, g_tab, dg);
}
struct Enc { u32 w[8]; bool operator==(const Enc& o) const { return memcmp(w, o.w, 32) == 0; } };
static Enc encode_multiple(u64 m, bool negate = false) {
  u32 k[8], nk[8]; sc_from_u64(k, m);
  if (negate) { sc_neg(nk, k); memcpy(k, nk, 32); }
  ge p; mul_generator(p, k);
  Enc e; ristretto_encode(e.w, p);
  return e;
}

struct Solver {
  int bits;
  u32 slot_mask, max_probe;
  SlotsArr slots;
  ge_niels step, gstep;
  explicit Solver(int baby_bits) : bits(baby_bits) {
    const u32 entries = 1u << bits, n_slots = 2 * entries;
    slot_mask = n_slots - 1; max_probe = n_slots < DLOG_MAX_PROBE ? n_slots : DLOG_MAX_PROBE;
    slots.tab.assign(n_slots, 0);
    ge b4, t; ge_generator(t);
    ge_dbl_full(b4, t); ge_dbl_full(t, b4); b4 = t;
    ge_to_niels(step, b4);
    ge w = b4;
    for (int i = 0; i < bits; ++i) { ge_dbl_full(t, w); w = t; }
    ge_neg(t, w);
    ge_to_niels(gstep, t);
    RunArr io;
    for (u32 run = 0; run * DLOG_RUN < entries; ++run) dlog_baby_lane<TAG>(run, entries, g_tab, step, io, slots, slot_mask, max_probe);
    CHECK(slots.overflowed == 0, "baby table overflowed");
    CHECK(slots.ys.size() == entries, "entries inserted: %zu", slots.ys.size());
    size_t used = 0;
    for (u64 v : slots.tab) used += v != 0;
    CHECK(used == entries, "slots used: %zu", used);
  }
  // the answer of eg_dlog_solver_solve for one element: found, value
  bool solve(const Enc& e, u64 lo, u64 hi, u64* value) {
    static const u32 zero[8] = {0};
    *value = 0;
    if (memcmp(e.w, zero, 32) == 0) return true;
    egdlog::Range R;
    if (egdlog::plan_range(bits, 1, lo, hi, &R) != egdlog::RANGE_OK) { CHECK(false, "range refused"); return false; }
    ge p;
    if (!ristretto_decode(p, e.w)) return false;
    fe_carry(p.X); fe_carry(p.Y); fe_carry(p.T);        // as the prepared form (k_prim_points_prepare) holds it
    bool found = false;
    RunArr io;
    for (u64 r = 0; r < R.runs; ++r) {                  // every lane runs: a confirmed hit must not depend on stopping early
      const u64 j0 = r * DLOG_RUN;
      const int steps = (int)(R.steps - j0 < (u64)DLOG_RUN ? R.steps - j0 : (u64)DLOG_RUN);
      SinkVec sink;
      dlog_giant_lane<TAG>(0, p, lo, R.span, j0, steps, bits, g_tab, gstep, io, slots, slot_mask, max_probe, sink);
      ++g_lanes;
      for (auto& c : sink.c) {
        CHECK(c.second >= lo && c.second < hi && c.second != 0, "candidate %llu outside [%llu, %llu)", (unsigned long long)c.second, (unsigned long long)lo, (unsigned long long)hi);
        if (encode_multiple(c.second) == e) {
          CHECK(!found || *value == c.second, "two different confirmed values");
          found = true; *value = c.second;
        } else ++g_false_candidates;
      }
    }
    g_found += found;
    return found;
  }
};

static void expect_found(Solver& s, u64 m, u64 lo, u64 hi) {
  u64 v = 0;
  const bool f = s.solve(encode_multiple(m), lo, hi, &v);
  CHECK(f && v == m, "bits %d: %llu not found in [%llu, %llu) (found %d value %llu)", s.bits, (unsigned long long)m, (unsigned long long)lo, (unsigned long long)hi, (int)f, (unsigned long long)v);
}
static void expect_absent(Solver& s, const Enc& e, u64 lo, u64 hi, const char* what) {
  u64 v = 0;
  const bool f = s.solve(e, lo, hi, &v);
  CHECK(!f, "bits %d: %s found in [%llu, %llu) as %llu", s.bits, what, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)v);
}

int main(int argc, char** argv) {
  const bool quick = argc > 1 && strcmp(argv[1], "quick") == 0;
  // a point with no small logarithm: [2^100 + 12345]G
  Enc far;
  { u32 k[8] = {12345, 0, 0, 16, 0, 0, 0, 0}; ge p; mul_generator(p, k); ristretto_encode(far.w, p); }
  for (int bits : {4, 6}) {
    Solver s(bits);
    if (bits == 6) {                                    // the keys, for the comparison with y([4 i]B) in Python integers
      for (auto& kv : s.slots.ys) {
        u32 w[8]; fe_to_words(w, kv.second);
        printf("KEY %u ", kv.first);
        for (int i = 7; i >= 0; --i) printf("%08x", w[i]);
        printf("\n");
      }
    }
    const u64 spans[] = {1, 2, 15, 16, 17, 63, 64, 65, 600};
    for (u64 lo : {(u64)0, (u64)1, (u64)37}) {
      for (u64 span : spans) {
        if (quick && span > 65) continue;
        const u64 hi = lo + span;
        for (u64 m = lo; m < hi; ++m) {
          if (m == 0) { u64 v = 1; Enc z; memset(z.w, 0, 32); CHECK(s.solve(z, lo, hi, &v) && v == 0, "identity"); continue; }
          expect_found(s, m, lo, hi);
        }
        if (lo > 1) expect_absent(s, encode_multiple(lo - 1), lo, hi, "lo - 1");
        expect_absent(s, encode_multiple(hi), lo, hi, "hi");
        expect_absent(s, encode_multiple(hi + 1), lo, hi, "hi + 1");
        expect_absent(s, encode_multiple(lo + span / 2 + 1, true), lo, hi, "a negated multiple");
        expect_absent(s, far, lo, hi, "a point with no small logarithm");
      }
      // the identity is 0 whatever the range, and an empty range holds nothing else
      { u64 v = 1; Enc z; memset(z.w, 0, 32); CHECK(s.solve(z, lo + 5, lo + 9, &v) && v == 0, "identity with lo > 0"); }
      expect_absent(s, encode_multiple(lo + 1), lo + 1, lo + 1, "a value in an empty range");
    }
    // more than one run per element: full runs, a run seam, the clipped last run (the longest chain the classes are asserted over)
    {
      const u64 lo = 1000003, W = 1ull << bits, span = W * (2 * DLOG_RUN + 5) - 3, hi = lo + span;
      for (u64 m : {lo, lo + 1, lo + W * DLOG_RUN - 1, lo + W * DLOG_RUN, lo + W * DLOG_RUN + 1, lo + 2 * W * DLOG_RUN - 1, lo + 2 * W * DLOG_RUN, hi - 1})
        expect_found(s, m, lo, hi);
      expect_absent(s, encode_multiple(hi), lo, hi, "hi past the last run");
      expect_absent(s, encode_multiple(lo - 1), lo, hi, "lo - 1 before the first run");
    }
    // the top of the 64-bit range: nothing wraps
    {
      const u64 hi = ~0ull, lo = hi - 200;
      for (u64 m : {lo, lo + 1, hi - 2, hi - 1}) expect_found(s, m, lo, hi);
      expect_absent(s, encode_multiple(hi), lo, hi, "2^64 - 1 = hi");
      expect_absent(s, encode_multiple(lo - 1), lo, hi, "lo - 1 at the top");
      expect_found(s, hi - 1, hi - 1, hi);
      expect_absent(s, encode_multiple(hi - 1), hi, hi, "a value in the empty range at the top");
    }
  }
  CHECK(g_false_candidates > 0, "4-bit tags produced no false candidate");
  printf("lanes %llu found %llu false_candidates %llu fe_mul %llu fe_sq %llu\n", g_lanes, g_found, g_false_candidates, g_fe_mul_count, g_fe_sq_count);
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
