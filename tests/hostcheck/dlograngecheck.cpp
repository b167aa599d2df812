// The pure-host range arithmetic of the discrete-log solver (elastic_elgamal_amd/csrc/dlog_host.hpp) at the corners of the 64-bit
// range.  Stand-alone program, built with -fsanitize=address,undefined by tests/test_dlog_solver_cpu.py: exit code 0 and "PASS" = every
// check held and no sanitizer finding.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../elastic_elgamal_amd/csrc/dlog_host.hpp"

using namespace egdlog;

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// the launches of a call as eg_dlog_solver_solve cuts them: every (element, run) exactly once, no launch above LAUNCH_LANES lanes
static void check_cuts(size_t n, uint64_t runs) {
  std::vector<unsigned char> seen((size_t)(n * runs), 0);
  const size_t eb = block_elems(n);
  for (size_t e0 = 0; e0 < n; e0 += eb) {
    const size_t ne = eb < n - e0 ? eb : n - e0;
    const uint64_t per = launch_runs(ne);
    for (uint64_t r0 = 0; r0 < runs; r0 += per) {
      const uint64_t nr = per < runs - r0 ? per : runs - r0;
      CHECK(ne * nr <= LAUNCH_LANES && ne * nr > 0, "launch of %zu x %llu lanes", ne, (unsigned long long)nr);
      for (size_t e = 0; e < ne; ++e)
        for (uint64_t r = 0; r < nr; ++r) ++seen[(size_t)((e0 + e) * runs + r0 + r)];
    }
  }
  for (unsigned char s : seen) CHECK(s == 1, "a lane is covered %d times (n %zu runs %llu)", (int)s, n, (unsigned long long)runs);
}

int main() {
  const uint64_t top = ~0ull;
  for (int bits = BABY_BITS_MIN; bits <= BABY_BITS_MAX; ++bits) {
    const uint64_t W = 1ull << bits;
    Range r;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)4000, (size_t)LAUNCH_LANES + 3}) {
      const uint64_t ms = max_span(bits, n);
      CHECK(ms >= W && ms <= SPAN_LIMIT, "max_span %llu", (unsigned long long)ms);
      CHECK(max_span(bits, n) <= max_span(bits, n ? n - 1 : 0) || n == 0, "max_span grows with n");
      // lo == hi: the empty range, anywhere
      for (uint64_t at : {(uint64_t)0, (uint64_t)1, top - 1, top}) {
        CHECK(plan_range(bits, n, at, at, &r) == RANGE_OK && r.span == 0 && r.steps == 0 && r.runs == 0, "empty range at %llu", (unsigned long long)at);
      }
      // span 1, at the bottom and at the top (hi = 2^64 - 1, lo = 2^64 - 2)
      CHECK(plan_range(bits, n, 0, 1, &r) == RANGE_OK && r.span == 1 && r.steps == 1 && r.runs == 1, "span 1");
      CHECK(plan_range(bits, n, top - 1, top, &r) == RANGE_OK && r.span == 1 && r.steps == 1 && r.runs == 1, "span 1 at the top");
      // reversed
      CHECK(plan_range(bits, n, 1, 0, &r) == RANGE_REVERSED && plan_range(bits, n, top, top - 1, &r) == RANGE_REVERSED && plan_range(bits, n, top, 0, &r) == RANGE_REVERSED, "reversed");
      // a span equal to max_span is taken, one above is refused - from 0 and ending at 2^64 - 1
      CHECK(plan_range(bits, n, 0, ms, &r) == RANGE_OK && r.span == ms, "span == max_span");
      CHECK(r.steps == ((ms - 1) >> bits) + 1 && r.runs == (r.steps + RUN - 1) / RUN, "steps of the widest call");
      CHECK(r.steps <= (SPAN_LIMIT >> bits) && (r.steps + RUN) <= (top >> bits), "(steps + RUN) W wraps");
      CHECK(plan_range(bits, n, 0, ms + 1, &r) == RANGE_TOO_WIDE, "span == max_span + 1");
      CHECK(plan_range(bits, n, top - ms, top, &r) == RANGE_OK && r.span == ms, "span == max_span at the top");
      CHECK(plan_range(bits, n, top - ms - 1, top, &r) == RANGE_TOO_WIDE, "span == max_span + 1 at the top");
      CHECK(plan_range(bits, n, 0, top, &r) == RANGE_TOO_WIDE, "the whole 64-bit range");
    }
    // steps and runs around the multiples of W and of RUN W
    for (uint64_t span : {W - 1, W, W + 1, RUN * W - 1, RUN * W, RUN * W + 1}) {
      CHECK(plan_range(bits, 1, 7, 7 + span, &r) == RANGE_OK, "plain range");
      CHECK(r.steps * W >= span && (r.steps - 1) * W < span, "steps cover the span exactly");
      CHECK(r.runs * RUN >= r.steps && (r.runs - 1) * RUN < r.steps, "runs cover the steps exactly");
    }
    // candidates: inside the span only, never 0, never wrapped
    uint64_t m = 0;
    CHECK(candidate_value(top - 200, 200, 0, 0, bits, &m) && m == top - 200, "first value at the top");
    CHECK(candidate_value(top - 200, 200, 0, 199, bits, &m) && m == top - 1, "last value at the top");
    CHECK(!candidate_value(top - 200, 200, 0, 200, bits, &m), "hi itself");
    CHECK(!candidate_value(top - 200, 200, 1, 0, bits, &m), "a step past the span at the top");
    CHECK(!candidate_value(0, 10, 0, 0, bits, &m), "zero is not a candidate");
    CHECK(candidate_value(0, W + 1, 1, 0, bits, &m) && m == W, "second giant step");
    CHECK(!candidate_value(5, W, 1, 0, bits, &m), "lo + W = hi");
    CHECK(candidate_value(5, W, 0, (uint32_t)(W - 1), bits, &m) && m == 5 + W - 1, "hi - 1");
  }
  check_cuts(0, 0); check_cuts(0, 5); check_cuts(1, 0);
  check_cuts(1, 1); check_cuts(1, 3 * LAUNCH_LANES + 7); check_cuts(5, LAUNCH_LANES); check_cuts(4000, 100);
  check_cuts(LAUNCH_LANES, 3); check_cuts(LAUNCH_LANES + 1, 2); check_cuts(3 * LAUNCH_LANES + 5, 1);
  CHECK(block_elems(0) == 0 && launch_runs(0) == LAUNCH_LANES && launch_runs(1) == LAUNCH_LANES && launch_runs(LAUNCH_LANES + 9) == 1, "cut sizes");
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
