// dlog_host.hpp -- range arithmetic of the bounded discrete-log solver (eg_dlog_solver_*, eg_hip.hip): pure host code, no HIP.
// tests/hostcheck/dlograngecheck.cpp compiles it alone under ASan + UBSan and walks the corners of the 64-bit range.
//
// A call searches [lo, hi) for every element with giant steps of W = 2^baby_bits values.  Element e needs
// steps = ceil((hi - lo) / W) giant steps, walked in runs of RUN consecutive steps per lane (dlog_kernels.cuh: DLOG_RUN).  A call is
// cut into launches of at most LAUNCH_LANES lanes (blocks of elements x chunks of runs), so that no launch is long and the host can
// stop between two launches once every element is answered.
//
// The two caps (first measurement on an MI355X, profiles/r11_dlog_solver.txt; both are fixed from that file):
//   LAUNCH_LANES = 2^17 lanes of 64 steps = 2^23 giant steps per launch: two waves per SIMD on 256 CUs, about 1 ms a launch;
//   CALL_STEPS   = 2^36 giant steps per call: about eight seconds at the measured 8.9 x 10^9 giant steps per second.
// The default table has 2^24 entries: 256 MiB, built in 2 ms; 16 elements in a span of 2^48 take 30 ms with it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EGDLOG_HD __host__ __device__ inline
#else
#define EGDLOG_HD inline
#endif

namespace egdlog {

constexpr int RUN = 64;
constexpr int BABY_BITS_MIN = 8, BABY_BITS_MAX = 28, BABY_BITS_DEFAULT = 24;
constexpr uint64_t LAUNCH_LANES = 1ull << 17;
constexpr uint64_t CALL_STEPS = 1ull << 36;
constexpr uint64_t SPAN_LIMIT = 1ull << 62;      // (steps + RUN) * W stays far below 2^64 in the kernels

// widest hi - lo that a call with n elements accepts
inline uint64_t max_span(int baby_bits, size_t n) {
  uint64_t per = CALL_STEPS / (n ? (uint64_t)n : 1ull);
  if (per == 0) per = 1;
  if (per > (SPAN_LIMIT >> baby_bits)) return SPAN_LIMIT;
  return per << baby_bits;
}

enum { RANGE_OK = 0, RANGE_REVERSED = 1, RANGE_TOO_WIDE = 2 };
struct Range {
  uint64_t span = 0;       // hi - lo
  uint64_t steps = 0;      // giant steps per element
  uint64_t runs = 0;       // lanes per element
};
inline int plan_range(int baby_bits, size_t n, uint64_t lo, uint64_t hi, Range* r) {
  if (lo > hi) return RANGE_REVERSED;
  r->span = hi - lo;
  if (r->span > max_span(baby_bits, n)) return RANGE_TOO_WIDE;
  r->steps = r->span ? ((r->span - 1) >> baby_bits) + 1 : 0;
  r->runs = (r->steps + RUN - 1) / RUN;
  return RANGE_OK;
}

// elements per block and runs per launch: elems * runs <= LAUNCH_LANES
inline size_t block_elems(size_t n) { return n < LAUNCH_LANES ? n : (size_t)LAUNCH_LANES; }
inline uint64_t launch_runs(size_t elems) { const uint64_t r = LAUNCH_LANES / (elems ? elems : 1); return r ? r : 1; }

// the value that giant step j and baby entry i stand for, if it lies in the range: lo + j W + i without wrapping
EGDLOG_HD bool candidate_value(uint64_t lo, uint64_t span, uint64_t j, uint32_t i, int baby_bits, uint64_t* m) {
  const uint64_t off = (j << baby_bits) + i;
  if (off >= span) return false;
  *m = lo + off;           // < hi: no wrap
  return *m != 0;
}

}  // namespace egdlog
