// open_gen_kernels.cuh -- the OPENER of synthetic ballots (eg_*_open_batch*, eg_hip.hip), beside the provers it mirrors: the values and the
// encryption randomness of the ballots that k_choice_encrypt / k_qv_encrypt make from the same arguments, so that tests and benchmarks
// have openings to audit (open_kernels.cuh).  One lane = one ballot; no point is multiplied: one ChaCha block and one sc_from_wide per
// slot, at the position where the generator drew it (open_host.hpp: choice_r_draw, qv_r_draw).  VARIABLE TIME like the provers: a real
// voting device opens its ballots on its own CPU.
// The voter's choice, where the caller gives none, comes from the second stream ~seed exactly as in the provers; the values array itself
// is the lane's memory of it.
#pragma once
#include "prover_kernels.cuh"
#include "open_host.hpp"

namespace eg {

struct OpenSecondStream {
  ChaChaRng sel;
  u32 buf[16];
  int pos;
  __device__ __forceinline__ explicit OpenSecondStream(u64 seed) : pos(16) { chacha_seed_from_u64(sel, ~seed); }
  __device__ __forceinline__ u32 next() {
    if (pos >= 16) { chacha_block(sel, buf); pos = 0; }
    u32 v = buf[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) v = (pos == q) ? buf[q] : v;
    ++pos;
    return v;
  }
};
__device__ __forceinline__ void open_put_rand(u32* rand, size_t item, ChaChaRng& rng, u64 draw) {
  u32 r[8];
  rng.counter = draw;
  rng_scalar(rng, r);
#pragma unroll
  for (int w = 0; w < 8; ++w) rand[item * 8 + w] = r[w];
}

// values: n x n_options uint64 (1 = chosen), rand: n x n_options x 8 words
__global__ void __launch_bounds__(NT) k_choice_open(u64 seed0, size_t n, int n_options, int single, int n_selected, const u32* selection,
                                                    u64 rng_skip, unsigned long long* values, u32* rand) {
  const u32 SW = (u32)((n_options + 31) / 32);
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const u64 seed = seed0 + i;
    unsigned long long* vo = values + i * (size_t)n_options;
    if (selection) {
      for (int k = 0; k < n_options; ++k) vo[k] = (selection[i * SW + ((u32)k >> 5)] >> (k & 31)) & 1u;
    } else {
      for (int k = 0; k < n_options; ++k) vo[k] = 0u;
      OpenSecondStream s2(seed);
      const int want = single ? 1 : n_selected;
      int got = 0;
#pragma unroll 1
      while (got < want) {
        const u32 k = s2.next() % (u32)n_options;
        if (!vo[k]) { vo[k] = 1u; ++got; }
      }
    }
    ChaChaRng rng;
    chacha_seed_from_u64(rng, seed);
    u32 skipped = 0;
#pragma unroll 1
    for (int k = 0; k < n_options; ++k) {
      open_put_rand(rand, i * (size_t)n_options + k, rng, ego::choice_r_draw(rng_skip, (u32)k, skipped));
      if (!vo[k]) ++skipped;
    }
  }
}

// values: n x n_options uint64 (the votes), rand as above; draws_per_vote = ego::range_draws of the vote range
__global__ void __launch_bounds__(NT) k_qv_open(u64 seed0, size_t n, int n_options, u64 credits, const u32* votes_in, u64 rng_skip,
                                                u64 draws_per_vote, unsigned long long* values, u32* rand) {
  const u32 NO = (u32)n_options;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const u64 seed = seed0 + i;
    unsigned long long* vo = values + i * (size_t)n_options;
    for (u32 k = 0; k < NO; ++k) vo[k] = votes_in ? votes_in[i * (size_t)n_options + k] : 0u;
    if (!votes_in) {      // as k_qv_encrypt: geometric, p = 0.8, from the second stream
      OpenSecondStream s2(seed);
#pragma unroll 1
      for (;;) {
        if (s2.next() % 10u >= 8u) break;
        const u32 k = s2.next() % NO;
        u64 c = 0;
        for (u32 j = 0; j < NO; ++j) { const u64 v = vo[j] + (j == k ? 1 : 0); c += v * v; }
        if (c > credits) break;
        vo[k] += 1u;
      }
    }
    ChaChaRng rng;
    chacha_seed_from_u64(rng, seed);
#pragma unroll 1
    for (u32 k = 0; k < NO; ++k) open_put_rand(rand, i * (size_t)n_options + k, rng, ego::qv_r_draw(rng_skip, k, draws_per_vote));
  }
}

}  // namespace eg
