// open_kernels.cuh -- the ballot-audit pass (eg_*_open_check*, eg_hip.hip): do the opened ballots of a pile encrypt what their openings say.
// The reference's proofs show that a ballot encrypts SOME admissible value; a voting device that encrypts option 2 when the voter pressed
// option 4 passes all of them.  Helios and ElectionGuard answer with the Benaloh challenge: before casting, the voter may have the device
// open the ballot - reveal the value v and the randomness r of every ciphertext -, anyone re-encrypts and compares, and the opened ballot
// is spoiled.  Boards publish the openings in bulk; this pass re-checks them.
//
// Audited piles are small beside a cast batch, so the parallelism comes from the ciphertexts:
//   k_open_check       one lane = one (ballot, slot) of a participating ballot: r < l, then P_R = [r/2]G and P_B = [v/2]G + [r/2]K over the
//                      narrow comb tables (halved scalars as in every equation of the engine: the encoder doubles), both through
//                      ge_double_encode_prepare, ONE fe_invert for the two N (Montgomery: one multiplication in, two out), both through
//                      ge_double_encode_finish, the byte compare against the 64 wire bytes; one verdict word into the scratch.  Nothing
//                      of the ballot is decoded.  No atomics, no lane waits on another.
//   k_open_resolve     one lane = one ballot, after the kernel boundary: the first non-zero word of its slots is its status; the two
//                      counters take one atomic per wavefront.
// The verdict is a pure function of the inputs.  The lane bodies are plain functions over their memory, so that the host check build
// (tests/hostcheck/opencheck.cpp) runs the same code serially on arrays.
#pragma once
#include "ge25519.cuh"
#include "sc25519.cuh"
#include "open_host.hpp"

namespace ego {

using eg::u32;
using eg::u64;

// The same point again, as far as the optimiser can tell another one.  prepare and finish both start with the doubling of P; inlined into
// one lane the compiler keeps the doubling's four intermediates of BOTH points alive across the inversion instead of the points alone,
// and the lane spills (96 VGPRs at two waves per SIMD).  Recomputing them, as k_encode_batch does, is 4 squarings a point.
EG_HD void open_forget(eg::ge& p) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < EG_NL; ++i) asm volatile("" : "+v"(p.X.v[i]), "+v"(p.Y.v[i]), "+v"(p.Z.v[i]), "+v"(p.T.v[i]));
#else
  (void)p;
#endif
}

// out_r = encode(2 pr), out_b = encode(2 pb) with one inversion between them
EG_HD void open_encode_pair(u32 out_r[8], u32 out_b[8], eg::ge& pr, eg::ge& pb) {
  eg::fe nr, nb, prod, inv, ir, ib;
  bool zr, zb;
  eg::ge_double_encode_prepare(nr, zr, pr);
  eg::ge_double_encode_prepare(nb, zb, pb);
  open_forget(pr);
  open_forget(pb);
  eg::fe_mul(prod, nr, nb);                    // neither is 0: prepare puts 1 in place of a zero N
  eg::fe_invert(inv, prod);
  eg::fe_mul(ir, inv, nb);
  eg::fe_mul(ib, inv, nr);
  eg::ge_double_encode_finish(out_r, pr, ir, zr);
  eg::ge_double_encode_finish(out_b, pb, ib, zb);
}

// Mem: rand(w, i) the eight words of r of item i = b n_slots + t, value(i), wire(w, b, t) the sixteen words R || B of slot t of ballot b.
// TabG, TabK: the comb tables (ge_fixed_mul_add).  Returns 0 or the check that failed (OPEN_*).  RANGE_CHECK = false exists for the host
// check alone, to show that check 1 is the only guard against r + l.
template <bool RANGE_CHECK = true, class Mem, class TabG, class TabK>
EG_HD u32 open_lane_check(const Mem& m, const TabG& tg, const TabK& tk, u64 b, u32 t, u32 n_slots, u32* enc_out = nullptr) {
  const u64 i = b * n_slots + t;
  u32 r[8], h[8], d[EG_COMB_WORDS];
  m.rand(r, i);
  if (RANGE_CHECK && !eg::sc_is_canonical(r)) return OPEN_BAD_SCALAR;
  eg::ge pr, pb;
  eg::sc_halve(h, r);
  eg::sc_recode_comb(d, h);
  eg::ge_identity(pr);
  eg::ge_fixed_mul_add(pr, tg, d);
  eg::ge_identity(pb);
  eg::ge_fixed_mul_add(pb, tk, d);
  eg::sc_from_u64(r, m.value(i));
  eg::sc_halve(h, r);
  eg::sc_recode_comb(d, h);
  eg::ge_fixed_mul_add(pb, tg, d);
  u32 enc[16], wire[16];
  open_encode_pair(enc, enc + 8, pr, pb);
  if (enc_out)
    for (int w = 0; w < 16; ++w) enc_out[w] = enc[w];
  m.wire(wire, b, t);
  u32 dr = 0, db = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) { dr |= enc[w] ^ wire[w]; db |= enc[8 + w] ^ wire[8 + w]; }
  return dr ? OPEN_R : db ? OPEN_B : 0u;
}
EG_HD u32 open_lane_word(u32 t, u32 check) { return check ? status_word(t, check) : 0u; }

// Mem: word(i) the verdict word of item i.  `st` is status_in[b] (0 without one); nothing of a ballot that does not participate is read
template <class Mem>
EG_HD u32 open_lane_resolve(const Mem& m, u64 b, u32 n_slots, u32 st, bool part, bool& failed) {
  failed = false;
  if (!part) return st;
  for (u32 t = 0; t < n_slots; ++t) {
    const u32 w = m.word(b * n_slots + t);
    if (w) { failed = true; return w; }
  }
  return 0u;
}

}  // namespace ego

#if defined(__HIPCC__)
#include "device_io.cuh"

namespace eg {

struct OpenMemDev {
  const uint8_t* ballots;
  const u32* items;                          // the plan's tally items: slot t is the 64 bytes at item items[2 t]
  u64 stride;
  const unsigned long long* values;
  const u32* rand_;
  const u32* words;
  __device__ __forceinline__ void rand(u32 w[8], u64 i) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = rand_[i * 8 + k];
  }
  __device__ __forceinline__ u64 value(u64 i) const { return values[i]; }
  __device__ __forceinline__ void wire(u32 w[16], u64 b, u32 t) const {
    const uint4* p = reinterpret_cast<const uint4*>(ballots + b * stride + (u64)items[2u * t] * 32u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = p[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
  __device__ __forceinline__ u32 word(u64 i) const { return words[i]; }
};

// lanes: the n x n_slots ciphertexts; a lane whose ballot does not participate leaves at once and writes nothing
__global__ void __launch_bounds__(NT, 2) k_open_check(OpenMemDev mem, const u32* status, u64 n, u32 n_slots, const uint4* tabG, const uint4* tabK,
                                                      u32* words) {
  const u64 i = (u64)blockIdx.x * NT + threadIdx.x;
  if (i >= n * n_slots) return;
  const u64 b = i / n_slots;
  const u32 t = (u32)(i - b * n_slots);
  if (status && status[b] != 0u) return;
  const FixedTable tg(tabG), tk(tabK);
  words[i] = ego::open_lane_word(t, ego::open_lane_check(mem, tg, tk, b, t, n_slots));
}
// whole blocks: every lane stays for the wave-level atomics.  status_out may be status: lane b alone reads and writes word b
__global__ void __launch_bounds__(NT) k_open_resolve(OpenMemDev mem, const u32* status, u64 n, u32 n_slots, u32* status_out, u32* found) {
  const u64 b = (u64)blockIdx.x * NT + threadIdx.x;
  const bool live = b < n;
  const u32 st = live && status ? status[b] : 0u;
  const bool part = live && st == 0u;
  bool failed;
  const u32 out = ego::open_lane_resolve(mem, b, n_slots, st, part, failed);
  if (live) status_out[b] = out;
  const unsigned long long mp = __ballot(part), mf = __ballot(failed);
  const int lane = threadIdx.x & 63;
  if (mp && lane == __ffsll((long long)mp) - 1) atomicAdd(found, (u32)__popcll(mp));
  if (mf && lane == __ffsll((long long)mf) - 1) atomicAdd(found + 1, (u32)__popcll(mf));
}

}  // namespace eg
#endif
