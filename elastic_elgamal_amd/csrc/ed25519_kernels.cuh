// ed25519_kernels.cuh -- Ed25519 signature checking of a batch, one lane per signature (eg_ed25519_*, eg_sha512_*: eg_hip.hip).  The rule,
// the codec and the lane functions are in ed25519.cuh; the argument rules and the scratch layout in ed25519_host.hpp.
//
// TWO kernels, with h parked in the caller's scratch (32 bytes an item):
//   k_ed25519_hash     h = SHA-512(R || A || prefix || msg) mod l.  Bytes in, 64-bit logic: sixteen schedule words, eight state words and
//                      the byte loads of a block in flight are 168 VGPR, so it runs at three waves per SIMD while it waits on uncoalesced
//                      byte loads, instead of the two of the curve kernel (192 VGPR) that a fused kernel would have.  Lanes that fail
//                      before the hash matters (a status word handed in, a roster index out of range, S >= l) hash nothing.
//   k_ed25519_verify   the rest of the rule: decode A, the small-order check, the per-lane radix-16 table of -A in the scratch, one chain of
//                      252 doublings for [h](-A), [S]B through the generator's comb, ed_encode, the compare.  A grid-stride loop: the tables
//                      are sized by the grid, not by n.
// The signer (k_ed25519_keypair, k_ed25519_sign) and k_sha512 make test and benchmark items; the signer keeps its hash inputs in private
// memory (R || A and the hash prefix come out of registers and go into the byte reader).  No kernel spills; the hash kernels keep the
// pointers and lengths of their ranges in a small stack array (DESIGN.md section 6f has the figures).
// Everything is variable time (ed25519.cuh, TIMING).
#pragma once
#include "device_io.cuh"
#include "ed25519.cuh"
#include "ed25519_host.hpp"

namespace eg {

static_assert(eged::NT == NT && eged::TABLE_BYTES == WS_QUADS * sizeof(uint4), "ed25519_host.hpp mirrors device_io.cuh");

struct EdItems {
  const unsigned char* msgs;      // item b: msg_len bytes at msgs + b * msg_stride
  size_t msg_stride, msg_len;
  const unsigned char* prefix;    // device copy, prefix_len bytes
  size_t prefix_len;
};
struct EdRoster {
  const u32* keys;                // n_keys x 8 words
  size_t n_keys;
  const u32* key_index;           // n words or null (item b uses key b)
};
__device__ __forceinline__ void ed_ld8(u32 w[8], const u32* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
}

__global__ void __launch_bounds__(NT) k_ed25519_hash(size_t n, EdItems it, EdRoster ro, const u32* sigs, const u32* status_in, u32* h_out) {
  const size_t b = (size_t)blockIdx.x * NT + threadIdx.x;
  if (b >= n) return;
  if (status_in && status_in[b]) return;
  const size_t k = ro.key_index ? (size_t)ro.key_index[b] : b;
  if (k >= ro.n_keys) return;
  u32 Sw[8]; ed_ld8(Sw, sigs + b * 16 + 8);
  if (!sc_is_canonical(Sw)) return;
  u32 h[8];
  ed_hash_mod_l(h, sha_ranges(reinterpret_cast<const unsigned char*>(sigs + b * 16), 32, reinterpret_cast<const unsigned char*>(ro.keys + k * 8), 32,
                              it.prefix, it.prefix_len, it.msgs + b * it.msg_stride, it.msg_len));
#pragma unroll
  for (int i = 0; i < 8; ++i) h_out[b * 8 + i] = h[i];
}

__global__ void __launch_bounds__(NT, 2) k_ed25519_verify(size_t n, EdRoster ro, const u32* sigs, const u32* h_in, const u32* status_in,
                                                          u32* status_out, const uint4* tabG, uint4* ws) {
  WsTable tab; tab.init(ws);
  const FixedTable tg(tabG);
  for (size_t b = (size_t)blockIdx.x * NT + threadIdx.x; b < n; b += (size_t)gridDim.x * NT) {
    const u32 st = status_in ? status_in[b] : 0u;
    if (st) { status_out[b] = st; continue; }
    const size_t k = ro.key_index ? (size_t)ro.key_index[b] : b;
    if (k >= ro.n_keys) { status_out[b] = ed_status(ED_BAD_INDEX); continue; }
    u32 Rw[8], Sw[8], Aw[8], hw[8];
    ed_ld8(Rw, sigs + b * 16); ed_ld8(Sw, sigs + b * 16 + 8); ed_ld8(Aw, ro.keys + k * 8);
    if (sc_is_canonical(Sw)) ed_ld8(hw, h_in + b * 8);          // parked only for lanes that hashed
    else {
#pragma unroll
      for (int i = 0; i < 8; ++i) hw[i] = 0;
    }
    status_out[b] = ed_status(ed_verify_lane(tab, tg, Rw, Sw, Aw, hw));
  }
}

__global__ void __launch_bounds__(NT, 2) k_ed25519_keypair(size_t n, const unsigned char* seeds, const uint4* tabG, u32* keys_out) {
  const size_t b = (size_t)blockIdx.x * NT + threadIdx.x;
  if (b >= n) return;
  const FixedTable tg(tabG);
  u32 Aw[8];
  ed_keypair_lane(Aw, tg, seeds + b * 32);
#pragma unroll
  for (int i = 0; i < 8; ++i) keys_out[b * 8 + i] = Aw[i];
}
__global__ void __launch_bounds__(NT, 2) k_ed25519_sign(size_t n, const unsigned char* seeds, EdItems it, const uint4* tabG, u32* sigs_out) {
  const size_t b = (size_t)blockIdx.x * NT + threadIdx.x;
  if (b >= n) return;
  const FixedTable tg(tabG);
  u32 sig[16];
  ed_sign_lane(sig, tg, seeds + b * 32, it.prefix, it.prefix_len, it.msgs + b * it.msg_stride, it.msg_len);
#pragma unroll
  for (int i = 0; i < 16; ++i) sigs_out[b * 16 + i] = sig[i];
}
__global__ void __launch_bounds__(NT) k_sha512(size_t n, EdItems it, u32* out) {
  const size_t b = (size_t)blockIdx.x * NT + threadIdx.x;
  if (b >= n) return;
  u32 dg[16];
  sha512_ranges(dg, sha_ranges(it.prefix, it.prefix_len, it.msgs + b * it.msg_stride, it.msg_len));
#pragma unroll
  for (int i = 0; i < 16; ++i) out[b * 16 + i] = dg[i];
}

}  // namespace eg
