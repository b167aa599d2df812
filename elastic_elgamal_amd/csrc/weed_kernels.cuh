// weed_kernels.cuh -- ballot weeding (eg_*_weed*, eg_hip.hip): which accepted ballots of a verified batch carry a tally ciphertext that
// is already on the bulletin board or in an earlier ballot of the batch.  The reference binds nothing of the voter into its transcripts
// (Transcript::new(b"encrypted_choice_ranges"), src/app/choice.rs:323), so a byte-for-byte copy of somebody's ballot verifies; a host
// drops such replays before it tallies (Cortier and Smyth, "Attacking and fixing Helios").
//
// The pass runs AFTER a verify entry, over the wire bytes that are still in device memory, and reads nothing of the engine but the plan's
// immutable tally items.  A KEY is the 64 wire bytes R || B of one tally ciphertext; equality is byte equality (accepted ballots have
// canonical encodings).  weed_host.hpp has the references and the layout:
//   k_weed_insert      one lane = one key of the board or of a participating ballot: hash the 64 bytes with the caller's secret seed,
//                      probe linearly; an empty slot is claimed by a 64-bit compare-and-swap; an occupied one is compared through the
//                      occupant's reference (the input buffers, read-only for the whole call) and, on equal bytes, lowered to the smaller
//                      reference.  A slot only ever changes between references to EQUAL bytes, so the compare needs no ordering; the
//                      probe loop is bounded by the number of slots and counts into found[2] instead of spinning.
//   k_weed_lookup      one lane = one ballot, after the kernel boundary (the only synchronisation: no flags, no waiting between
//                      workgroups): the owner of each of its keys is the key's smallest reference - a board entry, an earlier ballot,
//                      or the ballot itself; dup_of, status_out, the keep flag and the counters (one atomic per wavefront) follow.
//   k_weed_scan_*      exclusive prefix sum of the keep flags in ballot order (tiles of 1024, tops, apply), the fit check on its total
//   k_weed_copy        one lane = 16 bytes of a kept key -> the board, behind the first n_prior entries
// The verdict is the minimum over references, a pure function of the inputs: it depends neither on the seed nor on the order of the lanes.
// The lane bodies are plain functions over their memory, so that the host check build (tests/hostcheck/weedcheck.cpp) runs the same code
// serially, in any lane order, on arrays.
#pragma once
#include "weed_host.hpp"

namespace egw {

// seeded 64-bit mix of the eight 64-bit words of a key: two multiply / xor-shift rounds per word
EGW_HD uint64_t weed_hash(const uint32_t w[16], uint64_t seed) {
  uint64_t h = seed ^ 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    h = (h ^ x) * 0xff51afd7ed558ccdull;
    h ^= h >> 29;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 32;
  }
  return h;
}
EGW_HD bool weed_same(const uint32_t a[16], const uint32_t b[16]) {
  uint32_t d = 0;
  for (int i = 0; i < 16; ++i) d |= a[i] ^ b[i];
  return d == 0u;
}

// Table: peek(i) the slot's value now or a moment ago, claim(i, ref) = compare-and-swap from EMPTY returning what was there,
// lower(i, ref) = atomic minimum.  Keys: load(w, ref) the 16 words behind a reference.
// false: `slots` probes found neither an empty slot nor the key (the table is too small)
template <class Table, class Keys>
EGW_HD bool weed_lane_insert(Table& tab, const Keys& keys, uint64_t slots, uint64_t seed, uint64_t ref) {
  uint32_t mine[16], other[16];
  keys.load(mine, ref);
  uint64_t i = weed_hash(mine, seed) & (slots - 1);
  for (uint64_t probes = 0; probes < slots; ++probes, i = (i + 1) & (slots - 1)) {
    uint64_t v = tab.peek(i);
    if (v == EMPTY) {
      v = tab.claim(i, ref);
      if (v == EMPTY) return true;
    }
    keys.load(other, v);
    if (weed_same(mine, other)) {
      if (ref < v) tab.lower(i, ref);        // a value read earlier only over-estimates the slot: skipping is then exact
      return true;
    }
  }
  return false;
}
// the smallest reference to the bytes of `ref` (EMPTY: the key is not in the table - only after an overflow)
template <class Table, class Keys>
EGW_HD uint64_t weed_lane_owner(const Table& tab, const Keys& keys, uint64_t slots, uint64_t seed, uint64_t ref) {
  uint32_t mine[16], other[16];
  keys.load(mine, ref);
  uint64_t i = weed_hash(mine, seed) & (slots - 1);
  for (uint64_t probes = 0; probes < slots; ++probes, i = (i + 1) & (slots - 1)) {
    const uint64_t v = tab.peek(i);
    if (v == EMPTY || v == ref) return v;
    keys.load(other, v);
    if (weed_same(mine, other)) return v;
  }
  return EMPTY;
}
// dup_of of participating ballot b: EG_DUP_PRIOR if any key is owned by the board, else the smallest earlier ballot that owns one of
// its keys (a key it owns itself - also one it carries twice - says nothing), else EG_DUP_NONE
template <class Table, class Keys>
EGW_HD uint32_t weed_lane_ballot(const Table& tab, const Keys& keys, uint64_t slots, uint64_t seed, uint64_t b, uint32_t keys_per_ballot,
                                 bool& missing) {
  uint32_t dup = DUP_NONE;
  for (uint32_t k = 0; k < keys_per_ballot; ++k) {
    const uint64_t owner = weed_lane_owner(tab, keys, slots, seed, batch_ref(b, keys_per_ballot, k));
    if (owner == EMPTY) { missing = true; continue; }
    if (is_board_ref(owner)) { dup = DUP_PRIOR; continue; }
    const uint64_t ob = ref_ballot(owner, keys_per_ballot);
    if (ob < b && dup != DUP_PRIOR && (uint32_t)ob < dup) dup = (uint32_t)ob;
  }
  return dup;
}
EGW_HD uint32_t weed_status_out(uint32_t status, uint32_t dup) { return dup != DUP_NONE ? ST_DUPLICATE : status; }

// where quarter q (16 bytes) of key k of a kept ballot goes: board entry n_prior + rank K + k
EGW_HD uint64_t weed_append_entry(uint64_t n_prior, uint32_t rank, uint32_t keys_per_ballot, uint32_t k) {
  return n_prior + (uint64_t)rank * keys_per_ballot + k;
}
// what the scan kernels compute, serially: pos[b] = the rank of ballot b among the kept ones (0xffffffff: not kept); returns their number
inline uint32_t scan_keep(std::vector<uint32_t>& pos) {
  uint32_t run = 0;
  for (uint32_t& p : pos) p = p ? run++ : 0xffffffffu;
  return run;
}
EGW_HD bool append_fits(uint64_t n_prior, uint32_t kept, uint32_t keys_per_ballot, uint64_t board_cap) {
  return n_prior + (uint64_t)kept * keys_per_ballot <= board_cap;
}

}  // namespace egw

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "scan.cuh"

namespace eg {

constexpr int WEED_NT = 256;
static_assert(WEED_NT == SCAN_NT, "the scan kernels are launched with WEED_NT lanes");

struct WeedTableDev {
  unsigned long long* slots;
  __device__ __forceinline__ uint64_t peek(uint64_t i) const { return __hip_atomic_load(slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint64_t claim(uint64_t i, uint64_t ref) { return atomicCAS(slots + i, (unsigned long long)egw::EMPTY, (unsigned long long)ref); }
  __device__ __forceinline__ void lower(uint64_t i, uint64_t ref) { (void)atomicMin(slots + i, (unsigned long long)ref); }
};
struct WeedTableRead {                      // after the kernel boundary: plain loads
  const unsigned long long* slots;
  __device__ __forceinline__ uint64_t peek(uint64_t i) const { return slots[i]; }
};
struct WeedKeysDev {
  const uint8_t* ballots;
  const uint8_t* board;
  const uint32_t* items;                    // the plan's tally items: key k is items[2 k], items[2 k] + 1
  uint64_t stride, n, n_prior;
  uint32_t keys_per_ballot;
  __device__ __forceinline__ const uint4* at(uint64_t ref) const {
    if (egw::is_board_ref(ref)) return ref < n_prior ? reinterpret_cast<const uint4*>(board + ref * egw::KEY_BYTES) : nullptr;
    const uint64_t b = egw::ref_ballot(ref, keys_per_ballot);
    if (b >= n) return nullptr;             // references come from this call's own table: never, unless the scratch was written meanwhile
    return reinterpret_cast<const uint4*>(ballots + egw::key_offset(b, stride, items[2u * egw::ref_key(ref, keys_per_ballot)]));
  }
  __device__ __forceinline__ void load(uint32_t w[16], uint64_t ref) const {
    const uint4* p = at(ref);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = p ? p[q] : make_uint4(0u, 0u, 0u, 0u);
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
};
// *ctr += the lanes of the wavefront with `flag`, in one atomic (whole blocks only)
__device__ __forceinline__ void weed_wave_tally(uint32_t* ctr, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (uint32_t)__popcll(m));
}

// lanes: the n_prior board entries, then the n K keys of the batch; keys of ballots that do not participate are never read
__global__ void __launch_bounds__(WEED_NT) k_weed_insert(WeedKeysDev keys, const uint32_t* status, unsigned long long* slots, uint64_t n_slots,
                                                         uint64_t seed, uint32_t* found) {
  const uint64_t lanes = keys.n_prior + keys.n * keys.keys_per_ballot;
  WeedTableDev tab{slots};
  uint32_t over = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * WEED_NT + threadIdx.x; j < lanes; j += (uint64_t)gridDim.x * WEED_NT) {
    uint64_t ref = j;
    if (j >= keys.n_prior) {
      const uint64_t idx = j - keys.n_prior;
      if (status && status[idx / keys.keys_per_ballot] != 0u) continue;
      ref = egw::BATCH_BASE + idx;
    }
    if (!egw::weed_lane_insert(tab, keys, n_slots, seed, ref)) ++over;
  }
  if (over) atomicAdd(found + 2, over);
}
// whole blocks: every lane stays for the wave-level atomics.  status_out may be status: lane b alone reads and writes word b
__global__ void __launch_bounds__(WEED_NT) k_weed_lookup(WeedKeysDev keys, const uint32_t* status, const unsigned long long* slots,
                                                         uint64_t n_slots, uint64_t seed, uint32_t* dup_of, uint32_t* status_out, uint32_t* pos,
                                                         uint32_t* found) {
  const uint64_t b = (uint64_t)blockIdx.x * WEED_NT + threadIdx.x;
  const bool live = b < keys.n;
  const uint32_t st = live && status ? status[b] : 0u;
  const bool part = live && st == 0u;
  const WeedTableRead tab{slots};
  bool missing = false;
  const uint32_t dup = part ? egw::weed_lane_ballot(tab, keys, n_slots, seed, b, keys.keys_per_ballot, missing) : egw::DUP_NONE;
  if (live) {
    dup_of[b] = dup;
    if (status_out) status_out[b] = egw::weed_status_out(st, dup);
    pos[b] = part && dup == egw::DUP_NONE ? 1u : 0u;
  }
  weed_wave_tally(found, dup == egw::DUP_PRIOR);
  weed_wave_tally(found + 1, dup != egw::DUP_NONE && dup != egw::DUP_PRIOR);
  weed_wave_tally(found + 2, missing);
}

// ---- exclusive prefix sum of the keep flags (three launches: scan.cuh) --------------------------------------------------------------------
struct WeedKeepLoad {
  const uint32_t* pos; uint32_t n;
  __device__ __forceinline__ void operator()(uint32_t v[1], uint32_t i) const { v[0] = i < n ? pos[i] : 0u; }
};
__global__ void __launch_bounds__(WEED_NT) k_weed_scan_tiles(const uint32_t* pos, uint32_t n, uint32_t* tile_sums) {
  scan_tile_sums<1>(tile_sums, WeedKeepLoad{pos, n});
}
// one wavefront: tile sums -> exclusive prefix sums; the total, whether the kept keys fit the board, the new board count
__global__ void k_weed_scan_tops(uint32_t n_tiles, uint32_t* tile_sums, uint32_t keys_per_ballot, uint64_t n_prior, uint64_t board_cap,
                                 uint32_t* total_word, unsigned long long* board_count, uint32_t* found) {
  const uint32_t run = scan_tops<1>(n_tiles, tile_sums);
  if ((threadIdx.x & 63) == 0) {
    const bool fits = egw::append_fits(n_prior, run, keys_per_ballot, board_cap);
    if (total_word) { total_word[0] = run; total_word[1] = fits ? 1u : 0u; }
    *board_count = n_prior + (fits ? (uint64_t)run * keys_per_ballot : 0u);
    if (!fits) atomicAdd(found + 2, 1u);
  }
}
// pos[b]: keep flag -> rank among the kept ballots, 0xffffffff for the others
__global__ void __launch_bounds__(WEED_NT) k_weed_scan_apply(uint32_t* pos, uint32_t n, const uint32_t* tile_sums) {
  uint32_t v[SCAN_PER_LANE][1], run[1];
  scan_apply<1>(tile_sums, WeedKeepLoad{pos, n}, v, run);
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    const uint32_t i = scan_element(e);
    if (i < n) pos[i] = v[e][0] ? run[0] : 0xffffffffu;
    run[0] += v[e][0];
  }
}
// lanes: ballots x keys x 4 quarters of 16 bytes.  Nothing is written unless everything fits
__global__ void __launch_bounds__(WEED_NT) k_weed_copy(WeedKeysDev keys, const uint32_t* pos, const uint32_t* total_word, uint8_t* board,
                                                       uint64_t board_cap) {
  if (total_word[1] == 0u) return;
  const uint64_t per_ballot = 4ull * keys.keys_per_ballot, lanes = keys.n * per_ballot;
  for (uint64_t j = (uint64_t)blockIdx.x * WEED_NT + threadIdx.x; j < lanes; j += (uint64_t)gridDim.x * WEED_NT) {
    const uint64_t b = j / per_ballot;
    const uint32_t r = (uint32_t)(j % per_ballot), k = r >> 2, q = r & 3u;
    const uint32_t rank = pos[b];
    if (rank == 0xffffffffu) continue;
    const uint64_t entry = egw::weed_append_entry(keys.n_prior, rank, keys.keys_per_ballot, k);
    if (entry >= board_cap) continue;            // the fit check above says never
    const uint4* src = reinterpret_cast<const uint4*>(keys.ballots + egw::key_offset(b, keys.stride, keys.items[2u * k])) + q;
    reinterpret_cast<uint4*>(board + entry * egw::KEY_BYTES)[q] = *src;
  }
}

}  // namespace eg
#endif
