// weed_index_kernels.cuh -- ballot weeding against a persistent board index (eg_weed_index_*, eg_*_weed_indexed*, eg_hip.hip).
// weed_kernels.cuh clears a table for board + batch and re-inserts the whole board in every call: O(board) per batch.  Here the board's
// table is the caller's, kept in device memory between calls (weed_index_host.hpp has the two tables and the layout), and a call costs
// O(batch):
//   k_weed_insert           (weed_kernels.cuh, as it is, with n_prior = 0) the batch's own keys -> the batch table in the scratch
//   k_weed_lookup_indexed   one lane = one ballot, after the kernel boundary: per key, the index (plain loads) says EG_DUP_PRIOR; otherwise
//                           the batch table gives the owner by the minimum rule.  Same dup_of, status_out, keep flag and counters as
//                           k_weed_lookup: a board reference is below every batch reference, so "the index first" IS the minimum.
//   k_weed_scan_*, k_weed_copy   (weed_kernels.cuh, as they are) the kept keys -> the board, the new count
//   k_weed_index_add        lanes over board entries [n_prior, *board_count): the entries this call has just appended -> the index.  The
//                           count is read from device memory behind the kernel boundary; an append that did not fit left it at n_prior
//                           and nothing is added.  32-bit compare-and-swap from empty, atomic minimum on equal bytes.
//                           eg_weed_index_build_device is the same kernel over [0, n_prior) behind a memset of the index
//   k_weed_index_find       the owner lane over caller keys: the smallest board position of 64 bytes
// There are no tombstones: nothing is ever removed from a board, so a probe chain only grows and a reader never needs to skip a slot.
// Every probe loop is bounded by the slot count, and a reference is dereferenced only below the bound its Keys adapter carries
// (WeedKeysDev::at): a garbage index gives undefined verdicts, never a read outside the board.
#pragma once
#include "weed_index_host.hpp"
#include "weed_kernels.cuh"

namespace egw {

// dup_of of participating ballot b: EG_DUP_PRIOR if the index holds any of its keys, else by the batch table as weed_lane_ballot.
// `index` is a Table whose peek widens the 32-bit slots (index_widen); both tables are only read.  An index holds board positions only,
// all below BATCH_BASE, so its owner is never the key's own batch reference: anything but EMPTY is a hit.
template <class Index, class Table, class Keys>
EGW_HD uint32_t weed_lane_ballot_indexed(const Index& index, uint64_t index_slots, uint64_t index_seed, const Table& tab, const Keys& keys,
                                         uint64_t slots, uint64_t seed, uint64_t b, uint32_t keys_per_ballot, bool& missing) {
  uint32_t dup = DUP_NONE;
  for (uint32_t k = 0; k < keys_per_ballot; ++k) {
    const uint64_t ref = batch_ref(b, keys_per_ballot, k);
    if (weed_lane_owner(index, keys, index_slots, index_seed, ref) != EMPTY) { dup = DUP_PRIOR; continue; }
    const uint64_t owner = weed_lane_owner(tab, keys, slots, seed, ref);
    if (owner == EMPTY || is_board_ref(owner)) { missing = true; continue; }      // the batch table holds batch references only
    const uint64_t ob = ref_ballot(owner, keys_per_ballot);
    if (ob < b && dup != DUP_PRIOR && (uint32_t)ob < dup) dup = (uint32_t)ob;
  }
  return dup;
}
// pos of a caller key (Keys: batch reference q = query q): its smallest board position, or EG_DUP_NONE
template <class Index, class Keys>
EGW_HD uint32_t weed_lane_find(const Index& index, const Keys& keys, uint64_t index_slots, uint64_t index_seed, uint64_t q) {
  const uint64_t owner = weed_lane_owner(index, keys, index_slots, index_seed, BATCH_BASE + q);
  return is_board_ref(owner) ? (uint32_t)owner : DUP_NONE;
}

}  // namespace egw

#if defined(__HIPCC__)

namespace eg {

// the index while lanes insert into it: 32-bit atomics behind the 64-bit Table interface
struct WeedIndexDev {
  unsigned int* slots;
  __device__ __forceinline__ uint64_t peek(uint64_t i) const {
    return egw::index_widen(__hip_atomic_load(slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  __device__ __forceinline__ uint64_t claim(uint64_t i, uint64_t ref) { return egw::index_widen(atomicCAS(slots + i, egw::INDEX_EMPTY, (unsigned int)ref)); }
  __device__ __forceinline__ void lower(uint64_t i, uint64_t ref) { (void)atomicMin(slots + i, (unsigned int)ref); }
};
struct WeedIndexRead {                      // after the kernel boundary: plain loads
  const unsigned int* slots;
  __device__ __forceinline__ uint64_t peek(uint64_t i) const { return egw::index_widen(slots[i]); }
};
// caller keys for find: batch reference q -> the 64 bytes of query q; board positions as in WeedKeysDev
struct WeedFindKeysDev {
  const uint8_t* queries;
  const uint8_t* board;
  uint64_t n_q, n_prior;
  __device__ __forceinline__ void load(uint32_t w[16], uint64_t ref) const {
    const uint4* p = nullptr;
    if (egw::is_board_ref(ref)) { if (ref < n_prior) p = reinterpret_cast<const uint4*>(board + ref * egw::KEY_BYTES); }
    else if (ref - egw::BATCH_BASE < n_q) p = reinterpret_cast<const uint4*>(queries + (ref - egw::BATCH_BASE) * egw::KEY_BYTES);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = p ? p[q] : make_uint4(0u, 0u, 0u, 0u);
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
};

// whole blocks, as k_weed_lookup.  keys.n_prior is the board the index covers; the batch table holds batch references only
__global__ void __launch_bounds__(WEED_NT) k_weed_lookup_indexed(WeedKeysDev keys, const uint32_t* status, const unsigned int* index,
                                                                 uint64_t index_slots, uint64_t index_seed, const unsigned long long* slots,
                                                                 uint64_t n_slots, uint64_t seed, uint32_t* dup_of, uint32_t* status_out,
                                                                 uint32_t* pos, uint32_t* found) {
  const uint64_t b = (uint64_t)blockIdx.x * WEED_NT + threadIdx.x;
  const bool live = b < keys.n;
  const uint32_t st = live && status ? status[b] : 0u;
  const bool part = live && st == 0u;
  const WeedIndexRead idx{index};
  const WeedTableRead tab{slots};
  bool missing = false;
  const uint32_t dup = part ? egw::weed_lane_ballot_indexed(idx, index_slots, index_seed, tab, keys, n_slots, seed, b, keys.keys_per_ballot, missing)
                            : egw::DUP_NONE;
  if (live) {
    dup_of[b] = dup;
    if (status_out) status_out[b] = egw::weed_status_out(st, dup);
    pos[b] = part && dup == egw::DUP_NONE ? 1u : 0u;
  }
  weed_wave_tally(found, dup == egw::DUP_PRIOR);
  weed_wave_tally(found + 1, dup != egw::DUP_NONE && dup != egw::DUP_PRIOR);
  weed_wave_tally(found + 2, missing);
}

// board entries [first, end) -> the index; end = *board_count when that is given (this call's append, written by k_weed_scan_tops in an
// earlier launch), clamped to the board's room.  References at or above end are never dereferenced
__global__ void __launch_bounds__(WEED_NT) k_weed_index_add(const uint8_t* board, uint64_t first, uint64_t end, const unsigned long long* board_count,
                                                            uint64_t board_cap, unsigned int* index, uint64_t index_slots, uint64_t index_seed,
                                                            uint32_t* found) {
  if (board_count) end = *board_count;
  if (end > board_cap) end = board_cap;
  const WeedKeysDev keys{nullptr, board, nullptr, 0u, 0u, end, 1u};
  WeedIndexDev tab{index};
  uint32_t over = 0;
  for (uint64_t j = first + (uint64_t)blockIdx.x * WEED_NT + threadIdx.x; j < end; j += (uint64_t)gridDim.x * WEED_NT)
    if (!egw::weed_lane_insert(tab, keys, index_slots, index_seed, j)) ++over;
  if (over) atomicAdd(found, over);
}

__global__ void __launch_bounds__(WEED_NT) k_weed_index_find(WeedFindKeysDev keys, const unsigned int* index, uint64_t index_slots,
                                                             uint64_t index_seed, uint32_t* pos) {
  const WeedIndexRead idx{index};
  for (uint64_t q = (uint64_t)blockIdx.x * WEED_NT + threadIdx.x; q < keys.n_q; q += (uint64_t)gridDim.x * WEED_NT)
    pos[q] = egw::weed_lane_find(idx, keys, index_slots, index_seed, q);
}

}  // namespace eg
#endif
