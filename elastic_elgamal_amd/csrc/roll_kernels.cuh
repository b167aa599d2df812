// roll_kernels.cuh -- the voter-roll pass (eg_roll_*, eg_hip.hip): which participating ballot of every voter is the one that counts.
// A voter on the roll can sign any number of fresh, valid ballots: none is a replay (weeding) and every signature holds (the signature
// pass).  Systems that allow re-voting as a defence against coercion count one of them, by a policy (Helios, Estonia: the last one).
//
// The rule is a maximum over priority words (roll_host.hpp), so atomicMax alone decides it and no lane ever waits on another:
//   k_roll_claim       one lane = one ballot: a participating ballot with an index in range raises best[v] to its claim (its rank in the
//                      batch + 1; inside a batch the sequence order is the ballot order); the lanes of a wavefront that share a voter
//                      send one atomic between them (a bounded loop of at most 64 rounds)
//   k_roll_resolve     one lane = one ballot, after the kernel boundary (the only synchronisation): the batch winner of v from best[v],
//                      its word W, the old roll[v] - READ-ONLY here, the commit is a launch of its own, or a loser's read would race the
//                      winner's write - the verdict, the per-ballot outputs, the flag for the commit, the counters (one atomic a wavefront)
//   k_roll_scan_*      exclusive prefix sum of the displaced flags in ballot order (tiles of 1024, tops, apply): the order of `displaced`
//   k_roll_commit      the winning lane stores roll[v] = W (one writer per voter: a plain 64-bit store) and its displaced entry at its rank;
//                      it takes everything from the flags and never reads the status words again (status_out may be status_in)
//   k_roll_check       the verdict against a read-only roll
// The lane bodies are plain functions over their memory, so that the host check build (tests/hostcheck/rollcheck.cpp) runs the same code
// serially, in any lane order, on arrays.
#pragma once
#include "roll_host.hpp"

namespace egr {

constexpr uint32_t FLAG_NONE = 0;                 // the commit has nothing to do for this ballot
constexpr uint32_t FLAG_COMMIT = 1;               // batch winner above an empty word: store it
constexpr uint32_t FLAG_DISPLACED = 2;            // batch winner above a non-zero word: store it and report; after the scan, + rank

struct Verdict {
  uint32_t status;             // status_out
  uint64_t superseded_by;
  uint32_t group;
  uint64_t weight;
  uint32_t flag;
  bool superseded, off_roll, not_cast;
};
EGR_HD Verdict verdict_none(uint32_t st) { return Verdict{st, SEQ_NONE, GROUP_NONE, 0u, FLAG_NONE, false, false, false}; }

// Mem, the lanes' view of the memory: key_index(b), raise(v, claim) = atomic maximum, best(v), roll(v), group(v), weight(v)
// (EG_GROUP_NONE / 0 where the caller gave no roster array)
// the claim of ballot b on voter v; 0: none - it does not participate, or its index is off the roll
template <class Mem>
EGR_HD uint32_t roll_lane_claimant(const Mem& m, uint64_t b, uint64_t n, bool part, int policy, uint64_t n_keys, uint32_t& v) {
  v = 0;
  if (!part) return 0u;
  v = m.key_index(b);
  return v < n_keys ? claim_of(b, n, policy) : 0u;
}
template <class Mem>
EGR_HD void roll_lane_claim(Mem& m, uint64_t b, uint64_t n, bool part, int policy, uint64_t n_keys) {
  uint32_t v;
  const uint32_t claim = roll_lane_claimant(m, b, n, part, policy, n_keys, v);
  if (claim) m.raise(v, claim);
}
template <class Mem>
EGR_HD void roll_lane_keep(const Mem& m, uint32_t v, Verdict& V) {
  V.group = m.group(v);
  V.weight = m.weight(v);
}
// `st` is status_in[b] (0 without one); nothing of a ballot that does not participate is read
template <class Mem>
EGR_HD Verdict roll_lane_resolve(const Mem& m, uint64_t b, uint64_t n, uint32_t st, bool part, uint64_t seq_base, int policy, uint64_t n_keys) {
  Verdict V = verdict_none(st);
  if (!part) return V;
  const uint32_t v = m.key_index(b);
  if (v >= n_keys) { V.status = status_word(ROLL_OFF_ROLL); V.off_roll = true; return V; }
  const uint64_t W = word_of(seq_base + claimant(m.best(v), n, policy), policy);      // the batch winner of v
  const uint64_t old = m.roll(v), top = W > old ? W : old;                            // top: the new roll[v]
  if (word_of(seq_base + b, policy) == top) {
    roll_lane_keep(m, v, V);
    if (W > old) V.flag = old ? FLAG_DISPLACED : FLAG_COMMIT;                         // else: this very ballot is on the roll already
  } else {
    V.status = status_word(ROLL_SUPERSEDED);
    V.superseded_by = seq_of(top, policy);
    V.superseded = true;
  }
  return V;
}
template <class Mem>
EGR_HD Verdict roll_lane_check(const Mem& m, uint64_t b, uint32_t st, bool part, uint64_t seq_base, int policy, uint64_t n_keys) {
  Verdict V = verdict_none(st);
  if (!part) return V;
  const uint32_t v = m.key_index(b);
  if (v >= n_keys) { V.status = status_word(ROLL_OFF_ROLL); V.off_roll = true; return V; }
  const uint64_t top = m.roll(v);
  if (top == 0u) { V.status = status_word(ROLL_NOT_CAST); V.not_cast = true; return V; }
  if (word_of(seq_base + b, policy) == top) {
    roll_lane_keep(m, v, V);
  } else {
    V.status = status_word(ROLL_SUPERSEDED);
    V.superseded_by = seq_of(top, policy);
    V.superseded = true;
  }
  return V;
}
// Mem: key_index(b), roll(v), store(v, word), displace(rank, old_seq, new_seq); flag = the scratch word of ballot b after the scan
template <class Mem>
EGR_HD void roll_lane_commit(Mem& m, uint64_t b, uint64_t n, uint32_t flag, uint64_t seq_base, int policy, uint64_t n_keys, bool report) {
  if (flag == FLAG_NONE) return;
  const uint32_t v = m.key_index(b);
  if (v >= n_keys) return;                       // resolve set no flag for such a ballot: never, unless the scratch was written meanwhile
  const uint64_t old = m.roll(v);
  m.store(v, word_of(seq_base + b, policy));
  const uint64_t rank = (uint64_t)flag - FLAG_DISPLACED;
  if (report && flag >= FLAG_DISPLACED && rank < n) m.displace(rank, seq_of(old, policy), seq_base + b);
}

// what the scan kernels compute, serially: FLAG_DISPLACED -> FLAG_DISPLACED + rank among the displaced ones; returns their number
inline uint32_t scan_displaced(uint32_t* flag, size_t n) {
  uint32_t run = 0;
  for (size_t i = 0; i < n; ++i)
    if (flag[i] == FLAG_DISPLACED) flag[i] = FLAG_DISPLACED + run++;
  return run;
}

}  // namespace egr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "scan.cuh"

namespace eg {

constexpr int ROLL_NT = 256;
static_assert(ROLL_NT == SCAN_NT, "the scan kernels are launched with ROLL_NT lanes");

struct RollMemDev {
  const uint32_t* index;
  uint32_t* best_;
  unsigned long long* roll_;
  const uint32_t* groups;
  const unsigned long long* weights;
  unsigned long long* displaced;
  __device__ __forceinline__ uint32_t key_index(uint64_t b) const { return index[b]; }
  __device__ __forceinline__ void raise(uint32_t v, uint32_t claim) { (void)atomicMax(best_ + v, claim); }
  __device__ __forceinline__ uint32_t best(uint32_t v) const { return best_[v]; }
  __device__ __forceinline__ uint64_t roll(uint32_t v) const { return roll_[v]; }
  __device__ __forceinline__ uint32_t group(uint32_t v) const { return groups ? groups[v] : egr::GROUP_NONE; }
  __device__ __forceinline__ uint64_t weight(uint32_t v) const { return weights ? weights[v] : 0u; }
  __device__ __forceinline__ void store(uint32_t v, uint64_t word) { roll_[v] = word; }
  __device__ __forceinline__ void displace(uint64_t rank, uint64_t old_seq, uint64_t new_seq) {
    displaced[2 * rank] = old_seq;
    displaced[2 * rank + 1] = new_seq;
  }
};
struct RollOutDev {
  unsigned long long* superseded_by;
  uint32_t* status_out;
  uint32_t* groups_out;
  unsigned long long* weights_out;
  __device__ __forceinline__ void put(uint64_t b, const egr::Verdict& V) const {
    superseded_by[b] = V.superseded_by;
    if (status_out) status_out[b] = V.status;
    if (groups_out) groups_out[b] = V.group;
    if (weights_out) weights_out[b] = V.weight;
  }
};
// *ctr += the lanes of the wavefront with `flag`, in one atomic (whole blocks only)
__device__ __forceinline__ void roll_wave_tally(uint32_t* ctr, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (uint32_t)__popcll(m));
}

// whole blocks: every lane stays for the wave-level combine.  A flood of one key would put every atomic of the batch on one address - they
// serialise at ~11.5 ns each, 12.1 ms for 2^20 ballots, more than the signature pass takes (profiles/r18_voter_roll.txt) - so the lanes of
// a wavefront that share a voter send ONE.  Inside a batch the claims are ordered like the ballots: the largest claim of a set of lanes is
// that of its last lane under LAST and of its first under FIRST, and no reduction is needed.  Every round retires the first pending lane
// and all that share its voter: at most 64 rounds.
__global__ void __launch_bounds__(ROLL_NT) k_roll_claim(RollMemDev mem, const uint32_t* status, uint64_t n, int policy, uint64_t n_keys) {
  const uint64_t b = (uint64_t)blockIdx.x * ROLL_NT + threadIdx.x;
  const bool live = b < n;
  const int lane = threadIdx.x & 63;
  uint32_t v;
  const uint32_t claim = egr::roll_lane_claimant(mem, b, n, live && (!status || status[b] == 0u), policy, n_keys, v);
  bool pending = claim != 0u;
  for (int round = 0; round < 64; ++round) {
    const unsigned long long active = __ballot(pending);
    if (!active) break;
    const uint32_t lead = (uint32_t)__shfl((int)v, __ffsll((long long)active) - 1, 64);
    const bool mine = pending && v == lead;
    const unsigned long long peers = __ballot(mine);
    const int top = policy == egr::ROLL_LAST ? 63 - __clzll((long long)peers) : __ffsll((long long)peers) - 1;
    if (mine && lane == top) mem.raise(v, claim);
    if (mine) pending = false;
  }
}
// whole blocks: every lane stays for the wave-level atomics.  status_out may be status: lane b alone reads and writes word b
__global__ void __launch_bounds__(ROLL_NT) k_roll_resolve(RollMemDev mem, const uint32_t* status, uint64_t n, uint64_t seq_base, int policy,
                                                          uint64_t n_keys, RollOutDev out, uint32_t* flag, uint32_t* found) {
  const uint64_t b = (uint64_t)blockIdx.x * ROLL_NT + threadIdx.x;
  const bool live = b < n;
  const uint32_t st = live && status ? status[b] : 0u;
  const egr::Verdict V = egr::roll_lane_resolve(mem, b, n, st, live && st == 0u, seq_base, policy, n_keys);
  if (live) {
    out.put(b, V);
    flag[b] = V.flag;
  }
  roll_wave_tally(found, V.superseded);
  roll_wave_tally(found + 1, V.flag == egr::FLAG_DISPLACED);
  roll_wave_tally(found + 2, V.off_roll);
}
__global__ void __launch_bounds__(ROLL_NT) k_roll_check(RollMemDev mem, const uint32_t* status, uint64_t n, uint64_t seq_base, int policy,
                                                        uint64_t n_keys, RollOutDev out, uint32_t* found) {
  const uint64_t b = (uint64_t)blockIdx.x * ROLL_NT + threadIdx.x;
  const bool live = b < n;
  const uint32_t st = live && status ? status[b] : 0u;
  const egr::Verdict V = egr::roll_lane_check(mem, b, st, live && st == 0u, seq_base, policy, n_keys);
  if (live) out.put(b, V);
  roll_wave_tally(found, V.superseded);
  roll_wave_tally(found + 1, V.not_cast);
  roll_wave_tally(found + 2, V.off_roll);
}

// ---- exclusive prefix sum of the displaced flags (three launches: scan.cuh) ----------------------------------------------------------------
struct RollDisplacedLoad {
  const uint32_t* flag; uint32_t n;
  __device__ __forceinline__ void operator()(uint32_t v[1], uint32_t i) const { v[0] = i < n && flag[i] == egr::FLAG_DISPLACED ? 1u : 0u; }
};
__global__ void __launch_bounds__(ROLL_NT) k_roll_scan_tiles(const uint32_t* flag, uint32_t n, uint32_t* tile_sums) {
  scan_tile_sums<1>(tile_sums, RollDisplacedLoad{flag, n});
}
// one wavefront: tile sums -> exclusive prefix sums; the total is the number of displaced entries
__global__ void k_roll_scan_tops(uint32_t n_tiles, uint32_t* tile_sums, unsigned long long* displaced_count) {
  const uint32_t run = scan_tops<1>(n_tiles, tile_sums);
  if ((threadIdx.x & 63) == 0) *displaced_count = run;
}
// flag[b]: FLAG_DISPLACED -> FLAG_DISPLACED + rank among the displaced ones; the other words stay
__global__ void __launch_bounds__(ROLL_NT) k_roll_scan_apply(uint32_t* flag, uint32_t n, const uint32_t* tile_sums) {
  uint32_t v[SCAN_PER_LANE][1], run[1];
  scan_apply<1>(tile_sums, RollDisplacedLoad{flag, n}, v, run);
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    if (v[e][0]) flag[scan_element(e)] = egr::FLAG_DISPLACED + run[0];           // (set only below n)
    run[0] += v[e][0];
  }
}
__global__ void __launch_bounds__(ROLL_NT) k_roll_commit(RollMemDev mem, const uint32_t* flag, uint64_t n, uint64_t seq_base, int policy,
                                                         uint64_t n_keys) {
  const uint64_t b = (uint64_t)blockIdx.x * ROLL_NT + threadIdx.x;
  if (b >= n) return;
  egr::roll_lane_commit(mem, b, n, flag[b], seq_base, policy, n_keys, mem.displaced != nullptr);
}

}  // namespace eg
#endif
