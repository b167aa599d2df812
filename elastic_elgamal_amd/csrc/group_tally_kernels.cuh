// group_tally_kernels.cuh -- the per-group tally of a verified batch (eg_*_tally_grouped*, eg_hip.hip): tallies[g] = the homomorphic sum
// of the ciphertexts of the accepted ballots whose group id is g, for every g at once.  examples/voting.rs:199-203 adds every accepted
// ballot into ONE total; an election that publishes results per precinct needs one total per precinct, and a verify call per precinct
// costs a call's latency each.
//
// The pass runs AFTER a verify entry, over the wire bytes that are still in device memory, and reads nothing but the plan's immutable
// tally items (which 32-byte items of a ballot are its ciphertext points): no engine workspace, no running tally.  It is the keyed sum
// that pippenger.cuh solves for buckets, with the same shape (group_tally_host.hpp has the arithmetic):
//   k_gt_count       one lane = one ballot: accepted and id in range -> count[id] += 1 (wave-aggregated: one precinct may hold half of all
//                    ballots); an accepted ballot with an id >= n_groups other than EG_GROUP_NONE counts in bad[0].  Ids of rejected
//                    ballots are never read.
//   k_gt_scan_*      prefix sums over the groups (the three bodies of scan.cuh, which k_pip_scan_* wrap too, around this pass's piece
//                    sizes): list offsets, and pieces / first piece per group for every level at once
//   k_gt_fill        one lane = one ballot: append its index to its group's list (atomic cursor: the ORDER inside a list depends on
//                    timing, the sum does not - and the result is a canonical encoding)
//   k_gt_sum_wire    one lane = one piece x one tally slot: load the slot's wire item of up to S1 ballots (two 128-bit loads), decode, add.
//                    A point that does not decode - the caller's status words said "accepted" over bytes no verifier accepted - counts in
//                    bad[1] and adds the identity.
//   k_gt_sum_points  one lane = one piece x one slot of partial sums; repeated until every group has at most one entry
//   k_gt_encode      one lane = one group x one slot: canonical encoding (the identity, 32 zero bytes, for a group without ballots);
//                    the counts go out with slot 0
// The lane bodies of the last three and gt_bucket_of are plain functions over their memory, so that the host check build
// (tests/hostcheck/grouptallycheck.cpp, -DEG_BOUNDCHECK) runs the same code with other piece sizes on arrays.
// The weighted pass (eg_*_tally_weighted*) is the same pass with [weights[b]] x point at level 0 (ge_mul_u64, gt_lane_wire_weighted), a weight
// check in count and fill, and the exact sums of weights carried through the levels beside the points; it has kernels of its own for
// those steps (k_gtw_*) and shares the scan, k_gt_sum_points and k_gt_encode (tests/hostcheck/weightedtallycheck.cpp runs its lane bodies).
#pragma once
#include "ge25519.cuh"
#include "group_tally_host.hpp"

namespace eg {

// one level: group q owns entries [off[q], off[q] + cnt[q]) of the level's input, cut into pieces of <= S; its pieces are numbered from piece0[q]
struct GtLevel { const u32* cnt; const u32* off; const u32* piece0; };

// the group that piece u belongs to: the last q with piece0[q] <= u (empty groups share their successor's piece0 and are skipped)
EG_HD u32 gt_bucket_of(const u32* piece0, u32 n_groups, u32 u) {
  u32 lo = 0, hi = n_groups;                     // invariant: piece0[lo] <= u, (hi == n_groups or piece0[hi] > u)
  while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (piece0[mid] <= u) lo = mid; else hi = mid; }
  return lo;
}
// entries [beg, end) of piece u of its group
EG_HD void gt_piece_range(u32& beg, u32& end, const GtLevel& L, u32 n_groups, u32 u, u32 s) {
  const u32 q = gt_bucket_of(L.piece0, n_groups, u), k = u - L.piece0[q];
  const u32 lim = L.off[q] + L.cnt[q];
  beg = L.off[q] + k * s;
  end = lim - beg < s ? lim : beg + s;
}

// level 0, slot t of piece u: the sum of wire item `item` over the piece's ballots -> out[u n_slots + t]
template <class WireIO, class PointIO, class Bad>
EG_HD void gt_lane_wire(u32 u, u32 t, u32 n_slots, u32 s1, const GtLevel& L, u32 n_groups, const u32* idx, const WireIO& wire, u32 item,
                        PointIO& out, Bad& bad) {
  u32 beg, end;
  gt_piece_range(beg, end, L, n_groups, u, s1);
  ge acc; ge_identity(acc);
  for (u32 i = beg; i < end; ++i) {
    u32 w[8];
    wire.load(w, idx[i], item);
    ge p, sum;
    if (!ristretto_decode(p, w)) bad.undecodable();      // p is then the identity
    ge_add_full(sum, acc, p); acc = sum;
  }
  out.store((size_t)u * n_slots + t, acc);
}
// level l >= 1, slot t of piece u: the sum of up to s2 partial sums of the level before -> out[u n_slots + t]
template <class PointIn, class PointOut>
EG_HD void gt_lane_points(u32 u, u32 t, u32 n_slots, u32 s2, const GtLevel& L, u32 n_groups, const PointIn& in, PointOut& out) {
  u32 beg, end;
  gt_piece_range(beg, end, L, n_groups, u, s2);
  ge acc;
  in.load(acc, (size_t)beg * n_slots + t);
  for (u32 i = beg + 1; i < end; ++i) {
    ge p, sum;
    in.load(p, (size_t)i * n_slots + t);
    ge_add_full(sum, acc, p); acc = sum;
  }
  out.store((size_t)u * n_slots + t, acc);
}
// slot t of group g after the last level (pieces[g] is 0 or 1): its canonical encoding
template <class PointIn>
EG_HD void gt_lane_encode(u32 w[8], u32 g, u32 t, u32 n_slots, const u32* pieces, const u32* piece0, const PointIn& in) {
  if (pieces[g] == 0u) {
    for (int i = 0; i < 8; ++i) w[i] = 0u;             // Ciphertext::zero(): the identity encodes as zero bytes
    return;
  }
  ge p;
  in.load(p, (size_t)piece0[g] * n_slots + t);
  ristretto_encode(w, p);
}

// ---- the weighted pass (eg_*_tally_weighted*): tallies[g] = sum of [w_b] x the ciphertexts of g's accepted ballots, w_b < 2^bits ---------
// r = [w mod 2^bits] p, 1 <= bits <= 64: a left-to-right binary ladder of exactly `bits` steps, the same instruction stream whatever w
// is (lanes of a wavefront hold different weights): double, then add p or - by select - the identity.  ~16 field operations a bit; no
// table (a radix-16 table is 1.1 KiB a lane, and the pass owns no workspace).  Bits of w at and above `bits` are NOT looked at: the
// range check of the count / fill kernels is what keeps a longer weight out.
EG_HD void ge_mul_u64(ge& r, const ge& p, u64 w, int bits) {
  ge_cached pc, ident;
  ge_to_cached(pc, p);
  ge_cached_identity(ident);
  ge_p2 q;
  fe_0(q.X); fe_1(q.Y); fe_1(q.Z);
#pragma unroll 1
  for (int i = bits - 1; i >= 0; --i) {
    const bool skip = ((w >> i) & 1u) == 0u;
    ge_p1p1 t;
    ge acc;
    ge_dbl(t, q.X, q.Y, q.Z);
    ge_dbl_to_p3(acc, t);
    ge_cached c = pc;
    fe_cmov(c.YpX, ident.YpX, skip); fe_cmov(c.YmX, ident.YmX, skip);
    fe_cmov(c.Z2, ident.Z2, skip); fe_cmov(c.T2d, ident.T2d, skip);
    ge_add(t, acc, c);
    if (i > 0) ge_add_to_p2(q, t);      // next comes a doubling: T is not needed
    else ge_add_to_p3(r, t);
  }
}

// what the count and fill kernels decide about ballot b: 0 = not counted (rejected, or in no group), 1 = counted in group g, 2 = accepted
// with a stray id (bad[0]), 3 = accepted, id in range, weight of more than `bits` bits (bad[2]).  Ids and weights of rejected ballots are
// never read, weights of ballots in no group neither; groups == nullptr: every ballot in group 0.
template <class WeightIO>
EG_HD u32 gt_weighted_class(u32& g, u32 b, const u32* status, const u32* groups, u32 n_groups, const WeightIO& weights, int bits) {
  g = eggt::GROUP_NONE;
  if (status[b] != 0u) return 0u;
  g = groups ? groups[b] : 0u;
  if (g == eggt::GROUP_NONE) return 0u;
  if (g >= n_groups) return 2u;
  return eggt::weight_fits(weights.load(b), bits) ? 1u : 3u;
}

// level 0, slot t of piece u: the sum of [weight] x wire item `item` over the piece's ballots -> out[u n_slots + t]; the lane of slot 0
// also leaves the piece's sum of weights in sums[u]
template <class WireIO, class WeightIO, class PointIO, class SumIO, class Bad>
EG_HD void gt_lane_wire_weighted(u32 u, u32 t, u32 n_slots, u32 s1, const GtLevel& L, u32 n_groups, const u32* idx, const WireIO& wire, u32 item,
                                 const WeightIO& weights, int bits, PointIO& out, SumIO& sums, Bad& bad) {
  u32 beg, end;
  gt_piece_range(beg, end, L, n_groups, u, s1);
  ge acc; ge_identity(acc);
  u64 lo = 0, hi = 0;
  for (u32 i = beg; i < end; ++i) {
    const u32 b = idx[i];
    u32 w[8];
    wire.load(w, b, item);
    const u64 k = weights.load(b);
    ge p, m, sum;
    if (!ristretto_decode(p, w)) bad.undecodable();      // p is then the identity
    ge_mul_u64(m, p, k, bits);
    ge_add_full(sum, acc, m); acc = sum;
    lo += k; hi += lo < k ? 1u : 0u;
  }
  out.store((size_t)u * n_slots + t, acc);
  if (t == 0u) sums.store(u, lo, hi);
}
// level l >= 1, piece u: the sum of up to s2 weight sums of the level before -> out[u]
template <class SumIn, class SumOut>
EG_HD void gt_lane_weight_sums(u32 u, u32 s2, const GtLevel& L, u32 n_groups, const SumIn& in, SumOut& out) {
  u32 beg, end;
  gt_piece_range(beg, end, L, n_groups, u, s2);
  u64 lo = 0, hi = 0;
  for (u32 i = beg; i < end; ++i) {
    u64 a, c;
    in.load(a, c, i);
    lo += a; hi += c + (lo < a ? 1u : 0u);
  }
  out.store(u, lo, hi);
}
// group g after the last level (pieces[g] is 0 or 1): its sum of weights
template <class SumIn>
EG_HD void gt_lane_weight_sum_out(u64& lo, u64& hi, u32 g, const u32* pieces, const u32* piece0, const SumIn& in) {
  lo = 0; hi = 0;
  if (pieces[g] != 0u) in.load(lo, hi, piece0[g]);
}

}  // namespace eg

#if defined(__HIPCC__)
#include "pippenger.cuh"     // pip_wave_atomic_inc, pip_store_point / pip_load_point

namespace eg {

constexpr int GT_SEQ = eggt::SEQ;
struct GtScan { u32* offsets; u32* pieces[eggt::MAX_LEVELS]; u32* piece0[eggt::MAX_LEVELS]; u32* totals; u32* tile_sums; };

struct GtWireDev {
  const u32* wire;
  u32 stride_words;
  u32 n;                 // ballots behind `wire`
  __device__ __forceinline__ void load(u32 w[8], u32 b, u32 item) const {
    // an index list is only as good as the status words were stable between k_gt_count and k_gt_fill: a caller that lets a verify call
    // rewrite them meanwhile gets a wrong tally, never a read outside its ballots
    const uint4* p = reinterpret_cast<const uint4*>(wire + (size_t)(b < n ? b : 0u) * stride_words + (size_t)item * 8);
    const uint4 a = p[0], c = p[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = c.x; w[5] = c.y; w[6] = c.z; w[7] = c.w;
  }
};
struct GtPointsDev {
  uint4* base;
  __device__ __forceinline__ void store(size_t e, const ge& p) { pip_store_point(base + e * PT_QUADS, p); }
  __device__ __forceinline__ void load(ge& p, size_t e) const { pip_load_point(p, base + e * PT_QUADS); }
};
struct GtBadDev {
  u32 n = 0;
  __device__ __forceinline__ void undecodable() { ++n; }
};

// whole blocks: every lane stays for the wave-level atomics
__global__ void __launch_bounds__(NT) k_gt_count(u32 n, const u32* status, const u32* groups, u32 n_groups, u32* counts, u32* bad) {
  const u32 b0 = blockIdx.x * NT + threadIdx.x;
  const bool live = b0 < n;
  const u32 b = live ? b0 : n - 1u;
  const bool accepted = live && status[b] == 0u;
  const u32 g = accepted ? groups[b] : eggt::GROUP_NONE;            // the id of a rejected ballot is never read
  const bool stray = accepted && g >= n_groups && g != eggt::GROUP_NONE;
  const unsigned long long strays = __ballot(stray);
  if (strays && (threadIdx.x & 63) == __ffsll((long long)strays) - 1) atomicAdd(bad, (u32)__popcll(strays));
  (void)pip_wave_atomic_inc(counts, (size_t)g, accepted && g < n_groups);
}
__global__ void __launch_bounds__(NT) k_gt_fill(u32 n, const u32* status, const u32* groups, u32 n_groups, const u32* offsets, u32* cursors,
                                                u32* idx) {
  const u32 b0 = blockIdx.x * NT + threadIdx.x;
  const bool live = b0 < n;
  const u32 b = live ? b0 : n - 1u;
  const bool accepted = live && status[b] == 0u;
  const u32 g = accepted ? groups[b] : eggt::GROUP_NONE;
  const bool in = accepted && g < n_groups;
  const u32 pos = pip_wave_atomic_inc(cursors, (size_t)g, in);
  const u32 at = in ? offsets[g] + pos : 0u;                       // pos < counts[g]: the same ballots were counted by k_gt_count ...
  if (in && at < n) idx[at] = b;                                   // ... unless the caller let the status words change in between
}

// ---- prefix sums over the groups, for the lists and for every level of pieces at once (three launches: scan.cuh) ----------------------
struct GtLoad {
  const u32* counts; u32 n; int levels; u32 s1, s2;
  __device__ __forceinline__ void operator()(u32 v[GT_SEQ], u32 i) const { eggt::pieces_tuple(v, i < n ? counts[i] : 0u, levels, s1, s2); }
};
__global__ void __launch_bounds__(NT) k_gt_scan_tiles(const u32* counts, u32 n, int levels, u32 s1, u32 s2, GtScan S) {
  scan_tile_sums<GT_SEQ>(S.tile_sums, GtLoad{counts, n, levels, s1, s2});
}
__global__ void k_gt_scan_tops(u32 n_tiles, GtScan S) {            // launched with 64 * GT_SEQ threads
  const u32 total = scan_tops<GT_SEQ>(n_tiles, S.tile_sums);
  const int k = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0 && k >= 1) S.totals[k - 1] = total;
}
__global__ void __launch_bounds__(NT) k_gt_scan_apply(const u32* counts, u32 n, int levels, u32 s1, u32 s2, GtScan S) {
  u32 v[SCAN_PER_LANE][GT_SEQ], run[GT_SEQ];
  scan_apply<GT_SEQ>(S.tile_sums, GtLoad{counts, n, levels, s1, s2}, v, run);
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    const u32 i = scan_element(e);
    if (i < n) {
      S.offsets[i] = run[0];
#pragma unroll
      for (int l = 0; l < eggt::MAX_LEVELS; ++l)
        if (l < levels) { S.pieces[l][i] = v[e][l + 1]; S.piece0[l][i] = run[l + 1]; }
    }
#pragma unroll
    for (int k = 0; k < GT_SEQ; ++k) run[k] += v[e][k];
  }
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------------
// lanes: pieces of the level x tally slots, slot fastest (the lanes of a piece read neighbouring items of the same ballots)
__global__ void __launch_bounds__(NT, 2) k_gt_sum_wire(u32 s1, u32 n_slots, GtLevel L, const u32* total, u32 n_groups, const u32* idx,
                                                       GtWireDev wire, const u32* items, uint4* out, u32* bad) {
  const size_t lanes = (size_t)*total * n_slots;
  GtPointsDev o{out};
  GtBadDev nb;
  for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < lanes; j += (size_t)gridDim.x * NT) {
    const u32 u = (u32)(j / n_slots), t = (u32)(j % n_slots);
    gt_lane_wire(u, t, n_slots, s1, L, n_groups, idx, wire, items[t], o, nb);
  }
  if (nb.n) atomicAdd(bad + 1, nb.n);
}
__global__ void __launch_bounds__(NT, 2) k_gt_sum_points(u32 s2, u32 n_slots, GtLevel L, const u32* total, u32 n_groups, const uint4* in,
                                                         uint4* out) {
  const size_t lanes = (size_t)*total * n_slots;
  const GtPointsDev i{const_cast<uint4*>(in)};
  GtPointsDev o{out};
  for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < lanes; j += (size_t)gridDim.x * NT)
    gt_lane_points((u32)(j / n_slots), (u32)(j % n_slots), n_slots, s2, L, n_groups, i, o);
}
// pieces / piece0: the last level's; tallies: [n_groups][n_slots][8] words; out_counts may be null
__global__ void __launch_bounds__(NT, 2) k_gt_encode(u32 n_groups, u32 n_slots, const u32* pieces, const u32* piece0, const uint4* in,
                                                     const u32* counts, u32* tallies, u32* out_counts) {
  const size_t lanes = (size_t)n_groups * n_slots;
  const GtPointsDev i{const_cast<uint4*>(in)};
  for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < lanes; j += (size_t)gridDim.x * NT) {
    const u32 g = (u32)(j / n_slots), t = (u32)(j % n_slots);
    u32 w[8];
    gt_lane_encode(w, g, t, n_slots, pieces, piece0, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) tallies[j * 8 + k] = w[k];
    if (t == 0u && out_counts) out_counts[g] = counts[g];
  }
}

// ---- the weighted pass: count and fill with the weight check, the level-0 sum with the ladder, the weight sums beside the points ----------
// (the scan kernels, k_gt_sum_points and k_gt_encode serve it as they are)
struct GtWeightsDev {
  const u64* w;
  u32 n;                 // ballots behind `w`
  __device__ __forceinline__ u64 load(u32 b) const { return w[b < n ? b : 0u]; }      // clamped as GtWireDev::load, for the same reason
};
struct GtSumsDev {
  u64* base;             // (low, high) per piece
  __device__ __forceinline__ void store(u32 u, u64 lo, u64 hi) { base[2 * (size_t)u] = lo; base[2 * (size_t)u + 1] = hi; }
  __device__ __forceinline__ void load(u64& lo, u64& hi, u32 u) const { lo = base[2 * (size_t)u]; hi = base[2 * (size_t)u + 1]; }
};
// *ctr += the lanes of the wavefront with `flag`, in one atomic
__device__ __forceinline__ void gt_wave_tally(u32* ctr, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (u32)__popcll(m));
}

// whole blocks, as k_gt_count / k_gt_fill
__global__ void __launch_bounds__(NT) k_gtw_count(u32 n, const u32* status, const u32* groups, u32 n_groups, GtWeightsDev weights, int bits,
                                                  u32* counts, u32* bad) {
  const u32 b = blockIdx.x * NT + threadIdx.x;
  u32 g = eggt::GROUP_NONE;
  const u32 cls = b < n ? gt_weighted_class(g, b, status, groups, n_groups, weights, bits) : 0u;
  gt_wave_tally(bad, cls == 2u);
  gt_wave_tally(bad + 2, cls == 3u);
  (void)pip_wave_atomic_inc(counts, (size_t)g, cls == 1u);
}
__global__ void __launch_bounds__(NT) k_gtw_fill(u32 n, const u32* status, const u32* groups, u32 n_groups, GtWeightsDev weights, int bits,
                                                 const u32* offsets, u32* cursors, u32* idx) {
  const u32 b = blockIdx.x * NT + threadIdx.x;
  u32 g = eggt::GROUP_NONE;
  const bool in = b < n && gt_weighted_class(g, b, status, groups, n_groups, weights, bits) == 1u;
  const u32 pos = pip_wave_atomic_inc(cursors, (size_t)g, in);
  const u32 at = in ? offsets[g] + pos : 0u;                       // as k_gt_fill: inside the list unless the caller's words changed meanwhile
  if (in && at < n) idx[at] = b;
}
__global__ void __launch_bounds__(NT, 2) k_gtw_sum_wire(u32 s1, u32 n_slots, GtLevel L, const u32* total, u32 n_groups, const u32* idx,
                                                        GtWireDev wire, const u32* items, GtWeightsDev weights, int bits, uint4* out, u64* sums,
                                                        u32* bad) {
  const size_t lanes = (size_t)*total * n_slots;
  GtPointsDev o{out};
  GtSumsDev ws{sums};
  GtBadDev nb;
  for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < lanes; j += (size_t)gridDim.x * NT) {
    const u32 u = (u32)(j / n_slots), t = (u32)(j % n_slots);
    gt_lane_wire_weighted(u, t, n_slots, s1, L, n_groups, idx, wire, items[t], weights, bits, o, ws, nb);
  }
  if (nb.n) atomicAdd(bad + 1, nb.n);
}
// one lane = one piece of the level
__global__ void __launch_bounds__(NT) k_gtw_weight_sums(u32 s2, GtLevel L, const u32* total, u32 n_groups, const u64* in, u64* out) {
  const u32 pieces = *total;
  const GtSumsDev i{const_cast<u64*>(in)};
  GtSumsDev o{out};
  for (size_t u = (size_t)blockIdx.x * NT + threadIdx.x; u < pieces; u += (size_t)gridDim.x * NT) gt_lane_weight_sums((u32)u, s2, L, n_groups, i, o);
}
// pieces / piece0: the last level's; weight_sums: [n_groups][2] 64-bit words
__global__ void __launch_bounds__(NT) k_gtw_weight_sums_out(u32 n_groups, const u32* pieces, const u32* piece0, const u64* in, u64* weight_sums) {
  const GtSumsDev i{const_cast<u64*>(in)};
  for (size_t g = (size_t)blockIdx.x * NT + threadIdx.x; g < n_groups; g += (size_t)gridDim.x * NT) {
    u64 lo, hi;
    gt_lane_weight_sum_out(lo, hi, (u32)g, pieces, piece0, i);
    weight_sums[2 * g] = lo; weight_sums[2 * g + 1] = hi;
  }
}

}  // namespace eg
#endif
