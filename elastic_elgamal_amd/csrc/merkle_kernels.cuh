// merkle_kernels.cuh -- the receipt log (eg_merkle_*, eg_hip.hip): leaf hashes of a batch, the Merkle tree above the log, audit paths and
// the check of many receipts.  The rule is in include/eg_hip.h, the arithmetic and the layouts in merkle_host.hpp.
//
//   k_merkle_leaf        one lane = one ballot: leaf = H(0x00 || prefix || msg || extra) over three byte ranges, read as sha512_ranges
//                        reads them, for participating ballots only (bytes of the others are never read); the keep flag for the scan
//   k_merkle_scan_*      exclusive prefix sum of the keep flags in ballot order (tiles of 1024, tops, apply): the ranks; the tops kernel
//                        decides whether the append fits and writes the count and the found words
//   k_merkle_place       behind that kernel boundary: leaf_index, and the compacted copy of the leaves into the log (nothing unless all fit)
//   k_merkle_tile<T>     one workgroup reduces an aligned tile of 2^T nodes of one level through up to T levels in LDS (two buffers in turn,
//                        one barrier a level) and writes every level it makes to the node store; the ragged last tile follows the
//                        promotion rule from the GLOBAL node count of the level.  One launch per T levels; no lane waits on a lane of
//                        another workgroup, no atomics, no waiting loops
//   k_merkle_paths       one lane = one requested leaf: its audit path out of the log and the node store
//   k_merkle_check       one lane = one receipt: at most depth(N) node hashes and a compare
// THE NODE HASH is one block: 0x01 || l || r is 65 bytes, so the sixteen 32-bit words of the two children, shifted by the one domain byte
// with the funnel shift of sha512.cuh's rotations, are the block's words 0 .. 8; w[8] carries the last child byte and the padding's 0x80,
// w[15] = 520 bits.  No byte loop, no staging buffer; sha512_compress as it is.
// The lane bodies are plain functions over their memory, so that the host check build (tests/hostcheck/merklecheck.cpp) runs the same code
// serially on arrays.  Everything is variable time: the log is public data.
#pragma once
#include "merkle_host.hpp"
#include "sha512.cuh"

namespace eg {

// H(0x01 || l || r): children and result as the eight little-endian 32-bit words of their 32 bytes in memory; out may be l or r
EG_HD void merkle_node(u32 out[8], const u32 l[8], const u32 r[8]) {
  u32 c[16];                   // the 64 child bytes as big-endian words
#pragma unroll
  for (int i = 0; i < 8; ++i) { c[i] = __builtin_bswap32(l[i]); c[8 + i] = __builtin_bswap32(r[i]); }
  u64 w[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const u32 hi = eg_funnel(k ? c[2 * k - 1] : 0x01u, c[2 * k], 8);       // the domain byte 0x01 leads word 0
    const u32 lo = eg_funnel(c[2 * k], c[2 * k + 1], 8);
    w[k] = ((u64)hi << 32) | lo;
  }
  w[8] = (u64)((c[15] << 24) | 0x00800000u) << 32;                          // the last child byte, then the padding
#pragma unroll
  for (int k = 9; k < 15; ++k) w[k] = 0;
  w[15] = 520;                                                              // 65 bytes
  Sha512 s; sha512_init(s);
  sha512_compress(s, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[2 * i] = __builtin_bswap32((u32)(s.h[i] >> 32));
    out[2 * i + 1] = __builtin_bswap32((u32)s.h[i]);
  }
}
// the first 32 digest bytes as eight little-endian words
EG_HD void merkle_digest(u32 out[8], const Sha512& s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[2 * i] = __builtin_bswap32((u32)(s.h[i] >> 32));
    out[2 * i + 1] = __builtin_bswap32((u32)s.h[i]);
  }
}
// H of the empty string, the root of the empty tree: one block of padding
EG_HD void merkle_empty_root(u32 out[8]) {
  u64 w[16];
  w[0] = 0x8000000000000000ull;
#pragma unroll
  for (int k = 1; k < 16; ++k) w[k] = 0;
  Sha512 s; sha512_init(s);
  sha512_compress(s, w);
  merkle_digest(out, s);
}
// The leaf's message is three byte ranges of any length and alignment: the domain byte and the prefix, msg, extra.  It is sha512_ranges
// with three ranges, restated with a reader of scalar members only: the reader of sha512.cuh selects among the ADDRESSES of its ranges'
// pointers, which keeps them in a stack array (32 bytes of scratch a lane in k_sha512), and no kernel of the receipt log uses scratch.
// Both values are loaded before the select, so that the compiler selects among values.
struct MerkleRanges {
  const unsigned char *p0, *p1, *p2;
  size_t l0, l1, l2;
};
struct MerkleReader {
  const unsigned char *cur, *end;
  int next;            // the range after the current one
  bool padded;
  EG_HD void open(const MerkleRanges& r) { cur = r.p0; end = cur + r.l0; next = 1; padded = false; }
  EG_HD u64 word(const MerkleRanges& r) {
    u64 v = 0;
    if ((size_t)(end - cur) >= 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v = (v << 8) | cur[k];
      cur += 8;
      return v;
    }
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      while (cur == end && next < 3) {
        const unsigned char *a = r.p1, *b = r.p2;
        const size_t la = r.l1, lb = r.l2;
        cur = next == 1 ? a : b;
        end = cur + (next == 1 ? la : lb);
        ++next;
      }
      u32 byte = 0;
      if (cur != end) byte = *cur++;
      else if (!padded) { byte = 0x80u; padded = true; }
      v = (v << 8) | byte;
    }
    return v;
  }
};
EG_HD void merkle_leaf_hash(u32 out[8], const MerkleRanges& r) {
  const size_t total = r.l0 + r.l1 + r.l2;
  const size_t blocks = (total + 17 + 127) / 128;              // the 0x80 byte and the 128-bit length always fit the last block
  Sha512 s; sha512_init(s);
  MerkleReader rd; rd.open(r);
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = rd.word(r);
    if (b + 1 == blocks) w[15] = (u64)total << 3;
    sha512_compress(s, w);
  }
  merkle_digest(out, s);
}

// ---- the leaf pass ---------------------------------------------------------------------------------------------------------------------
// Mem: ranges(b) = the byte ranges of ballot b, leaf_put(b, w) / leaf_zero(b) = its row of the leaves (leaves_out, or the staging rows),
// keep(b, flag) = the scan's input
template <class Mem>
EG_HD void merkle_lane_leaf(Mem& m, uint64_t b, bool part) {
  if (part) {
    u32 h[8];
    merkle_leaf_hash(h, m.ranges(b));
    m.leaf_put(b, h);
  } else {
    m.leaf_zero(b);
  }
  m.keep(b, part ? 1u : 0u);
}
// Mem: rank(b) = the scan's output (NO_PATH: no leaf), index_put(b, v), leaf_word(b, w), tail_put(entry, w, v) = word w of the entry
// behind the first n_prior; lane = ballot b, word w of its leaf
template <class Mem>
EG_HD void merkle_lane_place(Mem& m, uint64_t b, uint32_t w, uint64_t n_prior, bool append, uint64_t room) {
  const uint32_t rank = m.rank(b);
  if (w == 0) m.index_put(b, rank == egm::NO_PATH ? egm::LEAF_NONE : n_prior + rank);
  if (append && rank != egm::NO_PATH && rank < room) m.tail_put(rank, w, m.leaf_word(b, w));
}
// what the scan kernels compute, serially: keep flag -> rank among the kept ballots, NO_PATH for the others; returns their number
inline uint32_t merkle_scan_serial(uint32_t* pos, size_t n) {
  uint32_t run = 0;
  for (size_t i = 0; i < n; ++i) pos[i] = pos[i] ? run++ : egm::NO_PATH;
  return run;
}

// ---- the tree --------------------------------------------------------------------------------------------------------------------------
// step s (1 .. steps) of tile `tile` of an input level with n_in nodes: lane t makes node g = tile 2^(TL - s) + t of the level s above the
// input, from the input itself (s == 1) or from the buffer of step s - 1.  Mem: in(g, w), lds_get(parity, local, w), lds_put(parity,
// local, w), out(s, g, w).  Steps of one tile run in order with a barrier between them; lanes of a step in any order.
template <int TL, class Mem>
EG_HD void merkle_tile_step(Mem& m, uint64_t tile, int s, uint32_t t, uint64_t n_in) {
  static_assert(TL >= 2 && TL <= 10, "a tile of 4 .. 1024 nodes");
  const uint64_t n_prev = egm::level_count(n_in, s - 1), n_s = egm::level_count(n_in, s);
  const uint64_t g = (tile << (TL - s)) + t;
  if (t >= (1u << (TL - s)) || g >= n_s) return;
  const bool pair = 2 * g + 1 < n_prev;          // else: the odd last node of the level below, promoted unchanged
  u32 l[8], r[8];
  if (s == 1) {
    m.in(2 * g, l);
    if (pair) m.in(2 * g + 1, r);
  } else {
    m.lds_get((s - 1) & 1, 2 * t, l);
    if (pair) m.lds_get((s - 1) & 1, 2 * t + 1, r);
  }
  if (pair) merkle_node(l, l, r);
  m.lds_put(s & 1, t, l);
  m.out(s, g, l);
}

// ---- paths and the check ---------------------------------------------------------------------------------------------------------------
// Mem: node(level, off, idx, w) = node idx of level `level` (0: the log; else the node store, whose level starts at node `off`),
// path_put(j, k, w), path_zero(j, k).  Returns path_len
template <class Mem>
EG_HD uint32_t merkle_lane_path(Mem& m, uint64_t j, uint64_t i, uint64_t n_leaves, int depth) {
  uint32_t len = 0;
  const bool known = i < n_leaves;
  if (known) {
    uint64_t off = 0, n = n_leaves;
    for (int level = 0; n > 1; ++level) {
      if ((i ^ 1u) < n) {
        u32 w[8];
        m.node(level, off, i ^ 1u, w);
        m.path_put(j, len++, w);
      }
      if (level >= 1) off += n;
      i >>= 1;
      n = (n + 1) >> 1;
    }
  }
  for (uint32_t k = len; k < (uint32_t)depth; ++k) m.path_zero(j, k);
  return known ? len : egm::NO_PATH;
}
// Mem: index(j), path_len(j), leaf(j, w), path(j, k, w), root(w).  The verdict: the first failure in the order index, length, root; no
// path byte is read unless the length is the one that (i, N) demands
template <class Mem>
EG_HD uint32_t merkle_lane_check(const Mem& m, uint64_t j, uint64_t n_leaves) {
  uint64_t i = m.index(j);
  if (i >= n_leaves) return egm::MERKLE_BAD_INDEX;
  if (m.path_len(j) != egm::path_len(i, n_leaves)) return egm::MERKLE_BAD_LENGTH;
  u32 h[8], p[8];
  m.leaf(j, h);
  uint32_t k = 0;
  for (uint64_t n = n_leaves; n > 1; n = (n + 1) >> 1, i >>= 1) {
    if ((i ^ 1u) >= n) continue;
    m.path(j, k++, p);
    if (i & 1u) merkle_node(h, p, h);
    else merkle_node(h, h, p);
  }
  m.root(p);
  u32 diff = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) diff |= h[q] ^ p[q];
  return diff ? egm::MERKLE_MISMATCH : 0u;
}

}  // namespace eg

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "scan.cuh"

namespace eg {

constexpr int MERKLE_NT = 256;
static_assert(MERKLE_NT == SCAN_NT, "the scan kernels are launched with MERKLE_NT lanes");

__device__ __forceinline__ void merkle_ld8(u32 w[8], const u32* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
}
__device__ __forceinline__ void merkle_st8(u32* p, const u32 w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = w[i];
}
// *ctr += the lanes of the wavefront with `flag`, in one atomic (whole blocks only)
__device__ __forceinline__ void merkle_wave_tally(uint32_t* ctr, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (uint32_t)__popcll(m));
}

struct MerkleItems {
  const unsigned char* msgs;      // ballot b: msg_len bytes at msgs + b * msg_stride
  size_t msg_stride, msg_len;
  const unsigned char* extra;     // ballot b: extra_len bytes at extra + b * extra_stride, or null
  size_t extra_stride, extra_len;
  const unsigned char* head;      // device: the domain byte 0x00 and the prefix, head_len = 1 + prefix_len bytes
  size_t head_len;
};
struct MerkleLeafDev {
  MerkleItems it;
  u32* rows;                      // n x 8 words: leaves_out, or the staging rows of the scratch
  bool zero;                      // rows are the caller's leaves_out: ballots without a leaf get a zeroed row
  u32* pos;
  __device__ __forceinline__ MerkleRanges ranges(uint64_t b) const {
    return MerkleRanges{it.head, it.msgs + b * it.msg_stride, it.extra ? it.extra + b * it.extra_stride : nullptr, it.head_len, it.msg_len,
                        it.extra_len};
  }
  __device__ __forceinline__ void leaf_put(uint64_t b, const u32 w[8]) { merkle_st8(rows + b * 8, w); }
  __device__ __forceinline__ void leaf_zero(uint64_t b) {
    if (!zero) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) rows[b * 8 + i] = 0u;
  }
  __device__ __forceinline__ void keep(uint64_t b, u32 flag) { pos[b] = flag; }
};
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_leaf(MerkleLeafDev mem, const u32* status, uint64_t n) {
  const uint64_t b = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  if (b >= n) return;
  merkle_lane_leaf(mem, b, !status || status[b] == 0u);
}

// ---- exclusive prefix sum of the keep flags (three launches: scan.cuh) ------------------------------------------------------------------
struct MerkleKeepLoad {
  const u32* pos; u32 n;
  __device__ __forceinline__ void operator()(u32 v[1], u32 i) const { v[0] = i < n ? pos[i] : 0u; }
};
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_scan_tiles(const u32* pos, u32 n, u32* tile_sums) {
  scan_tile_sums<1>(tile_sums, MerkleKeepLoad{pos, n});
}
// one wavefront: tile sums -> exclusive prefix sums; the total, whether the leaves fit the log, the new count, the found words
__global__ void k_merkle_scan_tops(u32 n_tiles, u32* tile_sums, uint64_t n_prior, uint64_t room, u32* total_word, unsigned long long* log_count,
                                   u32* found) {
  const u32 run = scan_tops<1>(n_tiles, tile_sums);
  if ((threadIdx.x & 63) == 0) {
    const bool fits = !log_count || run <= room;
    if (total_word) { total_word[0] = run; total_word[1] = fits ? 1u : 0u; }       // null: a call without ballots
    if (log_count) *log_count = n_prior + (fits ? run : 0u);
    if (found) { found[0] = run; found[1] = fits ? 0u : 1u; }
  }
}
// pos[b]: keep flag -> rank among the ballots with a leaf, NO_PATH for the others
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_scan_apply(u32* pos, u32 n, const u32* tile_sums) {
  u32 v[SCAN_PER_LANE][1], run[1];
  scan_apply<1>(tile_sums, MerkleKeepLoad{pos, n}, v, run);
#pragma unroll
  for (int e = 0; e < SCAN_PER_LANE; ++e) {
    const u32 i = scan_element(e);
    if (i < n) pos[i] = v[e][0] ? run[0] : egm::NO_PATH;
    run[0] += v[e][0];
  }
}
struct MerklePlaceDev {
  const u32* pos;
  const u32* rows;
  unsigned long long* leaf_index;
  u32* tail;                      // entry n_prior of the log, or null
  __device__ __forceinline__ u32 rank(uint64_t b) const { return pos[b]; }
  __device__ __forceinline__ void index_put(uint64_t b, uint64_t v) { leaf_index[b] = v; }
  __device__ __forceinline__ u32 leaf_word(uint64_t b, u32 w) const { return rows[b * 8 + w]; }
  __device__ __forceinline__ void tail_put(uint64_t entry, u32 w, u32 v) { tail[entry * 8 + w] = v; }
};
// lanes: ballots x the 8 words of a leaf.  Nothing is appended unless everything fits
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_place(MerklePlaceDev mem, uint64_t n, uint64_t n_prior, uint64_t room, const u32* total_word) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  if (j >= n * 8) return;
  merkle_lane_place(mem, j >> 3, (u32)(j & 7u), n_prior, mem.tail != nullptr && total_word[1] != 0u, room);
}

// ---- the tree --------------------------------------------------------------------------------------------------------------------------
struct MerkleTileArgs {
  const u32* in;                  // the input level: n_in nodes
  uint64_t n_in;
  u32* store;                     // the node store, or null
  uint64_t off[egm::T_LOG];       // off[s - 1]: where the level of step s starts in the store, in nodes
  u32* top;                       // without a store: where the level of the last step goes
  int steps;
};
template <int TL>
struct MerkleTileDev {
  const MerkleTileArgs& a;
  u32* odd;                       // steps 1, 3, ..: 2^(TL - 1) nodes, word-major
  u32* even;                      // steps 2, 4, ..: 2^(TL - 2) nodes
  __device__ __forceinline__ void in(uint64_t g, u32 w[8]) const { merkle_ld8(w, a.in + g * 8); }
  __device__ __forceinline__ void lds_get(int parity, u32 local, u32 w[8]) const {
    const u32* buf = parity ? odd : even;
    const u32 rows = parity ? 1u << (TL - 1) : 1u << (TL - 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = buf[i * rows + local];
  }
  __device__ __forceinline__ void lds_put(int parity, u32 local, const u32 w[8]) {
    u32* buf = parity ? odd : even;
    const u32 rows = parity ? 1u << (TL - 1) : 1u << (TL - 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) buf[i * rows + local] = w[i];
  }
  __device__ __forceinline__ void out(int s, uint64_t g, const u32 w[8]) {
    if (a.store) merkle_st8(a.store + (a.off[s - 1] + g) * 8, w);
    else if (s == a.steps) merkle_st8(a.top + g * 8, w);
  }
};
// A quarter of the tile in lanes: two hashes a lane at the first level, one from the second on.  With half the tile (one hash a lane,
// 8 waves) only one workgroup fits a CU at 151 VGPR and the CU idles through the narrow upper levels: 5.3 ms for 10^7 leaves, slower
// than a launch per level (profiles/r19_receipt_log.txt, run 1).  Three workgroups of 4 waves share a CU and fill each other's gaps.
template <int TL>
__global__ void __launch_bounds__(1 << (TL - 2)) k_merkle_tile(MerkleTileArgs a) {
  __shared__ u32 odd[8 << (TL - 1)];
  __shared__ u32 even[8 << (TL - 2)];
  MerkleTileDev<TL> mem{a, odd, even};
  for (int s = 1; s <= a.steps; ++s) {
#pragma unroll 1
    for (u32 t = threadIdx.x; t < (1u << (TL - s)); t += 1u << (TL - 2)) merkle_tile_step<TL>(mem, blockIdx.x, s, t, a.n_in);
    __syncthreads();
  }
}
// root = the one node of the top level (src), or H("") for the empty tree (src null)
__global__ void k_merkle_root(const u32* src, u32* root) {
  if (threadIdx.x || blockIdx.x) return;
  u32 w[8];
  if (src) merkle_ld8(w, src);
  else merkle_empty_root(w);
  merkle_st8(root, w);
}

// ---- paths and the check ---------------------------------------------------------------------------------------------------------------
struct MerklePathDev {
  const u32* log;
  const u32* store;
  u32* paths;
  size_t stride_words;            // 8 depth(N)
  __device__ __forceinline__ void node(int level, uint64_t off, uint64_t idx, u32 w[8]) const {
    merkle_ld8(w, level ? store + (off + idx) * 8 : log + idx * 8);
  }
  __device__ __forceinline__ void path_put(uint64_t j, u32 k, const u32 w[8]) { merkle_st8(paths + j * stride_words + k * 8, w); }
  __device__ __forceinline__ void path_zero(uint64_t j, u32 k) {
#pragma unroll
    for (int i = 0; i < 8; ++i) paths[j * stride_words + k * 8 + i] = 0u;
  }
};
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_paths(MerklePathDev mem, const unsigned long long* index, uint64_t m, uint64_t n_leaves,
                                                            int depth, u32* path_len) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  if (j >= m) return;
  path_len[j] = merkle_lane_path(mem, j, index[j], n_leaves, depth);
}
struct MerkleCheckDev {
  const unsigned long long* index_;
  const u32* leaves;
  const u32* paths;
  size_t stride_words;
  const u32* path_len_;
  const u32* root_;
  __device__ __forceinline__ uint64_t index(uint64_t j) const { return index_[j]; }
  __device__ __forceinline__ u32 path_len(uint64_t j) const { return path_len_[j]; }
  __device__ __forceinline__ void leaf(uint64_t j, u32 w[8]) const { merkle_ld8(w, leaves + j * 8); }
  __device__ __forceinline__ void path(uint64_t j, u32 k, u32 w[8]) const { merkle_ld8(w, paths + j * stride_words + k * 8); }
  __device__ __forceinline__ void root(u32 w[8]) const { merkle_ld8(w, root_); }
};
// whole blocks: every lane stays for the wave-level atomics
__global__ void __launch_bounds__(MERKLE_NT) k_merkle_check(MerkleCheckDev mem, uint64_t m, uint64_t n_leaves, u32* verdict, u32* found) {
  const uint64_t j = (uint64_t)blockIdx.x * MERKLE_NT + threadIdx.x;
  const bool live = j < m;
  const u32 v = live ? merkle_lane_check(mem, j, n_leaves) : 0u;
  if (live) verdict[j] = v;
  merkle_wave_tally(found, v == egm::MERKLE_BAD_INDEX);
  merkle_wave_tally(found + 1, v == egm::MERKLE_BAD_LENGTH);
  merkle_wave_tally(found + 2, v == egm::MERKLE_MISMATCH);
}

}  // namespace eg
#endif
