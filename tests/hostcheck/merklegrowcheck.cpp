// Host build of the receipt log's grow entry (elastic_elgamal_amd/csrc/merkle_grow_kernels.cuh, merkle_grow_host.hpp) under ASan + UBSan:
// the plan of merkle_grow_host.hpp, the lane function of the copy kernel and merkle_tile_step driven from tile0 run serially on arrays, as
// eg_merkle_grow_device launches them.  What the pass must never read is overwritten with junk AND poisoned, so that reading it aborts the
// program: the old store's nodes (L, j) with (j + 1) 2^L > m, and the leaves of the log below (m >> T) << T.
// Stand-alone program (tests/test_merkle_grow_cpu.py builds it and reads its report):
//   merklegrowcheck grow T_LOG FILE     lines of leaves (hex); for every 0 <= m <= N <= their number, with tiles of 2^T_LOG nodes (2 or 3):
//                                       the store of N out of the store of m, once with 16-byte and once with 4-byte units of the copy;
//                                       every word of the new store written exactly once, a canary behind it, the old store unchanged
//                                       -> "GROW m N <root> <store>"
//   merklegrowcheck plans T_LOG NMAX    the plan of every 0 <= m <= N <= NMAX: "PLAN m N", "LAUNCH level steps n_in tiles tile0",
//   merklegrowcheck plan T_LOG M N      "ROW src dst count" (in nodes), "COPIED total"; T_LOG 2 .. 10
//   merklegrowcheck overlap A NA B NB   "OVERLAP 0|1": the byte ranges [A, A + NA) and [B, B + NB)
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/merkle_grow_kernels.cuh"

using eg::u32;
static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

typedef std::vector<u32> Words;      // rows of 8 little-endian words = 32 bytes
static const u32 CANARY = 0xC0FFEE11u, JUNK = 0xBADC0DE5u;
static void put_hex(const u32* w, size_t words) {
  for (size_t i = 0; i < words; ++i) printf("%02x%02x%02x%02x", w[i] & 255u, (w[i] >> 8) & 255u, (w[i] >> 16) & 255u, w[i] >> 24);
}
static bool read_leaves(const char* path, Words& log) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return false; }
  char buf[256];
  while (fscanf(f, "%255s", buf) == 1) {
    if (strlen(buf) != 64) { fprintf(stderr, "a leaf is 64 hex digits\n"); fclose(f); return false; }
    for (int i = 0; i < 8; ++i) {
      u32 w = 0;
      for (int b = 0; b < 4; ++b) { unsigned v = 0; sscanf(buf + 8 * i + 2 * b, "%2x", &v); w |= (u32)v << (8 * b); }
      log.push_back(w);
    }
  }
  fclose(f);
  return true;
}
// the node store over the first n leaves, level by level with the promotion rule: the OLD store of a case (none of the code under test)
static void build_store(const Words& log, uint64_t n, Words& store) {
  store.clear();
  Words cur(log.begin(), log.begin() + n * 8);
  while (cur.size() > 8) {
    const size_t count = cur.size() / 8;
    Words next;
    for (size_t i = 0; i < (count + 1) / 2; ++i) {
      u32 h[8];
      if (2 * i + 1 < count) eg::merkle_node(h, &cur[16 * i], &cur[16 * i + 8]);
      else memcpy(h, &cur[16 * i], 32);
      next.insert(next.end(), h, h + 8);
    }
    store.insert(store.end(), next.begin(), next.end());
    cur.swap(next);
  }
  CHECK(store.size() == egm::nodes_total(n) * 8, "the store of %" PRIu64 " leaves has %zu words", n, store.size());
}

// the new store with a count of the writes to every word
struct NewStore {
  Words words;                   // nodes_total(N) x 8, then the canary
  std::vector<unsigned char> hits;
  void put(uint64_t word, u32 v) {
    CHECK(word < hits.size(), "word %" PRIu64 " of a store of %zu", word, hits.size());
    if (word >= hits.size()) return;
    words[word] = v;
    if (hits[word] < 255) ++hits[word];
  }
};
struct CopyArr {
  const u32* old_;               // an allocation of its own: poisoned where it must not be read
  uint64_t old_nodes;
  NewStore* out;
  uint64_t moved;
  void move16(uint64_t s, uint64_t d, u32 half) {
    CHECK(s < old_nodes && half < 2, "node %" PRIu64 " of an old store of %" PRIu64, s, old_nodes);
    for (u32 i = 0; i < 4; ++i) out->put(d * 8 + half * 4 + i, old_[s * 8 + half * 4 + i]);
    moved += 4;
  }
  void move4(uint64_t s, uint64_t d, u32 word) {
    CHECK(s < old_nodes && word < 8, "node %" PRIu64 " of an old store of %" PRIu64, s, old_nodes);
    out->put(d * 8 + word, old_[s * 8 + word]);
    moved += 1;
  }
};
template <int TL>
struct GrowTileArr {
  const u32* log;                // level 0: an allocation of its own, poisoned below the first tile that is read
  const egm::GrowLaunch* g;
  uint64_t in_off;               // where the input level starts in the new store (level >= 1)
  NewStore* out_;
  Words odd, even;
  void in(uint64_t i, u32 w[8]) const {
    CHECK(i >= (g->tile0 << TL) && i < g->n_in, "input node %" PRIu64 " of level %d", i, g->level);
    for (int k = 0; k < 8; ++k) w[k] = g->level ? out_->words.at((in_off + i) * 8 + k) : log[i * 8 + k];
    if (g->level) for (int k = 0; k < 8; ++k) CHECK(out_->hits.at((in_off + i) * 8 + k) == 1, "input node %" PRIu64 " of level %d is not there yet", i, g->level);
  }
  void lds_get(int parity, u32 local, u32 w[8]) const {
    const Words& buf = parity ? odd : even;
    const u32 rows = parity ? 1u << (TL - 1) : 1u << (TL - 2);
    for (int i = 0; i < 8; ++i) w[i] = buf.at(i * rows + local);
  }
  void lds_put(int parity, u32 local, const u32 w[8]) {
    Words& buf = parity ? odd : even;
    const u32 rows = parity ? 1u << (TL - 1) : 1u << (TL - 2);
    CHECK(local < rows, "LDS row %u of %u", local, rows);
    for (int i = 0; i < 8; ++i) buf.at(i * rows + local) = w[i];
  }
  void out(int s, uint64_t node, const u32 w[8]) {
    for (int i = 0; i < 8; ++i) out_->put((g->off[s - 1] + node) * 8 + i, w[i]);
  }
};
// what eg_merkle_grow_device does, with the launches as loops: the copy, the tile launches bottom-up, the root
template <int TL>
static void grow(uint64_t m, const u32* old_store, uint64_t n, const u32* log, bool wide, NewStore& ns, u32 root[8]) {
  const uint64_t total = egm::nodes_total(n);
  ns.words.assign(total * 8 + 8, CANARY);
  ns.hits.assign(total * 8, 0);
  const egm::GrowPlan P = egm::grow_plan(m, n, TL);
  CopyArr cm{old_store, egm::nodes_total(m), &ns, 0};
  const uint64_t units = P.table.total * (wide ? 2u : 8u);
  for (uint64_t u = units + 3; u-- > 0;) eg::merkle_lane_grow_copy(cm, P.table, u, wide);      // lanes in reverse order, three past the end
  CHECK(cm.moved == P.table.total * 8, "%" PRIu64 " words moved for %" PRIu64 " nodes", cm.moved, P.table.total);
  uint64_t in_off = 0;
  for (int k = 0; k < P.n_launches; ++k) {
    const egm::GrowLaunch& g = P.launch[k];
    for (uint64_t tile = g.tiles; tile-- > g.tile0;) {                    // tiles in reverse order: they are independent
      GrowTileArr<TL> mem{log, &g, in_off, &ns, Words(8u << (TL - 1), 0xABABABABu), Words(8u << (TL - 2), 0xABABABABu)};
      for (int s = 1; s <= g.steps; ++s)
        for (u32 t = 1u << (TL - 1); t-- > 0;) eg::merkle_tile_step<TL>(mem, tile, s, t, g.n_in);
    }
    in_off = g.off[g.steps - 1];
  }
  if (n == 0) eg::merkle_empty_root(root);
  else if (n == 1) memcpy(root, log, 32);
  else memcpy(root, &ns.words.at((total - 1) * 8), 32);
  for (int i = 0; i < 8; ++i) CHECK(ns.words.at(total * 8 + i) == CANARY, "(%" PRIu64 ", %" PRIu64 "): written behind the store", m, n);
  for (uint64_t i = 0; i < total * 8; ++i)
    if (ns.hits[i] != 1) { CHECK(false, "(%" PRIu64 ", %" PRIu64 "): word %" PRIu64 " of the store written %u times", m, n, i, ns.hits[i]); break; }
}
template <int TL>
static int cmd_grow(const char* path) {
  Words log;
  if (!read_leaves(path, log)) return 2;
  const uint64_t count = log.size() / 8;
  for (uint64_t m = 0; m <= count; ++m) {
    Words built;
    build_store(log, m, built);
    const uint64_t old_nodes = egm::nodes_total(m);
    // the old store in an allocation of its own; its ragged and promoted nodes are junk, and poisoned while the pass runs
    std::unique_ptr<u32[]> old_store(new u32[old_nodes * 8 + 8]), old_copy(new u32[old_nodes * 8 + 8]);
    if (old_nodes) memcpy(old_store.get(), built.data(), old_nodes * 32);
    std::vector<uint64_t> ragged;
    for (int level = 1; level <= egm::depth(m); ++level)
      for (uint64_t j = m >> level; j < egm::level_count(m, level); ++j) ragged.push_back(egm::level_offset(m, level) + j);
    for (uint64_t node : ragged) for (int i = 0; i < 8; ++i) old_store[node * 8 + i] = JUNK + (u32)node;
    memcpy(old_copy.get(), old_store.get(), old_nodes * 32);
    for (uint64_t n = m; n <= count; ++n) {
      const uint64_t first = (m >> TL) << TL;                             // leaves below are never read
      std::unique_ptr<u32[]> own(new u32[n * 8 + 8]);
      memcpy(own.get(), log.data(), n * 32);
      for (uint64_t i = 0; i < first * 8; ++i) own[i] = JUNK ^ (u32)i;
      for (uint64_t node : ragged) ASAN_POISON_MEMORY_REGION(old_store.get() + node * 8, 32);
      ASAN_POISON_MEMORY_REGION(own.get(), first * 32);
      NewStore wide, narrow;
      u32 root[8], root2[8];
      grow<TL>(m, old_store.get(), n, own.get(), true, wide, root);
      grow<TL>(m, old_store.get(), n, own.get(), false, narrow, root2);
      ASAN_UNPOISON_MEMORY_REGION(own.get(), first * 32);
      for (uint64_t node : ragged) ASAN_UNPOISON_MEMORY_REGION(old_store.get() + node * 8, 32);
      CHECK(wide.words == narrow.words && memcmp(root, root2, 32) == 0, "(%" PRIu64 ", %" PRIu64 "): the two widths of the copy differ", m, n);
      CHECK(memcmp(old_store.get(), old_copy.get(), old_nodes * 32) == 0, "(%" PRIu64 ", %" PRIu64 "): the old store changed", m, n);
      printf("GROW %" PRIu64 " %" PRIu64 " ", m, n); put_hex(root, 8); printf(" "); put_hex(wide.words.data(), egm::nodes_total(n) * 8); printf("\n");
    }
  }
  return 0;
}

static void put_plan(uint64_t m, uint64_t n, int t_log) {
  const egm::GrowPlan P = egm::grow_plan(m, n, t_log);
  printf("PLAN %" PRIu64 " %" PRIu64 "\n", m, n);
  CHECK(P.n_launches <= egm::GROW_LAUNCHES_MAX && P.table.n_rows <= (u32)egm::GROW_ROWS_MAX, "%d launches, %u rows", P.n_launches, P.table.n_rows);
  for (int k = 0; k < P.n_launches; ++k) {
    const egm::GrowLaunch& g = P.launch[k];
    printf("LAUNCH %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g.level, g.steps, g.n_in, g.tiles, g.tile0);
    for (int s = 1; s <= g.steps; ++s) CHECK(g.off[s - 1] == egm::level_offset(n, g.level + s), "offset of level %d", g.level + s);
  }
  for (u32 r = 0; r < P.table.n_rows; ++r) printf("ROW %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", P.table.row[r].src, P.table.row[r].dst, P.table.row[r].count);
  printf("COPIED %" PRIu64 "\n", P.table.total);
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 4 && strcmp(argv[1], "grow") == 0) {
    const int tl = atoi(argv[2]);
    if (tl == 2) rc = cmd_grow<2>(argv[3]);
    else if (tl == 3) rc = cmd_grow<3>(argv[3]);
    else { fprintf(stderr, "T_LOG is 2 or 3\n"); return 2; }
  } else if (argc == 4 && strcmp(argv[1], "plans") == 0) {
    const int tl = atoi(argv[2]);
    if (tl < 2 || tl > egm::T_LOG) { fprintf(stderr, "T_LOG is 2 .. 10\n"); return 2; }
    const uint64_t nmax = strtoull(argv[3], nullptr, 10);
    for (uint64_t n = 0; n <= nmax; ++n)
      for (uint64_t m = 0; m <= n; ++m) put_plan(m, n, tl);
  } else if (argc == 5 && strcmp(argv[1], "plan") == 0) {
    const int tl = atoi(argv[2]);
    const uint64_t m = strtoull(argv[3], nullptr, 10), n = strtoull(argv[4], nullptr, 10);
    if (tl < 2 || tl > egm::T_LOG || m > n || n >= egm::LEAVES_MAX) { fprintf(stderr, "T_LOG is 2 .. 10, M <= N < 2^31\n"); return 2; }
    put_plan(m, n, tl);
  } else if (argc == 6 && strcmp(argv[1], "overlap") == 0) {
    printf("OVERLAP %d\n", egm::ranges_overlap(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10),
                                              strtoull(argv[5], nullptr, 10)) ? 1 : 0);
  } else {
    fprintf(stderr, "usage: merklegrowcheck grow T_LOG FILE | plans T_LOG NMAX | plan T_LOG M N | overlap A NA B NB\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
