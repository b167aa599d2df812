// Host build of the receipt log (elastic_elgamal_amd/csrc/merkle_kernels.cuh, merkle_host.hpp, sha512.cuh) under ASan + UBSan: the lane
// functions of the leaf / place / tile / paths / check kernels run serially on arrays; every array access is bounds-checked, the bytes of
// ballots that do not participate and the path bytes of receipts with a wrong length are poisoned, so that reading either aborts the
// program.  Stand-alone program (tests/test_merkle_cpu.py builds it and reads its report):
//   merklecheck node FILE            lines "L R" (64 hex digits each) -> "NODE <hex>"
//   merklecheck trees T_LOG FILE     lines of leaves (hex); for every N = 0 .. their number the tree over the first N with tiles of
//                                    2^T_LOG (4 or 8) -> "TREE N <root> <store>"; a canary behind the store
//   merklecheck receipts FILE        the same leaves: for every N and every i = 0 .. N + 1 "PATH N i len <path>"; the check lanes over
//                                    the honest receipt, every wrong path_len (path bytes poisoned), a flipped bit in leaf, path and root
//   merklecheck leaves FILE          groups "n msg_len extra_len n_prior log_cap prefix|-" followed by n lines "status msg extra|-" ->
//                                    "INDEX ..", "LEAVES ..", "LOG count ..", "FOUND a b" per group
//   merklecheck layout N             the parts of both scratches
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/merkle_kernels.cuh"

using eg::u32;
static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

typedef std::vector<u32> Words;      // rows of 8 little-endian words = 32 bytes
static std::vector<unsigned char> unhex(const char* s) {
  std::vector<unsigned char> out;
  if (strcmp(s, "-") == 0) return out;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) { unsigned v = 0; sscanf(s + i, "%2x", &v); out.push_back((unsigned char)v); }
  return out;
}
static void put_hex(const u32* w, size_t words) {
  for (size_t i = 0; i < words; ++i) printf("%02x%02x%02x%02x", w[i] & 255u, (w[i] >> 8) & 255u, (w[i] >> 16) & 255u, w[i] >> 24);
}
static void words_of(u32 w[8], const std::vector<unsigned char>& b) {
  for (int i = 0; i < 8; ++i) w[i] = (u32)b.at(4 * i) | (u32)b.at(4 * i + 1) << 8 | (u32)b.at(4 * i + 2) << 16 | (u32)b.at(4 * i + 3) << 24;
}
static bool read_leaves(const char* path, Words& log) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return false; }
  char buf[256];
  while (fscanf(f, "%255s", buf) == 1) { u32 w[8]; words_of(w, unhex(buf)); log.insert(log.end(), w, w + 8); }
  fclose(f);
  return true;
}

// ---- the tree over the first n leaves of `log`, in launches of T levels; the store ends in a canary -------------------------------------
static const u32 CANARY = 0xC0FFEE11u;
template <int TL>
struct TileArr {
  const Words* in_;
  Words* store;                  // null: no node store
  const uint64_t* off;
  Words* top;
  int steps;
  Words odd, even;
  void in(uint64_t g, u32 w[8]) const { for (int i = 0; i < 8; ++i) w[i] = in_->at(g * 8 + i); }
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
  void out(int s, uint64_t g, const u32 w[8]) {
    if (store) for (int i = 0; i < 8; ++i) store->at((off[s - 1] + g) * 8 + i) = w[i];
    else if (s == steps) for (int i = 0; i < 8; ++i) top->at(g * 8 + i) = w[i];
  }
};
// what eg_merkle_tree_device does, with the launches as loops; with_store false: the top levels go through two scratch buffers
template <int TL>
static void build_tree(const Words& log, uint64_t n, bool with_store, Words& store, u32 root[8]) {
  const int depth = egm::depth(n);
  store.assign(with_store ? egm::nodes_total(n) * 8 + 8 : 0, CANARY);
  if (n == 0) { eg::merkle_empty_root(root); return; }
  Words cur(log.begin(), log.begin() + n * 8), next;
  uint64_t n_in = n;
  for (int level = 0; level < depth;) {
    const int steps = depth - level < TL ? depth - level : TL;
    uint64_t off[TL];
    for (int s = 1; s <= steps; ++s) off[s - 1] = egm::level_offset(n, level + s);
    const uint64_t n_out = egm::level_count(n_in, steps);
    next.assign(n_out * 8, 0xDEADBEEFu);
    const uint64_t tiles = (n_in + (1u << TL) - 1) >> TL;
    for (uint64_t tile = tiles; tile-- > 0;) {                           // tiles in reverse order: they are independent
      TileArr<TL> mem{&cur, with_store ? &store : nullptr, off, &next, steps, Words(8u << (TL - 1), 0xABABABABu), Words(8u << (TL - 2), 0xABABABABu)};
      for (int s = 1; s <= steps; ++s)
        for (u32 t = 1u << (TL - 1); t-- > 0;) eg::merkle_tile_step<TL>(mem, tile, s, t, n_in);     // lanes in reverse order
    }
    if (with_store) next.assign(store.begin() + off[steps - 1] * 8, store.begin() + (off[steps - 1] + n_out) * 8);
    cur.swap(next);
    n_in = n_out;
    level += steps;
  }
  CHECK(n_in == 1 && cur.size() == 8, "the top level has %" PRIu64 " nodes", n_in);
  memcpy(root, cur.data(), 32);
}
template <int TL>
static int cmd_trees(const char* path) {
  Words log;
  if (!read_leaves(path, log)) return 2;
  for (uint64_t n = 0; n <= log.size() / 8; ++n) {
    Words store, none;
    u32 root[8], root2[8];
    build_tree<TL>(log, n, true, store, root);
    build_tree<TL>(log, n, false, none, root2);
    CHECK(memcmp(root, root2, 32) == 0, "N = %" PRIu64 ": the root without a store differs", n);
    const uint64_t total = egm::nodes_total(n);
    for (int i = 0; i < 8; ++i) CHECK(store.at(total * 8 + i) == CANARY, "N = %" PRIu64 ": written behind the store", n);
    for (uint64_t i = 0; i < total * 8; ++i) if (store[i] == CANARY) { CHECK(false, "N = %" PRIu64 ": word %" PRIu64 " of the store not written", n, i); break; }
    printf("TREE %" PRIu64 " ", n); put_hex(root, 8); printf(" "); put_hex(store.data(), total * 8); printf("\n");
  }
  return 0;
}

// ---- receipts ------------------------------------------------------------------------------------------------------------------------
struct PathArr {
  const Words* log;
  const Words* store;
  uint64_t n;
  Words* paths;
  size_t stride_words;
  void node(int level, uint64_t off, uint64_t idx, u32 w[8]) const {
    CHECK(idx < egm::level_count(n, level) && (level == 0 || off == egm::level_offset(n, level)), "node %" PRIu64 " of level %d", idx, level);
    for (int i = 0; i < 8; ++i) w[i] = level ? store->at((off + idx) * 8 + i) : log->at(idx * 8 + i);
  }
  void path_put(uint64_t j, u32 k, const u32 w[8]) { for (int i = 0; i < 8; ++i) paths->at(j * stride_words + k * 8 + i) = w[i]; }
  void path_zero(uint64_t j, u32 k) { for (int i = 0; i < 8; ++i) paths->at(j * stride_words + k * 8 + i) = 0u; }
};
struct CheckArr {
  uint64_t index_;
  const u32* leaf_;
  const u32* path_;              // an allocation of its own: poisoned where it must not be read
  u32 len;
  const u32* root_;
  uint64_t index(uint64_t) const { return index_; }
  u32 path_len(uint64_t) const { return len; }
  void leaf(uint64_t, u32 w[8]) const { memcpy(w, leaf_, 32); }
  void path(uint64_t, u32 k, u32 w[8]) const { for (int i = 0; i < 8; ++i) w[i] = path_[k * 8 + i]; }
  void root(u32 w[8]) const { memcpy(w, root_, 32); }
};
static int cmd_receipts(const char* file) {
  Words log;
  if (!read_leaves(file, log)) return 2;
  unsigned long long proven = 0, bad_index = 0, bad_length = 0, mismatch = 0;
  for (uint64_t n = 0; n <= log.size() / 8; ++n) {
    Words store;
    u32 root[8];
    build_tree<4>(log, n, true, store, root);
    const int depth = egm::depth(n);
    const size_t stride = 8 * (size_t)depth;
    Words paths((n + 2) * stride + 8, 0x5A5A5A5Au);
    PathArr pm{&log, &store, n, &paths, stride};
    for (uint64_t i = 0; i <= n + 1; ++i) {
      const u32 len = eg::merkle_lane_path(pm, i, i, n, depth);
      printf("PATH %" PRIu64 " %" PRIu64 " %u ", n, i, len); put_hex(paths.data() + i * stride, stride); printf("\n");
      // the path in an allocation of its own, one entry longer than depth so that every wrong length has bytes to poison
      std::unique_ptr<u32[]> own(new u32[stride + 16]);
      memcpy(own.get(), paths.data() + i * stride, stride * 4);
      u32 leaf[8] = {0};
      if (i < n) memcpy(leaf, log.data() + i * 8, 32);
      CheckArr cm{i, leaf, own.get(), len, root};
      if (i >= n) {
        CHECK(len == egm::NO_PATH, "index %" PRIu64 " of %" PRIu64 " has a path", i, n);
        ASAN_POISON_MEMORY_REGION(own.get(), (stride + 16) * 4);
        for (u32 l : {0u, 1u, (u32)depth, egm::NO_PATH}) { cm.len = l; const u32 v = eg::merkle_lane_check(cm, 0, n); CHECK(v == egm::MERKLE_BAD_INDEX, "verdict %u", v); ++bad_index; }
        ASAN_UNPOISON_MEMORY_REGION(own.get(), (stride + 16) * 4);
        continue;
      }
      CHECK(len == egm::path_len(i, n) && len <= (u32)depth, "path length %u", len);
      u32 v = eg::merkle_lane_check(cm, 0, n);
      CHECK(v == 0, "leaf %" PRIu64 " of %" PRIu64 " is not proven: %u", i, n, v); proven += v == 0;
      ASAN_POISON_MEMORY_REGION(own.get(), (stride + 16) * 4);
      for (u32 l = 0; l <= (u32)depth + 2; ++l) {
        if (l == len) continue;
        cm.len = l; v = eg::merkle_lane_check(cm, 0, n);
        CHECK(v == egm::MERKLE_BAD_LENGTH, "length %u for %u: verdict %u", l, len, v); ++bad_length;
      }
      cm.len = egm::NO_PATH; v = eg::merkle_lane_check(cm, 0, n); CHECK(v == egm::MERKLE_BAD_LENGTH, "verdict %u", v); ++bad_length;
      ASAN_UNPOISON_MEMORY_REGION(own.get(), (stride + 16) * 4);
      cm.len = len;
      leaf[i % 8] ^= 1u << (i % 32); v = eg::merkle_lane_check(cm, 0, n); CHECK(v == egm::MERKLE_MISMATCH, "flipped leaf: %u", v); leaf[i % 8] ^= 1u << (i % 32); ++mismatch;
      u32 bent[8]; memcpy(bent, root, 32); bent[(i + 3) % 8] ^= 0x80000000u >> (i % 32);
      cm.root_ = bent; v = eg::merkle_lane_check(cm, 0, n); CHECK(v == egm::MERKLE_MISMATCH, "flipped root: %u", v); cm.root_ = root; ++mismatch;
      for (u32 k = 0; k < len; ++k) {
        own[k * 8 + (i + k) % 8] ^= 1u << ((i + 7 * k) % 32);
        v = eg::merkle_lane_check(cm, 0, n); CHECK(v == egm::MERKLE_MISMATCH, "flipped path entry %u: %u", k, v); ++mismatch;
        own[k * 8 + (i + k) % 8] ^= 1u << ((i + 7 * k) % 32);
      }
      v = eg::merkle_lane_check(cm, 0, n); CHECK(v == 0, "restored receipt: %u", v);
    }
    for (int i = 0; i < 8; ++i) CHECK(paths.at((n + 2) * stride + i) == 0x5A5A5A5Au, "written behind the paths");
  }
  printf("VERDICTS %llu %llu %llu %llu\n", proven, bad_index, bad_length, mismatch);
  return 0;
}

// ---- the leaf pass -------------------------------------------------------------------------------------------------------------------
struct LeafArr {
  std::vector<std::unique_ptr<unsigned char[]>>* msgs;     // every message and extra in an allocation of its own
  std::vector<std::unique_ptr<unsigned char[]>>* extras;
  size_t msg_len, extra_len;
  const std::vector<unsigned char>* head;
  Words* rows;
  bool zero;
  Words* pos;
  eg::MerkleRanges ranges(uint64_t b) const {
    return eg::MerkleRanges{head->data(), msgs->at(b).get(), extra_len ? extras->at(b).get() : nullptr, head->size(), msg_len, extra_len};
  }
  void leaf_put(uint64_t b, const u32 w[8]) { for (int i = 0; i < 8; ++i) rows->at(b * 8 + i) = w[i]; }
  void leaf_zero(uint64_t b) { if (zero) for (int i = 0; i < 8; ++i) rows->at(b * 8 + i) = 0u; }
  void keep(uint64_t b, u32 flag) { pos->at(b) = flag; }
};
struct PlaceArr {
  const Words* pos;
  const Words* rows;
  std::vector<uint64_t>* leaf_index;
  Words* tail;
  u32 rank(uint64_t b) const { return pos->at(b); }
  void index_put(uint64_t b, uint64_t v) { leaf_index->at(b) = v; }
  u32 leaf_word(uint64_t b, u32 w) const { return rows->at(b * 8 + w); }
  void tail_put(uint64_t entry, u32 w, u32 v) { tail->at(entry * 8 + w) = v; }
};
static int cmd_leaves(const char* file) {
  FILE* f = fopen(file, "r");
  if (!f) { perror(file); return 2; }
  unsigned long long n, msg_len, extra_len, n_prior, log_cap;
  static char buf[8192];
  while (fscanf(f, "%llu %llu %llu %llu %llu %8191s", &n, &msg_len, &extra_len, &n_prior, &log_cap, buf) == 6) {
    std::vector<unsigned char> head(1, 0x00);
    const std::vector<unsigned char> prefix = unhex(buf);
    head.insert(head.end(), prefix.begin(), prefix.end());
    std::vector<std::unique_ptr<unsigned char[]>> msgs, extras;
    std::vector<u32> status(n);
    for (uint64_t b = 0; b < n; ++b) {
      if (fscanf(f, "%u %8191s", &status[b], buf) != 2) { fprintf(stderr, "bad item\n"); fclose(f); return 2; }
      const std::vector<unsigned char> m = unhex(buf);
      if (fscanf(f, "%8191s", buf) != 1) { fprintf(stderr, "bad item\n"); fclose(f); return 2; }
      const std::vector<unsigned char> e = unhex(buf);
      if (m.size() != msg_len || e.size() != extra_len) { fprintf(stderr, "bad lengths\n"); fclose(f); return 2; }
      msgs.emplace_back(new unsigned char[msg_len + 1]); if (msg_len) memcpy(msgs.back().get(), m.data(), msg_len);
      extras.emplace_back(new unsigned char[extra_len + 1]); if (extra_len) memcpy(extras.back().get(), e.data(), extra_len);
      if (status[b]) {                                                    // never read
        ASAN_POISON_MEMORY_REGION(msgs.back().get(), msg_len + 1);
        ASAN_POISON_MEMORY_REGION(extras.back().get(), extra_len + 1);
      }
    }
    if (const char* why = egm::refuse_messages(n, true, msg_len, msg_len, true, prefix.size(), true, extra_len, extra_len)) { printf("REFUSED %s\n", why); continue; }
    if (const char* why = egm::refuse_leaves(n, n_prior, true, true, true, true, log_cap)) { printf("REFUSED %s\n", why); continue; }
    const uint64_t room = log_cap - n_prior;
    for (int with_out = 0; with_out < 2; ++with_out) {                  // the leaves in the caller's leaves_out, or in the staging rows
      Words rows(n * 8, 0x77777777u), pos(n, 0xEEEEEEEEu), tail((room < n ? room : n) * 8 + 8, CANARY);
      std::vector<uint64_t> index(n, 0x1111111111111111ull);
      LeafArr lm{&msgs, &extras, (size_t)msg_len, (size_t)extra_len, &head, &rows, with_out != 0, &pos};
      for (uint64_t b = n; b-- > 0;) eg::merkle_lane_leaf(lm, b, status[b] == 0u);
      const u32 total = eg::merkle_scan_serial(pos.data(), n);
      const bool fits = egm::append_fits(n_prior, total, log_cap);
      PlaceArr pm{&pos, &rows, &index, &tail};
      for (uint64_t j = n * 8; j-- > 0;) eg::merkle_lane_place(pm, j >> 3, (u32)(j & 7u), n_prior, fits, room);
      const uint64_t appended = fits ? total : 0;
      for (uint64_t i = appended * 8; i < tail.size(); ++i) CHECK(tail[i] == CANARY, "written behind the appended leaves");
      if (!with_out) {
        for (uint64_t b = 0; b < n; ++b) if (status[b]) CHECK(rows[b * 8] == 0x77777777u, "staging row of ballot %" PRIu64 " written", b);
        continue;
      }
      printf("INDEX"); for (uint64_t b = 0; b < n; ++b) printf(" %" PRIu64, index[b]); printf("\n");
      printf("LEAVES "); put_hex(rows.data(), n * 8); printf("\n");
      printf("LOG %" PRIu64 " ", (uint64_t)n_prior + appended); put_hex(tail.data(), appended * 8); printf("\n");
      printf("FOUND %u %u\n", total, fits ? 0u : 1u);
    }
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && strcmp(argv[1], "node") == 0) {
    FILE* f = fopen(argv[2], "r");
    if (!f) { perror(argv[2]); return 2; }
    char a[128], b[128];
    while (fscanf(f, "%127s %127s", a, b) == 2) {
      u32 l[8], r[8], h[8], alias[8];
      words_of(l, unhex(a)); words_of(r, unhex(b));
      eg::merkle_node(h, l, r);
      memcpy(alias, l, 32); eg::merkle_node(alias, alias, r); CHECK(memcmp(alias, h, 32) == 0, "out = l");
      memcpy(alias, r, 32); eg::merkle_node(alias, l, alias); CHECK(memcmp(alias, h, 32) == 0, "out = r");
      printf("NODE "); put_hex(h, 8); printf("\n");
    }
    fclose(f);
  } else if (argc == 4 && strcmp(argv[1], "trees") == 0) {
    const int tl = atoi(argv[2]);
    if (tl == 2) rc = cmd_trees<2>(argv[3]);
    else if (tl == 3) rc = cmd_trees<3>(argv[3]);
    else { fprintf(stderr, "T_LOG is 2 (tiles of 4) or 3 (tiles of 8)\n"); return 2; }
  } else if (argc == 3 && strcmp(argv[1], "receipts") == 0) {
    rc = cmd_receipts(argv[2]);
  } else if (argc == 3 && strcmp(argv[1], "leaves") == 0) {
    rc = cmd_leaves(argv[2]);
  } else if (argc == 3 && strcmp(argv[1], "layout") == 0) {
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const egm::LeafLayout L = egm::leaf_layout(n);
    const egm::TreeLayout T = egm::tree_layout(n);
    printf("LEAF tiles %u head %zu pos %zu tile_sums %zu total_word %zu leaves %zu total %zu\n", L.n_tiles, L.head, L.pos, L.tiles, L.total_word, L.leaves, L.total);
    printf("TREE ping %zu pong %zu total %zu\n", T.ping, T.pong, T.total);
  } else {
    fprintf(stderr, "usage: merklecheck node FILE | trees T_LOG FILE | receipts FILE | leaves FILE | layout N\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
