// Host build of the receipt log's audit entries (elastic_elgamal_amd/csrc/merkle_audit_kernels.cuh, merkle_audit_host.hpp) under ASan +
// UBSan: the lane functions of the heads / consistency / consistency-check kernels run serially on arrays; every array access is
// bounds-checked and the proof bytes of a check with a wrong length or a bad old size are poisoned, so that reading them aborts the
// program.  Stand-alone program (tests/test_merkle_audit_cpu.py builds it and reads its report):
//   merkleauditcheck audit FILE      lines of leaves (hex); for every N = 0 .. their number, over the node store of the first N:
//                                    "HEAD N s <head>" for every size s = 0 .. N + 1, "PROOF N m len <row>" for every old size m = 0 ..
//                                    N + 1 (a canary behind the rows), then the check lanes over the honest proof, every wrong proof_len,
//                                    a flipped bit in every entry, in the old root and in the new root, the proof of (m, N - 1) offered
//                                    at N, old sizes 0 and N + 1 -> "VERDICTS proven bad_index bad_length mismatch mismatch_old"
//   merkleauditcheck len M N         "LEN <eg_merkle_consistency_len>"
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/merkle_audit_kernels.cuh"

using eg::u32;
static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

typedef std::vector<u32> Words;      // rows of 8 little-endian words = 32 bytes
static const u32 CANARY = 0xC0FFEE11u;
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
// the node store over the first n leaves, level by level with the promotion rule; the root
static void build_store(const Words& log, uint64_t n, Words& store, u32 root[8]) {
  store.clear();
  if (n == 0) { eg::merkle_empty_root(root); return; }
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
  memcpy(root, cur.data(), 32);
  CHECK(store.size() == egm::nodes_total(n) * 8, "the store of %" PRIu64 " leaves has %zu words", n, store.size());
}

struct NodeArr {
  const Words* log;
  const Words* store;
  uint64_t n;
  void node(int level, uint64_t off, uint64_t idx, u32 w[8]) const {
    CHECK(idx < egm::level_count(n, level) && (level == 0 || off == egm::level_offset(n, level)), "node %" PRIu64 " of level %d", idx, level);
    for (int i = 0; i < 8; ++i) w[i] = level ? store->at((off + idx) * 8 + i) : log->at(idx * 8 + i);
  }
};
struct HeadArr : NodeArr {
  const std::vector<uint64_t>* sizes;
  Words* heads;
  uint64_t size(uint64_t j) const { return sizes->at(j); }
  void head_put(uint64_t j, const u32 w[8]) { for (int i = 0; i < 8; ++i) heads->at(j * 8 + i) = w[i]; }
  void head_zero(uint64_t j) { for (int i = 0; i < 8; ++i) heads->at(j * 8 + i) = 0u; }
};
struct ConsArr : NodeArr {
  Words* proofs;
  size_t stride_words;
  void proof_put(uint64_t j, u32 k, const u32 w[8]) {
    CHECK(k * 8 + 8 <= stride_words, "entry %u of a row of %zu words", k, stride_words);
    for (int i = 0; i < 8; ++i) proofs->at(j * stride_words + k * 8 + i) = w[i];
  }
  void proof_zero(uint64_t j, u32 k) { for (int i = 0; i < 8; ++i) proofs->at(j * stride_words + k * 8 + i) = 0u; }
};
struct ConsCheckArr {
  uint64_t old_;
  const u32* old_root_;
  const u32* proof_;             // an allocation of its own: poisoned where it must not be read
  u32 len;
  const u32* root_;
  uint64_t old_size(uint64_t) const { return old_; }
  u32 proof_len(uint64_t) const { return len; }
  void old_root(uint64_t, u32 w[8]) const { memcpy(w, old_root_, 32); }
  void proof(uint64_t, u32 k, u32 w[8]) const { for (int i = 0; i < 8; ++i) w[i] = proof_[k * 8 + i]; }
  void root(u32 w[8]) const { memcpy(w, root_, 32); }
};

static int cmd_audit(const char* file) {
  Words log;
  if (!read_leaves(file, log)) return 2;
  unsigned long long count[5] = {0, 0, 0, 0, 0};                          // by verdict
  Words prev_rows;                                                        // the proofs of the tree of N - 1 leaves
  std::vector<u32> prev_len;
  size_t prev_stride = 0;
  for (uint64_t n = 0; n <= log.size() / 8; ++n) {
    Words store;
    u32 root[8];
    build_store(log, n, store, root);
    const int depth = egm::depth(n);
    const size_t row = egm::consistency_row(n), stride = 8 * row;
    CHECK(row == (size_t)depth + 1, "row of %zu entries", row);
    // heads of every size 0 .. N + 1, lanes in reverse order
    std::vector<uint64_t> sizes;
    for (uint64_t s = 0; s <= n + 1; ++s) sizes.push_back(s);
    Words heads((n + 2) * 8 + 8, CANARY);
    HeadArr hm{{&log, &store, n}, &sizes, &heads};
    unsigned above = 0;
    for (uint64_t j = n + 2; j-- > 0;) above += eg::merkle_lane_head(hm, j, n) ? 1u : 0u;
    CHECK(above == 1, "%u sizes above N", above);
    for (int i = 0; i < 8; ++i) CHECK(heads.at((n + 2) * 8 + i) == CANARY, "written behind the heads");
    CHECK(memcmp(&heads[n * 8], root, 32) == 0, "the head of size N = %" PRIu64 " is not the root", n);
    for (uint64_t s = 0; s <= n + 1; ++s) { printf("HEAD %" PRIu64 " %" PRIu64 " ", n, s); put_hex(&heads[s * 8], 8); printf("\n"); }
    // proofs of every old size 0 .. N + 1
    Words rows((n + 2) * stride + 8, 0x5A5A5A5Au);
    std::vector<u32> lens(n + 2);
    ConsArr cm{{&log, &store, n}, &rows, stride};
    for (uint64_t m = n + 2; m-- > 0;) lens[m] = eg::merkle_lane_consistency(cm, m, m, n, (int)row);
    for (int i = 0; i < 8; ++i) CHECK(rows.at((n + 2) * stride + i) == 0x5A5A5A5Au, "written behind the proofs");
    for (uint64_t m = 0; m <= n + 1; ++m) {
      printf("PROOF %" PRIu64 " %" PRIu64 " %u ", n, m, lens[m]); put_hex(&rows[m * stride], stride); printf("\n");
      CHECK(lens[m] == egm::consistency_len(m, n), "length %u of (%" PRIu64 ", %" PRIu64 ")", lens[m], m, n);
      // the proof in an allocation of its own, three entries longer than the row so that every wrong length has bytes to poison
      const size_t own_words = stride + 24;
      std::unique_ptr<u32[]> own(new u32[own_words]);
      memset(own.get(), 0, own_words * 4);
      memcpy(own.get(), &rows[m * stride], stride * 4);
      u32 old_root[8] = {0};
      if (m <= n) memcpy(old_root, &heads[m * 8], 32);
      ConsCheckArr km{m, old_root, own.get(), lens[m], root};
      u32 v;
      if (m == 0 || m > n) {
        CHECK(lens[m] == egm::NO_PATH, "old size %" PRIu64 " of %" PRIu64 " has a proof", m, n);
        ASAN_POISON_MEMORY_REGION(own.get(), own_words * 4);
        for (u32 l : {0u, 1u, (u32)row, egm::NO_PATH}) { km.len = l; v = eg::merkle_lane_cons_check(km, 0, n); CHECK(v == egm::MERKLE_BAD_INDEX, "verdict %u", v); ++count[v < 5 ? v : 0]; }
        ASAN_UNPOISON_MEMORY_REGION(own.get(), own_words * 4);
        continue;
      }
      const u32 len = lens[m];
      CHECK(len <= (u32)row, "proof length %u", len);
      v = eg::merkle_lane_cons_check(km, 0, n);
      CHECK(v == 0, "(%" PRIu64 ", %" PRIu64 ") is not proven: %u", m, n, v); ++count[v < 5 ? v : 0];
      ASAN_POISON_MEMORY_REGION(own.get(), own_words * 4);
      for (u32 l = 0; l <= (u32)row + 2; ++l) {
        if (l == len) continue;
        km.len = l; v = eg::merkle_lane_cons_check(km, 0, n);
        CHECK(v == egm::MERKLE_BAD_LENGTH, "length %u for %u: verdict %u", l, len, v); ++count[v < 5 ? v : 0];
      }
      km.len = egm::NO_PATH; v = eg::merkle_lane_cons_check(km, 0, n); CHECK(v == egm::MERKLE_BAD_LENGTH, "verdict %u", v); ++count[v < 5 ? v : 0];
      ASAN_UNPOISON_MEMORY_REGION(own.get(), own_words * 4);
      km.len = len;
      for (u32 k = 0; k < len; ++k) {                                     // which of the two mismatches: the model says
        own[k * 8 + (m + k) % 8] ^= 1u << ((m + 7 * k) % 32);
        v = eg::merkle_lane_cons_check(km, 0, n);
        CHECK(v == egm::MERKLE_MISMATCH || v == egm::MERKLE_MISMATCH_OLD, "flipped entry %u: %u", k, v); ++count[v < 5 ? v : 0];
        own[k * 8 + (m + k) % 8] ^= 1u << ((m + 7 * k) % 32);
      }
      u32 bent[8];
      memcpy(bent, old_root, 32); bent[m % 8] ^= 1u << (n % 32);
      km.old_root_ = bent; v = eg::merkle_lane_cons_check(km, 0, n); km.old_root_ = old_root;
      CHECK(v == egm::MERKLE_MISMATCH || v == egm::MERKLE_MISMATCH_OLD, "flipped old root: %u", v); ++count[v < 5 ? v : 0];
      memcpy(bent, root, 32); bent[(m + 3) % 8] ^= 0x80000000u >> (m % 32);
      km.root_ = bent; v = eg::merkle_lane_cons_check(km, 0, n); km.root_ = root;
      CHECK(v == egm::MERKLE_MISMATCH, "flipped root: %u", v); ++count[v < 5 ? v : 0];
      v = eg::merkle_lane_cons_check(km, 0, n); CHECK(v == 0, "restored proof: %u", v);
      if (m < n) {                                                        // the proof that was issued for the tree of N - 1 leaves
        memset(own.get(), 0, own_words * 4);
        memcpy(own.get(), &prev_rows[m * prev_stride], prev_stride * 4);
        km.len = prev_len[m];
        v = eg::merkle_lane_cons_check(km, 0, n);
        CHECK(v != 0, "the proof of (%" PRIu64 ", %" PRIu64 ") proves at N", m, n - 1); ++count[v < 5 ? v : 0];
      }
    }
    prev_rows.swap(rows); prev_len.swap(lens); prev_stride = stride;
  }
  printf("VERDICTS %llu %llu %llu %llu %llu\n", count[0], count[1], count[2], count[3], count[4]);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && strcmp(argv[1], "audit") == 0) {
    rc = cmd_audit(argv[2]);
  } else if (argc == 4 && strcmp(argv[1], "len") == 0) {
    printf("LEN %u\n", egm::consistency_len(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10)));
  } else {
    fprintf(stderr, "usage: merkleauditcheck audit FILE | len M N\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
