// Host build of ballot weeding (elastic_elgamal_amd/csrc/weed_kernels.cuh, weed_host.hpp) under ASan + UBSan: the lane functions of the
// insert / lookup kernels run serially on arrays, in any lane order, with any table size; every array access is bounds-checked, and the
// bytes of ballots that do not participate are poisoned, so reading them aborts the program.
// Stand-alone program (tests/test_weed_cpu.py builds it and reads its report):
//   weedcheck run FILE SLOTS SEED ORDER   the whole pass over the case of FILE; SLOTS 0 = the library's table size, ORDER 0 = lanes in
//                                         index order, else the seed of a shuffle
//   weedcheck layout N N_PRIOR K          table slots and the parts of the scratch
//   weedcheck addr B STRIDE ITEM          byte offset of a key
//   weedcheck items                       adjacency of the R and B items for six election shapes
//   weedcheck refuse N N_PRIOR CAP K      what the argument rules say
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/host_plan.hpp"
#include "../../elastic_elgamal_amd/csrc/group_tally_host.hpp"
#include "../../elastic_elgamal_amd/csrc/weed_kernels.cuh"

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct TableArr {
  std::vector<uint64_t> slots;
  uint64_t peek(uint64_t i) const { return slots.at(i); }
  uint64_t claim(uint64_t i, uint64_t ref) { const uint64_t old = slots.at(i); if (old == egw::EMPTY) slots.at(i) = ref; return old; }
  void lower(uint64_t i, uint64_t ref) { if (ref < slots.at(i)) slots.at(i) = ref; }
};
// every ballot in an allocation of its own: key k is item 1 + 2 k of a ballot of 2 K + 1 items
struct KeysArr {
  const std::vector<std::unique_ptr<uint8_t[]>>* ballots;
  const std::vector<uint8_t>* board;
  uint64_t stride;
  uint32_t K;
  static uint32_t r_item(uint32_t k) { return 1u + 2u * k; }
  void load(uint32_t w[16], uint64_t ref) const {
    const uint8_t* p;
    if (egw::is_board_ref(ref)) {
      (void)board->at(ref * 64 + 63);
      p = board->data() + ref * 64;
    } else {
      p = ballots->at(egw::ref_ballot(ref, K)).get() + egw::key_offset(0, stride, r_item(egw::ref_key(ref, K)));
    }
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  }
};

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static bool unhex(uint8_t* out, const char* s, size_t bytes) {
  if (strlen(s) != 2 * bytes) return false;
  for (size_t i = 0; i < bytes; ++i) {
    const int a = hexval(s[2 * i]), b = hexval(s[2 * i + 1]);
    if (a < 0 || b < 0) return false;
    out[i] = (uint8_t)(a * 16 + b);
  }
  return true;
}
static void print_hex(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", p[i]); }

// FILE: "n K n_prior board_cap", n_prior lines "hex(64)", n lines "status hex(64 K)" (the hex of a ballot that does not participate is ignored)
static int cmd_run(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  const uint64_t want_slots = strtoull(argv[3], nullptr, 10), seed = strtoull(argv[4], nullptr, 10), order = strtoull(argv[5], nullptr, 10);
  unsigned long long n = 0, K = 0, n_prior = 0, board_cap = 0;
  if (fscanf(f, "%llu %llu %llu %llu", &n, &K, &n_prior, &board_cap) != 4 || K == 0) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  if (const char* why = egw::refuse(n, n_prior, board_cap)) { fprintf(stderr, "refused: %s\n", why); fclose(f); return 2; }
  const uint64_t stride = 32 * (2 * K + 1);
  std::vector<uint8_t> board(board_cap * 64, 0xEE);
  std::vector<char> line(128 * K + 64);
  for (uint64_t j = 0; j < n_prior; ++j)
    if (fscanf(f, "%s", line.data()) != 1 || !unhex(board.data() + 64 * j, line.data(), 64)) { fprintf(stderr, "bad board line\n"); fclose(f); return 2; }
  std::vector<uint32_t> status(n);
  std::vector<std::unique_ptr<uint8_t[]>> ballots;
  std::vector<uint8_t> keys(64 * K);
  for (uint64_t b = 0; b < n; ++b) {
    if (fscanf(f, "%u %s", &status[b], line.data()) != 2) { fprintf(stderr, "bad ballot line\n"); fclose(f); return 2; }
    ballots.emplace_back(new uint8_t[stride]);
    memset(ballots.back().get(), 0xA5, stride);
    if (status[b] == 0u) {
      if (!unhex(keys.data(), line.data(), 64 * K)) { fprintf(stderr, "bad ballot hex\n"); fclose(f); return 2; }
      for (uint32_t k = 0; k < K; ++k) memcpy(ballots.back().get() + 32 * KeysArr::r_item(k), keys.data() + 64 * k, 64);
    } else {
      ASAN_POISON_MEMORY_REGION(ballots.back().get(), stride);          // never read
    }
  }
  fclose(f);
  const egw::Layout L = egw::layout(n, n_prior, (uint32_t)K);
  const uint64_t slots = want_slots ? want_slots : L.slots;
  CHECK((slots & (slots - 1)) == 0, "slots is no power of two");
  TableArr tab{std::vector<uint64_t>(slots, egw::EMPTY)};
  const KeysArr io{&ballots, &board, stride, (uint32_t)K};

  // insert: every lane of k_weed_insert, in index order or shuffled
  std::vector<uint64_t> lanes;
  for (uint64_t j = 0; j < n_prior + n * K; ++j) lanes.push_back(j);
  if (order) { std::mt19937_64 rng(order); std::shuffle(lanes.begin(), lanes.end(), rng); }
  uint32_t found[3] = {0, 0, 0};
  for (uint64_t j : lanes) {
    uint64_t ref = j;
    if (j >= n_prior) {
      const uint64_t idx = j - n_prior;
      if (status[idx / K] != 0u) continue;
      ref = egw::BATCH_BASE + idx;
      CHECK(ref == egw::batch_ref(idx / K, (uint32_t)K, (uint32_t)(idx % K)), "reference of lane %" PRIu64, j);
    }
    if (!egw::weed_lane_insert(tab, io, slots, seed, ref)) ++found[2];
  }
  uint64_t used = 0;
  for (uint64_t v : tab.slots) used += v != egw::EMPTY;
  // lookup: every lane of k_weed_lookup
  std::vector<uint32_t> dup(n), out(n), pos(n);
  for (uint64_t b = 0; b < n; ++b) {
    const bool part = status[b] == 0u;
    bool missing = false;
    dup[b] = part ? egw::weed_lane_ballot(tab, io, slots, seed, b, (uint32_t)K, missing) : egw::DUP_NONE;
    out[b] = egw::weed_status_out(status[b], dup[b]);
    pos[b] = part && dup[b] == egw::DUP_NONE ? 1u : 0u;
    found[0] += dup[b] == egw::DUP_PRIOR;
    found[1] += dup[b] != egw::DUP_NONE && dup[b] != egw::DUP_PRIOR;
    found[2] += missing;
  }
  // append: scan, fit check, copy (every lane of k_weed_copy)
  const uint32_t kept = egw::scan_keep(pos);
  const bool fits = egw::append_fits(n_prior, kept, (uint32_t)K, board_cap);
  if (!fits) ++found[2];
  if (fits)
    for (uint64_t j = 0; j < n * K * 4; ++j) {
      const uint64_t b = j / (4 * K);
      const uint32_t r = (uint32_t)(j % (4 * K)), k = r >> 2, q = r & 3u;
      if (pos[b] == 0xffffffffu) continue;
      const uint64_t entry = egw::weed_append_entry(n_prior, pos[b], (uint32_t)K, k);
      for (int i = 0; i < 16; ++i) board.at(entry * 64 + 16 * q + i) = ballots.at(b)[egw::key_offset(0, stride, KeysArr::r_item(k)) + 16 * q + i];
    }
  const uint64_t count = n_prior + (fits ? (uint64_t)kept * K : 0);
  printf("SLOTS %" PRIu64 " USED %" PRIu64 "\nDUP :", slots, used);
  for (uint32_t d : dup) printf(" %u", d);
  printf("\nSTATUS :");
  for (uint32_t s : out) printf(" %u", s);
  printf("\nFOUND %u %u %u\nCOUNT %" PRIu64 "\nBOARD ", found[0], found[1], found[2], count);
  print_hex(board.data(), board.size());
  printf("\n");
  return 0;
}

static void print_items(const char* name, const eghost::Plan& P) {
  const std::vector<uint32_t> items = eggt::tally_items(P.pt_items, P.tally_slots);
  std::vector<uint32_t> r_items;
  const bool ok = egw::key_items(r_items, items);
  printf("ITEMS %s stride %zu adjacent %d :", name, (size_t)P.stride, ok ? 1 : 0);
  for (uint32_t it : r_items) printf(" %u", it);
  printf("\n");
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 6 && strcmp(argv[1], "run") == 0) {
    rc = cmd_run(argv);
  } else if (argc == 5 && strcmp(argv[1], "layout") == 0) {
    const egw::Layout L = egw::layout(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10));
    printf("LAYOUT slots %" PRIu64 " tiles %u table %zu pos %zu tile_sums %zu total_word %zu total %zu\n", L.slots, L.n_tiles, L.table, L.pos, L.tiles,
           L.total_word, L.total);
  } else if (argc == 5 && strcmp(argv[1], "addr") == 0) {
    printf("ADDR %" PRIu64 "\n", egw::key_offset(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10)));
  } else if (argc == 2 && strcmp(argv[1], "items") == 0) {
    print_items("single2", eghost::build_choice_plan(2, true));
    print_items("single5", eghost::build_choice_plan(5, true));
    print_items("single150", eghost::build_choice_plan(150, true));
    print_items("multi16", eghost::build_choice_plan(16, false));
    print_items("qv5_20", eghost::build_qv_plan(5, 20));
    print_items("qv3_10000", eghost::build_qv_plan(3, 10000));
    std::vector<uint32_t> r;
    CHECK(!egw::key_items(r, {4, 6}) && !egw::key_items(r, {4, 5, 8}) && !egw::key_items(r, {}) && egw::key_items(r, {4, 5, 9, 10}) && r.size() == 2,
          "key_items on hand-made plans");
  } else if (argc == 6 && strcmp(argv[1], "refuse") == 0) {
    const uint64_t n = strtoull(argv[2], nullptr, 10), n_prior = strtoull(argv[3], nullptr, 10), cap = strtoull(argv[4], nullptr, 10);
    const char* why = egw::refuse(n, n_prior, cap);
    if (!why) why = egw::refuse_keys(n, n_prior, (uint32_t)strtoul(argv[5], nullptr, 10));
    printf("REFUSE %s\n", why ? why : "-");
  } else {
    fprintf(stderr, "usage: weedcheck run FILE SLOTS SEED ORDER | layout N N_PRIOR K | addr B STRIDE ITEM | items | refuse N N_PRIOR CAP K\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
