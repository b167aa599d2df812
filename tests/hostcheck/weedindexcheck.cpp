// Host build of weeding against a persistent board index (elastic_elgamal_amd/csrc/weed_index_kernels.cuh, weed_index_host.hpp) under
// ASan + UBSan: the lane functions of k_weed_insert / k_weed_lookup_indexed / k_weed_index_add / k_weed_index_find run serially on
// arrays, in any lane order, with any slot count; every array access is bounds-checked, the Keys adapters refuse references at or above
// their bound exactly as WeedKeysDev::at does, and the bytes of ballots that do not participate are poisoned.
// Stand-alone program (tests/test_weed_index_cpu.py builds it and reads its report):
//   weedindexcheck seq FILE INDEX_SEED ORDER   a sequence of batches over one growing board: every batch through the indexed lanes AND through
//                                              the stateless lanes over the same board bytes (compared here), a read-only pass in front of
//                                              every appending one, and after the sequence find() over the maintained index against a freshly
//                                              built one.  ORDER 0 = lanes in index order, else the seed of a shuffle
//   weedindexcheck small SLOTS SEED            an index of SLOTS slots filled to exactly half with chains that wrap around the end, then
//                                              filled up, then one key more
//   weedindexcheck garbage SEED                an index of random words under every lane
//   weedindexcheck layout N K                  the scratch of an indexed call
//   weedindexcheck bytes BOARD_CAP             eg_weed_index_bytes
//   weedindexcheck refuse N N_PRIOR CAP K      what the argument rules say
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/weed_index_kernels.cuh"

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct TableArr {                           // the batch table: 64-bit references
  std::vector<uint64_t> slots;
  uint64_t peek(uint64_t i) const { return slots.at(i); }
  uint64_t claim(uint64_t i, uint64_t ref) { const uint64_t old = slots.at(i); if (old == egw::EMPTY) slots.at(i) = ref; return old; }
  void lower(uint64_t i, uint64_t ref) { if (ref < slots.at(i)) slots.at(i) = ref; }
};
struct IndexArr {                           // the board index: 32-bit slots behind the same interface (WeedIndexDev / WeedIndexRead)
  std::vector<uint32_t> slots;
  uint64_t peek(uint64_t i) const { return egw::index_widen(slots.at(i)); }
  uint64_t claim(uint64_t i, uint64_t ref) {
    const uint32_t old = slots.at(i);
    CHECK(ref < egw::N_LIMIT, "a reference of 2^31 or more goes into the index");
    if (old == egw::INDEX_EMPTY) slots.at(i) = (uint32_t)ref;
    return egw::index_widen(old);
  }
  void lower(uint64_t i, uint64_t ref) { if ((uint32_t)ref < slots.at(i)) slots.at(i) = (uint32_t)ref; }
};
static void words_of(uint32_t w[16], const uint8_t* p) {
  for (int i = 0; i < 16; ++i) w[i] = p ? (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24) : 0u;
}
// every ballot in an allocation of its own: key k is item 1 + 2 k of a ballot of 2 K + 1 items.  As WeedKeysDev: a board reference at or
// above `bound` and a ballot at or above n read as zeros and touch no memory
struct KeysArr {
  const std::vector<std::unique_ptr<uint8_t[]>>* ballots;
  const std::vector<uint8_t>* board;
  uint64_t stride, bound;
  uint32_t K;
  static uint32_t r_item(uint32_t k) { return 1u + 2u * k; }
  void load(uint32_t w[16], uint64_t ref) const {
    const uint8_t* p = nullptr;
    if (egw::is_board_ref(ref)) {
      if (ref < bound) { (void)board->at(ref * 64 + 63); p = board->data() + ref * 64; }
    } else if (ballots && egw::ref_ballot(ref, K) < ballots->size()) {
      p = ballots->at(egw::ref_ballot(ref, K)).get() + egw::key_offset(0, stride, r_item(egw::ref_key(ref, K)));
    }
    words_of(w, p);
  }
};
struct FindKeysArr {                        // WeedFindKeysDev
  const std::vector<uint8_t>* queries;
  const std::vector<uint8_t>* board;
  uint64_t n_q, bound;
  void load(uint32_t w[16], uint64_t ref) const {
    const uint8_t* p = nullptr;
    if (egw::is_board_ref(ref)) {
      if (ref < bound) { (void)board->at(ref * 64 + 63); p = board->data() + ref * 64; }
    } else if (ref - egw::BATCH_BASE < n_q) {
      (void)queries->at((ref - egw::BATCH_BASE) * 64 + 63);
      p = queries->data() + (ref - egw::BATCH_BASE) * 64;
    }
    words_of(w, p);
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
static std::vector<uint64_t> lane_order(uint64_t first, uint64_t end, uint64_t order) {
  std::vector<uint64_t> lanes;
  for (uint64_t j = first; j < end; ++j) lanes.push_back(j);
  if (order) { std::mt19937_64 rng(order); std::shuffle(lanes.begin(), lanes.end(), rng); }
  return lanes;
}

struct Batch {
  std::vector<uint32_t> status;
  std::vector<std::unique_ptr<uint8_t[]>> ballots;
};
struct Result {
  std::vector<uint32_t> dup, out;
  uint32_t found[3] = {0, 0, 0};
  uint64_t count = 0;
  bool operator==(const Result& o) const { return dup == o.dup && out == o.out && !memcmp(found, o.found, sizeof found) && count == o.count; }
};

// scan, fit check, copy: every lane of k_weed_scan_* and k_weed_copy (shared by both passes, as the kernels are)
static void append(Result& r, std::vector<uint32_t>& pos, const Batch& B, std::vector<uint8_t>& board, uint64_t n_prior, uint64_t board_cap, uint32_t K,
                   uint64_t stride) {
  const uint64_t n = B.ballots.size();
  const uint32_t kept = egw::scan_keep(pos);
  const bool fits = egw::append_fits(n_prior, kept, K, board_cap);
  if (!fits) ++r.found[2];
  if (fits)
    for (uint64_t j = 0; j < n * K * 4; ++j) {
      const uint64_t b = j / (4 * K);
      const uint32_t q4 = (uint32_t)(j % (4 * K)), k = q4 >> 2, q = q4 & 3u;
      if (pos[b] == 0xffffffffu) continue;
      const uint64_t entry = egw::weed_append_entry(n_prior, pos[b], K, k);
      for (int i = 0; i < 16; ++i) board.at(entry * 64 + 16 * q + i) = B.ballots.at(b)[egw::key_offset(0, stride, KeysArr::r_item(k)) + 16 * q + i];
    }
  r.count = n_prior + (fits ? (uint64_t)kept * K : 0);
}
static void tally(Result& r, uint64_t b, uint32_t status, bool missing, std::vector<uint32_t>& pos) {
  r.out[b] = egw::weed_status_out(status, r.dup[b]);
  pos[b] = status == 0u && r.dup[b] == egw::DUP_NONE ? 1u : 0u;
  r.found[0] += r.dup[b] == egw::DUP_PRIOR;
  r.found[1] += r.dup[b] != egw::DUP_NONE && r.dup[b] != egw::DUP_PRIOR;
  r.found[2] += missing;
}

// the stateless pass (weed_kernels.cuh): one table for board and batch, cleared and filled here
static Result stateless(const Batch& B, std::vector<uint8_t>& board, uint64_t n_prior, uint64_t board_cap, uint32_t K, uint64_t seed, uint64_t order,
                        bool do_append) {
  const uint64_t n = B.ballots.size(), stride = 32 * (2 * K + 1);
  const egw::Layout L = egw::layout(n, n_prior, K);
  TableArr tab{std::vector<uint64_t>(L.slots, egw::EMPTY)};
  const KeysArr io{&B.ballots, &board, stride, n_prior, K};
  Result r;
  r.dup.resize(n); r.out.resize(n);
  for (uint64_t j : lane_order(0, n_prior + n * K, order)) {
    uint64_t ref = j;
    if (j >= n_prior) {
      if (B.status[(j - n_prior) / K] != 0u) continue;
      ref = egw::BATCH_BASE + (j - n_prior);
    }
    if (!egw::weed_lane_insert(tab, io, L.slots, seed, ref)) ++r.found[2];
  }
  std::vector<uint32_t> pos(n);
  for (uint64_t b = 0; b < n; ++b) {
    bool missing = false;
    r.dup[b] = B.status[b] == 0u ? egw::weed_lane_ballot(tab, io, L.slots, seed, b, K, missing) : egw::DUP_NONE;
    tally(r, b, B.status[b], missing, pos);
  }
  r.count = n_prior;
  if (do_append) append(r, pos, B, board, n_prior, board_cap, K, stride);
  return r;
}
// the indexed pass: the launches of weed_indexed_launch (eg_hip.hip) in their order
static Result indexed(const Batch& B, std::vector<uint8_t>& board, uint64_t n_prior, uint64_t board_cap, uint32_t K, IndexArr& index, uint64_t index_seed,
                      uint64_t seed, uint64_t order, bool do_append) {
  const uint64_t n = B.ballots.size(), stride = 32 * (2 * K + 1), index_slots = index.slots.size();
  const egw::Layout L = egw::layout_indexed(n, K);
  TableArr tab{std::vector<uint64_t>(L.slots, egw::EMPTY)};
  const KeysArr io{&B.ballots, &board, stride, n_prior, K};
  const KeysArr batch_io{&B.ballots, &board, stride, 0, K};          // keys.n_prior = 0: the batch table never touches the board
  Result r;
  r.dup.resize(n); r.out.resize(n);
  for (uint64_t j : lane_order(0, n * K, order)) {                   // k_weed_insert
    if (B.status[j / K] != 0u) continue;
    if (!egw::weed_lane_insert(tab, batch_io, L.slots, seed, egw::BATCH_BASE + j)) ++r.found[2];
  }
  for (uint64_t v : tab.slots) CHECK(v == egw::EMPTY || !egw::is_board_ref(v), "a board reference in the batch table");
  std::vector<uint32_t> pos(n);
  const IndexArr& read_only = index;
  for (uint64_t b : lane_order(0, n, order)) {                       // k_weed_lookup_indexed
    bool missing = false;
    r.dup[b] = B.status[b] == 0u ? egw::weed_lane_ballot_indexed(read_only, index_slots, index_seed, tab, io, L.slots, seed, b, K, missing) : egw::DUP_NONE;
    tally(r, b, B.status[b], missing, pos);
  }
  r.count = n_prior;
  if (do_append) {
    append(r, pos, B, board, n_prior, board_cap, K, stride);
    const uint64_t end = std::min(r.count, board_cap);               // k_weed_index_add: the count comes from the scan, bounds the references
    const KeysArr board_io{nullptr, &board, 0, end, 1};
    for (uint64_t j : lane_order(n_prior, end, order ? order + 1 : 0))
      if (!egw::weed_lane_insert(index, board_io, index_slots, index_seed, j)) ++r.found[2];
  }
  return r;
}
static void build(IndexArr& index, const std::vector<uint8_t>& board, uint64_t n_prior, uint64_t index_seed, uint64_t order, uint32_t* over) {
  std::fill(index.slots.begin(), index.slots.end(), egw::INDEX_EMPTY);
  const KeysArr board_io{nullptr, &board, 0, n_prior, 1};
  for (uint64_t j : lane_order(0, n_prior, order))
    if (!egw::weed_lane_insert(index, board_io, index.slots.size(), index_seed, j)) ++*over;
}
static std::vector<uint32_t> find(const IndexArr& index, const std::vector<uint8_t>& queries, const std::vector<uint8_t>& board, uint64_t n_prior,
                                  uint64_t index_seed) {
  const FindKeysArr io{&queries, &board, queries.size() / 64, n_prior};
  std::vector<uint32_t> pos(io.n_q);
  for (uint64_t q = 0; q < io.n_q; ++q) pos[q] = egw::weed_lane_find(index, io, index.slots.size(), index_seed, q);
  return pos;
}

// FILE: "batches K n_prior board_cap", n_prior lines "hex(64)", then per batch "n append" and n lines "status hex(64 K)"
static int cmd_seq(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  const uint64_t index_seed = strtoull(argv[3], nullptr, 10), order = strtoull(argv[4], nullptr, 10);
  unsigned long long batches = 0, K = 0, n_prior = 0, board_cap = 0;
  if (fscanf(f, "%llu %llu %llu %llu", &batches, &K, &n_prior, &board_cap) != 4 || K == 0) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  if (const char* why = egw::refuse_indexed(0, n_prior, board_cap)) { fprintf(stderr, "refused: %s\n", why); fclose(f); return 2; }
  const uint64_t stride = 32 * (2 * K + 1);
  std::vector<uint8_t> board(board_cap * 64, 0xEE);
  std::vector<char> line(128 * K + 64);
  for (uint64_t j = 0; j < n_prior; ++j)
    if (fscanf(f, "%s", line.data()) != 1 || !unhex(board.data() + 64 * j, line.data(), 64)) { fprintf(stderr, "bad board line\n"); fclose(f); return 2; }
  CHECK(egw::index_bytes(board_cap) == 4 * egw::table_slots(board_cap), "index_bytes");
  IndexArr index{std::vector<uint32_t>(egw::table_slots(board_cap))};
  uint32_t over = 0;
  build(index, board, n_prior, index_seed, order, &over);
  CHECK(over == 0, "the first build overflowed");
  std::vector<uint8_t> keys(64 * K);
  for (uint64_t t = 0; t < batches; ++t) {
    unsigned long long n = 0, do_append = 0;
    if (fscanf(f, "%llu %llu", &n, &do_append) != 2) { fprintf(stderr, "bad batch header\n"); fclose(f); return 2; }
    if (const char* why = egw::refuse_indexed(n, n_prior, board_cap)) { fprintf(stderr, "refused: %s\n", why); fclose(f); return 2; }
    Batch B;
    B.status.resize(n);
    for (uint64_t b = 0; b < n; ++b) {
      if (fscanf(f, "%u %s", &B.status[b], line.data()) != 2) { fprintf(stderr, "bad ballot line\n"); fclose(f); return 2; }
      B.ballots.emplace_back(new uint8_t[stride]);
      memset(B.ballots.back().get(), 0xA5, stride);
      if (B.status[b] == 0u) {
        if (!unhex(keys.data(), line.data(), 64 * K)) { fprintf(stderr, "bad ballot hex\n"); fclose(f); return 2; }
        for (uint32_t k = 0; k < K; ++k) memcpy(B.ballots.back().get() + 32 * KeysArr::r_item(k), keys.data() + 64 * k, 64);
      } else {
        ASAN_POISON_MEMORY_REGION(B.ballots.back().get(), stride);          // never read
      }
    }
    const uint64_t hash_seed = 0x1234 + 77 * t + order;
    // the stateless lanes over the same board bytes, on a copy
    std::vector<uint8_t> board_s = board;
    const Result want = stateless(B, board_s, n_prior, board_cap, (uint32_t)K, hash_seed ^ 5, order, do_append != 0);
    // a read-only indexed pass first: the same verdicts, and not a byte of the index or the board changes
    const std::vector<uint32_t> index_before = index.slots;
    const std::vector<uint8_t> board_before = board;
    const Result ro = indexed(B, board, n_prior, board_cap, (uint32_t)K, index, index_seed, hash_seed, order, false);
    CHECK(index.slots == index_before && board == board_before, "batch %" PRIu64 ": the read-only pass wrote", t);
    CHECK(ro.dup == want.dup && ro.out == want.out && ro.found[0] == want.found[0] && ro.found[1] == want.found[1] && ro.count == n_prior,
          "batch %" PRIu64 ": the read-only pass differs from the stateless lanes", t);
    const Result got = do_append ? indexed(B, board, n_prior, board_cap, (uint32_t)K, index, index_seed, hash_seed, order, true) : ro;
    CHECK(got == want, "batch %" PRIu64 ": the indexed lanes differ from the stateless lanes", t);
    CHECK(board == board_s, "batch %" PRIu64 ": the boards differ", t);
    const bool index_changed = index.slots != index_before;
    if (got.count == n_prior) CHECK(!index_changed && board == board_before, "batch %" PRIu64 ": nothing was appended, yet the index or the board changed", t);
    uint64_t used = 0;
    for (uint32_t v : index.slots) used += v != egw::INDEX_EMPTY;
    CHECK(2 * used <= index.slots.size(), "the index is loaded above 0.5");
    printf("BATCH %" PRIu64 "\nDUP :", t);
    for (uint32_t d : got.dup) printf(" %u", d);
    printf("\nSTATUS :");
    for (uint32_t s : got.out) printf(" %u", s);
    printf("\nFOUND %u %u %u\nCOUNT %" PRIu64 "\nINDEX changed %d used %" PRIu64 "\n", got.found[0], got.found[1], got.found[2], got.count,
           index_changed ? 1 : 0, used);
    n_prior = got.count;
    for (auto& p : B.ballots) ASAN_UNPOISON_MEMORY_REGION(p.get(), stride);
  }
  fclose(f);
  // find over the maintained index and over a freshly built one (another seed, another order): every board entry at its smallest
  // position, 100 absent keys nowhere.  The tables need not be byte-equal
  std::map<std::vector<uint8_t>, uint32_t> first_at;
  for (uint64_t j = 0; j < n_prior; ++j) first_at.emplace(std::vector<uint8_t>(board.begin() + 64 * j, board.begin() + 64 * j + 64), (uint32_t)j);
  std::vector<uint8_t> queries(board.begin(), board.begin() + 64 * n_prior);
  std::mt19937_64 rng(4242);
  for (int i = 0; i < 100 * 64; ++i) queries.push_back((uint8_t)rng());
  IndexArr fresh{std::vector<uint32_t>(index.slots.size())};
  build(fresh, board, n_prior, index_seed ^ 0x5eed, order + 3, &over);
  CHECK(over == 0, "the fresh build overflowed");
  const std::vector<uint32_t> a = find(index, queries, board, n_prior, index_seed), b = find(fresh, queries, board, n_prior, index_seed ^ 0x5eed);
  CHECK(a == b, "find over the maintained index differs from find over a fresh one");
  uint64_t dups_on_board = 0;
  for (uint64_t q = 0; q < n_prior + 100; ++q) {
    const auto it = first_at.find(std::vector<uint8_t>(queries.begin() + 64 * q, queries.begin() + 64 * q + 64));
    const uint32_t want = it == first_at.end() ? egw::DUP_NONE : it->second;
    CHECK(a[q] == want, "find(%" PRIu64 ") = %u, want %u", q, a[q], want);
    if (q < n_prior && want != q) ++dups_on_board;
    if (q >= n_prior) CHECK(a[q] == egw::DUP_NONE, "an absent key was found");
  }
  uint64_t used = 0;
  for (uint32_t v : index.slots) used += v != egw::INDEX_EMPTY;
  CHECK(used == first_at.size(), "one slot per distinct key: %" PRIu64 " used, %zu distinct", used, first_at.size());
  printf("FINAL count %llu distinct %zu equal_entries %" PRIu64 "\nBOARD ", n_prior, first_at.size(), dups_on_board);
  print_hex(board.data(), board.size());
  printf("\n");
  return 0;
}

// keys whose chains start in the last two slots: with SLOTS / 2 of them the chains wrap around the end
static int cmd_small(char** argv) {
  const uint64_t slots = strtoull(argv[2], nullptr, 10), seed = strtoull(argv[3], nullptr, 10);
  CHECK(slots >= 4 && (slots & (slots - 1)) == 0, "slots");
  std::mt19937_64 rng(seed * 977 + slots);
  std::vector<uint8_t> board;
  auto add_key = [&](bool at_the_end) {
    for (;;) {
      uint8_t k[64];
      uint32_t w[16];
      for (auto& c : k) c = (uint8_t)rng();
      words_of(w, k);
      if (at_the_end && (egw::weed_hash(w, seed) & (slots - 1)) < slots - 2) continue;
      board.insert(board.end(), k, k + 64);
      return;
    }
  };
  for (uint64_t j = 0; j < slots / 2; ++j) add_key(true);
  IndexArr index{std::vector<uint32_t>(slots, egw::INDEX_EMPTY)};
  uint32_t over = 0;
  auto insert = [&](uint64_t j) {
    const KeysArr io{nullptr, &board, 0, board.size() / 64, 1};
    if (!egw::weed_lane_insert(index, io, slots, seed, j)) ++over;
  };
  for (uint64_t j = 0; j < slots / 2; ++j) insert(j);
  CHECK(over == 0, "half full");
  CHECK(index.slots[0] != egw::INDEX_EMPTY && index.slots[slots - 1] != egw::INDEX_EMPTY, "the chains do not wrap around the end");
  auto all_found = [&](uint64_t n) {
    std::vector<uint8_t> q(board.begin(), board.begin() + 64 * n);
    for (int i = 0; i < 64; ++i) q.push_back((uint8_t)(0xC3 ^ i));          // and one absent key
    const std::vector<uint32_t> pos = find(index, q, board, n, seed);
    for (uint64_t j = 0; j < n; ++j) CHECK(pos[j] == j, "find(%" PRIu64 ") = %u with %" PRIu64 " keys", j, pos[j], n);
    CHECK(pos[n] == egw::DUP_NONE, "the absent key was found");
  };
  all_found(slots / 2);
  const uint64_t half_used = std::count_if(index.slots.begin(), index.slots.end(), [](uint32_t v) { return v != egw::INDEX_EMPTY; });
  // a second copy of entry 0 behind them: one slot, the smaller position
  board.insert(board.end(), board.begin(), board.begin() + 64);
  insert(slots / 2);
  CHECK(over == 0 && (uint64_t)std::count_if(index.slots.begin(), index.slots.end(), [](uint32_t v) { return v != egw::INDEX_EMPTY; }) == half_used,
        "equal bytes took a second slot");
  board.resize(64 * (slots / 2));
  // filled up: a load of 1.0 still finds everything, and a lookup of an absent key terminates
  for (uint64_t j = slots / 2; j < slots; ++j) { add_key(false); insert(j); }
  CHECK(over == 0, "full");
  all_found(slots);
  // one slot too small: the lane reports and terminates
  add_key(false);
  insert(slots);
  CHECK(over == 1, "the overflow was not reported");
  printf("SMALL slots %" PRIu64 " half %" PRIu64 " over %u\n", slots, half_used, over);
  return 0;
}

// an index of random words (positions below n_prior, positions at or above it and beyond the board's room, all ones) under every lane:
// the loops terminate and nothing outside [0, bound) is dereferenced (the arrays end exactly there)
static int cmd_garbage(char** argv) {
  const uint64_t seed = strtoull(argv[2], nullptr, 10);
  std::mt19937_64 rng(seed);
  const uint32_t K = 3;
  const uint64_t n = 40, n_prior = 50, board_cap = 50 + n * K, stride = 32 * (2 * K + 1);
  std::vector<uint8_t> board(board_cap * 64);
  for (auto& c : board) c = (uint8_t)rng();
  Batch B;
  B.status.assign(n, 0);
  for (uint64_t b = 0; b < n; ++b) {
    B.ballots.emplace_back(new uint8_t[stride]);
    for (uint64_t i = 0; i < stride; ++i) B.ballots.back()[i] = (uint8_t)rng();
    if (b % 7 == 0) memset(B.ballots.back().get(), 0, stride);            // all-zero keys equal what a refused reference reads as
  }
  IndexArr index{std::vector<uint32_t>(egw::table_slots(board_cap))};
  for (int round = 0; round < 4; ++round) {
    for (auto& v : index.slots) {
      const uint64_t x = rng();
      v = round == 3 ? (uint32_t)x                                          // any word
          : x % 4 == 0 ? (uint32_t)(x >> 8) % (uint32_t)n_prior             // a position on the board
          : x % 4 == 1 ? (uint32_t)(n_prior + (x >> 8) % 1000)              // at or above n_prior
          : x % 4 == 2 ? 0x7fffffffu - (uint32_t)((x >> 8) % 5)             // far beyond the board
                       : (round == 0 ? egw::INDEX_EMPTY : (uint32_t)(x >> 40));      // round 0 keeps empty slots, later rounds are full
    }
    std::vector<uint8_t> brd = board;
    const Result r = indexed(B, brd, n_prior, board_cap, K, index, seed, seed + 1, round, true);
    std::vector<uint8_t> q(brd.begin(), brd.begin() + 64 * 60);
    const std::vector<uint32_t> pos = find(index, q, brd, r.count, seed);
    printf("GARBAGE round %d found %u %u %u count %" PRIu64 " pos0 %u\n", round, r.found[0], r.found[1], r.found[2], r.count, pos[0]);
    CHECK(r.count >= n_prior && r.count <= board_cap, "count");
  }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 5 && strcmp(argv[1], "seq") == 0) {
    rc = cmd_seq(argv);
  } else if (argc == 4 && strcmp(argv[1], "small") == 0) {
    rc = cmd_small(argv);
  } else if (argc == 3 && strcmp(argv[1], "garbage") == 0) {
    rc = cmd_garbage(argv);
  } else if (argc == 4 && strcmp(argv[1], "layout") == 0) {
    const egw::Layout L = egw::layout_indexed(strtoull(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10));
    printf("LAYOUT slots %" PRIu64 " tiles %u table %zu pos %zu tile_sums %zu total_word %zu total %zu\n", L.slots, L.n_tiles, L.table, L.pos, L.tiles,
           L.total_word, L.total);
  } else if (argc == 3 && strcmp(argv[1], "bytes") == 0) {
    printf("BYTES %zu\n", egw::index_bytes(strtoull(argv[2], nullptr, 10)));
  } else if (argc == 6 && strcmp(argv[1], "refuse") == 0) {
    const uint64_t n = strtoull(argv[2], nullptr, 10), n_prior = strtoull(argv[3], nullptr, 10), cap = strtoull(argv[4], nullptr, 10);
    const char* why = egw::refuse_indexed(n, n_prior, cap);
    if (!why) why = egw::refuse_indexed_keys(n, (uint32_t)strtoul(argv[5], nullptr, 10));
    printf("REFUSE %s\n", why ? why : "-");
  } else {
    fprintf(stderr, "usage: weedindexcheck seq FILE INDEX_SEED ORDER | small SLOTS SEED | garbage SEED | layout N K | bytes CAP | refuse N N_PRIOR CAP K\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
