// Host build of the voter-roll pass (elastic_elgamal_amd/csrc/roll_kernels.cuh, roll_host.hpp) under ASan + UBSan: the lane functions of
// the claim / resolve / commit / check kernels run serially on arrays, in any lane order; every array access is bounds-checked, the
// key_index of a ballot that does not participate is poisoned, and so are the status words once the resolve lanes have run, so that
// reading either aborts the program.
// Stand-alone program (tests/test_roll_cpu.py builds it and reads its report):
//   rollcheck cast FILE ORDER ALIAS     the whole cast over the case of FILE; ORDER 0 = lanes in index order, else the seed of a shuffle;
//                                       ALIAS 1 = status_out is status_in itself
//   rollcheck check FILE ORDER ALIAS    the check lanes over the same kind of file
//   rollcheck layout N N_KEYS           the parts of the scratch
//   rollcheck refuse N N_KEYS SEQ_BASE POLICY MASK   what the argument rules say; MASK: bit k = pointer k of egr::Have is there
//   rollcheck word SEQ POLICY           the word of a sequence number, and the sequence number of that word
// FILE: "n n_keys seq_base policy have_groups have_weights have_displaced", then n_keys lines "word group weight", then n lines
// "status key_index".  exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <random>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/roll_kernels.cuh"

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct MemArr {
  std::vector<std::unique_ptr<uint32_t[]>>* index;        // every key_index in an allocation of its own
  std::vector<uint32_t>* best_;
  std::vector<uint64_t>* roll_;
  const std::vector<uint32_t>* groups;                    // null: no roster array
  const std::vector<uint64_t>* weights;
  std::vector<uint64_t>* displaced;
  unsigned long long* stores;
  uint32_t key_index(uint64_t b) const { return index->at(b)[0]; }
  void raise(uint32_t v, uint32_t claim) { if (claim > best_->at(v)) best_->at(v) = claim; }
  uint32_t best(uint32_t v) const { return best_->at(v); }
  uint64_t roll(uint32_t v) const { return roll_->at(v); }
  uint32_t group(uint32_t v) const { return groups ? groups->at(v) : egr::GROUP_NONE; }
  uint64_t weight(uint32_t v) const { return weights ? weights->at(v) : 0u; }
  void store(uint32_t v, uint64_t word) { roll_->at(v) = word; ++*stores; }
  void displace(uint64_t rank, uint64_t old_seq, uint64_t new_seq) { displaced->at(2 * rank) = old_seq; displaced->at(2 * rank + 1) = new_seq; }
};

template <class T, class F>
static void print_row(const char* name, const std::vector<T>& v, F fmt) {
  printf("%s :", name);
  for (const T& x : v) fmt(x);
  printf("\n");
}

static int cmd_run(char** argv, bool cast) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  const uint64_t order = strtoull(argv[3], nullptr, 10);
  const bool alias = strtoull(argv[4], nullptr, 10) != 0;
  unsigned long long n = 0, n_keys = 0, seq_base = 0;
  int policy = 0, have_groups = 0, have_weights = 0, have_displaced = 0;
  if (fscanf(f, "%llu %llu %llu %d %d %d %d", &n, &n_keys, &seq_base, &policy, &have_groups, &have_weights, &have_displaced) != 7) {
    fprintf(stderr, "bad header\n"); fclose(f); return 2;
  }
  std::vector<uint64_t> roll(n_keys), weights(n_keys);
  std::vector<uint32_t> groups(n_keys);
  for (uint64_t v = 0; v < n_keys; ++v)
    if (fscanf(f, "%" SCNu64 " %u %" SCNu64, &roll[v], &groups[v], &weights[v]) != 3) { fprintf(stderr, "bad roster line\n"); fclose(f); return 2; }
  std::unique_ptr<uint32_t[]> status(new uint32_t[n + 1]);
  std::vector<std::unique_ptr<uint32_t[]>> index;
  for (uint64_t b = 0; b < n; ++b) {
    index.emplace_back(new uint32_t[2]);
    if (fscanf(f, "%u %u", &status[b], &index.back()[0]) != 2) { fprintf(stderr, "bad ballot line\n"); fclose(f); return 2; }
    if (status[b] != 0u) ASAN_POISON_MEMORY_REGION(index.back().get(), 2 * sizeof(uint32_t));        // never read
  }
  fclose(f);
  const egr::Have have{true, true, true, true, have_groups != 0, have_weights != 0, have_groups != 0, have_weights != 0, have_displaced != 0,
                       have_displaced != 0};
  if (const char* why = egr::refuse(n, n_keys, seq_base, policy, have)) { printf("REFUSED %s\n", why); return 0; }

  std::vector<uint64_t> lanes(n);
  for (uint64_t b = 0; b < n; ++b) lanes[b] = b;
  std::mt19937_64 rng(order);
  auto shuffle = [&]() { if (order) std::shuffle(lanes.begin(), lanes.end(), rng); };
  std::vector<uint32_t> best(cast ? n_keys : 0, 0u), flag(n, 0xdeadbeefu), out(n), groups_out(n);
  std::vector<uint64_t> by(n), weights_out(n), displaced(have_displaced ? 2 * n : 0, 0xEEEEEEEEEEEEEEEEull);
  unsigned long long stores = 0;
  MemArr mem{&index, &best, &roll, have_groups ? &groups : nullptr, have_weights ? &weights : nullptr, &displaced, &stores};
  uint32_t found[3] = {0, 0, 0};
  uint32_t* status_out = alias ? status.get() : out.data();
  if (cast) {
    shuffle();
    for (uint64_t b : lanes) egr::roll_lane_claim(mem, b, n, status[b] == 0u, policy, n_keys);
  }
  const std::vector<uint64_t> roll_before = roll;
  shuffle();
  for (uint64_t b : lanes) {
    const uint32_t st = status[b];
    const egr::Verdict V = cast ? egr::roll_lane_resolve(mem, b, n, st, st == 0u, seq_base, policy, n_keys)
                                : egr::roll_lane_check(mem, b, st, st == 0u, seq_base, policy, n_keys);
    by[b] = V.superseded_by; status_out[b] = V.status; groups_out[b] = V.group; weights_out[b] = V.weight;
    flag[b] = V.flag;
    found[0] += V.superseded;
    found[1] += cast ? V.flag == egr::FLAG_DISPLACED : V.not_cast;
    found[2] += V.off_roll;
    CHECK(V.superseded + V.off_roll + V.not_cast <= 1 && (V.flag == egr::FLAG_NONE || V.status == st), "verdict of ballot %" PRIu64, b);
  }
  CHECK(roll == roll_before, "the roll is read-only until the commit");
  if (alias) out.assign(status.get(), status.get() + n);
  uint64_t count = 0;
  if (cast) {
    ASAN_POISON_MEMORY_REGION(status.get(), (n + 1) * sizeof(uint32_t));          // the commit never reads a status word
    if (have_displaced) count = egr::scan_displaced(flag.data(), n);
    CHECK(!have_displaced || count == found[1], "the scan's total is the counter");
    shuffle();
    for (uint64_t b : lanes) egr::roll_lane_commit(mem, b, n, flag[b], seq_base, policy, n_keys, have_displaced != 0);
    ASAN_UNPOISON_MEMORY_REGION(status.get(), (n + 1) * sizeof(uint32_t));
    uint64_t changed = 0;
    for (uint64_t v = 0; v < n_keys; ++v) { changed += roll[v] != roll_before[v]; CHECK(roll[v] >= roll_before[v], "word %" PRIu64 " fell", v); }
    CHECK(changed == stores, "one writer per voter: %llu stores, %" PRIu64 " words changed", stores, changed);
    for (uint64_t k = 2 * count; k < displaced.size(); ++k) CHECK(displaced[k] == 0xEEEEEEEEEEEEEEEEull, "displaced written behind its count");
  } else {
    CHECK(stores == 0, "the check stores nothing");
  }
  for (auto& p : index) ASAN_UNPOISON_MEMORY_REGION(p.get(), 2 * sizeof(uint32_t));
  print_row("BY", by, [](uint64_t x) { printf(" %" PRIu64, x); });
  print_row("STATUS", out, [](uint32_t x) { printf(" %u", x); });
  if (have_groups) print_row("GROUPS", groups_out, [](uint32_t x) { printf(" %u", x); });
  if (have_weights) print_row("WEIGHTS", weights_out, [](uint64_t x) { printf(" %" PRIu64, x); });
  printf("FOUND %u %u %u\n", found[0], found[1], found[2]);
  print_row("ROLL", roll, [](uint64_t x) { printf(" %" PRIu64, x); });
  if (cast && have_displaced) {
    displaced.resize(2 * count);
    print_row("DISPLACED", displaced, [](uint64_t x) { printf(" %" PRIu64, x); });
  }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 5 && (strcmp(argv[1], "cast") == 0 || strcmp(argv[1], "check") == 0)) {
    rc = cmd_run(argv, argv[1][1] == 'a');
  } else if (argc == 4 && strcmp(argv[1], "layout") == 0) {
    const egr::Layout L = egr::layout(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    printf("LAYOUT tiles %u best %zu flag %zu tile_sums %zu total %zu\n", L.n_tiles, L.best, L.flag, L.tiles, L.total);
  } else if (argc == 7 && strcmp(argv[1], "refuse") == 0) {
    const unsigned mask = (unsigned)strtoul(argv[6], nullptr, 10);
    auto bit = [&](int k) { return (mask >> k & 1u) != 0; };
    const egr::Have h{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9)};
    const char* why = egr::refuse(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), atoi(argv[5]), h);
    printf("REFUSE %s\n", why ? why : "-");
  } else if (argc == 4 && strcmp(argv[1], "word") == 0) {
    const uint64_t seq = strtoull(argv[2], nullptr, 10);
    const int policy = atoi(argv[3]);
    const uint64_t w = egr::word_of(seq, policy);
    printf("WORD %" PRIu64 " SEQ %" PRIu64 "\n", w, egr::seq_of(w, policy));
    CHECK(w >= 1 && w <= egr::SEQ_END_MAX, "word out of range");
  } else {
    fprintf(stderr, "usage: rollcheck cast|check FILE ORDER ALIAS | layout N N_KEYS | refuse N N_KEYS SEQ_BASE POLICY MASK | word SEQ POLICY\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
