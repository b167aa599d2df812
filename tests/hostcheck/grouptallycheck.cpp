// Host build of the per-group tally (elastic_elgamal_amd/csrc/group_tally_kernels.cuh, group_tally_host.hpp) with -DEG_BOUNDCHECK under
// ASan + UBSan: the lane functions of the sum / encode kernels and gt_bucket_of run on arrays, with piece sizes of 2 and 3 so that a few
// dozen ballots walk six levels.  Every field operation asserts its limb-class precondition, every array access is bounds-checked.
// Stand-alone program (tests/test_group_tally_cpu.py builds it and reads its report):
//   grouptallycheck items                 the wire items behind the tally slots of six election shapes
//   grouptallycheck scan S1 S2 c0 c1 ..   offsets, pieces per level and the group of every piece for one vector of group counts
//   grouptallycheck run FILE S1 S2        the whole pipeline, serially, over the ballots of FILE
// exit code 0 = every internal check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../elastic_elgamal_amd/csrc/host_plan.hpp"
#include "../../elastic_elgamal_amd/csrc/group_tally_host.hpp"
#include "../../elastic_elgamal_amd/csrc/group_tally_kernels.cuh"

using namespace eg;

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct WireArr {
  const std::vector<uint8_t>* data;
  size_t stride;
  void load(u32 w[8], u32 b, u32 item) const {
    for (int i = 0; i < 8; ++i) {
      u32 x = 0;
      for (int j = 3; j >= 0; --j) x = (x << 8) | data->at((size_t)b * stride + (size_t)item * 32 + 4 * i + j);
      w[i] = x;
    }
  }
};
struct PointsArr {
  std::vector<ge> pts;
  std::vector<char> written;
  explicit PointsArr(size_t n) : pts(n), written(n, 0) {}
  void store(size_t e, const ge& p) { CHECK(!written.at(e), "entry %zu written twice", e); pts.at(e) = p; written.at(e) = 1; }
  void load(ge& p, size_t e) const { CHECK(written.at(e), "entry %zu read before it was written", e); p = pts.at(e); }
};
struct BadCount { u32 n = 0; void undecodable() { ++n; } };

static void print_items(const char* name, const eghost::Plan& P) {
  const std::vector<uint32_t> items = eggt::tally_items(P.pt_items, P.tally_slots);
  printf("ITEMS %s stride %zu :", name, (size_t)P.stride);
  for (uint32_t it : items) printf(" %u", it);
  printf("\n");
}

// the group of every piece, and the invariants of the last level
static void check_levels(const std::vector<u32>& counts, const eggt::Scan& S, int levels, u32 s1, u32 s2, bool print) {
  const u32 G = (u32)counts.size();
  const u32* cnt = counts.data();
  const u32* off = S.offsets.data();
  for (int l = 0; l < levels; ++l) {
    const u32 s = l == 0 ? s1 : s2;
    if (print) printf("BUCKETS %d :", l);
    u32 covered = 0;
    for (u32 u = 0; u < S.totals[l]; ++u) {
      const u32 q = gt_bucket_of(S.piece0[l].data(), G, u);
      CHECK(q < G && S.piece0[l][q] <= u && u < S.piece0[l][q] + S.pieces[l][q], "level %d piece %u -> group %u", l, u, q);
      u32 beg, end;
      const GtLevel lv{cnt, off, S.piece0[l].data()};
      gt_piece_range(beg, end, lv, G, u, s);
      CHECK(beg < end && end - beg <= s && beg >= off[q] && end <= off[q] + cnt[q], "level %d piece %u covers [%u, %u)", l, u, beg, end);
      covered += end - beg;
      if (print) printf(" %u", q);
    }
    if (print) printf("\n");
    u32 entries = 0;
    for (u32 q = 0; q < G; ++q) entries += cnt[q];
    CHECK(covered == entries, "level %d: pieces cover %u of %u entries", l, covered, entries);
    cnt = S.pieces[l].data(); off = S.piece0[l].data();
  }
  for (u32 q = 0; q < G; ++q) CHECK(S.pieces[levels - 1][q] <= 1u, "group %u has %u entries after the last level", q, S.pieces[levels - 1][q]);
}

static int cmd_scan(int argc, char** argv) {
  const u32 s1 = (u32)atoi(argv[2]), s2 = (u32)atoi(argv[3]);
  std::vector<u32> counts;
  uint64_t n = 0;
  for (int i = 4; i < argc; ++i) { counts.push_back((u32)strtoul(argv[i], nullptr, 10)); n += counts.back(); }
  const int levels = eggt::levels(n, s1, s2);
  if (levels > eggt::MAX_LEVELS) { fprintf(stderr, "too many levels\n"); return 2; }
  const eggt::Scan S = eggt::scan(counts, levels, s1, s2);
  printf("LEVELS %d\n", levels);
  printf("OFFSETS :");
  for (u32 v : S.offsets) printf(" %u", v);
  printf("\n");
  for (int l = 0; l < levels; ++l) {
    printf("PIECES %d total %u :", l, S.totals[l]);
    for (u32 v : S.pieces[l]) printf(" %u", v);
    printf("\nPIECE0 %d :", l);
    for (u32 v : S.piece0[l]) printf(" %u", v);
    printf("\n");
  }
  check_levels(counts, S, levels, s1, s2, true);
  return 0;
}

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

// FILE: "n n_groups n_options single" then one line per ballot: "status group hex"
static int cmd_run(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  const u32 s1 = (u32)atoi(argv[3]), s2 = (u32)atoi(argv[4]);
  unsigned n = 0, G = 0, n_options = 0, single = 0;
  if (fscanf(f, "%u %u %u %u", &n, &G, &n_options, &single) != 4 || G == 0) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  const eghost::Plan P = eghost::build_choice_plan((int)n_options, single != 0);
  const std::vector<uint32_t> items = eggt::tally_items(P.pt_items, P.tally_slots);
  const u32 T = (u32)items.size();
  const size_t stride = P.stride;
  std::vector<u32> status(n), groups(n);
  std::vector<uint8_t> wire((size_t)n * stride);
  std::vector<char> line(2 * stride + 64);
  for (unsigned b = 0; b < n; ++b) {
    if (fscanf(f, "%u %u %s", &status[b], &groups[b], line.data()) != 3 || strlen(line.data()) != 2 * stride) { fprintf(stderr, "bad ballot line %u\n", b); fclose(f); return 2; }
    for (size_t i = 0; i < stride; ++i) wire[b * stride + i] = (uint8_t)(hexval(line[2 * i]) * 16 + hexval(line[2 * i + 1]));
  }
  fclose(f);
  if (eggt::refuse(n, G)) { fprintf(stderr, "refused: %s\n", eggt::refuse(n, G)); return 2; }
  const int levels = eggt::levels(n, s1, s2);
  if (levels > eggt::MAX_LEVELS) { fprintf(stderr, "too many levels\n"); return 2; }

  // count (k_gt_count): ids of rejected ballots are never read
  u32 bad[2] = {0, 0};
  std::vector<u32> counts(G, 0);
  auto group_of = [&](unsigned b, bool* in) {
    *in = false;
    if (status[b] != 0u) return 0u;
    const u32 g = groups[b];
    if (g == eggt::GROUP_NONE) return 0u;
    if (g >= G) return g;
    *in = true;
    return g;
  };
  for (unsigned b = 0; b < n; ++b) {
    bool in;
    const u32 g = group_of(b, &in);
    if (in) ++counts.at(g);
    else if (status[b] == 0u && groups[b] != eggt::GROUP_NONE) ++bad[0];
  }
  const eggt::Scan S = eggt::scan(counts, levels, s1, s2);
  check_levels(counts, S, levels, s1, s2, false);
  // fill (k_gt_fill), from the LAST ballot down: the order inside a list must not matter
  std::vector<u32> cursors(G, 0), idx(n, 0xffffffffu);
  for (unsigned b = n; b-- > 0;) {
    bool in;
    const u32 g = group_of(b, &in);
    if (in) idx.at(S.offsets[g] + cursors[g]++) = b;
  }
  // the levels
  const WireArr w{&wire, stride};
  BadCount nb;
  std::vector<PointsArr> psum;
  const u32* cnt = counts.data();
  const u32* off = S.offsets.data();
  for (int l = 0; l < levels; ++l) {
    psum.emplace_back((size_t)S.totals[l] * T);
    const GtLevel lv{cnt, off, S.piece0[l].data()};
    for (u32 u = 0; u < S.totals[l]; ++u)
      for (u32 t = 0; t < T; ++t) {
        if (l == 0) gt_lane_wire(u, t, T, s1, lv, G, idx.data(), w, items[t], psum[0], nb);
        else gt_lane_points(u, t, T, s2, lv, G, psum[l - 1], psum[l]);
      }
    for (char c : psum[l].written) CHECK(c, "level %d left an entry unwritten", l);
    cnt = S.pieces[l].data(); off = S.piece0[l].data();
  }
  bad[1] = nb.n;
  printf("LEVELS %d\nBAD %u %u\nCOUNTS :", levels, bad[0], bad[1]);
  for (u32 c : counts) printf(" %u", c);
  printf("\n");
  for (u32 g = 0; g < G; ++g) {
    printf("TALLY %u ", g);
    for (u32 t = 0; t < T; ++t) {
      u32 enc[8];
      gt_lane_encode(enc, g, t, T, S.pieces[levels - 1].data(), S.piece0[levels - 1].data(), psum[levels - 1]);
      for (int i = 0; i < 8; ++i) printf("%02x%02x%02x%02x", enc[i] & 255u, (enc[i] >> 8) & 255u, (enc[i] >> 16) & 255u, enc[i] >> 24);
    }
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc == 2 && strcmp(argv[1], "items") == 0) {
    print_items("single2", eghost::build_choice_plan(2, true));
    print_items("single5", eghost::build_choice_plan(5, true));
    print_items("single150", eghost::build_choice_plan(150, true));
    print_items("multi16", eghost::build_choice_plan(16, false));
    print_items("qv5_20", eghost::build_qv_plan(5, 20));
    print_items("qv3_10000", eghost::build_qv_plan(3, 10000));
    rc = 0;
  } else if (argc >= 4 && strcmp(argv[1], "scan") == 0) {
    rc = cmd_scan(argc, argv);
  } else if (argc == 5 && strcmp(argv[1], "run") == 0) {
    rc = cmd_run(argv);
  } else {
    fprintf(stderr, "usage: grouptallycheck items | scan S1 S2 counts.. | run FILE S1 S2\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
