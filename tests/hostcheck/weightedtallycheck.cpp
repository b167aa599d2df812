// Host build of the weighted per-group tally (elastic_elgamal_amd/csrc/group_tally_kernels.cuh, group_tally_host.hpp) with -DEG_BOUNDCHECK
// under ASan + UBSan: ge_mul_u64 and the lane functions of the weighted pass run on arrays, with piece sizes of 2 and 3.  Every field
// operation asserts its limb-class precondition, every array access is bounds-checked.
// Stand-alone program (tests/test_weighted_tally_cpu.py builds it and reads its report):
//   weightedtallycheck mul FILE              lines "bits weight point-hex" -> the encoding of [weight mod 2^bits] point, by ge_mul_u64
//   weightedtallycheck layout n G T S1 S2    the scratch layout of the weighted pass beside the grouped one
//   weightedtallycheck run FILE S1 S2        the whole pipeline, serially, over the ballots of FILE
// exit code 0 = every internal check held.
#include <inttypes.h>
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
// weights of rejected ballots must never be read: reading one is an error here
struct WeightsArr {
  const std::vector<u64>* w;
  const std::vector<u32>* status;
  u64 load(u32 b) const { CHECK(status->at(b) == 0u, "the weight of rejected ballot %u was read", b); return w->at(b); }
};
struct PointsArr {
  std::vector<ge> pts;
  std::vector<char> written;
  explicit PointsArr(size_t n) : pts(n), written(n, 0) {}
  void store(size_t e, const ge& p) { CHECK(!written.at(e), "entry %zu written twice", e); pts.at(e) = p; written.at(e) = 1; }
  void load(ge& p, size_t e) const { CHECK(written.at(e), "entry %zu read before it was written", e); p = pts.at(e); }
};
struct SumsArr {
  std::vector<u64> v;
  std::vector<char> written;
  explicit SumsArr(size_t n) : v(2 * n), written(n, 0) {}
  void store(u32 u, u64 lo, u64 hi) { CHECK(!written.at(u), "weight sum %u written twice", u); v.at(2 * (size_t)u) = lo; v.at(2 * (size_t)u + 1) = hi; written.at(u) = 1; }
  void load(u64& lo, u64& hi, u32 u) const { CHECK(written.at(u), "weight sum %u read before it was written", u); lo = v.at(2 * (size_t)u); hi = v.at(2 * (size_t)u + 1); }
};
struct BadCount { u32 n = 0; void undecodable() { ++n; } };

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static void print_words(const u32 enc[8]) {
  for (int i = 0; i < 8; ++i) printf("%02x%02x%02x%02x", enc[i] & 255u, (enc[i] >> 8) & 255u, (enc[i] >> 16) & 255u, enc[i] >> 24);
}

// FILE: one line per product: "bits weight point-hex"
static int cmd_mul(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  int bits;
  unsigned long long weight;
  char hex[80];
  while (fscanf(f, "%d %llu %79s", &bits, &weight, hex) == 3) {
    if (strlen(hex) != 64 || bits < 1 || bits > 64) { fprintf(stderr, "bad line\n"); fclose(f); return 2; }
    u32 w[8];
    for (int i = 0; i < 8; ++i) {
      w[i] = 0;
      for (int j = 3; j >= 0; --j) w[i] = (w[i] << 8) | (u32)(hexval(hex[2 * (4 * i + j)]) * 16 + hexval(hex[2 * (4 * i + j) + 1]));
    }
    ge p, r;
    CHECK(ristretto_decode(p, w), "the point of a mul line does not decode");
    ge_mul_u64(r, p, (u64)weight, bits);
    u32 enc[8];
    ristretto_encode(enc, r);
    printf("MUL ");
    print_words(enc);
    printf("\n");
  }
  fclose(f);
  return 0;
}

static int cmd_layout(char** argv) {
  const size_t n = (size_t)strtoull(argv[2], nullptr, 10);
  const u32 G = (u32)strtoul(argv[3], nullptr, 10), T = (u32)atoi(argv[4]), s1 = (u32)atoi(argv[5]), s2 = (u32)atoi(argv[6]);
  const eggt::Layout L = eggt::layout(n, G, T, s1, s2);
  const eggt::WeightedLayout W = eggt::layout_weighted(n, G, T, s1, s2);
  CHECK(L.total == W.base.total && L.idx == W.base.idx && L.psum[0] == W.base.psum[0] && L.psum[1] == W.base.psum[1] && W.wsum[0] == L.total,
        "the weighted layout does not begin with the grouped one");
  printf("LAYOUT levels %d grouped %zu wsum0 %zu wsum1 %zu total %zu pieces0 %zu pieces1 %zu\n", L.n_levels, L.total, W.wsum[0], W.wsum[1], W.total,
         L.psum_points[0], L.psum_points[1]);
  return 0;
}

// FILE: "n n_groups n_options single weight_bits have_groups" then one line per ballot: "status group weight hex"
static int cmd_run(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  const u32 s1 = (u32)atoi(argv[3]), s2 = (u32)atoi(argv[4]);
  unsigned n = 0, G = 0, n_options = 0, single = 0, have_groups = 0;
  int bits = 0;
  if (fscanf(f, "%u %u %u %u %d %u", &n, &G, &n_options, &single, &bits, &have_groups) != 6 || G == 0) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  const eghost::Plan P = eghost::build_choice_plan((int)n_options, single != 0);
  const std::vector<uint32_t> items = eggt::tally_items(P.pt_items, P.tally_slots);
  const u32 T = (u32)items.size();
  const size_t stride = P.stride;
  std::vector<u32> status(n), groups(n);
  std::vector<u64> weight(n);
  std::vector<uint8_t> wire((size_t)n * stride);
  std::vector<char> line(2 * stride + 64);
  for (unsigned b = 0; b < n; ++b) {
    unsigned long long w;
    if (fscanf(f, "%u %u %llu %s", &status[b], &groups[b], &w, line.data()) != 4 || strlen(line.data()) != 2 * stride) { fprintf(stderr, "bad ballot line %u\n", b); fclose(f); return 2; }
    weight[b] = (u64)w;
    for (size_t i = 0; i < stride; ++i) wire[b * stride + i] = (uint8_t)(hexval(line[2 * i]) * 16 + hexval(line[2 * i + 1]));
  }
  fclose(f);
  if (eggt::refuse(n, G) || eggt::refuse_weight_bits(bits) || (!have_groups && G != 1)) { fprintf(stderr, "refused\n"); return 2; }
  const int levels = eggt::levels(n, s1, s2);
  if (levels > eggt::MAX_LEVELS) { fprintf(stderr, "too many levels\n"); return 2; }
  const u32* gp = have_groups ? groups.data() : nullptr;
  const WeightsArr wts{&weight, &status};

  // count (k_gtw_count)
  u32 bad[3] = {0, 0, 0};
  std::vector<u32> counts(G, 0);
  for (unsigned b = 0; b < n; ++b) {
    u32 g;
    const u32 cls = gt_weighted_class(g, b, status.data(), gp, G, wts, bits);
    if (cls == 1u) ++counts.at(g);
    else if (cls == 2u) ++bad[0];
    else if (cls == 3u) ++bad[2];
  }
  const eggt::Scan S = eggt::scan(counts, levels, s1, s2);
  // fill (k_gtw_fill), from the LAST ballot down: the order inside a list must not matter
  std::vector<u32> cursors(G, 0), idx(n, 0xffffffffu);
  for (unsigned b = n; b-- > 0;) {
    u32 g;
    if (gt_weighted_class(g, b, status.data(), gp, G, wts, bits) == 1u) idx.at(S.offsets[g] + cursors[g]++) = b;
  }
  // the levels: points and weight sums side by side
  const WireArr w{&wire, stride};
  BadCount nb;
  std::vector<PointsArr> psum;
  std::vector<SumsArr> wsum;
  const u32* cnt = counts.data();
  const u32* off = S.offsets.data();
  for (int l = 0; l < levels; ++l) {
    psum.emplace_back((size_t)S.totals[l] * T);
    wsum.emplace_back((size_t)S.totals[l]);
    const GtLevel lv{cnt, off, S.piece0[l].data()};
    for (u32 u = 0; u < S.totals[l]; ++u) {
      for (u32 t = 0; t < T; ++t) {
        if (l == 0) gt_lane_wire_weighted(u, t, T, s1, lv, G, idx.data(), w, items[t], wts, bits, psum[0], wsum[0], nb);
        else gt_lane_points(u, t, T, s2, lv, G, psum[l - 1], psum[l]);
      }
      if (l > 0) gt_lane_weight_sums(u, s2, lv, G, wsum[l - 1], wsum[l]);
    }
    for (char c : psum[l].written) CHECK(c, "level %d left an entry unwritten", l);
    for (char c : wsum[l].written) CHECK(c, "level %d left a weight sum unwritten", l);
    cnt = S.pieces[l].data(); off = S.piece0[l].data();
  }
  bad[1] = nb.n;
  printf("LEVELS %d\nBAD %u %u %u\nCOUNTS :", levels, bad[0], bad[1], bad[2]);
  for (u32 c : counts) printf(" %u", c);
  printf("\nSUMS :");
  for (u32 g = 0; g < G; ++g) {
    u64 lo, hi;
    gt_lane_weight_sum_out(lo, hi, g, S.pieces[levels - 1].data(), S.piece0[levels - 1].data(), wsum[levels - 1]);
    printf(" %" PRIu64 " %" PRIu64, lo, hi);
  }
  printf("\n");
  for (u32 g = 0; g < G; ++g) {
    printf("TALLY %u ", g);
    for (u32 t = 0; t < T; ++t) {
      u32 enc[8];
      gt_lane_encode(enc, g, t, T, S.pieces[levels - 1].data(), S.piece0[levels - 1].data(), psum[levels - 1]);
      print_words(enc);
    }
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc == 3 && strcmp(argv[1], "mul") == 0) {
    rc = cmd_mul(argv);
  } else if (argc == 7 && strcmp(argv[1], "layout") == 0) {
    rc = cmd_layout(argv);
  } else if (argc == 5 && strcmp(argv[1], "run") == 0) {
    rc = cmd_run(argv);
  } else {
    fprintf(stderr, "usage: weightedtallycheck mul FILE | layout n G T S1 S2 | run FILE S1 S2\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
