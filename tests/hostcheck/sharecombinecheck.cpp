// Host build of the batched share combination (elastic_elgamal_amd/csrc/share_combine_kernels.cuh, share_combine_host.hpp) with
// -DEG_BOUNDCHECK under ASan + UBSan: the lane functions of the three stages run serially on arrays laid out as the kernels lay the
// caller's scratch out.  Every field operation asserts its limb-class precondition, every array access is bounds-checked.
// Stand-alone program (tests/test_share_combine_cpu.py builds it and reads its report):
//   sharecombinecheck coeffs FILE        lines "k mask idx_0 .. idx_(k-1)" -> the scalars scale / denominator_i of the mask's columns
//   sharecombinecheck layout t m         the scratch layout
//   sharecombinecheck run FILE           the whole pipeline over the ciphertexts and columns of FILE
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../elastic_elgamal_amd/csrc/share_combine_host.hpp"
#include "../../elastic_elgamal_amd/csrc/share_combine_kernels.cuh"

using namespace eg;

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static bool unhex(std::vector<uint8_t>& out, const char* hex, size_t bytes) {
  if (strlen(hex) != 2 * bytes) return false;
  out.resize(bytes);
  for (size_t i = 0; i < bytes; ++i) {
    const int a = hexval(hex[2 * i]), b = hexval(hex[2 * i + 1]);
    if (a < 0 || b < 0) return false;
    out[i] = (uint8_t)(a * 16 + b);
  }
  return true;
}
static void words_of(u32 w[8], const std::vector<uint8_t>& bytes, size_t at) {
  for (int i = 0; i < 8; ++i) {
    u32 x = 0;
    for (int j = 3; j >= 0; --j) x = (x << 8) | bytes.at(at + 4 * (size_t)i + (size_t)j);
    w[i] = x;
  }
}
static void print_words(const u32 w[8]) {
  for (int i = 0; i < 8; ++i) printf("%02x%02x%02x%02x", w[i] & 255u, (w[i] >> 8) & 255u, (w[i] >> 16) & 255u, w[i] >> 24);
}

// the arrays of a call, laid out as the entry lays them out
struct StatusArr {
  const std::vector<u32>* st;      // [k][m], or null
  size_t m;
  bool accepted(int j, u32 c) const { return !st || st->at((size_t)j * m + c) == 0u; }
};
// items of columns that are not accepted must never be read: reading one is an error here
struct ItemsArr {
  const std::vector<uint8_t>* items;
  StatusArr status;
  size_t m;
  void load(u32 w[8], int j, u32 c, int part) const {
    CHECK(status.accepted(j, c), "the item of rejected column %d of ciphertext %u was read", j, c);
    words_of(w, *items, ((size_t)j * m + c) * 128 + (size_t)part * 32);
  }
};
struct CtArr {
  const std::vector<uint8_t>* cts;
  void load(u32 w[8], u32 c, int part) const { words_of(w, *cts, (size_t)c * 64 + (size_t)part * 32); }
};
// [i][word][lane], as ScCoefDev
struct CoefArr {
  std::vector<u32>* v;
  std::vector<char>* written;
  size_t lanes, lane;
  void store(int i, const u32 w[8]) {
    for (int q = 0; q < 8; ++q) v->at((size_t)(i * 8 + q) * lanes + lane) = w[q];
    written->at((size_t)i * lanes + lane) = 1;
  }
  void load(u32 w[8], int i) const {
    CHECK(written->at((size_t)i * lanes + lane), "coefficient %d read before it was written", i);
    for (int q = 0; q < 8; ++q) w[q] = v->at((size_t)(i * 8 + q) * lanes + lane);
  }
};
struct TableArr {
  std::vector<ge_cached>* v;
  size_t at0;
  void store(int e, const ge_cached& c) { v->at(at0 + (size_t)e) = c; }
  void load(ge_cached& c, int e) const { c = v->at(at0 + (size_t)e); }
};
struct TablesArr {
  std::vector<ge_cached>* v;       // [lane][chunk][8]
  size_t lane;
  int chunk;
  TableArr at(int n) const {
    CHECK(n >= 0 && n < chunk, "table %d of %d", n, chunk);
    return TableArr{v, (lane * (size_t)chunk + (size_t)n) * 8};
  }
};
struct DigitsArr {
  std::vector<u32> d = std::vector<u32>((size_t)SC_CHUNK * 8);
  void store(int n, int q, u32 x) { d.at((size_t)n * 8 + (size_t)q) = x; }
  int digit(int n, int i) const {
    const u32 w = d.at((size_t)n * 8 + (size_t)(i >> 3));
    const int nib = (int)((w >> (4 * (i & 7))) & 15u);
    return nib >= 8 ? nib - 16 : nib;
  }
};

// FILE: one line per case: "k mask idx_0 .. idx_(k-1)"
static int cmd_coeffs(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  int k;
  unsigned long long mask;
  while (fscanf(f, "%d %llu", &k, &mask) == 2) {
    if (k < 1 || k > 64) { fprintf(stderr, "bad line\n"); fclose(f); return 2; }
    std::vector<unsigned char> idx((size_t)k);
    for (int j = 0; j < k; ++j) {
      unsigned v;
      if (fscanf(f, "%u", &v) != 1 || v >= 64u) { fprintf(stderr, "bad index\n"); fclose(f); return 2; }
      idx[(size_t)j] = (unsigned char)v;
    }
    const u32 t = (u32)__builtin_popcountll(mask);
    if (!t || !sc_mask_valid((u64)mask, k, t)) { fprintf(stderr, "bad mask\n"); fclose(f); return 2; }
    const size_t lanes = 3, lane = 1;                  // a lane in the middle of a small slab: the stride is live
    std::vector<u32> v(lanes * t * 8, 0xdeadbeefu);
    std::vector<char> written(lanes * t, 0);
    CoefArr coef{&v, &written, lanes, lane};
    sc_lane_coeffs((u64)mask, idx.data(), coef);
    printf("COEF");
    for (u32 i = 0; i < t; ++i) {
      u32 w[8];
      coef.load(w, (int)i);
      CHECK(sc_is_canonical(w), "coefficient %u is not canonical", i);
      printf(" ");
      print_words(w);
    }
    printf("\n");
    for (size_t e = 0; e < v.size(); ++e)
      if (e % lanes != lane) CHECK(v[e] == 0xdeadbeefu, "a neighbour lane's coefficient word %zu was written", e);
  }
  fclose(f);
  return 0;
}

static int cmd_layout(char** argv) {
  const uint64_t t = strtoull(argv[2], nullptr, 10);
  const size_t m = (size_t)strtoull(argv[3], nullptr, 10);
  const egsc::Layout L = egsc::layout(t, m);
  printf("LAYOUT lanes %zu mask %zu coef %zu tables %zu total %zu chunk %d bytes %zu\n", L.lanes, L.mask, L.coef, L.tables, L.total, L.chunk,
         egsc::scratch_bytes(t, m));
  return 0;
}

// FILE: "shares threshold m k have_status want_plain", then k indexes, then per ciphertext one line "ct-hex" and k lines "status item-hex"
static int cmd_run(char** argv) {
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  unsigned long long shares = 0, threshold = 0;
  unsigned m = 0, have_status = 0, want_plain = 0;
  int k = 0;
  if (fscanf(f, "%llu %llu %u %d %u %u", &shares, &threshold, &m, &k, &have_status, &want_plain) != 6) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  std::vector<uint64_t> indexes((size_t)(k > 0 ? k : 0));
  for (int j = 0; j < k; ++j) {
    unsigned long long v;
    if (fscanf(f, "%llu", &v) != 1) { fprintf(stderr, "bad index\n"); fclose(f); return 2; }
    indexes[(size_t)j] = v;
  }
  const char* why = egsc::refuse_sizes(shares, threshold, m);
  if (!why) why = egsc::refuse_columns(shares, k, indexes.data());
  if (why) { fprintf(stderr, "refused: %s\n", why); fclose(f); return 2; }
  std::vector<uint8_t> cts((size_t)m * 64), items((size_t)k * m * 128), tmp;
  std::vector<u32> status((size_t)k * m);
  std::vector<char> line(300);
  for (unsigned c = 0; c < m; ++c) {
    if (fscanf(f, "%299s", line.data()) != 1 || !unhex(tmp, line.data(), 64)) { fprintf(stderr, "bad ciphertext %u\n", c); fclose(f); return 2; }
    memcpy(&cts[(size_t)c * 64], tmp.data(), 64);
    for (int j = 0; j < k; ++j) {
      unsigned st;
      if (fscanf(f, "%u %299s", &st, line.data()) != 2 || !unhex(tmp, line.data(), 128)) { fprintf(stderr, "bad item %u/%d\n", c, j); fclose(f); return 2; }
      status[(size_t)j * m + c] = st;
      memcpy(&items[((size_t)j * m + c) * 128], tmp.data(), 128);
    }
  }
  fclose(f);

  const u32 t = (u32)threshold;
  const egsc::Layout L = egsc::layout(threshold, m);
  CHECK(L.lanes >= m || L.lanes == egsc::SLAB, "a slab of %zu lanes for %u ciphertexts", L.lanes, m);
  CHECK(L.coef - L.mask >= L.lanes * 8 && L.tables - L.coef >= L.lanes * t * 32 && L.total - L.tables >= L.lanes * (size_t)L.chunk * egsc::TABLE_BYTES,
        "a part of the scratch is too small");
  unsigned char idx[egsc::MAX_SHARES] = {0};
  for (int j = 0; j < k; ++j) idx[j] = (unsigned char)indexes[(size_t)j];
  const StatusArr st{have_status ? &status : nullptr, m};
  const ItemsArr it{&items, st, m};
  const CtArr ct{&cts};
  std::vector<u64> masks(L.lanes, 0);
  std::vector<u32> coefv(L.lanes * t * 8, 0);
  std::vector<char> written(L.lanes * t, 0);
  std::vector<ge_cached> tables(L.lanes * (size_t)L.chunk * 8);
  u32 bad[3] = {0, 0, 0};
  // the three stages, each over the whole slab before the next begins, as three launches do
  for (u32 c = 0; c < m; ++c) masks.at(c) = sc_lane_select(bad[0], c, k, t, st, it, ct);
  if ((unsigned long long)k >= threshold)
    for (u32 c = m; c-- > 0;) {                          // from the last lane down: the order of lanes must not matter
      if (!sc_mask_valid(masks.at(c), k, t)) continue;
      CoefArr coef{&coefv, &written, L.lanes, c};
      sc_lane_coeffs(masks.at(c), idx, coef);
    }
  for (u32 c = 0; c < m; ++c) {
    u64 mask = masks.at(c);
    if (!sc_mask_valid(mask, k, t)) mask = 0;
    u32 dh[8] = {0}, plain[8] = {0};
    bool ok = mask != 0u;
    if (ok) {
      const CoefArr coef{&coefv, &written, L.lanes, c};
      TablesArr tabs{&tables, c, L.chunk};
      DigitsArr dig;
      ge D;
      u32 bad1 = 0, bad2 = 0;
      sc_lane_combine(D, bad1, mask, c, it, coef, tabs, dig);
      ok = bad1 == 0u;
      if (ok) ok = sc_lane_finish(dh, plain, want_plain != 0, bad2, c, D, ct);
      bad[1] += bad1; bad[2] += bad2;
      if (!ok) for (int q = 0; q < 8; ++q) { dh[q] = 0u; plain[q] = 0u; }
    }
    printf("CT %u %d %" PRIu64 " ", c, ok ? 1 : 0, ok ? (uint64_t)sc_used_of(mask, k, idx) : (uint64_t)0);
    print_words(dh);
    printf(" ");
    print_words(plain);
    printf("\n");
  }
  printf("BAD %u %u %u\n", bad[0], bad[1], bad[2]);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc == 3 && strcmp(argv[1], "coeffs") == 0) {
    rc = cmd_coeffs(argv);
  } else if (argc == 4 && strcmp(argv[1], "layout") == 0) {
    rc = cmd_layout(argv);
  } else if (argc == 3 && strcmp(argv[1], "run") == 0) {
    rc = cmd_run(argv);
  } else {
    fprintf(stderr, "usage: sharecombinecheck coeffs FILE | layout t m | run FILE\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
