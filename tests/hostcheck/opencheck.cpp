// Host build of the ballot-audit pass (elastic_elgamal_amd/csrc/open_kernels.cuh, open_host.hpp) with -DEG_BOUNDCHECK under ASan + UBSan:
// the lane functions of k_open_check and k_open_resolve run serially on arrays.  Every ballot, its values and its randomness live in heap
// allocations of their own that end where the data ends, and those of a ballot that does not participate are poisoned, so that reading
// them aborts the program; every field operation asserts its limb-class precondition.  The comb tables of G and K are made on demand.
// Stand-alone program (tests/test_open_cpu.py builds it and reads its report):
//   opencheck run FILE            the check lanes (in reverse order: no lane depends on another) and the resolve lanes over the case of
//                                 FILE; every encoding the halved-scalar encoder made is compared with a plain ristretto_encode of the
//                                 point computed by double-and-add.  Prints STATUS, FOUND and NOGUARD: the status words of the same lanes
//                                 with check 1 compiled out.
//   opencheck layout N N_SLOTS    the parts of the scratch
//   opencheck refuse N MASK N_SLOTS QUADS WORDS64 WORDS32   what the argument rules say; MASK: bit k = pointer k of ego::Have is there
//   opencheck draws choice SKIP BITS    the draw of every option's r; BITS = a string of 0 / 1, character k = option k chosen
//   opencheck draws qv SKIP N_OPTIONS N_RINGS SIZES_SUM
// FILE: "key_hex n n_slots stride have_status alias", n_slots item indices, then n lines "status ballot_hex v_0 .. r_hex_0 ..".
// exit code 0 = every internal check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../elastic_elgamal_amd/csrc/open_kernels.cuh"

using namespace eg;

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// comb table of a base with entries made on demand (the product's has millions; a comb touches one per window)
struct NielsOnDemand {
  int bits = 8;
  ge base;
  mutable std::map<int, ge_niels> cache;
  void load(ge_niels& c, int idx) const {
    if (idx < 0 || idx >= comb_windows(bits) * comb_entries(bits)) abort();
    auto it = cache.find(idx);
    if (it == cache.end()) {
      const int w = idx / comb_entries(bits), k = idx % comb_entries(bits) + 1;
      ge p = base;
      for (int i = 0; i < bits * w; ++i) { ge d; ge_dbl_full(d, p); p = d; }
      ge q; ge_identity(q);
      for (int bit = bits - 1; bit >= 0; --bit) {
        ge d; ge_dbl_full(d, q); q = d;
        if ((k >> bit) & 1) { ge t; ge_add_full(t, q, p); q = t; }
      }
      ge_niels n; ge_to_niels(n, q);
      it = cache.emplace(idx, n).first;
    }
    c = it->second;
  }
};
// [k]P by double-and-add over all 256 bits: no comb, no halving
static ge mul_plain(const ge& p, const u32 k[8]) {
  ge q; ge_identity(q);
  for (int bit = 255; bit >= 0; --bit) {
    ge d; ge_dbl_full(d, q); q = d;
    if ((k[bit >> 5] >> (bit & 31)) & 1u) { ge t; ge_add_full(t, q, p); q = t; }
  }
  return q;
}

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static bool unhex(std::vector<uint8_t>& out, const char* s) {
  out.clear();
  const size_t len = strlen(s);
  if (len % 2) return false;
  for (size_t i = 0; i < len; i += 2) {
    const int a = hexval(s[i]), b = hexval(s[i + 1]);
    if (a < 0 || b < 0) return false;
    out.push_back((uint8_t)(a * 16 + b));
  }
  return true;
}
static void words_of(u32* w, const uint8_t* p, int words) {
  for (int i = 0; i < words; ++i) w[i] = (u32)p[4 * i] | ((u32)p[4 * i + 1] << 8) | ((u32)p[4 * i + 2] << 16) | ((u32)p[4 * i + 3] << 24);
}

struct MemArr {
  std::vector<std::unique_ptr<uint8_t[]>> ballots;         // each `stride` bytes
  std::vector<std::unique_ptr<uint64_t[]>> values;         // each n_slots
  std::vector<std::unique_ptr<uint8_t[]>> rands;           // each n_slots x 32
  std::vector<uint32_t> items;                             // the wire item of every slot's R
  std::vector<uint32_t> words;
  size_t stride = 0;
  u32 n_slots = 0;
  void rand(u32 w[8], u64 i) const { words_of(w, rands.at(i / n_slots).get() + (i % n_slots) * 32, 8); }
  u64 value(u64 i) const { return values.at(i / n_slots)[i % n_slots]; }
  void wire(u32 w[16], u64 b, u32 t) const {
    const size_t off = (size_t)items.at(t) * 32;
    if (off + 64 > stride) abort();
    words_of(w, ballots.at(b).get() + off, 16);
  }
  u32 word(u64 i) const { return words.at(i); }
};

static std::vector<char> g_tok(1 << 20);
static bool next_token(FILE* f, std::string& out) {
  if (fscanf(f, "%1048575s", g_tok.data()) != 1) return false;
  out = g_tok.data();
  return true;
}

static int cmd_run(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  std::string t;
  std::vector<uint8_t> raw;
  auto num = [&]() -> unsigned long long { return next_token(f, t) ? strtoull(t.c_str(), nullptr, 10) : 0ull; };
  if (!next_token(f, t) || !unhex(raw, t.c_str()) || raw.size() != 32) { fprintf(stderr, "bad key\n"); fclose(f); return 2; }
  u32 kw[8];
  words_of(kw, raw.data(), 8);
  NielsOnDemand tg, tk;
  ge_generator(tg.base);
  if (!ristretto_decode(tk.base, kw)) { fprintf(stderr, "the key does not decode\n"); fclose(f); return 2; }
  const size_t n = num();
  MemArr m;
  m.n_slots = (u32)num();
  m.stride = num();
  const bool have_status = num() != 0, alias = num() != 0;
  for (u32 s = 0; s < m.n_slots; ++s) m.items.push_back((uint32_t)num());
  std::vector<uint32_t> status_in(n, 0u);
  for (size_t b = 0; b < n; ++b) {
    status_in[b] = (uint32_t)num();
    if (!next_token(f, t) || !unhex(raw, t.c_str()) || raw.size() != m.stride) { fprintf(stderr, "bad ballot %zu\n", b); fclose(f); return 2; }
    m.ballots.emplace_back(new uint8_t[m.stride]);
    memcpy(m.ballots.back().get(), raw.data(), m.stride);
    m.values.emplace_back(new uint64_t[m.n_slots]);
    for (u32 s = 0; s < m.n_slots; ++s) m.values.back()[s] = num();
    m.rands.emplace_back(new uint8_t[(size_t)m.n_slots * 32]);
    for (u32 s = 0; s < m.n_slots; ++s) {
      if (!next_token(f, t) || !unhex(raw, t.c_str()) || raw.size() != 32) { fprintf(stderr, "bad randomness %zu %u\n", b, s); fclose(f); return 2; }
      memcpy(m.rands.back().get() + (size_t)s * 32, raw.data(), 32);
    }
  }
  fclose(f);
  const uint32_t* sin = have_status ? status_in.data() : nullptr;
  auto part = [&](size_t b) { return !sin || sin[b] == 0u; };
  for (size_t b = 0; b < n; ++b)
    if (!part(b)) {
      ASAN_POISON_MEMORY_REGION(m.ballots[b].get(), m.stride);
      ASAN_POISON_MEMORY_REGION(m.values[b].get(), m.n_slots * sizeof(uint64_t));
      ASAN_POISON_MEMORY_REGION(m.rands[b].get(), (size_t)m.n_slots * 32);
    }
  const ego::Layout L = ego::layout(n, m.n_slots);
  CHECK(L.total >= n * m.n_slots * 4 && L.words == 0, "the layout has no room for the words");
  unsigned long long encoded = 0;
  std::vector<uint32_t> out_words[2];
  for (int guard = 1; guard >= 0; --guard) {
    m.words.assign(n * (size_t)m.n_slots, 0xdeadbeefu);              // words of other ballots are never read: resolve must not see these
    for (size_t i = n * (size_t)m.n_slots; i-- > 0;) {
      const u64 b = i / m.n_slots;
      const u32 s = (u32)(i % m.n_slots);
      if (!part(b)) continue;
      u32 enc[16] = {0}, r[8];
      m.rand(r, i);
      const bool reached = sc_is_canonical(r);                        // (beyond l the plain product below is another point)
      const u32 chk = guard ? ego::open_lane_check<true>(m, tg, tk, b, s, m.n_slots, enc) : ego::open_lane_check<false>(m, tg, tk, b, s, m.n_slots, enc);
      m.words[i] = ego::open_lane_word(s, chk);
      if (reached) {                                                  // the halved-scalar encoder against the plain one
        u32 v[8], want[8];
        sc_from_u64(v, m.value(i));
        const ge pr = mul_plain(tg.base, r), pv = mul_plain(tg.base, v), pk = mul_plain(tk.base, r);
        ge pb; ge_add_full(pb, pv, pk);
        ristretto_encode(want, pr);
        CHECK(memcmp(want, enc, 32) == 0, "ballot %" PRIu64 " slot %u: [r]G encodes differently", b, s);
        ristretto_encode(want, pb);
        CHECK(memcmp(want, enc + 8, 32) == 0, "ballot %" PRIu64 " slot %u: [v]G + [r]K encodes differently", b, s);
        ++encoded;
      }
    }
    std::vector<uint32_t> status_out(n, 0xabababu);
    if (alias) status_out = status_in;
    uint32_t found[2] = {0, 0};
    for (size_t b = 0; b < n; ++b) {
      const uint32_t st = sin ? (alias ? status_out[b] : sin[b]) : 0u;
      bool failed;
      status_out[b] = ego::open_lane_resolve(m, b, m.n_slots, st, part(b), failed);
      found[0] += part(b);
      found[1] += failed;
    }
    out_words[guard] = status_out;
    if (guard) printf("FOUND : %u %u\n", found[0], found[1]);
  }
  printf("STATUS :");
  for (uint32_t w : out_words[1]) printf(" %u", w);
  printf("\nNOGUARD :");
  for (uint32_t w : out_words[0]) printf(" %u", w);
  printf("\nENCODED %llu\n", encoded);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
  if (argc == 3 && strcmp(argv[1], "run") == 0) rc = cmd_run(argv[2]);
  else if (argc == 4 && strcmp(argv[1], "layout") == 0) {
    const ego::Layout L = ego::layout(num(2), (uint32_t)num(3));
    printf("LAYOUT words %zu total %zu\n", L.words, L.total);
  } else if (argc == 8 && strcmp(argv[1], "refuse") == 0) {
    const unsigned long long mask = num(3);
    const ego::Have h{(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0, (mask & 16) != 0};
    const char* why = ego::refuse(num(2), h);
    if (!why) why = ego::refuse_alignment(num(5), num(6), num(7));
    if (!why) why = ego::refuse_items(num(2), (uint32_t)num(4));
    printf("REFUSE %s\n", why ? why : "-");
  } else if (argc == 5 && strcmp(argv[1], "draws") == 0 && strcmp(argv[2], "choice") == 0) {
    printf("DRAWS :");
    uint32_t skipped = 0;
    for (uint32_t k = 0; argv[4][k]; ++k) {
      printf(" %" PRIu64, ego::choice_r_draw(num(3), k, skipped));
      skipped += argv[4][k] == '0';
    }
    printf("\n");
  } else if (argc == 7 && strcmp(argv[1], "draws") == 0 && strcmp(argv[2], "qv") == 0) {
    printf("DRAWS :");
    for (uint32_t k = 0; k < num(4); ++k) printf(" %" PRIu64, ego::qv_r_draw(num(3), k, ego::range_draws((uint32_t)num(5), num(6))));
    printf("\n");
  } else {
    fprintf(stderr, "usage: opencheck run FILE | layout N N_SLOTS | refuse N MASK N_SLOTS QUADS WORDS64 WORDS32 | draws choice SKIP BITS | draws qv SKIP N_OPTIONS N_RINGS SIZES_SUM\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
