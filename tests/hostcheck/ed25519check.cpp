// Host build of the Ed25519 pass (elastic_elgamal_amd/csrc/sha512.cuh, ed25519.cuh, ed25519_host.hpp) with -DEG_BOUNDCHECK under
// ASan + UBSan: the lane functions of the kernels run serially on arrays.  Every byte range handed to the hash lives in a heap allocation
// that ends where the range ends, at a chosen offset mod 8, so a read past a range aborts the program; every field operation asserts its
// limb-class precondition.
// Stand-alone program (tests/test_ed25519_cpu.py builds it and reads its report); "-" stands for an empty hex string:
//   ed25519check sha FILE        lines "shift l0 l1 l2 msghex digesthex": the message cut into ranges of l0, l1, l2 and the rest, each
//                                starting at address = shift mod 8
//   ed25519check codec FILE      lines "enchex expect": 0 decodes, re-encodes to itself and has large order; 2 refused; 3 small order
//   ed25519check verify FILE     lines "prefixhex msghex keyhex sighex status": the hash lane and the verify lane, the exact status word
//   ed25519check sign FILE       lines "seedhex prefixhex msghex keyhex sighex": the key-pair lane and the sign lane, byte for byte
//   ed25519check layout N CUS    the parts of the scratch
//   ed25519check refuse N HAVE_MSGS STRIDE LEN HAVE_PREFIX PREFIX_LEN N_KEYS HAVE_INDEX
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
#include "../../elastic_elgamal_amd/csrc/ed25519.cuh"
#include "../../elastic_elgamal_amd/csrc/ed25519_host.hpp"

using namespace eg;

static unsigned long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// the lane's radix-16 table
struct ArrTable {
  ge_cached e[8];
  void store(int i, const ge_cached& c) { if (i < 0 || i > 7) abort(); e[i] = c; }
  void load(ge_cached& c, int i) const { if (i < 0 || i > 7) abort(); c = e[i]; }
};
// comb table of B with entries made on demand (the product's has millions; a comb touches one per window)
struct NielsOnDemand {
  int bits = 8;
  mutable std::map<int, ge_niels> cache;
  void load(ge_niels& c, int idx) const {
    if (idx < 0 || idx >= comb_windows(bits) * comb_entries(bits)) abort();
    auto it = cache.find(idx);
    if (it == cache.end()) {
      const int w = idx / comb_entries(bits), k = idx % comb_entries(bits) + 1;
      ge p; ge_generator(p);
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
static NielsOnDemand g_tab;

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static bool unhex(std::vector<uint8_t>& out, const char* s) {
  out.clear();
  if (strcmp(s, "-") == 0) return true;
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
// a byte range in an allocation of its own that ends with it and starts at `shift` mod 8 (operator new[] returns 16-byte aligned memory)
struct Range {
  std::unique_ptr<uint8_t[]> mem;
  uint8_t* p;
  size_t len;
  Range(const uint8_t* src, size_t n, unsigned shift) : mem(new uint8_t[(shift & 7u) + n + 0]), p(mem.get() + (shift & 7u)), len(n) {
    memset(mem.get(), 0xEE, shift & 7u);
    if (n) memcpy(p, src, n);
  }
};
static std::vector<char> g_line(1 << 16);
static bool next_tokens(FILE* f, std::vector<std::string>& tok, size_t want) {
  tok.clear();
  for (size_t i = 0; i < want; ++i) {
    if (fscanf(f, "%65535s", g_line.data()) != 1) return false;
    tok.emplace_back(g_line.data());
  }
  return true;
}

static int cmd_sha(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  std::vector<std::string> t;
  std::vector<uint8_t> msg, want;
  unsigned long long cases = 0;
  while (next_tokens(f, t, 6)) {
    const unsigned shift = (unsigned)strtoul(t[0].c_str(), nullptr, 10);
    size_t l[4] = {strtoull(t[1].c_str(), nullptr, 10), strtoull(t[2].c_str(), nullptr, 10), strtoull(t[3].c_str(), nullptr, 10), 0};
    if (!unhex(msg, t[4].c_str()) || !unhex(want, t[5].c_str()) || want.size() != 64 || l[0] + l[1] + l[2] > msg.size()) { fprintf(stderr, "bad sha line\n"); fclose(f); return 2; }
    l[3] = msg.size() - l[0] - l[1] - l[2];
    const Range r0(msg.data(), l[0], shift), r1(msg.data() + l[0], l[1], shift + 1), r2(msg.data() + l[0] + l[1], l[2], shift + 3),
        r3(msg.data() + l[0] + l[1] + l[2], l[3], shift + 5);
    u32 dg[16];
    sha512_ranges(dg, sha_ranges(r0.p, r0.len, r1.p, r1.len, r2.p, r2.len, r3.p, r3.len));
    uint8_t got[64];
    ed_words_to_bytes(got, dg, 16);
    CHECK(memcmp(got, want.data(), 64) == 0, "sha512 of %zu bytes cut %zu %zu %zu %zu shift %u", msg.size(), l[0], l[1], l[2], l[3], shift);
    ++cases;
  }
  fclose(f);
  printf("SHA %llu\n", cases);
  return 0;
}

static int cmd_codec(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  std::vector<std::string> t;
  std::vector<uint8_t> enc;
  unsigned long long cases = 0;
  while (next_tokens(f, t, 2)) {
    const int expect = atoi(t[1].c_str());
    if (!unhex(enc, t[0].c_str()) || enc.size() != 32) { fprintf(stderr, "bad codec line\n"); fclose(f); return 2; }
    u32 w[8], back[8];
    words_of(w, enc.data(), 8);
    ge p;
    const bool ok = ed_decode(p, w);
    if (expect == 2) { CHECK(!ok, "%s decodes", t[0].c_str()); }
    else {
      CHECK(ok, "%s does not decode", t[0].c_str());
      if (ok) {
        ed_encode(back, p);
        CHECK(memcmp(back, w, 32) == 0, "%s does not re-encode to itself", t[0].c_str());
        CHECK(ed_is_small_order(p) == (expect == 3), "%s: small order %d expected %d", t[0].c_str(), (int)ed_is_small_order(p), expect == 3);
        // a projective form of the same point encodes alike
        ge d, q; ge_dbl_full(d, p); ge_add_full(q, d, p);     // 3P with Z != 1
        ge n; ge_neg(n, d); ge r; ge_add_full(r, q, n);       // 3P - 2P
        ed_encode(back, r);
        CHECK(memcmp(back, w, 32) == 0, "%s: 3P - 2P encodes differently", t[0].c_str());
      }
    }
    ++cases;
  }
  fclose(f);
  printf("CODEC %llu\n", cases);
  return 0;
}

// the two kernels' lanes for one item: what k_ed25519_hash parks, then what k_ed25519_verify writes
static u32 verify_item(const std::vector<uint8_t>& prefix, const std::vector<uint8_t>& msg, const std::vector<uint8_t>& key, const std::vector<uint8_t>& sig,
                       bool* h_zero = nullptr) {
  u32 Rw[8], Sw[8], Aw[8], hw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  words_of(Rw, sig.data(), 8); words_of(Sw, sig.data() + 32, 8); words_of(Aw, key.data(), 8);
  if (sc_is_canonical(Sw)) {
    const Range r(sig.data(), 32, 0), a(key.data(), 32, 4), p(prefix.data(), prefix.size(), 1), m(msg.data(), msg.size(), 1 + (unsigned)prefix.size());
    ed_hash_mod_l(hw, sha_ranges(r.p, 32, a.p, 32, p.p, p.len, m.p, m.len));
  }
  if (h_zero) { u32 any = 0; for (int i = 0; i < 8; ++i) any |= hw[i]; *h_zero = any == 0; }
  ArrTable tab;
  return ed_status(ed_verify_lane(tab, g_tab, Rw, Sw, Aw, hw));
}
static int cmd_verify(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  std::vector<std::string> t;
  std::vector<uint8_t> prefix, msg, key, sig;
  unsigned long long cases = 0, accepted = 0;
  while (next_tokens(f, t, 5)) {
    if (!unhex(prefix, t[0].c_str()) || !unhex(msg, t[1].c_str()) || !unhex(key, t[2].c_str()) || !unhex(sig, t[3].c_str()) || key.size() != 32 || sig.size() != 64) {
      fprintf(stderr, "bad verify line\n"); fclose(f); return 2;
    }
    const u32 want = (u32)strtoul(t[4].c_str(), nullptr, 10), got = verify_item(prefix, msg, key, sig);
    CHECK(got == want, "verify case %llu: status %u, expected %u", cases, got, want);
    accepted += got == 0;
    ++cases;
  }
  fclose(f);
  printf("VERIFY %llu ACCEPTED %llu\n", cases, accepted);
  return 0;
}

static int cmd_sign(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  std::vector<std::string> t;
  std::vector<uint8_t> seed, prefix, msg, key, sig;
  unsigned long long cases = 0;
  while (next_tokens(f, t, 5)) {
    if (!unhex(seed, t[0].c_str()) || !unhex(prefix, t[1].c_str()) || !unhex(msg, t[2].c_str()) || !unhex(key, t[3].c_str()) || !unhex(sig, t[4].c_str()) ||
        seed.size() != 32 || key.size() != 32 || sig.size() != 64) { fprintf(stderr, "bad sign line\n"); fclose(f); return 2; }
    const Range s(seed.data(), 32, 3), p(prefix.data(), prefix.size(), 5), m(msg.data(), msg.size(), 7);
    u32 Aw[8], sg[16];
    ed_keypair_lane(Aw, g_tab, s.p);
    uint8_t got[64];
    ed_words_to_bytes(got, Aw, 8);
    CHECK(memcmp(got, key.data(), 32) == 0, "sign case %llu: public key differs", cases);
    ed_sign_lane(sg, g_tab, s.p, p.p, p.len, m.p, m.len);
    ed_words_to_bytes(got, sg, 16);
    CHECK(memcmp(got, sig.data(), 64) == 0, "sign case %llu: signature differs", cases);
    // what was signed verifies; S = 0 and h = 0 cannot be made without inverting the hash, so the nearest constructions: the key [a]B with
    // R = the identity's encoding and S = 0 holds exactly when h = 0, and must otherwise be a mismatch - never a crash of the zero digits
    CHECK(verify_item(prefix, msg, key, sig) == 0, "sign case %llu: the signature does not verify", cases);
    std::vector<uint8_t> zero_sig(64, 0); zero_sig[0] = 1;
    bool h_zero = false;
    const u32 st = verify_item(prefix, msg, key, zero_sig, &h_zero);
    CHECK(st == (h_zero ? 0u : ed_status(ED_MISMATCH)), "sign case %llu: S = 0 under R = identity gives %u", cases, st);
    // h = 0 handed to the verify lane itself (the hash lane cannot be made to give it): R' = [S]B, all sixty-four digits of the chain zero
    {
      u32 Rw[8], Sw[8], hw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      words_of(Sw, sig.data() + 32, 8);
      ed_mul_base_encode(Rw, g_tab, Sw);
      ArrTable tab;
      CHECK(ed_verify_lane(tab, g_tab, Rw, Sw, Aw, hw) == ED_OK, "sign case %llu: h = 0 with R = [S]B", cases);
      Rw[0] ^= 1u;
      CHECK(ed_verify_lane(tab, g_tab, Rw, Sw, Aw, hw) == ED_MISMATCH, "sign case %llu: h = 0 with another R", cases);
    }
    ++cases;
  }
  fclose(f);
  printf("SIGN %llu\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc == 3 && strcmp(argv[1], "sha") == 0) rc = cmd_sha(argv[2]);
  else if (argc == 3 && strcmp(argv[1], "codec") == 0) rc = cmd_codec(argv[2]);
  else if (argc == 3 && strcmp(argv[1], "verify") == 0) rc = cmd_verify(argv[2]);
  else if (argc == 3 && strcmp(argv[1], "sign") == 0) rc = cmd_sign(argv[2]);
  else if (argc == 4 && strcmp(argv[1], "layout") == 0) {
    const eged::Layout L = eged::layout(strtoull(argv[2], nullptr, 10), (unsigned)strtoul(argv[3], nullptr, 10));
    printf("LAYOUT blocks %u prefix %zu h %zu tables %zu total %zu\n", L.blocks, L.prefix, L.h, L.tables, L.total);
    CHECK(eged::TABLE_BYTES == 8 * 4 * EG_NL * sizeof(u32), "a table is 8 cached entries of 4 x EG_NL limbs");
  } else if (argc == 10 && strcmp(argv[1], "refuse") == 0) {
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    const char* why = eged::refuse_messages(num(2), num(3) != 0, num(4), num(5), num(6) != 0, num(7));
    if (!why) why = eged::refuse_roster(num(2), num(8), num(9) != 0);
    printf("REFUSE %s\n", why ? why : "-");
  } else {
    fprintf(stderr, "usage: ed25519check sha|codec|verify|sign FILE | layout N CUS | refuse N HAVE_MSGS STRIDE LEN HAVE_PREFIX PREFIX_LEN N_KEYS HAVE_INDEX\n");
    return 2;
  }
  if (rc) return rc;
  printf(g_fail ? "FAIL %llu\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
