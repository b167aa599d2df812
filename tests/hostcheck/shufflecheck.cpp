// Host build of the shuffle verifier (elastic_elgamal_amd/csrc/shuffle_kernels.cuh, shuffle_host.hpp) with -DEG_BOUNDCHECK under
// ASan + UBSan: the lane functions of the kernels run serially on arrays, in the arrangement of the kernels - the chain rows in tiles of
// 63 with the neighbour's point handed over in plain code.  The two roots are a bottom-up tree over H32 made here, and the five sums
// (which the library takes from its product entry) are plain double-and-add sums, so the closing lane sees what it sees on the device.
// Stand-alone program (tests/test_shuffle_cpu.py builds it and compares its report with tests/shuffle_ref.py):
//   shufflecheck key FILE        lines "seedhex j tries": prints "used keyhex" per line (used = 0: exhausted)
//   shufflecheck hash FILE       lines "1 inhex outhex chex hhex" | "2 chathex thathex" | "seed prefixhex n Khex h0hex root1hex" |
//                                "u seed1hex i" | "x seed1hex root2hex headhex": prints the lane's output in hex per line
//   shufflecheck verify FILE     a statement and a proof: line "n prefixhex Khex", then keyhex (n + 1 generators), inhex, outhex, proofhex;
//                                prints "mask f0 f1 f2 f3" and the n row words
//   shufflecheck layout N CUS TREE MSM_BIG MSM_SMALL      fills every part of the scratch with a byte of its own behind a canary and
//                                prints "total chain_grid"; fails if parts overlap, leave the total or touch the canary
//   shufflecheck refuse N KEY_CAP IN OUT K PREFIX PREFIX_LEN KEY PROOF VERDICT FOUND      prints the refusal or "ok"
// exit code 0 = every internal check held.  "-" stands for an empty hex string.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../elastic_elgamal_amd/csrc/shuffle_kernels.cuh"

using namespace eg;

struct ArrTable {
  ge_cached e[8];
  void store(int i, const ge_cached& c) { if (i < 0 || i > 7) abort(); e[i] = c; }
  void load(ge_cached& c, int i) const { if (i < 0 || i > 7) abort(); c = e[i]; }
};
// comb table of G with entries made on demand (the product's has millions; a comb touches one per window)
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
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  if (s.size() % 2) { fprintf(stderr, "odd hex\n"); exit(2); }
  for (size_t i = 0; i < s.size(); i += 2) {
    const int a = hexval(s[i]), b = hexval(s[i + 1]);
    if (a < 0 || b < 0) { fprintf(stderr, "bad hex\n"); exit(2); }
    out.push_back((uint8_t)(a * 16 + b));
  }
  return out;
}
static std::vector<u32> words_of(const std::vector<uint8_t>& b) {
  if (b.size() % 4) { fprintf(stderr, "not whole words\n"); exit(2); }
  std::vector<u32> w(b.size() / 4);
  for (size_t i = 0; i < w.size(); ++i) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
  return w;
}
static void print_words(const u32* w, int n) {
  for (int i = 0; i < n; ++i) printf("%02x%02x%02x%02x", w[i] & 255, (w[i] >> 8) & 255, (w[i] >> 16) & 255, w[i] >> 24);
}
static std::vector<std::string> split(const std::string& line) {
  std::istringstream in(line);
  std::vector<std::string> out;
  for (std::string t; in >> t;) out.push_back(t);
  return out;
}

// MTH bottom up over 32-byte leaves (8 words each): node = H32(0x01 || l || r), an odd last node is promoted
static void mth(u32 root[8], std::vector<u32> level) {
  size_t n = level.size() / 8;
  if (n == 0) { u32 dg[16]; sha512_ranges(dg, sha_ranges(nullptr, 0)); memcpy(root, dg, 32); return; }
  while (n > 1) {
    std::vector<u32> up;
    for (size_t i = 0; i < n; i += 2) {
      if (i + 1 < n) {
        ShufMsg m; m.open(); m.byte(1); m.words(&level[i * 8], 8); m.words(&level[(i + 1) * 8], 8);
        u32 dg[16]; m.digest(dg);
        up.insert(up.end(), dg, dg + 8);
      } else up.insert(up.end(), &level[i * 8], &level[i * 8] + 8);
    }
    level.swap(up);
    n = level.size() / 8;
  }
  memcpy(root, level.data(), 32);
}

// out = enc(sum [k_t]P_t + [r]G), ok = every P_t decodes: what the product entry gives (scalars below l)
static bool product(u32 out[8], const std::vector<const u32*>& scalars, const std::vector<const u32*>& points, const u32 r[8]) {
  ge acc; ge_identity(acc);
  bool ok = true;
  for (size_t t = 0; t < scalars.size(); ++t) {
    ge p, q, s;
    ok = ristretto_decode(p, points[t]) && ok;
    ArrTable tab;
    ge_var_table_build(tab, p);
    u32 dg[8];
    sc_recode_radix16(dg, scalars[t]);
    ge_var_mul(q, tab, dg);
    ge_add_full(s, acc, q);
    acc = s;
  }
  u32 sk[EG_COMB_WORDS];
  sc_recode_comb(sk, r);
  ge_fixed_mul_add(acc, g_tab, sk);
  ristretto_encode(out, acc);
  return ok;
}

static int cmd_key(const char* file) {
  std::ifstream in(file);
  for (std::string line; std::getline(in, line);) {
    const auto f = split(line);
    if (f.size() != 3) continue;
    const auto seed = unhex(f[0]);
    u32 h[8];
    const u32 used = shuffle_key_lane(h, seed.data(), (u32)seed.size(), strtoull(f[1].c_str(), nullptr, 10), (u32)strtoul(f[2].c_str(), nullptr, 10));
    printf("%u ", used); print_words(h, 8); printf("\n");
  }
  return 0;
}

static int cmd_hash(const char* file) {
  std::ifstream in(file);
  for (std::string line; std::getline(in, line);) {
    const auto f = split(line);
    if (f.empty()) continue;
    if (f[0] == "1" && f.size() == 5) {
      const auto a = words_of(unhex(f[1])), b = words_of(unhex(f[2])), c = words_of(unhex(f[3])), h = words_of(unhex(f[4]));
      u32 leaf[8]; shuffle_leaf1_lane(leaf, a.data(), b.data(), c.data(), h.data()); print_words(leaf, 8);
    } else if (f[0] == "2" && f.size() == 3) {
      const auto a = words_of(unhex(f[1])), b = words_of(unhex(f[2]));
      u32 leaf[8]; shuffle_leaf2_lane(leaf, a.data(), b.data()); print_words(leaf, 8);
    } else if (f[0] == "seed" && f.size() == 6) {
      const auto p = unhex(f[1]);
      const auto K = words_of(unhex(f[3])), h0 = words_of(unhex(f[4])), r1 = words_of(unhex(f[5]));
      u32 s[16]; shuffle_seed_lane(s, p.data(), (u32)p.size(), strtoull(f[2].c_str(), nullptr, 10), K.data(), h0.data(), r1.data()); print_words(s, 16);
    } else if (f[0] == "u" && f.size() == 3) {
      const auto s = words_of(unhex(f[1]));
      u32 u[8]; shuffle_u_lane(u, s.data(), strtoull(f[2].c_str(), nullptr, 10)); print_words(u, 8);
    } else if (f[0] == "x" && f.size() == 4) {
      const auto s = words_of(unhex(f[1])), r2 = words_of(unhex(f[2])), head = words_of(unhex(f[3]));
      u32 x[8]; shuffle_x_lane(x, s.data(), r2.data(), head.data()); print_words(x, 8);
    } else { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    printf("\n");
  }
  return 0;
}

// the whole pass, stage by stage as eg_shuffle_verify_device launches it
static int cmd_verify(const char* file) {
  std::ifstream in(file);
  std::string l0, l1, l2, l3, l4;
  std::getline(in, l0); std::getline(in, l1); std::getline(in, l2); std::getline(in, l3); std::getline(in, l4);
  const auto f = split(l0);
  const size_t n = strtoull(f[0].c_str(), nullptr, 10);
  const auto prefix = unhex(f[1]);
  const auto K = words_of(unhex(f[2])), key = words_of(unhex(l1)), ins = words_of(unhex(l2)), outs = words_of(unhex(l3)), proof = words_of(unhex(l4));
  if (n == 0 || key.size() < (n + 1) * 8 || ins.size() != n * 16 || outs.size() != n * 16 || proof.size() != egsh::proof_bytes(n) / 4) { fprintf(stderr, "bad sizes\n"); return 2; }
  const u32 *c = &proof[72], *chat = c + n * 8, *that = chat + n * 8, *shat = that + n * 8, *sprime = shat + n * 8;
  // leaf1, the five decodings of a row
  std::vector<u32> leaves(n * 8);
  std::vector<unsigned char> rowbad(n);
  for (size_t i = 0; i < n; ++i) {
    shuffle_leaf1_lane(&leaves[i * 8], &ins[i * 16], &outs[i * 16], c + i * 8, &key[(i + 1) * 8]);
    bool ok = true;
    const u32* pts[5] = {&ins[i * 16], &ins[i * 16 + 8], &outs[i * 16], &outs[i * 16 + 8], c + i * 8};
    for (int k = 0; k < 5; ++k) { ge p; ok = ristretto_decode(p, pts[k]) && ok; }
    rowbad[i] = ok ? 0 : 1;
  }
  u32 root1[8], seed1[16], root2[8], x[8], negx[8];
  mth(root1, leaves);
  shuffle_seed_lane(seed1, prefix.data(), (u32)prefix.size(), n, K.data(), key.data(), root1);
  for (size_t i = 0; i < n; ++i) shuffle_leaf2_lane(&leaves[i * 8], chat + i * 8, that + i * 8);
  mth(root2, leaves);
  shuffle_x_lane(x, seed1, root2, proof.data());
  sc_neg(negx, x);
  // scalars: u_i, -x u_i, s'_i (0 when not canonical), the product of the u_i
  std::vector<u32> xu(n * 8), sp(n * 8);
  u32 u[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    u32 ui[8], p[8];
    shuffle_u_lane(ui, seed1, i);
    sc_mul(&xu[i * 8], negx, ui);
    sc_mul(p, u, ui); memcpy(u, p, 32);
    memcpy(&sp[i * 8], sprime + i * 8, 32);
    if (!sc_is_canonical(&sp[i * 8])) memset(&sp[i * 8], 0, 32);
  }
  // the chain kernel: tiles of 63 rows, lane l decodes element 63 tile + l - 1, lanes 1 .. 63 take lane l - 1's point
  std::vector<u32> rows(n);
  u32 found[4] = {0, 0, 0xffffffffu, 0xffffffffu};
  for (size_t tile = 0; tile < egsh::chain_tiles(n); ++tile) {
    ge pt[64];
    bool okp[64];
    for (int lane = 0; lane < 64; ++lane) {
      const size_t e = tile * egsh::WAVE_ROWS + (size_t)lane;
      u32 w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (e == 0) memcpy(w, key.data(), 32);
      else if (e <= n) memcpy(w, chat + (e - 1) * 8, 32);
      okp[lane] = ristretto_decode(pt[lane], w);
    }
    for (int lane = 1; lane < 64; ++lane) {
      const size_t e = tile * egsh::WAVE_ROWS + (size_t)lane;
      if (e > n) continue;
      const size_t row = e - 1;
      bool fails = false;
      if (shuffle_row_evaluates(okp[lane], okp[lane - 1], shat + row * 8, sprime + row * 8)) {
        ArrTable t0, t1;
        fails = shuffle_chain_row(t0, t1, g_tab, pt[lane], pt[lane - 1], negx, shat + row * 8, sprime + row * 8, that + row * 8);
      }
      const u32 word = shuffle_row_word(rowbad[row] != 0, okp[lane], shat + row * 8, sprime + row * 8, fails);
      rows[row] = word;
      if (word & SHUF_ROW_BAD) { ++found[0]; if (row < found[2]) found[2] = (u32)row; }
      if (word & SHUF_ROW_CHAIN) { ++found[1]; if (row < found[3]) found[3] = (u32)row; }
    }
  }
  // the fold lane's head scalars, then the products as the entry lays them out
  u32 s[4][8], zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ns4[8], xuu[8];
  u32 headbad = 0;
  for (int k = 0; k < 4; ++k) {
    memcpy(s[k], &proof[40 + k * 8], 32);
    if (!sc_is_canonical(s[k])) { headbad = 1; memset(s[k], 0, 32); }
  }
  sc_neg(ns4, s[3]);
  sc_mul(xuu, x, u);
  u32 out_big[32], out_small[16];
  unsigned char ok_big[4], ok_small[2];
  for (int prob = 0; prob < 4; ++prob) {
    std::vector<const u32*> sc_, pt_;
    for (size_t i = 0; i < n; ++i) {
      sc_.push_back(prob == 0 ? negx : &xu[i * 8]);
      pt_.push_back(prob < 2 ? c + i * 8 : prob == 2 ? &ins[i * 16 + 8] : &ins[i * 16]);
    }
    for (size_t i = 0; i < n; ++i) {
      sc_.push_back(prob == 0 ? x : &sp[i * 8]);
      pt_.push_back(prob < 2 ? &key[(i + 1) * 8] : prob == 2 ? &outs[i * 16 + 8] : &outs[i * 16]);
    }
    ok_big[prob] = product(out_big + prob * 8, sc_, pt_, prob == 0 ? s[0] : prob == 1 ? s[2] : prob == 2 ? zero : ns4) ? 1 : 0;
  }
  ok_small[0] = product(out_small, {negx, xuu}, {chat + (n - 1) * 8, key.data()}, s[1]) ? 1 : 0;
  ok_small[1] = product(out_small + 8, {ns4, zero}, {K.data(), key.data()}, zero) ? 1 : 0;
  const u32 mask = shuffle_close_lane(proof.data(), out_big, ok_big, out_small, ok_small, found, headbad);
  printf("%u %u %u %u %u\n", mask, found[0], found[1], found[2], found[3]);
  for (size_t i = 0; i < n; ++i) printf("%u%c", rows[i], i + 1 == n ? '\n' : ' ');
  return 0;
}

static int cmd_layout(char** a) {
  const uint64_t n = strtoull(a[0], nullptr, 10);
  const egsh::Layout L = egsh::layout(n, (unsigned)strtoul(a[1], nullptr, 10), strtoull(a[2], nullptr, 10), strtoull(a[3], nullptr, 10), strtoull(a[4], nullptr, 10));
  const size_t CANARY = 64;
  std::vector<unsigned char> buf(L.total + CANARY, 0xC5);
  struct Part { size_t off, bytes; };
  const size_t two_n = 2 * (size_t)n;
  const Part parts[] = {{L.prefix, 256}, {L.state, egsh::STATE_BYTES}, {L.leaves, (size_t)n * 32}, {L.rowbad, (size_t)n}, {L.tree, strtoull(a[2], nullptr, 10)},
                        {L.upart, (size_t)egsh::row_blocks(n) * 32}, {L.big_scalars, 4 * two_n * 32}, {L.big_points, 4 * two_n * 32}, {L.big_r, 128},
                        {L.big_out, 128}, {L.big_ok, 4}, {L.small_scalars, 128}, {L.small_points, 128}, {L.small_r, 64}, {L.small_out, 64}, {L.small_ok, 2},
                        {L.tables, (size_t)L.chain_grid * egsh::NT * 2 * egsh::TABLE_BYTES},
                        {L.msm, std::max<size_t>(strtoull(a[3], nullptr, 10), strtoull(a[4], nullptr, 10))}};
  int id = 1, bad = 0;
  for (const Part& p : parts) {
    if (p.off % 256 || p.off + p.bytes > L.total) { fprintf(stderr, "part %d leaves the scratch or is not aligned\n", id); ++bad; break; }
    memset(buf.data() + p.off, id++, p.bytes);
  }
  id = 1;
  for (const Part& p : parts) {
    for (size_t i = 0; i < p.bytes && !bad; ++i) if (buf[p.off + i] != id) { fprintf(stderr, "part %d is overwritten at %zu\n", id, i); ++bad; }
    ++id;
  }
  for (size_t i = 0; i < CANARY; ++i) if (buf[L.total + i] != 0xC5) ++bad;
  printf("%zu %u\n", L.total, L.chain_grid);
  return bad ? 1 : 0;
}

static int cmd_refuse(char** a) {
  const char* why = egsh::refuse_verify(strtoull(a[0], nullptr, 10), strtoull(a[1], nullptr, 10), atoi(a[2]), atoi(a[3]), atoi(a[4]), atoi(a[5]),
                                        strtoull(a[6], nullptr, 10), atoi(a[7]), atoi(a[8]), atoi(a[9]), atoi(a[10]));
  printf("%s\n", why ? why : "ok");
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc == 3 && !strcmp(argv[1], "key")) rc = cmd_key(argv[2]);
  else if (argc == 3 && !strcmp(argv[1], "hash")) rc = cmd_hash(argv[2]);
  else if (argc == 3 && !strcmp(argv[1], "verify")) rc = cmd_verify(argv[2]);
  else if (argc == 7 && !strcmp(argv[1], "layout")) rc = cmd_layout(argv + 2);
  else if (argc == 13 && !strcmp(argv[1], "refuse")) rc = cmd_refuse(argv + 2);
  else fprintf(stderr, "usage: shufflecheck key|hash|verify FILE | layout N CUS TREE MSM_BIG MSM_SMALL | refuse ...\n");
  if (rc == 0) printf("PASS\n");
  return rc;
}
