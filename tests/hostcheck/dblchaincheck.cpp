// dblchaincheck.cpp -- TEST-ONLY stand-alone program (tests/test_dbl_chain_cpu.py builds it with -DEG_BOUNDCHECK and
// -fsanitize=address,undefined and runs it): the fused square-and-subtract (fe_sq2_sub), the chain doubling (ge_dbl_chain,
// ge_dbl_chain_sgn), the comb product with the sign on the accumulator (ge_teeth_mul) and the fixed comb with the wave-uniform
// zero-digit path (ge_fixed_mul_add), each against the form it replaces, on the host compilation of the device headers.
//   dblchaincheck records OP IN OUT      n records of 80 words + 8 float classes -> n x 80 words (tests/dblchaindev/chain_ops.cuh)
//   dblchaincheck comb SCALARS OUT       32-byte scalars -> for both shapes: enc(P), then enc([k]P) per scalar; exit 1 on a difference
//   dblchaincheck fixed SCALARS OUT      32-byte scalars -> enc([k]G) per scalar; exit 1 on a difference
//   dblchaincheck counts                 fe_sq / fe_mul per doubling and per 5 x 51 comb product
//   dblchaincheck outside CLASS_F        fe_sq2_sub with f at the top of CLASS_F: prints "ran" unless the bound check aborts first
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <vector>
#include "../dblchaindev/chain_ops.cuh"

using namespace eg;

struct ArrTable {
  ge_cached e[8];
  void store(int i, const ge_cached& c) { e[i] = c; }
  void load(ge_cached& c, int i) const { c = e[i]; }
};
// the comb table of a base, stored the way the device stores it (device_io.cuh BaseTable): packed, 4 x 256 bits per entry
struct ArrBase {
  u32 w[64][32];
  void store(int i, const ge_cached& c) {
    fe a = c.YpX, b = c.YmX, z = c.Z2;
    fe_carry(a); fe_carry(b); fe_carry(z);
    fe_pack8(w[i], a); fe_pack8(w[i] + 8, b); fe_pack8(w[i] + 16, z); fe_pack8(w[i] + 24, c.T2d);
  }
  void load(ge_cached& c, int i) const {
    fe_unpack8(c.YpX, w[i]); fe_unpack8(c.YmX, w[i] + 8); fe_unpack8(c.Z2, w[i] + 16); fe_unpack8(c.T2d, w[i] + 24);
  }
};
// fixed-base comb table of the generator with entries computed on demand
struct ArrNiels {
  int bits = EG_COMB_BITS;
  mutable std::map<int, ge_niels> cache;
  void load(ge_niels& c, int idx) const {
    auto it = cache.find(idx);
    if (it == cache.end()) {
      const int w = idx / comb_entries(bits), k = idx % comb_entries(bits) + 1;    // entry = [k * 2^(B w)] G
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

// ---- the forms that the product's code replaces ---------------------------------------------------------------------------------
// ge_teeth_mul with the column's sign on the ENTRY (ge_cached_cneg) and the unfused doubling (ge_dbl)
template <int T, class TableIO>
static void ref_teeth_mul_entryneg(ge& acc, TableIO& io, u64 rows[T]) {
  {
    int idx; bool neg;
    sc_teeth_next<T>(rows, idx, neg);
    ge_cached cur;
    io.load(cur, idx);
    fe t = cur.YpX; fe_cmov(cur.YpX, cur.YmX, neg); fe_cmov(cur.YmX, t, neg);
    fe_sub4(acc.X, cur.YpX, cur.YmX); fe_carry(acc.X);
    fe_add(acc.Y, cur.YpX, cur.YmX); fe_carry(acc.Y);
    acc.Z = cur.Z2;
  }
  for (int c = Teeth<T>::COLS - 2; c >= 0; --c) {
    int idx; bool neg;
    sc_teeth_next<T>(rows, idx, neg);
    ge_cached cur;
    io.load(cur, idx);
    ge_p1p1 t;
    ge_dbl(t, acc.X, acc.Y, acc.Z);
    ge_dbl_to_p3(acc, t);
    ge_cached_cneg(cur, neg);
    ge_add(t, acc, cur);
    ge_add_to_p3(acc, t);
  }
}
// ge_fixed_mul_add with the identity selected over all 27 limbs in every window, whatever the digit
template <class NielsIO>
static void ref_fixed_mul_add_select(ge& acc, NielsIO& io, const u32 k[EG_COMB_WORDS], int& zero_digits) {
  ge_niels ident; ge_niels_identity(ident);
  const int bits = io.bits, windows = comb_windows(bits);
  u32 carry = 0;
  for (int i = 0; i < windows; ++i) {
    const int d = sc_comb_digit(k, i, carry, bits);
    ge_niels c; io.load(c, ge_fixed_index(i, d, bits));
    zero_digits |= (d == 0) << i;
    fe_cmov(c.ypx, ident.ypx, d == 0); fe_cmov(c.ymx, ident.ymx, d == 0); fe_cmov(c.xy2d, ident.xy2d, d == 0);
    ge_niels_cneg(c, d < 0);
    ge_p1p1 t; ge_madd(t, acc, c);
    ge_add_to_p3(acc, t);
  }
}

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  uint8_t buf[4096]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
static void write_file(const char* path, const std::vector<uint8_t>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v.data(), 1, v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}
static void scalar_words(u32 w[8], const uint8_t* b) {
  for (int i = 0; i < 8; ++i) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
}
static void push_encoding(std::vector<uint8_t>& out, const ge& p, u32 enc[8]) {
  ristretto_encode(enc, p);
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) out.push_back((uint8_t)(enc[i] >> (8 * j)));
}

static int run_records(int op, const char* in_path, const char* out_path) {
  const std::vector<uint8_t> in = read_file(in_path);
  const size_t rec = 4 * (CHAIN_WORDS + CHAIN_SLOTS);
  if (op < 0 || op >= COP_COUNT || in.size() % rec != 0) { fprintf(stderr, "bad records\n"); return 2; }
  const size_t n = in.size() / rec;
  std::vector<uint8_t> out(n * 4 * CHAIN_WORDS);
  for (size_t r = 0; r < n; ++r) {
    u32 w[CHAIN_WORDS], o[CHAIN_WORDS]; float cls[CHAIN_SLOTS];
    memcpy(w, &in[r * rec], sizeof w); memcpy(cls, &in[r * rec + sizeof w], sizeof cls);
    memset(o, 0, sizeof o);
    chain_op(op, w, cls, o);
    {                                   // the promised class-1 results hold their limbs (fe_check_values aborts otherwise)
      const float one[CHAIN_SLOTS] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
      fe h;
      if (op == COP_SQ2_SUB) for (int s = 0; s < 3; ++s) co_load(h, o, one, s);
      else { co_load(h, o, one, 3); co_load(h, o, one, 7); }
    }
    memcpy(&out[r * 4 * CHAIN_WORDS], o, sizeof o);
  }
  write_file(out_path, out);
  printf("records %zu\n", n);
  return 0;
}

// P = [2^40 + 12345] G made with the full-width helpers (which the pull request's code does not touch)
static void comb_base(ge& p) {
  ge g; ge_generator(g);
  ge q; ge_identity(q);
  const u64 k = (1ull << 40) + 12345ull;
  for (int bit = 40; bit >= 0; --bit) {
    ge d; ge_dbl_full(d, q); q = d;
    if ((k >> bit) & 1) { ge t; ge_add_full(t, q, g); q = t; }
  }
  p = q;
}

template <int T>
static int run_comb_t(const std::vector<uint8_t>& sc, std::vector<uint8_t>& out) {
  ge p; comb_base(p);
  static ArrBase tab; ArrTable tmp;
  ge_teeth_tables_build<T>(tab, tmp, p);
  u32 enc[8], ref[8];
  push_encoding(out, p, enc);
  int bad = 0;
  for (size_t i = 0; i < sc.size() / 32; ++i) {
    u32 kw[8]; scalar_words(kw, &sc[32 * i]);
    u64 rows[T], rows2[T];
    sc_recode_teeth<T>(rows, kw); sc_recode_teeth<T>(rows2, kw);
    ge a, b;
    ge_teeth_mul<T>(a, tab, rows);
    ref_teeth_mul_entryneg<T>(b, tab, rows2);
    ristretto_encode(ref, b);
    push_encoding(out, a, enc);
    if (memcmp(enc, ref, sizeof enc) != 0) { fprintf(stderr, "comb %d teeth: scalar %zu differs from the entry-negating form\n", T, i); bad = 1; }
  }
  return bad;
}

static int run_fixed(const std::vector<uint8_t>& sc, std::vector<uint8_t>& out, int& zero_windows) {
  static ArrNiels tab;
  int bad = 0;
  u32 enc[8], ref[8];
  for (size_t i = 0; i < sc.size() / 32; ++i) {
    u32 kw[8], dg[EG_COMB_WORDS]; scalar_words(kw, &sc[32 * i]);
    sc_recode_comb(dg, kw);
    ge a, b; ge_identity(a); ge_identity(b);
    ge_fixed_mul_add(a, tab, dg);
    ref_fixed_mul_add_select(b, tab, dg, zero_windows);
    ristretto_encode(ref, b);
    push_encoding(out, a, enc);
    if (memcmp(enc, ref, sizeof enc) != 0) { fprintf(stderr, "fixed comb: scalar %zu differs from the always-select form\n", i); bad = 1; }
  }
  return bad;
}

static int run_counts() {
  ge p; comb_base(p);
  ge_p1p1 t; ge_p2 q;
  unsigned long long m0 = g_fe_mul_count, s0 = g_fe_sq_count;
  ge_dbl_chain(t, p.X, p.Y, p.Z); ge_dbl_to_p2(q, t);
  printf("dbl_chain sq %llu mul %llu\n", g_fe_sq_count - s0, g_fe_mul_count - m0);
  m0 = g_fe_mul_count; s0 = g_fe_sq_count;
  ge_dbl_chain_sgn(t, p.X, p.Y, p.Z, true); ge_dbl_to_p2(q, t);
  printf("dbl_chain_sgn sq %llu mul %llu\n", g_fe_sq_count - s0, g_fe_mul_count - m0);
  m0 = g_fe_mul_count; s0 = g_fe_sq_count;
  ge_dbl(t, p.X, p.Y, p.Z); ge_dbl_to_p2(q, t);
  printf("dbl sq %llu mul %llu\n", g_fe_sq_count - s0, g_fe_mul_count - m0);
  static ArrBase tab; ArrTable tmp;
  ge_teeth_tables_build<5>(tab, tmp, p);
  u32 kw[8] = {0x9abcdef1u, 0x12345678u, 0x0fedcba9u, 0x87654321u, 0x13579bdfu, 0x2468ace0u, 0x0badcafeu, 0x01234567u};
  u64 rows[5]; sc_recode_teeth<5>(rows, kw);
  ge acc;
  m0 = g_fe_mul_count; s0 = g_fe_sq_count;
  ge_teeth_mul<5>(acc, tab, rows);
  printf("comb5 sq %llu mul %llu\n", g_fe_sq_count - s0, g_fe_mul_count - m0);
  return 0;
}

static int run_outside(float cf) {
  fe f, g, h;
  for (int i = 0; i < EG_NL; ++i) { f.v[i] = (u32)(cf * (float)(1u << fe_w(i))); g.v[i] = (u32)(3.9f * (float)(1u << fe_w(i))); }
  EG_SETCLS(f, cf); EG_SETCLS(g, 3.9f);
  fe_sq2_sub(h, f, g);
  u32 w[8]; fe_to_words(w, h);
  printf("ran %08x\n", w[0]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "records")) return run_records(atoi(argv[2]), argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "comb")) {
    const std::vector<uint8_t> sc = read_file(argv[2]);
    std::vector<uint8_t> out;
    const int bad = run_comb_t<5>(sc, out) | run_comb_t<6>(sc, out);
    write_file(argv[3], out);
    printf("comb %zu scalars x 2 shapes\n", sc.size() / 32);
    return bad;
  }
  if (argc == 4 && !strcmp(argv[1], "fixed")) {
    const std::vector<uint8_t> sc = read_file(argv[2]);
    std::vector<uint8_t> out;
    int zero_windows = 0;
    const int bad = run_fixed(sc, out, zero_windows);
    write_file(argv[3], out);
    printf("fixed %zu scalars, zero digits seen in windows %#x of %d\n", sc.size() / 32, zero_windows, comb_windows(EG_COMB_BITS));
    return bad;
  }
  if (argc == 2 && !strcmp(argv[1], "counts")) return run_counts();
  if (argc == 3 && !strcmp(argv[1], "outside")) return run_outside((float)atof(argv[2]));
  fprintf(stderr, "usage: dblchaincheck records OP IN OUT | comb SCALARS OUT | fixed SCALARS OUT | counts | outside CLASS_F\n");
  return 2;
}
