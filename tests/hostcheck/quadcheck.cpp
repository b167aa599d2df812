// quadcheck.cpp -- TEST-ONLY host build of the quad-lane point arithmetic (csrc/ge25519_quad.cuh) with -DEG_BOUNDCHECK under UBSan.
// A quad is emulated as an array of four lanes (QuadHost); the operations are the ones the device compiles, so every executed path
// asserts the limb-class preconditions of fe25519.cuh.  tests/test_quad_arith_cpu.py compares every quad operation with the one-lane
// operation of ge25519.cuh and with Python integers, and whole products with the oracle.  The product never loads this library.
#include <string.h>
#include <map>
#include "../quaddev/quad_ops.cuh"
#include "../../elastic_elgamal_amd/csrc/sc25519.cuh"

using namespace eg;
typedef QuadHost::var<fe> qv;

static void words_from_bytes(u32* w, const uint8_t* b, int nwords) {
  for (int i = 0; i < nwords; ++i) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
}
static void bytes_from_words(uint8_t* b, const u32* w, int nwords) {
  for (int i = 0; i < nwords; ++i) for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}
static fe fe_raw(const u32* limbs, float cls) {
  fe f;
  for (int i = 0; i < EG_NL; ++i) f.v[i] = limbs[i];
  f.cls = cls;
  return f;
}
static void put(u32* out, const fe& f) { for (int i = 0; i < EG_NL; ++i) out[i] = f.v[i]; }

// the comb table of a base as the device stores it (BaseTable: packed, Y+X | Y-X | 2Z | 2dT), written and read by quads
struct QuadArrBase {
  u32 w[64][32];
  static int element(int r) { return r < 2 ? r : (r == 2 ? 3 : 2); }
  void store(QuadHost&, int e, const qv& d) { for (int r = 0; r < 4; ++r) fe_pack8(w[e] + 8 * element(r), d.v[r]); }
  void load(QuadHost&, qv& d, int e, bool neg) const {
    for (int r = 0; r < 4; ++r) fe_unpack8(d.v[r], w[e] + 8 * (r < 2 ? (r ^ (neg ? 1 : 0)) : element(r)));
  }
  // the same table read by ONE lane (device_io.cuh: BaseTable::load)
  void load(ge_cached& c, int e) const {
    fe_unpack8(c.YpX, w[e]); fe_unpack8(c.YmX, w[e] + 8); fe_unpack8(c.Z2, w[e] + 16); fe_unpack8(c.T2d, w[e] + 24);
  }
};
// fixed-base comb table with entries computed on demand, delivered to a quad as the device delivers them (QuadFixedTable)
struct QuadArrNiels {
  ge base;
  int bits = EG_COMB_BITS;
  mutable std::map<int, ge_niels> cache;
  void load(QuadHost&, qv& d, int idx, bool neg) const {
    auto it = cache.find(idx);
    if (it == cache.end()) {
      const int w = idx / comb_entries(bits), k = idx % comb_entries(bits) + 1;
      ge p = base;
      for (int i = 0; i < bits * w; ++i) { ge t; ge_dbl_full(t, p); p = t; }
      ge q; ge_identity(q);
      for (int bit = bits - 1; bit >= 0; --bit) {
        ge t; ge_dbl_full(t, q); q = t;
        if ((k >> bit) & 1) { ge s; ge_add_full(s, q, p); q = s; }
      }
      ge_niels n; ge_to_niels(n, q);
      it = cache.emplace(idx, n).first;
    }
    const ge_niels& n = it->second;
    d.v[0] = neg ? n.ymx : n.ypx;
    d.v[1] = neg ? n.ypx : n.ymx;
    d.v[2] = n.xy2d;
    fe_0(d.v[3]); d.v[3].v[0] = 2;
  }
};

extern "C" {

// One quad operation and its one-lane counterpart on RAW limbs.  a: four field elements (a point X Y Z T, or an addend in the one-lane
// order Y+X, Y-X, 2Z, 2dT) with classes ca; b: the addend of an addition, classes cb.  out_quad / out_lane: four field elements each,
// in the one-lane order.  Operations: 0 doubling, 1 addition of a cached point, 2 addition of a Niels point (b[2] ignored: 2Z = 2),
// 3 point -> addend, 4 negated addend, 5 negated point, 6 addend -> projective point (X Y Z; T is not produced), 7 select the identity,
// 8 doubling by the quad alone (classes that ge_dbl does not admit), 9 addend -> point with T, 10 addend with 2dT negated only (after a
// table load that has already swapped Y+X and Y-X), 11 select the neutral addend, 12 one-lane addend -> quad.
int qc_op(int op, const u32 a[4][EG_NL], const float ca[4], const u32 b[4][EG_NL], const float cb[4], u32 out_quad[4][EG_NL], u32 out_lane[4][EG_NL]) {
  if (op < 0 || op >= QOP_COUNT) return 0;
  QuadHost q;
  fe A[4], B[4];
  for (int i = 0; i < 4; ++i) { A[i] = fe_raw(a[i], ca[i]); B[i] = fe_raw(b[i], cb[i]); }
  // the quad: the case code the device build runs (tests/quaddev/quad_ops.cuh)
  {
    qv a_pt, a_cd, b_cd, res;
    for (int r = 0; r < 4; ++r) { a_pt.v[r] = A[r]; a_cd.v[r] = A[quad_cached_order(r)]; b_cd.v[r] = B[quad_cached_order(r)]; }
    if (op != QOP_CACHED_CNEG && op != QOP_CACHED_TO_P2 && op != QOP_CACHED_TO_P3 && op != QOP_CACHED_NEG_T && op != QOP_CACHED_IDENTITY) a_cd = a_pt;      // unused there; keeps its classes out of the way
    bool cached;
    quad_case(q, op, a_pt, a_cd, b_cd, res, cached);
    for (int r = 0; r < 4; ++r) put(out_quad[cached ? quad_cached_order(r) : r], res.v[r]);
  }
  // one lane: the operation of ge25519.cuh
  fe r4[4];
  ge p0{A[0], A[1], A[2], A[3]}, p;
  ge_cached c0{A[0], A[1], A[2], A[3]};
  ge_p1p1 t;
  switch (op) {
    case QOP_DBL:
      ge_dbl(t, A[0], A[1], A[2]);
      ge_dbl_to_p3(p, t);
      r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T;
      break;
    case QOP_DBL_WIDE:        // the quad admits wider classes than ge_dbl (which squares X + Y): no one-lane counterpart
      for (int r = 0; r < 4; ++r) r4[r] = fe_raw(out_quad[r], 1.0f);
      break;
    case QOP_ADD: { ge_cached cc{B[0], B[1], B[2], B[3]}; ge_add(t, p0, cc); ge_add_to_p3(p, t); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break; }
    case QOP_MADD: { ge_niels nn{B[0], B[1], B[3]}; ge_madd(t, p0, nn); ge_add_to_p3(p, t); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break; }
    case QOP_TO_CACHED: { ge_cached cc; ge_to_cached_lazy(cc, p0); r4[0] = cc.YpX; r4[1] = cc.YmX; r4[2] = cc.Z2; r4[3] = cc.T2d; break; }
    case QOP_CACHED_CNEG: ge_cached_cneg(c0, true); r4[0] = c0.YpX; r4[1] = c0.YmX; r4[2] = c0.Z2; r4[3] = c0.T2d; break;
    case QOP_NEG: ge_neg(p, p0); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break;
    case QOP_CACHED_TO_P2: ge_cached_to_p3(p, c0); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break;
    case QOP_CACHED_TO_P3: ge_cached_to_p3(p, c0); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break;
    case QOP_CACHED_NEG_T: ge_cached_cneg(c0, true); r4[0] = c0.YmX; r4[1] = c0.YpX; r4[2] = c0.Z2; r4[3] = c0.T2d; break;     // swapped back
    case QOP_CACHED_IDENTITY: ge_cached_identity(c0); r4[0] = c0.YpX; r4[1] = c0.YmX; r4[2] = c0.Z2; r4[3] = c0.T2d; break;
    case QOP_FROM_CACHED: r4[0] = c0.YpX; r4[1] = c0.YmX; r4[2] = c0.Z2; r4[3] = c0.T2d; break;
    default: ge_identity(p); r4[0] = p.X; r4[1] = p.Y; r4[2] = p.Z; r4[3] = p.T; break;
  }
  for (int r = 0; r < 4; ++r) put(out_lane[r], r4[r]);
  return 1;
}
}  // extern "C"

// out = enc([k]P + [r]G): the comb table of P built by a quad, the product and the fixed-base comb over G evaluated by a quad; with
// lane_reads != 0 the product is evaluated by ONE lane (ge_teeth_mul) over the table the quad built: the layouts agree.
template <int T>
static int teeth_product(const uint8_t k[32], const uint8_t p_enc[32], const uint8_t r[32], int lane_reads, uint8_t out[32]) {
  static QuadArrNiels g_tab;
  static bool ready = false;
  if (!ready) { ge_generator(g_tab.base); ready = true; }
  u32 kw[8], rw[8], pw[8], o[8];
  words_from_bytes(kw, k, 8); words_from_bytes(rw, r, 8); words_from_bytes(pw, p_enc, 8);
  ge p;
  if (!ristretto_decode(p, pw)) return 0;
  QuadHost q;
  qv c;
  quad_from_ge(q, c, p);
  static QuadArrBase tab;
  quad_teeth_tables_build<T>(q, tab, c);
  u64 rows[T];
  sc_recode_teeth<T>(rows, kw);
  qv acc;
  if (lane_reads) {
    ge a; ge_teeth_mul<T>(a, tab, rows);
    quad_from_ge(q, acc, a);
  } else {
    quad_teeth_mul<T>(q, acc, tab, rows);
  }
  u32 dr[EG_COMB_WORDS];
  sc_recode_comb(dr, rw);
  quad_fixed_mul_add(q, acc, g_tab, dr);
  ge res{acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
  ristretto_encode(o, res);
  bytes_from_words(out, o, 8);
  return 1;
}

extern "C" int qc_double_mul_generator(int teeth, const uint8_t k[32], const uint8_t p_enc[32], const uint8_t r[32], int lane_reads, uint8_t out[32]) {
  if (teeth == 5) return teeth_product<5>(k, p_enc, r, lane_reads, out);
  if (teeth == 7) return teeth_product<7>(k, p_enc, r, lane_reads, out);
  return teeth_product<6>(k, p_enc, r, lane_reads, out);
}
// out = enc([r]G) from the identity: the fixed-base comb alone (an equation without a variable base)
extern "C" int qc_mul_generator(const uint8_t r[32], uint8_t out[32]) {
  static QuadArrNiels g_tab;
  static bool ready = false;
  if (!ready) { ge_generator(g_tab.base); ready = true; }
  u32 rw[8], o[8], dr[EG_COMB_WORDS];
  words_from_bytes(rw, r, 8);
  QuadHost q;
  qv acc;
  quad_identity(q, acc);
  sc_recode_comb(dr, rw);
  quad_fixed_mul_add(q, acc, g_tab, dr);
  ge res{acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
  ristretto_encode(o, res);
  bytes_from_words(out, o, 8);
  return 1;
}

// out = enc([k](P_1 + .. + P_m) + [r]G) through the comb table of the SUM, made by a quad from the members' tables without a doubling
// (quad_teeth_tables_sum); m <= 8.  Also the one-lane reader over the quad's table when lane_reads != 0.
template <int T>
static int sum_product(const uint8_t k[32], const uint8_t* p_encs, int m, const uint8_t r[32], int lane_reads, uint8_t out[32]) {
  static QuadArrNiels g_tab;
  static bool ready = false;
  if (!ready) { ge_generator(g_tab.base); ready = true; }
  if (m < 1 || m > 8) return 0;
  static QuadArrBase member[8], tab;
  QuadHost q;
  for (int i = 0; i < m; ++i) {
    u32 pw[8]; words_from_bytes(pw, p_encs + 32 * i, 8);
    ge p;
    if (!ristretto_decode(p, pw)) return 0;
    qv c; quad_from_ge(q, c, p);
    quad_teeth_tables_build<T>(q, member[i], c);
  }
  quad_teeth_tables_sum<T>(q, tab, m, [&](int t, int g, qv& e) { member[t].load(q, e, g, false); });
  u32 kw[8], rw[8], o[8], dr[EG_COMB_WORDS];
  words_from_bytes(kw, k, 8); words_from_bytes(rw, r, 8);
  u64 rows[T];
  sc_recode_teeth<T>(rows, kw);
  qv acc;
  if (lane_reads) { ge a; ge_teeth_mul<T>(a, tab, rows); quad_from_ge(q, acc, a); }
  else quad_teeth_mul<T>(q, acc, tab, rows);
  sc_recode_comb(dr, rw);
  quad_fixed_mul_add(q, acc, g_tab, dr);
  ge res{acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
  ristretto_encode(o, res);
  bytes_from_words(out, o, 8);
  return 1;
}
extern "C" int qc_sum_mul_generator(int teeth, const uint8_t k[32], const uint8_t* p_encs, int m, const uint8_t r[32], int lane_reads, uint8_t out[32]) {
  if (teeth == 5) return sum_product<5>(k, p_encs, m, r, lane_reads, out);
  if (teeth == 7) return sum_product<7>(k, p_encs, m, r, lane_reads, out);
  return sum_product<6>(k, p_encs, m, r, lane_reads, out);
}
