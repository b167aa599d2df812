// sha512.cuh -- SHA-512 (FIPS 180-4) over byte ranges, one message per lane.  Host and device: the host check build
// (tests/hostcheck/ed25519check.cpp) runs the same code on arrays.
//
// The message of a lane is the concatenation of up to four byte ranges of any length and alignment (Ed25519 hashes R || A || prefix || msg;
// the prefix length shifts the alignment of everything behind it), so the input is read byte by byte and assembled into the sixteen
// big-endian 64-bit words of a block in registers: no staging buffer, no indexed local array.  The 80 rounds run as five rolled groups of
// sixteen with a 16-word rolling schedule, so every index into the schedule is a compile-time constant and the round constant is a uniform
// load.  gfx950 has no 64-bit rotate: a word is a (hi, lo) pair and every rotation is two 32-bit funnel shifts (v_alignbit_b32, eg_funnel
// of fe25519.cuh), a rotation by 32 or more the same with the halves swapped.
#pragma once
#include "fe25519.cuh"

namespace eg {

template <int N>
EG_HD u64 sha_rotr(u64 x) {
  static_assert(N > 0 && N < 64 && N != 32, "rotation amounts of SHA-512");
  const u32 a = (u32)x, b = (u32)(x >> 32);
  const u32 lo = N < 32 ? a : b, hi = N < 32 ? b : a;          // N >= 32: the halves change places first
  constexpr int S = N & 31;
  return ((u64)eg_funnel(lo, hi, S) << 32) | (u64)eg_funnel(hi, lo, S);
}
EG_HD u64 sha_Sigma0(u64 x) { return sha_rotr<28>(x) ^ sha_rotr<34>(x) ^ sha_rotr<39>(x); }
EG_HD u64 sha_Sigma1(u64 x) { return sha_rotr<14>(x) ^ sha_rotr<18>(x) ^ sha_rotr<41>(x); }
EG_HD u64 sha_sigma0(u64 x) { return sha_rotr<1>(x) ^ sha_rotr<8>(x) ^ (x >> 7); }
EG_HD u64 sha_sigma1(u64 x) { return sha_rotr<19>(x) ^ sha_rotr<61>(x) ^ (x >> 6); }

struct Sha512 { u64 h[8]; };

EG_HD void sha512_init(Sha512& s) {
  s.h[0] = 0x6a09e667f3bcc908ull; s.h[1] = 0xbb67ae8584caa73bull; s.h[2] = 0x3c6ef372fe94f82bull; s.h[3] = 0xa54ff53a5f1d36f1ull;
  s.h[4] = 0x510e527fade682d1ull; s.h[5] = 0x9b05688c2b3e6c1full; s.h[6] = 0x1f83d9abfb41bd6bull; s.h[7] = 0x5be0cd19137e2179ull;
}

// one block: w = its sixteen big-endian words (destroyed: the rolling schedule)
EG_HD void sha512_compress(Sha512& s, u64 w[16]) {
  constexpr u64 K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull,
  };
  u64 a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll 1
  for (int r = 0; r < 80; r += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (r) w[i] += sha_sigma1(w[(i + 14) & 15]) + w[(i + 9) & 15] + sha_sigma0(w[(i + 1) & 15]);
      const u64 t1 = h + sha_Sigma1(e) + ((e & f) ^ (~e & g)) + K[r + i] + w[i];
      const u64 t2 = sha_Sigma0(a) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
  }
  s.h[0] += a; s.h[1] += b; s.h[2] += c; s.h[3] += d; s.h[4] += e; s.h[5] += f; s.h[6] += g; s.h[7] += h;
}

// up to four byte ranges, read as one message; a range of length 0 may have a null pointer
struct ShaRanges {
  const unsigned char* p[4];
  size_t len[4];
};
EG_HD ShaRanges sha_ranges(const unsigned char* p0, size_t l0, const unsigned char* p1 = nullptr, size_t l1 = 0,
                           const unsigned char* p2 = nullptr, size_t l2 = 0, const unsigned char* p3 = nullptr, size_t l3 = 0) {
  ShaRanges r;
  r.p[0] = p0; r.len[0] = l0; r.p[1] = p1; r.len[1] = l1; r.p[2] = p2; r.len[2] = l2; r.p[3] = p3; r.len[3] = l3;
  return r;
}
// reads the ranges front to back; past their end: the padding's 0x80, then zeros
struct ShaReader {
  const unsigned char *cur, *end;
  int next;            // the range after the current one
  bool padded;
  EG_HD void open(const ShaRanges& r) { cur = r.p[0]; end = cur + r.len[0]; next = 1; padded = false; }
  EG_HD void advance(const ShaRanges& r) {
    while (cur == end && next < 4) {
      // a select chain, not an index: the ranges stay in registers
      const unsigned char* p = next == 1 ? r.p[1] : next == 2 ? r.p[2] : r.p[3];
      const size_t l = next == 1 ? r.len[1] : next == 2 ? r.len[2] : r.len[3];
      cur = p; end = p + l; ++next;
    }
  }
  EG_HD u64 word(const ShaRanges& r) {
    u64 v = 0;
    if ((size_t)(end - cur) >= 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v = (v << 8) | cur[k];
      cur += 8;
      return v;
    }
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      advance(r);
      u32 byte = 0;
      if (cur != end) byte = *cur++;
      else if (!padded) { byte = 0x80u; padded = true; }
      v = (v << 8) | byte;
    }
    return v;
  }
};

// SHA-512 of the concatenated ranges: out = the 64 digest bytes as sixteen little-endian 32-bit words (what sc_from_wide takes)
EG_HD void sha512_ranges(u32 out[16], const ShaRanges& r) {
  const size_t total = r.len[0] + r.len[1] + r.len[2] + r.len[3];
  const size_t blocks = (total + 17 + 127) / 128;              // the 0x80 byte and the 128-bit length always fit the last block
  Sha512 s; sha512_init(s);
  ShaReader rd; rd.open(r);
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = rd.word(r);
    if (b + 1 == blocks) w[15] = (u64)total << 3;              // w[14] = 0: messages are far below 2^61 bytes
    sha512_compress(s, w);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 hi = (u32)(s.h[i] >> 32), lo = (u32)s.h[i];
    out[2 * i] = __builtin_bswap32(hi);
    out[2 * i + 1] = __builtin_bswap32(lo);
  }
}

}  // namespace eg
