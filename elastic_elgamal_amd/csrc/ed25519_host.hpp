// ed25519_host.hpp -- argument rules and scratch layout of the Ed25519 entries (eg_ed25519_*, eg_sha512_*; eg_hip.hip; kernels:
// ed25519_kernels.cuh): pure host code, no HIP.  tests/hostcheck/ed25519check.cpp compiles it under ASan + UBSan beside the lane functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace eged {

constexpr uint64_t N_LIMIT = 1ull << 31;          // n must stay below
constexpr size_t PREFIX_MAX = 255;
constexpr size_t PREFIX_BYTES = 256;              // its room at the start of the scratch
constexpr size_t H_BYTES = 32;                    // the parked h of one item
constexpr size_t TABLE_BYTES = 8 * 9 * 16;        // a lane's radix-16 table of -A: WS_QUADS uint4 (device_io.cuh)
constexpr unsigned NT = 256;                      // lanes per block
constexpr unsigned BLOCKS_PER_CU = 4;             // grid of the curve kernel: at most this many blocks per CU, each lane striding over its items

// what is wrong with the message arguments that every entry shares (nullptr = fine)
inline const char* refuse_messages(uint64_t n, bool have_msgs, uint64_t msg_stride, uint64_t msg_len, bool have_prefix, uint64_t prefix_len) {
  if (n >= N_LIMIT) return "n is 2^31 or more";
  if (prefix_len > PREFIX_MAX) return "prefix_len is above 255";
  if (prefix_len && !have_prefix) return "null prefix with prefix_len > 0";
  if (msg_stride < msg_len) return "msg_stride is below msg_len";
  if (n && msg_len && !have_msgs) return "null msgs";
  return nullptr;
}
// the roster rules of a verification
inline const char* refuse_roster(uint64_t n, uint64_t n_keys, bool have_index) {
  if (n && n_keys == 0) return "n_keys is 0";
  if (!have_index && n_keys != n) return "no key_index: n_keys must equal n";
  return nullptr;
}

inline unsigned grid_blocks(size_t n, unsigned cus) {
  const size_t want = (n + NT - 1) / NT, cap = (size_t)(cus ? cus : 1) * BLOCKS_PER_CU;
  return (unsigned)(want < cap ? want : cap);
}

// the caller's scratch of a verification, in bytes from its start (every part 256-byte aligned); n == 0 needs none
struct Layout {
  unsigned blocks;             // grid of the curve kernel
  size_t prefix, h, tables, total;
};
inline Layout layout(size_t n, unsigned cus) {
  Layout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  L.blocks = grid_blocks(n, cus);
  L.prefix = take(n ? PREFIX_BYTES : 0);
  L.h = take(n * H_BYTES);
  L.tables = take((size_t)L.blocks * NT * TABLE_BYTES);
  L.total = off;
  return L;
}

}  // namespace eged
