// transcript_script.cuh -- TEST-ONLY: one interpreter of transcript scripts over merlin.cuh (unchanged), shared by the host build
// (tests/hostcheck/hostcheck.cpp: hc_transcript_script over ArrState, with the bound checks and UBSan) and the device build
// (tests/merlindev/merlindev.hip over the product's LDS storage strides).  The scripts come from tests/transcript_scripts.py, which
// documents the operations; what they must give comes from the oracle's transcript (oracle/transcript.c), never from this code.
//
// Binary form, little-endian 32-bit words: n_ops, then per operation (op, label, b, c) with label = byte offset into the blob << 12 |
// length, then the label bytes.  The blob is uniform over a launch; every case has its own message area of msg_bytes bytes (a
// multiple of 4) and its own out_words output words, written in script order.
#pragma once
#include <stddef.h>
#include "../../elastic_elgamal_amd/csrc/merlin.cuh"

namespace eg {

enum : u32 { TS_INIT = 1, TS_APPEND_BYTES, TS_APPEND_WORDS, TS_APPEND_U64, TS_CHALLENGE64, TS_SQUEEZE, TS_EXPORT_IMPORT, TS_CLONE, TS_POS,
             TS_OP_END };
constexpr u32 TS_MAX_SQUEEZE_BYTES = 1024, TS_MAX_SQUEEZE_WORDS = 64;

// Output words of one case, or -1 for a script that would read or write outside its buffers (checked on the host before any run).
inline long ts_out_words(const u32* blob, size_t blob_bytes, size_t msg_bytes) {
  if (!blob || blob_bytes < 4 || blob_bytes % 4 || msg_bytes % 4) return -1;
  const u32 n_ops = blob[0];
  if (n_ops == 0 || n_ops > (blob_bytes - 4) / 16) return -1;
  long out = 0;
  for (u32 k = 0; k < n_ops; ++k) {
    const u32 op = blob[1 + 4 * k], la = blob[2 + 4 * k], b = blob[3 + 4 * k], c = blob[4 + 4 * k];
    if (op < TS_INIT || op >= TS_OP_END) return -1;
    if ((k == 0) != (op == TS_INIT)) return -1;                       // exactly the first operation makes the transcript
    const size_t off = la >> 12, len = la & 0xfffu;
    if (len > 255 || off > blob_bytes || len > blob_bytes - off) return -1;
    switch (op) {
      case TS_APPEND_BYTES:
      case TS_APPEND_WORDS: {
        const size_t whole = ((size_t)c + 3) / 4 * 4;                    // the word form reads the word its tail bytes lie in
        if (b % 4 || b > msg_bytes || whole > msg_bytes - b) return -1;
        break;
      }
      case TS_APPEND_U64:
        if (b % 4 || b > msg_bytes || 8 > msg_bytes - b) return -1;
        break;
      case TS_CHALLENGE64: out += 16; break;
      case TS_SQUEEZE:
        if (b > TS_MAX_SQUEEZE_BYTES || c > TS_MAX_SQUEEZE_WORDS) return -1;
        out += (long)((b + 3) / 4 + c);
        break;
      case TS_POS: out += 1; break;
      default: break;
    }
  }
  return out;
}

template <class S>
EG_HD void ts_scrub(Transcript<S>& t) {        // a "fresh" transcript holds nothing the next import or clone could lean on
#pragma unroll 1
  for (int i = 0; i < 50; ++i) t.st.wr(i, 0xa5a5a5a5u ^ (u32)i);
  t.pos = 77; t.pos_begin = 99; t.cur_flags = 0xffu;
}

// Runs a checked script (ts_out_words >= 0) of one case.  a and b are two transcripts over separate storage; export/import and clone
// move the running transcript from one to the other.
template <class S>
EG_HD void ts_run(Transcript<S>& a, Transcript<S>& b, const u32* blob, const u32* msg, u32* out) {
  Transcript<S>* cur = &a;
  Transcript<S>* oth = &b;
  const char* bytes = reinterpret_cast<const char*>(blob);
  const u32 n_ops = blob[0];
  u32 o = 0;
#pragma unroll 1
  for (u32 k = 0; k < n_ops; ++k) {
    const u32 op = blob[1 + 4 * k], la = blob[2 + 4 * k], x = blob[3 + 4 * k], y = blob[4 + 4 * k];
    const char* label = bytes + (la >> 12);
    const int label_len = (int)(la & 0xfffu);
    switch (op) {
      case TS_INIT:
        merlin_init(*cur, label, label_len);
        break;
      case TS_APPEND_BYTES:
        merlin_append_bytes(*cur, label, label_len, reinterpret_cast<const char*>(msg) + x, (int)y);
        break;
      case TS_APPEND_WORDS:
        merlin_append_words(*cur, label, label_len, msg + (x >> 2), (int)y);
        break;
      case TS_APPEND_U64:
        merlin_append_u64(*cur, label, label_len, (u64)msg[x >> 2] | ((u64)msg[(x >> 2) + 1] << 32));
        break;
      case TS_CHALLENGE64: {
        u32 w[16];
        merlin_challenge64(*cur, label, label_len, w);
#pragma unroll 1
        for (int i = 0; i < 16; ++i) out[o++] = w[i];
        break;
      }
      case TS_SQUEEZE: {                       // challenge_bytes(label, x + 4 y): x bytes one at a time, then y words
        merlin_frame(*cur, label, label_len, x + 4u * y);
        strobe_begin_op(*cur, EG_FLAG_PRF);
        u32 acc = 0;
#pragma unroll 1
        for (u32 i = 0; i < x; ++i) {
          acc |= strobe_squeeze_byte(*cur) << (8u * (i & 3u));
          if ((i & 3u) == 3u) { out[o++] = acc; acc = 0; }
        }
        if (x & 3u) out[o++] = acc;
#pragma unroll 1
        for (u32 i = 0; i < y; ++i) out[o++] = strobe_squeeze_word(*cur);
        break;
      }
      case TS_EXPORT_IMPORT: {
        u32 w[52];
        merlin_export(*cur, w);
        ts_scrub(*oth);
        merlin_import(*oth, w);
        ts_scrub(*cur);
        Transcript<S>* t = cur; cur = oth; oth = t;
        break;
      }
      case TS_CLONE: {
        ts_scrub(*oth);
        merlin_clone(*oth, *cur);
        ts_scrub(*cur);
        Transcript<S>* t = cur; cur = oth; oth = t;
        break;
      }
      case TS_POS:
        out[o++] = cur->pos | (cur->pos_begin << 8);
        break;
      default:
        break;
    }
  }
}

}  // namespace eg
