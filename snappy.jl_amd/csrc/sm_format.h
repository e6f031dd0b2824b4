// sm_format.h -- the snappy raw format's constants and rules as plain C++ (no HIP header): what
// the kernels (through sm_device.h), the host rules (sm_host_rules.h) and the host checker share.
// Format rules follow the reference's src/internal.jl:15-85 and src/varint.jl; nothing here is
// transcribed from the reference's tables (CHAR_TABLE is derived from the tag rules in
// char_entry()).
#pragma once
#include <stdint.h>

#include "common/smc_layout.h"

namespace sm {

constexpr uint32_t kBlockSize = 65536;        // internal.jl:31
constexpr uint32_t kInputMarginBytes = 15;    // internal.jl:32
constexpr uint32_t kMaxHashTableSize = 16384; // internal.jl:33
constexpr uint32_t kHashMul = 0x1e35a7bdu;    // internal.jl:94
constexpr int kWave = 64;

// status codes (mirror include/snappy_mi355x.h)
enum : int32_t {
  kOk = 0,
  kInvalidInput = 1,
  kBufferTooSmall = 2,
  kErrInputTooLarge = 16,
  kErrInvalid = 17,
  kErrVarint = smc::kErrVarint,
  kErrCopyOffset = 19,
  kErrCopyLength = 20,
  kErrLiteral = 21,
  kErrDevice = 32,  // SM_ERR_DEVICE: a block length that is a compressor error mark (>= kOutLenError)
  kErrCross = 64,  // internal: a fragment's copy reads another fragment (never returned by the ABI)
};

SMC_HD inline uint32_t max_compressed_length(uint32_t n) { return 32 + n + n / 6; }

// SM_OUT_LEN_ERROR: a compressor's error mark in d_out_len (include/snappy_mi355x.h).  A device
// decoder handed such a length (a caller passing comp_len straight on) reports kErrDevice without
// reading the slot: the mark is an error, never a stream length (Snappy.jl:50 raises, never decodes).
constexpr uint32_t kOutLenError = 0xfff00000u;

// internal.jl:107-113
SMC_HD inline uint32_t hashtable_size(uint64_t n) {
  uint32_t ht = 256;
  while (ht < kMaxHashTableSize && ht < n) ht <<= 1;
  return ht;
}

// internal.jl:35-46 layout: bits 0-7 length, 8-10 copy offset>>8, 11-13 extra bytes.
SMC_HD inline uint32_t char_entry(uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  // branch-free on the device: the kind-switch compiles to a divergent branch tree that a wave of
  // mixed tags runs every arm of (exec masks, ~16 SALU); these are selects on the same values
  const uint32_t kind = c & 3, hi = c >> 2;
  const uint32_t tlc = __builtin_amdgcn_perm(0u, 0x04020100u, kind);  // copy tag bytes 1/2/4 (kind 0: 0)
  const uint32_t lit = hi < 60 ? hi + 1 : (((hi - 59) << 11) | 1);
  const uint32_t cp1 = (1u << 11) | ((c >> 5) << 8) | (4 + (hi & 7));
  const uint32_t cpx = (tlc << 11) | (hi + 1);
  return kind == 0 ? lit : (kind == 1 ? cp1 : cpx);
#else
  uint32_t kind = c & 3, hi = c >> 2;
  if (kind == 0) return hi < 60 ? hi + 1 : (((hi - 59) << 11) | 1);
  if (kind == 1) return (1u << 11) | ((c >> 5) << 8) | (4 + ((c >> 2) & 7));
  if (kind == 2) return (2u << 11) | (hi + 1);
  return (4u << 11) | (hi + 1);
#endif
}

using smc::varint_len;

// ---- one tag (internal.jl:426-462) ---------------------------------------------------------------
// What every walker -- the kernels' scalar steps, host_walk, literal_only -- reads from a tag byte
// and the four bytes behind it: the table entry and the trailer, the low taglen bytes of the
// lookahead.  The leniencies live here and nowhere else: the literal length is len + trailer in
// UInt32 arithmetic (it wraps), and the lookahead arrives zero-padded past the input's end.
struct Tag {
  uint32_t c;        // the tag byte
  uint32_t entry;    // its table entry (char_entry)
  uint32_t taglen;   // bytes behind the tag byte that belong to the tag (0..4): entry >> 11
  uint32_t trailer;  // the low taglen bytes of the lookahead
  SMC_HD uint32_t len() const { return entry & 0xff; }  // a copy's length, a literal's base length
  SMC_HD bool is_copy() const { return (c & 3) != 0; }
  SMC_HD uint32_t offset() const { return (entry & 0x700) + trailer; }  // (a copy's)
  SMC_HD uint32_t literal_len() const { return len() + trailer; }       // (a literal's; u32 wrap, as the reference)
  SMC_HD uint32_t out_bytes() const { return is_copy() ? len() : literal_len(); }
  // bytes in the stream: the tag and, for a literal, its bytes (64-bit: a wrapped length stays exact)
  SMC_HD uint64_t size() const { return is_copy() ? 1 + taglen : 1ull + taglen + literal_len(); }
};

// The tag with tag byte c; tr_raw = the four stream bytes after it, little-endian, zero where the
// input has ended (internal.jl:426-430).  Loading them is the caller's business.  In two steps for
// a caller that fetches the lookahead after it knows the tag byte (a wave's scalar step reads each
// through readfirstlane, and the order of those is the order of its instructions).
SMC_HD inline Tag tag_head(uint32_t c) {
  const uint32_t entry = char_entry(c);
  return {c, entry, entry >> 11, 0u};
}
SMC_HD inline Tag with_trailer(Tag t, uint32_t tr_raw) {
  t.trailer = t.taglen >= 4 ? tr_raw : (tr_raw & ((1u << (8 * t.taglen)) - 1u));
  return t;
}
SMC_HD inline Tag decode_tag(uint32_t c, uint32_t tr_raw) { return with_trailer(tag_head(c), tr_raw); }
// ... from the eight stream bytes at the tag
SMC_HD inline Tag decode_tag8(uint64_t hv) { return decode_tag((uint32_t)hv & 0xff, (uint32_t)(hv >> 8)); }

// Output bytes of a tag the window walk sized (sm_dec_walk.h walk_window: size csz != 255, so a
// copy or a literal of at most 200 bytes): a copy's length, and for a literal, whose size is
// 1 + taglen + length, the rest -- no trailer needed.
SMC_HD inline uint32_t window_out_bytes(uint32_t c, uint32_t csz) {
  const uint32_t e = char_entry(c);
  return (c & 3) ? (e & 0xff) : csz - 1 - (e >> 11);
}

// The reference's three checks of tag t in their order (incremental_copy! internal.jl:499, :505;
// copy_literal! :518), in its arithmetic: t writes at output position op of `size` declared
// bytes, and a literal's bytes start at lsrc of N input bytes.
// Two shorter forms are equivalent, which is why no caller needs its own:
//  * :499 `op - 1 <= offset - 1` with unsigned wrap is offset == 0 || offset > op: offset 0 wraps
//    to 0xffffffff, above any 32-bit op, and otherwise both sides drop the same 1;
//  * :505's leniency (no length check on the 2 x 8-byte fast path, :500) never clears an error:
//    it needs avail_out >= 16 >= len, and the error is avail_out < len.  So :505 is
//    op + len > size.
SMC_HD inline int32_t check_tag(const Tag& t, uint64_t op, uint32_t size, uint64_t lsrc, uint32_t N) {
  const int64_t avail_out = (int64_t)size - (int64_t)op;
  if (t.is_copy()) {
    const uint32_t offset = t.offset();
    if ((int64_t)op <= (int64_t)(uint32_t)(offset - 1u)) return kErrCopyOffset;                                  // :499
    if (!(t.len() <= 16 && offset >= 8 && avail_out >= 16) && avail_out < (int64_t)t.len()) return kErrCopyLength;  // :505
    return kOk;
  }
  const uint32_t litlen = t.literal_len();
  const int64_t avail_in = (int64_t)N - (int64_t)lsrc;
  return avail_out < (int64_t)litlen || avail_in < (int64_t)litlen ? kErrLiteral : kOk;                           // :518
}

// bytes of the literal tag for a run of len (>0) bytes (internal.jl:271-284)
SMC_HD inline uint32_t literal_tag_bytes(uint32_t len) {
  uint32_t n = len - 1;
  return n < 60 ? 1 : n < 256 ? 2 : n < 65536 ? 3 : n < (1u << 24) ? 4 : 5;
}

// bytes emit_copy! (internal.jl:306-329) produces for (offset, len)
SMC_HD inline uint32_t copy_tag_bytes(uint32_t offset, uint32_t len) {
  if (len < 12) return (offset < 2048) ? 2 : 3;
  uint32_t b = 0;
  while (len >= 68) { b += 3; len -= 64; }
  if (len > 64) { b += 3; len -= 60; }
  return b + ((len < 12 && offset < 2048) ? 2 : 3);
}

}  // namespace sm
