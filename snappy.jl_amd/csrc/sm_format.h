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

using smc::varint_byte;
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

// ---- the emit rules: what a compressor writes for one token ---------------------------------------
// A tag's bytes packed little-endian (byte j of the stream is bytes >> 8 j) and how many they are.
struct TagBytes {
  uint64_t bytes;
  uint32_t size;
  SMC_HD uint8_t byte(uint32_t j) const { return (uint8_t)(bytes >> (8 * j)); }
};

// Which runs get the one-byte literal tag.  The format allows it up to 60 bytes, and the fast
// modes, the literal fallbacks and the screen use all of it (kLiteralStd).  The reference does so
// only below 60 (quirk Q3, internal.jl:271: a 60-byte run gets a two-byte tag), and reference mode
// reproduces that byte for byte (kLiteralQ3).  The two differ at len = 60 and nowhere else.
enum LiteralRule : uint32_t { kLiteralStd = 0, kLiteralQ3 = 1 };

// emit_literal!'s tag (internal.jl:271-284) for a run of len (> 0) bytes: len - 1 in the tag byte,
// or 60..63 there and len - 1 in the 1..4 bytes behind it.  literal_tag1 is the one-byte form alone,
// for a caller that knows its run is shorter than 60 bytes (both rules agree there): the fast
// parse's runs between two copies of one lane, where the general form's selects cost 1.4% of the
// kernel.
SMC_HD inline uint32_t literal_tag1(uint32_t len) { return (len - 1) << 2; }
SMC_HD inline TagBytes literal_tag(uint32_t len, LiteralRule rule) {
  const uint32_t n = len - 1;
  const uint32_t count = n < 60u - rule ? 0 : n < 256 ? 1 : n < 65536 ? 2 : n < (1u << 24) ? 3 : 4;
  return {count ? ((59 + count) << 2) | ((uint64_t)n << 8) : literal_tag1(len), 1 + count};
}
// ... and its size under the standard rule
SMC_HD inline uint32_t literal_tag_bytes(uint32_t len) { return literal_tag(len, kLiteralStd).size; }

// One emit_copy_upto_64! piece (internal.jl:289-304), len in 4..64: the two-byte form (length and
// offset bits 8..10 in the tag byte) for short near copies, else the three-byte form.  Both
// encodings, then a select: no branch on the device.
SMC_HD inline TagBytes copy_piece(uint32_t offset, uint32_t len) {
  const bool c1 = len < 12 && offset < 2048;
  const uint32_t e1 = (1u + ((len - 4) << 2) + ((offset >> 3) & 0xe0u)) | ((offset & 0xffu) << 8);
  const uint32_t e2 = (2u + ((len - 1) << 2)) | (offset << 8);
  return {c1 ? e1 : e2, c1 ? 2u : 3u};
}

// emit_copy!'s split (internal.jl:306-329): the next piece of a copy with `remaining` (>= 4) bytes
// to go -- 64 while 68 or more remain, 60 when more than 64 do (so the last piece is at least 4)
SMC_HD inline uint32_t copy_piece_len(uint32_t remaining) {
  return remaining >= 68 ? 64u : remaining > 64 ? 60u : remaining;
}

// Bytes emit_copy! produces for (offset, len), any len >= 4, in closed form: the pieces before the
// last are (len - 1) >> 6 three-byte ones, and the last piece R is shorter than 12 exactly when
// ((len - 1) & 63) < 11 (R = m + 4 for m = ((len - 1) & 63) + 1 < 4, else m).  The host checker
// steps copy_piece_len over every len up to 65536 against it.  No multiply (3 n as n + 2 n).
SMC_HD inline uint32_t copy_tag_bytes(uint32_t offset, uint32_t len) {
  const uint32_t t = len - 1, n = t >> 6;
  return n + 2 * n + (((t & 63) < 11 && offset < 2048) ? 2u : 3u);
}

// A block of n bytes written as ONE literal, the fallback of every parse that came out larger
// (and the screen's output): varint(n) when the block carries its header, the standard literal
// tag, the bytes.  An empty block is its header alone.  The size, and byte j of the varint and tag.
SMC_HD inline uint32_t block_literal_bytes(uint32_t n, bool header) {
  return (header ? varint_len(n) : 0u) + (n ? literal_tag_bytes(n) + n : 0u);
}
SMC_HD inline uint8_t block_literal_head_byte(uint32_t n, bool header, uint32_t j) {
  const uint32_t hv = header ? varint_len(n) : 0u;
  return j < hv ? varint_byte(n, j, hv) : literal_tag(n, kLiteralStd).byte(j - hv);
}

// ---- the parts of one block (k_compress_sc_span's outputs) joined into the block's stream --------
// part_len[i]: part i's length, or a compressor's error mark.  A mark, or a part longer than its
// pitch (it would have run into the next part's slot: never expected), refuses the block: mark is
// the parts' marks or-ed, kOutLenError | 8 for an over-long part.  Part 0 may instead hold a
// screened block's literal with its header (part0_literal: up to 5 bytes over the bare literal).
// Otherwise bytes is the block's length in the stream and before the bytes ahead of part j: the
// parts behind one another, or -- when they sum to more than the block as one literal, or the
// block is empty -- that literal (block_literal_bytes; before = 0, only j = 0 writes it).
struct PartsVerdict {
  uint32_t mark;    // != 0: the block's error mark, nothing is written
  uint32_t bytes;
  uint32_t before;
  bool literal;
};
SMC_HD inline PartsVerdict parts_verdict(const uint32_t* part_len, uint32_t parts, uint32_t j, uint32_t pitch,
                                         uint32_t n, bool header, bool part0_literal) {
  const uint32_t lit = block_literal_bytes(n, header);
  uint32_t sum = 0, before = 0, mark = 0;
  for (uint32_t i = 0; i < parts; ++i) {
    const uint32_t L = part_len[i];
    const uint32_t bound = (i == 0 && part0_literal && lit + 5u > pitch) ? lit + 5u : pitch;
    if (L >= kOutLenError)
      mark |= L;
    else if (L > bound)
      mark |= kOutLenError | 8u;
    else {
      sum += L;
      before += i < j ? L : 0u;
    }
  }
  const bool literal = n == 0 || sum > lit;
  return {mark, literal ? lit : sum, literal ? 0u : before, literal};
}

}  // namespace sm
