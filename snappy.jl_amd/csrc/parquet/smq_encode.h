// smq_encode.h -- the rules of the page encoder (include/snappy_mi355x_parquet_write.h), shared by
// its kernels (smq_encode.hip) and the host (smq_host.cpp, which the sanitizer driver runs): the
// rewrite of a PageHeader around a new body, the sizes of a page's stage slot and of its output, and
// a page's status.  The walk is walk_pages<EncodeWalk> (smq_format.h).  Plain functions, compiled for
// the host and the device alike.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_parquet_write.h"
#include "smq_format.h"

namespace smq {

constexpr uint32_t kMaxBody = 0x7fffffffu;  // compressed_page_size is an i32

// the zigzag code of an i32, which a compact-protocol i32 field holds as a varint
SMC_HD inline uint32_t zigzag32(int32_t v) { return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31); }

// ---- the header rewrite ---------------------------------------------------------------------------
// The header's bytes as they are, except: field 3's value becomes the zigzag varint of the new body's
// length; field 4's value, where the header has one, that of the new body's CRC-32 as an i32; the
// header byte of the v2 field 7, where the header has one, gets type nibble 1 (true).  Both varints
// may change their length, so the rule is one of positions: byte i of the new header is a byte of
// one of the two varints or byte src(i) of the old header -- every thread of a pack can write its own.
struct Rewrite {
  Sites s;
  uint32_t a_at, a_old, a_new, a_val;  // the patched varint that comes first in the header
  uint32_t b_at, b_old, b_new, b_val;  // the second (b_old 0: none; b_at is then the header's length)
  uint32_t new_len;
};

SMC_HD inline Rewrite make_rewrite(uint32_t hdr_len, const Sites& s, uint32_t new_body_len, uint32_t crc) {
  const uint32_t v3 = zigzag32((int32_t)new_body_len), v4 = zigzag32((int32_t)crc);
  const uint32_t n3 = smc::varint_len(v3), n4 = s.f4_len ? smc::varint_len(v4) : 0u;
  Rewrite w;
  w.s = s;
  if (s.f4_len && s.f4_at < s.f3_at) {
    w.a_at = s.f4_at, w.a_old = s.f4_len, w.a_new = n4, w.a_val = v4;
    w.b_at = s.f3_at, w.b_old = s.f3_len, w.b_new = n3, w.b_val = v3;
  } else {
    w.a_at = s.f3_at, w.a_old = s.f3_len, w.a_new = n3, w.a_val = v3;
    w.b_at = s.f4_len ? s.f4_at : hdr_len, w.b_old = s.f4_len, w.b_new = n4, w.b_val = v4;
  }
  w.new_len = hdr_len - w.a_old - w.b_old + w.a_new + w.b_new;
  return w;
}

// byte i < w.new_len of the rewritten header; old(j) is byte j of the header as it was
template <typename Old>
SMC_HD inline uint8_t rewritten_byte(const Rewrite& w, Old old, uint32_t i) {
  uint32_t src;
  if (i < w.a_at) {
    src = i;
  } else if (i < w.a_at + w.a_new) {
    return smc::varint_byte(w.a_val, i - w.a_at, w.a_new);
  } else {
    const uint32_t b_out = w.b_at - w.a_old + w.a_new;  // where the second varint goes
    if (i < b_out) src = i - w.a_new + w.a_old;
    else if (i < b_out + w.b_new) return smc::varint_byte(w.b_val, i - b_out, w.b_new);
    else src = i - w.a_new + w.a_old - w.b_new + w.b_old;
  }
  const uint8_t b = (uint8_t)old(src);
  return w.s.f7_at && src == w.s.f7_at ? (uint8_t)((b & 0xf0) | kTrue) : b;
}

// ---- a page's sizes ---------------------------------------------------------------------------------
// The stage slot of a page with output: its level bytes and behind them room for the section's raw
// stream, rounded up as the framing library's slots are (smc_layout.h); a page that is stepped over
// has none.
SMC_HD inline uint64_t stage_slot(const Page& p) {
  return p.output ? (p.levels + smc::max_compressed_length(section_want(p)) + 15) / 16 * 16 : 0u;
}
// the fragments the raw compressor counts for a page: only a section above 64 KiB has any
SMC_HD inline uint64_t encode_fragments(const Page& p) {
  return p.output && section_want(p) > kFragment ? fragments(section_want(p)) : 0u;
}
// an upper bound on what the page becomes: both varints at their longest
SMC_HD inline uint64_t page_bound(const Page& p) {
  if (!p.output) return (uint64_t)p.hdr_len + p.body_len;
  return (uint64_t)p.hdr_len + 8 + p.levels + smc::max_compressed_length(section_want(p));
}

// A page's status once its section is compressed: comp_len is the raw compressor's length for it
// (0 with comp_status not SM_OK).  A page that is stepped over has SM_OK.
SMC_HD inline int32_t page_verdict(bool output, uint32_t levels, uint32_t comp_len, int32_t comp_status) {
  if (!output) return SM_OK;
  if (comp_status != SM_OK || comp_len == 0) return SM_ERR_DEVICE;
  return (uint64_t)levels + comp_len > kMaxBody ? (int32_t)SM_ERR_INPUT_TOO_LARGE : (int32_t)SM_OK;
}

// A chunk's status and length: over the caller's bounds SM_ERR_ARGUMENT; else the walk's error; else
// its first failing page's status (fail == kNoSlot: none); else SM_BUFFER_TOO_SMALL with the size
// needed when that is above cap; else SM_OK with the size.  Only SM_OK writes.
struct EncodeVerdict {
  int32_t status;
  uint64_t length;
};
SMC_HD inline EncodeVerdict encode_verdict(bool over, int32_t pre, bool failed, int32_t fail_status, uint64_t need, uint64_t cap) {
  if (over) return EncodeVerdict{SM_ERR_ARGUMENT, 0};
  if (pre != SM_OK) return EncodeVerdict{pre, 0};
  if (failed) return EncodeVerdict{fail_status, 0};
  return EncodeVerdict{need > cap ? (int32_t)SM_BUFFER_TOO_SMALL : (int32_t)SM_OK, need};
}

}  // namespace smq
