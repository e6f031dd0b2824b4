// smf_range.h -- the rules of the ranged decode (smf_uncompress_ranges_device), shared by its
// kernels (smf_range.hip) and the host (smf_range_plan in smf_host.cpp, which the sanitizer driver
// runs): the touched-chunk search, the checks of an index entry and the direct-or-edge decision.
// Plain functions over pointers, compiled for the host and the device alike, so the host checker
// tests the code the kernels run.  The index is an untrusted hint: every function here is total
// over its arguments, and what it returns keeps the decode inside the stream and the range.
// Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smf_format.h"
#include "smf_slots.h"

namespace smf {

constexpr uint32_t kMaxIndexChunks = 0x7fffffffu;  // a longer index: SM_ERR_ARGUMENT
constexpr uint64_t kEdgePitch = kBlock;            // an edge slot: one whole chunk

// How many of off[0, cnt) are <= v, for a non-decreasing off; any other array gives some value in
// [0, cnt].  At most 32 steps, every read inside off[0, cnt).
template <typename T>
SMC_HD inline uint32_t upper_bound(const T* off, uint32_t cnt, T v) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct RangeChunks {
  uint32_t first, count;  // chunks [first, first + count) get a slot each; count 0: nothing is decoded
  int32_t status;         // SM_OK, or SM_ERR_ARGUMENT for a range that leaves the stream
};

// The chunks of range [lo, lo + len): from the one that holds lo to the one that holds
// lo + len - 1.  Taking the upper bound skips empty chunks at both ends (of equal offsets, the last
// one is found, and that one is not empty); empty chunks in between keep a slot and are passed over.
// chunk_off has nchunks + 1 entries.  first + count <= nchunks whatever chunk_off holds.
SMC_HD inline RangeChunks range_chunks(const uint64_t* chunk_off, uint32_t nchunks, uint64_t lo, uint64_t len) {
  RangeChunks r{0, 0, SM_OK};
  if (len == 0) return r;
  if (lo + len < lo || lo + len > chunk_off[nchunks] || nchunks == 0) {
    r.status = SM_ERR_ARGUMENT;
    return r;
  }
  uint32_t f = upper_bound(chunk_off, nchunks + 1, lo);
  f = f ? f - 1 : 0;
  if (f > nchunks - 1) f = nchunks - 1;
  uint32_t l = f + upper_bound(chunk_off + f, nchunks + 1 - f, lo + (len - 1));
  l = l > f ? l - 1 : f;
  if (l > nchunks - 1) l = nchunks - 1;
  r.first = f;
  r.count = l - f + 1;
  return r;
}

// The checks of a touched entry: chunk c of an n-byte stream, off0 / off1 = chunk_off[c], [c + 1].
// SM_OK means: the payload lies inside the stream, the chunk's bytes are [off0, off0 + ulen)
// without overflow, and ulen fits an edge slot.
SMC_HD inline int32_t entry_check(uint32_t type, uint64_t pay_off, uint32_t pay_len, uint32_t ulen, uint64_t off0,
                                  uint64_t off1, uint64_t n) {
  if (type > SMF_CHUNK_UNCOMPRESSED) return SM_ERR_ARGUMENT;
  if (ulen > kBlock) return SM_ERR_ARGUMENT;
  if (off1 < off0 || off1 - off0 != ulen) return SM_ERR_ARGUMENT;
  if (pay_off > n || n - pay_off < pay_len) return SM_ERR_ARGUMENT;
  if (type == SMF_CHUNK_UNCOMPRESSED && pay_len != ulen) return SM_ERR_ARGUMENT;
  return SM_OK;
}

struct Place {
  int32_t status;    // SM_OK, or SM_ERR_ARGUMENT: the chunk is not decoded
  uint32_t edge;     // 0: decoded straight into the range's output at `dst`; 1 / 2: into the range's
                     // first / second edge slot, of which bytes [src, src + n) go to `dst`
  uint32_t src, n;
  uint64_t dst;      // offset in the range's output; dst + (edge ? n : ulen) <= len
};

// Where a checked chunk (bytes [a, a + u) of the content, u > 0) of range [lo, lo + len) decodes
// to.  Wholly inside the range: direct.  Else it has to be the range's first or last chunk and to
// meet the range -- with a consistent index every other chunk lies inside -- so a range never
// needs more than its two edge slots.
SMC_HD inline Place chunk_place(uint64_t a, uint32_t u, uint64_t lo, uint64_t len, bool is_first, bool is_last) {
  Place p{SM_OK, 0, 0, 0, 0};
  if (a >= lo && a - lo <= len && len - (a - lo) >= u) {
    p.dst = a - lo;
    return p;
  }
  const uint64_t s = a > lo ? a : lo;
  const uint64_t e = a + u < lo + len ? a + u : lo + len;  // (neither sum overflows: both were checked)
  if (!(is_first || is_last) || s >= e) {
    p.status = SM_ERR_ARGUMENT;
    return p;
  }
  p.edge = is_first ? 1 : 2;
  p.src = (uint32_t)(s - a);
  p.n = (uint32_t)(e - s);
  p.dst = s - lo;
  return p;
}

// Slot k of a range's `count`: chunk first + k.  skip: an empty chunk in between, not touched.
// (The searches never end on an empty chunk of a consistent index: there it fails the range.)
SMC_HD inline Place slot_place(const smf_chunks& ch, const uint64_t* chunk_off, uint64_t n, uint32_t c, uint64_t lo,
                               uint64_t len, bool is_first, bool is_last, bool& skip) {
  const uint32_t u = ch.ulen[c];
  skip = u == 0 && !(is_first || is_last);
  Place p{SM_OK, 0, 0, 0, 0};
  if (skip) return p;
  if (u == 0) {
    p.status = SM_ERR_ARGUMENT;
    return p;
  }
  p.status = entry_check(ch.type[c], ch.pay_off[c], ch.pay_len[c], u, chunk_off[c], chunk_off[c + 1], n);
  if (p.status != SM_OK) return p;
  return chunk_place(chunk_off[c], u, lo, len, is_first, is_last);
}

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct RangeScratch {
  GroupHeader* hdr;
  // per slot (m = max_range_chunks): the stage's arrays (a slot's group is its range; out_off is
  // relative to the edge slots), and of an edge slot the bytes that go to the range's output
  Slots slots;
  uint64_t* trim_dst;
  uint32_t *trim_src, *trim_len;
  // per range
  uint32_t *first, *count, *base;
  int32_t* rpre;
  uintptr_t end;
};

inline RangeScratch carve_range(uint8_t* buf, size_t nranges, size_t m) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  RangeScratch s;
  s.hdr = c.take<GroupHeader>(1);
  s.slots = carve_slots(c, m, nranges, true, true, true);
  s.trim_dst = c.take<uint64_t>(m);
  s.trim_src = c.take<uint32_t>(m);
  s.trim_len = c.take<uint32_t>(m);
  s.first = c.take<uint32_t>(nranges);
  s.count = c.take<uint32_t>(nranges);
  s.base = c.take<uint32_t>(nranges + 1);
  s.rpre = c.take<int32_t>(nranges);
  s.end = c.p;
  return s;
}
inline size_t range_meta_bytes(size_t nranges, size_t m) { return (size_t)carve_range(nullptr, nranges, m).end; }
inline size_t range_edge_bytes(size_t nranges) { return 2 * nranges * (size_t)kEdgePitch; }

}  // namespace smf
