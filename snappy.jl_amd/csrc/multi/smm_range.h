// smm_range.h -- the rules of the ranged decode of indexed raw streams
// (include/snappy_mi355x_multi_range.h, smm_uncompress_ranges_device), shared by its kernels
// (smm_range.hip) and the host (smm_range_plan in smm_host.cpp, which the sanitizer driver runs):
// what is decided about a range before any fragment byte is read, the fragments it touches, where
// each of them decodes to, the verdicts, and the scratch layout.  Plain functions over pointers,
// compiled for the host and the device alike.  The index is an untrusted hint: every function here
// is total over its arguments, and what it returns keeps the decode inside the stream and the
// range.  The fragment arithmetic and the entry check are smm_plan.h's, the varint rule
// smc_layout.h's.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_multi_range.h"
#include "smm_plan.h"

namespace smm {

constexpr uint64_t kEdgePitch = kBlock;     // an edge slot: one whole fragment
constexpr uint32_t kNoSlot = 0xffffffffu;   // a range none of whose slots failed

// the fragments that hold bytes [lo, lo + len): raw fragments are 65,536 bytes apart in every stream
SMC_HD inline uint32_t range_fragment_count(uint32_t lo, uint32_t len) {
  if (len == 0) return 0;
  return (uint32_t)((((uint64_t)lo + len - 1) / kBlock) - lo / kBlock + 1);
}

// ---- the stream-level rule -------------------------------------------------------------------------
// What is known about range (s, lo, len) before any fragment byte is read.  SM_OK with first = count
// = 0 for an empty range, whatever else holds; SM_OK with the stream's numbers in c and the touched
// fragments [first, first + count) of it; else SM_ERR_ARGUMENT with count 0.  Reads in_off[s],
// in_len[s], frag_first[s], frag_first[s + 1] and the stream's first min(n, 5) bytes, each only
// after the checks that make it readable: nothing of another stream, and no entry of frag_pos.
// On SM_OK with count > 0: c.e0 + c.count <= nentries, first + count <= c.count, lo + len <= c.D.
struct RangeSpan {
  uint32_t first, count;
  int32_t status;
};
SMC_HD inline RangeSpan range_span(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                                   const uint32_t* frag_first, uint32_t nentries, uint32_t s, uint32_t lo, uint32_t len,
                                   Candidate& c) {
  c = Candidate{0, 0, 0, 0};
  if (len == 0) return {0, 0, SM_OK};
  const RangeSpan bad{0, 0, SM_ERR_ARGUMENT};
  if (s >= nstreams) return bad;
  const uint32_t n = in_len[s];
  if (n >= SM_OUT_LEN_ERROR) return bad;  // (an error mark, not a length: nothing of it is read)
  const uint8_t* const p = in + in_off[s];
  if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)p[i]; }, n, c.D, c.hv) != 0) return bad;
  const uint32_t e0 = frag_first[s], e1 = frag_first[s + 1];
  if (e0 > e1 || e1 > nentries) return bad;
  c.e0 = e0;
  c.count = e1 - e0;
  if (c.count != fragment_count(c.D)) return bad;
  if ((uint64_t)lo + len > c.D) return bad;
  return {lo / kBlock, range_fragment_count(lo, len), SM_OK};
}

// ---- a touched fragment ----------------------------------------------------------------------------
// Where fragment f (of `count`, of a stream that declares D) of range [lo, lo + len) decodes to.
// A whole 64 KiB wholly inside the range: straight into the range's output at dst, all n = 65,536
// bytes.  Else -- partly covered, or the stream's short last fragment -- into an edge slot, of which
// bytes [src, src + n) go to dst.  For every argument
// src + n <= fragment_length(D, f, count) and dst + n <= len (n is 0 where the two do not meet).
struct Place {
  uint32_t edge;  // 0: direct; 1: by an edge slot
  uint32_t src, n, dst;
};
SMC_HD inline Place fragment_place(uint32_t D, uint32_t f, uint32_t count, uint32_t lo, uint32_t len) {
  const uint64_t a = (uint64_t)kBlock * f, b = a + fragment_length(D, f, count);
  const uint64_t r0 = lo, r1 = r0 + len;
  if (a >= r0 && b <= r1 && b - a == kBlock) return {0, 0, kBlock, (uint32_t)(a - r0)};
  const uint64_t s = a > r0 ? a : r0, e = b < r1 ? b : r1;
  if (s >= e) return {1, 0, 0, 0};
  return {1, (uint32_t)(s - a), (uint32_t)(e - s), (uint32_t)(s - r0)};
}

// A range's edge slots: only its first and its last fragment can be partly covered or short (every
// fragment between them is 64 KiB inside the range), so 0, 1 or 2; `which` is the slot fragment f gets, 0 or 1.
SMC_HD inline uint32_t range_edges(uint32_t D, uint32_t count, uint32_t first, uint32_t nfrag, uint32_t lo, uint32_t len) {
  if (nfrag == 0) return 0;
  const uint32_t e = fragment_place(D, first, count, lo, len).edge;
  return nfrag == 1 ? e : e + fragment_place(D, first + nfrag - 1, count, lo, len).edge;
}
SMC_HD inline uint32_t edge_which(uint32_t D, uint32_t count, uint32_t first, uint32_t f, uint32_t lo, uint32_t len) {
  return f == first ? 0u : fragment_place(D, first, count, lo, len).edge;
}

// A slot's arguments for the raw fragment decoder: fragment f of the range's stream (n bytes, c its
// numbers, pos its entries), by the entry check of smm_uncompress_device.  SM_ERR_ARGUMENT: the slot
// is not decoded.  Reads pos[f] and, below the last fragment, pos[f + 1].
struct SlotArgs {
  int32_t status;
  uint32_t in_lo, in_len, frag_len;  // the fragment's bytes in the stream, and what it must decode to
  Place place;
};
SMC_HD inline SlotArgs slot_args(const uint32_t* pos, const Candidate& c, uint32_t n, uint32_t f, uint32_t lo,
                                 uint32_t len) {
  SlotArgs a{SM_ERR_ARGUMENT, 0, 0, 0, {0, 0, 0, 0}};
  uint32_t p0, p1;
  if (f >= c.count || !fragment_range(pos, f, c.count, c.hv, n, p0, p1)) return a;
  a.status = SM_OK;
  a.in_lo = p0;
  a.in_len = p1 - p0;
  a.frag_len = fragment_length(c.D, f, c.count);
  a.place = fragment_place(c.D, f, c.count, lo, len);
  return a;
}

// ---- verdicts --------------------------------------------------------------------------------------
// a slot: the entry check's status, else what the fragment decoder said
SMC_HD inline int32_t slot_verdict(int32_t pre, int32_t decoded) { return pre != SM_OK ? pre : decoded; }

// A range: over the bound nothing is served; a failed stream-level rule; else the verdict of its
// first failing slot in stream order (first_failed: that verdict, SM_OK when none failed).
SMC_HD inline int32_t range_verdict(bool stop, int32_t pre, int32_t first_failed) {
  if (stop) return SM_ERR_ARGUMENT;
  return pre != SM_OK ? pre : first_failed;
}

// ---- scratch (smc::Carve: a null base measures) ----------------------------------------------------
struct RangeHeader {
  uint32_t total;  // the slots of all ranges (saturated)
  uint32_t stop;   // more of them than max_range_fragments: nothing is decoded
};

struct RangeScratch {
  RangeHeader* hdr;
  // per range (n): the stream's numbers, the touched span, the scanned slot and edge counts, the
  // stream-level status and the lowest failing slot
  uint32_t *D, *hv, *e0, *count, *first, *nfrag, *nedge, *base, *ebase, *fail;
  int32_t* pre;
  // per slot (m): the fragment decoder's arguments and results (out_off is relative to the edge
  // slots), the entry check's status, the slot's range, and of an edge slot the bytes that go to
  // the range's output
  uint64_t *f_in_off, *f_out_off, *trim_dst;
  uint32_t *f_in_len, *f_len, *f_out_len, *range, *trim_src, *trim_len;
  int32_t *f_status, *f_pre;
  uintptr_t end;
};
inline RangeScratch carve_range(uint8_t* buf, size_t n, size_t m) {
  Carve c{reinterpret_cast<uintptr_t>(buf)};
  RangeScratch s;
  s.hdr = c.take<RangeHeader>(1);
  s.D = c.take<uint32_t>(n);
  s.hv = c.take<uint32_t>(n);
  s.e0 = c.take<uint32_t>(n);
  s.count = c.take<uint32_t>(n);
  s.first = c.take<uint32_t>(n);
  s.nfrag = c.take<uint32_t>(n);
  s.nedge = c.take<uint32_t>(n);
  s.base = c.take<uint32_t>(n + 1);
  s.ebase = c.take<uint32_t>(n + 1);
  s.fail = c.take<uint32_t>(n);
  s.pre = c.take<int32_t>(n);
  s.f_in_off = c.take<uint64_t>(m);
  s.f_out_off = c.take<uint64_t>(m);
  s.trim_dst = c.take<uint64_t>(m);
  s.f_in_len = c.take<uint32_t>(m);
  s.f_len = c.take<uint32_t>(m);
  s.f_out_len = c.take<uint32_t>(m);
  s.range = c.take<uint32_t>(m);
  s.trim_src = c.take<uint32_t>(m);
  s.trim_len = c.take<uint32_t>(m);
  s.f_status = c.take<int32_t>(m);
  s.f_pre = c.take<int32_t>(m);
  s.end = c.p;
  return s;
}
inline size_t range_arrays_bytes(size_t n, size_t m) { return (size_t)carve_range(nullptr, n, m).end; }
// the edge slots: two per range, and never more than there are slots (one at the least: the
// fragment decoder takes them as its output base)
inline size_t range_edge_slots(size_t n, size_t m) {
  const size_t e = 2 * n < m ? 2 * n : m;
  return e ? e : 1;
}
inline size_t range_scratch_bytes(size_t n, size_t m) {
  return range_arrays_bytes(n, m) + range_edge_slots(n, m) * (size_t)kEdgePitch;
}

#if defined(__HIPCC__)
// ---- launchers (smm_range.hip); all pointers are device pointers -----------------------------------
struct RangeArgs {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint32_t nstreams;
  const uint32_t* frag_first;
  const uint32_t* frag_pos;
  uint32_t nentries;
  const uint32_t* range_stream;
  const uint32_t* lo;
  const uint32_t* len;
  uint32_t n, m;  // ranges, max_range_fragments
  uint8_t* out;
  const uint64_t* out_off;
  uint32_t* out_len;
  int32_t* status;
  uint8_t* edge;  // range_edge_slots(n, m) slots of kEdgePitch bytes
  RangeScratch s;
};
// find, scan, slots: the fragment decoder's arguments
hipError_t launch_range_plan(const RangeArgs& a, hipStream_t st);
// behind the fragment decoder: trim, verdict, result
hipError_t launch_range_finish(const RangeArgs& a, hipStream_t st);
#endif

}  // namespace smm
