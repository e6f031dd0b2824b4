// smm_plan.h -- what the device plans of the multi-stream library (smm_kernels.hip) and its host
// side (smm_host.cpp, smm_api.hip) share: the fragment arithmetic, the index rules of
// smm_uncompress_device, the rule that builds an index (smm_index_device), the scratch layout, and
// the launchers' interfaces.  The rules are plain functions over pointers, compiled for the host and
// the device alike, so the host checker (smm_index_check, run under sanitizers by
// smm_host_check.cpp) tests the code the kernels run.  The index walk has two forms, the scalar
// loop here (smm_index_host) and one wave's window walk (smm_index.hip): both size a tag by
// sm_format.h's decode_tag rule, and the tests hold them against each other.
// Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_multi.h"
#include "../common/smc_layout.h"
#include "../sm_format.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace smm {

using smc::max_compressed_length;

constexpr uint32_t kBlock = SM_BLOCK_SIZE;
constexpr uint32_t kMaxInput = 0x7fffffffu;   // a longer stream: SM_ERR_INPUT_TOO_LARGE, unread
constexpr uint32_t kNoStream = 0xffffffffu;   // a fragment slot no stream owns
constexpr uint64_t kSlotPitch = smc::kMultiSlotPitch;  // a fragment's slot
constexpr uint32_t kDummy = 64;               // a long stream's slot in the short-stream call: "00", with the
                                              // room an empty input's slot has (sm_max_compressed_length(0) = 32)

constexpr uint32_t kIndexStage = 4096;        // bytes of a stream the index walk stages into LDS per piece
                                              // (smm_index.hip; a prefetched second piece lies beside it)

SMC_HD inline uint32_t fragment_count(uint64_t len) { return (uint32_t)((len + kBlock - 1) / kBlock); }
using smc::varint_len;

// ---- the index rules (include/snappy_mi355x_multi.h, smm_uncompress_device) ------------------
// The rule on d_frag_first at element s < nstreams: from 0, non-decreasing, the last <= max_fragments.
SMC_HD inline bool first_rule(const uint32_t* first, uint32_t s, uint32_t nstreams, uint32_t max_fragments) {
  if (s == 0 && first[0] != 0) return false;
  if (first[s] > first[s + 1]) return false;
  return s + 1 < nstreams || first[nstreams] <= max_fragments;
}

struct Candidate {
  uint32_t D, hv, e0, count;  // declared length, varint bytes, first entry, entries (= fragments)
};

// Stream-level rules, everything but the positions: p[0..n) is the stream, cap its output room,
// [e0, e1) its entries.  Bounds first: a candidate's entries lie inside d_frag_pos.
SMC_HD inline bool stream_candidate(const uint8_t* p, uint32_t n, uint32_t cap, uint32_t e0, uint32_t e1,
                                    uint32_t max_fragments, Candidate& c) {
  if (e0 > e1 || e1 > max_fragments) return false;
  if (n >= SM_OUT_LEN_ERROR) return false;  // (an error mark, not a length: the decoder's business)
  if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)p[i]; }, n, c.D, c.hv) != 0) return false;  // (reads at most min(n, 5) bytes)
  if (c.D <= kBlock || c.D > cap) return false;
  c.e0 = e0;
  c.count = e1 - e0;
  return c.count == fragment_count(c.D);
}

// Fragment f of a candidate: its bytes [lo, hi) in the stream.  pos: the stream's `count` entries.
// True for every f exactly when the first position is hv, the positions increase strictly and the
// last is below n; and a fragment that passes alone lies inside the stream whatever the others hold.
SMC_HD inline bool fragment_range(const uint32_t* pos, uint32_t f, uint32_t count, uint32_t hv, uint32_t n,
                                  uint32_t& lo, uint32_t& hi) {
  lo = pos[f];
  hi = f + 1 < count ? pos[f + 1] : n;
  if (f == 0 && lo != hv) return false;
  return lo >= hv && lo < hi && hi <= n;
}

// what fragment f of `count` must decode to
SMC_HD inline uint32_t fragment_length(uint32_t D, uint32_t f, uint32_t count) {
  return f + 1 < count ? kBlock : D - kBlock * (count - 1);
}

// ---- building an index (include/snappy_mi355x_multi.h, smm_index_device) ----------------------
// A stream's entries: D, the varint's bytes and fragment_count(D) when the length is no error mark,
// the header parses and D fits the room; else all zero.
struct IndexCount {
  uint32_t D, hv, count;
};
SMC_HD inline IndexCount index_count(const uint8_t* p, uint32_t n, uint32_t cap) {
  uint32_t D, hv;
  if (n >= SM_OUT_LEN_ERROR) return {0, 0, 0};
  if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)p[i]; }, n, D, hv) != 0 || D > cap) return {0, 0, 0};
  return {D, hv, fragment_count(D)};
}

// The positions of a stream that declares more than 64 KiB: the tag sizes from hv on, no copy made
// and no offset or length checked.  A tag must start at every output multiple of 65536 below D;
// pos[f] is where.  Bytes at or past n read as zero (the decoder's zero-padded lookahead), and
// positions and outputs are 64-bit, so a literal length that wraps ends the walk at x >= n.  False,
// with all `count` entries zero, when the stream ends first or a tag crosses such a multiple.
inline bool index_walk(const uint8_t* p, uint32_t n, uint32_t hv, uint32_t count, uint32_t* pos) {
  uint64_t x = hv, o = 0;
  uint32_t f = 0;
  while (x < n) {
    const uint64_t at = (uint64_t)kBlock * f;
    if (o > at) break;
    if (o == at) {
      pos[f++] = (uint32_t)x;
      if (f == count) return true;
    }
    uint32_t tr = 0;
    for (uint32_t k = 0; k < 4; ++k) tr |= (x + 1 + k < n ? (uint32_t)p[x + 1 + k] : 0u) << (8 * k);
    const sm::Tag t = sm::decode_tag(p[x], tr);
    x += t.size();
    o += t.out_bytes();
  }
  for (f = 0; f < count; ++f) pos[f] = 0;
  return false;
}

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
using smc::Carve;

struct Header {  // the plans' words for the kernels behind them
  uint32_t nlong;     // compress: fragments of the long streams; uncompress: of the candidates
  uint32_t nindex;    // compress: index entries
  uint32_t stop;      // compress: more fragments than max_fragments; uncompress: d_frag_first broken
  uint32_t indexed;   // uncompress: streams decoded by fragments
};

struct CompressScratch {
  uint64_t *s_out_off, *f_in_off, *f_slot_off, *gpos;
  uint32_t *s_in_len, *s_comp_len, *lfirst, *ifirst, *bad, *f_in_len, *f_comp_len, *f_stream;
  uint8_t* dummy;
  uintptr_t end;
};
inline CompressScratch carve_compress(uint8_t* base, size_t n, size_t m) {
  Carve c{reinterpret_cast<uintptr_t>(base)};
  CompressScratch s;
  s.s_out_off = c.take<uint64_t>(n);
  s.f_in_off = c.take<uint64_t>(m);
  s.f_slot_off = c.take<uint64_t>(m);
  s.gpos = c.take<uint64_t>(m + 1);
  s.s_in_len = c.take<uint32_t>(n);
  s.s_comp_len = c.take<uint32_t>(n);
  s.lfirst = c.take<uint32_t>(n + 1);
  s.ifirst = c.take<uint32_t>(n + 1);
  s.bad = c.take<uint32_t>(n);
  s.f_in_len = c.take<uint32_t>(m);
  s.f_comp_len = c.take<uint32_t>(m);
  s.f_stream = c.take<uint32_t>(m);
  s.dummy = c.take<uint8_t>(n * kDummy);
  s.end = c.p;
  return s;
}

struct DecodeScratch {
  uint64_t *f_in_off, *f_out_off;
  uint32_t *D, *hv, *e0, *efirst, *cand, *bad, *indexed, *fb_in_len, *fb_cap, *f_in_len, *f_len, *f_out_len, *f_stream;
  int32_t* f_status;
  uintptr_t end;
};
inline DecodeScratch carve_decode(uint8_t* base, size_t n, size_t m) {
  Carve c{reinterpret_cast<uintptr_t>(base)};
  DecodeScratch s;
  s.f_in_off = c.take<uint64_t>(m);
  s.f_out_off = c.take<uint64_t>(m);
  s.D = c.take<uint32_t>(n);
  s.hv = c.take<uint32_t>(n);
  s.e0 = c.take<uint32_t>(n);
  s.efirst = c.take<uint32_t>(n + 1);
  s.cand = c.take<uint32_t>(n);
  s.bad = c.take<uint32_t>(n);
  s.indexed = c.take<uint32_t>(n);
  s.fb_in_len = c.take<uint32_t>(n);
  s.fb_cap = c.take<uint32_t>(n);
  s.f_in_len = c.take<uint32_t>(m);
  s.f_len = c.take<uint32_t>(m);
  s.f_out_len = c.take<uint32_t>(m);
  s.f_stream = c.take<uint32_t>(m);
  s.f_status = c.take<int32_t>(m);
  s.end = c.p;
  return s;
}
struct IndexScratch {
  uint32_t *D, *hv, *stop;  // per stream: the declared length (0: no entries) and the varint's bytes; the overflow word
  uintptr_t end;
};
inline IndexScratch carve_index(uint8_t* base, size_t n) {
  Carve c{reinterpret_cast<uintptr_t>(base)};
  IndexScratch s;
  s.D = c.take<uint32_t>(n);
  s.hv = c.take<uint32_t>(n);
  s.stop = c.take<uint32_t>(1);
  s.end = c.p;
  return s;
}
inline size_t compress_meta_bytes(size_t n, size_t m) { return (size_t)carve_compress(nullptr, n, m).end; }
inline size_t decode_meta_bytes(size_t n, size_t m) { return (size_t)carve_decode(nullptr, n, m).end; }
inline size_t index_scratch_bytes(size_t n) { return (size_t)carve_index(nullptr, n).end; }
constexpr size_t kHeaderBytes = 256;
inline size_t scratch_bytes(size_t n, size_t m) {
  const size_t c = compress_meta_bytes(n, m) + m * kSlotPitch, d = decode_meta_bytes(n, m), i = index_scratch_bytes(n);
  return kHeaderBytes + (c > d ? (c > i ? c : i) : (d > i ? d : i));
}

#if defined(__HIPCC__)
// the stream (smm_kernels.hip) or the range (smm_range.hip) that owns slot j: the largest s < n with
// first[s] <= j (first: an exclusive scan from 0, n + 1 entries, j < first[n]) -- one with no slots
// is never the largest
__device__ inline uint32_t owner(const uint32_t* first, uint32_t n, uint32_t j) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- launchers (smm_kernels.hip); all pointers are device pointers -----------------------------
struct CompressPlan {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint32_t n, m;
  uint8_t* out;
  const uint64_t* out_off;
  uint32_t* out_len;
  int32_t* status;
  uint32_t* frag_first;  // both or neither
  uint32_t* frag_pos;
  const uint8_t* slots;
  CompressScratch s;
  Header* hdr;
};
// the counts' scans and the two raw calls' argument arrays
hipError_t launch_compress_plan(const CompressPlan& p, hipStream_t st);
// behind the raw calls: the fragments' places, the packed long streams, every stream's results
hipError_t launch_pack(const CompressPlan& p, hipStream_t st);

struct DecodePlan {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint32_t n, m;
  const uint64_t* out_off;
  const uint32_t* out_cap;
  uint32_t* out_len;
  int32_t* status;
  const uint32_t* frag_first;
  const uint32_t* frag_pos;
  DecodeScratch s;
  Header* hdr;
};
// the index rules and the raw fragment decoder's arguments
hipError_t launch_decode_plan(const DecodePlan& p, hipStream_t st);
// behind the fragment decoder: the verdicts and the fallback's masked arguments
hipError_t launch_reduce(const DecodePlan& p, hipStream_t st);
// behind the fallback: the indexed streams' results over its own
hipError_t launch_merge(const DecodePlan& p, hipStream_t st);

struct IndexPlan {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint32_t n, m;
  const uint32_t* out_cap;  // NULL: no cap
  uint32_t* frag_first;
  uint32_t* frag_pos;
  uint8_t* built;
  int32_t* status;
  IndexScratch s;
};
// smm_index.hip: the counts' scan with the short streams' entries, then a walk per long stream
hipError_t launch_index(const IndexPlan& p, hipStream_t st);
#endif

}  // namespace smm
