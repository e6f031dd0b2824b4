// smo_streams.h -- the rules of the batched calls (smo_uncompress_streams_device,
// smo_compress_streams_device), shared by their kernels (smo_kernels.hip) and the host
// (smo_streams_plan in smo_host.cpp, which the sanitizer driver runs): what a walked stream of a
// batch gets, a slot's and a stream's verdict, the tiling of the copies and the scratch layouts.
// The walk itself is walk_chunks (smo_format.h).  Plain functions, compiled for the host and the
// device alike, so the host checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smo_format.h"

namespace smo {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, chunks or pieces: SM_ERR_ARGUMENT
constexpr uint32_t kNoSlot = 0xffffffffu;      // a slot of no stream; a stream without a failing slot
constexpr uint32_t kNoCopy = 0xffffffffu;      // a slot's copy length when its chunk is not a stored one

struct Header {    // a plan's words for the kernels behind it
  uint32_t total;  // slots in use (0 over the bound: nothing is decoded or packed)
  uint32_t over;   // the streams need more slots than the caller's bound
};

struct StreamPlan {
  int32_t status;  // the walk's error, SM_BUFFER_TOO_SMALL, or SM_OK: what is known before any decode
  uint32_t slots;  // its chunks when it is decoded, else 0
  uint64_t length; // the declared lengths: before the error, else of the whole stream (the size needed)
};

// What a walked stream gets with `cap` bytes of room: only a well-formed stream that fits is decoded.
SMC_HD inline StreamPlan stream_plan(const Walk& w, uint64_t cap) {
  StreamPlan p{w.status, 0, w.total};
  if (p.status == SM_OK && w.total > cap) p.status = SM_BUFFER_TOO_SMALL;
  if (p.status == SM_OK) p.slots = w.nchunks;
  return p;
}

// A slot's status: SM_OK for a slot no chunk took and for a stored chunk (the raw decoder's answer
// for its empty stand-in is ignored), else the raw decoder's.
SMC_HD inline int32_t slot_verdict(uint32_t stream, uint32_t copy_len, int32_t dec_status) {
  return stream == kNoSlot || copy_len != kNoCopy ? (int32_t)SM_OK : dec_status;
}

// A stream's status: SM_ERR_ARGUMENT over the caller's bound, else the plan's, else its first
// failing slot's raw decoder status (fail == kNoSlot: none failed).
SMC_HD inline int32_t stream_verdict(bool over, int32_t pre, uint32_t fail, int32_t fail_status) {
  if (over) return SM_ERR_ARGUMENT;
  if (pre != SM_OK) return pre;
  return fail != kNoSlot ? fail_status : (int32_t)SM_OK;
}

// The stream of slot j: first[r] <= j < first[r + 1] in the scan first[0, nstreams] (of equal
// entries the last one, so streams without slots are passed over).  j < first[nstreams].
SMC_HD inline uint32_t slot_stream(const uint32_t* first, uint32_t nstreams, uint32_t j) {
  uint32_t lo = 0, hi = nstreams;  // first[lo] <= j < first[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- the copies' grid -----------------------------------------------------------------------------
// A slot's bytes (a stored chunk on decode, a chunk's payload on compress) are copied in tiles of
// kCopyTile bytes, tile t by the workgroups of row t mod rows.  With many slots one row does (a
// workgroup a slot); with few, a long slot is spread over as many rows as fill the device
// (kCopyGroups workgroups), at most one per tile of the longest slot there can be.
constexpr uint32_t kCopyTile = 16384;
constexpr uint32_t kCopyGroups = 2048;  // 256 CUs x 8 workgroups

SMC_HD inline uint32_t copy_rows(uint32_t slots, uint32_t longest) {
  const uint32_t tiles = longest / kCopyTile + (longest % kCopyTile ? 1 : 0);
  const uint32_t want = slots ? kCopyGroups / slots : kCopyGroups;
  const uint32_t rows = tiles < want ? tiles : want;
  return rows ? rows : 1;
}

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct DecodeStreams {
  Header* hdr;
  // per slot (m = max_chunks): the two smm calls' arguments (offsets relative to d_in and d_out) and
  // results.  A stored chunk's slot has in_len 0 and cap 0 for them -- the raw decoder returns from
  // it at once -- and its payload's length in copy_len (else kNoCopy); a slot no chunk took has
  // in_len 0, cap 0, copy_len kNoCopy and stream kNoSlot
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *cap, *out_len, *stream, *copy_len;
  int32_t *dec_status, *index_status;
  uint32_t *frag_first, *frag_pos;  // m + 1, max(max_fragments, 1): the index smm_index_device builds
  uint8_t* built;
  // per stream
  uint64_t* length;
  uint32_t *count, *first, *fail;
  int32_t* pre;
  uintptr_t end;
};

inline DecodeStreams carve_decode_streams(uint8_t* buf, size_t nstreams, size_t m, size_t max_fragments) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  DecodeStreams s;
  s.hdr = c.take<Header>(1);
  s.in_off = c.take<uint64_t>(m);
  s.out_off = c.take<uint64_t>(m);
  s.in_len = c.take<uint32_t>(m);
  s.cap = c.take<uint32_t>(m);
  s.out_len = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.copy_len = c.take<uint32_t>(m);
  s.dec_status = c.take<int32_t>(m);
  s.index_status = c.take<int32_t>(m);
  s.frag_first = c.take<uint32_t>(m + 1);
  s.frag_pos = c.take<uint32_t>(max_fragments ? max_fragments : 1);
  s.built = c.take<uint8_t>(m);
  s.length = c.take<uint64_t>(nstreams);
  s.count = c.take<uint32_t>(nstreams);
  s.first = c.take<uint32_t>(nstreams + 1);
  s.fail = c.take<uint32_t>(nstreams);
  s.pre = c.take<int32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t decode_streams_bytes(size_t nstreams, size_t m, size_t max_fragments) {
  return (size_t)carve_decode_streams(nullptr, nstreams, m, max_fragments).end;
}

struct CompressStreams {
  Header* hdr;
  // per piece (m = max_pieces): smm_compress_device's arguments and results, and the choice
  uint64_t *in_off, *slot_off;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the chunk sizes over all pieces
  uint32_t *in_len, *comp_len, *stream;
  int32_t* comp_status;
  uint8_t* stored;  // 1: the chunk holds the piece itself
  // per stream
  uint32_t *first, *bad;
  uintptr_t end;
};

inline CompressStreams carve_compress_streams(uint8_t* buf, size_t nstreams, size_t m) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  CompressStreams s;
  s.hdr = c.take<Header>(1);
  s.in_off = c.take<uint64_t>(m);
  s.slot_off = c.take<uint64_t>(m);
  s.size_scan = c.take<uint64_t>(m + 1);
  s.in_len = c.take<uint32_t>(m);
  s.comp_len = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.comp_status = c.take<int32_t>(m);
  s.stored = c.take<uint8_t>(m);
  s.first = c.take<uint32_t>(nstreams + 1);
  s.bad = c.take<uint32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t compress_streams_bytes(size_t nstreams, size_t m) {
  return (size_t)carve_compress_streams(nullptr, nstreams, m).end;
}
// The raw compressor's output slots of a compress call: a piece's bound, rounded up to 256 bytes
// (the multi library's alignment of its own fragment slots).
SMC_HD inline uint64_t slot_pitch(uint32_t block_size) { return (smc::max_compressed_length(block_size) + 255) / 256 * 256; }
inline size_t compress_streams_slot_bytes(size_t m, uint32_t block_size) { return m * (size_t)slot_pitch(block_size); }

}  // namespace smo
