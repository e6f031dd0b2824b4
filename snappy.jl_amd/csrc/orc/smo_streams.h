// smo_streams.h -- the rules of the batched calls (smo_uncompress_streams_device,
// smo_compress_streams_device), shared by their kernels (smo_kernels.hip) and the host
// (smo_streams_plan in smo_host.cpp, which the sanitizer driver runs): what a walked stream of a
// batch gets, a slot's verdict and the scratch layouts (the shared slot rules are ../common/smc_slots.h's).
// The walk itself is walk_chunks (smo_format.h).  Plain functions, compiled for the host and the
// device alike, so the host checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common/smc_slots.h"
#include "smo_format.h"

namespace smo {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, chunks or pieces: SM_ERR_ARGUMENT
using smc::kNoSlot;                            // a slot of no stream; a stream without a failing slot
constexpr uint32_t kNoCopy = 0xffffffffu;      // a slot's copy length when its chunk is not a stored one

using Header = smc::PlanHeader;

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

// (A stream's status is smc::plan_verdict over its first failing slot's raw decoder status; the
// stream of a slot is its smc::slot_owner in the scan first[0, nstreams]; the copies of the stored
// chunks and of the packed payloads are tiled by smc::copy_rows for slots of block_size bytes.)

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
