// smb_streams.h -- the rules of the batched calls (smb_uncompress_streams_device,
// smb_compress_streams_device), shared by their kernels (smb_kernels.hip) and the host
// (smb_streams_plan in smb_host.cpp, which the sanitizer driver runs): what a walked stream of a
// batch gets and the scratch layouts (the slot rules are ../common/smc_slots.h's).  The walk itself is
// walk_blocks (smb_format.h).  Plain functions, compiled for the host and the device alike, so the
// host checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common/smc_slots.h"
#include "smb_format.h"

namespace smb {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, chunks or blocks: SM_ERR_ARGUMENT
using smc::kNoSlot;                            // a slot of no stream; a stream without a failing slot
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

// (A stream's status is smc::plan_verdict over its first failing slot's raw decoder status; the
// stream of a slot is its smc::slot_owner in the scan first[0, nstreams].)

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct DecodeStreams {
  Header* hdr;
  // per slot (m = max_chunks): the two smm calls' arguments (offsets relative to d_in and d_out) and
  // results; a slot no chunk took has in_len 0, cap 0 and stream kNoSlot
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *cap, *out_len, *stream;
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
  // per piece (m = max_blocks): smm_compress_device's arguments and results
  uint64_t *in_off, *slot_off;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the chunk sizes over all pieces
  uint32_t *in_len, *comp_len, *stream;
  int32_t* comp_status;
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
  s.first = c.take<uint32_t>(nstreams + 1);
  s.bad = c.take<uint32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t compress_streams_bytes(size_t nstreams, size_t m) {
  return (size_t)carve_compress_streams(nullptr, nstreams, m).end;
}
// The raw compressor's output slots of a compress call: a piece's bound, rounded up to 16 bytes
// (the framing library's pitch: the same pieces through the same kind of pack).
constexpr uint64_t kSlotPitch = smc::kFramingSlotPitch;
inline size_t compress_streams_slot_bytes(size_t m) { return m * (size_t)kSlotPitch; }

}  // namespace smb
