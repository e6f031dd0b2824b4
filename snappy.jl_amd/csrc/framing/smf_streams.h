// smf_streams.h -- the rules of the batched stream calls (smf_uncompress_streams_device,
// smf_compress_streams_device), shared by their kernels (smf_streams.hip) and the host
// (smf_streams_plan in smf_host.cpp, which the sanitizer driver runs): what a walked stream of a
// batch gets (its status, its slots, its length), and the scratch layouts.  The walk itself is
// walk_stream (smf_format.h).  Plain functions, compiled for the host and the device alike, so the
// host checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smf_format.h"
#include "smf_range.h"
#include "smf_slots.h"

namespace smf {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, chunks or blocks: SM_ERR_ARGUMENT

struct StreamPlan {
  int32_t status;  // the walk's error, SM_BUFFER_TOO_SMALL, or SM_OK: what is known before any decode
  uint32_t slots;  // its data chunks when it is decoded, else 0
  uint64_t length; // the declared lengths: before the error, else of the whole stream (the size needed)
};

// What a walked stream gets with `cap` bytes of room: only a well-formed stream that fits is decoded.
SMC_HD inline StreamPlan stream_plan(const Walk& w, uint64_t cap) {
  StreamPlan p{w.status, 0, w.total};
  if (p.status == SM_OK && w.total > cap) p.status = SM_BUFFER_TOO_SMALL;
  if (p.status == SM_OK) p.slots = w.nchunks;
  return p;
}

// blocks of an n-byte input (the encoder rule: 64 KiB each)
SMC_HD inline uint64_t stream_blocks(uint64_t n) { return n / kBlock + (n % kBlock ? 1 : 0); }

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct DecodeStreams {
  GroupHeader* hdr;
  // per slot (m = max_chunks): the walked entry (in_off is relative to d_in), the raw decoder's
  // arguments (out_off is relative to d_out), the verdict; a slot's group is its stream
  Slots slots;
  // per stream
  uint32_t *count, *first;
  int32_t* pre;
  uint64_t* length;
  uintptr_t end;
};

inline DecodeStreams carve_decode_streams(uint8_t* buf, size_t nstreams, size_t m) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  DecodeStreams s;
  s.hdr = c.take<GroupHeader>(1);
  s.slots = carve_slots(c, m, nstreams, true, false, true);
  s.length = c.take<uint64_t>(nstreams);
  s.count = c.take<uint32_t>(nstreams);
  s.first = c.take<uint32_t>(nstreams + 1);
  s.pre = c.take<int32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t decode_streams_bytes(size_t nstreams, size_t m) {
  return (size_t)carve_decode_streams(nullptr, nstreams, m).end;
}

struct CompressStreams {
  GroupHeader* hdr;
  // per block (m = max_blocks)
  uint64_t *in_off, *slot_off;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the chunk sizes over all blocks
  uint32_t *in_len, *comp_len, *crc, *stream;
  uint8_t* type;
  // per stream
  uint32_t *first, *bad;
  uintptr_t end;
};

inline CompressStreams carve_compress_streams(uint8_t* buf, size_t nstreams, size_t m) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  CompressStreams s;
  s.hdr = c.take<GroupHeader>(1);
  s.in_off = c.take<uint64_t>(m);
  s.slot_off = c.take<uint64_t>(m);
  s.size_scan = c.take<uint64_t>(m + 1);
  s.in_len = c.take<uint32_t>(m);
  s.comp_len = c.take<uint32_t>(m);
  s.crc = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.type = c.take<uint8_t>(m);
  s.first = c.take<uint32_t>(nstreams + 1);
  s.bad = c.take<uint32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t compress_streams_bytes(size_t nstreams, size_t m) {
  return (size_t)carve_compress_streams(nullptr, nstreams, m).end;
}
// the raw compressor's output slots of a compress call
inline size_t compress_streams_slot_bytes(size_t m) { return m * (size_t)smc::kFramingSlotPitch; }

}  // namespace smf
