// smf_streams.h -- the rules of the batched stream calls (smf_uncompress_streams_device,
// smf_compress_streams_device), shared by their kernels (smf_streams.hip) and the host
// (smf_streams_plan in smf_host.cpp, which the sanitizer driver runs): the walk of one stream of a
// batch over walk_step, what a walked stream gets (its status, its slots, its length), and the
// scratch layouts.  Plain functions, compiled for the host and the device alike, so the host checker
// tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smf_format.h"
#include "smf_range.h"

namespace smf {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, chunks or blocks: SM_ERR_ARGUMENT

// One stream of n bytes, chunk by chunk (walk_step).  fetch(pos, have, h) brings the `have` bytes at
// pos into h -- the only access to the stream, so no byte at n or behind it is read, whatever lies
// there; entry(k, at, c) gets data chunk k, which starts at byte `at` of the stream's content.
template <typename Fetch, typename Entry>
SMC_HD inline Walk walk_stream(uint64_t n, Fetch fetch, Entry entry) {
  Walk w;
  uint64_t pos = 0;
  for (;;) {
    const uint32_t have = pos < n ? (uint32_t)(n - pos < kHeadBytes ? n - pos : kHeadBytes) : 0u;
    uint8_t h[kHeadBytes];
    fetch(pos, have, h);
    Chunk c;
    if (!walk_step(w, h, have, pos, n, c)) break;
    if (c.data) {
      entry(w.nchunks, w.total, c);
      ++w.nchunks;
      w.total += c.ulen;
    }
    pos = c.next;
  }
  return w;
}

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
struct StreamsHeader {  // the plan's words for the kernels behind it
  uint32_t total;       // slots in use (0 over the bound: nothing is decoded or packed)
  uint32_t over;        // the streams need more slots than the caller's bound
};

struct DecodeStreams {
  StreamsHeader* hdr;
  // per slot (m = max_chunks): the index entry, the raw decoder's arguments, the verdict
  smf_chunks ch;  // pay_off is relative to d_in
  uint64_t* out_off;  // relative to d_out
  uint32_t *cap, *dec_len, *dec_out_len, *crc_out, *stream;
  int32_t *dec_status, *slot_status;
  // per stream
  uint32_t *count, *first, *fail;
  int32_t* pre;
  uint64_t* length;
  uintptr_t end;
};

inline DecodeStreams carve_decode_streams(uint8_t* buf, size_t nstreams, size_t m) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  DecodeStreams s;
  s.hdr = c.take<StreamsHeader>(1);
  s.ch.pay_off = c.take<uint64_t>(m);
  s.out_off = c.take<uint64_t>(m);
  s.ch.pay_len = c.take<uint32_t>(m);
  s.ch.crc = c.take<uint32_t>(m);
  s.ch.ulen = c.take<uint32_t>(m);
  s.cap = c.take<uint32_t>(m);
  s.dec_len = c.take<uint32_t>(m);
  s.dec_out_len = c.take<uint32_t>(m);
  s.crc_out = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.dec_status = c.take<int32_t>(m);
  s.slot_status = c.take<int32_t>(m);
  s.ch.type = c.take<uint8_t>(m);
  s.length = c.take<uint64_t>(nstreams);
  s.count = c.take<uint32_t>(nstreams);
  s.first = c.take<uint32_t>(nstreams + 1);
  s.fail = c.take<uint32_t>(nstreams);
  s.pre = c.take<int32_t>(nstreams);
  s.end = c.p;
  return s;
}
inline size_t decode_streams_bytes(size_t nstreams, size_t m) {
  return (size_t)carve_decode_streams(nullptr, nstreams, m).end;
}

struct CompressStreams {
  StreamsHeader* hdr;
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
  s.hdr = c.take<StreamsHeader>(1);
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
