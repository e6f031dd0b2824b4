// sma_streams.h -- the rules of the batched calls (sma_uncompress_streams_device,
// sma_compress_streams_device), shared by their kernels (sma_kernels.hip) and the host
// (sma_streams_plan in sma_host.cpp, which the sanitizer driver runs): what a walked stream of a
// batch gets, a slot's verdict and the scratch layouts (the shared slot rules are
// ../common/smc_slots.h's).  The walk itself is walk_stream (sma_format.h).  Plain functions, compiled for the host and the device alike, so the
// host checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common/smc_slots.h"
#include "sma_format.h"

namespace sma {

constexpr uint32_t kMaxStreams = 0x7fffffffu;  // more streams, blocks or queries: SM_ERR_ARGUMENT
using smc::kNoSlot;                            // a slot of no stream; a stream without a failing slot
constexpr uint32_t kSearchTile = 65536;        // the sync search's tile: candidates, by their first byte

using Header = smc::PlanHeader;  // (over: the streams need more than one of the caller's bounds)

struct StreamPlan {
  int32_t status;   // the walk's error, SM_BUFFER_TOO_SMALL, or SM_OK: what is known before any decode
  uint32_t slots;   // its blocks when it is decoded, else 0
  uint64_t length;  // the declared lengths: before the error, else of the whole stream (the size needed)
  uint64_t objects;
};

// What a walked stream gets with `cap` bytes of room: only a well-formed stream that fits is decoded.
SMC_HD inline StreamPlan stream_plan(const Walk& w, uint64_t cap) {
  StreamPlan p{w.status, 0, w.total, w.objects};
  if (p.status == SM_OK && w.total > cap) p.status = SM_BUFFER_TOO_SMALL;
  if (p.status == SM_OK) p.slots = w.nblocks;
  return p;
}

// A slot's status: the raw decoder's when it failed -- the checksum covers the output, so only a
// block that decoded is held against it -- else SMA_ERR_CRC where the checksums differ.
SMC_HD inline int32_t slot_verdict(int32_t dec_status, bool verify, uint32_t stored, uint32_t computed) {
  if (dec_status != SM_OK) return dec_status;
  return verify && stored != computed ? (int32_t)SMA_ERR_CRC : (int32_t)SM_OK;
}

// (A stream's status is smc::plan_verdict over its first failing slot's status; the stream of a
// slot is its smc::slot_owner in the scan first[0, nstreams].)

// an encoded block whose raw stream is there and within its bound
SMC_HD inline bool block_ok(int32_t comp_status, uint32_t comp_len, uint32_t in_len) {
  return comp_status == SM_OK && comp_len != 0 && comp_len <= smc::max_compressed_length(in_len);
}

inline bool valid_blocks(const sma_blocks& b) {
  return b.pay_off && b.pay_len && b.ulen && b.count && b.crc && b.out_off;
}

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct DecodeStreams {
  Header* hdr;
  // per slot (m = max_blocks): the two smm calls' and the CRC call's arguments (offsets relative to
  // d_in and d_out) and results; a slot no block took has in_len 0, cap 0 and stream kNoSlot
  uint64_t *in_off, *out_off, *crc_len;
  uint32_t *in_len, *cap, *out_len, *stream, *stored, *computed;
  int32_t *dec_status, *index_status, *slot_status;
  uint32_t *frag_first, *frag_pos;  // m + 1, max(max_fragments, 1): the index smm_index_device builds
  uint8_t* built;
  // per stream
  uint64_t *length, *objects;
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
  s.crc_len = c.take<uint64_t>(m);
  s.in_len = c.take<uint32_t>(m);
  s.cap = c.take<uint32_t>(m);
  s.out_len = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.stored = c.take<uint32_t>(m);
  s.computed = c.take<uint32_t>(m);
  s.dec_status = c.take<int32_t>(m);
  s.index_status = c.take<int32_t>(m);
  s.slot_status = c.take<int32_t>(m);
  s.frag_first = c.take<uint32_t>(m + 1);
  s.frag_pos = c.take<uint32_t>(max_fragments ? max_fragments : 1);
  s.built = c.take<uint8_t>(m);
  s.length = c.take<uint64_t>(nstreams);
  s.objects = c.take<uint64_t>(nstreams);
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
  // per block (m = max_blocks): smm_compress_device's and smq_crc32_device's arguments and results
  uint64_t *in_off, *slot_off, *crc_len, *count;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the block sizes over all blocks
  uint32_t *in_len, *comp_len, *stream, *crc;
  int32_t* comp_status;
  // per stream
  uint32_t* fail;
  uint8_t* stage;  // stage_bytes: the raw compressor's output
  uintptr_t end;
};

inline CompressStreams carve_compress_streams(uint8_t* buf, size_t nstreams, size_t m, size_t stage_bytes) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  CompressStreams s;
  s.hdr = c.take<Header>(1);
  s.in_off = c.take<uint64_t>(m);
  s.slot_off = c.take<uint64_t>(m);
  s.crc_len = c.take<uint64_t>(m);
  s.count = c.take<uint64_t>(m);
  s.size_scan = c.take<uint64_t>(m + 1);
  s.in_len = c.take<uint32_t>(m);
  s.comp_len = c.take<uint32_t>(m);
  s.stream = c.take<uint32_t>(m);
  s.crc = c.take<uint32_t>(m);
  s.comp_status = c.take<int32_t>(m);
  s.fail = c.take<uint32_t>(nstreams);
  s.stage = c.take<uint8_t>(stage_bytes ? stage_bytes : 1);
  s.end = c.p;
  return s;
}
inline size_t compress_streams_bytes(size_t nstreams, size_t m, size_t stage_bytes) {
  return (size_t)carve_compress_streams(nullptr, nstreams, m, stage_bytes).end;
}

}  // namespace sma
