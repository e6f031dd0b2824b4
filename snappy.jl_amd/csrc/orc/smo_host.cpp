// smo_host.cpp -- the host-only part of the ORC library (include/snappy_mi355x_orc.h): the walk over
// a host buffer, the size helpers and the host plan of the batched decode.  No HIP and no call into
// the other libraries, so this file also builds alone (the sanitizer driver, smo_host_check.cpp).
#include "smo_format.h"
#include "smo_streams.h"

namespace smo {

const char* host_message(sm_status st) {
  switch (st) {
    case SMO_ERR_TRUNCATED: return "ORC stream: truncated chunk header or chunk.";
    case SMO_ERR_CHUNK_TOO_LARGE: return "ORC stream: a chunk declares more bytes than the compression block size.";
    default: return nullptr;
  }
}

}  // namespace smo

extern "C" {

size_t smo_max_length(size_t n, uint32_t block_size) {
  return smo::valid_block_size(block_size) ? (size_t)smo::max_length(n, block_size) : 0;
}

uint64_t smo_max_chunks(uint64_t n) { return n / SMO_HEADER_LENGTH; }

sm_status smo_index(const uint8_t* buf, size_t n, uint32_t block_size, const smo_chunks* chunks, uint32_t max_chunks,
                    smo_summary* summary) {
  if (!summary || (!buf && n) || !smo::valid_block_size(block_size)) return SM_ERR_ARGUMENT;
  if (chunks && max_chunks && (!chunks->pay_off || !chunks->pay_len || !chunks->ulen || !chunks->original))
    return SM_ERR_ARGUMENT;
  const smo::Walk w = smo::walk_chunks(block_size, n, smo::ByteFetch{buf}, [&](uint32_t k, uint64_t, const smo::Chunk& c) {
    if (!chunks || k >= max_chunks) return;
    chunks->pay_off[k] = c.pay_off;
    chunks->pay_len[k] = c.pay_len;
    chunks->ulen[k] = c.ulen;
    chunks->original[k] = c.original ? 1 : 0;
  });
  summary->total_length = w.total;
  summary->nchunks = w.nchunks;
  summary->status = smo::walk_status(w, chunks != nullptr, max_chunks);
  return summary->status;
}

sm_status smo_uncompressed_length(const uint8_t* buf, size_t n, uint32_t block_size, size_t* result) {
  smo_summary s;
  const sm_status st = smo_index(buf, n, block_size, nullptr, 0, &s);
  if (st == SM_OK && result) *result = (size_t)s.total_length;
  return st;
}

size_t smo_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots, uint32_t max_fragments, uint32_t block_size) {
  const size_t decode = smo::decode_streams_bytes(nstreams, max_slots, max_fragments);
  const size_t compress = smo::compress_streams_bytes(nstreams, max_slots) +
                          (smo::valid_block_size(block_size) ? smo::compress_streams_slot_bytes(max_slots, block_size) : 0);
  return decode > compress ? decode : compress;
}

// the device's decode plan, stream by stream (smo_streams.h)
sm_status smo_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           uint32_t block_size, const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first,
                           uint64_t* out_len, int32_t* status, uint64_t* total_chunks, uint64_t* total_fragments) {
  if (nstreams > smo::kMaxStreams || max_chunks > smo::kMaxStreams || !smo::valid_block_size(block_size))
    return SM_ERR_ARGUMENT;
  if (nstreams && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nstreams; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0, fragments = 0;
  for (uint32_t r = 0; r < nstreams; ++r) {
    const uint8_t* const p = in_len[r] ? in + in_off[r] : nullptr;
    uint64_t frags = 0;  // of this stream's compressed chunks, should it be decoded
    const smo::Walk w = smo::walk_chunks(block_size, in_len[r], smo::ByteFetch{p}, [&](uint32_t, uint64_t, const smo::Chunk& c) {
      if (!c.original) frags += smo::fragments(c.ulen);
    });
    const smo::StreamPlan sp = smo::stream_plan(w, out_cap ? out_cap[r] : UINT64_MAX);
    if (first) first[r] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    if (out_len) out_len[r] = sp.length;
    if (status) status[r] = sp.status;
    sum += sp.slots;
    if (sp.status == SM_OK) fragments += frags;
  }
  if (first) first[nstreams] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  if (total_chunks) *total_chunks = sum;
  if (total_fragments) *total_fragments = fragments;
  if (sum <= max_chunks) return SM_OK;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status) status[r] = SM_ERR_ARGUMENT;
    if (out_len) out_len[r] = 0;
  }
  return SM_BUFFER_TOO_SMALL;
}

}  // extern "C"
