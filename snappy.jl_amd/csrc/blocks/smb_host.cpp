// smb_host.cpp -- the host-only part of the blocks library (include/snappy_mi355x_blocks.h): the
// walk over a host buffer, the size helpers and the host plan of the batched decode.  No HIP and no
// call into the other libraries, so this file also builds alone (the sanitizer driver,
// smb_host_check.cpp).
#include "smb_format.h"
#include "smb_streams.h"

namespace smb {

const char* host_message(sm_status st) {
  switch (st) {
    case SMB_ERR_NO_HEADER: return "Block stream does not start with the snappy-java header.";
    case SMB_ERR_BAD_HEADER: return "Block stream: corrupt snappy-java header.";
    case SMB_ERR_TRUNCATED: return "Block stream: truncated length field, header or chunk.";
    case SMB_ERR_CHUNK_TOO_LARGE: return "Block stream: block or chunk of more than 2147483647 uncompressed bytes.";
    case SMB_ERR_BLOCK_LENGTH: return "Block stream: a block's chunks declare more bytes than the block.";
    default: return nullptr;
  }
}

}  // namespace smb

extern "C" {

size_t smb_max_length(size_t n, int format) { return (size_t)smb::max_length(n, format); }

uint64_t smb_max_chunks(uint64_t n, int format) {
  const uint64_t fixed = smb::stream_prefix(format);
  return n < fixed ? 0 : (n - fixed) / 5;
}

sm_status smb_index(const uint8_t* buf, size_t n, int format, const smb_chunks* chunks, uint32_t max_chunks,
                    smb_summary* summary) {
  if (!summary || (!buf && n) || !smb::valid_format(format)) return SM_ERR_ARGUMENT;
  if (chunks && max_chunks && (!chunks->pay_off || !chunks->pay_len || !chunks->ulen)) return SM_ERR_ARGUMENT;
  const smb::Walk w = smb::walk_blocks(format, n, smb::ByteFetch{buf}, [&](uint32_t k, uint64_t, const smb::Chunk& c) {
    if (!chunks || k >= max_chunks) return;
    chunks->pay_off[k] = c.pay_off;
    chunks->pay_len[k] = c.pay_len;
    chunks->ulen[k] = c.ulen;
  });
  summary->total_length = w.total;
  summary->nchunks = w.nchunks;
  summary->status = smb::walk_status(w, chunks != nullptr, max_chunks);
  return summary->status;
}

sm_status smb_uncompressed_length(const uint8_t* buf, size_t n, int format, size_t* result) {
  smb_summary s;
  const sm_status st = smb_index(buf, n, format, nullptr, 0, &s);
  if (st == SM_OK && result) *result = (size_t)s.total_length;
  return st;
}

size_t smb_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots, uint32_t max_fragments) {
  const size_t decode = smb::decode_streams_bytes(nstreams, max_slots, max_fragments);
  const size_t compress = smb::compress_streams_bytes(nstreams, max_slots) + smb::compress_streams_slot_bytes(max_slots);
  return decode > compress ? decode : compress;
}

// the device's decode plan, stream by stream (smb_streams.h)
sm_status smb_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           int format, const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first, uint64_t* out_len,
                           int32_t* status, uint64_t* total_chunks, uint64_t* total_fragments) {
  if (nstreams > smb::kMaxStreams || max_chunks > smb::kMaxStreams || !smb::valid_format(format)) return SM_ERR_ARGUMENT;
  if (nstreams && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nstreams; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0, fragments = 0;
  for (uint32_t r = 0; r < nstreams; ++r) {
    const uint8_t* const p = in_len[r] ? in + in_off[r] : nullptr;
    uint64_t frags = 0;  // of this stream's chunks, should it be decoded
    const smb::Walk w = smb::walk_blocks(format, in_len[r], smb::ByteFetch{p},
                                         [&](uint32_t, uint64_t, const smb::Chunk& c) { frags += smb::stream_blocks(c.ulen); });
    const smb::StreamPlan sp = smb::stream_plan(w, out_cap ? out_cap[r] : UINT64_MAX);
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
