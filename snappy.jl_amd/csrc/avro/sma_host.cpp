// sma_host.cpp -- the host-only part of the Avro container library
// (include/snappy_mi355x_avro.h): the walk over a host buffer, the size helpers, the host plan of
// the batched decode, the sync search's host twin and the header writer.  No HIP and no call into
// the other libraries, so this file also builds alone (the sanitizer driver, sma_host_check.cpp).
#include <string.h>

#include "sma_format.h"
#include "sma_streams.h"

namespace sma {

const char* host_message(sm_status st) {
  switch (st) {
    case SMA_ERR_NO_HEADER: return "Avro file does not start with the object container magic.";
    case SMA_ERR_BAD_HEADER: return "Avro file: corrupt metadata map in the header.";
    case SMA_ERR_TRUNCATED: return "Avro file: truncated long, header, block or sync marker.";
    case SMA_ERR_VARLONG: return "Avro file: a long of more than 64 bits.";
    case SMA_ERR_CODEC: return "Avro file: avro.codec is missing or is not snappy.";
    case SMA_ERR_BLOCK: return "Avro file: a block with a negative count or an impossible size.";
    case SMA_ERR_TOO_LARGE: return "Avro file: a block of more than 2147483647 bytes.";
    case SMA_ERR_SYNC: return "Avro file: a block is not followed by the sync marker.";
    case SMA_ERR_CRC: return "Avro file: a block's CRC-32 does not match its uncompressed bytes.";
    default: return nullptr;
  }
}

namespace {

// appends to a buffer of `cap` bytes, counting on when it is full or absent
struct Writer {
  uint8_t* out;
  size_t cap, n = 0;
  void byte(uint8_t b) {
    if (out && n < cap) out[n] = b;
    ++n;
  }
  void bytes(const uint8_t* p, size_t len) {
    if (out && n <= cap && len <= cap - n && len) memcpy(out + n, p, len);
    n += len;
  }
  void put_long(int64_t v) {
    const uint32_t nb = long_len(v);
    for (uint32_t i = 0; i < nb; ++i) byte(long_byte(v, i, nb));
  }
  void text(const char* s) {
    const size_t len = strlen(s);
    put_long((int64_t)len);
    bytes((const uint8_t*)s, len);
  }
};

}  // namespace

}  // namespace sma

extern "C" {

uint64_t sma_max_blocks(uint64_t n) { return n / sma::kMinBlock; }

uint64_t sma_max_block_length(uint64_t len) { return sma::max_block_length(len); }

uint64_t sma_stage_length(uint64_t len) { return sma::stage_length(len); }

sm_status sma_index(const uint8_t* buf, size_t n, int kind, const uint8_t* sync, const sma_blocks* blocks,
                    uint32_t max_blocks, sma_summary* summary) {
  if (!summary || (!buf && n) || !sma::valid_kind(kind) || (kind == SMA_INPUT_BLOCKS && !sync)) return SM_ERR_ARGUMENT;
  if (blocks && max_blocks && !sma::valid_blocks(*blocks)) return SM_ERR_ARGUMENT;
  sma::ByteFetch fetch{buf};
  const sma::Walk w = sma::walk_stream(kind, n, fetch, sync, [&](uint32_t k, uint64_t at, const sma::Block& b) {
    if (!blocks || k >= max_blocks) return;
    blocks->pay_off[k] = b.pay_off;
    blocks->pay_len[k] = b.pay_len;
    blocks->ulen[k] = b.ulen;
    blocks->count[k] = b.count;
    blocks->crc[k] = b.crc;
    blocks->out_off[k] = at;
  });
  summary->total_length = w.total;
  summary->nblocks = w.nblocks;
  summary->status = sma::walk_status(w, blocks != nullptr, max_blocks);
  summary->objects = w.objects;
  summary->header_length = w.header_len;
  memcpy(summary->sync, w.sync, sma::kSync);
  return summary->status;
}

sm_status sma_uncompressed_length(const uint8_t* buf, size_t n, int kind, const uint8_t* sync, size_t* result) {
  sma_summary s;
  const sm_status st = sma_index(buf, n, kind, sync, nullptr, 0, &s);
  if (st == SM_OK && result) *result = (size_t)s.total_length;
  return st;
}

size_t sma_streams_scratch_bytes(uint32_t nstreams, uint32_t max_blocks, uint32_t max_fragments, uint64_t stage_bytes) {
  const size_t decode = sma::decode_streams_bytes(nstreams, max_blocks, max_fragments);
  const size_t compress = sma::compress_streams_bytes(nstreams, max_blocks, (size_t)stage_bytes + 64);
  return decode > compress ? decode : compress;
}

// the device's decode plan, stream by stream (sma_streams.h)
sm_status sma_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams, int kind,
                           const uint8_t* sync, const uint64_t* out_cap, uint32_t max_blocks, uint32_t* first,
                           uint64_t* out_len, int32_t* status, uint64_t* objects, uint64_t* total_blocks,
                           uint64_t* total_fragments) {
  if (nstreams > sma::kMaxStreams || max_blocks > sma::kMaxStreams || !sma::valid_kind(kind)) return SM_ERR_ARGUMENT;
  if (nstreams && (!in_off || !in_len || (kind == SMA_INPUT_BLOCKS && !sync))) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nstreams; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0, fragments = 0;
  for (uint32_t r = 0; r < nstreams; ++r) {
    sma::ByteFetch fetch{in_len[r] ? in + in_off[r] : nullptr};
    uint64_t frags = 0;  // of this stream's blocks, should it be decoded
    const sma::Walk w = sma::walk_stream(kind, in_len[r], fetch, sync ? sync + (size_t)sma::kSync * r : nullptr,
                                         [&](uint32_t, uint64_t, const sma::Block& b) { frags += sma::decode_fragments(b.ulen); });
    const sma::StreamPlan sp = sma::stream_plan(w, out_cap ? out_cap[r] : UINT64_MAX);
    if (first) first[r] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    if (out_len) out_len[r] = sp.length;
    if (status) status[r] = sp.status;
    if (objects) objects[r] = sp.objects;
    sum += sp.slots;
    if (sp.status == SM_OK) fragments += frags;
  }
  if (first) first[nstreams] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  if (total_blocks) *total_blocks = sum;
  if (total_fragments) *total_fragments = fragments;
  if (sum <= max_blocks) return SM_OK;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status) status[r] = SM_ERR_ARGUMENT;
    if (out_len) out_len[r] = 0;
    if (objects) objects[r] = 0;
  }
  return SM_BUFFER_TOO_SMALL;
}

sm_status sma_find_sync(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint8_t* sync,
                        uint32_t nstreams, const uint32_t* q_stream, const uint64_t* q_from, uint32_t nqueries,
                        uint64_t* pos) {
  if (nstreams > sma::kMaxStreams || nqueries > sma::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nqueries == 0) return SM_OK;
  if (nstreams == 0 || !in_off || !in_len || !sync || !q_stream || !q_from || !pos) return SM_ERR_ARGUMENT;
  for (uint32_t i = 0; i < nqueries; ++i)
    if (q_stream[i] >= nstreams || (in_len[q_stream[i]] && !in)) return SM_ERR_ARGUMENT;
  for (uint32_t i = 0; i < nqueries; ++i) {
    const uint32_t r = q_stream[i];
    pos[i] = sma::find_sync_host(in_len[r] ? in + in_off[r] : nullptr, in_len[r], sync + (size_t)sma::kSync * r, q_from[i]);
  }
  return SM_OK;
}

sm_status sma_write_header(const uint8_t* schema, size_t schema_len, const uint8_t* extra, const uint64_t* extra_off,
                           uint32_t npairs, const uint8_t* sync, uint8_t* out, size_t out_cap, size_t* out_len) {
  if ((!schema && schema_len) || !sync || !out_len || (npairs && (!extra_off || !extra))) return SM_ERR_ARGUMENT;
  for (uint32_t i = 0; i < 2 * npairs; ++i)
    if (extra_off[i] > extra_off[i + 1]) return SM_ERR_ARGUMENT;
  sma::Writer w{out, out_cap};
  const uint8_t magic[4] = {0x4f, 0x62, 0x6a, 0x01};
  w.bytes(magic, 4);
  w.put_long(2 + (int64_t)npairs);
  w.text("avro.schema");
  w.put_long((int64_t)schema_len);
  w.bytes(schema, schema_len);
  w.text("avro.codec");
  w.text("snappy");
  for (uint32_t i = 0; i < 2 * npairs; ++i) {
    const uint64_t len = extra_off[i + 1] - extra_off[i];
    w.put_long((int64_t)len);
    w.bytes(extra + extra_off[i], (size_t)len);
  }
  w.put_long(0);
  w.bytes(sync, sma::kSync);
  *out_len = w.n;
  return out && w.n > out_cap ? (sm_status)SM_BUFFER_TOO_SMALL : (sm_status)SM_OK;
}

}  // extern "C"
