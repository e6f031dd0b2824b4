// smf_host.cpp -- the host-only part of the framing library (include/snappy_mi355x_framing.h):
// the chunk walker over a host buffer, the bytewise CRC-32C, the size helpers and the host plans of
// the ranged and the batched decode.  No HIP and no
// call into the raw codec, so this file also builds alone (the sanitizer driver, smf_host_check.cpp).
#include "smf_format.h"
#include "smf_range.h"
#include "smf_streams.h"

namespace {

struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t b = 0; b < 256; ++b) {
      uint32_t c = b;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? smf::kPoly : 0u);
      t[b] = c;
    }
  }
};

const CrcTable& crc_table() {
  static const CrcTable tab;
  return tab;
}

}  // namespace

namespace smf {

// T_k[b]: byte b followed by k zero bytes (the slicing tables; T_0 is the bytewise table).
// tab[i] = T_(15-i): a granule's byte i has 15-i bytes behind it.  tab[16+j] = T_(N-1-j), N =
// 16 kCrcThreads: a register's byte j stands in for byte j of the N bytes that follow it.
void build_crc_lut(CrcLut* T) {
  const uint32_t* t0 = crc_table().t;
  const uint32_t N = 16 * kCrcThreads;
  uint32_t cur[256];
  for (uint32_t b = 0; b < 256; ++b) cur[b] = t0[b];
  for (uint32_t k = 0; k < N; ++k) {
    if (k < 16)
      for (uint32_t b = 0; b < 256; ++b) T->tab[15 - k][b] = cur[b];
    if (k >= N - 4)
      for (uint32_t b = 0; b < 256; ++b) T->tab[16 + (N - 1 - k)][b] = cur[b];
    for (uint32_t b = 0; b < 256; ++b) cur[b] = (cur[b] >> 8) ^ t0[cur[b] & 0xff];
  }
  uint32_t x128 = 0x40000000u;  // x
  for (int i = 0; i < 7; ++i) x128 = gf_mul(x128, x128);
  T->xpow[0] = 0x80000000u;  // 1
  for (uint32_t g = 0; g < kCrcPow; ++g) T->xpow[g + 1] = gf_mul(T->xpow[g], x128);
  T->xpow2[0] = x128;
  for (uint32_t k = 0; k + 1 < 32; ++k) T->xpow2[k + 1] = gf_mul(T->xpow2[k], T->xpow2[k]);
}

const char* host_message(sm_status st) {
  switch (st) {
    case SMF_ERR_NO_IDENTIFIER: return "Framed stream does not start with a stream identifier.";
    case SMF_ERR_BAD_IDENTIFIER: return "Framed stream: corrupt stream identifier.";
    case SMF_ERR_RESERVED_CHUNK: return "Framed stream: unskippable reserved chunk type.";
    case SMF_ERR_TRUNCATED: return "Framed stream: truncated chunk.";
    case SMF_ERR_CHUNK_TOO_LARGE: return "Framed stream: chunk of more than 65536 uncompressed bytes.";
    case SMF_ERR_CRC: return "Framed stream: CRC-32C mismatch.";
    default: return nullptr;
  }
}

}  // namespace smf

extern "C" {

size_t smf_max_framed_length(size_t n) { return 10 + 8 * ((n + 65535) / 65536) + n; }

uint32_t smf_crc32c(const void* buf, size_t n) {
  const uint32_t* t = crc_table().t;
  const uint8_t* p = (const uint8_t*)buf;
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

uint32_t smf_crc32c_mask(uint32_t crc) { return smf::mask(crc); }

sm_status smf_index(const uint8_t* buf, size_t n, const smf_chunks* chunks, uint32_t max_chunks,
                    smf_summary* summary) {
  if (!summary || (!buf && n)) return SM_ERR_ARGUMENT;
  if (chunks && max_chunks && !smf::valid_chunks(*chunks)) return SM_ERR_ARGUMENT;
  const smf::Walk w = smf::walk_stream(n, smf::ByteFetch{buf}, [&](uint32_t k, uint64_t, const smf::Chunk& c) {
    if (chunks && k < max_chunks) smf::store_chunk(*chunks, k, c);
  });
  summary->total_length = w.total;
  summary->nchunks = w.nchunks;
  summary->status = smf::walk_status(w, chunks != nullptr, max_chunks);
  return summary->status;
}

sm_status smf_uncompressed_length(const uint8_t* buf, size_t n, size_t* result) {
  smf_summary s;
  const sm_status st = smf_index(buf, n, nullptr, 0, &s);
  if (st == SM_OK && result) *result = (size_t)s.total_length;
  return st;
}

sm_status smf_chunk_offsets(const uint32_t* ulen, uint32_t nchunks, uint64_t* chunk_off) {
  if (!chunk_off || (nchunks && !ulen)) return SM_ERR_ARGUMENT;
  uint64_t at = 0;
  for (uint32_t c = 0; c < nchunks; ++c) {
    chunk_off[c] = at;
    at += ulen[c];
  }
  chunk_off[nchunks] = at;
  return SM_OK;
}

uint64_t smf_range_chunk_count(uint64_t lo, uint64_t len) {
  if (len == 0 || lo + len < lo) return 0;
  return (lo + len - 1) / smf::kBlock - lo / smf::kBlock + 1;
}

// the device's plan, range by range and slot by slot (smf_range.h)
sm_status smf_range_plan(const smf_chunks* chunks, const uint64_t* chunk_off, uint32_t nchunks, uint64_t n,
                         const uint64_t* lo, const uint64_t* len, uint32_t nranges, uint32_t max_range_chunks,
                         uint32_t* first, uint32_t* count, int32_t* status, uint64_t* total) {
  if (!chunk_off || nchunks > smf::kMaxIndexChunks || nranges > smf::kMaxIndexChunks) return SM_ERR_ARGUMENT;
  if (nranges && (!lo || !len)) return SM_ERR_ARGUMENT;
  smf_chunks ch;
  if (!smf::take_chunks(chunks, nchunks, ch)) return SM_ERR_ARGUMENT;
  uint64_t sum = 0;
  for (uint32_t r = 0; r < nranges; ++r) {
    const smf::RangeChunks rc = smf::range_chunks(chunk_off, nchunks, lo[r], len[r]);
    int32_t st = rc.status;
    for (uint32_t k = 0; k < rc.count && st == SM_OK; ++k) {
      bool skip;
      st = smf::slot_place(ch, chunk_off, n, rc.first + k, lo[r], len[r], k == 0, k == rc.count - 1, skip).status;
    }
    if (first) first[r] = rc.first;
    if (count) count[r] = rc.count;
    if (status) status[r] = st;
    sum += rc.count;
  }
  if (total) *total = sum;
  if (sum <= max_range_chunks) return SM_OK;
  for (uint32_t r = 0; r < nranges && status; ++r) status[r] = SM_ERR_ARGUMENT;
  return SM_BUFFER_TOO_SMALL;
}

size_t smf_range_scratch_bytes(uint32_t nranges, uint32_t max_range_chunks) {
  return smf::range_meta_bytes(nranges, max_range_chunks) + smf::range_edge_bytes(nranges);
}

uint64_t smf_max_data_chunks(uint64_t n) { return n < SMF_IDENTIFIER_LENGTH ? 0 : (n - SMF_IDENTIFIER_LENGTH) / 8; }

size_t smf_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots) {
  const size_t decode = smf::decode_streams_bytes(nstreams, max_slots);
  const size_t compress = smf::compress_streams_bytes(nstreams, max_slots) + smf::compress_streams_slot_bytes(max_slots);
  return decode > compress ? decode : compress;
}

// the device's decode plan, stream by stream (smf_streams.h)
sm_status smf_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first, uint64_t* out_len,
                           int32_t* status, uint64_t* total) {
  if (nstreams > smf::kMaxStreams || max_chunks > smf::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nstreams && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nstreams; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0;
  for (uint32_t r = 0; r < nstreams; ++r) {
    const uint8_t* const p = in_len[r] ? in + in_off[r] : nullptr;
    const smf::Walk w = smf::walk_stream(in_len[r], smf::ByteFetch{p}, [](uint32_t, uint64_t, const smf::Chunk&) {});
    const smf::StreamPlan sp = smf::stream_plan(w, out_cap ? out_cap[r] : UINT64_MAX);
    if (first) first[r] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    if (out_len) out_len[r] = sp.length;
    if (status) status[r] = sp.status;
    sum += sp.slots;
  }
  if (first) first[nstreams] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  if (total) *total = sum;
  if (sum <= max_chunks) return SM_OK;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status) status[r] = SM_ERR_ARGUMENT;
    if (out_len) out_len[r] = 0;
  }
  return SM_BUFFER_TOO_SMALL;
}

}  // extern "C"
