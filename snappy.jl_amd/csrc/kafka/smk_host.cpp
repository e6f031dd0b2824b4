// smk_host.cpp -- the host-only part of the Kafka segment library
// (include/snappy_mi355x_kafka.h): the walk and the heads over host buffers, the two plans by the
// rules the kernels run, the size helpers and the writer of one batch.  No HIP; of the other
// libraries only the blocks library's and the framing library's host-only entry points (smb_index,
// smf_crc32c), so this file builds with their host-only files alone (the sanitizer driver,
// smk_host_check.cpp).
#include <string.h>

#include <vector>

#include "../../../include/snappy_mi355x_framing.h"
#include "smk_format.h"

namespace smk {

const char* host_message(sm_status st) {
  switch (st) {
    case SMK_ERR_TRUNCATED: return "Log segment: a record batch runs past the end of the segment.";
    case SMK_ERR_MAGIC: return "Log segment: a record batch whose magic is not 2.";
    case SMK_ERR_LENGTH: return "Log segment: a batch length below 49 or negative.";
    case SMK_ERR_CODEC: return "Log segment: a record batch whose codec is neither none nor snappy.";
    case SMK_ERR_TOO_LARGE: return "Log segment: a record batch of more than 2147483598 bytes of records.";
    case SMK_ERR_CRC: return "Log segment: a record batch's CRC-32C does not match its stored bytes.";
    case SMB_ERR_NO_HEADER: return "Log segment: a batch's snappy-java stream does not start with its header.";
    case SMB_ERR_BAD_HEADER: return "Log segment: corrupt snappy-java header in a record batch.";
    case SMB_ERR_TRUNCATED: return "Log segment: truncated snappy-java chunk in a record batch.";
    case SMB_ERR_CHUNK_TOO_LARGE: return "Log segment: a snappy-java chunk of more than 2147483647 uncompressed bytes.";
    default: return nullptr;
  }
}

namespace {

// a recorded batch's head on the host: batch_head, and for a snappy-java batch the blocks library's walk
struct HostHead {
  uint32_t kind = kStored, declared = 0, chunks = 0;
  uint64_t fragments = 0;  // of its chunks (kXerial) or of itself (kRaw)
  int32_t status = SM_OK;
};

HostHead host_head(const uint8_t* seg, const Batch& b) {
  ByteFetch fetch{seg};
  const Head h = batch_head(fetch, b);
  HostHead r;
  r.kind = h.kind;
  r.declared = h.declared;
  r.status = h.status;
  if (h.kind == kRaw && h.status == SM_OK) r.fragments = decode_fragments(h.declared);
  if (h.kind != kXerial) return r;
  const uint8_t* const p = seg + b.pos + kHeader;
  const size_t n = b.length - kMinLength;
  smb_summary s;
  smb_index(p, n, SMB_FORMAT_XERIAL, nullptr, 0, &s);
  r.status = xerial_head(s.status, s.total_length, r.declared);
  if (r.status != SM_OK) return r;
  r.chunks = s.nchunks;
  std::vector<uint64_t> pay_off(s.nchunks + 1);
  std::vector<uint32_t> pay_len(s.nchunks + 1), ulen(s.nchunks + 1);
  const smb_chunks c{pay_off.data(), pay_len.data(), ulen.data()};
  smb_index(p, n, SMB_FORMAT_XERIAL, &c, s.nchunks, &s);
  for (uint32_t k = 0; k < s.nchunks; ++k) r.fragments += decode_fragments(ulen[k]);
  return r;
}

// a segment on the host: its walk, its heads up to the first failing one, what the device's plan needs
struct HostSegment {
  Walk walk;
  int32_t head_status = SM_OK;  // the first failing head's
  uint64_t length = 0;          // the rewritten lengths before the first failure
  uint64_t chunks = 0, zero_chunks = 0, x_fragments = 0, r_fragments = 0;
};

template <typename Each>
HostSegment host_segment(const uint8_t* seg, uint64_t n, Each each) {
  HostSegment r;
  ByteFetch fetch{seg};
  r.walk = walk_segment(fetch, n, [&](uint32_t k, const Batch& b) {
    const HostHead h = host_head(seg, b);
    each(k, b, h);
    if (h.status == SM_OK && h.kind == kXerial && h.declared == 0) r.zero_chunks += h.chunks;
    if (r.head_status != SM_OK) return;
    if (h.status != SM_OK) {
      r.head_status = h.status;
      return;
    }
    r.length += rewritten_length(h.declared);
    r.chunks += h.chunks;
    if (h.kind == kXerial) r.x_fragments += h.fragments;
    else r.r_fragments += h.fragments;
  });
  return r;
}

uint32_t scan32(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }  // (an entry of `first`, as the device's scan saturates it)

}  // namespace

}  // namespace smk

extern "C" {

uint64_t smk_max_segment_length(uint64_t n, uint64_t nbatches) { return smk::max_segment_length(n, nbatches); }

uint64_t smk_stage_length(uint64_t len) { return smk::stage_length(len); }

size_t smk_segments_scratch_bytes(uint32_t nsegments, uint32_t max_batches, uint32_t max_fragments, uint64_t stage_bytes) {
  const size_t decode = smk::decode_bytes(nsegments, max_batches, max_fragments);
  const size_t compress = smk::compress_bytes(nsegments, max_batches, (size_t)stage_bytes + 64);
  return decode > compress ? decode : compress;
}

sm_status smk_index(const uint8_t* buf, size_t n, uint64_t* pos, uint32_t* length, uint32_t* codec, uint64_t* declared,
                    int32_t* status, uint32_t max_batches, smk_summary* summary) {
  if (!summary || (!buf && n)) return SM_ERR_ARGUMENT;
  const bool arrays = pos || length || codec || declared || status;
  const smk::HostSegment g = smk::host_segment(buf, n, [&](uint32_t k, const smk::Batch& b, const smk::HostHead& h) {
    if (k >= max_batches) return;
    if (pos) pos[k] = b.pos;
    if (length) length[k] = b.length;
    if (codec) codec[k] = b.codec;
    if (declared) declared[k] = h.declared;
    if (status) status[k] = h.status;
  });
  summary->total_length = g.length;
  summary->valid_length = g.walk.valid;
  summary->nbatches = g.walk.nbatches;
  summary->status = g.walk.status != SM_OK ? g.walk.status
                    : g.head_status != SM_OK ? g.head_status
                    : arrays && g.walk.nbatches > max_batches ? (int32_t)SM_BUFFER_TOO_SMALL : (int32_t)SM_OK;
  return summary->status;
}

// the device's decode plan, segment by segment
sm_status smk_segments_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nsegments,
                            const uint64_t* out_cap, uint32_t max_batches, uint32_t max_chunks, uint32_t* first,
                            uint64_t* out_len, int32_t* status, uint64_t* total_batches, uint64_t* total_chunks,
                            uint64_t* total_fragments) {
  if (nsegments > smk::kMaxCount || max_batches > smk::kMaxCount || max_chunks > smk::kMaxCount) return SM_ERR_ARGUMENT;
  if (nsegments && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nsegments; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t batches = 0, chunks = 0, zero_chunks = 0, x_fragments = 0, r_fragments = 0;
  for (uint32_t r = 0; r < nsegments; ++r) {
    const smk::HostSegment g = smk::host_segment(in_len[r] ? in + in_off[r] : nullptr, in_len[r],
                                                 [](uint32_t, const smk::Batch&, const smk::HostHead&) {});
    const int32_t st = smk::segment_plan(g.walk.status, g.head_status, g.length, out_cap ? out_cap[r] : UINT64_MAX);
    if (first) first[r] = smk::scan32(batches);
    if (out_len) out_len[r] = g.length;
    if (status) status[r] = st;
    batches += g.walk.nbatches;
    zero_chunks += g.zero_chunks;
    if (st != SM_OK) continue;
    chunks += g.chunks;
    x_fragments += g.x_fragments;
    r_fragments += g.r_fragments;
  }
  if (first) first[nsegments] = smk::scan32(batches);
  if (zero_chunks > chunks) chunks = zero_chunks;
  if (total_batches) *total_batches = batches;
  if (total_chunks) *total_chunks = chunks;
  if (total_fragments) *total_fragments = x_fragments > r_fragments ? x_fragments : r_fragments;
  if (batches <= max_batches && chunks <= max_chunks) return SM_OK;
  for (uint32_t r = 0; r < nsegments; ++r) {
    if (out_len) out_len[r] = 0;
    if (status) status[r] = SM_ERR_ARGUMENT;
  }
  return SM_BUFFER_TOO_SMALL;
}

sm_status smk_compress_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nsegments,
                            uint32_t max_batches, uint32_t* first, uint64_t* room, int32_t* status, uint64_t* total_batches,
                            uint64_t* total_blocks, uint64_t* stage_bytes) {
  if (nsegments > smk::kMaxCount || max_batches > smk::kMaxCount) return SM_ERR_ARGUMENT;
  if (nsegments && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nsegments; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t batches = 0, blocks = 0, stage = 0;
  for (uint32_t r = 0; r < nsegments; ++r) {
    smk::ByteFetch fetch{in_len[r] ? in + in_off[r] : nullptr};
    uint64_t seg_blocks = 0, seg_stage = 0;
    const smk::Walk w = smk::walk_segment(fetch, in_len[r], [&](uint32_t, const smk::Batch& b) {
      if (!smk::compressed_here(b)) return;
      seg_blocks += smk::blocks_of(b.length - smk::kMinLength);
      seg_stage += smk::stage_length(b.length - smk::kMinLength);
    });
    if (first) first[r] = smk::scan32(batches);
    if (room) room[r] = smk::max_segment_length(in_len[r], w.nbatches);
    if (status) status[r] = w.status;
    batches += w.nbatches;
    if (w.status != SM_OK) continue;
    blocks += seg_blocks;
    stage += seg_stage;
  }
  if (first) first[nsegments] = smk::scan32(batches);
  if (total_batches) *total_batches = batches;
  if (total_blocks) *total_blocks = blocks;
  if (stage_bytes) *stage_bytes = stage;
  if (batches <= max_batches) return SM_OK;
  for (uint32_t r = 0; r < nsegments && status; ++r) status[r] = SM_ERR_ARGUMENT;
  return SM_BUFFER_TOO_SMALL;
}

sm_status smk_write_batch(uint64_t base_offset, uint32_t partition_leader_epoch, uint32_t attributes, const uint8_t* tail,
                          const uint8_t* records, size_t records_len, uint8_t* out, size_t out_cap, size_t* out_len) {
  if (!out_len || !tail || (!records && records_len) || attributes > 0xffffu || (attributes & smk::kCodecMask)) return SM_ERR_ARGUMENT;
  if (records_len > smk::kMaxDeclared) return SM_ERR_INPUT_TOO_LARGE;
  *out_len = smk::kHeader + records_len;
  if (!out) return SM_OK;
  if (out_cap < *out_len) return SM_BUFFER_TOO_SMALL;
  const uint32_t L = smk::kMinLength + (uint32_t)records_len;
  for (uint32_t i = 0; i < 8; ++i) out[i] = (uint8_t)(base_offset >> (8 * (7 - i)));
  for (uint32_t i = 0; i < 4; ++i) out[8 + i] = (uint8_t)(L >> (8 * (3 - i)));
  for (uint32_t i = 0; i < 4; ++i) out[12 + i] = (uint8_t)(partition_leader_epoch >> (8 * (3 - i)));
  out[16] = (uint8_t)smk::kMagic;
  out[smk::kAttributesAt] = (uint8_t)(attributes >> 8);
  out[smk::kAttributesAt + 1] = (uint8_t)attributes;
  memcpy(out + 23, tail, smk::kHeader - 23);
  if (records_len) memcpy(out + smk::kHeader, records, records_len);
  const uint32_t c = smf_crc32c(out + smk::kCrcFrom, *out_len - smk::kCrcFrom);
  for (uint32_t i = 0; i < 4; ++i) out[smk::kCrcAt + i] = (uint8_t)(c >> (8 * (3 - i)));
  return SM_OK;
}

}  // extern "C"
