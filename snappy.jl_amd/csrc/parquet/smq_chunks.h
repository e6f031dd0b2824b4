// smq_chunks.h -- the rules of the batched call (smq_uncompress_chunks_device), shared by its kernels
// (smq_kernels.hip) and the host (smq_chunks_plan in smq_host.cpp, which the sanitizer driver runs):
// what a walked chunk of a batch gets, a slot's verdict (a chunk's is smc::plan_verdict) and
// the scratch layout -- and the encoder's slots and their carve (smqe_compress_chunks_device; its
// rules are smq_encode.h's).  The walk itself is walk_pages (smq_format.h).  Plain functions, compiled for
// the host and the device alike, so the host checker tests the code the kernels run.  Not part of
// the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../../include/snappy_mi355x_parquet_write.h"
#include "../common/smc_slots.h"
#include "smq_format.h"

namespace smq {

constexpr uint32_t kMaxChunks = 0x7fffffffu;  // more chunks or pages: SM_ERR_ARGUMENT
using smc::kNoSlot;                           // a slot of no chunk; a chunk without a failing slot

struct Header {    // a plan's words for the kernels behind it: smc::PlanHeader's two and the CRC pass's
  uint32_t total;  // slots in use (0 over the bound: nothing is decoded)
  uint32_t over;   // the chunks need more slots than the caller's bound
  uint32_t segments;  // CRC segments of all slots (0 without verification)
  uint32_t pad;
};

struct ChunkPlan {
  int32_t status;   // the walk's error, SM_BUFFER_TOO_SMALL, or SM_OK: what is known before any decode
  uint32_t slots;   // its pages when it is decoded, else 0
  uint64_t length;  // the uncompressed sizes: before the error, else of the whole chunk (the size needed)
};

// What a walked chunk gets with `cap` bytes of room: only a well-formed chunk that fits is decoded.
SMC_HD inline ChunkPlan chunk_plan(const Walk& w, uint64_t cap) {
  ChunkPlan p{w.status, 0, w.total};
  if (p.status == SM_OK && w.total > cap) p.status = SM_BUFFER_TOO_SMALL;
  if (p.status == SM_OK) p.slots = w.npages;
  return p;
}

// A slot's status: SM_OK for a slot no page took; SMQ_ERR_CRC when its body was checked (`checked`)
// and does not have the header's CRC; else the raw decoder's for a compressed section; else SM_OK.
SMC_HD inline int32_t slot_verdict(uint32_t chunk, bool checked, uint32_t crc_got, uint32_t crc_want, bool compressed,
                                   int32_t dec_status) {
  if (chunk == kNoSlot) return SM_OK;
  if (checked && crc_got != crc_want) return SMQ_ERR_CRC;
  return compressed ? dec_status : (int32_t)SM_OK;
}

// A slot's stored bytes (level bytes, a section that is not compressed) are copied in tiles
// (smc::copy_tiled).  A page has no bound short of 2 GiB, so the rows (smc::copy_rows) are sized for
// pages of kCopyTypical bytes (the writers' default page size); a longer one is strided.
constexpr uint32_t kCopyTypical = 1u << 20;

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
struct DecodeChunks {
  Header* hdr;
  // per slot (m = max_pages): the page's body and output (offsets relative to d_in and d_out), what
  // of the body is copied, and the two smm calls' arguments and results.  A slot without a
  // compressed section has in_len 0 and cap 0 for them -- the raw decoder returns from it at once;
  // a slot no page took has all lengths 0 and chunk kNoSlot
  uint64_t *body_off, *page_out, *in_off, *out_off;
  uint32_t *body_len, *copy_len, *in_len, *cap, *out_len, *chunk, *flags, *crc_want, *crc_got, *seg_first;
  int32_t *dec_status, *index_status;
  uint32_t *frag_first, *frag_pos;  // m + 1, max(max_fragments, 1): the index smm_index_device builds
  uint8_t* built;
  // per chunk
  uint64_t* length;
  uint32_t *count, *first, *fail;
  int32_t* pre;
  uintptr_t end;
};

inline DecodeChunks carve_decode_chunks(uint8_t* buf, size_t nchunks, size_t m, size_t max_fragments) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  DecodeChunks s;
  s.hdr = c.take<Header>(1);
  s.body_off = c.take<uint64_t>(m);
  s.page_out = c.take<uint64_t>(m);
  s.in_off = c.take<uint64_t>(m);
  s.out_off = c.take<uint64_t>(m);
  s.body_len = c.take<uint32_t>(m);
  s.copy_len = c.take<uint32_t>(m);
  s.in_len = c.take<uint32_t>(m);
  s.cap = c.take<uint32_t>(m);
  s.out_len = c.take<uint32_t>(m);
  s.chunk = c.take<uint32_t>(m);
  s.flags = c.take<uint32_t>(m);
  s.crc_want = c.take<uint32_t>(m);
  s.crc_got = c.take<uint32_t>(m);
  s.seg_first = c.take<uint32_t>(m + 1);
  s.dec_status = c.take<int32_t>(m);
  s.index_status = c.take<int32_t>(m);
  s.frag_first = c.take<uint32_t>(m + 1);
  s.frag_pos = c.take<uint32_t>(max_fragments ? max_fragments : 1);
  s.built = c.take<uint8_t>(m);
  s.length = c.take<uint64_t>(nchunks);
  s.count = c.take<uint32_t>(nchunks);
  s.first = c.take<uint32_t>(nchunks + 1);
  s.fail = c.take<uint32_t>(nchunks);
  s.pre = c.take<int32_t>(nchunks);
  s.end = c.p;
  return s;
}
inline size_t decode_chunks_bytes(size_t nchunks, size_t m, size_t max_fragments) {
  return (size_t)carve_decode_chunks(nullptr, nchunks, m, max_fragments).end;
}

// ---- the encoder's scratch (smqe_compress_chunks_device) ---------------------------------------------
// The stage's first bytes belong to no page: a slot without a section is an empty stream to the raw
// compressor, which wants room for sm_max_compressed_length(0) bytes wherever it writes.
constexpr uint64_t kStageDump = 32;
struct EncodeChunks {
  Header* hdr;
  // per slot (m = max_pages).  The page in the input: its header's place (relative to d_in), the
  // lengths and the patch sites; the raw compressor's arguments and results (a slot without a section
  // -- a page that is stepped over, a slot no page took -- is an empty stream that compresses to the
  // stage's dump bytes); the staged body (relative to the stage); the page in the output
  uint64_t *hdr_in, *in_off, *comp_off, *body_off, *page_out, *stage_len;
  uint32_t *hdr_len, *old_body, *levels, *in_len, *comp_len, *new_body, *new_hdr, *chunk, *flags, *crc_acc, *seg_first;
  uint32_t* sites;  // SMQE_SITES words a slot
  int32_t *comp_status, *slot_status;
  // per chunk
  uint32_t *count, *first, *fail, *go;
  int32_t* pre;
  uint8_t* stage;  // stage_bytes (kStageDump at the least), from a 16-byte boundary
  uintptr_t end;
};

inline EncodeChunks carve_encode_chunks(uint8_t* buf, size_t nchunks, size_t m, size_t stage_bytes) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  EncodeChunks s;
  s.hdr = c.take<Header>(1);
  for (uint64_t** a : {&s.hdr_in, &s.in_off, &s.comp_off, &s.body_off, &s.page_out, &s.stage_len}) *a = c.take<uint64_t>(m);
  for (uint32_t** a : {&s.hdr_len, &s.old_body, &s.levels, &s.in_len, &s.comp_len, &s.new_body, &s.new_hdr, &s.chunk, &s.flags, &s.crc_acc})
    *a = c.take<uint32_t>(m);
  s.seg_first = c.take<uint32_t>(m + 1);
  s.sites = c.take<uint32_t>(m * SMQE_SITES);
  s.comp_status = c.take<int32_t>(m);
  s.slot_status = c.take<int32_t>(m);
  s.count = c.take<uint32_t>(nchunks);
  s.first = c.take<uint32_t>(nchunks + 1);
  s.fail = c.take<uint32_t>(nchunks);
  s.go = c.take<uint32_t>(nchunks);
  s.pre = c.take<int32_t>(nchunks);
  s.stage = c.take<uint8_t>(stage_bytes < kStageDump ? kStageDump : stage_bytes);
  s.end = c.p;
  return s;
}
inline size_t encode_chunks_bytes(size_t nchunks, size_t m, size_t stage_bytes) {
  return (size_t)carve_encode_chunks(nullptr, nchunks, m, stage_bytes).end;
}

// smq_crc32_device's own arrays: per range the scan of its segments and its register
struct CrcRanges {
  Header* hdr;
  uint32_t *seg_first, *acc;
  uintptr_t end;
};
inline CrcRanges carve_crc_ranges(uint8_t* buf, size_t n) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  CrcRanges s;
  s.hdr = c.take<Header>(1);
  s.seg_first = c.take<uint32_t>(n + 1);
  s.acc = c.take<uint32_t>(n);
  s.end = c.p;
  return s;
}
inline size_t crc_ranges_bytes(size_t n) { return (size_t)carve_crc_ranges(nullptr, n).end; }

}  // namespace smq
