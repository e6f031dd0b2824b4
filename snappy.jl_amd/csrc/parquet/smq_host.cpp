// smq_host.cpp -- the host-only part of the Parquet page library (include/snappy_mi355x_parquet.h):
// the walk over a host buffer, the size helpers, the host plan of the batched decode, the CRC
// tables and the host's model of the CRC kernel.  No HIP and no call into the other libraries, so
// this file also builds alone (the sanitizer driver, smq_host_check.cpp).
#include "smq_chunks.h"
#include "smq_crc.h"
#include "smq_encode.h"
#include "smq_format.h"

namespace smq {

const char* host_message(sm_status st) {
  switch (st) {
    case SMQ_ERR_HEADER: return "Parquet column chunk: malformed page header.";
    case SMQ_ERR_TRUNCATED: return "Parquet column chunk: truncated page header or page.";
    case SMQ_ERR_SIZE_MISMATCH: return "Parquet column chunk: a page's values do not have the declared size.";
    case SMQ_ERR_CRC: return "Parquet column chunk: a page's bytes do not have the stored CRC-32.";
    default: return nullptr;
  }
}

void build_crc_lut(CrcLut* T) {
  uint32_t t0[256];  // the byte table
  for (uint32_t b = 0; b < 256; ++b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? kCrcPoly : 0u);
    t0[b] = c;
  }
  // cur[b] after k steps: byte b followed by k zero bytes
  const uint32_t N = 16 * kCrcThreads;
  uint32_t cur[256];
  for (uint32_t b = 0; b < 256; ++b) cur[b] = t0[b];
  for (uint32_t k = 0; k < N; ++k) {
    if (k < 16)
      for (uint32_t b = 0; b < 256; ++b) T->tab[15 - k][b] = cur[b];
    if (k >= N - 4)  // (byte j of a register stands N - 1 - j bytes before the end of N zero bytes)
      for (uint32_t b = 0; b < 256; ++b) T->tab[16 + (N - 1 - k)][b] = cur[b];
    for (uint32_t b = 0; b < 256; ++b) cur[b] = (cur[b] >> 8) ^ t0[cur[b] & 0xff];
  }
  uint32_t x128 = 0x40000000u;  // x
  for (int i = 0; i < 7; ++i) x128 = gf_mul(x128, x128);
  T->xpow[0] = 0x80000000u;  // 1
  for (uint32_t g = 0; g < kCrcPow; ++g) T->xpow[g + 1] = gf_mul(T->xpow[g], x128);
  T->segpow[0] = T->xpow[kCrcPow];
  for (uint32_t k = 0; k + 1 < kCrcSegPow; ++k) T->segpow[k + 1] = gf_mul(T->segpow[k], T->segpow[k]);
}

uint32_t crc32_model(const CrcLut* T, const uint8_t* p, uint32_t n) {
  const uint32_t* tab = &T->tab[0][0];
  const uint32_t nseg = crc_segments(n);
  uint32_t acc = 0;
  for (uint32_t i = 0; i < nseg; ++i) {
    const uint8_t* q = p + crc_segment_start(n, i);
    const uint32_t len = crc_segment_len(n, i);
    const CrcSplit sp = crc_split(q, len);
    uint32_t s = crc_head(tab, T, q, sp, i == 0 ? 0xffffffffu : 0u);
    for (uint32_t t = 0; t < kCrcThreads && t < sp.G; ++t) s ^= crc_lane_granules(tab, T, q + sp.head, sp.G, t);
    acc ^= crc_shift_segments(T, crc_tail(tab, q, len, sp, s), nseg - 1 - i);
  }
  return n ? ~acc : 0u;
}

}  // namespace smq

extern "C" {

uint64_t smq_max_pages(uint64_t n) { return n / 7; }

sm_status smq_index(const uint8_t* buf, size_t n, const smq_pages* pages, uint32_t max_pages, smq_summary* summary) {
  if (!summary || (!buf && n)) return SM_ERR_ARGUMENT;
  if (pages && max_pages && !smq::valid_pages(*pages)) return SM_ERR_ARGUMENT;
  smq::Frame stack[SMQ_MAX_DEPTH];
  smq::ByteFetch fetch{buf};
  const smq::Walk w = smq::walk_pages(n, fetch, stack, [&](uint32_t k, uint64_t at, const smq::Page& p) {
    if (pages && k < max_pages) smq::store_page(*pages, k, at, p);
  });
  summary->total_length = w.total;
  summary->npages = w.npages;
  summary->status = smq::walk_status(w, pages != nullptr, max_pages);
  return summary->status;
}

sm_status smq_uncompressed_length(const uint8_t* buf, size_t n, size_t* result) {
  smq_summary s;
  const sm_status st = smq_index(buf, n, nullptr, 0, &s);
  if (st == SM_OK && result) *result = (size_t)s.total_length;
  return st;
}

size_t smq_chunks_scratch_bytes(uint32_t nchunks, uint32_t max_pages, uint32_t max_fragments) {
  return smq::decode_chunks_bytes(nchunks, max_pages, max_fragments);
}

// the device's decode plan, chunk by chunk (smq_chunks.h)
sm_status smq_chunks_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nchunks,
                          const uint64_t* out_cap, uint32_t max_pages, uint32_t* first, uint64_t* out_len, int32_t* status,
                          uint64_t* total_pages, uint64_t* total_fragments) {
  if (nchunks > smq::kMaxChunks || max_pages > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (nchunks && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nchunks; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0, fragments = 0;
  smq::Frame stack[SMQ_MAX_DEPTH];
  for (uint32_t r = 0; r < nchunks; ++r) {
    smq::ByteFetch fetch{in_len[r] ? in + in_off[r] : nullptr};
    uint64_t frags = 0;  // of this chunk's compressed sections, should it be decoded
    const smq::Walk w = smq::walk_pages(in_len[r], fetch, stack, [&](uint32_t, uint64_t, const smq::Page& p) {
      if (p.flags & SMQ_PAGE_COMPRESSED) frags += smq::fragments(smq::section_want(p));
    });
    const smq::ChunkPlan cp = smq::chunk_plan(w, out_cap ? out_cap[r] : UINT64_MAX);
    if (first) first[r] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    if (out_len) out_len[r] = cp.length;
    if (status) status[r] = cp.status;
    sum += cp.slots;
    if (cp.status == SM_OK) fragments += frags;
  }
  if (first) first[nchunks] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  if (total_pages) *total_pages = sum;
  if (total_fragments) *total_fragments = fragments;
  if (sum <= max_pages) return SM_OK;
  for (uint32_t r = 0; r < nchunks; ++r) {
    if (status) status[r] = SM_ERR_ARGUMENT;
    if (out_len) out_len[r] = 0;
  }
  return SM_BUFFER_TOO_SMALL;
}

// ---- the page encoder (include/snappy_mi355x_parquet_write.h) ------------------------------------------

uint64_t smqe_max_chunk_length(uint64_t n, uint64_t pages) { return n + n / 6 + 40 * pages; }

uint64_t smqe_stage_bound(uint64_t total_in_bytes, uint64_t pages) {
  return smq::kStageDump + total_in_bytes + total_in_bytes / 6 + 48 * pages;
}

sm_status smqe_rewrite_header(const uint8_t* hdr, size_t n, uint64_t new_body_len, uint32_t crc, uint8_t* out, size_t cap,
                              size_t* out_len) {
  if (!out_len || (!hdr && n) || (!out && cap)) return SM_ERR_ARGUMENT;
  smq::Frame stack[SMQ_MAX_DEPTH];
  smq::ByteFetch fetch{hdr};
  smq::Reader<smq::ByteFetch> r(fetch, n, stack);
  smq::HeaderFields h;
  smq::read_page_header<smq::EncodeWalk>(r, h);
  if (!r.ok()) return r.status;
  if (!smq::header_fields_ok<smq::EncodeWalk>(h)) return SMQ_ERR_HEADER;
  if (r.pos > 0xffffffffull) return SMQ_ERR_HEADER;
  if (new_body_len > smq::kMaxBody) return SM_ERR_INPUT_TOO_LARGE;
  const smq::Rewrite w = smq::make_rewrite((uint32_t)r.pos, smq::header_sites(h, 0), (uint32_t)new_body_len, crc);
  *out_len = w.new_len;
  if (w.new_len > cap) return SM_BUFFER_TOO_SMALL;
  for (uint32_t i = 0; i < w.new_len; ++i) out[i] = smq::rewritten_byte(w, fetch, i);
  return SM_OK;
}

sm_status smqe_index(const uint8_t* buf, size_t n, const smq_pages* pages, uint32_t* sites, uint32_t max_pages,
                     smq_summary* summary) {
  if (!summary || (!buf && n)) return SM_ERR_ARGUMENT;
  if (pages && max_pages && !smq::valid_pages(*pages)) return SM_ERR_ARGUMENT;
  smq::Frame stack[SMQ_MAX_DEPTH];
  smq::ByteFetch fetch{buf};
  const smq::Walk w = smq::walk_pages<smq::EncodeWalk>(n, fetch, stack, [&](uint32_t k, uint64_t at, const smq::Page& p) {
    if (!pages || k >= max_pages) return;
    smq::store_page(*pages, k, at, p);
    if (sites) {
      const uint32_t v[SMQE_SITES] = {p.sites.f3_at, p.sites.f3_len, p.sites.f4_at, p.sites.f4_len, p.sites.f7_at};
      for (uint32_t i = 0; i < SMQE_SITES; ++i) sites[(size_t)k * SMQE_SITES + i] = v[i];
    }
  });
  summary->total_length = w.total;
  summary->npages = w.npages;
  summary->status = smq::walk_status(w, pages != nullptr, max_pages);
  return summary->status;
}

size_t smqe_scratch_bytes(uint32_t nchunks, uint32_t max_pages, uint64_t stage_bytes) {
  return smq::encode_chunks_bytes(nchunks, max_pages, (size_t)stage_bytes);
}

// the device's encode plan, chunk by chunk (smq_encode.h)
sm_status smqe_chunks_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nchunks,
                           uint32_t max_pages, uint32_t* first, int32_t* status, uint64_t* out_bound, uint64_t* total_pages,
                           uint64_t* stage_bytes, uint64_t* total_fragments) {
  if (nchunks > smq::kMaxChunks || max_pages > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (nchunks && (!in_off || !in_len)) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nchunks; ++r)
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
  uint64_t sum = 0, stage = smq::kStageDump, fragments = 0;
  smq::Frame stack[SMQ_MAX_DEPTH];
  for (uint32_t r = 0; r < nchunks; ++r) {
    smq::ByteFetch fetch{in_len[r] ? in + in_off[r] : nullptr};
    uint64_t slots = 0, frags = 0, bound = 0;  // of this chunk, should it be compressed
    const smq::Walk w = smq::walk_pages<smq::EncodeWalk>(in_len[r], fetch, stack, [&](uint32_t, uint64_t, const smq::Page& p) {
      slots += smq::stage_slot(p);
      frags += smq::encode_fragments(p);
      bound += smq::page_bound(p);
    });
    const bool ok = w.status == SM_OK;
    if (first) first[r] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    if (status) status[r] = w.status;
    if (out_bound) out_bound[r] = ok ? bound : 0;
    if (ok) {
      sum += w.npages;
      stage += slots;
      fragments += frags;
    }
  }
  if (first) first[nchunks] = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  if (total_pages) *total_pages = sum;
  if (stage_bytes) *stage_bytes = stage;
  if (total_fragments) *total_fragments = fragments;
  if (sum <= max_pages) return SM_OK;
  for (uint32_t r = 0; r < nchunks; ++r) {
    if (status) status[r] = SM_ERR_ARGUMENT;
    if (out_bound) out_bound[r] = 0;
  }
  return SM_BUFFER_TOO_SMALL;
}

}  // extern "C"
