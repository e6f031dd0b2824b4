// smt_format.h -- the rules of the LevelDB table file (include/snappy_mi355x_table.h), shared by
// the host (smt_host.cpp) and the kernels (smt_kernels.hip): the footer, a block's head, the index
// walk, a block's and a table's verdict, the encoder's choice and the scratch layouts.  Plain
// functions, compiled for the host and the device alike, so the host checker tests the code the
// kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../../include/snappy_mi355x_table.h"
#include "../common/smc_layout.h"
#include "../common/smc_slots.h"

namespace smt {

constexpr uint64_t kFooter = SMT_FOOTER_LENGTH;
constexpr uint64_t kTrailer = SMT_BLOCK_TRAILER;    // the type byte and the fixed32 checksum
constexpr uint64_t kMagic = 0xdb4775248b80fb57ull;  // 57 fb 80 8b 24 75 47 db on disk
constexpr uint64_t kMaxSize = 0x7ffffffeull;        // a handle's size above it is refused
constexpr uint64_t kMaxDeclared = 0x7fffffffull;    // a declared length above it is refused
constexpr uint32_t kMaxCount = 0x7fffffffu;         // more tables or blocks: SM_ERR_ARGUMENT
constexpr uint32_t kNone = 0xffffffffu;             // a table without a failing block
constexpr uint32_t kMinEntry = 5;                   // three one-byte fields and a two-byte handle
enum : uint32_t { kStored = 0, kSnappy = 1 };

struct Handle {
  uint64_t off, size;
};

// a handle against a table of n >= 48 bytes: the block and its trailer lie in front of the footer
SMC_HD inline int32_t check_handle(const Handle& h, uint64_t n) {
  const uint64_t limit = n - kFooter;
  if (h.size > limit || limit - h.size < kTrailer || h.off > limit - h.size - kTrailer) return SMT_ERR_HANDLE;
  return h.size > kMaxSize ? (int32_t)SMT_ERR_TOO_LARGE : (int32_t)SM_OK;
}

// a handle at [pos, end): fetch(p) is byte p, asked for p < end only.  0 with pos behind it.
template <typename Fetch>
SMC_HD inline int32_t read_handle(Fetch& fetch, uint64_t& pos, uint64_t end, Handle& h) {
  uint32_t len;
  uint64_t room = end - pos;
  if (smc::parse_varint64([&](uint32_t i) { return fetch(pos + i); }, room > 10 ? 10u : (uint32_t)room, h.off, len)) return 1;
  pos += len;
  room = end - pos;
  if (smc::parse_varint64([&](uint32_t i) { return fetch(pos + i); }, room > 10 ? 10u : (uint32_t)room, h.size, len)) return 1;
  pos += len;
  return 0;
}

// The footer of a table of n bytes.
template <typename Fetch>
SMC_HD inline int32_t read_footer(Fetch& fetch, uint64_t n, Handle& meta, Handle& index) {
  meta = Handle{0, 0};
  index = Handle{0, 0};
  if (n < kFooter) return SMT_ERR_TRUNCATED;
  uint64_t magic = 0;
  for (uint32_t i = 0; i < 8; ++i) magic |= (uint64_t)(fetch(n - 8 + i) & 0xffu) << (8 * i);
  if (magic != kMagic) return SMT_ERR_MAGIC;
  uint64_t pos = n - kFooter;
  const uint64_t end = n - 8;
  if (read_handle(fetch, pos, end, meta) || read_handle(fetch, pos, end, index)) return SMT_ERR_FOOTER;
  const int32_t st = check_handle(meta, n);
  return st != SM_OK ? st : check_handle(index, n);
}

// The head of the block at (off, size), whose size + 5 bytes the caller knows to be there: at most
// six bytes are read, the type and the first min(size, 5) of a compressed block's contents.
template <typename Fetch>
SMC_HD inline int32_t block_head(Fetch& fetch, uint64_t off, uint64_t size, uint32_t& type, uint64_t& declared) {
  type = fetch(off + size) & 0xffu;
  declared = 0;
  if (type == kStored) {
    declared = size;
    return SM_OK;
  }
  if (type != kSnappy) return SMT_ERR_TYPE;
  uint32_t d, hv;
  if (smc::parse_varint32([&](uint32_t i) { return fetch(off + i); }, size > 5 ? 5u : (uint32_t)size, d, hv) != 0) return SM_ERR_VARINT;
  if (d > kMaxDeclared) return SMT_ERR_TOO_LARGE;
  declared = d;
  return SM_OK;
}

// the stored checksum behind the type byte
template <typename Fetch>
SMC_HD inline uint32_t block_crc(Fetch& fetch, uint64_t off, uint64_t size) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < 4; ++i) c |= (fetch(off + size + 1 + i) & 0xffu) << (8 * i);
  return c;
}

struct IndexWalk {
  uint64_t bytes = 0;  // the recorded handles' sizes
  uint32_t nblocks = 0;
  int32_t status = SM_OK;
};

// The index block's contents, m bytes, of a table of n bytes: the one walk.  fetch(p), p < m, is the
// only access; no key byte is read.  entry(k, handle) gets entry k.
template <typename Fetch, typename Entry>
SMC_HD inline IndexWalk walk_index(Fetch& fetch, uint64_t m, uint64_t n, Entry entry) {
  IndexWalk w;
  w.status = SMT_ERR_INDEX;
  if (m < 4) return w;
  uint32_t r = 0;
  for (uint32_t i = 0; i < 4; ++i) r |= (fetch(m - 4 + i) & 0xffu) << (8 * i);
  if (r > (m - 4) / 4) return w;
  const uint64_t limit = m - 4 * (1 + (uint64_t)r);
  uint64_t p = 0, key_len = 0;
  while (p != limit) {
    if (limit - p < 3) return w;
    uint32_t f[3], hv;
    for (uint32_t k = 0; k < 3; ++k) {
      const uint64_t room = limit - p;
      if (smc::parse_varint32([&](uint32_t i) { return fetch(p + i); }, room > 5 ? 5u : (uint32_t)room, f[k], hv) != 0) return w;
      p += hv;
    }
    if ((uint64_t)f[1] + f[2] > limit - p) return w;
    if (f[0] > key_len) return w;
    key_len = (uint64_t)f[0] + f[1];
    uint64_t v = p + f[1];  // the value, behind the key's own bytes
    Handle h;
    if (read_handle(fetch, v, p + f[1] + f[2], h)) return w;
    const int32_t st = check_handle(h, n);
    if (st != SM_OK) {
      w.status = st;
      return w;
    }
    entry(w.nblocks, h);
    ++w.nblocks;
    w.bytes += h.size;
    p += (uint64_t)f[1] + f[2];
  }
  w.status = SM_OK;
  return w;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

// ---- verdicts -----------------------------------------------------------------------------------
// What is known of a table before its index is walked: the footer's status, the index block's type,
// its checksum, then the raw decoder's status on it (the head's varint or the decode).
SMC_HD inline int32_t index_verdict(int32_t footer, int32_t head, bool verify, uint32_t stored, uint32_t computed,
                                    uint32_t type, int32_t dec_status) {
  if (footer != SM_OK) return footer;
  if (head == SMT_ERR_TYPE) return head;
  if (verify && stored != computed) return SMT_ERR_CRC;
  if (head != SM_OK) return head;
  return type == kSnappy ? dec_status : (int32_t)SM_OK;
}

// A decoded block's status: the checksum covers the stored bytes, so it outranks the decoder.
SMC_HD inline int32_t block_verdict(bool verify, uint32_t stored, uint32_t computed, uint32_t type, int32_t dec_status) {
  if (verify && stored != computed) return SMT_ERR_CRC;
  return type == kSnappy ? dec_status : (int32_t)SM_OK;
}

// A table's status before any block is decoded and whether it is decoded: the index stage's, its
// first failing head's, SM_BUFFER_TOO_SMALL against its room.
SMC_HD inline int32_t table_plan(int32_t index_status, int32_t head_status, uint64_t total, uint64_t cap) {
  if (index_status != SM_OK) return index_status;
  if (head_status != SM_OK) return head_status;
  return total > cap ? (int32_t)SM_BUFFER_TOO_SMALL : (int32_t)SM_OK;
}

// ---- the encoder rule ---------------------------------------------------------------------------
// LevelDB's 12.5 % rule
SMC_HD inline bool keep_compressed(int32_t comp_status, uint32_t clen, uint32_t len) {
  return comp_status == SM_OK && clen != 0 && clen < len - len / 8;
}
SMC_HD inline uint64_t max_block_length(uint64_t len) { return len + kTrailer; }
SMC_HD inline uint64_t stage_length(uint64_t len) { return (smc::max_compressed_length(len) + 15) / 16 * 16; }
SMC_HD inline uint64_t decode_fragments(uint64_t ulen) { return (ulen + 65535) / 65536; }
SMC_HD inline uint64_t encode_fragments(uint64_t len) { return len > 65536 ? (len + 65535) / 65536 : 0; }
using smc::round16;

// bytes of v as a varint64, and byte i of them
SMC_HD inline uint32_t varint64_len(uint64_t v) {
  uint32_t k = 1;
  while (v >= 128) {
    v >>= 7;
    ++k;
  }
  return k;
}
SMC_HD inline uint8_t varint64_byte(uint64_t v, uint32_t i, uint32_t nb) {
  const uint32_t low = (uint32_t)(v >> (7 * i)) & 127u;
  return (uint8_t)(i + 1 < nb ? low + 128u : low);
}

const char* host_message(sm_status st);  // smt_host.cpp: the SMT_ERR_* texts, else NULL

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
using Header = smc::PlanHeader;  // total: entries (blocks) in use; over: more than one of the caller's bounds

struct Decode {
  Header* hdr;
  // per table (nt): the index stage
  uint64_t *ix_in_off, *ix_out_off, *ix_crc_off, *t_len;
  uint32_t *ix_in_len, *ix_cap, *ix_out_len, *ix_crc_len, *ix_stored, *ix_computed, *ix_type, *ix_len, *ix_size, *count, *first, *fail;
  int32_t *ix_footer, *ix_head, *ix_dec, *ix_status, *t_pre;
  uint8_t* ix_live;
  // per block (m): the handles (absolute in d_in for the decode), the heads, the slots' arguments
  uint64_t *h_off, *h_size, *b_in_off, *b_out_off, *b_crc_off, *prefix;  // prefix: m + 1
  uint32_t *b_in_len, *b_cap, *b_out_len, *b_crc_len, *b_stored, *b_computed, *b_type, *b_decl, *b_table, *b_copy;
  int32_t *b_head, *b_dec, *b_index_status;
  uint32_t *frag_first, *frag_pos;  // m + 1, max(max_fragments, 1)
  uint8_t* built;
  uint8_t* index;  // index_bytes: the decoded index blocks
  uintptr_t end;
};

inline Decode carve_decode(uint8_t* buf, size_t nt, size_t m, size_t index_bytes, size_t max_fragments) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  Decode s;
  s.hdr = c.take<Header>(1);
  for (uint64_t** p : {&s.ix_in_off, &s.ix_out_off, &s.ix_crc_off, &s.t_len}) *p = c.take<uint64_t>(nt);
  for (uint32_t** p : {&s.ix_in_len, &s.ix_cap, &s.ix_out_len, &s.ix_crc_len, &s.ix_stored, &s.ix_computed, &s.ix_type, &s.ix_len,
                       &s.ix_size, &s.count, &s.fail})
    *p = c.take<uint32_t>(nt);
  s.first = c.take<uint32_t>(nt + 1);
  for (int32_t** p : {&s.ix_footer, &s.ix_head, &s.ix_dec, &s.ix_status, &s.t_pre}) *p = c.take<int32_t>(nt);
  s.ix_live = c.take<uint8_t>(nt);
  for (uint64_t** p : {&s.h_off, &s.h_size, &s.b_in_off, &s.b_out_off, &s.b_crc_off}) *p = c.take<uint64_t>(m);
  s.prefix = c.take<uint64_t>(m + 1);
  for (uint32_t** p : {&s.b_in_len, &s.b_cap, &s.b_out_len, &s.b_crc_len, &s.b_stored, &s.b_computed, &s.b_type, &s.b_decl,
                       &s.b_table, &s.b_copy})
    *p = c.take<uint32_t>(m);
  for (int32_t** p : {&s.b_head, &s.b_dec, &s.b_index_status}) *p = c.take<int32_t>(m);
  s.frag_first = c.take<uint32_t>(m + 1);
  s.frag_pos = c.take<uint32_t>(max_fragments ? max_fragments : 1);
  s.built = c.take<uint8_t>(m);
  s.index = c.take<uint8_t>(index_bytes + 16);
  s.end = c.p;
  return s;
}
inline size_t decode_bytes(size_t nt, size_t m, size_t index_bytes, size_t max_fragments) {
  return (size_t)carve_decode(nullptr, nt, m, index_bytes, max_fragments).end;
}

struct Compress {
  Header* hdr;
  // per block (m)
  uint64_t *in_off, *slot_off, *crc_off;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the packed block sizes over all blocks
  uint32_t *in_len, *comp_len, *table, *crc_len, *crc, *chosen, *type;
  int32_t* comp_status;
  uint32_t* fail;  // per table
  uint8_t* stage;  // stage_bytes: the raw compressor's output
  uintptr_t end;
};

inline Compress carve_compress(uint8_t* buf, size_t nt, size_t m, size_t stage_bytes) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  Compress s;
  s.hdr = c.take<Header>(1);
  for (uint64_t** p : {&s.in_off, &s.slot_off, &s.crc_off}) *p = c.take<uint64_t>(m);
  s.size_scan = c.take<uint64_t>(m + 1);
  for (uint32_t** p : {&s.in_len, &s.comp_len, &s.table, &s.crc_len, &s.crc, &s.chosen, &s.type}) *p = c.take<uint32_t>(m);
  s.comp_status = c.take<int32_t>(m);
  s.fail = c.take<uint32_t>(nt);
  s.stage = c.take<uint8_t>(stage_bytes ? stage_bytes : 1);
  s.end = c.p;
  return s;
}
inline size_t compress_bytes(size_t nt, size_t m, size_t stage_bytes) {
  return (size_t)carve_compress(nullptr, nt, m, stage_bytes).end;
}

}  // namespace smt
