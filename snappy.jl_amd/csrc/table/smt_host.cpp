// smt_host.cpp -- the host-only part of the LevelDB table library
// (include/snappy_mi355x_table.h): the footer, the index walk and a block's head over host buffers,
// the size helpers and the writer of a table's tail.  No HIP and no call into the other libraries,
// so this file also builds alone (the sanitizer driver, smt_host_check.cpp).
#include <string.h>

#include "smt_format.h"

namespace smt {

const char* host_message(sm_status st) {
  switch (st) {
    case SMT_ERR_TRUNCATED: return "Table file: shorter than its 48-byte footer.";
    case SMT_ERR_MAGIC: return "Table file: the footer does not end with LevelDB's table magic.";
    case SMT_ERR_FOOTER: return "Table file: corrupt block handle in the footer.";
    case SMT_ERR_HANDLE: return "Table file: a block handle points outside the bytes in front of the footer.";
    case SMT_ERR_TOO_LARGE: return "Table file: a block of more than 2147483647 bytes.";
    case SMT_ERR_TYPE: return "Table file: a block's compression type is neither none nor Snappy.";
    case SMT_ERR_INDEX: return "Table file: corrupt index block.";
    case SMT_ERR_CRC: return "Table file: a block's masked CRC-32C does not match its stored bytes.";
    default: return nullptr;
  }
}

namespace {

// the running CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) is kept bit by bit in the Writer:
// the tail's three short blocks only.  The device path takes its checksums from the framing library.
uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// appends to a buffer of `cap` bytes, counting on when it is full or absent; the running checksum
// of the block being written is kept beside it
struct Writer {
  uint8_t* out;
  size_t cap, n = 0;
  uint32_t crc = 0xffffffffu;
  void byte(uint8_t b) {
    if (out && n < cap) out[n] = b;
    ++n;
    crc ^= b;
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0x82F63B78u & (0u - (crc & 1u)));
  }
  void bytes(const uint8_t* p, size_t len) {
    for (size_t i = 0; i < len; ++i) byte(p[i]);
  }
  void varint64(uint64_t v) {
    const uint32_t nb = varint64_len(v);
    for (uint32_t i = 0; i < nb; ++i) byte(varint64_byte(v, i, nb));
  }
  void fixed32(uint32_t v) {
    for (uint32_t i = 0; i < 4; ++i) byte((uint8_t)(v >> (8 * i)));
  }
  // the type byte (stored) and the masked checksum of the bytes since the last trailer
  void trailer() {
    byte(kStored);
    const uint32_t c = mask_crc(~crc);
    fixed32(c);
    crc = 0xffffffffu;
  }
};

}  // namespace

}  // namespace smt

extern "C" {

uint64_t smt_max_blocks(uint64_t index_bytes) { return index_bytes / smt::kMinEntry; }

uint64_t smt_max_block_length(uint64_t len) { return smt::max_block_length(len); }

uint64_t smt_stage_length(uint64_t len) { return smt::stage_length(len); }

sm_status smt_footer(const uint8_t* buf, size_t n, uint64_t* meta_off, uint64_t* meta_size, uint64_t* index_off,
                     uint64_t* index_size) {
  if ((!buf && n) || !meta_off || !meta_size || !index_off || !index_size) return SM_ERR_ARGUMENT;
  smt::ByteFetch fetch{buf};
  smt::Handle meta, index;
  const int32_t st = smt::read_footer(fetch, n, meta, index);
  *meta_off = meta.off;
  *meta_size = meta.size;
  *index_off = index.off;
  *index_size = index.size;
  return st;
}

sm_status smt_block_head(const uint8_t* buf, size_t n, uint64_t off, uint64_t size, uint32_t* type, uint64_t* declared) {
  if ((!buf && n) || !type || !declared) return SM_ERR_ARGUMENT;
  *type = 0;
  *declared = 0;
  if (size > n || n - size < smt::kTrailer || off > n - size - smt::kTrailer) return SMT_ERR_HANDLE;
  if (size > smt::kMaxSize) return SMT_ERR_TOO_LARGE;
  smt::ByteFetch fetch{buf};
  return smt::block_head(fetch, off, size, *type, *declared);
}

sm_status smt_index_bound(const uint8_t* buf, size_t n, uint64_t* index_bytes) {
  if ((!buf && n) || !index_bytes) return SM_ERR_ARGUMENT;
  *index_bytes = 0;
  smt::ByteFetch fetch{buf};
  smt::Handle meta, index;
  const int32_t st = smt::read_footer(fetch, n, meta, index);
  if (st != SM_OK) return st;
  uint32_t type;
  return smt::block_head(fetch, index.off, index.size, type, *index_bytes);
}

sm_status smt_walk_index(const uint8_t* contents, size_t m, uint64_t table_len, uint64_t* handles_off,
                         uint64_t* handles_size, uint32_t max, smt_summary* summary) {
  if (!summary || (!contents && m) || table_len < smt::kFooter || !handles_off != !handles_size) return SM_ERR_ARGUMENT;
  smt::ByteFetch fetch{contents};
  const smt::IndexWalk w = smt::walk_index(fetch, m, table_len, [&](uint32_t k, const smt::Handle& h) {
    if (!handles_off || k >= max) return;
    handles_off[k] = h.off;
    handles_size[k] = h.size;
  });
  summary->total_length = w.bytes;
  summary->nblocks = w.nblocks;
  summary->status = w.status != SM_OK ? w.status : handles_off && w.nblocks > max ? (int32_t)SM_BUFFER_TOO_SMALL : (int32_t)SM_OK;
  return summary->status;
}

size_t smt_tables_scratch_bytes(uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes, uint32_t max_fragments,
                                uint64_t stage_bytes) {
  const size_t decode = smt::decode_bytes(ntables, max_blocks, (size_t)max_index_bytes, max_fragments);
  const size_t compress = smt::compress_bytes(ntables, max_blocks, (size_t)stage_bytes + 64);
  return decode > compress ? decode : compress;
}

sm_status smt_write_tail(const uint8_t* keys, const uint64_t* key_off, uint32_t nblocks, const uint64_t* handle_off,
                         const uint64_t* handle_size, uint64_t base, uint8_t* out, size_t out_cap, size_t* out_len) {
  if (!out_len || (nblocks && (!key_off || !handle_off || !handle_size))) return SM_ERR_ARGUMENT;
  for (uint32_t j = 0; j < nblocks; ++j)
    if (key_off[j] > key_off[j + 1] || key_off[j + 1] - key_off[j] > 0xffffffffull || (key_off[j + 1] > key_off[j] && !keys))
      return SM_ERR_ARGUMENT;
  smt::Writer w{out, out_cap};
  // the metaindex block: no entries, the restart array {0}, its count 1
  const smt::Handle meta{base, 8};
  w.fixed32(0);
  w.fixed32(1);
  w.trailer();
  // the index block: restart interval 1, so every entry is a restart point and shares nothing
  const uint64_t index_at = base + w.n;
  for (uint32_t j = 0; j < nblocks; ++j) {
    const uint64_t klen = key_off[j + 1] - key_off[j];
    w.varint64(0);
    w.varint64(klen);
    w.varint64(smt::varint64_len(handle_off[j]) + smt::varint64_len(handle_size[j]));
    if (klen) w.bytes(keys + key_off[j], (size_t)klen);
    w.varint64(handle_off[j]);
    w.varint64(handle_size[j]);
  }
  {
    // the restart array: every entry's offset in the contents (an empty block keeps the one restart 0)
    uint64_t at = 0;
    for (uint32_t j = 0; j < nblocks; ++j) {
      if (at > 0xffffffffull) return SM_ERR_INPUT_TOO_LARGE;
      w.fixed32((uint32_t)at);
      const uint64_t klen = key_off[j + 1] - key_off[j];
      const uint32_t vlen = smt::varint64_len(handle_off[j]) + smt::varint64_len(handle_size[j]);
      at += 1 + smt::varint64_len(klen) + 1 + klen + vlen;
    }
    if (nblocks == 0) w.fixed32(0);
    w.fixed32(nblocks ? nblocks : 1u);
  }
  const smt::Handle index{index_at, base + w.n - index_at};
  w.trailer();
  // the footer: the two handles, the padding, the magic
  const size_t footer_at = w.n;
  w.varint64(meta.off);
  w.varint64(meta.size);
  w.varint64(index.off);
  w.varint64(index.size);
  while (w.n - footer_at < smt::kFooter - 8) w.byte(0);
  for (uint32_t i = 0; i < 8; ++i) w.byte((uint8_t)(smt::kMagic >> (8 * i)));
  *out_len = w.n;
  return out && w.n > out_cap ? (sm_status)SM_BUFFER_TOO_SMALL : (sm_status)SM_OK;
}

}  // extern "C"
