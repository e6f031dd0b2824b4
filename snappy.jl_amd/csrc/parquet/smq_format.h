// smq_format.h -- the rules of a Parquet column chunk's pages (include/snappy_mi355x_parquet.h),
// shared by the host walkers (smq_host.cpp) and the one-wave device walkers (smq_kernels.hip,
// smq_encode.hip): one walk, written once over the Thrift reader of smq_thrift.h, so that all give
// the same status for the same chunk; the page encoder runs it under its own policy (EncodeWalk).  Plain functions, compiled for the host and the device alike.  Not part of the
// public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_parquet.h"
#include "../common/smc_layout.h"
#include "smq_thrift.h"

namespace smq {

constexpr uint32_t kFragment = 65536;  // the raw codec's block: a longer section may decode by fragments

struct Walk {
  uint64_t total = 0;   // uncompressed sizes so far
  uint32_t npages = 0;  // pages so far
  int32_t status = SM_OK;
};

// The two policies of the one walk.  DecodeWalk reads a compression=SNAPPY chunk (the public
// header's walk).  EncodeWalk reads the same pages in their plain form, as a writer holds them before
// compression (snappy_mi355x_parquet_write.h): the sections are not Snappy yet, so none is looked at,
// a page with output must have compressed_page_size == uncompressed_page_size, a field that is
// patched must occur once, and the header's patch sites are recorded.
struct DecodeWalk {
  static constexpr bool encode = false;
};
struct EncodeWalk {
  static constexpr bool encode = true;
};

// Where an encoder patches a PageHeader, from the header's first byte (EncodeWalk only; else zeros):
// the bytes of field 3's value, those of field 4's value (f4_len 0: the header has no crc) and the
// field header byte of the data_page_header_v2's field 7 (0: it has none; no header starts with it).
struct Sites {
  uint32_t f3_at, f3_len, f4_at, f4_len, f7_at;
};

struct Page {
  uint64_t hdr_off;  // from the chunk's first byte
  uint32_t hdr_len, body_len, usize, levels;
  int32_t num_values, type, encoding;
  uint32_t flags, crc;
  bool output;  // a data or dictionary page: its usize bytes are the chunk's output at the walk's total
  Sites sites = {0, 0, 0, 0, 0};
};

// the values section of a page with output: the body behind the level bytes, and its decoded size
SMC_HD inline uint32_t section_len(const Page& p) { return p.body_len - p.levels; }
SMC_HD inline uint32_t section_want(const Page& p) { return p.usize - p.levels; }
// the bytes that go to the output as they are stored, from the body's start: the level bytes, and
// behind them a section that is not compressed
SMC_HD inline uint32_t copy_len(const Page& p) {
  return !p.output ? 0u : (p.flags & SMQ_PAGE_COMPRESSED) ? p.levels : p.body_len;
}

// what a PageHeader's fields hold, as far as the walk reads them
struct HeaderFields {
  int32_t type = 0, usize = 0, csize = 0, crc = 0;
  uint32_t seen = 0;  // bit id: field id of the PageHeader was there with its type
  // num_values and encoding of fields 5, 7 and 8 (named, not indexed: they stay in registers)
  int32_t data_values = 0, data_encoding = 0, dict_values = 0, dict_encoding = 0, v2_values = 0, v2_encoding = 0;
  int32_t def_len = 0, rep_len = 0;
  bool is_compressed = true;
  // EncodeWalk only: the patch sites as positions in the chunk (f3_end 0: no field 3 yet), and
  // whether a patched field came twice
  uint64_t f3_at = 0, f3_end = 0, f4_at = 0, f4_end = 0, f7_at = 0;
  bool repeated = false;
};

// a page type's struct: num_values at id 1, encoding at `encoding_id`; v2: the data_page_header_v2,
// with the level lengths and is_compressed
template <typename Policy, typename Fetch>
SMQ_INLINE void read_page_type_header(Reader<Fetch>& r, int32_t encoding_id, bool v2, int32_t& num_values, int32_t& encoding,
                                         HeaderFields& h) {
  int32_t id = 0;
  uint32_t t;
  for (;;) {
    const uint64_t at = r.pos;  // the field header's byte
    if (!r.field(id, t)) break;
    if (id == 1 && t == kI32) num_values = r.i32();
    else if (id == encoding_id && t == kI32) encoding = r.i32();
    else if (v2 && id == 5 && t == kI32) h.def_len = r.i32();
    else if (v2 && id == 6 && t == kI32) h.rep_len = r.i32();
    else if (v2 && id == 7 && (t == kTrue || t == kFalse)) {
      h.is_compressed = t == kTrue;
      if (Policy::encode) {
        if (h.f7_at) h.repeated = true;
        h.f7_at = at;
      }
    } else r.skip(t, 2);
  }
}

template <typename Policy, typename Fetch>
SMQ_INLINE void read_page_header(Reader<Fetch>& r, HeaderFields& h) {
  int32_t id = 0;
  uint32_t t;
  while (r.field(id, t)) {
    if (id >= 1 && id <= 4 && t == kI32) {
      const uint64_t at = r.pos;
      const int32_t v = r.i32();
      (id == 1 ? h.type : id == 2 ? h.usize : id == 3 ? h.csize : h.crc) = v;
      if (Policy::encode && id >= 3) {
        if (h.seen & (1u << id)) h.repeated = true;
        (id == 3 ? h.f3_at : h.f4_at) = at;
        (id == 3 ? h.f3_end : h.f4_end) = r.pos;
      }
      h.seen |= 1u << id;
    } else if ((id == 5 || id == 7 || id == 8) && t == kStruct) {
      if (id == 5) read_page_type_header<Policy>(r, 2, false, h.data_values, h.data_encoding, h);
      else if (id == 7) read_page_type_header<Policy>(r, 2, false, h.dict_values, h.dict_encoding, h);
      else read_page_type_header<Policy>(r, 4, true, h.v2_values, h.v2_encoding, h);
      h.seen |= 1u << id;
    } else {
      r.skip(t, 1);
    }
  }
}

// the checks of a PageHeader's own fields 1 to 4: all of 1, 2 and 3 as i32, no size below 0, and
// for an encoder no patched field twice
template <typename Policy>
SMQ_INLINE bool header_fields_ok(const HeaderFields& h) {
  if ((h.seen & 0xeu) != 0xeu || h.usize < 0 || h.csize < 0) return false;
  return !(Policy::encode && h.repeated);
}

// the patch sites of the header that starts at byte `at` of its chunk
SMQ_INLINE Sites header_sites(const HeaderFields& h, uint64_t at) {
  return Sites{(uint32_t)(h.f3_at - at), (uint32_t)(h.f3_end - h.f3_at), h.f4_end ? (uint32_t)(h.f4_at - at) : 0u,
               (uint32_t)(h.f4_end - h.f4_at), h.f7_at ? (uint32_t)(h.f7_at - at) : 0u};
}

// One chunk of n bytes.  fetch(pos) is its byte pos < n -- the only access to the chunk; stack is
// the Thrift reader's SMQ_MAX_DEPTH frames; entry(k, at, p) gets page k, whose output (if any)
// starts at byte `at` of the chunk's content.
template <typename Policy = DecodeWalk, typename Fetch, typename Entry>
SMQ_INLINE Walk walk_pages(uint64_t n, Fetch& fetch, Frame* stack, Entry entry) {
  Walk w;
  Reader<Fetch> r(fetch, n, stack);
  while (r.pos != n) {
    const uint64_t at = r.pos;
    HeaderFields h;
    read_page_header<Policy>(r, h);
    if (!r.ok()) {
      w.status = r.status;
      break;
    }
    w.status = SMQ_ERR_HEADER;  // until the header's own checks are through
    if (!header_fields_ok<Policy>(h)) break;
    const int32_t sub = h.type == SMQ_PAGE_DATA ? 0 : h.type == SMQ_PAGE_DICTIONARY ? 1 : h.type == SMQ_PAGE_DATA_V2 ? 2 : -1;
    if (sub >= 0 && !(h.seen & (1u << (sub == 0 ? 5 : sub == 1 ? 7 : 8)))) break;
    Page p{at, (uint32_t)(r.pos - at), (uint32_t)h.csize, (uint32_t)h.usize, 0, 0, h.type, 0,
           (h.seen & (1u << 4)) ? SMQ_PAGE_HAS_CRC : 0u, (h.seen & (1u << 4)) ? (uint32_t)h.crc : 0u, sub >= 0};
    if (sub >= 0) {
      p.num_values = sub == 0 ? h.data_values : sub == 1 ? h.dict_values : h.v2_values;
      p.encoding = sub == 0 ? h.data_encoding : sub == 1 ? h.dict_encoding : h.v2_encoding;
    }
    if (sub == 2) {
      if (h.def_len < 0 || h.rep_len < 0) break;
      const uint64_t levels = (uint64_t)h.def_len + (uint64_t)h.rep_len;
      if (levels > p.usize || levels > p.body_len) break;
      p.levels = (uint32_t)levels;
    }
    if (p.body_len > n - r.pos) {
      w.status = SMQ_ERR_TRUNCATED;
      break;
    }
    if (Policy::encode) {
      p.sites = header_sites(h, at);
      if (p.output && p.body_len != p.usize) {  // (a plain page: nothing of its section is looked at)
        w.status = SMQ_ERR_SIZE_MISMATCH;
        break;
      }
    } else if (p.output) {
      const uint32_t len = section_len(p), want = section_want(p);
      w.status = SMQ_ERR_SIZE_MISMATCH;
      if (sub == 2 && !h.is_compressed) {
        if (len != want) break;
      } else if (len == 0) {
        if (want != 0) break;
      } else {
        const uint64_t sec = r.pos + p.levels;
        uint32_t d, hv;
        if (smc::parse_varint32([&](uint32_t i) { return fetch(sec + i); }, len, d, hv) != 0) {
          w.status = SM_ERR_VARINT;
          break;
        }
        if (d != want) break;
        p.flags |= SMQ_PAGE_COMPRESSED;
      }
    }
    w.status = SM_OK;
    entry(w.npages, w.total, p);
    ++w.npages;
    if (p.output) w.total += p.usize;
    r.pos += p.body_len;
  }
  return w;
}

// the walk's final status: its first error, else whether the entries fitted
SMC_HD inline int32_t walk_status(const Walk& w, bool stored, uint32_t max_pages) {
  if (w.status != SM_OK) return w.status;
  return stored && w.npages > max_pages ? SM_BUFFER_TOO_SMALL : SM_OK;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

// the 64 KiB fragments of a section that decodes to d bytes (smm_fragment_count)
SMC_HD inline uint64_t fragments(uint64_t d) { return d / kFragment + (d % kFragment ? 1 : 0); }

// page k of a walk into the arrays of an smq_pages, at entry j; its output at `at`
SMC_HD inline void store_page(const smq_pages& t, uint64_t j, uint64_t at, const Page& p) {
  t.hdr_off[j] = p.hdr_off;
  t.hdr_len[j] = p.hdr_len;
  t.body_len[j] = p.body_len;
  t.usize[j] = p.usize;
  t.levels[j] = p.levels;
  t.out_off[j] = at;
  t.num_values[j] = p.num_values;
  t.type[j] = p.type;
  t.encoding[j] = p.encoding;
  t.flags[j] = p.flags;
  t.crc[j] = p.crc;
}

inline bool valid_pages(const smq_pages& t) {
  return t.hdr_off && t.hdr_len && t.body_len && t.usize && t.levels && t.out_off && t.num_values && t.type && t.encoding &&
         t.flags && t.crc;
}

const char* host_message(sm_status st);  // smq_host.cpp: the SMQ_ERR_* texts, else NULL

}  // namespace smq
