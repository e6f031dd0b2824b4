// smf_format.h -- the framing format's rules, shared by the host walkers (smf_host.cpp) and the
// one-wave device walkers (smf_kernels.hip, smf_streams.hip): one chunk step and one loop around
// it, written once, so that all give the same status for the same stream.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_framing.h"
#include "../common/smc_layout.h"

namespace smf {

constexpr uint32_t kPoly = 0x82F63B78u;  // CRC-32C, reflected
constexpr uint32_t kBlock = 65536;       // uncompressed bytes per data chunk, at most
// the bytes of a chunk a walk step looks at: header (4), CRC (4), the payload's varint (<= 5)
constexpr uint32_t kHeadBytes = 13;

SMC_HD inline uint32_t mask(uint32_t crc) { return ((crc >> 15) | (crc << 17)) + 0xa282ead8u; }

struct Walk {
  uint64_t total = 0;    // declared uncompressed bytes so far
  uint32_t nchunks = 0;  // data chunks so far
  int32_t status = SM_OK;
  bool first = true;     // no identifier seen yet
};

struct Chunk {
  bool data;  // a data chunk (the fields below are set), else a skipped one
  uint8_t type;
  uint64_t pay_off;
  uint32_t pay_len, crc, ulen;
  uint64_t next;  // the next chunk's position
};

// One chunk at pos of an n-byte stream; h[0, have) = its first min(kHeadBytes, n - pos) bytes.
// false: the walk is over -- at the end of the stream, or at an error (w.status).
SMC_HD inline bool walk_step(Walk& w, const uint8_t* h, uint32_t have, uint64_t pos, uint64_t n, Chunk& c) {
  c.data = false;
  if (pos >= n) {
    if (w.first) w.status = SMF_ERR_NO_IDENTIFIER;  // (an empty stream)
    return false;
  }
  const uint32_t type = h[0];
  if (w.first && type != 0xff) {
    w.status = SMF_ERR_NO_IDENTIFIER;
    return false;
  }
  if (have < 4) {
    w.status = SMF_ERR_TRUNCATED;
    return false;
  }
  const uint32_t len = h[1] | ((uint32_t)h[2] << 8) | ((uint32_t)h[3] << 16);
  const uint64_t rem = n - pos - 4;
  c.type = (uint8_t)type;
  c.next = pos + 4 + len;
  if (type == 0xff) {
    if (len != 6) {
      w.status = SMF_ERR_BAD_IDENTIFIER;
      return false;
    }
    if (rem < 6) {
      w.status = SMF_ERR_TRUNCATED;
      return false;
    }
    const uint8_t id[6] = {0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};  // "sNaPpY"
    for (uint32_t i = 0; i < 6; ++i) {
      if (h[4 + i] != id[i]) {
        w.status = SMF_ERR_BAD_IDENTIFIER;
        return false;
      }
    }
    w.first = false;
    return true;
  }
  if (type >= 0x80) {  // padding (0xfe) and reserved skippable chunks
    if (rem < len) {
      w.status = SMF_ERR_TRUNCATED;
      return false;
    }
    return true;
  }
  if (type >= 2) {
    w.status = SMF_ERR_RESERVED_CHUNK;
    return false;
  }
  if (len < 4) {  // no room for the CRC
    w.status = SMF_ERR_TRUNCATED;
    return false;
  }
  if (type == SMF_CHUNK_UNCOMPRESSED && len > kBlock + 4) {
    w.status = SMF_ERR_CHUNK_TOO_LARGE;
    return false;
  }
  if (rem < len) {
    w.status = SMF_ERR_TRUNCATED;
    return false;
  }
  c.crc = h[4] | ((uint32_t)h[5] << 8) | ((uint32_t)h[6] << 16) | ((uint32_t)h[7] << 24);
  c.pay_len = len - 4;
  c.pay_off = pos + 8;
  if (type == SMF_CHUNK_UNCOMPRESSED) {
    c.ulen = c.pay_len;
  } else {  // the raw stream's varint32 header (the raw decoder's rules: at most 5 bytes, the 5th < 0x10)
    uint32_t v, hv;
    if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)h[8 + i]; }, c.pay_len, v, hv) != 0) {
      w.status = SM_ERR_VARINT;
      return false;
    }
    if (v > kBlock) {
      w.status = SMF_ERR_CHUNK_TOO_LARGE;
      return false;
    }
    c.ulen = v;
  }
  c.data = true;
  return true;
}

// the walk's final status: its first structural error, else whether the entries fitted
SMC_HD inline int32_t walk_status(const Walk& w, bool stored, uint32_t max_chunks) {
  if (w.status != SM_OK) return w.status;
  return stored && w.nchunks > max_chunks ? SM_BUFFER_TOO_SMALL : SM_OK;
}

// One stream of n bytes, chunk by chunk: the one loop around walk_step.  fetch(pos, have, h) brings
// the `have` bytes at pos into h -- the only access to the stream, so no byte at n or behind it is
// read, whatever lies there; entry(k, at, c) gets data chunk k, which starts at byte `at` of the
// stream's content.
template <typename Fetch, typename Entry>
SMC_HD inline Walk walk_stream(uint64_t n, Fetch fetch, Entry entry) {
  Walk w;
  uint64_t pos = 0;
  for (;;) {
    const uint32_t have = pos < n ? (uint32_t)(n - pos < kHeadBytes ? n - pos : kHeadBytes) : 0u;
    uint8_t h[kHeadBytes];
    fetch(pos, have, h);
    Chunk c;
    if (!walk_step(w, h, have, pos, n, c)) break;
    if (c.data) {
      entry(w.nchunks, w.total, c);
      ++w.nchunks;
      w.total += c.ulen;
    }
    pos = c.next;
  }
  return w;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  void operator()(uint64_t pos, uint32_t have, uint8_t* h) const {
    for (uint32_t i = 0; i < have; ++i) h[i] = p[pos + i];
  }
};

// entry k of an index
SMC_HD inline void store_chunk(const smf_chunks& ch, uint32_t k, const Chunk& c) {
  ch.type[k] = c.type;
  ch.pay_off[k] = c.pay_off;
  ch.pay_len[k] = c.pay_len;
  ch.crc[k] = c.crc;
  ch.ulen[k] = c.ulen;
}

// an index the caller handed in: every array is there
inline bool valid_chunks(const smf_chunks& ch) { return ch.type && ch.pay_off && ch.pay_len && ch.crc && ch.ulen; }

// A call's index of n entries into ch: null arrays for none, else the caller's, which has to be
// there whole (false: SM_ERR_ARGUMENT).
inline bool take_chunks(const smf_chunks* given, uint64_t n, smf_chunks& ch) {
  ch = smf_chunks{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (n == 0) return true;
  if (!given || !valid_chunks(*given)) return false;
  ch = *given;
  return true;
}

// ---- the encoder rule ---------------------------------------------------------------------------
constexpr uint8_t kTypeNone = 0xff;  // the compressor left an error mark for the block: nothing is packed

// A block of n bytes whose Snappy stream has c bytes (or is an error mark): the chunk's type -- 0x00
// iff the stream is strictly shorter than the block -- and, returned, the chunk's size in the stream.
SMC_HD inline uint32_t encoder_chunk(uint32_t c, uint32_t n, uint8_t& type) {
  if (c >= SM_OUT_LEN_ERROR) {
    type = kTypeNone;
    return 0;
  }
  type = c < n ? SMF_CHUNK_COMPRESSED : SMF_CHUNK_UNCOMPRESSED;
  return 8u + (type == SMF_CHUNK_COMPRESSED ? c : n);
}

// ---- CRC-32C in parallel (k_crc32c, smf_kernels.hip) ------------------------------------------
// Polynomials over GF(2) mod P in the reflected register's bit order: bit 31 is x^0.  A raw
// register s (zero init, no final xor) followed by k zero bytes becomes s * x^(8k) mod P.
constexpr uint32_t kCrcThreads = 256;  // lanes of a block's CRC; lane t owns the 16-byte granules
                                       // whose distance from the last one is t mod kCrcThreads
constexpr uint32_t kCrcTabs = 20;      // tab[i], i < 16: byte i of a granule, advanced to the granule's end;
                                       // tab[16 + j]: byte j of a register, advanced by kCrcThreads granules
constexpr uint32_t kCrcPow = 4096;     // xpow[g] = x^(128 g) mod P for g <= kCrcPow (64 KiB of granules)

struct CrcLut {
  uint32_t tab[kCrcTabs][256];
  uint32_t xpow[kCrcPow + 1];
  uint32_t xpow2[32];  // x^(128 * 2^k) mod P: longer blocks, by square and multiply
};

SMC_HD inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32; ++i) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1) ? kPoly : 0u);
  }
  return p;
}

// x^(128 g) mod P
SMC_HD inline uint32_t gf_xpow(const CrcLut* T, uint32_t g) {
  if (g <= kCrcPow) return T->xpow[g];
  uint32_t r = 0x80000000u;
  for (uint32_t k = 0; g; ++k, g >>= 1)
    if (g & 1) r = gf_mul(r, T->xpow2[k]);
  return r;
}

// one granule (16 bytes, little-endian dwords w[0..3]) behind register s, which is
// kCrcThreads granules old
SMC_HD inline uint32_t crc_granule(const uint32_t* tab, uint32_t s, const uint32_t* w) {
  uint32_t r = tab[16 * 256 + (s & 0xff)] ^ tab[17 * 256 + ((s >> 8) & 0xff)] ^ tab[18 * 256 + ((s >> 16) & 0xff)] ^
               tab[19 * 256 + (s >> 24)];
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t v = w[k];
    r ^= tab[(4 * k) * 256 + (v & 0xff)] ^ tab[(4 * k + 1) * 256 + ((v >> 8) & 0xff)] ^
         tab[(4 * k + 2) * 256 + ((v >> 16) & 0xff)] ^ tab[(4 * k + 3) * 256 + (v >> 24)];
  }
  return r;
}

void build_crc_lut(CrcLut* T);     // smf_host.cpp
const char* host_message(sm_status st);  // smf_host.cpp: the SMF_ERR_* texts, else NULL

}  // namespace smf
