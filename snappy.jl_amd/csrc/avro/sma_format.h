// sma_format.h -- the rules of the Avro object container file with the snappy codec
// (include/snappy_mi355x_avro.h), shared by the host walkers (sma_host.cpp) and the one-wave device
// walkers (sma_kernels.hip): one walk, written once, so that all give the same status for the same
// stream; the sync search's rule; and the encoder's sizes and bytes.  Plain functions, compiled for
// the host and the device alike.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_avro.h"
#include "../common/smc_layout.h"

namespace sma {

constexpr uint32_t kMaxDeclared = 0x7fffffffu;  // a payload or a block that declares more is refused
constexpr uint32_t kSync = SMA_SYNC_LENGTH;
constexpr uint32_t kMinBlock = 1 + 1 + 5 + kSync;  // count, size, an empty raw stream (1) + the checksum (4), the marker
constexpr uint32_t kBlockExtra = 10 + 10 + 4 + kSync;  // the most a block adds to its payload: two longs, checksum, marker

SMC_HD inline bool valid_kind(int kind) { return kind == SMA_INPUT_FILE || kind == SMA_INPUT_BLOCKS; }

struct Walk {
  uint64_t total = 0;       // declared uncompressed bytes so far
  uint64_t objects = 0;     // the blocks' counts so far (saturating)
  uint64_t header_len = 0;  // SMA_INPUT_FILE: the bytes in front of the first block, once the header is read
  uint32_t nblocks = 0;
  int32_t status = SM_OK;
  uint8_t sync[kSync] = {};  // the marker: the header's, or the caller's
};

struct Block {
  uint64_t pay_off;  // the payload (a raw Snappy stream), from the stream's first byte
  uint32_t pay_len, ulen;
  uint64_t count;  // objects
  uint32_t crc;    // the stored checksum of the uncompressed bytes
};

// A long at pos: a zigzag varint of at most 10 bytes, little-endian 7-bit groups.  fetch(p) is byte
// p of the stream, asked for p < n only.  0 with the value and pos behind it, else the status.
template <typename Fetch>
SMC_HD inline int32_t read_long(Fetch& fetch, uint64_t n, uint64_t& pos, int64_t& v) {
  uint64_t u = 0;
  uint32_t shift = 0;
  for (uint32_t i = 0;; ++i) {
    if (pos >= n) return SMA_ERR_TRUNCATED;
    const uint32_t b = fetch(pos);
    ++pos;
    if (i == 9) {  // the 10th byte holds bit 63 alone
      if (b > 1) return SMA_ERR_VARLONG;
      u |= (uint64_t)b << 63;
      break;
    }
    u |= (uint64_t)(b & 127u) << shift;
    shift += 7;
    if (b < 128) break;
  }
  v = (int64_t)((u >> 1) ^ (~(u & 1) + 1));
  return SM_OK;
}

// bytes of v as a long, and byte i of them
SMC_HD inline uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
SMC_HD inline uint32_t long_len(int64_t v) {
  uint64_t u = zigzag(v);
  uint32_t k = 1;
  while (u >= 128) {
    u >>= 7;
    ++k;
  }
  return k;
}
SMC_HD inline uint8_t long_byte(int64_t v, uint32_t i, uint32_t nb) {
  const uint32_t low = (uint32_t)(zigzag(v) >> (7 * i)) & 127u;
  return (uint8_t)(i + 1 < nb ? low + 128u : low);
}

// the bytes [pos, pos + len) of the stream against a text
template <typename Fetch>
SMC_HD inline bool equals(Fetch& fetch, uint64_t pos, const char* text, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i)
    if (fetch(pos + i) != (uint32_t)(uint8_t)text[i]) return false;
  return true;
}

// The file header at 0: the magic, the metadata map, the marker.  Leaves pos behind the marker.
template <typename Fetch>
SMC_HD inline int32_t walk_header(Fetch& fetch, uint64_t n, uint64_t& pos, uint8_t* sync) {
  const uint8_t magic[4] = {0x4f, 0x62, 0x6a, 0x01};
  if (n == 0) return SMA_ERR_NO_HEADER;
  for (uint32_t i = 0; i < 4 && i < n; ++i)
    if (fetch(i) != magic[i]) return SMA_ERR_NO_HEADER;
  if (n < 4) return SMA_ERR_TRUNCATED;
  pos = 4;
  bool seen = false, snappy = false;
  for (;;) {
    int64_t c;
    int32_t st = read_long(fetch, n, pos, c);
    if (st != SM_OK) return st;
    if (c == 0) break;
    if (c < 0) {
      if (c == INT64_MIN) return SMA_ERR_BAD_HEADER;
      c = -c;
      int64_t bytes;
      st = read_long(fetch, n, pos, bytes);
      if (st != SM_OK) return st;
      if (bytes < 0) return SMA_ERR_BAD_HEADER;
    }
    for (; c > 0; --c) {  // (no bound on c: a pair takes two bytes at the least, so the stream's end stops it)
      int64_t len;
      st = read_long(fetch, n, pos, len);
      if (st != SM_OK) return st;
      if (len < 0) return SMA_ERR_BAD_HEADER;
      if ((uint64_t)len > n - pos) return SMA_ERR_TRUNCATED;
      const bool codec = len == 10 && equals(fetch, pos, "avro.codec", 10);
      pos += (uint64_t)len;
      st = read_long(fetch, n, pos, len);
      if (st != SM_OK) return st;
      if (len < 0) return SMA_ERR_BAD_HEADER;
      if ((uint64_t)len > n - pos) return SMA_ERR_TRUNCATED;
      if (codec) {
        seen = true;
        snappy = len == 6 && equals(fetch, pos, "snappy", 6);
      }
      pos += (uint64_t)len;
    }
  }
  if (n - pos < kSync) return SMA_ERR_TRUNCATED;
  for (uint32_t i = 0; i < kSync; ++i) sync[i] = (uint8_t)fetch(pos + i);
  pos += kSync;
  return seen && snappy ? (int32_t)SM_OK : (int32_t)SMA_ERR_CODEC;
}

// One stream of n bytes: the one walk.  fetch(p), p < n, is the only access to the stream, so no
// byte at n or behind it is read, whatever lies there; marker: the caller's 16 bytes
// (SMA_INPUT_BLOCKS), unused for a file; entry(k, at, b) gets block k, whose output starts at byte
// `at` of the stream's content.  A block's bytes are read front to back (its payload's varint, then
// the checksum and the marker behind it) and judged in the documented order.
template <typename Fetch, typename Entry>
SMC_HD inline Walk walk_stream(int kind, uint64_t n, Fetch& fetch, const uint8_t* marker, Entry entry) {
  Walk w;
  uint64_t pos = 0;
  if (kind == SMA_INPUT_FILE) {
    w.status = walk_header(fetch, n, pos, w.sync);
    if (w.status != SM_OK) {  // (a refused codec's marker is not handed out either)
      for (uint32_t i = 0; i < kSync; ++i) w.sync[i] = 0;
      return w;
    }
    w.header_len = pos;
  } else {
    for (uint32_t i = 0; i < kSync; ++i) w.sync[i] = marker[i];
  }
  while (pos != n) {
    int64_t count, size;
    w.status = read_long(fetch, n, pos, count);
    if (w.status != SM_OK) break;
    if (count < 0) {
      w.status = SMA_ERR_BLOCK;
      break;
    }
    w.status = read_long(fetch, n, pos, size);
    if (w.status != SM_OK) break;
    if (size < 4) {  // (negative, or no room for the checksum)
      w.status = SMA_ERR_BLOCK;
      break;
    }
    const uint64_t rest = n - pos;
    if ((uint64_t)size > rest || rest - (uint64_t)size < kSync) {
      w.status = SMA_ERR_TRUNCATED;
      break;
    }
    if ((uint64_t)size - 4 > kMaxDeclared) {
      w.status = SMA_ERR_TOO_LARGE;
      break;
    }
    const uint32_t pay_len = (uint32_t)(size - 4);
    uint32_t d, hv;
    const int32_t varint = smc::parse_varint32([&](uint32_t i) { return fetch(pos + i); }, pay_len, d, hv);
    const uint64_t tail = pos + pay_len;  // the checksum, the marker behind it
    uint32_t crc = 0;
    for (uint32_t i = 0; i < 4; ++i) crc = (crc << 8) | fetch(tail + i);
    bool synced = true;
    for (uint32_t i = 0; i < kSync; ++i) synced = synced && fetch(tail + 4 + i) == w.sync[i];
    if (!synced) {
      w.status = SMA_ERR_SYNC;
      break;
    }
    if (varint != 0) {
      w.status = SM_ERR_VARINT;
      break;
    }
    if (d > kMaxDeclared) {
      w.status = SMA_ERR_TOO_LARGE;
      break;
    }
    const Block b{pos, pay_len, d, (uint64_t)count, crc};
    entry(w.nblocks, w.total, b);
    ++w.nblocks;
    w.total += d;
    w.objects = w.objects + (uint64_t)count < w.objects ? UINT64_MAX : w.objects + (uint64_t)count;
    pos = tail + 4 + kSync;
  }
  return w;
}

// the walk's final status: its first structural error, else whether the entries fitted
SMC_HD inline int32_t walk_status(const Walk& w, bool stored, uint32_t max_blocks) {
  if (w.status != SM_OK) return w.status;
  return stored && w.nblocks > max_blocks ? SM_BUFFER_TOO_SMALL : SM_OK;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

// ---- the sync search ---------------------------------------------------------------------------
// The marker as two little-endian words, and the 16 bytes at byte k (0..15) of the 32 bytes
// w[0..3]: a candidate is compared 16 bytes at a time.
struct Marker {
  uint64_t lo, hi;
};
SMC_HD inline Marker load_marker(const uint8_t* m) {
  Marker r{0, 0};
  for (uint32_t i = 0; i < 8; ++i) {
    r.lo |= (uint64_t)m[i] << (8 * i);
    r.hi |= (uint64_t)m[8 + i] << (8 * i);
  }
  return r;
}
SMC_HD inline bool marker_at(const uint64_t* w, uint32_t k, const Marker& m) {
  const uint32_t q = k >> 3, s = 8 * (k & 7);
  const uint64_t a = s ? (w[q] >> s) | (w[q + 1] << (64 - s)) : w[q];
  const uint64_t b = s ? (w[q + 1] >> s) | (w[q + 2] << (64 - s)) : w[q + 1];
  return a == m.lo && b == m.hi;
}
// The answer of one query over a host buffer, by the rule the kernel's tiles apply: the least
// p >= from with p + 16 <= n and the marker at p, else n.
inline uint64_t find_sync_host(const uint8_t* p, uint64_t n, const uint8_t* marker, uint64_t from) {
  const Marker m = load_marker(marker);
  for (uint64_t at = from; at + kSync <= n && at >= from; ++at) {
    uint64_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < kSync; ++i) w[i >> 3] |= (uint64_t)p[at + i] << (8 * (i & 7));
    if (marker_at(w, 0, m)) return at;
  }
  return n;
}

// ---- the encoder rule ---------------------------------------------------------------------------
// what a block of `count` objects whose raw stream has `comp` bytes takes: the two longs, the
// payload, the checksum, the marker
SMC_HD inline uint64_t block_bytes(uint64_t count, uint32_t comp) {
  return (uint64_t)long_len((int64_t)count) + long_len((int64_t)comp + 4) + comp + 4 + kSync;
}
SMC_HD inline uint64_t max_block_length(uint64_t len) { return smc::max_compressed_length(len) + kBlockExtra; }
// a block's place in the stage: its raw stream's bound, rounded up to 16 bytes
SMC_HD inline uint64_t stage_length(uint64_t len) { return (smc::max_compressed_length(len) + 15) / 16 * 16; }
// the multi library's two fragment bounds: the decoder's index holds every slot's fragments, the
// compressor without an index counts those of its streams of more than 64 KiB
SMC_HD inline uint64_t decode_fragments(uint64_t ulen) { return (ulen + 65535) / 65536; }
SMC_HD inline uint64_t encode_fragments(uint64_t len) { return len > 65536 ? (len + 65535) / 65536 : 0; }

const char* host_message(sm_status st);  // sma_host.cpp: the SMA_ERR_* texts, else NULL

}  // namespace sma
