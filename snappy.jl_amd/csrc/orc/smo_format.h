// smo_format.h -- the rules of ORC's compression chunks (include/snappy_mi355x_orc.h), shared by the
// host walkers (smo_host.cpp) and the one-wave device walkers (smo_kernels.hip): one walk, written
// once, so that all give the same status for the same stream; and the encoder rule's sizes.
// Plain functions, compiled for the host and the device alike.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_orc.h"
#include "../common/smc_layout.h"

namespace smo {

constexpr uint32_t kFragment = 65536;  // the raw codec's block: a longer piece is compressed by fragments
// the bytes a walk step looks at: a chunk header (3) and the payload's varint (<= 5)
constexpr uint32_t kHeadBytes = 8;

SMC_HD inline bool valid_block_size(uint32_t block_size) { return block_size >= 1 && block_size <= SMO_MAX_BLOCK_SIZE; }

struct Walk {
  uint64_t total = 0;    // declared uncompressed bytes so far
  uint32_t nchunks = 0;  // chunks so far
  int32_t status = SM_OK;
};

struct Chunk {
  uint64_t pay_off;
  uint32_t pay_len, ulen;
  bool original;
};

// One stream of n bytes.  fetch(pos, have, h) brings the `have` = min(kHeadBytes, n - pos) bytes at
// pos into h -- the only access to the stream, so no byte at n or behind it is read, whatever lies
// there; entry(k, at, c) gets chunk k, whose output starts at byte `at` of the stream's content.
template <typename Fetch, typename Entry>
SMC_HD inline Walk walk_chunks(uint32_t block_size, uint64_t n, Fetch fetch, Entry entry) {
  Walk w;
  uint64_t pos = 0;
  while (pos != n) {
    const uint32_t have = (uint32_t)(n - pos < kHeadBytes ? n - pos : kHeadBytes);
    uint8_t h[kHeadBytes];
    fetch(pos, have, h);
    if (have < SMO_HEADER_LENGTH) {
      w.status = SMO_ERR_TRUNCATED;
      break;
    }
    const uint32_t H = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16);
    const uint32_t L = H >> 1;
    const bool original = (H & 1u) != 0;
    if (L > n - pos - SMO_HEADER_LENGTH) {
      w.status = SMO_ERR_TRUNCATED;
      break;
    }
    uint32_t d = L, hv;  // (the varint's bytes lie inside the payload, so inside h[0, have))
    if (!original && smc::parse_varint32([&](uint32_t i) { return (uint32_t)h[SMO_HEADER_LENGTH + i]; }, L, d, hv) != 0) {
      w.status = SM_ERR_VARINT;
      break;
    }
    if (d > block_size) {
      w.status = SMO_ERR_CHUNK_TOO_LARGE;
      break;
    }
    const Chunk c{pos + SMO_HEADER_LENGTH, L, d, original};
    entry(w.nchunks, w.total, c);
    ++w.nchunks;
    w.total += d;
    pos += (uint64_t)SMO_HEADER_LENGTH + L;
  }
  return w;
}

// the walk's final status: its first structural error, else whether the entries fitted
SMC_HD inline int32_t walk_status(const Walk& w, bool stored, uint32_t max_chunks) {
  if (w.status != SM_OK) return w.status;
  return stored && w.nchunks > max_chunks ? SM_BUFFER_TOO_SMALL : SM_OK;
}

// the walk's fetch from a host buffer (bytes the stream does not have read as zero)
struct ByteFetch {
  const uint8_t* p;
  void operator()(uint64_t pos, uint32_t have, uint8_t* h) const {
    for (uint32_t i = 0; i < kHeadBytes; ++i) h[i] = i < have ? p[pos + i] : (uint8_t)0;
  }
};

// the 64 KiB fragments of a chunk that declares d bytes (smm_fragment_count)
SMC_HD inline uint64_t fragments(uint64_t d) { return d / kFragment + (d % kFragment ? 1 : 0); }

// ---- the encoder rule ---------------------------------------------------------------------------
// pieces of an n-byte input: block_size bytes each
SMC_HD inline uint64_t stream_pieces(uint64_t n, uint32_t block_size) { return n / block_size + (n % block_size ? 1 : 0); }

// a piece is stored when its raw stream of `comp` bytes is not shorter than it
SMC_HD inline bool piece_stored(uint32_t piece, uint32_t comp) { return comp >= piece; }

// Byte i (< 3) of the header of a chunk of L payload bytes.
SMC_HD inline uint8_t chunk_header_byte(uint32_t i, uint32_t L, bool original) {
  return (uint8_t)(((L << 1) | (original ? 1u : 0u)) >> (8 * i));
}

SMC_HD inline uint64_t max_length(uint64_t n, uint32_t block_size) {
  return n + SMO_HEADER_LENGTH * stream_pieces(n, block_size);
}

// the bound smm_compress_device gets on the pieces' fragments: only pieces above 64 KiB have any
SMC_HD inline uint64_t piece_fragment_bound(uint64_t max_pieces, uint32_t block_size) {
  return block_size > kFragment ? max_pieces * fragments(block_size) : 0;
}

const char* host_message(sm_status st);  // smo_host.cpp: the SMO_ERR_* texts, else NULL

}  // namespace smo
