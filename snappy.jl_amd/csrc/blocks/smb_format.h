// smb_format.h -- the rules of the two block containers (include/snappy_mi355x_blocks.h), shared by
// the host walkers (smb_host.cpp) and the one-wave device walkers (smb_kernels.hip): one walk,
// written once, so that all give the same status for the same stream; and the encoder rule's sizes.
// Plain functions, compiled for the host and the device alike.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_blocks.h"
#include "../common/smc_layout.h"

namespace smb {

constexpr uint32_t kBlock = 65536;            // the encoder's piece
constexpr uint32_t kMaxDeclared = 0x7fffffffu;  // a block or a chunk that declares more is refused
constexpr uint32_t kMagicWord = 0x82534e41u;  // a header's first four bytes, read as a length
// the bytes a walk step looks at: a XERIAL header (16), or a HADOOP block length (4), a chunk
// length (4) and the payload's varint (<= 5)
constexpr uint32_t kHeadBytes = 16;

SMC_HD inline bool valid_format(int format) { return format == SMB_FORMAT_HADOOP || format == SMB_FORMAT_XERIAL; }

SMC_HD inline uint32_t be32(const uint8_t* h) {
  return ((uint32_t)h[0] << 24) | ((uint32_t)h[1] << 16) | ((uint32_t)h[2] << 8) | (uint32_t)h[3];
}

struct Walk {
  uint64_t total = 0;    // declared uncompressed bytes so far
  uint32_t nchunks = 0;  // chunks so far
  int32_t status = SM_OK;
};

struct Chunk {
  uint64_t pay_off;
  uint32_t pay_len, ulen;
};

// A XERIAL header in h[0, have), of which `skip` leading bytes are known to match the magic (the
// repeated header's four were read as its length): 0 when it is good, else its status.  At the
// stream's start a mismatch is `mismatch` = SMB_ERR_NO_HEADER, behind it SMB_ERR_BAD_HEADER.
SMC_HD inline int32_t check_header(const uint8_t* h, uint32_t have, uint32_t skip, int32_t mismatch) {
  const uint8_t magic[8] = {0x82, 0x53, 0x4e, 0x41, 0x50, 0x50, 0x59, 0x00};
  if (skip == 0) {  // the first header: the bytes present decide between no header and a cut one
    if (have == 0) return mismatch;
    for (uint32_t i = 0; i < 8 && i < have; ++i)
      if (h[i] != magic[i]) return mismatch;
  }
  if (have < SMB_XERIAL_HEADER_LENGTH) return SMB_ERR_TRUNCATED;
  for (uint32_t i = skip; i < 8; ++i)
    if (h[i] != magic[i]) return mismatch;
  return be32(h + 8) == 0 ? (int32_t)SMB_ERR_BAD_HEADER : (int32_t)SM_OK;
}

// One stream of n bytes: the one walk of both formats.  fetch(pos, have, h) brings the `have` =
// min(kHeadBytes, n - pos) bytes at pos into h -- the only access to the stream, so no byte at n or
// behind it is read, whatever lies there; entry(k, at, c) gets chunk k, whose output starts at byte
// `at` of the stream's content.
template <typename Fetch, typename Entry>
SMC_HD inline Walk walk_blocks(int format, uint64_t n, Fetch fetch, Entry entry) {
  Walk w;
  const bool hadoop = format == SMB_FORMAT_HADOOP;
  uint64_t pos = 0;
  uint64_t need = 0;  // HADOOP: the bytes the current block's chunks have yet to declare
  bool start = !hadoop;  // XERIAL: the first header has not been read
  for (;;) {
    if (pos == n && !start && need == 0) break;  // (inside a HADOOP block the next chunk's length is cut: below)
    const uint32_t have = (uint32_t)(n - pos < kHeadBytes ? n - pos : kHeadBytes);
    uint8_t h[kHeadBytes];
    fetch(pos, have, h);
    if (start) {
      w.status = check_header(h, have, 0, SMB_ERR_NO_HEADER);
      if (w.status != SM_OK) break;
      start = false;
      pos = SMB_XERIAL_HEADER_LENGTH;
      continue;
    }
    uint32_t o = 0;  // the chunk's length field in h
    if (hadoop && need == 0) {
      if (have < 4) {
        w.status = SMB_ERR_TRUNCATED;
        break;
      }
      const uint32_t U = be32(h);
      if (U > kMaxDeclared) {
        w.status = SMB_ERR_CHUNK_TOO_LARGE;
        break;
      }
      if (U == 0) {  // an empty block: the walk goes on
        pos += 4;
        continue;
      }
      need = U;
      o = 4;
    }
    if (have < o + 4) {  // (o + 4 <= 8 < kHeadBytes: the stream ends here)
      w.status = SMB_ERR_TRUNCATED;
      break;
    }
    const uint32_t L = be32(h + o);
    if (!hadoop && L == kMagicWord) {  // a repeated header
      w.status = check_header(h, have, 4, SMB_ERR_BAD_HEADER);
      if (w.status != SM_OK) break;
      pos += SMB_XERIAL_HEADER_LENGTH;
      continue;
    }
    if (L > n - pos - o - 4) {
      w.status = SMB_ERR_TRUNCATED;
      break;
    }
    uint32_t d, hv;  // (the varint's bytes lie inside the payload, so inside h[0, have): o + 9 <= 13)
    if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)h[o + 4 + i]; }, L, d, hv) != 0) {
      w.status = SM_ERR_VARINT;
      break;
    }
    if (d > kMaxDeclared) {
      w.status = SMB_ERR_CHUNK_TOO_LARGE;
      break;
    }
    const Chunk c{pos + o + 4, L, d};
    entry(w.nchunks, w.total, c);
    ++w.nchunks;
    w.total += d;
    pos += (uint64_t)o + 4 + L;
    if (hadoop) {
      if (d > need) {
        w.status = SMB_ERR_BLOCK_LENGTH;
        break;
      }
      need -= d;
    }
  }
  return w;
}

// the walk's final status: its first structural error, else whether the entries fitted
SMC_HD inline int32_t walk_status(const Walk& w, bool stored, uint32_t max_chunks) {
  if (w.status != SM_OK) return w.status;
  return stored && w.nchunks > max_chunks ? SM_BUFFER_TOO_SMALL : SM_OK;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  void operator()(uint64_t pos, uint32_t have, uint8_t* h) const {
    for (uint32_t i = 0; i < have; ++i) h[i] = p[pos + i];
  }
};

// ---- the encoder rule ---------------------------------------------------------------------------
// pieces of an n-byte input: 64 KiB each
SMC_HD inline uint64_t stream_blocks(uint64_t n) { return n / kBlock + (n % kBlock ? 1 : 0); }
// what stands before a chunk's payload (HADOOP: the block's ulen and clen; XERIAL: clen), and before
// a stream's first chunk
SMC_HD inline uint32_t chunk_prefix(int format) { return format == SMB_FORMAT_HADOOP ? 8u : 4u; }
SMC_HD inline uint32_t stream_prefix(int format) { return format == SMB_FORMAT_HADOOP ? 0u : (uint32_t)SMB_XERIAL_HEADER_LENGTH; }

// Byte i of a stream's prefix: the XERIAL header -- or, of an empty HADOOP input, its one empty
// block (stream_fixed_bytes of them).
SMC_HD inline uint8_t stream_prefix_byte(int format, uint32_t i) {
  const uint8_t header[SMB_XERIAL_HEADER_LENGTH] = {0x82, 0x53, 0x4e, 0x41, 0x50, 0x50, 0x59, 0x00, 0, 0, 0, 1, 0, 0, 0, 1};
  return format == SMB_FORMAT_HADOOP ? (uint8_t)0 : header[i];
}
// the bytes of a stream of an n-byte input that are no chunk
SMC_HD inline uint32_t stream_fixed_bytes(int format, uint64_t n) {
  return format == SMB_FORMAT_HADOOP ? (n == 0 ? 4u : 0u) : (uint32_t)SMB_XERIAL_HEADER_LENGTH;
}

// Byte i of a chunk's prefix for a piece of `piece` bytes whose raw stream has `comp` bytes.
SMC_HD inline uint8_t chunk_prefix_byte(int format, uint32_t i, uint32_t piece, uint32_t comp) {
  const uint32_t v = (format == SMB_FORMAT_HADOOP && i < 4) ? piece : comp;
  return (uint8_t)(v >> (8 * (3 - (i & 3))));
}

SMC_HD inline uint64_t max_length(uint64_t n, int format) {
  const uint64_t full = n / kBlock, rest = n % kBlock;
  uint64_t sum = full * (smc::max_compressed_length(kBlock) + chunk_prefix(format));
  if (rest) sum += smc::max_compressed_length(rest) + chunk_prefix(format);
  return sum + stream_fixed_bytes(format, n);
}

const char* host_message(sm_status st);  // smb_host.cpp: the SMB_ERR_* texts, else NULL

}  // namespace smb
