// sm_format.h -- the snappy raw format's constants and rules as plain C++ (no HIP header): what
// the kernels (through sm_device.h), the host rules (sm_host_rules.h) and the host checker share.
// Format rules follow the reference's src/internal.jl:15-85 and src/varint.jl; nothing here is
// transcribed from the reference's tables (CHAR_TABLE is derived from the tag rules in
// char_entry()).
#pragma once
#include <stdint.h>

#include "common/smc_layout.h"

namespace sm {

constexpr uint32_t kBlockSize = 65536;        // internal.jl:31
constexpr uint32_t kInputMarginBytes = 15;    // internal.jl:32
constexpr uint32_t kMaxHashTableSize = 16384; // internal.jl:33
constexpr uint32_t kHashMul = 0x1e35a7bdu;    // internal.jl:94
constexpr int kWave = 64;

// status codes (mirror include/snappy_mi355x.h)
enum : int32_t {
  kOk = 0,
  kInvalidInput = 1,
  kBufferTooSmall = 2,
  kErrInputTooLarge = 16,
  kErrInvalid = 17,
  kErrVarint = 18,
  kErrCopyOffset = 19,
  kErrCopyLength = 20,
  kErrLiteral = 21,
  kErrDevice = 32,  // SM_ERR_DEVICE: a block length that is a compressor error mark (>= kOutLenError)
  kErrCross = 64,  // internal: a fragment's copy reads another fragment (never returned by the ABI)
};

SMC_HD inline uint32_t max_compressed_length(uint32_t n) { return 32 + n + n / 6; }

// SM_OUT_LEN_ERROR: a compressor's error mark in d_out_len (include/snappy_mi355x.h).  A device
// decoder handed such a length (a caller passing comp_len straight on) reports kErrDevice without
// reading the slot: the mark is an error, never a stream length (Snappy.jl:50 raises, never decodes).
constexpr uint32_t kOutLenError = 0xfff00000u;

// internal.jl:107-113
SMC_HD inline uint32_t hashtable_size(uint64_t n) {
  uint32_t ht = 256;
  while (ht < kMaxHashTableSize && ht < n) ht <<= 1;
  return ht;
}

// internal.jl:35-46 layout: bits 0-7 length, 8-10 copy offset>>8, 11-13 extra bytes.
SMC_HD inline uint32_t char_entry(uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  // branch-free on the device: the kind-switch compiles to a divergent branch tree that a wave of
  // mixed tags runs every arm of (exec masks, ~16 SALU); these are selects on the same values
  const uint32_t kind = c & 3, hi = c >> 2;
  const uint32_t tlc = __builtin_amdgcn_perm(0u, 0x04020100u, kind);  // copy tag bytes 1/2/4 (kind 0: 0)
  const uint32_t lit = hi < 60 ? hi + 1 : (((hi - 59) << 11) | 1);
  const uint32_t cp1 = (1u << 11) | ((c >> 5) << 8) | (4 + (hi & 7));
  const uint32_t cpx = (tlc << 11) | (hi + 1);
  return kind == 0 ? lit : (kind == 1 ? cp1 : cpx);
#else
  uint32_t kind = c & 3, hi = c >> 2;
  if (kind == 0) return hi < 60 ? hi + 1 : (((hi - 59) << 11) | 1);
  if (kind == 1) return (1u << 11) | ((c >> 5) << 8) | (4 + ((c >> 2) & 7));
  if (kind == 2) return (2u << 11) | (hi + 1);
  return (4u << 11) | (hi + 1);
#endif
}

SMC_HD inline uint32_t varint_len(uint32_t v) {
  return v < (1u << 7) ? 1 : v < (1u << 14) ? 2 : v < (1u << 21) ? 3 : v < (1u << 28) ? 4 : 5;
}

// bytes of the literal tag for a run of len (>0) bytes (internal.jl:271-284)
SMC_HD inline uint32_t literal_tag_bytes(uint32_t len) {
  uint32_t n = len - 1;
  return n < 60 ? 1 : n < 256 ? 2 : n < 65536 ? 3 : n < (1u << 24) ? 4 : 5;
}

// bytes emit_copy! (internal.jl:306-329) produces for (offset, len)
SMC_HD inline uint32_t copy_tag_bytes(uint32_t offset, uint32_t len) {
  if (len < 12) return (offset < 2048) ? 2 : 3;
  uint32_t b = 0;
  while (len >= 68) { b += 3; len -= 64; }
  if (len > 64) { b += 3; len -= 60; }
  return b + ((len < 12 && offset < 2048) ? 2 : 3);
}

}  // namespace sm
