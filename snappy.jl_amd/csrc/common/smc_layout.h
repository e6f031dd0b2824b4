// smc_layout.h -- what the three libraries' host sides share about device memory layouts: the
// scratch carver and the companions' slot pitches -- and about the stream header: the varint32
// rule, once, for hosts and kernels alike.  Plain C++ (the host checkers compile it with the host
// compiler alone).  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SMC_HD __host__ __device__
#else
#define SMC_HD
#endif

namespace smc {

// Consecutive arrays of one scratch buffer, each rounded up to 16 bytes.  The base is an integer,
// so a null base measures: a layout is one carve_x(base, ...) that takes its arrays and records
// c.p as its end, and its size is carve_x(0, ...).end -- never a sum kept beside the carve.
// (constexpr for that use: measuring makes no pointer out of an integer.)
struct Carve {
  uintptr_t p;
  template <typename T>
  constexpr T* take(size_t n) {
    const uintptr_t at = p;
    p += (n * sizeof(T) + 15) / 16 * 16;
    return __builtin_is_constant_evaluated() ? nullptr : reinterpret_cast<T*>(at);
  }
};

SMC_HD constexpr uint64_t max_compressed_length(uint64_t n) { return 32 + n + n / 6; }  // src/Snappy.jl:80-82

// ---- the varint32 stream header (src/varint.jl) ----------------------------------------------
// bytes encode32! writes for v (varint.jl:46-69)
SMC_HD inline uint32_t varint_len(uint32_t v) {
  return v < (1u << 7) ? 1 : v < (1u << 14) ? 2 : v < (1u << 21) ? 3 : v < (1u << 28) ? 4 : 5;
}

// byte i (< nb) of the nb = varint_len(v) bytes encode32! writes for v: every emitter's one header
// rule, whichever thread or lane writes the byte (the caller has nb: it sized the header by it)
SMC_HD inline uint8_t varint_byte(uint32_t v, uint32_t i, uint32_t nb) {
  return (uint8_t)(((v >> (7 * i)) & 0x7f) | (i + 1 < nb ? 0x80 : 0));
}

// parse32 (varint.jl:12-37) over a byte accessor: at(i) is byte i of a header of which n bytes
// exist.  Returns 0 with the value and the header's length hv (1..5), or kErrVarint when the header
// is truncated, longer than 5 bytes or its 5th byte is 0x10 or more (value is then unspecified,
// hv 0).  Reads at(i) for i < min(n, 5) only, in order, and stops at the header's last byte.  Where
// the bytes come from -- a buffer at an offset, the lanes of a wave, a staged chunk head -- is the
// caller's business.
constexpr int32_t kErrVarint = 18;  // SM_ERR_VARINT (include/snappy_mi355x.h)
template <typename At>
SMC_HD inline int32_t parse_varint32(At at, uint32_t n, uint32_t& value, uint32_t& hv) {
  int32_t st = kErrVarint;
  value = 0;
  hv = 0;
  for (uint32_t i = 0; i < 5; ++i) {
    if (i >= n) break;
    const uint32_t b = at(i);
    if (i < 4) {
      value |= (b & 0x7f) << (7 * i);
      if (b < 0x80) {
        st = 0;
        hv = i + 1;
        break;
      }
    } else {
      value |= (b & 0x7f) << 28;
      if (b < 0x10) {
        st = 0;
        hv = 5;
      }
    }
  }
  return st;
}

// A varint64 (LevelDB's GetVarint64Ptr: a block handle's offset and size) over a byte accessor: up
// to 10 bytes of 7-bit groups, of which n exist.  Returns 0 with the value and its length (1..10),
// or kErrVarint when it runs past n or its 10th byte is above 1 (bits past the 64th, or an 11th
// byte).  Reads at(i) for i < min(n, 10) only, in order, and stops at the last byte.
template <typename At>
SMC_HD inline int32_t parse_varint64(At at, uint32_t n, uint64_t& value, uint32_t& len) {
  value = 0;
  len = 0;
  for (uint32_t i = 0; i < 10; ++i) {
    if (i >= n) break;
    const uint64_t b = at(i);
    if (i == 9) {
      if (b > 1) break;
      value |= b << 63;
      len = 10;
      return 0;
    }
    value |= (b & 0x7f) << (7 * i);
    if (b < 0x80) {
      len = i + 1;
      return 0;
    }
  }
  return kErrVarint;
}

// A 64 KiB block's output slot.  Two pitches, and they stay two (allocation sizes and the slots'
// alignment are behaviour): framing rounds the bound up to 16 bytes, multi takes the raw fragment
// compressor's slot (the bound + 8, rounded up to 256).
constexpr uint64_t kFramingSlotPitch = (max_compressed_length(65536) + 15) / 16 * 16;
constexpr uint64_t kMultiSlotPitch = (max_compressed_length(65536) + 8 + 255) / 256 * 256;
static_assert(kFramingSlotPitch == 76496 && kMultiSlotPitch == 76544, "the slot pitches are part of the layout");

}  // namespace smc
