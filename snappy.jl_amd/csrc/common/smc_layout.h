// smc_layout.h -- what the three libraries' host sides share about device memory layouts: the
// scratch carver and the companions' slot pitches.  Plain C++ (the host checkers compile it with
// the host compiler alone).  Not part of the public ABI.
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

// A 64 KiB block's output slot.  Two pitches, and they stay two (allocation sizes and the slots'
// alignment are behaviour): framing rounds the bound up to 16 bytes, multi takes the raw fragment
// compressor's slot (the bound + 8, rounded up to 256).
constexpr uint64_t kFramingSlotPitch = (max_compressed_length(65536) + 15) / 16 * 16;
constexpr uint64_t kMultiSlotPitch = (max_compressed_length(65536) + 8 + 255) / 256 * 256;
static_assert(kFramingSlotPitch == 76496 && kMultiSlotPitch == 76544, "the slot pitches are part of the layout");

}  // namespace smc
