// smc_device.h -- the device helpers the companion libraries' kernels share (smf_kernels.hip,
// smf_range.hip, smm_kernels.hip).  All inline: they vanish into their callers.  copy_bytes also
// compiles for the host, where the framing host checker runs it under sanitizers.
// Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smc_layout.h"

#if !defined(__HIPCC__)
#include <assert.h>
#endif

namespace smc {

// n bytes from src to dst, both at any alignment, by `nthreads` threads of which this is `tid`:
// aligned 16-byte loads of the granules src wholly covers, bytes for the partial granules at both
// ends (no byte outside [src, src + n) is read), stores at dst's alignment (none outside
// [dst, dst + n)).
SMC_HD inline void copy_bytes(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ dst, uint32_t tid,
                              uint32_t nthreads) {
  const uint32_t to_granule = (16u - (uint32_t)((uintptr_t)src & 15)) & 15u;
  const uint32_t head = n < to_granule ? n : to_granule;
  const uint32_t G = (n - head) / 16;
  const uint8_t* const g = src + head;
  for (uint32_t u = tid; u < G; u += nthreads) {
#if !defined(__HIPCC__)
    assert(((uintptr_t)(g + 16 * (size_t)u) & 15) == 0 && g + 16 * (size_t)u >= src);
#endif
    struct {
      uint32_t w[4];
    } v;
    __builtin_memcpy(&v, __builtin_assume_aligned(g + 16 * (size_t)u, 16), 16);
    __builtin_memcpy(dst + head + 16 * u, &v, 16);
  }
  const uint32_t edge = n - 16 * G;  // head bytes, then the tail's
  for (uint32_t i = tid; i < edge; i += nthreads) {
    const uint32_t j = i < head ? i : 16 * G + i;
    dst[j] = src[j];
  }
}

#if defined(__HIPCC__)

constexpr uint32_t kWave = 64;

// Exclusive scan of v over the workgroup; total = the sum.  The contract: the workgroup is 256
// threads in x (four waves), every one of them calls, and sh is 4 u64 of LDS that only
// block_scan touches (consecutive calls may share it: the first barrier orders them).
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* sh, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = v;
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint64_t o = __shfl_up(inc, d, kWave);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // (sh is free again)
  if (lane == kWave - 1) sh[w] = inc;
  __syncthreads();
  uint64_t pre = 0;
  for (uint32_t k = 0; k < w; ++k) pre += sh[k];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  return pre + inc - v;
}

__device__ inline uint32_t sat32(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

#endif  // __HIPCC__

}  // namespace smc
