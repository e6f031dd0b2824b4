// smc_device.h -- the device helpers the companion libraries' kernels share: the byte mover, the
// workgroup's scans, the one-wave walkers' fetches (but the framing library's, smf_device.h) and
// the tiled copy.  All inline: they vanish into their callers.  copy_bytes also compiles for the
// host, where the framing host checker runs it under sanitizers.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "smc_layout.h"
#include "smc_slots.h"

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

// The exclusive scan of value(i), i < n, by one workgroup (block_scan's contract: 256 threads, sh
// its 4 u64 of LDS), tile by tile: each(i, value(i), the sum before i).  Returns the total to every thread.
template <typename Value, typename Each>
__device__ inline uint64_t tile_scan(uint32_t n, uint64_t* sh, Value value, Each each) {
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 256) {  // (uniform: every thread takes every tile)
    const uint32_t i = b0 + threadIdx.x;
    const uint64_t v = i < n ? value(i) : 0u;
    uint64_t total;
    const uint64_t ex = block_scan(v, sh, total);
    if (i < n) each(i, v, carry + ex);
    carry += total;
  }
  return carry;
}

// The exclusive scan of cnt(r) over the groups against the bound m, by one workgroup: first[0,
// ngroups] (and first_out, if given) and the header's total and over (smc::PlanHeader, or a
// library's longer one).  Over the bound the scan is not used (it saturates).
template <typename Count, typename Hdr>
__device__ inline void count_scan(uint32_t ngroups, uint32_t m, Count cnt, uint32_t* first, uint32_t* first_out, Hdr* hdr,
                                  uint64_t* sh) {
  const uint64_t sum = tile_scan(ngroups, sh, cnt, [&](uint32_t r, uint64_t, uint64_t at) {
    first[r] = sat32(at);
    if (first_out) first_out[r] = sat32(at);
  });
  if (threadIdx.x == 0) {
    const bool over = sum > m;
    first[ngroups] = sat32(sum);
    if (first_out) first_out[ngroups] = sat32(sum);
    hdr->over = over ? 1u : 0u;
    hdr->total = over ? 0u : (uint32_t)sum;
  }
}

// ---- the one-wave walkers ------------------------------------------------------------------------
constexpr uint32_t kWalkWaves = 4;  // groups a workgroup of the walkers takes: one per wave
constexpr uint32_t kWindow = 64;    // bytes of its input a wave holds: one per lane

// the group of this wave of walkers, as the wave's own value (its loads of the group's arguments
// are then the wave's too)
__device__ inline uint32_t walker_index() {
  return __builtin_amdgcn_readfirstlane(blockIdx.x * kWalkWaves + (threadIdx.x >> 6));
}

// A walker's fetch of fixed heads, by one wave: a step's bytes (HeadBytes of them) come in by one
// load, a byte a lane, and every lane then takes the same step, so a chunk costs one dependent
// load.  The bytes are read out of their lanes into scalar registers, so the step's arithmetic and
// its branches are the wave's, not a lane's.  Multi-byte fields are put together from these bytes:
// a stream sits at any alignment.
template <uint32_t HeadBytes>
struct HeadFetch {
  const uint8_t* in;
  uint32_t lane;
  __device__ void operator()(uint64_t pos, uint32_t have, uint8_t* h) const {
    const uint32_t mine = lane < have ? in[pos + lane] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < HeadBytes; ++i) h[i] = (uint8_t)__builtin_amdgcn_readlane((int)mine, (int)i);
  }
};

// A walker's fetch of variable-length fields of no fixed place, by one wave: the wave keeps a
// window of kWindow bytes of its input, a byte a lane, read by one load; fetch(pos) reads the byte
// out of its lane into a scalar register, so the parse -- its arithmetic and its branches -- is the
// wave's, not a lane's.  When the cursor leaves the window (in either direction) the window is read
// again from the cursor on: a field starts at any alignment and may span several windows, and bytes
// that are stepped over cost no load at all.  Bytes at or behind the input's end are not read.
struct WindowFetch {
  const uint8_t* in;
  uint64_t n;
  uint32_t lane;
  uint64_t base = 0;
  uint32_t mine = 0;
  bool valid = false;
  __device__ uint32_t operator()(uint64_t pos) {
    if (!valid || pos < base || pos - base >= kWindow) {
      base = pos;
      mine = base + lane < n ? in[base + lane] : 0u;
      valid = true;
    }
    const uint32_t at = __builtin_amdgcn_readfirstlane((uint32_t)(pos - base));
    return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)at) & 0xffu;
  }
};

// ---- the tiled copy ------------------------------------------------------------------------------
// n bytes from src to dst by this workgroup's row of the grid (copy_rows): tile t goes to row
// t mod gridDim.y.  A tile is a multiple of 16 bytes, so every tile of a slot meets the source at
// the same alignment; copy_bytes reads nothing outside [src, src + n) and writes nothing outside
// [dst, dst + n).
__device__ inline void copy_tiled(const uint8_t* src, uint32_t n, uint8_t* dst) {
  for (uint64_t o = (uint64_t)blockIdx.y * kCopyTile; o < n; o += (uint64_t)gridDim.y * kCopyTile) {
    const uint32_t len = n - o < kCopyTile ? (uint32_t)(n - o) : kCopyTile;
    copy_bytes(src + o, len, dst + o, threadIdx.x, blockDim.x);
  }
}

// the copies' grid: a workgroup a used slot (striding, where the bound is far above what a device
// holds at once) in x, the rows of a slot's tiles in y
inline dim3 copy_grid(uint32_t m, uint32_t longest) {
  return dim3(m < 8 * kCopyGroups ? m : 8 * kCopyGroups, copy_rows(m, longest));
}

#endif  // __HIPCC__

}  // namespace smc
