// smq_device.h -- the device helpers the Parquet page library's kernels share (smq_kernels.hip,
// smq_encode.hip): the one-wave walkers' fetch, the tiled scan and the tiled copy.  All inline: they
// vanish into their callers.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smq_chunks.h"

namespace smq {

constexpr uint32_t kWalkWaves = 4;  // chunks a workgroup of the walkers takes: one per wave
constexpr uint32_t kWindow = 64;    // bytes of a chunk a wave holds: one per lane

// The walker's fetch (walk_pages), by one wave.  A page header is a run of variable-length fields
// of no fixed place, so the wave keeps a window of kWindow bytes of its chunk, a byte a lane, read
// by one load; fetch(pos) reads the byte out of its lane into a scalar register, so the parse --
// its arithmetic and its branches -- is the wave's, not a lane's.  When the cursor leaves the
// window (in either direction: the walk looks ahead at a section's varint) the window is read
// again from the cursor on: a header starts at any alignment and may span several windows, and a
// binary that is stepped over costs no load at all.  Bytes at or behind the chunk's end are not
// read (the reader never asks for them either).
struct WaveFetch {
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

// the chunk of this wave of walkers, as the wave's own value
__device__ inline uint32_t walker_chunk() {
  return __builtin_amdgcn_readfirstlane(blockIdx.x * kWalkWaves + (threadIdx.x >> 6));
}

// The exclusive scan of value(i), i < n, by one workgroup (block_scan's contract: 256 threads, sh
// its 4 u64 of LDS), tile by tile: each(i, value(i), the sum before i).  Returns the total to every thread.
template <typename Value, typename Each>
__device__ inline uint64_t tile_scan(uint32_t n, uint64_t* sh, Value value, Each each) {
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 256) {  // (uniform: every thread takes every tile)
    const uint32_t i = b0 + threadIdx.x;
    const uint64_t v = i < n ? value(i) : 0u;
    uint64_t total;
    const uint64_t ex = smc::block_scan(v, sh, total);
    if (i < n) each(i, v, carry + ex);
    carry += total;
  }
  return carry;
}

// n bytes from src to dst by this workgroup's row of the grid (copy_rows): tile t goes to row
// t mod gridDim.y.  A tile is a multiple of 16 bytes, so every tile of a slot meets the source at
// the same alignment; copy_bytes reads nothing outside [src, src + n) and writes nothing outside
// [dst, dst + n).
__device__ inline void copy_tiled(const uint8_t* src, uint32_t n, uint8_t* dst) {
  for (uint64_t o = (uint64_t)blockIdx.y * kCopyTile; o < n; o += (uint64_t)gridDim.y * kCopyTile) {
    const uint32_t len = n - o < kCopyTile ? (uint32_t)(n - o) : kCopyTile;
    smc::copy_bytes(src + o, len, dst + o, threadIdx.x, blockDim.x);
  }
}

}  // namespace smq
