// smf_device.h -- the device helpers the framing kernels share (smf_kernels.hip, smf_range.hip,
// smf_streams.hip): the one-wave fetch of the chunk walk and the packing of one chunk (the scans are
// ../common/smc_device.h's).  All inline: they vanish into their callers.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smf_format.h"
#include "smf_slots.h"

namespace smf {

// base + off where off may stand for a place before base (the ranged decode's output offsets are
// relative to its edge slots: k_range_slots)
__device__ inline uint8_t* at(uint8_t* base, uint64_t off) { return (uint8_t*)((uintptr_t)base + off); }

// The walker's fetch (walk_stream), by one wave: a step's bytes (header, CRC, varint: kHeadBytes)
// come in by one load, a byte a lane, and every lane then takes the same step, so a chunk costs one
// dependent load.
struct WaveFetch {
  const uint8_t* in;
  uint32_t lane;
  __device__ void operator()(uint64_t pos, uint32_t have, uint8_t* h) const {
    const uint32_t mine = lane < have ? in[pos + lane] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < kHeadBytes; ++i) h[i] = (uint8_t)__shfl((int)mine, (int)i, smc::kWave);
  }
};

// The exclusive scan of cnt(r) over the groups against the bound m, by one workgroup: the shared
// count scan, under the name the framing kernels know it by.
template <typename Count>
__device__ inline void scan_counts(uint32_t ngroups, uint32_t m, Count cnt, uint32_t* first, uint32_t* first_out,
                                   GroupHeader* hdr, uint64_t* sh) {
  smc::count_scan(ngroups, m, cnt, first, first_out, hdr, sh);
}

// One chunk at d, by the workgroups (blockIdx.x, *) of k_frame_pack and k_streams_pack: the header
// and the CRC field, then the payload -- the block's Snappy stream (0x00) or the block (0x01);
// blockIdx.y strides the payload.  Nothing for a block with an error mark.
__device__ inline void pack_chunk(uint32_t type, const uint8_t* __restrict__ block, uint32_t n,
                                  const uint8_t* __restrict__ comp, uint32_t c, uint32_t crc, uint8_t* __restrict__ d) {
  if (type == kTypeNone) return;
  const uint32_t t = threadIdx.x;
  const uint32_t pl = type == SMF_CHUNK_COMPRESSED ? c : n;
  if (blockIdx.y == 0 && t < 8) {
    const uint32_t L = pl + 4;
    d[t] = t == 0 ? (uint8_t)type : (t < 4 ? (uint8_t)(L >> (8 * (t - 1))) : (uint8_t)(crc >> (8 * (t - 4))));
  }
  smc::copy_bytes(type == SMF_CHUNK_COMPRESSED ? comp : block, pl, d + 8, blockIdx.y * blockDim.x + t,
                  gridDim.y * blockDim.x);
}

}  // namespace smf
