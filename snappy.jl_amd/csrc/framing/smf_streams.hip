// smf_streams.hip -- a batch of framed streams per call (smf_uncompress_streams_device,
// smf_compress_streams_device): gfx950 kernels and their launchers (smf_internal.h).  Plumbing
// around the raw codec's batched calls and k_crc32c, which run once over all chunks of all streams;
// the decisions are the shared rules of smf_streams.h and smf_format.h, taken per stream and per
// slot on the device, so a call needs no host synchronisation.  The decode's slot stage
// behind the plan is the shared one (smf_slots.h); the walk's fetch and the scans are smf_device.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smf_device.h"
#include "smf_format.h"
#include "smf_internal.h"
#include "smf_streams.h"

namespace smf {

namespace {

using smc::block_scan;

constexpr uint32_t kWalkWaves = 4;  // streams a workgroup of the walkers takes: one per wave

}  // namespace

// ---- decode: the plan ----------------------------------------------------------------------------
// The counting walk, one wave per stream: what the stream gets (stream_plan) before any byte of it
// is decoded.  The walks of a workgroup's waves are independent: no barrier in here.
__global__ __launch_bounds__(256) void k_streams_count(DecodeStreamsArgs a) {
  const uint32_t r = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (r >= a.nstreams) return;
  const WaveFetch fetch{a.in + a.in_off[r], threadIdx.x & 63};
  const Walk w = walk_stream(a.in_len[r], fetch, [](uint32_t, uint64_t, const Chunk&) {});
  if (fetch.lane == 0) {
    const StreamPlan p = stream_plan(w, a.out_cap[r]);
    a.s.count[r] = p.slots;
    a.s.pre[r] = p.status;
    a.s.length[r] = p.length;
    a.s.slots.fail[r] = kNoSlot;
  }
}

__global__ __launch_bounds__(256) void k_streams_scan(DecodeStreamsArgs a) {
  __shared__ uint64_t sh[4];
  scan_counts(a.nstreams, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.first, a.chunk_first, a.s.hdr, sh);
}

// The storing walk of the streams that are decoded: data chunk k of stream r is slot first[r] + k.
// Its payload's offset is relative to d_in and its output's to d_out (the stream's place plus the
// declared lengths before it, the walk's own running total), so the raw decoder, the copy and the
// CRC pass each run once over all slots.  cap = the declared length: the raw decoder's capacity and
// the CRC pass's length; dec_len = the payload's length for a 0x00 chunk, else 0 (the raw decoder
// returns at once on an empty stream).  The walk is the counting walk's over the same bytes; a slot
// past the stream's count is never stored.
__global__ __launch_bounds__(256) void k_streams_fill(DecodeStreamsArgs a) {
  const uint32_t r = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (r >= a.nstreams || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[r], base = a.s.first[r];
  if (cnt == 0) return;
  const uint64_t in_off = a.in_off[r], out_off = a.out_off[r];
  const WaveFetch fetch{a.in + in_off, threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_stream(a.in_len[r], fetch, [&](uint32_t k, uint64_t at, const Chunk& c) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    a.s.slots.type[j] = c.type;
    a.s.slots.in_off[j] = in_off + c.pay_off;
    a.s.slots.crc_want[j] = c.crc;
    a.s.slots.out_off[j] = out_off + at;
    a.s.slots.cap[j] = c.ulen;
    a.s.slots.dec_len[j] = c.type == SMF_CHUNK_COMPRESSED ? c.pay_len : 0u;
    a.s.slots.group[j] = r;
  });
}

// The slots no chunk took (all of them over the bound): empty streams with no room, which the raw
// decoder returns from at once and nothing else touches.
__global__ __launch_bounds__(256) void k_streams_unused(DecodeStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m || j < a.s.hdr->total) return;
  a.s.slots.type[j] = SMF_CHUNK_COMPRESSED;
  a.s.slots.in_off[j] = 0;
  a.s.slots.crc_want[j] = 0;
  a.s.slots.out_off[j] = 0;
  a.s.slots.cap[j] = 0;
  a.s.slots.dec_len[j] = 0;
  a.s.slots.group[j] = kNoSlot;
}

hipError_t launch_streams_plan(const DecodeStreamsArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nstreams + kWalkWaves - 1) / kWalkWaves;
  hipLaunchKernelGGL(k_streams_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_streams_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) {
    hipLaunchKernelGGL(k_streams_fill, dim3(walkers), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_streams_unused, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// ---- compress: the plan --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cstreams_scan(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  scan_counts(a.nstreams, a.m, [&](uint32_t r) { return stream_blocks(a.in_len[r]); }, a.s.first, nullptr, a.s.hdr, sh);
  for (uint32_t r = threadIdx.x; r < a.nstreams; r += 256) a.s.bad[r] = 0;
}

// Slot j: its stream (a search in the scanned counts; of equal entries the last one, so streams
// without blocks are passed over), its 64 KiB of it and its output slot.  An unused slot (all of
// them over the bound) is an empty block that packs nothing.
__global__ __launch_bounds__(256) void k_cstreams_blocks(CompressStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  uint64_t in_off = 0;
  uint32_t in_len = 0, stream = kNoSlot;
  if (j < a.s.hdr->total) {
    const uint32_t r = upper_bound(a.s.first, a.nstreams + 1, j) - 1;  // first[r] <= j < first[r + 1]
    const uint64_t o = (uint64_t)(j - a.s.first[r]) * kBlock, n = a.in_len[r];
    if (r < a.nstreams && o < n) {  // (always, for the scan of these lengths)
      stream = r;
      in_off = a.in_off[r] + o;
      in_len = (uint32_t)(n - o < kBlock ? n - o : kBlock);
    }
  }
  a.s.in_off[j] = in_off;
  a.s.in_len[j] = in_len;
  a.s.slot_off[j] = (uint64_t)j * smc::kFramingSlotPitch;
  a.s.stream[j] = stream;
  a.s.type[j] = kTypeNone;
}

hipError_t launch_cstreams_plan(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cstreams_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_cstreams_blocks, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress: the pack --------------------------------------------------------------------------
// The encoder rule (encoder_chunk, as k_frame_scan) and the scan of the chunk sizes over all used
// slots, by one workgroup: a chunk's place in its stream is 10 plus its scan minus the scan at its
// stream's first block.  An error mark packs nothing and marks its stream.
__global__ __launch_bounds__(256) void k_cstreams_sizes(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < used; base += 256) {  // (uniform: every thread takes every tile)
    const uint32_t j = base + threadIdx.x;
    uint64_t size = 0;
    if (j < used && a.s.stream[j] != kNoSlot) {
      uint8_t ty;
      size = encoder_chunk(a.s.comp_len[j], a.s.in_len[j], ty);
      a.s.type[j] = ty;
      if (ty == kTypeNone) a.s.bad[a.s.stream[j]] = 1;  // (any writer: the same value)
    }
    uint64_t total;
    const uint64_t ex = block_scan(size, sh, total);
    if (j < used) a.s.size_scan[j] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.s.size_scan[used] = carry;
}

// blockIdx.x = the slot, blockIdx.y strides the payload
__global__ __launch_bounds__(256) void k_streams_pack(CompressStreamsArgs a) {
  const uint32_t j = blockIdx.x;
  const uint32_t r = a.s.stream[j];
  if (r == kNoSlot) return;
  uint8_t* const d = a.out + a.out_off[r] + SMF_IDENTIFIER_LENGTH + (a.s.size_scan[j] - a.s.size_scan[a.s.first[r]]);
  pack_chunk(a.s.type[j], a.in + a.s.in_off[j], a.s.in_len[j], a.slots + a.s.slot_off[j], a.s.comp_len[j], a.s.crc[j], d);
}

// Per stream: the identifier, the length and the status; over the bound SM_ERR_ARGUMENT, no length
// and no byte.
__global__ __launch_bounds__(256) void k_cstreams_result(CompressStreamsArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nstreams) return;
  if (a.s.hdr->over) {
    a.status[r] = SM_ERR_ARGUMENT;
    a.out_len[r] = 0;
    return;
  }
  const uint8_t id[SMF_IDENTIFIER_LENGTH] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
  uint8_t* const d = a.out + a.out_off[r];
  for (uint32_t i = 0; i < SMF_IDENTIFIER_LENGTH; ++i) d[i] = id[i];
  a.out_len[r] = SMF_IDENTIFIER_LENGTH + (a.s.size_scan[a.s.first[r + 1]] - a.s.size_scan[a.s.first[r]]);
  a.status[r] = a.s.bad[r] ? SM_ERR_DEVICE : SM_OK;
}

hipError_t launch_cstreams_pack(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cstreams_sizes, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_streams_pack, dim3(a.m, 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_cstreams_result, dim3((a.nstreams + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smf
