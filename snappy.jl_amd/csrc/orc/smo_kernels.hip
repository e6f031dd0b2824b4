// smo_kernels.hip -- a batch of ORC compression streams per call (smo_uncompress_streams_device,
// smo_compress_streams_device): gfx950 kernels and their launchers (smo_internal.h).  Plumbing
// around the multi library's three device calls, which run once over all chunks of all streams, and
// the copies of the stored chunks; the decisions are the shared rules of smo_format.h and
// smo_streams.h, taken per stream and per slot on the device, so a call needs no host
// synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smo_format.h"
#include "smo_internal.h"
#include "smo_streams.h"

namespace smo {

namespace {

// the walkers' fetch (walk_chunks): a step's kHeadBytes, the little-endian header put together from them
using WaveFetch = smc::HeadFetch<kHeadBytes>;

}  // namespace

// ---- decode: the plan ----------------------------------------------------------------------------
// The counting walk, one wave per stream: what the stream gets (stream_plan) before any byte of it
// is decoded.  The walks of a workgroup's waves are independent: no barrier in here.
__global__ __launch_bounds__(256) void k_orc_count(DecodeStreamsArgs a) {
  const uint32_t r = smc::walker_index();
  if (r >= a.nstreams) return;
  const WaveFetch fetch{a.in + a.in_off[r], threadIdx.x & 63};
  const Walk w = walk_chunks(a.block_size, a.in_len[r], fetch, [](uint32_t, uint64_t, const Chunk&) {});
  if (fetch.lane == 0) {
    const StreamPlan p = stream_plan(w, a.out_cap[r]);
    a.s.count[r] = p.slots;
    a.s.pre[r] = p.status;
    a.s.length[r] = p.length;
    a.s.fail[r] = kNoSlot;
  }
}

__global__ __launch_bounds__(256) void k_orc_scan(DecodeStreamsArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.nstreams, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.first, a.chunk_first, a.s.hdr, sh);
}

// The slots no chunk took (all of them over the bound) become empty streams with no room, which
// the multi library's calls return from at once.  Then the storing walk of the streams that are
// decoded: chunk k of stream r is slot first[r] + k; its payload's offset is relative to d_in and its
// output's to d_out (the stream's place plus the declared lengths before it, the walk's own running
// total).  A compressed chunk's capacity is its declared length; a stored chunk stands before the
// raw decoder as an empty stream with no room, and its payload's length is the copy's.  The walk is
// the counting walk's over the same bytes; a slot past the stream's count is never stored.
__global__ __launch_bounds__(256) void k_orc_fill(DecodeStreamsArgs a) {
  for (uint64_t j = (uint64_t)a.s.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    a.s.in_off[j] = 0;
    a.s.out_off[j] = 0;
    a.s.in_len[j] = 0;
    a.s.cap[j] = 0;
    a.s.copy_len[j] = kNoCopy;
    a.s.stream[j] = kNoSlot;
  }
  const uint32_t r = smc::walker_index();
  if (r >= a.nstreams || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[r], base = a.s.first[r];
  if (cnt == 0) return;
  const uint64_t in_off = a.in_off[r], out_off = a.out_off[r];
  const WaveFetch fetch{a.in + in_off, threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_chunks(a.block_size, a.in_len[r], fetch, [&](uint32_t k, uint64_t at, const Chunk& c) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    a.s.in_off[j] = in_off + c.pay_off;
    a.s.out_off[j] = out_off + at;
    a.s.in_len[j] = c.original ? 0u : c.pay_len;
    a.s.cap[j] = c.original ? 0u : c.ulen;
    a.s.copy_len[j] = c.original ? c.pay_len : kNoCopy;
    a.s.stream[j] = r;
  });
}

hipError_t launch_decode_plan(const DecodeStreamsArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nstreams + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_orc_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_orc_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_orc_fill, dim3(walkers), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- decode: the stored chunks -------------------------------------------------------------------
// blockIdx.x strides the used slots, blockIdx.y a slot's tiles.  A stored chunk's payload goes from
// d_in straight to its place in d_out; the walk has checked that the payload lies inside its stream
// and the plan that the declared lengths fit the stream's room.
__global__ __launch_bounds__(256) void k_orc_copy(DecodeStreamsArgs a) {
  const uint32_t total = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
    const uint32_t n = a.s.copy_len[j];
    if (a.s.stream[j] == kNoSlot || n == kNoCopy) continue;
    smc::copy_tiled(a.in + a.s.in_off[j], n, a.out + a.s.out_off[j]);
  }
}

// ---- decode: the results -------------------------------------------------------------------------
// A slot's verdict (slot_verdict); a failing one bids for its stream's first.
__global__ __launch_bounds__(256) void k_orc_verdict(DecodeStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t r = a.s.stream[j];
  const int32_t st = slot_verdict(r, a.s.copy_len[j], a.s.dec_status[j]);
  if (a.chunk_status) a.chunk_status[j] = st;
  if (st != SM_OK) atomicMin(&a.s.fail[r], j);
}

__global__ __launch_bounds__(256) void k_orc_result(DecodeStreamsArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nstreams) return;
  const bool over = a.s.hdr->over != 0;
  const uint32_t fail = over ? kNoSlot : a.s.fail[r];
  a.status[r] = smc::plan_verdict(over, a.s.pre[r], fail, fail != kNoSlot ? a.s.dec_status[fail] : (int32_t)SM_OK);
  a.out_len[r] = over ? 0 : a.s.length[r];
}

hipError_t launch_decode_result(const DecodeStreamsArgs& a, hipStream_t s) {
  if (a.m) {
    hipLaunchKernelGGL(k_orc_copy, smc::copy_grid(a.m, a.block_size), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_orc_verdict, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_orc_result, dim3((a.nstreams + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress: the plan --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_corc_scan(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.nstreams, a.m, [&](uint32_t r) { return stream_pieces(a.in_len[r], a.block_size); }, a.s.first, nullptr,
             a.s.hdr, sh);
  for (uint32_t r = threadIdx.x; r < a.nstreams; r += 256) a.s.bad[r] = 0;
}

// Slot j: its stream, its block_size bytes of it and its output slot.  An unused slot (all of them
// over the bound) is an empty piece that packs nothing.
__global__ __launch_bounds__(256) void k_corc_pieces(CompressStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  uint64_t in_off = 0;
  uint32_t in_len = 0, stream = kNoSlot;
  if (j < a.s.hdr->total) {
    const uint32_t r = smc::slot_owner(a.s.first, a.nstreams, j);
    const uint64_t o = (uint64_t)(j - a.s.first[r]) * a.block_size, n = a.in_len[r];
    if (o < n) {  // (always, for the scan of these lengths)
      stream = r;
      in_off = a.in_off[r] + o;
      in_len = (uint32_t)(n - o < a.block_size ? n - o : a.block_size);
    }
  }
  a.s.in_off[j] = in_off;
  a.s.in_len[j] = in_len;
  a.s.slot_off[j] = (uint64_t)j * slot_pitch(a.block_size);
  a.s.stream[j] = stream;
}

hipError_t launch_compress_plan(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_corc_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_corc_pieces, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress: the pack --------------------------------------------------------------------------
// a piece whose raw stream is there and within its bound (else it packs nothing and marks its stream)
__device__ inline bool piece_ok(const CompressStreamsArgs& a, uint32_t j) {
  return a.s.comp_status[j] == SM_OK && a.s.comp_len[j] <= smc::max_compressed_length(a.s.in_len[j]);
}

// The choice per piece (piece_stored) and the scan of the chunk sizes over all used slots, by one
// workgroup: a chunk's place in its stream is its scan minus the scan at its stream's first piece.
__global__ __launch_bounds__(256) void k_corc_sizes(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        if (a.s.stream[j] == kNoSlot) return 0;
        if (piece_ok(a, j)) {
          const bool stored = piece_stored(a.s.in_len[j], a.s.comp_len[j]);
          a.s.stored[j] = stored ? 1 : 0;
          return (uint64_t)SMO_HEADER_LENGTH + (stored ? a.s.in_len[j] : a.s.comp_len[j]);
        }
        a.s.bad[a.s.stream[j]] = 1;  // (any writer: the same value)
        return 0;
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.size_scan[j] = at; });
  if (threadIdx.x == 0) a.s.size_scan[used] = sum;
}

// blockIdx.x strides the used slots, blockIdx.y a slot's tiles.  The header by byte stores; the
// payload from the raw compressor's slot, or of a stored piece from the input itself.
__global__ __launch_bounds__(256) void k_corc_pack(CompressStreamsArgs a) {
  const uint32_t total = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
    const uint32_t r = a.s.stream[j];
    if (r == kNoSlot || !piece_ok(a, j)) continue;
    const bool stored = a.s.stored[j] != 0;
    const uint32_t L = stored ? a.s.in_len[j] : a.s.comp_len[j];
    uint8_t* const d = a.out + a.out_off[r] + (a.s.size_scan[j] - a.s.size_scan[a.s.first[r]]);
    if (blockIdx.y == 0 && threadIdx.x < SMO_HEADER_LENGTH) d[threadIdx.x] = chunk_header_byte(threadIdx.x, L, stored);
    smc::copy_tiled(stored ? a.in + a.s.in_off[j] : a.slots + a.s.slot_off[j], L, d + SMO_HEADER_LENGTH);
  }
}

// Per stream: the length and the status; over the bound SM_ERR_ARGUMENT, no length and no byte.
__global__ __launch_bounds__(256) void k_corc_result(CompressStreamsArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nstreams) return;
  if (a.s.hdr->over) {
    a.status[r] = SM_ERR_ARGUMENT;
    a.out_len[r] = 0;
    return;
  }
  a.out_len[r] = a.s.size_scan[a.s.first[r + 1]] - a.s.size_scan[a.s.first[r]];
  a.status[r] = a.s.bad[r] ? SM_ERR_DEVICE : SM_OK;
}

hipError_t launch_compress_pack(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_corc_sizes, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_corc_pack, smc::copy_grid(a.m, a.block_size), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_corc_result, dim3((a.nstreams + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smo
