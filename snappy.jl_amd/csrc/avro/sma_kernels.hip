// sma_kernels.hip -- a batch of Avro container streams per call (sma_uncompress_streams_device,
// sma_find_sync_device, sma_compress_streams_device): gfx950 kernels and their launchers
// (sma_internal.h).  Plumbing around the multi library's three device calls and the Parquet
// library's batched CRC-32, which run once over all blocks of all streams; the decisions are the
// shared rules of sma_format.h and sma_streams.h, taken per stream and per slot on the device, so a
// call needs no host synchronisation.  The sync search is the one parallel pass over the bytes here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "sma_format.h"
#include "sma_internal.h"
#include "sma_streams.h"

namespace sma {

namespace {

__device__ inline void store_block(const sma_blocks& t, uint32_t j, uint64_t at, const Block& b) {
  t.pay_off[j] = b.pay_off;
  t.pay_len[j] = b.pay_len;
  t.ulen[j] = b.ulen;
  t.count[j] = b.count;
  t.crc[j] = b.crc;
  t.out_off[j] = at;
}

}  // namespace

// ---- decode: the plan ----------------------------------------------------------------------------
// The counting walk, one wave per stream: what the stream gets (stream_plan) before any byte of it
// is decoded.  The walks of a workgroup's waves are independent: no barrier in here.
__global__ __launch_bounds__(256) void k_avro_count(DecodeStreamsArgs a) {
  const uint32_t r = smc::walker_index();
  if (r >= a.nstreams) return;
  smc::WindowFetch fetch{a.in + a.in_off[r], a.in_len[r], threadIdx.x & 63};
  const uint8_t* const marker = a.kind == SMA_INPUT_BLOCKS ? a.sync + (uint64_t)kSync * r : nullptr;
  const Walk w = walk_stream(a.kind, a.in_len[r], fetch, marker, [](uint32_t, uint64_t, const Block&) {});
  if (fetch.lane == 0) {
    const StreamPlan p = stream_plan(w, a.out_cap[r]);
    a.s.count[r] = p.slots;
    a.s.pre[r] = p.status;
    a.s.length[r] = p.length;
    a.s.objects[r] = p.objects;
    a.s.fail[r] = kNoSlot;
  }
}

// the exclusive scan of the streams' slots against the bound m, by one workgroup
__global__ __launch_bounds__(256) void k_avro_scan(DecodeStreamsArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.nstreams, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.first, a.block_first, a.s.hdr, sh);
}

// The slots no block took (all of them over the bound) become empty streams with no room, which
// the multi library's calls and the CRC call return from at once.  Then the storing walk of the
// streams that are decoded: block k of stream r is slot first[r] + k; its payload's offset is
// relative to d_in and its output's to d_out (the stream's place plus the declared lengths before
// it, the walk's own running total), its capacity the declared length.  The walk is the counting
// walk's over the same bytes; a slot past the stream's count is never stored.
__global__ __launch_bounds__(256) void k_avro_fill(DecodeStreamsArgs a) {
  for (uint64_t j = (uint64_t)a.s.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    a.s.in_off[j] = 0;
    a.s.out_off[j] = 0;
    a.s.crc_len[j] = 0;
    a.s.in_len[j] = 0;
    a.s.cap[j] = 0;
    a.s.stored[j] = 0;
    a.s.stream[j] = kNoSlot;
    if (a.table) store_block(a.blocks, (uint32_t)j, 0, Block{0, 0, 0, 0, 0});
  }
  const uint32_t r = smc::walker_index();
  if (r >= a.nstreams || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[r], base = a.s.first[r];
  if (cnt == 0) return;
  const uint64_t in_off = a.in_off[r], out_off = a.out_off[r];
  smc::WindowFetch fetch{a.in + in_off, a.in_len[r], threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  const uint8_t* const marker = a.kind == SMA_INPUT_BLOCKS ? a.sync + (uint64_t)kSync * r : nullptr;
  walk_stream(a.kind, a.in_len[r], fetch, marker, [&](uint32_t k, uint64_t at, const Block& b) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    a.s.in_off[j] = in_off + b.pay_off;
    a.s.out_off[j] = out_off + at;
    a.s.crc_len[j] = b.ulen;
    a.s.in_len[j] = b.pay_len;
    a.s.cap[j] = b.ulen;
    a.s.stored[j] = b.crc;
    a.s.stream[j] = r;
    if (a.table) store_block(a.blocks, j, at, b);
  });
}

hipError_t launch_decode_plan(const DecodeStreamsArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nstreams + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_avro_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_avro_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_avro_fill, dim3(walkers), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- decode: the results -------------------------------------------------------------------------
// A slot's verdict (slot_verdict); a failing one bids for its stream's first.
__global__ __launch_bounds__(256) void k_avro_verdict(DecodeStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t r = a.s.stream[j];
  const int32_t st = r == kNoSlot ? (int32_t)SM_OK
                                  : slot_verdict(a.s.dec_status[j], a.verify_crc != 0, a.s.stored[j],
                                                 a.verify_crc ? a.s.computed[j] : 0u);
  a.s.slot_status[j] = st;
  if (a.block_status) a.block_status[j] = st;
  if (st != SM_OK) atomicMin(&a.s.fail[r], j);
}

__global__ __launch_bounds__(256) void k_avro_result(DecodeStreamsArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nstreams) return;
  const bool over = a.s.hdr->over != 0;
  const uint32_t fail = over ? kNoSlot : a.s.fail[r];
  a.status[r] = smc::plan_verdict(over, a.s.pre[r], fail, fail != kNoSlot ? a.s.slot_status[fail] : (int32_t)SM_OK);
  a.out_len[r] = over ? 0 : a.s.length[r];
  if (a.objects) a.objects[r] = over ? 0 : a.s.objects[r];
}

hipError_t launch_decode_result(const DecodeStreamsArgs& a, hipStream_t s) {
  if (a.m) hipLaunchKernelGGL(k_avro_verdict, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_avro_result, dim3((a.nstreams + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- the sync search -----------------------------------------------------------------------------
namespace {

// The 16 bytes at offset p of the stream S[0, n) as two little-endian words.  S + p is a multiple of
// 16: a granule that lies wholly inside the stream comes by one aligned load, one that reaches
// over either end byte by byte, the bytes outside reading as zero without being read.
__device__ inline void load_granule(const uint8_t* S, uint64_t n, int64_t p, uint64_t& lo, uint64_t& hi) {
  if (p >= 0 && (uint64_t)p + 16 <= n) {
    struct {
      uint64_t w[2];
    } v;
    __builtin_memcpy(&v, __builtin_assume_aligned(S + p, 16), 16);
    lo = v.w[0];
    hi = v.w[1];
    return;
  }
  lo = 0;
  hi = 0;
  for (uint32_t i = 0; i < 16; ++i) {
    const int64_t at = p + (int64_t)i;
    const uint64_t b = at >= 0 && (uint64_t)at < n ? S[at] : 0u;
    if (i < 8) lo |= b << (8 * i);
    else hi |= b << (8 * (i - 8));
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_sync_init(FindSyncArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < a.nqueries) a.pos[q] = a.in_len[a.q_stream[q]];
}

// blockIdx.x = the query, blockIdx.y strides its tiles.  The searched range is cut at the 16-byte
// granules of the address space, from the granule that holds `from`: a thread takes one granule's 16
// candidates, which need that granule and the next one (its neighbour lane's, handed over by a
// shuffle; the wave's last lane loads its own) -- so a tile's last candidates look 15 bytes into the
// next tile, and a marker belongs to the one tile that holds its first byte.  A tile whose first
// byte lies behind the answer so far is not read: the answer only falls.
__global__ __launch_bounds__(256) void k_sync_search(FindSyncArgs a) {
  const uint32_t q = blockIdx.x;
  const uint32_t r = a.q_stream[q];
  const uint64_t n = a.in_len[r], from = a.q_from[q];
  if (n < kSync || from > n - kSync) return;  // (no room for a marker at or after `from`)
  const uint8_t* const S = a.in + a.in_off[r];
  const uint64_t last = n - kSync;  // the last candidate
  const Marker m = load_marker(a.sync + (uint64_t)kSync * r);
  // the first granule, relative to the stream: -15 .. from
  const int64_t g0 = (int64_t)from - (int64_t)(((uintptr_t)S + from) & 15);
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long* const best = (unsigned long long*)&a.pos[q];
  for (uint64_t t = blockIdx.y;; t += gridDim.y) {
    const int64_t tile = g0 + (int64_t)(t * kSearchTile);
    if (tile > (int64_t)last) break;
    if (tile > 0 && (uint64_t)tile > *(volatile unsigned long long*)best) break;
    for (uint32_t i = 0; i < kSearchTile / (16 * 256); ++i) {
      const int64_t first = tile + (int64_t)(16u * 256u * i);  // (uniform)
      if (first > (int64_t)last) break;
      const int64_t p0 = first + 16 * (int64_t)threadIdx.x;
      uint64_t w[4];
      load_granule(S, n, p0, w[0], w[1]);
      w[2] = __shfl_down(w[0], 1, 64);
      w[3] = __shfl_down(w[1], 1, 64);
      if (lane == 63) load_granule(S, n, p0 + 16, w[2], w[3]);
      uint64_t found = UINT64_MAX;
#pragma unroll
      for (uint32_t k = 16; k-- > 0;) {
        const int64_t p = p0 + (int64_t)k;
        if (p >= (int64_t)from && p <= (int64_t)last && marker_at(w, k, m)) found = (uint64_t)p;
      }
      if (found != UINT64_MAX) atomicMin(best, (unsigned long long)found);
    }
  }
}

hipError_t launch_find_sync(const FindSyncArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_sync_init, dim3((a.nqueries + 255) / 256), dim3(256), 0, s, a);
  // rows of tiles per query: enough workgroups for the device when the queries are few
  const uint32_t rows = a.nqueries >= 2048 ? 1u : 2048u / a.nqueries > 256u ? 256u : 2048u / a.nqueries;
  hipLaunchKernelGGL(k_sync_search, dim3(a.nqueries, rows), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress: the plan --------------------------------------------------------------------------
// By one workgroup: the blocks against max_blocks, the scan of their stage slots against
// stage_bytes, their fragments against max_fragments.  Over a bound nothing is compressed.
__global__ __launch_bounds__(256) void k_cavro_plan(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t total = a.block_first[a.nstreams];
  const uint32_t used = total > a.m ? 0u : total;
  uint64_t mine = 0;  // the fragments of this thread's blocks: a sum, not a scan
  const uint64_t stage = smc::tile_scan(
      used, sh,
      [&](uint32_t j) {
        const uint32_t len = a.block_len[j];
        mine += encode_fragments(len);
        return stage_length(len);
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.slot_off[j] = at; });
  uint64_t frags;
  (void)smc::block_scan(mine, sh, frags);
  for (uint32_t r = threadIdx.x; r < a.nstreams; r += 256) a.s.fail[r] = kNoSlot;
  if (threadIdx.x == 0) {
    const bool over = total > a.m || stage > a.stage_bytes || frags > a.max_fragments;
    a.s.hdr->over = over ? 1u : 0u;
    a.s.hdr->total = over ? 0u : total;
  }
}

// Slot j: its block, its stream.  An unused slot (all of them over a bound) is an empty block that
// packs nothing.
__global__ __launch_bounds__(256) void k_cavro_slots(CompressStreamsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const bool used = j < a.s.hdr->total;
  const uint32_t len = used ? a.block_len[j] : 0u;
  a.s.in_off[j] = used ? a.block_off[j] : 0u;
  a.s.in_len[j] = len;
  a.s.crc_len[j] = len;
  a.s.count[j] = used ? a.block_count[j] : 0u;
  a.s.stream[j] = used ? smc::slot_owner(a.block_first, a.nstreams, j) : kNoSlot;
  if (!used) a.s.slot_off[j] = a.stage_bytes;  // (the spare bytes behind the stage: an empty raw stream harms nothing there)
}

hipError_t launch_compress_plan(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cavro_plan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_cavro_slots, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress: the pack --------------------------------------------------------------------------
// The scan of the block sizes over all used slots, by one workgroup: a block's place in its stream
// is the stream's header plus its scan minus the scan at its stream's first block.  A block whose
// raw stream is missing bids for its stream's first failure: that stream is not written.
__global__ __launch_bounds__(256) void k_cavro_sizes(CompressStreamsArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        if (block_ok(a.s.comp_status[j], a.s.comp_len[j], a.s.in_len[j])) return block_bytes(a.s.count[j], a.s.comp_len[j]);
        atomicMin(&a.s.fail[a.s.stream[j]], j);
        return 0;
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.size_scan[j] = at; });
  if (threadIdx.x == 0) a.s.size_scan[used] = sum;
}

// blockIdx.x = the slot, blockIdx.y strides the payload; the first row also writes the two longs in
// front of it and the checksum (big-endian) and the marker behind it
__global__ __launch_bounds__(256) void k_cavro_pack(CompressStreamsArgs a) {
  const uint32_t j = blockIdx.x;
  if (j >= a.s.hdr->total) return;
  const uint32_t r = a.s.stream[j];
  if (r == kNoSlot || a.s.fail[r] != kNoSlot) return;
  const uint32_t c = a.s.comp_len[j];
  const int64_t count = (int64_t)a.s.count[j], size = (int64_t)c + 4;
  const uint32_t l1 = long_len(count), l2 = long_len(size);
  uint8_t* const d = a.out + a.out_off[r] + (a.head_len ? a.head_len[r] : 0u) + (a.s.size_scan[j] - a.s.size_scan[a.block_first[r]]);
  if (blockIdx.y == 0) {
    const uint32_t i = threadIdx.x;
    if (i < l1) d[i] = long_byte(count, i, l1);
    else if (i < l1 + l2) d[i] = long_byte(size, i - l1, l2);
    else if (i < l1 + l2 + 4) d[c + i] = (uint8_t)(a.s.crc[j] >> (8 * (3 - (i - l1 - l2))));
    else if (i < l1 + l2 + 4 + kSync) d[c + i] = a.sync[(uint64_t)kSync * r + (i - l1 - l2 - 4)];
  }
  smc::copy_bytes(a.s.stage + a.s.slot_off[j], c, d + l1 + l2, blockIdx.y * blockDim.x + threadIdx.x, gridDim.y * blockDim.x);
}

// A workgroup per stream (strided): its header copied in front, the length and the status; over a
// bound SM_ERR_ARGUMENT, no length and no byte; a stream with a failed block: that block's status
// (SM_ERR_DEVICE when the compressor reported none), no length and no byte.
__global__ __launch_bounds__(256) void k_cavro_result(CompressStreamsArgs a) {
  const bool over = a.s.hdr->over != 0;
  for (uint32_t r = blockIdx.x; r < a.nstreams; r += gridDim.x) {
    const uint32_t fail = over ? kNoSlot : a.s.fail[r];
    const bool write = !over && fail == kNoSlot;
    const uint64_t head = a.head_len ? a.head_len[r] : 0u;
    if (write && head) {
      const uint8_t* const src = a.in + a.head_off[r];
      uint8_t* const dst = a.out + a.out_off[r];
      for (uint64_t o = 0; o < head; o += 1u << 30) {
        const uint32_t len = head - o < (1u << 30) ? (uint32_t)(head - o) : 1u << 30;
        smc::copy_bytes(src + o, len, dst + o, threadIdx.x, blockDim.x);
      }
    }
    if (threadIdx.x == 0) {
      if (over) {
        a.status[r] = SM_ERR_ARGUMENT;
        a.out_len[r] = 0;
      } else if (fail != kNoSlot) {
        a.status[r] = a.s.comp_status[fail] != SM_OK ? a.s.comp_status[fail] : (int32_t)SM_ERR_DEVICE;
        a.out_len[r] = 0;
      } else {
        a.status[r] = SM_OK;
        a.out_len[r] = head + (a.s.size_scan[a.block_first[r + 1]] - a.s.size_scan[a.block_first[r]]);
      }
    }
  }
}

hipError_t launch_compress_pack(const CompressStreamsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cavro_sizes, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_cavro_pack, dim3(a.m, 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_cavro_result, dim3(a.nstreams < 1024 ? a.nstreams : 1024), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sma
