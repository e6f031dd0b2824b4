// smk_kernels.hip -- batches of Kafka log segments (smk_uncompress_segments_device,
// smk_compress_segments_device): gfx950 kernels and their launchers (smk_internal.h).  Plumbing
// around the blocks library's two device calls (the snappy-java stream), the multi library's index
// builder and decoder (raw streams) and the framing library's batched CRC-32C; the decisions are the
// shared rules of smk_format.h, taken per segment and per batch on the device, so a call needs no
// host synchronisation.  A segment is one serial walk by one wave; once its batches are known,
// every batch's head, slot, header and verdict is a thread's (or a workgroup's) own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smk_format.h"
#include "smk_internal.h"

namespace smk {

namespace {

constexpr uint32_t kLongest = 1u << 20;  // the payload the copies' rows are sized for (a longer one is strided)

// a thread's own bytes of global memory, one load each, at any alignment
struct DeviceBytes {
  const uint8_t* p;
  __device__ uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

__device__ inline Batch batch_of(const Batches& b, uint32_t j) { return Batch{b.pos[j], b.length[j], b.codec[j]}; }

// the segment of slot j, kNoSlot for a slot no batch took
__device__ inline uint32_t segment_of(const WalkArgs& w, uint32_t j) { return j < w.hdr->total ? w.b.segment[j] : kNoSlot; }

}  // namespace

// ---- the walks -----------------------------------------------------------------------------------
// The counting walk, one wave per segment.  The walks of a workgroup's waves are independent: no
// barrier in here.
__global__ __launch_bounds__(256) void k_kafka_count(WalkArgs a) {
  const uint32_t r = smc::walker_index();
  if (r >= a.ns) return;
  smc::WindowFetch fetch{a.in + a.in_off[r], a.in_len[r], threadIdx.x & 63};
  const Walk w = walk_segment(fetch, a.in_len[r], [](uint32_t, const Batch&) {});
  if (fetch.lane == 0) {
    a.g.count[r] = w.nbatches;
    a.g.walk[r] = w.status;
    a.g.fail[r] = kNoSlot;
  }
}

// the exclusive scan of the segments' batches against the bound m, by one workgroup
__global__ __launch_bounds__(256) void k_kafka_scan(WalkArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.ns, a.m, [&](uint32_t r) { return a.g.count[r]; }, a.g.first, a.batch_first, a.hdr, sh);
}

// The slots no batch took (all of them over the bound) are marked; then the storing walk: batch k
// of segment r is slot first[r] + k.  The walk is the counting walk's over the same bytes; a slot
// past the segment's count is never stored.
__global__ __launch_bounds__(256) void k_kafka_fill(WalkArgs a) {
  for (uint64_t j = (uint64_t)a.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    a.b.pos[j] = 0;
    a.b.length[j] = kMinLength;
    a.b.codec[j] = 0;
    a.b.segment[j] = kNoSlot;
  }
  const uint32_t r = smc::walker_index();
  if (r >= a.ns || a.hdr->over) return;
  const uint32_t cnt = a.g.count[r], base = a.g.first[r];
  if (cnt == 0) return;
  smc::WindowFetch fetch{a.in + a.in_off[r], a.in_len[r], threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_segment(fetch, a.in_len[r], [&](uint32_t k, const Batch& b) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    a.b.pos[j] = b.pos;
    a.b.length[j] = b.length;
    a.b.codec[j] = b.codec;
    a.b.segment[j] = r;
  });
}

hipError_t launch_walk(const WalkArgs& w, hipStream_t s) {
  const uint32_t walkers = (w.ns + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_kafka_count, dim3(walkers), dim3(256), 0, s, w);
  hipLaunchKernelGGL(k_kafka_scan, dim3(1), dim3(256), 0, s, w);
  if (w.m) hipLaunchKernelGGL(k_kafka_fill, dim3(walkers), dim3(256), 0, s, w);
  return hipGetLastError();
}

// ---- decode: the heads ---------------------------------------------------------------------------
// A thread per slot: the batch's head -- at most eight bytes of its payload -- and the four of its
// checksum, at any alignment, all inside the segment's range (the walk checked the batch against
// it).  A snappy-java batch becomes a stream of the blocks library's call with no room, which
// reports its size and decodes nothing; every other slot is an empty stream there.
__global__ __launch_bounds__(256) void k_kafka_head(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m) return;
  Head h{kStored, 0, SM_OK};
  uint32_t stored = 0;
  uint64_t x_off = 0, x_len = 0;
  const uint32_t t = segment_of(a.w, j);
  if (t != kNoSlot) {
    DeviceBytes fetch{a.w.in + a.w.in_off[t]};
    const Batch b = batch_of(a.w.b, j);
    h = batch_head(fetch, b);
    stored = be32(fetch, b.pos + kCrcAt);
    if (h.kind == kXerial) {
      x_off = a.w.in_off[t] + b.pos + kHeader;
      x_len = b.length - kMinLength;
    }
  }
  a.s.kind[j] = h.kind;
  a.s.decl[j] = h.declared;
  a.s.head[j] = h.status;
  a.s.stored[j] = stored;
  a.s.x_in_off[j] = x_off;
  a.s.x_in_len[j] = x_len;
  a.s.x_out_off[j] = 0;
  a.s.x_cap[j] = 0;
  a.s.x_len[j] = 0;
  a.s.x_status[j] = SM_OK;
}

hipError_t launch_heads(const DecodeArgs& a, hipStream_t s) {
  if (a.w.m) hipLaunchKernelGGL(k_kafka_head, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- decode: the plan ----------------------------------------------------------------------------
// By one workgroup: the snappy-java batches' heads from the sizing call (xerial_head), every failing
// head's bid for its segment's first, and the scan of the rewritten lengths over all recorded
// batches.  More chunks than the bound, by that call's word, is the whole call's.
__global__ __launch_bounds__(256) void k_kafka_sizes(DecodeArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.w.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        int32_t st = a.s.head[j];
        uint32_t d = a.s.decl[j];
        if (a.s.kind[j] == kXerial) {
          st = xerial_head(a.s.x_status[j], a.s.x_len[j], d);
          if (st == SM_ERR_ARGUMENT) a.w.hdr->over = 1u;  // (any writer: the same value)
          a.s.head[j] = st;
          a.s.decl[j] = d;
        }
        if (st != SM_OK) atomicMin(&a.w.g.fail[a.w.b.segment[j]], j);
        return st == SM_OK ? rewritten_length(d) : 0u;
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.prefix[j] = at; });
  if (threadIdx.x == 0) a.s.prefix[used] = sum;
}

// A thread per segment: its status before any byte is written (segment_plan) and its length -- the
// rewritten lengths of its batches, or of those before its first failing head.
__global__ __launch_bounds__(256) void k_kafka_plan(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.w.ns) return;
  if (a.w.hdr->over) {
    a.w.g.pre[t] = SM_ERR_ARGUMENT;
    a.out_len[t] = 0;
    return;
  }
  const uint32_t lo = a.w.g.first[t], hi = a.w.g.first[t + 1], f = a.w.g.fail[t];
  const uint64_t sum = a.s.prefix[f != kNoSlot ? f : hi] - a.s.prefix[lo];
  a.w.g.pre[t] = segment_plan(a.w.g.walk[t], f != kNoSlot ? a.s.head[f] : (int32_t)SM_OK, sum, a.out_cap[t]);
  a.out_len[t] = sum;
  a.w.g.fail[t] = kNoSlot;  // (from here on: the first batch whose decode or checksum fails)
}

// A thread per slot: the batch's arguments for the three decoders' calls, the copy and the two
// checksum calls, and the caller's per-batch arrays.  A batch that is not written is an empty stream
// with no room everywhere, which those calls return from at once.
__global__ __launch_bounds__(256) void k_kafka_place(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m) return;
  const bool over = a.w.hdr->over != 0;
  const uint32_t t = over ? kNoSlot : segment_of(a.w, j);
  const bool live = t != kNoSlot && a.w.g.pre[t] == SM_OK;
  const Batch b = batch_of(a.w.b, j);
  const uint32_t kind = a.s.kind[j], d = a.s.decl[j], p = b.length - kMinLength;
  const uint64_t rel = t != kNoSlot ? a.s.prefix[j] - a.s.prefix[a.w.g.first[t]] : 0u;
  const uint64_t src = live ? a.w.in_off[t] + b.pos : 0u, dst = live ? a.out_off[t] + rel : 0u;
  const bool xerial = live && kind == kXerial, raw = live && kind == kRaw;
  a.s.out_at[j] = dst;
  a.s.x_in_len[j] = xerial ? p : 0u;
  a.s.x_cap[j] = xerial ? d : 0u;
  a.s.x_out_off[j] = xerial ? dst + kHeader : 0u;
  a.s.r_in_off[j] = live ? src + kHeader : 0u;
  a.s.r_in_len[j] = raw ? p : 0u;
  a.s.r_cap[j] = raw ? d : 0u;
  a.s.r_out_off[j] = raw ? dst + kHeader : 0u;
  a.s.r_status[j] = SM_OK;
  a.s.copy[j] = live && kind == kStored ? d : 0u;
  a.s.ci_off[j] = live ? src + kCrcFrom : 0u;
  a.s.ci_len[j] = live && a.verify ? b.length + kLengthEnd - kCrcFrom : 0u;
  a.s.co_off[j] = live ? dst + kCrcFrom : 0u;
  a.s.co_len[j] = live ? kHeader - kCrcFrom + d : 0u;
  a.s.computed[j] = 0;
  a.s.crc[j] = 0;
  a.s.status[j] = SM_OK;
  if (t == kNoSlot) return;
  if (a.batch_in_off) a.batch_in_off[j] = b.pos;
  if (a.batch_out_off) a.batch_out_off[j] = rel;
  if (a.batch_len) a.batch_len[j] = d;
  if (a.batch_codec) a.batch_codec[j] = b.codec;
  if (a.batch_status) a.batch_status[j] = SM_OK;
}

hipError_t launch_decode_plan(const DecodeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_kafka_sizes, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_kafka_plan, dim3((a.w.ns + 255) / 256), dim3(256), 0, s, a);
  if (a.w.m) hipLaunchKernelGGL(k_kafka_place, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- decode: the gate ----------------------------------------------------------------------------
// The snappy-java decode counts the chunks of the written batches against max_chunks itself and, over
// it, decodes nothing and answers SM_ERR_ARGUMENT for every stream: that is then the whole call's.
__global__ __launch_bounds__(256) void k_kafka_gate_find(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m) return;
  if (a.s.co_len[j] != 0 && a.s.kind[j] == kXerial && a.s.x_status[j] == SM_ERR_ARGUMENT) a.w.hdr->over = 1u;
}

// ... and no other slot is decoded, copied, packed or summed
__global__ __launch_bounds__(256) void k_kafka_gate_shut(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m || !a.w.hdr->over) return;
  a.s.r_in_len[j] = 0;
  a.s.r_cap[j] = 0;
  a.s.copy[j] = 0;
  a.s.ci_len[j] = 0;
  a.s.co_len[j] = 0;
}

hipError_t launch_gate(const DecodeArgs& a, hipStream_t s) {
  if (a.w.m) {
    hipLaunchKernelGGL(k_kafka_gate_find, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kafka_gate_shut, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// ---- decode: the stored payloads, the headers ----------------------------------------------------
// blockIdx.x strides the slots, blockIdx.y the tiles of one
__global__ __launch_bounds__(256) void k_kafka_copy(DecodeArgs a) {
  for (uint32_t j = blockIdx.x; j < a.w.m; j += gridDim.x) {
    if (!a.s.copy[j]) continue;
    smc::copy_tiled(a.w.in + a.s.r_in_off[j], a.s.copy[j], a.out + a.s.out_at[j] + kHeader);
  }
}

// 64 threads per slot, a header byte each (header_byte): the crc's bytes are zero until its store
__global__ __launch_bounds__(256) void k_kafka_pack(DecodeArgs a) {
  const uint64_t at = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t j = at / 64;
  const uint32_t i = (uint32_t)(at % 64);
  if (j >= a.w.m || i >= kHeader || a.s.co_len[j] == 0) return;
  const uint8_t* const src = a.w.in + a.s.r_in_off[j] - kHeader;
  a.out[a.s.out_at[j] + i] = header_byte([&](uint32_t k) { return (uint32_t)src[k]; }, i, kMinLength + a.s.decl[j], kCodecNone);
}

hipError_t launch_decode_pack(const DecodeArgs& a, hipStream_t s) {
  if (a.w.m) {
    hipLaunchKernelGGL(k_kafka_copy, smc::copy_grid(a.w.m, kLongest), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kafka_pack, dim3((uint32_t)(((uint64_t)a.w.m * 64 + 255) / 256)), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// a thread per slot: the four bytes of its checksum, big-endian, byte by byte (a batch sits at any
// alignment), in front of the range the checksum covers
__global__ __launch_bounds__(256) void k_kafka_crc(uint8_t* out, const uint64_t* crc_off, const uint32_t* crc_len, const uint32_t* crc,
                                                   uint32_t m) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m || crc_len[j] == 0) return;
  uint8_t* const p = out + crc_off[j] - (kCrcFrom - kCrcAt);
  const uint32_t c = crc[j];
  for (uint32_t i = 0; i < 4; ++i) p[i] = (uint8_t)(c >> (8 * (3 - i)));
}

hipError_t launch_crc_store(uint8_t* out, const uint64_t* crc_off, const uint32_t* crc_len, const uint32_t* crc, uint32_t m,
                            hipStream_t s) {
  if (m) hipLaunchKernelGGL(k_kafka_crc, dim3((m + 255) / 256), dim3(256), 0, s, out, crc_off, crc_len, crc, m);
  return hipGetLastError();
}

// ---- decode: the results -------------------------------------------------------------------------
// A thread per slot: a written batch's verdict (batch_verdict); a failing one bids for its segment's first.
__global__ __launch_bounds__(256) void k_kafka_verdict(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m || a.s.co_len[j] == 0) return;
  const int32_t st = batch_verdict(a.verify != 0, a.s.stored[j], a.s.computed[j], a.s.kind[j], a.s.x_status[j], a.s.r_status[j]);
  a.s.status[j] = st;
  if (a.batch_status) a.batch_status[j] = st;
  if (st != SM_OK) atomicMin(&a.w.g.fail[a.w.b.segment[j]], j);
}

__global__ __launch_bounds__(256) void k_kafka_result(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.w.ns) return;
  const bool over = a.w.hdr->over != 0;
  const uint32_t f = over ? kNoSlot : a.w.g.fail[t];
  a.status[t] = smc::plan_verdict(over, a.w.g.pre[t], f, f != kNoSlot ? a.s.status[f] : (int32_t)SM_OK);
  if (over) a.out_len[t] = 0;
}

hipError_t launch_decode_result(const DecodeArgs& a, hipStream_t s) {
  if (a.w.m) hipLaunchKernelGGL(k_kafka_verdict, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_kafka_result, dim3((a.w.ns + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress ------------------------------------------------------------------------------------
namespace {

// whether slot j's payload goes through the compressor: an uncompressed batch with records, of a
// segment whose walk found no error
__device__ inline bool compresses(const CompressArgs& a, uint32_t j) {
  return a.w.g.walk[a.w.b.segment[j]] == SM_OK && compressed_here(batch_of(a.w.b, j));
}

}  // namespace

// By one workgroup: the scan of the payloads' stage slots against stage_bytes, their 64 KiB pieces
// against max_blocks.  Over a bound nothing is compressed.
__global__ __launch_bounds__(256) void k_ckafka_plan(CompressArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.w.hdr->total;
  uint64_t mine = 0;  // the pieces of this thread's batches: a sum, not a scan
  const uint64_t stage = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        if (!compresses(a, j)) return 0;
        const uint64_t p = a.w.b.length[j] - kMinLength;
        mine += blocks_of(p);
        return stage_length(p);
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.slot_off[j] = at; });
  uint64_t blocks;
  (void)smc::block_scan(mine, sh, blocks);
  if (threadIdx.x == 0 && (stage > a.stage_bytes || blocks > a.max_blocks)) {
    a.w.hdr->over = 1u;
    a.w.hdr->total = 0u;
  }
}

// Slot j: its payload as a stream of the blocks library's encoder.  A slot that is not compressed
// (all of them over a bound) is an empty input, whose 16 header bytes land in the spare bytes behind
// the stage.
__global__ __launch_bounds__(256) void k_ckafka_slots(CompressArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.w.m) return;
  const bool comp = j < a.w.hdr->total && compresses(a, j);
  a.s.c_in_off[j] = comp ? a.w.in_off[a.w.b.segment[j]] + a.w.b.pos[j] + kHeader : 0u;
  a.s.c_in_len[j] = comp ? a.w.b.length[j] - kMinLength : 0u;
  if (!comp) a.s.slot_off[j] = a.stage_bytes;
  a.s.c_len[j] = 0;
  a.s.c_status[j] = SM_OK;
  a.s.co_off[j] = 0;
  a.s.co_len[j] = 0;
  a.s.crc[j] = 0;
}

hipError_t launch_compress_plan(const CompressArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ckafka_plan, dim3(1), dim3(256), 0, s, a);
  if (a.w.m) hipLaunchKernelGGL(k_ckafka_slots, dim3((a.w.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The scan of the encoded batch sizes over all recorded batches, by one workgroup: a batch's place
// in its segment is its scan minus the scan at its segment's first batch.  A batch whose stream is
// missing bids for its segment's first failure: that segment is not written.
__global__ __launch_bounds__(256) void k_ckafka_sizes(CompressArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.w.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        const uint32_t t = a.w.b.segment[j];
        if (a.w.g.walk[t] != SM_OK) return 0;
        const Batch b = batch_of(a.w.b, j);
        const bool comp = compressed_here(b);
        if (comp && (a.s.c_status[j] != SM_OK || a.s.c_len[j] > xerial_max_length(b.length - kMinLength))) {
          atomicMin(&a.w.g.fail[t], j);
          return 0;
        }
        return encoded_length(b, comp ? a.s.c_len[j] : 0u);
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.size_scan[j] = at; });
  if (threadIdx.x == 0) a.s.size_scan[used] = sum;
}

// blockIdx.x strides the slots, blockIdx.y the tiles of one.  A batch that was uncompressed: its
// stream behind its rewritten header (the first row's 61 threads; the crc's bytes are zero until
// its store) and the range its checksum covers; a batch that was compressed: its bytes as they are.
__global__ __launch_bounds__(256) void k_ckafka_pack(CompressArgs a) {
  const uint32_t used = a.w.hdr->total;
  for (uint32_t j = blockIdx.x; j < used; j += gridDim.x) {
    const uint32_t t = a.w.b.segment[j];
    if (a.w.g.walk[t] != SM_OK || a.w.g.fail[t] != kNoSlot) continue;
    const Batch b = batch_of(a.w.b, j);
    const uint64_t rel = a.s.size_scan[j] - a.s.size_scan[a.w.g.first[t]];
    const uint8_t* const src = a.w.in + a.w.in_off[t] + b.pos;
    uint8_t* const d = a.out + a.out_off[t] + rel;
    if (b.codec != kCodecNone) {
      smc::copy_tiled(src, kLengthEnd + b.length, d);
      continue;
    }
    const uint32_t clen = compressed_here(b) ? (uint32_t)a.s.c_len[j] : 0u;
    if (blockIdx.y == 0) {
      const uint32_t i = threadIdx.x;
      if (i < kHeader) d[i] = header_byte([&](uint32_t k) { return (uint32_t)src[k]; }, i, kMinLength + clen, kCodecSnappy);
      if (i == 0) {
        a.s.co_off[j] = a.out_off[t] + rel + kCrcFrom;
        a.s.co_len[j] = kHeader - kCrcFrom + clen;
      }
    }
    smc::copy_tiled(a.s.stage + a.s.slot_off[j], clen, d + kHeader);
  }
}

hipError_t launch_compress_pack(const CompressArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ckafka_sizes, dim3(1), dim3(256), 0, s, a);
  if (a.w.m) hipLaunchKernelGGL(k_ckafka_pack, smc::copy_grid(a.w.m, kLongest), dim3(256), 0, s, a);
  return hipGetLastError();
}

// A thread per segment: over a bound SM_ERR_ARGUMENT; the walk's error; SM_ERR_DEVICE for a missing
// stream; each with no length (and no byte was written); else its length.
__global__ __launch_bounds__(256) void k_ckafka_result(CompressArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.w.ns) return;
  const bool over = a.w.hdr->over != 0;
  const int32_t st = over ? (int32_t)SM_ERR_ARGUMENT
                          : a.w.g.walk[t] != SM_OK ? a.w.g.walk[t] : a.w.g.fail[t] != kNoSlot ? (int32_t)SM_ERR_DEVICE : (int32_t)SM_OK;
  a.status[t] = st;
  a.out_len[t] = st != SM_OK ? 0u : a.s.size_scan[a.w.g.first[t + 1]] - a.s.size_scan[a.w.g.first[t]];
}

hipError_t launch_compress_result(const CompressArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ckafka_result, dim3((a.w.ns + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smk
