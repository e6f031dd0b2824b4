// smq_kernels.hip -- a batch of Parquet column chunks per call (smq_uncompress_chunks_device): gfx950
// kernels and their launchers (smq_internal.h).  The walker over the chunks' Thrift page headers,
// and plumbing around the multi library's two device calls, which run once over the compressed
// sections of all pages of all chunks: the copies of level bytes and stored sections, the verdicts.
// The CRC pass is smq_crc.hip's.  The decisions are the shared rules of smq_format.h and
// smq_chunks.h, taken per chunk and per slot on the device, so a call needs no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smq_chunks.h"
#include "smq_format.h"
#include "smq_internal.h"

namespace smq {

// ---- the plan ------------------------------------------------------------------------------------
// The counting walk, one wave per chunk: what the chunk gets (chunk_plan) before any byte of it is
// decoded.  The walks of a workgroup's waves are independent: no barrier in here.  The Thrift
// reader's frames are the wave's own piece of LDS (every lane writes the same value).
__global__ __launch_bounds__(256) void k_pq_count(DecodeChunksArgs a) {
  __shared__ Frame frames[smc::kWalkWaves][SMQ_MAX_DEPTH];
  const uint32_t r = smc::walker_index();
  if (r >= a.nchunks) return;
  const uint64_t n = a.in_len[r];
  smc::WindowFetch fetch{a.in + a.in_off[r], n, threadIdx.x & 63};
  const Walk w = walk_pages(n, fetch, frames[threadIdx.x >> 6], [](uint32_t, uint64_t, const Page&) {});
  if (fetch.lane == 0) {
    const ChunkPlan p = chunk_plan(w, a.out_cap[r]);
    a.s.count[r] = p.slots;
    a.s.pre[r] = p.status;
    a.s.length[r] = p.length;
    a.s.fail[r] = kNoSlot;
  }
}

// the exclusive scan of the chunks' slots against the bound m, by one workgroup
__global__ __launch_bounds__(256) void k_pq_scan(DecodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.nchunks, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.first, a.page_first, a.s.hdr, sh);
  if (threadIdx.x == 0) a.s.hdr->segments = 0;
}

// The slots no page took (all of them over the bound) become empty: nothing to copy, to check or to
// decode.  Then the storing walk of the chunks that are decoded: page k of chunk r is slot
// first[r] + k; its body's offset is relative to d_in and its output's to d_out (the chunk's place
// plus the uncompressed sizes before it, the walk's own running total).  A compressed section's
// capacity is exactly `want`; any other slot stands before the raw decoder as an empty stream with
// no room.  The walk is the counting walk's over the same bytes; a slot past the chunk's count is
// never stored.
__global__ __launch_bounds__(256) void k_pq_fill(DecodeChunksArgs a) {
  __shared__ Frame frames[smc::kWalkWaves][SMQ_MAX_DEPTH];
  for (uint64_t j = (uint64_t)a.s.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    a.s.body_off[j] = 0;
    a.s.page_out[j] = 0;
    a.s.in_off[j] = 0;
    a.s.out_off[j] = 0;
    a.s.body_len[j] = 0;
    a.s.copy_len[j] = 0;
    a.s.in_len[j] = 0;
    a.s.cap[j] = 0;
    a.s.chunk[j] = kNoSlot;
    a.s.flags[j] = 0;
    a.s.crc_want[j] = 0;
    a.s.crc_got[j] = 0;
    if (a.table) store_page(a.pages, j, 0, Page{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false});
  }
  const uint32_t r = smc::walker_index();
  if (r >= a.nchunks || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[r], base = a.s.first[r];
  if (cnt == 0) return;
  const uint64_t in_off = a.in_off[r], out_off = a.out_off[r], n = a.in_len[r];
  smc::WindowFetch fetch{a.in + in_off, n, threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_pages(n, fetch, frames[threadIdx.x >> 6], [&](uint32_t k, uint64_t at, const Page& p) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    const uint64_t body = in_off + p.hdr_off + p.hdr_len;
    const bool compressed = (p.flags & SMQ_PAGE_COMPRESSED) != 0;
    a.s.body_off[j] = body;
    a.s.page_out[j] = out_off + at;
    a.s.in_off[j] = body + p.levels;
    a.s.out_off[j] = out_off + at + p.levels;
    a.s.body_len[j] = p.output ? p.body_len : 0u;  // (a page that is stepped over is not checked)
    a.s.copy_len[j] = copy_len(p);
    a.s.in_len[j] = compressed ? section_len(p) : 0u;
    a.s.cap[j] = compressed ? section_want(p) : 0u;
    a.s.chunk[j] = r;
    a.s.flags[j] = p.output ? p.flags : 0u;
    a.s.crc_want[j] = p.crc;
    a.s.crc_got[j] = 0;
    if (a.table) store_page(a.pages, j, at, p);
  });
}

// With verification: the scan of the CRC segments of the slots whose header carries a crc, by one
// workgroup (the segment pass finds a segment's slot in it).
__global__ __launch_bounds__(256) void k_pq_segments(DecodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh, [&](uint32_t j) -> uint64_t { return (a.s.flags[j] & SMQ_PAGE_HAS_CRC) ? crc_segments(a.s.body_len[j]) : 0u; },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.seg_first[j] = smc::sat32(at); });
  if (threadIdx.x == 0) {
    a.s.seg_first[used] = smc::sat32(sum);
    a.s.hdr->segments = smc::sat32(sum);
  }
}

hipError_t launch_decode_plan(const DecodeChunksArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nchunks + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_pq_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pq_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) {
    hipLaunchKernelGGL(k_pq_fill, dim3(walkers), dim3(256), 0, s, a);
    if (a.verify_crc) hipLaunchKernelGGL(k_pq_segments, dim3(1), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// ---- the stored bytes ----------------------------------------------------------------------------
// blockIdx.x strides the used slots, blockIdx.y a slot's tiles.  A page's level bytes, and its
// section when that is stored, go from d_in straight to the page's place in d_out; the walk has
// checked that the body lies inside its chunk and the plan that the pages fit the chunk's room.
__global__ __launch_bounds__(256) void k_pq_copy(DecodeChunksArgs a) {
  const uint32_t total = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
    const uint32_t n = a.s.copy_len[j];
    if (a.s.chunk[j] == kNoSlot || n == 0) continue;
    smc::copy_tiled(a.in + a.s.body_off[j], n, a.out + a.s.page_out[j]);
  }
}

// ---- the results ---------------------------------------------------------------------------------
// A slot's verdict (slot_verdict); a failing one bids for its chunk's first.
__global__ __launch_bounds__(256) void k_pq_verdict(DecodeChunksArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t r = a.s.chunk[j], flags = a.s.flags[j];
  const uint32_t n = a.s.body_len[j];
  const uint32_t got = n ? ~a.s.crc_got[j] : 0u;  // (the register's complement; the CRC of nothing is 0)
  const int32_t st = slot_verdict(r, a.verify_crc && (flags & SMQ_PAGE_HAS_CRC), got, a.s.crc_want[j],
                                  (flags & SMQ_PAGE_COMPRESSED) != 0, a.s.dec_status[j]);
  a.s.dec_status[j] = st;  // (from here on the slot's own status)
  if (a.page_status) a.page_status[j] = st;
  if (st != SM_OK) atomicMin(&a.s.fail[r], j);
}

__global__ __launch_bounds__(256) void k_pq_result(DecodeChunksArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nchunks) return;
  const bool over = a.s.hdr->over != 0;
  const uint32_t fail = over ? kNoSlot : a.s.fail[r];
  a.status[r] = smc::plan_verdict(over, a.s.pre[r], fail, fail != kNoSlot ? a.s.dec_status[fail] : (int32_t)SM_OK);
  a.out_len[r] = over ? 0 : a.s.length[r];
}

hipError_t launch_decode_result(const DecodeChunksArgs& a, const CrcLut* T, hipStream_t s) {
  if (a.m) {
    hipLaunchKernelGGL(k_pq_copy, smc::copy_grid(a.m, kCopyTypical), dim3(256), 0, s, a);
    if (a.verify_crc) {
      const hipError_t e = launch_crc_segments(CrcJobs{a.in, a.s.body_off, a.s.body_len, nullptr, a.s.seg_first, a.m, a.s.hdr, a.s.crc_got}, T, s);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pq_verdict, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_pq_result, dim3((a.nchunks + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smq
