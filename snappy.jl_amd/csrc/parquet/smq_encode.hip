// smq_encode.hip -- a batch of plain Parquet column chunks per call becomes compression=SNAPPY chunks
// (smqe_compress_chunks_device): gfx950 kernels and their launchers (smq_internal.h).  The decoder's
// pipeline turned round: the one-wave walkers over the Thrift page headers, with the encode policy;
// the multi library's compressor once over the values sections of all pages of all chunks, into a
// stage; the level bytes in front of them; the CRC pass of smq_crc.hip over the staged bodies; then
// the sizes, which need the CRCs (a header's length depends on its crc's varint), and the pack.  The
// decisions are the shared rules of smq_format.h and smq_encode.h, taken per chunk and per slot on the
// device, so a call needs no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smq_chunks.h"
#include "smq_encode.h"
#include "smq_format.h"
#include "smq_internal.h"

namespace smq {

namespace {

// a slot without a page: nothing to compress (an empty stream, to the stage's dump bytes), to copy,
// to check or to pack
__device__ inline void clear_slot(const EncodeChunksArgs& a, uint64_t j) {
  a.s.hdr_in[j] = 0;
  a.s.in_off[j] = 0;
  a.s.comp_off[j] = 0;
  a.s.body_off[j] = 0;
  a.s.page_out[j] = 0;
  a.s.stage_len[j] = 0;
  a.s.hdr_len[j] = 0;
  a.s.old_body[j] = 0;
  a.s.levels[j] = 0;
  a.s.in_len[j] = 0;
  a.s.new_body[j] = 0;
  a.s.new_hdr[j] = 0;
  a.s.chunk[j] = kNoSlot;
  a.s.flags[j] = 0;
  a.s.crc_acc[j] = 0;
  for (uint32_t k = 0; k < SMQE_SITES; ++k) a.s.sites[j * SMQE_SITES + k] = 0;
  a.s.slot_status[j] = SM_OK;
}

__device__ inline Sites slot_sites(const EncodeChunksArgs& a, uint32_t j) {
  const uint32_t* w = a.s.sites + (uint64_t)j * SMQE_SITES;
  return Sites{w[0], w[1], w[2], w[3], w[4]};
}

// the rewrite of slot j's header around its staged body (the CRC pass is through)
__device__ inline Rewrite slot_rewrite(const EncodeChunksArgs& a, uint32_t j) {
  const uint32_t n = a.s.new_body[j];
  return make_rewrite(a.s.hdr_len[j], slot_sites(a, j), n, n ? ~a.s.crc_acc[j] : 0u);  // (the CRC of nothing is 0)
}

}  // namespace

// ---- the plan ------------------------------------------------------------------------------------
// The counting walk, one wave per chunk: a chunk without a walk error takes a slot per page.
__global__ __launch_bounds__(256) void k_pqe_count(EncodeChunksArgs a) {
  __shared__ Frame frames[smc::kWalkWaves][SMQ_MAX_DEPTH];
  const uint32_t r = smc::walker_index();
  if (r >= a.nchunks) return;
  const uint64_t n = a.in_len[r];
  smc::WindowFetch fetch{a.in + a.in_off[r], n, threadIdx.x & 63};
  const Walk w = walk_pages<EncodeWalk>(n, fetch, frames[threadIdx.x >> 6], [](uint32_t, uint64_t, const Page&) {});
  if (fetch.lane == 0) {
    a.s.count[r] = w.status == SM_OK ? w.npages : 0u;
    a.s.pre[r] = w.status;
    a.s.fail[r] = kNoSlot;
    a.s.go[r] = 0;
  }
}

// the exclusive scan of the chunks' slots against the bound m, by one workgroup
__global__ __launch_bounds__(256) void k_pqe_scan(EncodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  smc::count_scan(a.nchunks, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.first, a.page_first, a.s.hdr, sh);
  if (threadIdx.x == 0) a.s.hdr->segments = 0;
}

// The slots no page took (all of them over the bound) become empty.  Then the storing walk: page k
// of chunk r is slot first[r] + k, with its header's place and patch sites, its section as the raw
// compressor's input (offsets relative to d_in) and the size of its stage slot.  The walk is the
// counting walk's over the same bytes; a slot past the chunk's count is never stored.
__global__ __launch_bounds__(256) void k_pqe_fill(EncodeChunksArgs a) {
  __shared__ Frame frames[smc::kWalkWaves][SMQ_MAX_DEPTH];
  for (uint64_t j = (uint64_t)a.s.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    clear_slot(a, j);
    if (a.table) store_page(a.pages, j, 0, Page{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false});
  }
  const uint32_t r = smc::walker_index();
  if (r >= a.nchunks || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[r], base = a.s.first[r];
  if (cnt == 0) return;
  const uint64_t in_off = a.in_off[r], n = a.in_len[r];
  smc::WindowFetch fetch{a.in + in_off, n, threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_pages<EncodeWalk>(n, fetch, frames[threadIdx.x >> 6], [&](uint32_t k, uint64_t at, const Page& p) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    const uint64_t hdr = in_off + p.hdr_off;
    a.s.hdr_in[j] = hdr;
    a.s.in_off[j] = hdr + p.hdr_len + p.levels;
    a.s.comp_off[j] = 0;
    a.s.body_off[j] = 0;
    a.s.page_out[j] = 0;
    a.s.stage_len[j] = stage_slot(p);
    a.s.hdr_len[j] = p.hdr_len;
    a.s.old_body[j] = p.body_len;
    a.s.levels[j] = p.levels;
    a.s.in_len[j] = p.output ? section_want(p) : 0u;
    a.s.new_body[j] = 0;
    a.s.new_hdr[j] = 0;
    a.s.chunk[j] = r;
    // (as the output's page table has them: every section that is written is a raw stream)
    a.s.flags[j] = (p.flags & SMQ_PAGE_HAS_CRC) | (p.output ? SMQ_PAGE_COMPRESSED : 0u);
    a.s.crc_acc[j] = 0;
    const uint32_t sites[SMQE_SITES] = {p.sites.f3_at, p.sites.f3_len, p.sites.f4_at, p.sites.f4_len, p.sites.f7_at};
    for (uint32_t i = 0; i < SMQE_SITES; ++i) a.s.sites[(uint64_t)j * SMQE_SITES + i] = sites[i];
    a.s.slot_status[j] = SM_OK;
    if (a.table) store_page(a.pages, j, at, p);
  });
}

// The scan of the stage slots and the sum of the fragments, by one workgroup, against the caller's
// two other bounds: a page's body is staged at its slot (behind the dump bytes), its section's raw
// stream behind the level bytes.  Over a bound nothing is compressed: every slot becomes empty.
__global__ __launch_bounds__(256) void k_pqe_stage(EncodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  uint64_t mine = 0;  // the fragments of this thread's slots: a sum, not a scan
  const uint64_t stage = smc::tile_scan(
      used, sh,
      [&](uint32_t j) {
        const uint32_t n = a.s.in_len[j];
        if (n > kFragment) mine += fragments(n);
        return a.s.stage_len[j];
      },
      [&](uint32_t j, uint64_t v, uint64_t at) {
        a.s.body_off[j] = kStageDump + at;
        a.s.comp_off[j] = v ? kStageDump + at + a.s.levels[j] : 0u;
      });
  uint64_t frags;
  (void)smc::block_scan(mine, sh, frags);
  // (uniform; without a stage slot nothing is staged, and the dump bytes are the scratch's own)
  if ((stage == 0 || kStageDump + stage <= a.stage_bytes) && frags <= a.max_fragments) return;
  for (uint32_t j = threadIdx.x; j < used; j += 256) {
    clear_slot(a, j);
    if (a.table) store_page(a.pages, j, 0, Page{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false});
  }
  if (threadIdx.x == 0) {  // (every thread read `used` before the scans' barriers)
    a.s.hdr->over = 1;
    a.s.hdr->total = 0;
  }
}

hipError_t launch_encode_plan(const EncodeChunksArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nchunks + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_pqe_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pqe_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_pqe_fill, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pqe_stage, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- the staged bodies -----------------------------------------------------------------------------
// blockIdx.x strides the used slots, blockIdx.y a slot's tiles: a page's level bytes go from d_in to
// the front of its stage slot (the walk has checked that they lie inside the chunk).
__global__ __launch_bounds__(256) void k_pqe_levels(EncodeChunksArgs a) {
  const uint32_t total = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
    const uint32_t n = a.s.levels[j];
    if (n == 0) continue;
    smc::copy_tiled(a.in + a.s.hdr_in[j] + a.s.hdr_len[j], n, a.s.stage + a.s.body_off[j]);
  }
}

// Behind the compressor, by one workgroup: a page's status (page_verdict; a failing one bids for its
// chunk's first), the new body's length, and the scan of the CRC segments of the bodies whose header
// carries a crc (the segment pass finds a segment's slot in it).
__global__ __launch_bounds__(256) void k_pqe_bodies(EncodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        const uint32_t flags = a.s.flags[j];
        const bool output = (flags & SMQ_PAGE_COMPRESSED) != 0;
        const int32_t st = page_verdict(output, a.s.levels[j], a.s.comp_len[j], a.s.comp_status[j]);
        const uint32_t body = !output ? a.s.old_body[j] : st == SM_OK ? a.s.levels[j] + a.s.comp_len[j] : 0u;
        a.s.new_body[j] = body;
        a.s.slot_status[j] = st;
        if (st != SM_OK) atomicMin(&a.s.fail[a.s.chunk[j]], j);
        return output && st == SM_OK && (flags & SMQ_PAGE_HAS_CRC) ? crc_segments(body) : 0u;
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.seg_first[j] = smc::sat32(at); });
  if (a.page_status)
    for (uint32_t j = threadIdx.x; j < a.m; j += 256) a.page_status[j] = j < used ? a.s.slot_status[j] : (int32_t)SM_OK;
  if (threadIdx.x == 0) {
    a.s.seg_first[used] = smc::sat32(sum);
    a.s.hdr->segments = smc::sat32(sum);
  }
}

// ---- the sizes and the results ---------------------------------------------------------------------
// A workgroup per chunk (strided): every page's new header length by the rewrite rule, the exclusive
// sums that place the pages, the chunk's length against its room and its result (encode_verdict).
__global__ __launch_bounds__(256) void k_pqe_size(EncodeChunksArgs a) {
  __shared__ uint64_t sh[4];
  const bool over = a.s.hdr->over != 0;
  for (uint32_t r = blockIdx.x; r < a.nchunks; r += gridDim.x) {  // (uniform: the workgroup's chunk)
    const uint32_t base = a.s.first[r], cnt = over ? 0u : a.s.count[r];
    const uint64_t need = smc::tile_scan(
        cnt, sh,
        [&](uint32_t k) -> uint64_t {
          const uint32_t j = base + k;
          if (!(a.s.flags[j] & SMQ_PAGE_COMPRESSED)) {
            a.s.new_hdr[j] = a.s.hdr_len[j];
            return (uint64_t)a.s.hdr_len[j] + a.s.old_body[j];
          }
          const Rewrite w = slot_rewrite(a, j);
          a.s.new_hdr[j] = w.new_len;
          if (a.table && w.s.f4_len) a.pages.crc[j] = a.s.new_body[j] ? ~a.s.crc_acc[j] : 0u;
          return (uint64_t)w.new_len + a.s.new_body[j];
        },
        [&](uint32_t k, uint64_t, uint64_t at) {
          const uint32_t j = base + k;
          a.s.page_out[j] = at;
          if (a.table) {
            a.pages.hdr_off[j] = at;
            a.pages.hdr_len[j] = a.s.new_hdr[j];
            a.pages.body_len[j] = a.s.new_body[j];
            a.pages.flags[j] = a.s.flags[j];
          }
        });
    if (threadIdx.x == 0) {
      const uint32_t fail = over ? kNoSlot : a.s.fail[r];
      const EncodeVerdict v = encode_verdict(over, a.s.pre[r], fail != kNoSlot, fail != kNoSlot ? a.s.slot_status[fail] : (int32_t)SM_OK,
                                             need, a.out_cap[r]);
      a.status[r] = v.status;
      a.out_len[r] = v.length;
      a.s.go[r] = v.status == SM_OK ? 1u : 0u;
    }
  }
}

// ---- the pack ----------------------------------------------------------------------------------------
// blockIdx.x strides the used slots, blockIdx.y a slot's tiles.  Of a chunk that is written every page
// goes to its place: the rewritten header byte by byte (rewritten_byte: each thread its own bytes, by
// the slot's first row), the staged body behind it; a page that was stepped over comes from the input
// as it is.  The sizes have been checked against the chunk's room, the stage slot holds the body, and
// the walk has checked that header and body lie inside the chunk.
__global__ __launch_bounds__(256) void k_pqe_pack(EncodeChunksArgs a) {
  const uint32_t total = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
    const uint32_t r = a.s.chunk[j];
    if (r == kNoSlot || !a.s.go[r]) continue;
    uint8_t* const dst = a.out + a.out_off[r] + a.s.page_out[j];
    const uint8_t* const hdr = a.in + a.s.hdr_in[j];
    const uint32_t hdr_len = a.s.hdr_len[j];
    if (a.s.flags[j] & SMQ_PAGE_COMPRESSED) {
      const Rewrite w = slot_rewrite(a, j);
      if (blockIdx.y == 0)
        for (uint32_t i = threadIdx.x; i < w.new_len; i += blockDim.x)
          dst[i] = rewritten_byte(w, [&](uint32_t k) { return hdr[k]; }, i);
      smc::copy_tiled(a.s.stage + a.s.body_off[j], a.s.new_body[j], dst + w.new_len);
    } else {
      smc::copy_tiled(hdr, hdr_len, dst);
      smc::copy_tiled(hdr + hdr_len, a.s.old_body[j], dst + hdr_len);
    }
  }
}

hipError_t launch_encode_result(const EncodeChunksArgs& a, const CrcLut* T, hipStream_t s) {
  const dim3 copies = smc::copy_grid(a.m, kCopyTypical);
  if (a.m) {
    hipLaunchKernelGGL(k_pqe_levels, copies, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_pqe_bodies, dim3(1), dim3(256), 0, s, a);
    const hipError_t e = launch_crc_segments(CrcJobs{a.s.stage, a.s.body_off, a.s.new_body, nullptr, a.s.seg_first, a.m, a.s.hdr, a.s.crc_acc}, T, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_pqe_size, dim3(a.nchunks < smc::kCopyGroups ? a.nchunks : smc::kCopyGroups), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_pqe_pack, copies, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smq
