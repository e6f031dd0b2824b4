// smf_range.hip -- the seek index and the ranged decode of the framing library: gfx950 kernels and
// their launchers (smf_range.h).  Plumbing around the raw codec's batched decoder and k_crc32c, as
// smf_kernels.hip's decode is; the decisions are the shared rules of smf_range.h, taken per range
// and per slot on the device, so a call needs no host synchronisation.  The slot stage behind
// the plan is the shared one (smf_slots.h); the scans are smf_device.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smf_device.h"
#include "smf_format.h"
#include "smf_internal.h"
#include "smf_range.h"

namespace smf {

namespace {

using smc::copy_bytes;

}  // namespace

// ---- the seek index ------------------------------------------------------------------------------
// chunk_off = the exclusive scan of ulen, chunk_off[nchunks] = the total, by one workgroup
__global__ __launch_bounds__(256) void k_chunk_offsets(const uint32_t* __restrict__ ulen, uint32_t nchunks,
                                                       uint64_t* __restrict__ chunk_off) {
  __shared__ uint64_t sh[4];
  const uint64_t total = smc::tile_scan(nchunks, sh, [&](uint32_t c) { return ulen[c]; },
                                   [&](uint32_t c, uint64_t, uint64_t o) { chunk_off[c] = o; });
  if (threadIdx.x == 0) chunk_off[nchunks] = total;
}

hipError_t launch_chunk_offsets(const uint32_t* ulen, uint32_t nchunks, uint64_t* chunk_off, hipStream_t s) {
  hipLaunchKernelGGL(k_chunk_offsets, dim3(1), dim3(256), 0, s, ulen, nchunks, chunk_off);
  return hipGetLastError();
}

// The encoder's index, behind k_frame_scan: block b is data chunk b.  *status is k_frame_scan's.
__global__ __launch_bounds__(256) void k_frame_index_out(const uint8_t* type, const uint64_t* dst_off,
                                                         const uint32_t* comp_len, const uint32_t* in_len,
                                                         const uint32_t* crc, uint32_t nblk, uint64_t n, smf_chunks ch,
                                                         uint64_t* chunk_off, uint32_t* nchunks, const int32_t* status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nblk) {
    const uint8_t ty = type[b];
    ch.type[b] = ty;
    ch.pay_off[b] = dst_off[b] + 8;
    ch.pay_len[b] = ty == SMF_CHUNK_COMPRESSED ? comp_len[b] : in_len[b];
    ch.crc[b] = crc[b];
    ch.ulen[b] = in_len[b];
    chunk_off[b] = (uint64_t)b * kBlock;
  } else if (b == nblk) {
    chunk_off[nblk] = n;
    *nchunks = *status == SM_OK ? nblk : 0u;
  }
}

hipError_t launch_frame_index_out(const PackArgs& a, uint64_t n, const smf_chunks& ch, uint64_t* chunk_off,
                                  uint32_t* nchunks, const int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_frame_index_out, dim3(a.nblk / 256 + 1), dim3(256), 0, s, a.type, a.dst_off, a.comp_len, a.in_len,
                     a.crc, a.nblk, n, ch, chunk_off, nchunks, status);
  return hipGetLastError();
}

// ---- the range plan ------------------------------------------------------------------------------
// Per range: its chunks (two bounded searches) and whether it leaves the stream.
__global__ __launch_bounds__(256) void k_range_find(RangeArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nranges) return;
  const RangeChunks rc = range_chunks(a.chunk_off, a.nchunks, a.lo[r], a.len[r]);
  a.s.first[r] = rc.first;
  a.s.count[r] = rc.count;
  a.s.rpre[r] = rc.status;
  a.s.slots.fail[r] = kNoSlot;
}

// base = the exclusive scan of the counts over the ranges, and the compare with max_range_chunks
__global__ __launch_bounds__(256) void k_range_counts(RangeArgs a) {
  __shared__ uint64_t sh[4];
  scan_counts(a.nranges, a.m, [&](uint32_t r) { return a.s.count[r]; }, a.s.base, nullptr, a.s.hdr, sh);
}

// Slot j: its range (a search in the scanned counts), its chunk, the entry checks, and what the raw
// decoder, the copy, the CRC pass and the trim get for it.  A slot that is not decoded -- unused,
// an empty chunk, a failed check, or every slot over the bound -- is an empty stream with no room:
// the raw decoder returns at once, and nothing else touches it.  Offsets of outputs are relative
// to the edge slots' base, which is what the raw decoder and the CRC pass get as their buffer.
__global__ __launch_bounds__(256) void k_range_slots(RangeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  uint64_t in_off = 0, out_off = 0, trim_dst = 0;
  uint32_t dec_len = 0, cap = 0, trim_src = 0, trim_len = 0, range = kNoSlot, want = 0;
  int32_t pre = SM_OK;
  uint8_t type = SMF_CHUNK_COMPRESSED;
  if (j < a.s.hdr->total) {
    const uint32_t r = upper_bound(a.s.base, a.nranges + 1, j) - 1;  // base[r] <= j < base[r + 1]
    const uint32_t k = r < a.nranges ? j - a.s.base[r] : kNoSlot, cnt = r < a.nranges ? a.s.count[r] : 0u;
    if (k < cnt) {  // (always, for the bases the scan wrote)
      const uint32_t c = a.s.first[r] + k;
      bool skip;
      const Place p = slot_place(a.ch, a.chunk_off, a.n, c, a.lo[r], a.len[r], k == 0, k == cnt - 1, skip);
      if (!skip) {
        range = r;
        pre = p.status;
        if (pre == SM_OK) {
          type = a.ch.type[c];
          const uint8_t* const target = p.edge ? a.edge + (2 * (uint64_t)r + (p.edge - 1)) * kEdgePitch
                                               : a.out + a.out_off[r] + p.dst;
          out_off = (uint64_t)(uintptr_t)target - (uint64_t)(uintptr_t)a.edge;
          in_off = a.ch.pay_off[c];
          cap = a.ch.ulen[c];
          want = a.ch.crc[c];
          if (type == SMF_CHUNK_COMPRESSED) dec_len = a.ch.pay_len[c];
          if (p.edge) {
            trim_src = p.src;
            trim_len = p.n;
            trim_dst = a.out_off[r] + p.dst;
          }
        }
      }
    }
  }
  a.s.slots.in_off[j] = in_off;
  a.s.slots.out_off[j] = out_off;
  a.s.trim_dst[j] = trim_dst;
  a.s.slots.dec_len[j] = dec_len;
  a.s.slots.cap[j] = cap;
  a.s.trim_src[j] = trim_src;
  a.s.trim_len[j] = trim_len;
  a.s.slots.group[j] = range;
  a.s.slots.crc_want[j] = want;
  a.s.slots.pre[j] = pre;
  a.s.slots.type[j] = type;
}

hipError_t launch_range_plan(const RangeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_range_find, dim3((a.nranges + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_range_counts, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_range_slots, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- behind the raw decoder ----------------------------------------------------------------------
// An edge slot's covered bytes to the range's output.  The plan's numbers keep the reads inside
// the slot (trim_src + trim_len <= the chunk's length <= the slot) and the writes inside the range
// (trim_dst - out_off[r] + trim_len <= len), whatever the chunk decoded to.
__global__ __launch_bounds__(256) void k_range_trim(RangeArgs a) {
  const uint32_t j = blockIdx.x;
  const uint32_t n = a.s.trim_len[j];
  if (n == 0) return;
  copy_bytes(at(a.edge, a.s.slots.out_off[j] + a.s.trim_src[j]), n, a.out + a.s.trim_dst[j],
             blockIdx.y * blockDim.x + threadIdx.x, gridDim.y * blockDim.x);
}

hipError_t launch_range_trim(const RangeArgs& a, hipStream_t s) {
  if (a.m == 0) return hipSuccess;
  hipLaunchKernelGGL(k_range_trim, dim3(a.m, 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smf
