// smm_range.hip -- the ranged decode of indexed raw streams: gfx950 kernels and their launchers
// (smm_range.h).  Plumbing around the raw codec's fragment decoder, as smm_kernels.hip's decode
// is: the decisions are the shared rules of smm_range.h, taken per range and per slot on the
// device, so a call needs no host synchronisation.  A slot is one touched fragment of one range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "../sm_device.h"
#include "smm_range.h"

namespace smm {

namespace {

using smc::block_scan;
using smc::copy_bytes;
using smc::sat32;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTrimRows = 2;  // workgroups per edge slot: 65,536 bytes at the most, 16 per thread and step

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1) / kThreads; }

// a word every lane of the wave holds alike, in scalar registers
using sm::uniform;
__device__ inline uint64_t uniform64(uint64_t v) {
  return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
}

}  // namespace

// ---- the plan ------------------------------------------------------------------------------------
// Per range: the stream-level rule, the touched span, and how many slots and edge slots it needs.
__global__ __launch_bounds__(kThreads) void k_mrange_find(RangeArgs a) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n) return;
  const uint32_t lo = a.lo[r], len = a.len[r];
  Candidate c;
  const RangeSpan sp = range_span(a.in, a.in_off, a.in_len, a.nstreams, a.frag_first, a.nentries, a.range_stream[r], lo,
                                  len, c);
  a.s.D[r] = c.D;
  a.s.hv[r] = c.hv;
  a.s.e0[r] = c.e0;
  a.s.count[r] = c.count;
  a.s.first[r] = sp.first;
  a.s.nfrag[r] = sp.count;
  a.s.nedge[r] = range_edges(c.D, c.count, sp.first, sp.count, lo, len);
  a.s.pre[r] = sp.status;
  a.s.fail[r] = kNoSlot;
}

// base / ebase = the exclusive scans of the slot and the edge counts over the ranges, by one
// workgroup, and the compare with max_range_fragments.  (Edges are at most two per range and at
// most the slots, so under the bound they fit the edge slots the call allocated.)
__global__ __launch_bounds__(kThreads) void k_mrange_scan(RangeArgs a) {
  __shared__ uint64_t sh[4];
  uint64_t carry = 0, ecarry = 0;
  for (uint32_t at = 0; at < a.n; at += kThreads) {  // (uniform: every thread takes every tile)
    const uint32_t r = at + threadIdx.x;
    uint64_t t, et;
    const uint64_t ex = block_scan(r < a.n ? a.s.nfrag[r] : 0u, sh, t);
    const uint64_t eex = block_scan(r < a.n ? a.s.nedge[r] : 0u, sh, et);
    if (r < a.n) {
      a.s.base[r] = sat32(carry + ex);
      a.s.ebase[r] = sat32(ecarry + eex);
    }
    carry += t;
    ecarry += et;
  }
  if (threadIdx.x == 0) {
    a.s.base[a.n] = sat32(carry);
    a.s.ebase[a.n] = sat32(ecarry);
    a.s.hdr->total = sat32(carry);
    a.s.hdr->stop = carry > a.m;
  }
}

// Slot j: its range (a search in the scanned counts), its fragment, the entry check, and what the
// fragment decoder and the trim get for it.  A slot that is not decoded -- past the total, a failed
// entry, or every slot over the bound -- is an empty input that must decode to nothing: the decoder
// returns at once, and its status for the slot is ignored.  Output offsets are relative to the edge
// slots, which the fragment decoder gets as its output base: a direct slot's is its place in d_out
// minus that base modulo 2^64, which the device's flat 64-bit address arithmetic turns back into
// its address (as k_cplan_fill's dummy slots, and the framing library's ranged decode).
__global__ __launch_bounds__(kThreads) void k_mrange_slots(RangeArgs a) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= a.m) return;
  uint64_t in_off = 0, out_off = 0, trim_dst = 0;
  uint32_t in_len = 0, flen = 0, trim_src = 0, trim_len = 0, range = kNoSlot;
  int32_t pre = SM_OK;
  if (!a.s.hdr->stop && j < a.s.hdr->total) {
    const uint32_t r = owner(a.s.base, a.n, j);
    const uint32_t k = j - a.s.base[r];
    if (k < a.s.nfrag[r]) {  // (always, for the bases the scan wrote)
      range = r;
      const uint32_t s = a.range_stream[r], lo = a.lo[r], len = a.len[r], first = a.s.first[r], f = first + k;
      const Candidate c{a.s.D[r], a.s.hv[r], a.s.e0[r], a.s.count[r]};
      const SlotArgs sa = slot_args(a.frag_pos + c.e0, c, a.in_len[s], f, lo, len);
      pre = sa.status;
      if (pre == SM_OK) {
        in_off = a.in_off[s] + sa.in_lo;
        in_len = sa.in_len;
        flen = sa.frag_len;
        const uint64_t at = a.out_off[r] + sa.place.dst;
        const uint8_t* target = a.out + at;
        if (sa.place.edge) {
          target = a.edge + ((uint64_t)a.s.ebase[r] + edge_which(c.D, c.count, first, f, lo, len)) * kEdgePitch;
          trim_src = sa.place.src;
          trim_len = sa.place.n;
          trim_dst = at;
        }
        out_off = (uint64_t)(uintptr_t)target - (uint64_t)(uintptr_t)a.edge;
      }
    }
  }
  a.s.f_in_off[j] = in_off;
  a.s.f_in_len[j] = in_len;
  a.s.f_out_off[j] = out_off;
  a.s.f_len[j] = flen;
  a.s.range[j] = range;
  a.s.f_pre[j] = pre;
  a.s.trim_dst[j] = trim_dst;
  a.s.trim_src[j] = trim_src;
  a.s.trim_len[j] = trim_len;
}

hipError_t launch_range_plan(const RangeArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_mrange_find, dim3(blocks_for(a.n)), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(k_mrange_scan, dim3(1), dim3(kThreads), 0, st, a);
  if (a.m) hipLaunchKernelGGL(k_mrange_slots, dim3(blocks_for(a.m)), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

// ---- behind the fragment decoder -----------------------------------------------------------------
// An edge slot's covered bytes to the range's output; blockIdx.x = the slot, blockIdx.y strides its
// bytes.  The slot's words are the same for every lane and go through scalar registers.  The plan's
// numbers keep the reads inside the slot (trim_src + trim_len <= the fragment's length <= the slot)
// and the writes inside the range (trim_dst - out_off[r] + trim_len <= len), whatever the fragment
// decoded to; a fragment that failed is not copied.
__global__ __launch_bounds__(kThreads) void k_mrange_trim(RangeArgs a) {
  const uint32_t j = blockIdx.x;
  const uint32_t n = uniform(a.s.trim_len[j]);
  if (n == 0 || uniform((uint32_t)a.s.f_status[j]) != (uint32_t)SM_OK) return;
  const uint8_t* const src = a.edge + uniform64(a.s.f_out_off[j]) + uniform(a.s.trim_src[j]);
  copy_bytes(src, n, a.out + uniform64(a.s.trim_dst[j]), blockIdx.y * kThreads + threadIdx.x, gridDim.y * kThreads);
}

// a failing slot enters its range's minimum: the first failing fragment in stream order
__global__ __launch_bounds__(kThreads) void k_mrange_verdict(RangeArgs a) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t r = a.s.range[j];
  if (r == kNoSlot) return;
  if (slot_verdict(a.s.f_pre[j], a.s.f_status[j]) != SM_OK) atomicMin(&a.s.fail[r], j);
}

__global__ __launch_bounds__(kThreads) void k_mrange_result(RangeArgs a) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n) return;
  const uint32_t fj = a.s.fail[r];
  const int32_t failed = fj < a.m ? slot_verdict(a.s.f_pre[fj], a.s.f_status[fj]) : SM_OK;
  const int32_t st = range_verdict(a.s.hdr->stop != 0, a.s.pre[r], failed);
  a.status[r] = st;
  a.out_len[r] = st == SM_OK ? a.len[r] : 0u;
}

hipError_t launch_range_finish(const RangeArgs& a, hipStream_t st) {
  if (a.m) {
    hipLaunchKernelGGL(k_mrange_trim, dim3(a.m, kTrimRows), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_mrange_verdict, dim3(blocks_for(a.m)), dim3(kThreads), 0, st, a);
  }
  hipLaunchKernelGGL(k_mrange_result, dim3(blocks_for(a.n)), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace smm
