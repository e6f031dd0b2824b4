// smm_kernels.hip -- the multi-stream library's gfx950 kernels and their launchers (smm_plan.h).
//
// k_pack is the hot one: it moves every compressed byte of the long streams once, out of the
// fragment slots to their places behind one another (16-byte loads from the 256-byte-aligned slots,
// 16-byte stores at the destination's alignment).  The rest is planning around the raw codec's
// batched calls: scans by one workgroup, per-stream and per-fragment argument arrays, verdicts.
// Every decision that depends on the data (how many fragments there are, which stream is indexed)
// is taken here and handed on in memory (smm::Header), so the host never waits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smm_plan.h"

namespace smm {

namespace {

using smc::block_scan;
using smc::copy_bytes;
using smc::sat32;

constexpr uint32_t kThreads = 256;

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

// ---- compress: plan ------------------------------------------------------------------------------
// The scans, by one workgroup: lfirst = the long streams' fragment slots, ifirst = the index entries
// of all streams.  hdr->stop: more of either than max_fragments holds (the index only when asked for).
__global__ __launch_bounds__(kThreads) void k_cplan_scan(const uint32_t* __restrict__ in_len, uint32_t n, uint32_t m,
                                                        int want_index, uint32_t* lfirst, uint32_t* ifirst, Header* hdr) {
  __shared__ uint64_t sh[4];
  uint64_t lcarry = 0, icarry = 0;
  for (uint32_t base = 0; base < n; base += kThreads) {  // (uniform: every thread takes every tile)
    const uint32_t s = base + threadIdx.x;
    const uint32_t len = s < n ? in_len[s] : 0u;
    const uint32_t cnt = len > kMaxInput ? 0u : fragment_count(len);
    uint64_t lt, it;
    const uint64_t lex = block_scan(len > kBlock ? cnt : 0u, sh, lt);
    const uint64_t iex = block_scan(cnt, sh, it);
    if (s < n) {
      lfirst[s] = sat32(lcarry + lex);
      ifirst[s] = sat32(icarry + iex);
    }
    lcarry += lt;
    icarry += it;
  }
  if (threadIdx.x == 0) {
    lfirst[n] = sat32(lcarry);
    ifirst[n] = sat32(icarry);
    hdr->nlong = sat32(lcarry);
    hdr->nindex = sat32(icarry);
    hdr->stop = lcarry > m || (want_index && icarry > m);
    hdr->indexed = 0;
  }
}

// The argument arrays of the two raw calls.  Thread i serves stream i and slot i.
//  - short call (one item per stream, headers on): a stream of at most 64 KiB as it is, into the
//    caller's slot; every other stream as the empty input into a dummy slot of its own.  The raw
//    call takes offsets from one base pointer, d_out: the dummy's is its distance from d_out
//    modulo 2^64, which the device's flat 64-bit address arithmetic turns back into its address.
//  - fragment call (one item per slot): slot j < nlong is fragment j - lfirst[s] of its stream s.
// After hdr->stop everything is empty and goes to scratch.
__global__ __launch_bounds__(kThreads) void k_cplan_fill(CompressPlan p) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool stop = p.hdr->stop != 0;
  if (i < p.n) {
    const uint32_t len = p.in_len[i];
    const bool direct = !stop && len <= kBlock;
    p.s.s_in_len[i] = direct ? len : 0u;
    p.s.s_out_off[i] = direct ? p.out_off[i] : (uint64_t)(uintptr_t)(p.s.dummy + (uint64_t)kDummy * i) - (uint64_t)(uintptr_t)p.out;
    p.s.bad[i] = 0;
  }
  if (i < p.m) {
    uint64_t off = 0;
    uint32_t len = 0, s = kNoStream;
    if (!stop && i < p.hdr->nlong) {
      s = owner(p.s.lfirst, p.n, i);
      const uint32_t f = i - p.s.lfirst[s];
      off = p.in_off[s] + (uint64_t)kBlock * f;
      len = min(kBlock, p.in_len[s] - kBlock * f);
    }
    p.s.f_in_off[i] = off;
    p.s.f_in_len[i] = len;
    p.s.f_slot_off[i] = kSlotPitch * i;
    p.s.f_stream[i] = s;
  }
}

hipError_t launch_compress_plan(const CompressPlan& p, hipStream_t st) {
  hipLaunchKernelGGL(k_cplan_scan, dim3(1), dim3(kThreads), 0, st, p.in_len, p.n, p.m, p.frag_first ? 1 : 0, p.s.lfirst,
                     p.s.ifirst, p.hdr);
  hipLaunchKernelGGL(k_cplan_fill, dim3(blocks_for(max(p.n, p.m))), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

// ---- compress: pack ------------------------------------------------------------------------------
// gpos = the exclusive scan of the fragments' compressed sizes over all slots, by one workgroup:
// fragment j of stream s then starts hv + gpos[j] - gpos[lfirst[s]] bytes into its stream.  A
// fragment whose size is an error mark counts nothing and flags its stream.
__global__ __launch_bounds__(kThreads) void k_pack_scan(const uint32_t* __restrict__ comp_len, const uint32_t* f_stream,
                                                       const Header* hdr, uint64_t* gpos, uint32_t* bad) {
  __shared__ uint64_t sh[4];
  const uint32_t total = hdr->stop ? 0u : hdr->nlong;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < total; base += kThreads) {
    const uint32_t j = base + threadIdx.x;
    uint32_t c = 0;
    if (j < total) {
      c = comp_len[j];
      if (c > (uint32_t)max_compressed_length(kBlock)) {  // an error mark (or no size a slot can hold)
        c = 0;
        bad[f_stream[j]] = 1;  // (any writer: the same value)
      }
    }
    uint64_t t;
    const uint64_t ex = block_scan(c, sh, t);
    if (j < total) gpos[j] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) gpos[total] = carry;
}

// The long streams.  blockIdx.x = the slot, blockIdx.y strides its bytes.  The slot's fragment goes
// behind its predecessor; the stream's fragment 0 also writes the header and the stream's results.
// A stream that would not fit sm_max_compressed_length(len) is not written (SM_ERR_DEVICE): the raw
// compressor's own bounds make that impossible, and a slot is never overrun on their word alone.
__global__ __launch_bounds__(kThreads) void k_pack(CompressPlan p) {
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  if (p.hdr->stop || j >= p.hdr->nlong) return;
  const uint32_t s = p.s.f_stream[j];
  const uint32_t j0 = p.s.lfirst[s], j1 = p.s.lfirst[s + 1];
  const uint32_t len = p.in_len[s], hv = varint_len(len);
  const uint64_t rel = p.s.gpos[j] - p.s.gpos[j0], total = hv + (p.s.gpos[j1] - p.s.gpos[j0]);
  const bool bad = p.s.bad[s] != 0 || total > max_compressed_length(len);
  uint8_t* const dst = p.out + p.out_off[s];
  if (blockIdx.y == 0) {
    if (t == 0 && p.frag_pos) p.frag_pos[p.s.ifirst[s] + (j - j0)] = bad ? 0u : (uint32_t)(hv + rel);
    if (j == j0) {
      if (t < hv && !bad) dst[t] = smc::varint_byte(len, t, hv);
      if (t == 0) {
        p.out_len[s] = bad ? 0u : (uint32_t)total;
        p.status[s] = bad ? SM_ERR_DEVICE : SM_OK;
      }
    }
  }
  if (bad) return;
  copy_bytes(p.slots + kSlotPitch * j, p.s.f_comp_len[j], dst + hv + rel, blockIdx.y * kThreads + t, gridDim.y * kThreads);
}

// Every other stream's results, and d_frag_first.  Thread i serves stream i (and entry n).
__global__ __launch_bounds__(kThreads) void k_cfinish(CompressPlan p) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i > p.n) return;
  const bool stop = p.hdr->stop != 0;
  if (p.frag_first && !stop) p.frag_first[i] = p.s.ifirst[i];
  if (i == p.n) return;
  const uint32_t len = p.in_len[i];
  if (stop || len > kMaxInput) {
    p.out_len[i] = 0;
    p.status[i] = stop ? SM_ERR_ARGUMENT : SM_ERR_INPUT_TOO_LARGE;
  } else if (len <= kBlock) {
    const uint32_t c = p.s.s_comp_len[i];
    const bool mark = c >= SM_OUT_LEN_ERROR;
    p.out_len[i] = mark ? 0u : c;
    p.status[i] = mark ? SM_ERR_DEVICE : SM_OK;
    if (p.frag_pos && len) p.frag_pos[p.s.ifirst[i]] = mark ? 0u : varint_len(len);
  }
}

hipError_t launch_pack(const CompressPlan& p, hipStream_t st) {
  if (p.m) {
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(kThreads), 0, st, p.s.f_comp_len, p.s.f_stream, p.hdr, p.s.gpos, p.s.bad);
    hipLaunchKernelGGL(k_pack, dim3(p.m, 4), dim3(kThreads), 0, st, p);
  }
  hipLaunchKernelGGL(k_cfinish, dim3(blocks_for(p.n + 1)), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

// ---- uncompress: plan ----------------------------------------------------------------------------
// The rules on d_frag_first and on each stream (smm_plan.h), and efirst = the scan of the candidates'
// fragment counts, by one workgroup.  A candidate's entries lie inside d_frag_pos whatever the rest
// of d_frag_first holds; with d_frag_first in order they are disjoint, so the candidates' fragments
// are at most max_fragments.  hdr->stop: d_frag_first is broken, no stream is indexed.
__global__ __launch_bounds__(kThreads) void k_dplan_scan(DecodePlan p) {
  __shared__ uint64_t sh[4];
  __shared__ int broken;
  if (threadIdx.x == 0) broken = 0;
  __syncthreads();
  uint64_t carry = 0;
  for (uint32_t base = 0; base < p.n; base += kThreads) {
    const uint32_t s = base + threadIdx.x;
    uint32_t cnt = 0;
    if (s < p.n) {
      if (!first_rule(p.frag_first, s, p.n, p.m)) broken = 1;  // (any writer: the same value)
      Candidate c{0, 0, 0, 0};
      const bool ok = stream_candidate(p.in + p.in_off[s], p.in_len[s], p.out_cap[s], p.frag_first[s], p.frag_first[s + 1],
                                       p.m, c);
      p.s.cand[s] = ok;
      p.s.D[s] = c.D;
      p.s.hv[s] = c.hv;
      p.s.e0[s] = c.e0;
      p.s.bad[s] = 0;
      cnt = ok ? c.count : 0u;
    }
    uint64_t t;
    const uint64_t ex = block_scan(cnt, sh, t);
    if (s < p.n) p.s.efirst[s] = sat32(carry + ex);
    carry += t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool stop = broken || carry > p.m;
    p.s.efirst[p.n] = sat32(carry);
    p.hdr->nlong = stop ? 0u : (uint32_t)carry;
    p.hdr->nindex = 0;
    p.hdr->stop = stop;
    p.hdr->indexed = 0;
  }
}

// The raw fragment decoder's arguments.  Slot j < nlong is fragment j - efirst[s] of candidate s:
// its bytes by the position rules, decoded straight to d_out_off[s] + 65536 f.  A fragment that
// breaks a rule is an empty item and flags its stream; the other slots are empty items.
__global__ __launch_bounds__(kThreads) void k_dplan_fill(DecodePlan p) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.m) return;
  uint64_t in_off = 0, out_off = 0;
  uint32_t in_len = 0, flen = 0, s = kNoStream;
  if (j < p.hdr->nlong) {
    s = owner(p.s.efirst, p.n, j);
    const uint32_t f = j - p.s.efirst[s], D = p.s.D[s], count = fragment_count(D);
    uint32_t lo, hi;
    if (fragment_range(p.frag_pos + p.s.e0[s], f, count, p.s.hv[s], p.in_len[s], lo, hi)) {
      in_off = p.in_off[s] + lo;
      in_len = hi - lo;
      out_off = p.out_off[s] + (uint64_t)kBlock * f;
      flen = fragment_length(D, f, count);
    } else {
      p.s.bad[s] = 1;  // (any writer: the same value)
    }
  }
  p.s.f_in_off[j] = in_off;
  p.s.f_in_len[j] = in_len;
  p.s.f_out_off[j] = out_off;
  p.s.f_len[j] = flen;
  p.s.f_stream[j] = s;
}

hipError_t launch_decode_plan(const DecodePlan& p, hipStream_t st) {
  hipLaunchKernelGGL(k_dplan_scan, dim3(1), dim3(kThreads), 0, st, p);
  if (p.m) hipLaunchKernelGGL(k_dplan_fill, dim3(blocks_for(p.m)), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

// ---- uncompress: reduce and merge -------------------------------------------------------------------
// a failing fragment flags its stream
__global__ __launch_bounds__(kThreads) void k_dverdict(DecodePlan p) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.hdr->nlong) return;
  if (p.s.f_status[j] != SM_OK) p.s.bad[p.s.f_stream[j]] = 1;
}

// The verdict per stream and the fallback's arguments: an indexed stream is masked out of it (an
// empty input, no room), every other stream goes in as the caller gave it.
__global__ __launch_bounds__(kThreads) void k_dreduce(DecodePlan p) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= p.n) return;
  const bool idx = !p.hdr->stop && p.s.cand[s] && !p.s.bad[s];
  p.s.indexed[s] = idx;
  p.s.fb_in_len[s] = idx ? 0u : p.in_len[s];
  p.s.fb_cap[s] = idx ? 0u : p.out_cap[s];
  if (idx) atomicAdd(&p.hdr->indexed, 1u);
}

hipError_t launch_reduce(const DecodePlan& p, hipStream_t st) {
  if (p.m) hipLaunchKernelGGL(k_dverdict, dim3(blocks_for(p.m)), dim3(kThreads), 0, st, p);
  hipLaunchKernelGGL(k_dreduce, dim3(blocks_for(p.n)), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

// the fallback wrote every stream's results; the indexed streams' own go over them
__global__ __launch_bounds__(kThreads) void k_dmerge(DecodePlan p) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= p.n || !p.s.indexed[s]) return;
  p.out_len[s] = p.s.D[s];
  p.status[s] = SM_OK;
}

hipError_t launch_merge(const DecodePlan& p, hipStream_t st) {
  hipLaunchKernelGGL(k_dmerge, dim3(blocks_for(p.n)), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace smm
