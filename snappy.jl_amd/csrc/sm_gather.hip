// sm_gather.hip -- the assembly kernels behind the compressors: compressed fragments and parts to
// their places in one stream or in the caller's slots.  They serve the fast modes, the single-buffer
// call and the sharded API alike; none of them parses.
#include "sm_device.h"
#include "sm_internal.h"

namespace sm {

// ---- gather (single-stream assembly) ---------------------------------------------------

__global__ __launch_bounds__(256) void k_gather(const uint8_t* __restrict__ src, const uint64_t* src_off,
                                                 const uint32_t* len, const uint64_t* dst_off,
                                                 uint8_t* __restrict__ dst) {
  const uint32_t b = blockIdx.x;
  const uint8_t* s = src + src_off[b];
  uint8_t* d = dst + dst_off[b];
  const uint32_t n = len[b];
  for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) d[k] = s[k];
}

// ---- the single-buffer call's device-side bookkeeping (sm_compress, small inputs) ----------
// Fragment f of the input is [64 KiB f, +64 KiB) and compresses into slot f (fixed pitch).
__global__ __launch_bounds__(256) void k_frag_plan(uint64_t n, uint32_t nfrag, uint64_t slot, uint64_t* in_off,
                                                   uint32_t* in_len, uint64_t* out_off) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nfrag) return;
  const uint64_t b = (uint64_t)f * kBlockSize;
  in_off[f] = b;
  in_len[f] = (uint32_t)min((uint64_t)kBlockSize, n - b);
  out_off[f] = (uint64_t)f * slot;
}

// n bytes from s8 (16-byte aligned) to g (any alignment) by the workgroup's part y of ny:
// aligned 16-byte stores of byte-shifted units, the partial units at both ends by bytes (part 0;
// they share a 16-byte unit with the neighbouring pieces)
__device__ __attribute__((always_inline)) inline void gather_unit(const uint8_t* __restrict__ s8, uint32_t n,
                                                                 uint8_t* __restrict__ g, uint32_t y, uint32_t ny) {
  const uint4* s16 = reinterpret_cast<const uint4*>(s8);
  const uint32_t ad = (uint32_t)((uintptr_t)g & 15);
  const uint32_t u0 = ad ? 1u : 0u, u1 = (n + ad) >> 4;  // whole units [u0, u1); unit u = bytes [16u - ad, +16)
  uint4* const g16 = reinterpret_cast<uint4*>(g - ad);
  const uint32_t sb = (16 - ad) & 15, dw = sb >> 2, bs = sb & 3;
  const uint32_t stride = blockDim.x * ny;
  for (uint32_t u = u0 + y * blockDim.x + threadIdx.x; u < u1; u += stride) {
    const uint32_t j = 16 * u - ad;
    // the second granule only when the unit straddles two (sb != 0: it then holds source byte 16u < n);
    // for an aligned g it would lie wholly past the piece on its last unit
    const uint4 A = s16[j >> 4], B = sb ? s16[(j >> 4) + 1] : make_uint4(0, 0, 0, 0);
    const uint32_t x[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint32_t r5[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      uint32_t vv = x[q];
#pragma unroll
      for (int dd = 1; dd < 4; ++dd) vv = dw == (uint32_t)dd ? x[q + dd] : vv;
      r5[q] = vv;
    }
    g16[u] = make_uint4(__builtin_amdgcn_alignbyte(r5[1], r5[0], bs), __builtin_amdgcn_alignbyte(r5[2], r5[1], bs),
                        __builtin_amdgcn_alignbyte(r5[3], r5[2], bs), __builtin_amdgcn_alignbyte(r5[4], r5[3], bs));
  }
  if (y == 0) {
    const uint32_t nh = min(u0 ? 16 - ad : 0u, n);
    const uint32_t tb = max(16 * u1 > ad ? 16 * u1 - ad : 0u, nh);
    if (threadIdx.x < nh + (n - tb)) {
      const uint32_t jj = threadIdx.x < nh ? threadIdx.x : tb + (threadIdx.x - nh);
      g[jj] = s8[jj];
    }
  }
}

// Fragment b's len[b] bytes from src + src_off[b] (16-byte aligned) to dst + (the lengths of
// fragments 0..b-1, one lane each: nfrag <= 64) at any alignment: aligned 16-byte stores of
// byte-shifted units, the partial units at both ends by bytes (they share a 16-byte unit with the
// neighbouring fragments); blockIdx.y strides the units.  tot[0] = the sum, tot[1] = 1 when a
// length is an error mark or over its fragment's bound (never expected): then nothing is copied.
__global__ __launch_bounds__(256) void k_gather16(const uint8_t* __restrict__ src, const uint64_t* src_off,
                                                  const uint32_t* len, const uint32_t* in_len, uint32_t nfrag,
                                                  uint64_t* tot, uint8_t* __restrict__ dst) {
  __shared__ uint32_t sh[2];
  const uint32_t b = blockIdx.x;
  if (threadIdx.x < kWave) {
    const uint32_t l = threadIdx.x;
    const uint32_t L = l < nfrag ? len[l] : 0u;
    const bool bad = l < nfrag && (uint64_t)L > 32 + (uint64_t)in_len[l] + in_len[l] / 6;
    const uint32_t before = scan_dpp(l < b ? L : 0u);  // (lanes < b: their lengths; < 2^17 each)
    const uint32_t all = scan_dpp(bad ? 0u : L);
    const bool anybad = ballot(bad) != 0;
    if (l == 63) {
      sh[0] = before;
      sh[1] = anybad;
      if (b == 0 && blockIdx.y == 0) {
        tot[0] = all;
        tot[1] = anybad;
      }
    }
  }
  __syncthreads();
  if (sh[1]) return;
  gather_unit(src + src_off[b], len[b], dst + sh[0], blockIdx.y, gridDim.y);
}

// The head of a block written as one literal (block_literal_head_byte: the varint when the block
// carries its header, then the tag) at g, by the workgroup's first threads; returns its size
__device__ inline uint32_t put_literal_head(uint8_t* g, uint32_t n, bool header, bool writes) {
  const uint32_t h = block_literal_bytes(n, header) - n;
  if (writes && threadIdx.x < h) g[threadIdx.x] = block_literal_head_byte(n, header, threadIdx.x);
  return h;
}

// k_gather16 for the parts of k_compress_sc_span: unit u = part u % parts of block u / parts (one
// thread each: nblk * parts <= 256, parts a power of 2 <= 64, so a block's parts are lanes of one
// wave), at src + out_off[block] + part pitch.  A block whose parts sum to more than one literal
// of the block is written as that literal instead, from the input.  tot[0] = the total; tot[1] =
// 1 on an error mark or an over-long part (nothing is copied).
// This is parts_verdict's rule (sm_format.h) with every part on a thread of its own: the sum by
// butterfly, the offsets by a scan over all blocks' parts.  The call is on the single-buffer
// path's latency, where the rule as a loop per thread cost 2.5 to 3 us of 53 (DESIGN.md section
// 3.7), so the bounds stay written out here; the literal's size and head come from the shared rules.
__global__ __launch_bounds__(256) void k_gather_parts(const uint8_t* __restrict__ src, const uint64_t* out_off,
                                                      ScSpan sp, const uint8_t* __restrict__ in,
                                                      const uint64_t* in_off, const uint32_t* in_len, uint32_t nunit,
                                                      uint64_t* tot, uint8_t* __restrict__ dst) {
  __shared__ uint32_t wsum[4], ex[256], eff[256], code;
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t L = t < nunit ? sp.part_len[t] : 0u;
  const uint32_t nb = t < nunit ? in_len[t / sp.parts] : 0u;
  const uint32_t lit = block_literal_bytes(nb, false);
  // error marks (>= kOutLenError), and any part longer than its pitch; part 0 may instead be a
  // screened block's literal (parts_verdict's part0_literal)
  const uint32_t bound = (t % sp.parts == 0) ? max((uint32_t)sp.pitch, lit + 5u) : (uint32_t)sp.pitch;
  const bool big = t < nunit && L > bound;
  const uint32_t Lv = big ? 0u : L;
  uint32_t sum = Lv;  // the block's parts
  for (uint32_t d = 1; d < sp.parts; d <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)d, 64);
  const bool over = t < nunit && nb && sum > lit;
  const uint32_t E = over ? (t % sp.parts == 0 ? lit : 0u) : Lv;  // this unit's bytes in the stream
  const uint32_t inc = scan_dpp(E);
  const uint64_t anybig = ballot(big);
  if (t == 0) code = 0;
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  if (lane == 0 && anybig) code = 1;
  uint32_t pre = 0;
  for (uint32_t k = 0; k < w; ++k) pre += wsum[k];
  ex[t] = pre + inc - E;
  eff[t] = over ? 1u : 0u;
  __syncthreads();
  const uint32_t u = blockIdx.x;
  if (u == 0 && blockIdx.y == 0 && t == 0) {
    tot[0] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    tot[1] = code;
  }
  if (code) return;
  const uint32_t b = u / sp.parts, j = u % sp.parts;
  uint8_t* const g = dst + ex[u];
  if (!eff[u]) {
    gather_unit(src + out_off[b] + (uint64_t)j * sp.pitch, sp.part_len[u], g, blockIdx.y, gridDim.y);
  } else if (j == 0) {  // the block as one literal: its tag, then its bytes
    const uint32_t n = in_len[b];
    gather_unit(in + in_off[b], n, g + put_literal_head(g, n, false, blockIdx.y == 0), blockIdx.y, gridDim.y);
  }
}

// The parts of the device batch calls' remainder blocks (k_compress_sc_span with sp.blk_pitch) into
// the caller's slots: workgroup (u, y) takes part j = u % parts of block b = u / parts (a's arrays
// start at the first remainder block), which goes behind the block's parts before it at a.out +
// a.out_off[b]; a.out_len[b] = parts_verdict's bytes, or its mark (nothing is copied).  What the
// whole-block kernel's writer does per block is done here: a block whose parts sum to more than
// one literal of the block is written as that literal from the input, and an empty block is its
// header alone.  A block the screen emitted is in its slot already.
__global__ __launch_bounds__(256) void k_gather_parts_batch(CompressArgs a, const uint8_t* __restrict__ src, ScSpan sp) {
  const uint32_t b = blockIdx.x / sp.parts, j = blockIdx.x % sp.parts, t = threadIdx.x;
  const uint32_t* const pl = sp.part_len + b * sp.parts;
  if (pl[0] == kPartScreened) return;  // (the screen wrote a.out_len[b] too)
  const bool first = j == 0 && blockIdx.y == 0;
  const uint32_t n = a.in_len[b];
  // (uniform: at most 16 lengths)
  const PartsVerdict v = parts_verdict(pl, sp.parts, j, (uint32_t)sp.pitch, n, a.header != 0, false);
  if (first && t == 0) a.out_len[b] = v.mark ? v.mark : v.bytes;
  if (v.mark) return;
  uint8_t* const dst = a.out + a.out_off[b];
  if (!v.literal) {
    gather_unit(src + b * sp.blk_pitch + j * sp.pitch, pl[j], dst + v.before, blockIdx.y, gridDim.y);
    return;
  }
  if (j) return;  // one literal: the header, the tag, the block's bytes (any alignment: by bytes)
  const uint32_t h = put_literal_head(dst, n, a.header != 0, blockIdx.y == 0);
  const uint8_t* const in = a.in + a.in_off[b];
  for (uint32_t k = blockIdx.y * blockDim.x + t; k < n; k += blockDim.x * gridDim.y) dst[h + k] = in[k];
}

// ---- a sharded stream's fragments at their places in it (Snappy.jl:29-35) ----------
// Fragment b (len[b] bytes at src + src_off[b]) to dst + (dst_off[b] - base): dst_off[b] is the
// fragment's offset in the whole stream (the all-gathered exclusive scan behind the varint
// header), base = 0 with the header (dst is the stream from its first byte and varint(total) is
// written there) or dst_off[0] without it (dst is the caller's byte range from its first
// fragment).  loc_off[b] (optional) receives dst_off[b] - base.  A length that is an error mark,
// a fragment that would end past cap, or with the header a fragment that would start inside it
// (dst_off[b] < varint_len(total): its bytes would race the header's), copies nothing and sets
// *status = SM_ERR_DEVICE (optional; never cleared here).  blockIdx.y strides the fragment's
// 16-byte units.
__global__ __launch_bounds__(256) void k_place(const uint8_t* __restrict__ src, const uint64_t* src_off,
                                               const uint32_t* len, const uint64_t* dst_off, uint32_t nfrag,
                                               uint64_t total, int header, uint64_t cap, uint8_t* __restrict__ dst,
                                               uint64_t* loc_off, int32_t* status) {
  const uint32_t b = blockIdx.x;
  if (header && b == 0 && blockIdx.y == 0) {  // varint(total), src/varint.jl:46-69
    const uint32_t hv = varint_len((uint32_t)total);
    if (threadIdx.x < hv && threadIdx.x < cap) dst[threadIdx.x] = varint_byte((uint32_t)total, threadIdx.x, hv);
  }
  if (b >= nfrag) return;  // (an empty stream: the header alone)
  const uint64_t base = header ? 0ull : dst_off[0];
  const uint32_t n = len[b];
  const uint64_t at = dst_off[b] - base;  // (a mark earlier in the scan wraps this past cap)
  const bool bad = n >= kOutLenError || at > cap || cap - at < n || (header && at < varint_len((uint32_t)total));
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    if (loc_off) loc_off[b] = at;
    if (bad && status) *status = kErrDevice;
  }
  if (bad) return;
  const uint8_t* const s = src + src_off[b];
  if (((uintptr_t)s & 15) == 0) {
    gather_unit(s, n, dst + at, blockIdx.y, gridDim.y);
  } else {
    for (uint32_t k = blockIdx.y * blockDim.x + threadIdx.x; k < n; k += blockDim.x * gridDim.y) dst[at + k] = s[k];
  }
}

hipError_t launch_place(const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint64_t* dst_off,
                        uint32_t nfrag, uint64_t total, int header, uint64_t cap, uint8_t* dst, uint64_t* loc_off,
                        int32_t* status, hipStream_t s) {
  if (nfrag == 0 && !header) return hipSuccess;
  hipLaunchKernelGGL(k_place, dim3(max(nfrag, 1u), 4), dim3(256), 0, s, src, src_off, len, dst_off, nfrag, total, header,
                     cap, dst, loc_off, status);
  return hipGetLastError();
}

hipError_t launch_frag_plan(uint64_t n, uint32_t nfrag, uint64_t slot, uint64_t* in_off, uint32_t* in_len,
                            uint64_t* out_off, hipStream_t s) {
  hipLaunchKernelGGL(k_frag_plan, dim3((nfrag + 255) / 256), dim3(256), 0, s, n, nfrag, slot, in_off, in_len, out_off);
  return hipGetLastError();
}

hipError_t launch_parts_gather(const uint8_t* src, const uint64_t* out_off, const ScSpan& sp, const uint8_t* in,
                               const uint64_t* in_off, const uint32_t* in_len, uint32_t nblk, uint64_t* tot,
                               uint8_t* dst, hipStream_t s) {
  const uint32_t nunit = nblk * sp.parts;
  if (nblk == 0 || sp.parts == 0 || sp.parts > kWave || (sp.parts & (sp.parts - 1)) || nunit > 256)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_parts, dim3(nunit, 4), dim3(256), 0, s, src, out_off, sp, in, in_off, in_len, nunit,
                     tot, dst);
  return hipGetLastError();
}

hipError_t launch_batch_parts_gather(const CompressArgs& a, const uint8_t* src, const ScSpan& sp, hipStream_t s) {
  if (a.nblk == 0 || sp.parts == 0 || sp.blk_pitch == 0) return hipErrorInvalidValue;
  // (a part of at most 8 super-chunks is one or two passes of a workgroup's 16-byte units)
  k_gather_parts_batch<<<dim3(a.nblk * sp.parts, sp.span > 8 ? 4 : 1), dim3(256), 0, s>>>(a, src, sp);
  return hipGetLastError();
}

hipError_t launch_frag_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* out_len,
                              const uint32_t* in_len, uint32_t nfrag, uint64_t* tot, uint8_t* dst, hipStream_t s) {
  if (nfrag == 0 || nfrag > kWave) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather16, dim3(nfrag, 4), dim3(256), 0, s, src, src_off, out_len, in_len, nfrag, tot, dst);
  return hipGetLastError();
}

hipError_t launch_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* len,
                         const uint64_t* dst_off, uint8_t* dst, uint32_t nblk, hipStream_t s) {
  if (nblk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather, dim3(nblk), dim3(256), 0, s, src, src_off, len, dst_off, dst);
  return hipGetLastError();
}

}  // namespace sm
