// sm_device.h -- CDNA4 wave primitives shared by the gfx950 kernels, over the format's constants
// and rules (sm_format.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_format.h"

namespace sm {

// ---- wave primitives -------------------------------------------------------------

__device__ inline uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ inline uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// the lane predicate of an SGPR lane mask (free: the mask is the predicate)
__device__ inline bool inverse_ballot(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

__device__ inline uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ inline uint32_t readlane(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }

__device__ inline uint32_t ctz64(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }

// inclusive wave-wide prefix sum (64 lanes)
__device__ inline uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += t;
  }
  return v;
}

// inclusive wave-64 scan with DPP (row_shr 1/2/4/8 within rows, row_bcast 15/31 across)
__device__ inline uint32_t scan_dpp(uint32_t v) {
  v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);
  return v;
}

// Unaligned little-endian loads from an LDS byte array, built from aligned dword reads +
// v_alignbyte_b32.  A misaligned ds_read_b32/b64 is serviced one lane per LDS cycle (~64
// cycles per wave-instruction) against 2-8 aligned and ~15 for this form on random
// addresses (tools/lds_bench.hip, measured on MI355X).
// the LDS byte address of a pointer into a __shared__ array
__device__ inline uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// lds_ld32: the array must have >= 4 readable bytes past pos+3.
__device__ inline uint32_t lds_ld32(const uint8_t* lds, uint32_t pos) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(lds + (pos & ~3u));
  uint32_t lo = w[0], hi = w[1];
  return __builtin_amdgcn_alignbyte(hi, lo, pos);  // (v_alignbyte_b32 shifts by 8 * S2[1:0]: no & 3)
}

// lds_ld64: >= 4 readable bytes past pos+7.
__device__ inline uint64_t lds_ld64(const uint8_t* lds, uint32_t pos) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(lds + (pos & ~3u));
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], sh = pos;  // (alignbyte: S2[1:0] only)
  return ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32) | __builtin_amdgcn_alignbyte(w1, w0, sh);
}

__device__ inline uint32_t hash32(uint32_t bytes, uint32_t shift) { return (bytes * kHashMul) >> shift; }

// Wave-cooperative copy of len bytes from an LDS byte array (at s) to global memory.
// 16-byte-aligned stores for the body; byte stores for the unaligned head/tail.
__device__ inline void wave_copy_lds_to_global(uint8_t* __restrict__ g, const uint8_t* lds, uint32_t s,
                                               uint32_t len, uint32_t lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)g & 15)) & 15);
  if (head > len) head = len;
  if (lane < head) g[lane] = lds[s + lane];
  g += head; s += head; len -= head;
  uint32_t n16 = len >> 4;
  uint4* g16 = reinterpret_cast<uint4*>(g);
  for (uint32_t k = lane; k < n16; k += kWave) {
    uint32_t p = s + 16 * k;
    uint4 v;
    v.x = lds_ld32(lds, p);
    v.y = lds_ld32(lds, p + 4);
    v.z = lds_ld32(lds, p + 8);
    v.w = lds_ld32(lds, p + 12);
    g16[k] = v;
  }
  uint32_t done = n16 << 4;
  if (lane < len - done) g[done + lane] = lds[s + done + lane];
}

// Wave-cooperative global->LDS load of len bytes (block staging).  lds must be 16-B
// aligned; src may have any alignment.
__device__ inline void wave_load_global_to_lds(uint8_t* lds, const uint8_t* __restrict__ src, uint32_t len,
                                               uint32_t lane) {
  if (((uintptr_t)src & 15) == 0) {
    const uint4* s16 = reinterpret_cast<const uint4*>(src);
    uint4* d16 = reinterpret_cast<uint4*>(lds);
    uint32_t n16 = len >> 4;
    for (uint32_t k = lane; k < n16; k += kWave) d16[k] = s16[k];
    for (uint32_t k = (n16 << 4) + lane; k < len; k += kWave) lds[k] = src[k];
  } else if (((uintptr_t)src & 3) == 0) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(lds);
    uint32_t n4 = len >> 2;
    for (uint32_t k = lane; k < n4; k += kWave) d4[k] = s4[k];
    for (uint32_t k = (n4 << 2) + lane; k < len; k += kWave) lds[k] = src[k];
  } else {
    for (uint32_t k = lane; k < len; k += kWave) lds[k] = src[k];
  }
}

// first i (relative) at which a[i1+i] != a[i2+i], capped at avail; LDS-resident bytes.
// One wave round compares 256 bytes (4 per lane).  Reads stay below i2+avail+3 (clamped).
__device__ inline uint32_t wave_match_length(const uint8_t* lds, uint32_t i1, uint32_t i2, uint32_t avail,
                                             uint32_t lane) {
  uint32_t base = 0;
  for (;;) {
    uint32_t off = base + 4 * lane;
    uint32_t res;
    bool stop;
    if (off >= avail) {
      res = avail; stop = true;
    } else {
      uint32_t x = lds_ld32(lds, i1 + off) ^ lds_ld32(lds, i2 + off);
      uint32_t fb = x ? (uint32_t)(__builtin_ctz(x) >> 3) : 4u;
      res = off + fb;
      if (res > avail) res = avail;
      stop = (fb < 4) || (off + 4 >= avail);
    }
    uint64_t m = ballot(stop);
    if (m) return readlane(res, ctz64(m));
    base += 4 * kWave;
  }
}

}  // namespace sm
