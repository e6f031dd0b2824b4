// smf_kernels.hip -- the framing format's gfx950 kernels and their launchers (smf_internal.h).
//
// k_crc32c is the hot path: it reads every byte once more than the raw codec does.  gfx950 has no
// CRC or carry-less-multiply instruction, so a block's CRC is table lookups in LDS, made parallel
// by the CRC's linearity over GF(2) (see k_crc32c).  The other kernels are plumbing around the raw
// codec's batched calls: per-block planning and scans by one workgroup, byte copies, the one-wave
// chunk walker.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smf_device.h"
#include "smf_format.h"
#include "smf_internal.h"

namespace smf {

namespace {

using smc::block_scan;
using smc::copy_bytes;
using smc::kWave;

__device__ inline uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

}  // namespace

// ---- CRC-32C of a batch of blocks ----------------------------------------------------------------
// One workgroup of kCrcThreads lanes per block (grid-strided, so the tables are staged in LDS once
// per workgroup).  The block is [head bytes][G aligned 16-byte granules][tail bytes], head and tail
// shorter than a granule.  Lane t takes the granules at distance r = t, t + 256, ... from the last
// one, oldest first, as coalesced 16-byte loads: a lane's register, 256 granules old, is advanced by
// four lookups (tab[16..19]) and the new granule enters by sixteen (tab[0..15]) -- all independent,
// so nothing but the xor tree is serial.  Its register then stands t granules before the end:
// times x^(128 t) (gf_mul, once per block).  The registers add up (xor) over the workgroup.  The
// 0xffffffff init lives in the head alone: the lane that owns the head runs it bytewise from the
// init and multiplies by x^(128 G).  The tail runs bytewise behind the sum.
// LDS: 20 KiB of tables; the lookups are random over the 32 banks of ds_read_b32 (about 3.5
// lanes on the busiest bank of a 32-lane group) -- measured rates: DESIGN.md section 8.
__global__ __launch_bounds__(kCrcThreads) void k_crc32c(const uint8_t* __restrict__ in, const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ len, uint32_t nblk,
                                                        uint32_t* __restrict__ crc, int masked,
                                                        const CrcLut* __restrict__ T) {
  __shared__ uint32_t tab[kCrcTabs * 256];
  __shared__ uint32_t red[kCrcThreads / kWave];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t i = t; i < kCrcTabs * 256; i += kCrcThreads) tab[i] = (&T->tab[0][0])[i];
  const uint32_t mult = T->xpow[t];  // x^(128 t)
  __syncthreads();
  for (uint32_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const uint8_t* p = in + off[b];
    const uint32_t n = len[b];
    const uint32_t head = min(n, (16u - (uint32_t)((uintptr_t)p & 15)) & 15u);
    const uint32_t G = (n - head) / 16;
    const uint4* g = reinterpret_cast<const uint4*>(p + head);
    uint32_t s = 0;
    if (t < G) {
      uint32_t idx = (G - 1 - t) % kCrcThreads;       // this lane's oldest granule
      uint32_t cnt = (G - 1 - t) / kCrcThreads + 1;  // and how many it owns
      for (; cnt >= 4; cnt -= 4, idx += 4 * kCrcThreads) {
        const uint4 v0 = g[idx], v1 = g[idx + kCrcThreads], v2 = g[idx + 2 * kCrcThreads], v3 = g[idx + 3 * kCrcThreads];
        s = crc_granule(tab, s, &v0.x);
        s = crc_granule(tab, s, &v1.x);
        s = crc_granule(tab, s, &v2.x);
        s = crc_granule(tab, s, &v3.x);
      }
      for (; cnt; --cnt, idx += kCrcThreads) {
        const uint4 v = g[idx];
        s = crc_granule(tab, s, &v.x);
      }
      s = gf_mul(mult, s);
    }
    if (t == kCrcThreads - 1) {  // (the lane with the fewest granules)
      uint32_t h = 0xffffffffu;
      for (uint32_t i = 0; i < head; ++i) h = tab[15 * 256 + ((h ^ p[i]) & 0xff)] ^ (h >> 8);
      s ^= gf_mul(gf_xpow(T, G), h);
    }
    for (uint32_t d = 1; d < kWave; d <<= 1) s ^= (uint32_t)__shfl_xor((int)s, (int)d, kWave);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (t == 0) {
      uint32_t c = red[0] ^ red[1] ^ red[2] ^ red[3];
      for (uint32_t i = head + 16 * G; i < n; ++i) c = tab[15 * 256 + ((c ^ p[i]) & 0xff)] ^ (c >> 8);
      c ^= 0xffffffffu;
      crc[b] = masked ? mask(c) : c;
    }
    __syncthreads();  // (red is read before the next block's sums land)
  }
}

hipError_t launch_crc32c(const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t nblk, uint32_t* crc,
                         int masked, const CrcLut* T, hipStream_t s) {
  if (nblk == 0) return hipSuccess;
  // 8 workgroups fit a CU (20.5 KiB of LDS each); beyond 256 CUs' worth the blocks are strided
  hipLaunchKernelGGL(k_crc32c, dim3(min(nblk, 2048u)), dim3(kCrcThreads), 0, s, in, off, len, nblk, crc, masked, T);
  return hipGetLastError();
}

// ---- compress ------------------------------------------------------------------------------------
// block b = input [64 KiB b, +64 KiB) -> slot b (pitch bytes each)
__global__ __launch_bounds__(256) void k_frame_blocks(uint64_t n, uint32_t nblk, uint64_t pitch, uint64_t* in_off,
                                                      uint32_t* in_len, uint64_t* slot_off) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblk) return;
  const uint64_t o = (uint64_t)b * kBlock;
  in_off[b] = o;
  in_len[b] = (uint32_t)min((uint64_t)kBlock, n - o);
  slot_off[b] = (uint64_t)b * pitch;
}

// The encoder rule and the chunks' places, by one workgroup: block b is a 0x00 chunk iff its
// Snappy stream is strictly shorter than the block, else a 0x01 chunk; dst_off[b] = 10 + the sizes
// of the chunks before it.  An error mark packs nothing (type kTypeNone) and sets SM_ERR_DEVICE.
__global__ __launch_bounds__(256) void k_frame_scan(const uint32_t* comp_len, const uint32_t* in_len, uint32_t nblk,
                                                    uint8_t* type, uint64_t* dst_off, uint64_t* out_len,
                                                    int32_t* status) {
  __shared__ uint64_t sh[4];
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  uint64_t carry = SMF_IDENTIFIER_LENGTH;
  for (uint32_t base = 0; base < nblk; base += 256) {  // (uniform: every thread takes every tile)
    const uint32_t b = base + threadIdx.x;
    uint64_t size = 0;
    if (b < nblk) {
      uint8_t ty;
      size = encoder_chunk(comp_len[b], in_len[b], ty);
      type[b] = ty;
      if (ty == kTypeNone) bad = 1;  // (any writer: the same value)
    }
    uint64_t total;
    const uint64_t ex = block_scan(size, sh, total);
    if (b < nblk) dst_off[b] = carry + ex;
    carry += total;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *out_len = carry;
    *status = bad ? SM_ERR_DEVICE : SM_OK;
  }
}

// The identifier, the chunk headers and the payloads, packed behind one another.  blockIdx.x = the
// block, blockIdx.y strides the payload.
__global__ __launch_bounds__(256) void k_frame_pack(const uint8_t* __restrict__ in, const uint64_t* in_off,
                                                    const uint32_t* in_len, const uint8_t* __restrict__ slots,
                                                    const uint64_t* slot_off, const uint32_t* comp_len,
                                                    const uint32_t* crc, const uint8_t* type, const uint64_t* dst_off,
                                                    uint32_t nblk, uint8_t* __restrict__ dst) {
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  if (b == 0 && blockIdx.y == 0 && t < SMF_IDENTIFIER_LENGTH) {
    const uint8_t id[SMF_IDENTIFIER_LENGTH] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
    dst[t] = id[t];
  }
  if (b >= nblk) return;  // (the empty input: the identifier alone)
  pack_chunk(type[b], in + in_off[b], in_len[b], slots + slot_off[b], comp_len[b], crc[b], dst + dst_off[b]);
}

hipError_t launch_frame_compress_plan(uint64_t n, uint32_t nblk, uint64_t pitch, uint64_t* in_off, uint32_t* in_len,
                                      uint64_t* slot_off, hipStream_t s) {
  if (nblk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_frame_blocks, dim3((nblk + 255) / 256), dim3(256), 0, s, n, nblk, pitch, in_off, in_len, slot_off);
  return hipGetLastError();
}

hipError_t launch_frame_pack(const PackArgs& a, uint64_t* out_len, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_frame_scan, dim3(1), dim3(256), 0, s, a.comp_len, a.in_len, a.nblk, a.type, a.dst_off, out_len,
                     status);
  hipLaunchKernelGGL(k_frame_pack, dim3(max(a.nblk, 1u), 4), dim3(256), 0, s, a.in, a.in_off, a.in_len, a.slots,
                     a.slot_off, a.comp_len, a.crc, a.type, a.dst_off, a.nblk, a.dst);
  return hipGetLastError();
}

// ---- index ---------------------------------------------------------------------------------------
// One wave walks the chunk chain.  A step's bytes (header, CRC, varint: kHeadBytes) come in by one
// load, a byte a lane, and every lane then takes the same step, so a chunk costs one dependent load.
// The loop and the fetch are walk_stream's and WaveFetch's, written out: through them the compiler
// turns the varint's branches into selects on the dependent chain, and smf_uncompress_device's walk
// of 10,000 chunks measured 0.13 ms (1 %) slower than this form.  stored == 0: count only.
__global__ __launch_bounds__(64) void k_frame_index(const uint8_t* __restrict__ in, uint64_t n, smf_chunks ch, int stored,
                                                    uint32_t max_chunks, smf_summary* sum) {
  const uint32_t lane = lane_id();
  Walk w;
  uint64_t pos = 0;
  for (;;) {
    const uint32_t have = pos < n ? (uint32_t)min((uint64_t)kHeadBytes, n - pos) : 0u;
    const uint32_t mine = lane < have ? in[pos + lane] : 0u;
    uint8_t h[kHeadBytes];
#pragma unroll
    for (uint32_t i = 0; i < kHeadBytes; ++i) h[i] = (uint8_t)__shfl((int)mine, (int)i, kWave);
    Chunk c;
    if (!walk_step(w, h, have, pos, n, c)) break;
    if (c.data) {
      if (stored && w.nchunks < max_chunks && lane == 0) store_chunk(ch, w.nchunks, c);
      ++w.nchunks;
      w.total += c.ulen;
    }
    pos = c.next;
  }
  if (lane == 0) {
    sum->total_length = w.total;
    sum->nchunks = w.nchunks;
    sum->status = walk_status(w, stored != 0, max_chunks);
  }
}

hipError_t launch_frame_index(const uint8_t* in, uint64_t n, const smf_chunks* ch, uint32_t max_chunks, smf_summary* sum,
                              hipStream_t s) {
  smf_chunks c = ch ? *ch : smf_chunks{nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(k_frame_index, dim3(1), dim3(64), 0, s, in, n, c, ch ? 1 : 0, max_chunks, sum);
  return hipGetLastError();
}

__global__ void k_frame_result(uint64_t* d_len, uint64_t len, const smf_summary* sum, int32_t* d_status, int32_t status) {
  if (threadIdx.x != 0) return;
  if (sum) {  // (smf_uncompressed_length_device: the walk's summary, still on the device)
    len = sum->total_length;
    status = sum->status;
  }
  if (d_len) *d_len = len;
  if (d_status) *d_status = status;
}

hipError_t launch_frame_result(uint64_t* d_len, uint64_t len, const smf_summary* sum, int32_t* d_status, int32_t status,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_frame_result, dim3(1), dim3(64), 0, s, d_len, len, sum, d_status, status);
  return hipGetLastError();
}

// ---- uncompress ----------------------------------------------------------------------------------
// Chunk c's place (the scan of the declared lengths) and what the raw decoder gets for it, by one
// workgroup.  pre[c]: SM_OK, or why the chunk is not decoded.  cap[c] = its declared length (0 when
// not decoded): the decoder's capacity and the CRC pass's length.  dec_len[c] = the payload's length
// for a 0x00 chunk to decode, else 0 -- the raw decoder returns at once on an empty stream
// (its status for that chunk is not looked at).
__global__ __launch_bounds__(256) void k_frame_plan(smf_chunks ch, uint32_t nchunks, uint64_t out_capacity, Slots s,
                                                    uint64_t* out_len) {
  __shared__ uint64_t sh[4];
  const uint64_t total = smc::tile_scan(nchunks, sh, [&](uint32_t c) { return ch.ulen[c]; }, [&](uint32_t c, uint64_t ulen, uint64_t o) {
    const uint32_t ty = ch.type[c], pl = ch.pay_len[c], u = (uint32_t)ulen;
    int32_t st = SM_OK;
    if (ty > SMF_CHUNK_UNCOMPRESSED) st = SM_ERR_ARGUMENT;
    else if (u > kBlock || (ty == SMF_CHUNK_UNCOMPRESSED && pl != u)) st = SMF_ERR_CHUNK_TOO_LARGE;
    else if (o > out_capacity || out_capacity - o < u) st = SM_BUFFER_TOO_SMALL;
    s.out_off[c] = o;
    s.pre[c] = st;
    s.cap[c] = st == SM_OK ? u : 0u;
    s.dec_len[c] = st == SM_OK && ty == SMF_CHUNK_COMPRESSED ? pl : 0u;
  });
  if (threadIdx.x == 0) {
    *out_len = total;
    s.fail[0] = kNoSlot;
  }
}

// ---- the slot stage (smf_slots.h) -----------------------------------------------------------------
// 0x01 slots: the payload is the output.  blockIdx.x = the slot, blockIdx.y strides the payload.
__global__ __launch_bounds__(256) void k_slot_copy(const uint8_t* __restrict__ in, uint8_t* __restrict__ out_base,
                                                   Slots s) {
  const uint32_t j = blockIdx.x;
  if (s.type[j] != SMF_CHUNK_UNCOMPRESSED) return;
  copy_bytes(in + s.in_off[j], s.cap[j], at(out_base, s.out_off[j]), blockIdx.y * blockDim.x + threadIdx.x,
             gridDim.y * blockDim.x);
}

// Per slot its verdict (slot_verdict); a failing slot enters its group's minimum.
__global__ __launch_bounds__(256) void k_slot_verify(Slots s, uint32_t m) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t g = s.group ? s.group[j] : 0u;
  int32_t st = SM_OK;
  if (g != kNoSlot) {
    st = slot_verdict(s.pre ? s.pre[j] : (int32_t)SM_OK, s.type[j], s.dec_status[j], s.crc_out[j], s.crc_want[j]);
    if (st != SM_OK) atomicMin(&s.fail[g], j);
  }
  s.slot_status[j] = st;
}

// Per group its status (group_verdict) and the length it reports.
__global__ __launch_bounds__(256) void k_group_result(Slots s, Groups g) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= g.n) return;
  const bool over = g.hdr && g.hdr->over;
  const uint32_t f = s.fail[r];
  const int32_t st =
      group_verdict(over, g.pre ? g.pre[r] : (int32_t)SM_OK, f, f != kNoSlot ? s.slot_status[f] : (int32_t)SM_OK);
  g.status[r] = st;
  if (g.out_len) g.out_len[r] = over || (st != SM_OK && !g.len_on_error) ? 0 : g.len[r];
}

hipError_t launch_frame_plan(const smf_chunks& ch, uint32_t nchunks, uint64_t out_capacity, const Slots& sl,
                             uint64_t* out_len, hipStream_t s) {
  hipLaunchKernelGGL(k_frame_plan, dim3(1), dim3(256), 0, s, ch, nchunks, out_capacity, sl, out_len);
  return hipGetLastError();
}

hipError_t launch_slot_copy(const uint8_t* in, uint8_t* out_base, const Slots& sl, uint32_t m, hipStream_t s) {
  hipLaunchKernelGGL(k_slot_copy, dim3(m, 4), dim3(256), 0, s, in, out_base, sl);
  return hipGetLastError();
}

hipError_t launch_slot_verify(const Slots& sl, uint32_t m, hipStream_t s) {
  hipLaunchKernelGGL(k_slot_verify, dim3((m + 255) / 256), dim3(256), 0, s, sl, m);
  return hipGetLastError();
}

hipError_t launch_group_result(const Slots& sl, const Groups& g, hipStream_t s) {
  hipLaunchKernelGGL(k_group_result, dim3((g.n + 255) / 256), dim3(256), 0, s, sl, g);
  return hipGetLastError();
}

}  // namespace smf
