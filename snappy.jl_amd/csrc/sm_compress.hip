// sm_compress.hip -- batched 64 KiB-block snappy compression for gfx950 (MI355X).
//
//  k_compress_exact  -- "reference mode": byte-identical to Snappy.jl's compress
//                       (src/internal.jl:127-250 incl. quirks Q1/Q3, src/Snappy.jl:20-36 incl.
//                       Q2).  The greedy parse is serial, so one wave runs it per block as
//                       wave-uniform code; five blocks share a CU (the block is read from HBM,
//                       only the 32 KiB table is in LDS).  See "reference mode" below.
//
//  k_compress_fast   -- "fast mode", see sm_compress_fast.hip.
//
// The kernels that assemble compressed fragments into streams are in sm_gather.hip.
//
// Data layout in HBM: input blocks at in[in_off[b]], outputs at out[out_off[b]] (caller
// reserves max_compressed_length(len)+5 per block, i.e. fixed slots), out_len[b] = bytes.
#include <type_traits>

#include "sm_device.h"
#include "sm_internal.h"

namespace sm {


// ---- output emission (global memory, wave-uniform op) -------------------------------

__device__ inline uint32_t emit_varint(uint8_t* dst, uint32_t op, uint32_t v, uint32_t lane) {
  uint32_t nb = varint_len(v);
  if (lane < nb) dst[op + lane] = varint_byte(v, lane, nb);
  return op + nb;
}

// emit_copy! (internal.jl:306-329, single lane): the pieces of copy_piece_len, each a copy_piece
__device__ inline uint32_t put_copy(uint8_t* dst, uint32_t op, uint32_t offset, uint32_t len) {
  do {
    const uint32_t l = copy_piece_len(len);
    const TagBytes c = copy_piece(offset, l);
    dst[op] = c.byte(0);
    dst[op + 1] = c.byte(1);
    if (c.size > 2) dst[op + 2] = c.byte(2);
    op += c.size;
    len -= l;
  } while (len);
  return op;
}

// ---- reference mode ------------------------------------------------------------------
//
// The reference's greedy parse (internal.jl:127-250) is serial: the hash table carries state
// from probe to probe (:189-193), and skip and limit depend on it.  One wave runs it per block
// as wave-uniform code.  The kernel's speed is therefore how many parses run at once per CU,
// times how short each parse's dependency chain is:
//
//  * Five parses per CU.  The block is read in place from HBM through a buffer resource
//    (range-checked to exactly the block; its lines stay in L2), and the only LDS is the
//    32 KiB table of 16 K u16 positions (0 = empty = candidate 0, as the reference's 0xffff
//    fill reads, Snappy.jl:30, internal.jl:190-191).
//    Staging the block in LDS instead fits one parse per CU (2.3-2.8 GB/s measured).
//  * Batched exact probes.  After every copy the literal search probes positions p0 + D[k],
//    D[0] = 0, D[k+1] = D[k] + (skip_k >> 5), skip_0 = 32, skip_{k+1} = skip_k + (skip_k >> 5)
//    (:162-175): a fixed sequence, so 64 probes go in one step, lane j = probe k0 + j.  Probe k
//    runs only if p0 + D[k+1] <= ip_limit (:175, checked before the probe).  Its candidate is
//    the table entry as of just before it (:190).  Each lane exchanges its half-dword entry
//    with ds_mskor_rtn_b32; the lanes of one LDS instruction are serviced in ascending lane
//    order on gfx950 (tools/probe_lds.hip; the byte-parity tests pin it), so every lane gets
//    its exact sequential candidate.  The first lane whose candidate matches is the
//    reference's match; the inserts of later lanes never happened sequentially and are undone
//    exactly: for each hash, the first later lane's returned entry is the correct value.
//  * Fused verification.  A copy step compares 256 bytes at cand and ip in one round; bytes
//    [0, 4) are the reference's verification (:238), the rest find_match_length (:216).  The
//    words at ip-1 and ip for the next step's hashes (:228-231) come out of the same round's
//    registers (two readlanes), not from another load.
//  * Deferred emission.  A copy is a token (position, offset, length) written into lane
//    (copy index mod 64); every 64 copies the wave emits them together: sizes, a DPP scan for
//    the output offsets, then each lane writes its literal run (the bytes since the previous
//    copy; runs over 64 bytes by the whole wave) and its copy tags.  The bytes equal the
//    reference's in-line emission (:200, :217), which depends only on the token sequence.

constexpr uint32_t kMaxProbes = 320;  // D[k] > 65536 for k >= ~250: a search never gets further
constexpr uint32_t kProbeSteps = kMaxProbes / kWave;
constexpr uint32_t kTabBytes = 2 * kMaxHashTableSize;

// The block in HBM through a raw buffer resource over exactly [0, n): a dword load at offset o
// returns 0 when o + 4 > n (the whole dword), and unaligned dword loads are served (both
// measured on gfx950, tools/probes/buffer_range.hip).  word(pos) therefore loads at
// min(pos, n - 4) and shifts, so the bytes below n are exact and the bytes past it read 0
// (the zero slack the reference's find_match_length never compares) -- and no load touches
// memory past the block.  A position at or past n (a shift of 32 or more) gives 0 explicitly:
// such a shift is undefined in C++, and the hardware's v_lshrrev would mask it to 5 bits.
struct BlockBytes {
  __amdgpu_buffer_rsrc_t r;
  uint32_t nm4;  // n - 4 (word() is used only when n >= 15)
  __device__ uint32_t word(uint32_t pos) const {
    const uint32_t pc = min(pos, nm4), sh = pos - pc;  // sh: 0..3 below n, >= 4 at or past n
    const uint32_t w = __builtin_amdgcn_raw_buffer_load_b32(r, (int)pc, 0, 0);
    return sh < 4 ? w >> (sh << 3) : 0u;
  }
  __device__ uint32_t byte(uint32_t pos) const { return __builtin_amdgcn_raw_buffer_load_b8(r, (int)pos, 0, 0); }
};

// The block staged in LDS (one parse per CU, for single calls and small batches): the same bytes
// as BlockBytes -- exact below n, 0 at and past n (the staging zeroes 32 bytes past n, and a
// position past n is clamped to n) -- at LDS latency instead of L2/HBM latency on the parse's
// dependency chain (a lone 64 KiB fragment's parse is that chain: ~2 loads per probe step).
struct LdsBytes {
  const uint8_t* blk;
  uint32_t n;
  __device__ uint32_t word(uint32_t pos) const { return lds_ld32(blk, min(pos, n)); }
  __device__ uint32_t byte(uint32_t pos) const { return blk[min(pos, n)]; }
};
constexpr uint32_t kLdsBlockPad = 32;

// Table entry h is half (h & 1) of dword h >> 1 and holds a position, 0 when never written.
// The reference stores pos - 1 with 0xffff = empty and reads candidate (entry + 1) mod 2^16
// (Snappy.jl:30, internal.jl:190-191): the same candidates, position 0 and "empty" alike
// giving 0, without the decode on the parse's chain.  The probe's exchange and its wait are
// one asm statement with an early-clobber result, so the compiler cannot copy the result
// register before the data lands.  Returns the entry's old value (the candidate).
__device__ inline uint32_t tab_probe(uint32_t* t, uint32_t h, uint32_t p) {
  const uint32_t sh = (h & 1u) << 4;
  const uint32_t addr = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) uint32_t*)(&t[h >> 1]));
  const uint32_t mk = 0xffffu << sh, v = p << sh;
  uint32_t old;
  asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(old)
               : "v"(addr), "v"(mk), "v"(v)
               : "memory");
  return (old >> sh) & 0xffffu;
}

// wave-cooperative copy of len block bytes from s to global memory (16-byte stores in the body)
template <class B>
__device__ inline void copy_to_global(const B& S, uint8_t* __restrict__ g, uint32_t s, uint32_t len,
                                      uint32_t lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)g & 15)) & 15);
  if (head > len) head = len;
  if (lane < head) g[lane] = (uint8_t)S.byte(s + lane);
  g += head; s += head; len -= head;
  const uint32_t n16 = len >> 4;
  uint4* g16 = reinterpret_cast<uint4*>(g);
  // four 16-byte units per lane per step, all loads issued before the stores (a whole
  // incompressible block is one literal: 64 steps of one load round trip each otherwise)
  constexpr uint32_t kU = 4;
  for (uint32_t k0 = lane; k0 < n16; k0 += kU * kWave) {
    uint4 v[kU];
#pragma unroll
    for (uint32_t i = 0; i < kU; ++i) {
      const uint32_t p = s + 16 * (k0 + i * kWave);
      if (k0 + i * kWave < n16) v[i] = make_uint4(S.word(p), S.word(p + 4), S.word(p + 8), S.word(p + 12));
    }
#pragma unroll
    for (uint32_t i = 0; i < kU; ++i)
      if (k0 + i * kWave < n16) g16[k0 + i * kWave] = v[i];
  }
  const uint32_t done = n16 << 4;
  if (lane < len - done) g[done + lane] = (uint8_t)S.byte(s + done + lane);
}

// internal.jl:252-287, whole wave, with the reference's tag rule (kLiteralQ3)
template <class B>
__device__ inline uint32_t emit_literal_w(const B& S, uint8_t* dst, uint32_t op, uint32_t start,
                                          uint32_t len, uint32_t lane) {
  const TagBytes t = literal_tag(len, kLiteralQ3);
  if (lane < t.size) dst[op + lane] = t.byte(lane);
  op += t.size;
  copy_to_global(S, dst + op, start, len, lane);
  return op + len;
}

// Emission of ntok (<= 64) queued copies: lane t holds copy t (tk = position | offset << 16,
// tl = length), preceded by its literal run from the previous copy's end (`base` for t = 0).
// Returns the new output offset; base becomes the last copy's end.
template <class B>
__device__ uint32_t flush_copies(const B& S, uint8_t* __restrict__ dst, uint32_t op, uint32_t& base,
                                 uint32_t ntok, uint32_t tk, uint32_t tl, uint32_t lane) {
  const bool act = lane < ntok;
  const uint32_t pos = tk & 0xffffu, off = tk >> 16;
  const uint32_t end = pos + tl;
  const uint32_t pend = __shfl_up(end, 1, kWave);
  const uint32_t ls = lane == 0 ? base : pend;
  const uint32_t ll = act ? pos - ls : 0u;
  const TagBytes lg = literal_tag(ll, kLiteralQ3);  // (:271-284; a run is < 65536 bytes here: 3 bytes at most)
  const uint32_t lt = ll == 0 ? 0u : lg.size;
  const uint32_t ct = act ? copy_tag_bytes(off, tl) : 0u;
  const uint32_t sz = lt + ll + ct;
  const uint32_t inc = scan_dpp(sz);
  const uint32_t o = op + inc - sz;
  const uint32_t lo = o + lt;
  if (lt > 0) dst[o] = lg.byte(0);
  if (lt > 1) dst[o + 1] = lg.byte(1);
  if (lt > 2) dst[o + 2] = lg.byte(2);
  for (uint32_t i = 0;; i += 4) {  // runs up to 64 bytes: lane-private, four bytes a step
    const bool go = ll <= 64 && i < ll;
    if (!ballot(go)) break;
    if (go) {
      const uint32_t w = S.word(ls + i), r = ll - i;
      uint8_t* q = dst + lo + i;
      q[0] = (uint8_t)w;
      if (r > 1) q[1] = (uint8_t)(w >> 8);
      if (r > 2) q[2] = (uint8_t)(w >> 16);
      if (r > 3) q[3] = (uint8_t)(w >> 24);
    }
  }
  for (uint64_t lm = ballot(ll > 64); lm; lm &= lm - 1) {  // longer runs: the whole wave
    const uint32_t t = ctz64(lm);
    copy_to_global(S, dst + readlane(lo, t), readlane(ls, t), readlane(ll, t), lane);
  }
  if (act) put_copy(dst, lo + ll, off, tl);
  base = readlane(end, ntok - 1);
  return op + readlane(inc, kWave - 1);
}

// lane l of old := v (v and l wave-uniform; no builtin for v_writelane_b32 in this compiler)
__device__ inline uint32_t writelane(uint32_t v, uint32_t l, uint32_t old) {
  asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(v), "{m0}"(l));
  return old;
}

// kLds = false: the block read in place from HBM (BlockBytes), five parses per CU -- batches;
// kLds = true: the block staged in LDS (LdsBytes), one parse per CU -- at most one block per CU
// (single calls: alice29.txt's 64 KiB fragments 4.95 ms -> see DESIGN.md section 3.1).  The
// parse below is the same code for both, so the bytes are identical.
template <bool kLds>
__global__ __launch_bounds__(64) void k_compress_exact(CompressArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t stab[kTabBytes / 4];
  __shared__ __attribute__((aligned(16))) uint8_t sblk[kLds ? kBlockSize + kLdsBlockPad : 16];

  const uint32_t b = blockIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t n = a.in_len[b];
  uint8_t* dst = a.out + a.out_off[b];
  if (n > kBlockSize) {  // batch contract violated: refuse (positions are 16-bit)
    if (lane == 0) a.out_len[b] = kNotABlock;
    return;
  }
  std::conditional_t<kLds, LdsBytes, BlockBytes> S;
  if constexpr (kLds) {
    const uint8_t* src = a.in + a.in_off[b];
    wave_load_global_to_lds(sblk, src, n, lane);
    for (uint32_t k = n + lane; k < n + kLdsBlockPad; k += kWave) sblk[k] = 0;  // zeros past the block
    S.blk = sblk;
    S.n = n;
  } else {
    S.r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.in + a.in_off[b]), (short)0, (int)n, 0x00020000);
    S.nm4 = n - 4;
  }
  const uint32_t tsize = a.table_size ? a.table_size : hashtable_size(n);      // Snappy.jl:27 (Q2)
  const uint32_t shift = 32 - (31 - __builtin_clz(tsize));                     // internal.jl:128
  for (uint32_t k = lane; k < tsize / 2; k += kWave) stab[k] = 0;              // Snappy.jl:30
  // probe offsets D[64 i + lane] and D[64 i + lane + 1] (:170-172), in registers
  uint32_t Dk[kProbeSteps] = {}, Dn[kProbeSteps] = {};
  {
    uint32_t d = 0, skip = 32;
#pragma unroll
    for (uint32_t i = 0; i < kProbeSteps; ++i) {
      for (uint32_t l = 0; l < kWave; ++l) {
        Dk[i] = writelane(d, l, Dk[i]);
        if (l) Dn[i] = writelane(d, l - 1, Dn[i]);
        else if (i) Dn[i - 1] = writelane(d, kWave - 1, Dn[i - 1]);
        const uint32_t step = skip >> 5;
        skip += step;
        d = min(d + step, 0x20000u);
      }
    }
    Dn[kProbeSteps - 1] = writelane(d, kWave - 1, Dn[kProbeSteps - 1]);
  }
  __syncthreads();

  uint32_t op = a.header ? emit_varint(dst, 0, n, lane) : 0;                   // Snappy.jl:26
  if (n == 0) {
    if (lane == 0) a.out_len[b] = op;
    return;
  }
  const uint32_t e = n - 1;                  // inclusive end (ip_end)
  const int32_t ip_limit = (int32_t)n - 16;  // internal.jl:131, Q1: 1-based ip_end-15
  uint32_t ip = 0, next_emit = 0, base = 0, ntok = 0, tk = 0, tl = 0;

  if (n >= kInputMarginBytes) {                                                // internal.jl:133
    for (;;) {
      ip += 1;                                                                 // :163
      // literal search, 64 probes per step (:167-194)
      const uint32_t p0 = ip;
      // the step that ends the search: its lanes' position, hash, old entry and validity
      uint32_t p = 0, h = 0, raw = 0;
      bool valid = false;
      uint64_t hm = 0;
#pragma unroll
      for (uint32_t i = 0; i < kProbeSteps; ++i) {
        p = p0 + Dk[i];
        valid = (int32_t)(p0 + Dn[i]) <= ip_limit;                             // :175
        const uint32_t cur = S.word(p);
        h = hash32(cur, shift);
        raw = 0;
        if (__builtin_expect(valid, 1)) raw = tab_probe(stab, h, p);                                // :190 (raw = candidate)
        // (raw < p: a candidate is an earlier position.  The ascending lane order makes that so on
        // gfx950; the compare makes a different order a missed match, never a wrapped offset)
        hm = ballot(valid && raw < p && S.word(raw) == cur);                   // :193
        if (hm || ballot(valid) != ~0ull) break;                               // a match, or :175
      }
      const bool found = hm != 0;
      uint32_t cand = 0;
      if (__builtin_expect(found, 1)) {
        const uint32_t j = ctz64(hm);
        const uint32_t pj = readlane(p, j);
        if (valid && lane > j && raw <= pj)                                    // undo later probes
          reinterpret_cast<uint16_t*>(stab)[h] = (uint16_t)raw;
        ip = pj;
        cand = readlane(raw, j);
      }
      if (__builtin_expect(!found, 0)) break;                                  // -> remainder
      for (;;) {                                                               // :211-239
        // bytes [0, 4) of a round are the verification (:238; known equal after a probe hit),
        // the rest find_match_length (:216).  Reads past the block return 0 and are capped.
        const uint32_t avail = n - ip;
        // first mismatching byte of a lane's word, 4 if none (ffbl(0) = ~0)
        auto fbyte = [](uint32_t x) {
          uint32_t r;
          asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
          return min(r >> 3, 4u);
        };
        uint32_t A = S.word(ip + 4 * lane);
        uint32_t fb = fbyte(A ^ S.word(cand + 4 * lane));
        // lanes whose word reaches the end (4 lane + 4 >= avail) stop the round too
        const uint64_t lim0 = avail > 4 * kWave ? 0ull : ~0ull << ((avail - 1) >> 2);
        uint64_t m = ballot(fb < 4) | lim0;
        uint32_t f, rb = 0;
        if (__builtin_expect(m != 0, 1)) {
          f = min(readlane(4 * lane + fb, ctz64(m)), avail);
        } else {
          for (;;) {  // matches of 256 bytes and more
            rb += 4 * kWave;
            const uint32_t off = rb + 4 * lane;
            fb = fbyte(S.word(ip + off) ^ S.word(cand + off));
            m = ballot(fb < 4 || off + 4 >= avail);
            if (__builtin_expect(m != 0, 1)) {
              f = min(readlane(off + fb, ctz64(m)), avail);
              break;
            }
          }
        }
        // :238; cand >= ip (a later position, only if the table's insert order broke) fails as a
        // verification does: the guard the lane-order assumption lacked
        if (__builtin_expect(f < 4 || cand >= ip, 0)) break;
        // The next candidate first (:228-235, one lane: insert ip-1, read and replace the entry
        // for ip), so the bookkeeping below runs under its LDS round trip.  Past ip_limit the
        // inserts are never read: the parse ends there.
        const uint32_t ipn = ip + f;                                           // :217-220
        uint32_t wp, wc;
        if (__builtin_expect(rb == 0 && f <= 4 * kWave - 4, 1)) {  // words at ipn-1, ipn: lanes (f-1)/4, +1
          const uint32_t k = (f - 1) >> 2, r8 = ((f - 1) & 3u) << 3;
          const uint64_t w = ((uint64_t)readlane(A, k + 1) << 32) | readlane(A, k);
          wp = (uint32_t)(w >> r8);
          wc = (uint32_t)(w >> (r8 + 8));
        } else {
          wp = uniform(S.word(ipn - 1));
          wc = uniform(S.word(ipn));
        }
        // (every lane stores the same value at the same address: one lane's store, no exec mask)
        uint16_t* u = reinterpret_cast<uint16_t*>(stab);
        u[hash32(wp, shift)] = (uint16_t)(ipn - 1);
        const uint32_t h2 = hash32(wc, shift);
        const uint32_t raw = u[h2];
        u[h2] = (uint16_t)ipn;
        tk = writelane(ip | ((ip - cand) << 16), ntok, tk);
        tl = writelane(f, ntok, tl);
        ++ntok;
        ip = ipn;
        next_emit = ip;
        if (__builtin_expect(ntok == kWave, 0)) {
          op = flush_copies(S, dst, op, base, ntok, tk, tl, lane);
          ntok = 0;
        }
        if (__builtin_expect((int32_t)ip >= ip_limit, 0)) break;               // :222
        cand = readlane(raw, 0);
      }
      if (__builtin_expect((int32_t)ip >= ip_limit, 0)) break;                 // :222 -> remainder
    }
  }
  if (ntok) op = flush_copies(S, dst, op, base, ntok, tk, tl, lane);
  if (next_emit <= e) op = emit_literal_w(S, dst, op, next_emit, e - next_emit + 1, lane);  // :244-248
  if (lane == 0) a.out_len[b] = op;
}

hipError_t launch_compress(const CompressArgs& a, int mode, hipStream_t s) {
  if (a.nblk == 0) return hipSuccess;
  if (mode != 0) return launch_compress_fast(a, mode, s);
  // at most one block per CU: each parse gets a CU and reads its block from LDS; more: five
  // parses per CU reading their blocks in place (the LDS holds one staged block)
  if (a.nblk <= compress_grid())
    hipLaunchKernelGGL(k_compress_exact<true>, dim3(a.nblk), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_compress_exact<false>, dim3(a.nblk), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace sm
