// sm_dec_walk.h -- what the decoder's engines (sm_decompress.hip: batch decode, fragments,
// validate; sm_dec_stream.hip: the single-stream paths) share: zero-padded stream loads, the
// speculative tag sizes and the pointer-doubling walk over a 256-byte window, the LDS stage and its
// tag readers, and the stream header.  The rule for one tag (decode_tag), the reference's checks
// (check_tag) and the varint rule (smc::parse_varint32) are plain C++ in sm_format.h and
// common/smc_layout.h; here they only get their bytes.
#pragma once
#include "sm_device.h"

namespace sm {

typedef uint16_t __attribute__((aligned(1))) du16u;
typedef uint32_t __attribute__((aligned(1))) du32u;
typedef uint64_t __attribute__((aligned(1))) du64u;
typedef uint32_t __attribute__((ext_vector_type(4), aligned(1))) du128u;

// 16 bytes at any address: one global_load_dwordx4 / global_store_dwordx4
__device__ inline uint4 ld16u(const uint8_t* p) {
  const du128u v = *reinterpret_cast<const du128u*>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ inline void st16u(uint8_t* p, uint4 v) {
  du128u t;
  t.x = v.x, t.y = v.y, t.z = v.z, t.w = v.w;
  *reinterpret_cast<du128u*>(p) = t;
}

constexpr uint32_t kMaxBatchLit = 200;  // longer literals stop a window walk (size 255)
constexpr int kWalkLevels = 5;  // tables J0..J4 in LDS; J5 (bit 5 of a lane's chain index) = J4 o J4
constexpr int kJtRow = 256;             // a jump-table row (u8): positions 0..254, 255 = beyond the window
constexpr int kJt = kWalkLevels * kJtRow / 2;  // u16 words of a walk's jump tables (1.25 KB)
__device__ inline uint32_t load_word(const uint8_t* __restrict__ in, uint32_t N, uint32_t p) {
  if (p + 3 < N && (((uintptr_t)(in + p)) & 3) == 0) return *reinterpret_cast<const uint32_t*>(in + p);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) v |= (p + k < N ? (uint32_t)in[p + k] : 0u) << (8 * k);
  return v;
}

__device__ inline uint64_t load8z(const uint8_t* __restrict__ in, uint32_t N, uint32_t p) {
  return (uint64_t)load_word(in, N, p) | ((uint64_t)load_word(in, N, p + 4) << 32);
}

// Speculative size of a tag starting at a window position (u8; 255 = a literal the batch walk
// leaves to the general path, which decodes any tag): a copy 1 + taglen; a literal without
// length bytes (hi < 60) 1 + len; one length byte b (tag byte 0xf0) 2 + (b + 1) when that
// literal is <= kMaxBatchLit bytes, else 255; two to four length bytes (hi >= 61: longer than
// 256 bytes in a minimal encoding) always 255.  In SWAR: copy sizes by a v_perm_b32 byte
// lookup on the kind bits, short literals as hi + 2 per byte; a word holding a literal tag byte
// with length bytes (63% of the text windows: a copy's offset byte 0xf0/f4/f8/fc somewhere in
// the 256 bytes) fixes those bytes in SWAR too (no per-byte path).  tools/check_tag_sizes.c
// restates the per-byte definition and checks this form against it (tests/test_host_logic.py).
__device__ inline uint32_t pack_sizes(uint32_t cur, uint32_t nxt) {
  const uint32_t K = cur & 0x03030303u, H = (cur >> 2) & 0x3f3f3f3fu;
  const uint32_t csz = __builtin_amdgcn_perm(0u, 0x05030200u, K);       // kind 1/2/3 -> 2/3/5
  const uint32_t ml = __builtin_amdgcn_perm(0u, 0x000000ffu, K);        // 0xff per literal byte (kind 0)
  uint32_t sz = (csz & ~ml) | ((H + 0x02020202u) & ml);
  const uint32_t h60 = (H + 0x44444444u) & 0x80808080u & ml;           // 0x80: a literal with length bytes
  if (h60) {
    const uint32_t hm = h60 | (h60 - (h60 >> 7));                       // 0xff there
    const uint32_t b = __builtin_amdgcn_alignbyte(nxt, cur, 1);         // the byte after each position
    const uint32_t e = cur ^ 0xf0f0f0f0u;                               // 0 at a one-length-byte tag
    const uint32_t ne = (((e & 0x7f7f7f7fu) + 0x7f7f7f7fu) | e) & 0x80808080u;  // 0x80: not 0xf0
    const uint32_t bb = (((b >> 1) & 0x7f7f7f7fu) + 0x1c1c1c1cu) & 0x80808080u;  // 0x80: b >= 200
    const uint32_t st = ne | bb;                                        // 0x80: size 255
    const uint32_t sm = st | (st - (st >> 7));
    const uint32_t v = (b | sm) + (0x03030303u & ~sm);                  // b + 3 (<= 202) or 0xff: no carry
    sz = (sz & ~hm) | (v & hm);
  }
  return sz;
}

// the literals the batch walk stops at (size 255 above), for a scalar walk's step over them
__device__ inline bool walk_stop_literal(uint32_t c, uint64_t lit) {
  return (c & 3) == 0 && ((c >> 2) >= 61 || lit > kMaxBatchLit);
}

// Tag walk over a 255-byte window by pointer doubling (VALU + LDS, no serial loop).
// cw = the 8 stream bytes at window position 4*lane; rlim = the parse limit relative to the
// window (window end or N-1, internal.jl:416), clamped to 255.  Every lane computes the
// speculative sizes of its 4 positions (packed u8 in `sizes`, 255 = a literal too long for a
// batch).  J0[p] = p + size(p), clamped to 255 (beyond the window: position 255 is never a tag
// of this window, and its entry maps to itself, so no read is conditional); a long literal is a
// stop node (J0[p] = p).  Positions at or after rlim need no stops: a chain's positions increase,
// so the tags before rlim are a prefix of lanes and the final count drops the rest.
// J_k = J_{k-1} o J_{k-1}, k < 5, in LDS as u8 rows (positions are bytes: a read's address is the
// row base plus the value, and five rows take 1.25 KB), J5 = J4 o J4 applied as two J4 reads:
// 64 tags = chain elements 0..63.  Lane t then holds tag t directly -- J_k applied for every set
// bit k of t -- with its window position cpos and size csz; stop nodes are fixed points, so the
// tags are a prefix of lanes.  Returns their count.
__device__ inline uint32_t walk_window(uint64_t cw, uint32_t rlim, uint16_t* jt16, uint32_t lane, uint32_t& cpos,
                                       uint32_t& csz, uint32_t& sizes) {
  uint8_t* const jt = reinterpret_cast<uint8_t*>(jt16);
  rlim = min(rlim, 255u);
  sizes = pack_sizes((uint32_t)cw, (uint32_t)(cw >> 32));
  auto rd = [&](int k, uint32_t x) -> uint32_t { return jt[k * kJtRow + x]; };
  auto row = [&](int k, const uint32_t (&J)[4]) {
    *reinterpret_cast<uint32_t*>(jt + k * kJtRow + 4 * lane) = J[0] | (J[1] << 8) | (J[2] << 16) | (J[3] << 24);
  };
  uint32_t J[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p = 4 * lane + j;
    const uint32_t sz = (sizes >> (8 * j)) & 0xff;
    J[j] = sz == 255 ? p : min(p + sz, 255u);  // 255: beyond the window
  }
  row(0, J);
  // The J_k are powers of J0, so they commute: lane t applies J_k for bit k of t as soon as row k
  // is built, its read issued with the next row's reads (the chain does not wait for every row)
  uint32_t c = 0;
#pragma unroll
  for (int k = 1; k < kWalkLevels; ++k) {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const uint32_t t = rd(k - 1, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) J[j] = rd(k - 1, J[j]);
    c = ((lane >> (k - 1)) & 1u) ? t : c;
    row(k, J);
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the u8 reads below follow the row stores
  {
    const uint32_t t = rd(kWalkLevels - 1, c);
    c = ((lane >> (kWalkLevels - 1)) & 1u) ? t : c;
  }
  if (lane >= 32) {  // J5 = J4 o J4
    c = rd(kWalkLevels - 1, c);
    c = rd(kWalkLevels - 1, c);
  }
  // (the shuffle runs with every lane active: a ds_bpermute from an inactive lane reads 0)
  const uint32_t szw = __shfl(sizes, (c >> 2) & 63u, 64);
  const uint32_t sz = (szw >> (8 * (c & 3))) & 0xffu;
  cpos = c;
  csz = sz;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the next walk's stores follow these reads
  return (uint32_t)__builtin_popcountll(ballot(c < rlim && sz != 255));
}

// bytes [s, s+len) of the stream into LDS, zero past N (the reference's zero-padded lookahead)
__device__ inline void stage_bytes(uint8_t* buf, const uint8_t* __restrict__ in, uint32_t N, uint32_t s, uint32_t len,
                                   uint32_t lane) {
  // dword k = stream bytes [s+4k, s+4k+4): two aligned global dwords + v_alignbyte, all of a
  // lane's loads issued before its LDS stores (len % 256 == 0 words per lane is not assumed)
  // Branch-free, so that every load is in flight at once (loads under divergent branches get a
  // wait at each join: six serial round trips per stage).  Aligned dwords are clamped to the one
  // holding byte N - 1 (the aligned dword at in + s - mis shares in[s]'s page), and the bytes at
  // or past N are masked to zero.
  constexpr int kU = 6;
  uint32_t* dst = reinterpret_cast<uint32_t*>(buf);
  const uint32_t nw = (len + 3) / 4;
  if (N == 0) {
    for (uint32_t k = lane; k < nw; k += kWave) dst[k] = 0;
    return;
  }
  const uint32_t mis = (uint32_t)((uintptr_t)(in + s) & 3u);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in + s - mis);
  const int64_t klast = ((intptr_t)((uintptr_t)(in + N - 1) & ~(uintptr_t)3) - (intptr_t)src) / 4;  // (< 0: s >= N)
  for (uint32_t k0 = lane; k0 < nw; k0 += kU * kWave) {
    uint32_t w[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t k = k0 + u * kWave;
      w[u] = __builtin_amdgcn_alignbyte(src[min(k + 1, klast)], src[min(k, klast)], mis);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t b = (uint64_t)s + 4 * (k0 + u * kWave);  // stream offset of word k
      const uint64_t v = b < N ? (uint64_t)N - b : 0u;       // its bytes below N
      w[u] &= v >= 4 ? 0xffffffffu : (uint32_t)((1ull << (8 * v)) - 1);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (k0 + u * kWave < nw) dst[k0 + u * kWave] = w[u];
  }
}

// the stream tag at byte rel of an LDS copy (stage_bytes: zero past the input's end)
__device__ inline Tag tag_at(const uint8_t* buf, uint32_t rel) { return decode_tag8(lds_ld64(buf, rel)); }

// Tags of the staged window at chunk byte rel0 (walk_window over buf, rlim <= 256): lane t <
// ntok gets tag t's chunk position, its output bytes and the exclusive scan of them.  ntok == 0
// means a long literal (or nothing parseable) at rel0: the caller takes one scalar step.
__device__ inline uint32_t window_tags(const uint8_t* buf, uint32_t rel0, uint32_t rlim, uint16_t* jt, uint32_t lane,
                                       uint32_t& rel, uint32_t& next, uint32_t& outb, uint32_t& excl) {
  uint32_t cpos, csz, sizes;
  const uint32_t ntok = walk_window(lds_ld64(buf, rel0 + 4 * lane), rlim, jt, lane, cpos, csz, sizes);
  const bool mine = lane < ntok;
  const uint32_t c = buf[rel0 + (mine ? cpos : 0u)];
  outb = !mine ? 0u : window_out_bytes(c, csz);
  excl = scan_dpp(outb) - outb;
  rel = rel0 + cpos;
  next = rel + csz;
  return ntok;
}

// varint32 stream header (varint.jl:12-37): size and the first tag's position; kErrVarint on
// more than 5 bytes, a 5th byte >= 0x10 or a truncated header
__device__ inline int32_t parse_header(const uint8_t* in, uint32_t N, uint32_t lane, uint32_t& size, uint32_t& ip) {
  const uint32_t hb = (lane < 5 && lane < N) ? in[lane] : 0;
  return smc::parse_varint32([&](uint32_t i) { return readlane(hb, i); }, N, size, ip);
}

}  // namespace sm
