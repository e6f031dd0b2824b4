// smq_crc.h -- CRC-32 (IEEE, the page checksum of Parquet) in parallel: the segment rule and the
// table arithmetic shared by the kernel (smq_crc.hip), the table builder and the host's model of the
// kernel (smq_host.cpp, which the sanitizer driver runs).  gfx950 has no CRC or carry-less-multiply
// instruction, so a segment's CRC is table lookups in LDS made parallel by the CRC's linearity over
// GF(2), as the framing library's CRC-32C is; the polynomial, the segments and the combine are this
// library's own.  Plain functions, compiled for the host and the device alike.  Not part of the
// public ABI.
//
// Polynomials over GF(2) mod P in the reflected register's bit order: bit 31 is x^0.  A raw
// register s (no final xor) followed by k zero bytes becomes s * x^(8k) mod P.  A range of n bytes is
// cut into segments of kCrcSegment bytes, the short one FIRST: every later segment is a full one, so
// the bytes behind segment i are (nseg - 1 - i) * kCrcSegment and its register moves to the range's
// end by powers of the one constant x^(8 kCrcSegment).  Segment 0 starts from the init 0xffffffff,
// the others from 0; the range's register is the xor of the moved segment registers (the kernel adds
// each with an atomic xor: the number of segments of a call is not known on the host, so there is no
// per-segment array to size), and the CRC is that register's complement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common/smc_layout.h"

namespace smq {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcSegment = 65536;
constexpr uint32_t kCrcThreads = 256;  // lanes of a segment's CRC; lane t owns the 16-byte granules
                                       // whose distance from the last one is t mod kCrcThreads
constexpr uint32_t kCrcTabs = 20;      // tab[i], i < 16: byte i of a granule, advanced to the granule's end;
                                       // tab[16 + j]: byte j of a register, advanced by kCrcThreads granules
constexpr uint32_t kCrcPow = kCrcSegment / 16;  // xpow[g] = x^(128 g) mod P for g <= kCrcPow
constexpr uint32_t kCrcSegPow = 16;    // segpow[k] = x^(8 kCrcSegment 2^k): 2^15 segments hold 2^31 bytes

struct CrcLut {
  uint32_t tab[kCrcTabs][256];
  uint32_t xpow[kCrcPow + 1];
  uint32_t segpow[kCrcSegPow];
};

SMC_HD inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32; ++i) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1) ? kCrcPoly : 0u);
  }
  return p;
}

// the segments of an n-byte range, and segment i's place in it
SMC_HD inline uint32_t crc_segments(uint32_t n) { return n / kCrcSegment + (n % kCrcSegment ? 1 : 0); }
SMC_HD inline uint32_t crc_first_segment(uint32_t n) { return n % kCrcSegment ? n % kCrcSegment : (n ? kCrcSegment : 0); }
SMC_HD inline uint32_t crc_segment_start(uint32_t n, uint32_t i) {
  return i ? crc_first_segment(n) + (i - 1) * kCrcSegment : 0;
}
SMC_HD inline uint32_t crc_segment_len(uint32_t n, uint32_t i) { return i ? kCrcSegment : crc_first_segment(n); }

// s moved over k whole segments: s * x^(8 kCrcSegment k)
SMC_HD inline uint32_t crc_shift_segments(const CrcLut* T, uint32_t s, uint32_t k) {
  for (uint32_t b = 0; k && b < kCrcSegPow; ++b, k >>= 1)
    if (k & 1) s = gf_mul(s, T->segpow[b]);
  return s;
}

// one granule (16 bytes, little-endian dwords w[0..3]) behind register s, which is
// kCrcThreads granules old
SMC_HD inline uint32_t crc_granule(const uint32_t* tab, uint32_t s, const uint32_t* w) {
  uint32_t r = tab[16 * 256 + (s & 0xff)] ^ tab[17 * 256 + ((s >> 8) & 0xff)] ^ tab[18 * 256 + ((s >> 16) & 0xff)] ^
               tab[19 * 256 + (s >> 24)];
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t v = w[k];
    r ^= tab[(4 * k) * 256 + (v & 0xff)] ^ tab[(4 * k + 1) * 256 + ((v >> 8) & 0xff)] ^
         tab[(4 * k + 2) * 256 + ((v >> 16) & 0xff)] ^ tab[(4 * k + 3) * 256 + (v >> 24)];
  }
  return r;
}

// one byte behind register c (tab[15]: a granule's last byte is the plain byte table)
SMC_HD inline uint32_t crc_byte(const uint32_t* tab, uint32_t c, uint32_t b) {
  return tab[15 * 256 + ((c ^ b) & 0xff)] ^ (c >> 8);
}

// A segment p[0, n) is [head bytes][G aligned 16-byte granules][tail bytes], head and tail shorter
// than a granule.
struct CrcSplit {
  uint32_t head, G;
};
SMC_HD inline CrcSplit crc_split(const uint8_t* p, uint32_t n) {
  const uint32_t to_granule = (16u - (uint32_t)((uintptr_t)p & 15)) & 15u;
  const uint32_t head = n < to_granule ? n : to_granule;
  return CrcSplit{head, (n - head) / 16};
}

// Lane t's share of the granules g[0, G) (g = p + head, 16-byte aligned), t < G: those at distance
// t, t + kCrcThreads, ... from the last one, oldest first; its register then stands t granules
// before the granules' end and is moved there (xpow[t]).
SMC_HD inline uint32_t crc_lane_granules(const uint32_t* tab, const CrcLut* T, const uint8_t* g, uint32_t G, uint32_t t) {
  uint32_t idx = (G - 1 - t) % kCrcThreads;      // this lane's oldest granule
  uint32_t cnt = (G - 1 - t) / kCrcThreads + 1;  // and how many it owns
  uint32_t s = 0;
  struct Granule {
    uint32_t w[4];
  };
  const auto load = [&](uint32_t i) {
    Granule v;
    __builtin_memcpy(&v, __builtin_assume_aligned(g + 16 * (size_t)i, 16), 16);
    return v;
  };
  for (; cnt >= 4; cnt -= 4, idx += 4 * kCrcThreads) {  // (four loads in flight)
    const Granule v0 = load(idx), v1 = load(idx + kCrcThreads), v2 = load(idx + 2 * kCrcThreads), v3 = load(idx + 3 * kCrcThreads);
    s = crc_granule(tab, s, v0.w);
    s = crc_granule(tab, s, v1.w);
    s = crc_granule(tab, s, v2.w);
    s = crc_granule(tab, s, v3.w);
  }
  for (; cnt; --cnt, idx += kCrcThreads) {
    const Granule v = load(idx);
    s = crc_granule(tab, s, v.w);
  }
  return gf_mul(T->xpow[t], s);
}

// the head's share: the init runs through the head bytes and moves over the G granules
SMC_HD inline uint32_t crc_head(const uint32_t* tab, const CrcLut* T, const uint8_t* p, CrcSplit sp, uint32_t init) {
  uint32_t h = init;
  for (uint32_t i = 0; i < sp.head; ++i) h = crc_byte(tab, h, p[i]);
  return h ? gf_mul(T->xpow[sp.G], h) : 0u;
}

// the tail's bytes behind the sum c of all shares
SMC_HD inline uint32_t crc_tail(const uint32_t* tab, const uint8_t* p, uint32_t n, CrcSplit sp, uint32_t c) {
  for (uint32_t i = sp.head + 16 * sp.G; i < n; ++i) c = crc_byte(tab, c, p[i]);
  return c;
}

void build_crc_lut(CrcLut* T);  // smq_host.cpp
// the kernel's arithmetic, lane by lane, on the host (smq_host.cpp): the CRC-32 of p[0, n)
uint32_t crc32_model(const CrcLut* T, const uint8_t* p, uint32_t n);

}  // namespace smq
