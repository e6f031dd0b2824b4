// sm_host_rules.h -- what the host side of the main library (sm_api.hip) decides from bytes it
// does not trust -- a caller's compressed stream, the device's index records, a batch's offsets
// and lengths -- and every scratch layout it hands to the kernels.  Plain C++: no HIP header, so
// the stand-alone checker (sm_host_check.cpp, make host_check) runs this very code under ASan and
// UBSan on the CPU.  The first part is the small types the kernels share (sm_internal.h includes
// this file).  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/snappy_mi355x.h"
#include "common/smc_layout.h"
#include "sm_format.h"

namespace sm {

// ---- types and constants shared with the kernels -------------------------------------------------
// One large stream decoded in parallel (sm_uncompress): an index pass over 4 KiB chunks of the
// compressed body (sm_dec_stream.hip), then one wave per 64 KiB output fragment (sm_decompress.hip).
constexpr uint32_t kIdxChunk = 4096;  // compressed bytes per index chunk
constexpr uint32_t kIdxEntries = 64;  // entry offsets 0..63 covered per chunk
// path 4 (a small stream on the device): bytes per index chunk -- kSmallChunkFine for bodies of
// mostly copies (shorter index and fill latency per chunk), kSmallChunk when literals are long or
// the body large (fewer chain elements).  small_chunk() picks.
constexpr uint32_t kSmallChunk = 1024;
constexpr uint32_t kSmallChunkFine = 512;
constexpr uint32_t kSmallChunkTiny = 128;  // small bodies of mostly copies (small_chunk)
#ifndef SM_SMALL_HOPS
#define SM_SMALL_HOPS 1024
#endif
constexpr uint32_t kSmallHops = SM_SMALL_HOPS;  // path 4: chain steps per pointer per resolve launch
constexpr uint32_t kOneLaunchHops = 256u << 10;  // path 4: outputs up to this size resolve in one launch of size hops
constexpr uint32_t kDeepLevels = 4;     // path 4: deep-entry records per chain (consecutive long literals)
constexpr uint32_t kDeepChains = 4;     // path 4: deep-record chains per chunk (distinct entry-lane exits)
struct StreamFrag {
  uint32_t y;    // a true tag start at or before the fragment's first tag (chunk entry)
  uint32_t O;    // output position of the tag at y
  uint32_t F;    // the fragment's first output position (a multiple of 65536)
  uint32_t lim;  // output limit (0xffffffff for the last fragment: parse to the end)
};
// Any large stream (copies may reach into earlier blocks): origin pointers per output byte,
// resolved by pointer jumping (sm_dec_stream.hip).  Path element = the tags starting in [y, ex),
// whose out bytes of output start at O.
struct OriginPath {
  uint32_t y, ex, O, out;
};
// sm_uncompress path 5: a stream of at most kLitSpans literal tags.  Literal s's bytes are at
// in + src[s] (any alignment) and go to out + dst[s], dst[s + 1] = dst[s] + its length, dst[n] the
// stream's length (the declared one, which the literals cover exactly).
constexpr uint32_t kLitSpans = 16;
struct LitSpans {
  uint32_t src[kLitSpans];
  uint32_t dst[kLitSpans + 1];
  uint32_t n;
};

// (from here on host code only, inline and internal to the library: no symbol of it is exported)
#pragma GCC visibility push(hidden)

// ---- which path a single stream takes (sm_uncompress) --------------------------------------------
#ifndef SM_SMALL_BODY8  // path 4 when the body is at most SM_SMALL_BODY8/8 of the output
#define SM_SMALL_BODY8 8
#endif
#ifndef SM_SMALL_MIN
#define SM_SMALL_MIN 4096
#endif
constexpr uint32_t kSmallMinOutput = SM_SMALL_MIN;  // smaller streams: the one-wave decode
constexpr uint32_t kSmallMaxChunks = (1u << 20) / kSmallChunk;  // compressed bodies up to 1 MiB
constexpr uint32_t kSmallMaxOutput = 64u << 20;    // 4 B of origin pointer per output byte
constexpr uint32_t kParallelMinOutput = 4 * 65536;  // smaller streams: one wave is as fast
constexpr size_t kPinnedInMax = 16u << 20;   // host inputs up to this size go through the pinned staging
constexpr uint32_t kPinnedOutMax = 16u << 20;      // outputs the last kernel writes into the pinned staging

// Is the stream (n bytes, header of hdr, declared size) a path-4 candidate?  A body longer than
// its output is all literals, which the in-order engine copies HBM to HBM at bandwidth: path 0 is
// faster there -- fireworks.jpeg 59 us against ~100; a body just under its output is random data
// with short copies sprinkled in, which path 0 walks in small batches of one wave: alice29.snappy's
// fast stream 573 us there, 114 us in path 4, so path 4 takes everything up to body == output
// (round 4's bound was 7/8).
inline bool small_candidate(size_t n, size_t hdr, uint32_t size) {
  return size >= kSmallMinOutput && size <= kSmallMaxOutput && n > hdr &&
         (uint64_t)(n - hdr) * 8 <= (uint64_t)size * SM_SMALL_BODY8 &&
         (n - hdr + kSmallChunk - 1) / kSmallChunk <= kSmallMaxChunks;
}
// ... a candidate for the parallel decode (paths 1, 2, 3)?  (hdr <= n: the header parsed)
inline bool parallel_candidate(size_t n, size_t hdr, uint32_t size) {
  return size >= kParallelMinOutput && n - hdr >= 2 * kIdxChunk;
}

// sm_uncompress path 5: are the stream's tags literals only?  At most kLitSpans of them (an
// incompressible input's stream has one literal per 64 KiB block), each with at most 3 length
// bytes, inside the input and the declared length, together covering both exactly.  Then the
// reference's decode (internal.jl:411-527: every tag starts before the input's last byte, and
// copy_literal!'s checks pass) is those literals' bytes in order, and Snappy.jl:50's length check
// holds.  Anything else -- a copy tag, a 4-byte length, more tags, a stream that ends early or
// late -- is not path 5, and the other paths reproduce the reference's accept/reject.  Reads the
// tag headers only (at most 4 bytes a tag); the bytes move on the device.
inline bool literal_only(const uint8_t* c, size_t n, size_t hdr, uint32_t size, LitSpans& sp) {
  size_t p = hdr;
  uint64_t o = 0;
  sp.n = 0;
  while (p < n) {
    if (sp.n == kLitSpans) return false;
    uint32_t tr = 0;  // (the length bytes: at most 3 are accepted, and they must lie inside the input)
    for (uint32_t k = 0; k < 3; ++k) tr |= (p + 1 + k < n ? (uint32_t)c[p + 1 + k] : 0u) << (8 * k);
    const Tag t = decode_tag(c[p], tr);
    if (t.is_copy()) return false;
    const size_t q = p + 1 + t.taglen;
    if (t.taglen > 3 || q > n) return false;
    const uint64_t len = t.literal_len();  // (at most 2^24: no wrap with 3 length bytes)
    if (q + len > n || o + len > size) return false;
    sp.src[sp.n] = (uint32_t)q;
    sp.dst[sp.n] = (uint32_t)o;
    ++sp.n;
    o += len;
    p = q + len;
  }
  sp.dst[sp.n] = (uint32_t)o;
  return sp.n > 0 && o == size;
}

// Host tag walk over [p, lim) of a stream (zero-padded lookahead, internal.jl:426-462): where it
// leaves the range and how much output the tags make.  Used when a chunk is entered deeper than
// the entry offsets the index kernel covers.
inline void host_walk(const uint8_t* comp, uint32_t n, uint64_t p, uint64_t lim, uint64_t* exit_pos, uint64_t* produced) {
  uint64_t o = 0;
  while (p < lim) {
    uint32_t tr = 0;
    for (uint32_t k = 0; k < 4; ++k) tr |= (p + 1 + k < n ? (uint32_t)comp[p + 1 + k] : 0u) << (8 * k);
    const Tag t = decode_tag(comp[p], tr);
    p += t.size();
    o += t.out_bytes();
  }
  *exit_pos = p;
  *produced = o;
}

// ---- the parallel decode's true path ---------------------------------------------------------------
// A path element: the chunk entry y, the output before it O, the output of its tags, where they end.
struct PathChunk {
  uint64_t y, O, out, ex;
};
enum class PathEnd {
  kExact,       // the elements' output is the declared size
  kFirstError,  // the path ends short or long: a tag fails, find the first (path_first_error)
  kFallBack,    // an element makes no progress (ex <= y): the in-order decode decides
};
// The true path of stream comp[0, n) (body from ip0, declared size) over the index records rec:
// (exit, output) u32 pairs, kIdxEntries per kIdxChunk-byte chunk of the body.
inline PathEnd true_path(const uint8_t* comp, uint32_t n, uint32_t ip0, uint32_t size, const uint32_t* rec,
                         std::vector<PathChunk>& path) {
  const uint32_t nchunks = (n - ip0 + kIdxChunk - 1) / kIdxChunk;
  path.clear();
  path.reserve(nchunks + 16);
  uint64_t y = ip0, O = 0;
  while (y < (uint64_t)n - 1) {  // internal.jl:416
    const uint64_t c = (y - ip0) / kIdxChunk, base = ip0 + c * kIdxChunk, l = y - base;
    // the walk enters a chunk a few bytes in: the head of a record a few chunks ahead
    if (c + 8 < nchunks) __builtin_prefetch(&rec[2 * (c + 8) * kIdxEntries]);
    uint64_t ex, ot;
    if (l < kIdxEntries) {
      ex = rec[2 * (c * kIdxEntries + l)];
      ot = rec[2 * (c * kIdxEntries + l) + 1];
    } else {
      host_walk(comp, n, y, std::min<uint64_t>(base + kIdxChunk, (uint64_t)n - 1), &ex, &ot);
    }
    path.push_back({y, O, ot, ex});
    O += ot;
    if (ex <= y) return PathEnd::kFallBack;
    y = ex;
    if (O > size) break;  // a tag of this element (or an earlier one) fails: find the first
  }
  return O == size ? PathEnd::kExact : PathEnd::kFirstError;
}

// the 64 KiB output fragments of an exact path: each starts its parse at the last element at or
// before its first output byte
inline std::vector<StreamFrag> path_frags(const std::vector<PathChunk>& path, uint32_t size) {
  const uint32_t nfrag = (uint32_t)(((uint64_t)size + 65535) / 65536);
  std::vector<StreamFrag> frags(nfrag);
  size_t k = 0;
  for (uint32_t f = 0; f < nfrag; ++f) {
    const uint64_t F = (uint64_t)f * 65536;
    while (k + 1 < path.size() && path[k].O + path[k].out <= F) ++k;
    frags[f] = {(uint32_t)path[k].y, (uint32_t)path[k].O, (uint32_t)F,
                f + 1 == nfrag ? 0xffffffffu : (uint32_t)(F + 65536)};
  }
  return frags;
}

// The path for the kernels.  saturate (path_first_error, any path): an element past 2^32 of output
// is past any declared size, so its O saturates (it fails its checks) and O + out stays in 32 bits.
// Without it (launch_origin_fill, an exact path): valid only with n and size below 2^31.
inline std::vector<OriginPath> origin_path(const std::vector<PathChunk>& path, bool saturate) {
  std::vector<OriginPath> op(path.size());
  for (size_t e = 0; e < path.size(); ++e) {
    const PathChunk& c = path[e];
    if (saturate) {
      const uint64_t O = std::min<uint64_t>(c.O, 0xffffffffull), out = std::min<uint64_t>(c.out, 0xffffffffull - O);
      op[e] = {(uint32_t)c.y, (uint32_t)std::min<uint64_t>(c.ex, 0xffffffffull), (uint32_t)O, (uint32_t)out};
    } else {
      op[e] = {(uint32_t)c.y, (uint32_t)c.ex, (uint32_t)c.O, (uint32_t)c.out};
    }
  }
  return op;
}

// ---- path 4's plan ---------------------------------------------------------------------------------
// Index chunk size for path 4: 512-byte chunks halve the index and fill kernels' per-chunk walk
// (both latency chains of 256-byte windows) but double the chain's elements and split more long
// literals into deep entries.  Measured single calls (fast streams, r05): html (body 0.22 of the
// output) 83 -> 70 us, alice29.txt (0.56) 82 -> 74, paper-100k.pdf (0.82, long literals) 145 ->
// 184, urls.10K (0.48, 336 KB body) 150 -> 156.  So: fine chunks for bodies up to 0.6 of the
// output and 256 KiB.
#ifndef SM_SMALL_FINE_BODY10
#define SM_SMALL_FINE_BODY10 6
#endif
#ifndef SM_SMALL_TINY_BODY
#define SM_SMALL_TINY_BODY 16384  // bodies up to this size ...
#endif
#ifndef SM_SMALL_TINY_BODY10
#define SM_SMALL_TINY_BODY10 9    // ... and at most this many tenths of the output: 128-byte chunks
#endif
// path 4's index chunk: 128 bytes for small bodies with copies (sample-tweet.json 52 -> 45 us, 4-16
// KiB of text 51-56 -> 45-48 us), 512 for bodies of mostly copies, else 1024 (literal-rich
// streams, where finer chunks lengthen the chain: paper-100k.pdf 137 -> 168 us at 512)
inline uint32_t small_chunk(uint32_t body, uint32_t size) {
  if (body <= SM_SMALL_TINY_BODY && (uint64_t)body * 10 <= (uint64_t)size * SM_SMALL_TINY_BODY10)
    return kSmallChunkTiny;
  if ((uint64_t)body * 10 > (uint64_t)size * SM_SMALL_FINE_BODY10 || body > (256u << 10)) return kSmallChunk;
  return kSmallChunkFine;
}
struct SmallPlan {
  uint32_t chunk, nchunks;
  uint32_t rounds, hops;  // resolve launches, chain steps per pointer in each
};
inline SmallPlan small_plan(uint32_t body, uint32_t size) {
  SmallPlan p{small_chunk(body, size), 0, 1, kSmallHops};  // kSmallHops^rounds >= size: every chain (at most size steps) resolves
  p.nchunks = (body + p.chunk - 1) / p.chunk;
  if (size <= kOneLaunchHops)
    p.hops = std::max(p.hops, size);  // one launch of size hops (up to 256 KiB of output: one dispatch fewer)
  else
    for (uint64_t reach = kSmallHops; reach < size; reach *= kSmallHops) ++p.rounds;
  return p;
}

// ---- host batches ----------------------------------------------------------------------------------
// Shard [b0, b1) of a host batch, rebased so the single-context call copies only the shard's
// bytes: offsets relative to the shard's lowest input / output offset.
struct Shard {
  uint32_t b0 = 0, n = 0;
  uint64_t in_base = 0, out_base = 0;
  std::vector<uint64_t> in_off, out_off;
};
inline std::vector<Shard> make_shards(int nctx, uint32_t nblk, const uint64_t* in_off, const uint64_t* out_off) {
  std::vector<Shard> sh((size_t)nctx);
  for (int i = 0; i < nctx; ++i) {
    Shard& s = sh[(size_t)i];
    s.b0 = (uint32_t)((uint64_t)nblk * (uint64_t)i / (uint64_t)nctx);
    s.n = (uint32_t)((uint64_t)nblk * (uint64_t)(i + 1) / (uint64_t)nctx) - s.b0;
    if (s.n == 0) continue;
    s.in_base = *std::min_element(in_off + s.b0, in_off + s.b0 + s.n);
    s.out_base = *std::min_element(out_off + s.b0, out_off + s.b0 + s.n);
    s.in_off.resize(s.n);
    s.out_off.resize(s.n);
    for (uint32_t k = 0; k < s.n; ++k) {
      s.in_off[k] = in_off[s.b0 + k] - s.in_base;
      s.out_off[k] = out_off[s.b0 + k] - s.out_base;
    }
  }
  return sh;
}

// The compressor's lengths as the host receives them: a length above the block's bound is an
// error mark (SM_OUT_LEN_ERROR | k: a bounded wait inside the kernel gave up; 0xffffffff: a block
// over 64 KiB, rejected before the launch here).  Checked before any length is summed, allocated
// or gathered, so a mark never becomes a copy size.
inline sm_status check_compressed_lengths(const uint32_t* out_len, const uint32_t* in_len, uint32_t nblk) {
  for (uint32_t b = 0; b < nblk; ++b)
    if (out_len[b] > max_compressed_length(in_len[b])) return out_len[b] >= SM_OUT_LEN_ERROR ? SM_ERR_DEVICE : SM_ERR_ARGUMENT;
  return SM_OK;
}

// ---- the varint header (src/varint.jl; sm_parse32 and sm_encode32 export these) ------------------
inline sm_status parse32(const uint8_t* buf, size_t len, size_t off, uint32_t* value, size_t* next) {
  uint32_t result, hv;
  const uint32_t n = (uint32_t)std::min<size_t>(off < len ? len - off : 0, 5);
  if (smc::parse_varint32([&](uint32_t i) { return (uint32_t)buf[off + i]; }, n, result, hv) != 0) return SM_ERR_VARINT;
  if (value) *value = result;
  if (next) *next = off + hv;
  return SM_OK;
}
inline size_t encode32(uint8_t* buf, uint32_t v) {
  size_t i = 0;
  while (v >= 0x80) {
    buf[i++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  buf[i++] = (uint8_t)v;
  return i;
}

// ---- scratch layouts (smc::Carve: a null base measures, so a size is carve_x(nullptr, ...).end) --
inline smc::Carve carve_at(void* base) { return smc::Carve{reinterpret_cast<uintptr_t>(base)}; }

// the host batch calls' tables in ctx->meta (decode: sm_uncompress_batch, which adds out_cap and status)
struct BatchTables {
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *out_len, *out_cap;
  int32_t* status;
  size_t end;
};
inline BatchTables carve_batch(void* base, size_t nblk, bool decode) {
  smc::Carve c = carve_at(base);
  BatchTables t{c.take<uint64_t>(nblk), c.take<uint64_t>(nblk), c.take<uint32_t>(nblk), c.take<uint32_t>(nblk)};
  t.out_cap = c.take<uint32_t>(decode ? nblk : 0);
  t.status = c.take<int32_t>(decode ? nblk : 0);
  t.end = c.p - reinterpret_cast<uintptr_t>(base);
  return t;
}

// one stream's arguments and results in ctx->meta (sm_validate_compressed_buffer, sm_uncompress)
struct SingleMeta {
  uint64_t* off;  // in_off = out_off = 0
  uint32_t *in_len, *cap;
  uint32_t* out_len;  // (out_len, status) as one pair: path 0's launch_to_host reads both from here
  int32_t* status;
  size_t end;
};
inline SingleMeta carve_single(void* base) {
  smc::Carve c = carve_at(base);
  SingleMeta m{c.take<uint64_t>(1), c.take<uint32_t>(1), c.take<uint32_t>(1), c.take<uint32_t>(2)};
  m.status = reinterpret_cast<int32_t*>(m.out_len + 1);
  m.end = c.p - reinterpret_cast<uintptr_t>(base);
  return m;
}

// sm_compress's fragment tables in ctx->meta; part_len: the split parse's part lengths, at most
// kMaxParts (nfrag * parts) of them
constexpr uint32_t kMaxParts = 256;
struct FragTables {
  uint64_t *in_off, *out_off, *dst_off;
  uint32_t *in_len, *out_len, *part_len;
  size_t end;
};
inline FragTables carve_frags(void* base, size_t nfrag) {
  smc::Carve c = carve_at(base);
  FragTables t{c.take<uint64_t>(nfrag), c.take<uint64_t>(nfrag), c.take<uint64_t>(nfrag),
               c.take<uint32_t>(nfrag), c.take<uint32_t>(nfrag), c.take<uint32_t>(kMaxParts)};
  t.end = c.p - reinterpret_cast<uintptr_t>(base);
  return t;
}

// the parallel decode in ctx->idx: the index records (2 u32 per entry), the fragment table, the
// fragments' statuses
struct ParallelScratch {
  uint32_t* rec;
  StreamFrag* frags;
  int32_t* st;
  size_t end;
};
inline size_t parallel_rec_words(size_t nchunks) { return 2 * nchunks * kIdxEntries; }
inline ParallelScratch carve_parallel(void* base, size_t nchunks, size_t nfrag) {
  smc::Carve c = carve_at(base);
  ParallelScratch t{c.take<uint32_t>(parallel_rec_words(nchunks)), c.take<StreamFrag>(nfrag), c.take<int32_t>(nfrag)};
  t.end = c.p - reinterpret_cast<uintptr_t>(base);
  return t;
}

// the origin-pointer decode in ctx->org: a pointer per output byte, the path, its elements'
// statuses, the resolve rounds' pending count.  path_first_error takes it with size 0.
struct OriginScratch {
  uint32_t* P;
  OriginPath* path;
  int32_t* st;
  uint32_t* pend;
  size_t end;
};
inline OriginScratch carve_origin(void* base, size_t size, size_t npath) {
  smc::Carve c = carve_at(base);
  OriginScratch t{c.take<uint32_t>(size), c.take<OriginPath>(npath), c.take<int32_t>(npath), c.take<uint32_t>(1)};
  t.end = c.p - reinterpret_cast<uintptr_t>(base);
  return t;
}

// path 4 in ctx->idx (launch_small_decode): the records with the deep records behind them as one
// array, the path, the control words
struct SmallScratch {
  uint32_t* rec;
  OriginPath* path;
  uint32_t* ctl;
  size_t end;
};
inline SmallScratch carve_small(void* base, size_t nchunks, size_t rounds) {
  smc::Carve c = carve_at(base);
  SmallScratch t{c.take<uint32_t>(nchunks * (2 * kIdxEntries + 4 * kDeepChains * kDeepLevels)), c.take<OriginPath>(nchunks),
                 c.take<uint32_t>(4 + rounds)};
  t.end = c.p - reinterpret_cast<uintptr_t>(base);
  return t;
}

#pragma GCC visibility pop

}  // namespace sm
