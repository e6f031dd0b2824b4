// sm_dec_stream.hip -- the single-stream decode paths of sm_uncompress for gfx950 (MI355X): the
// stream index with its deep walks, the origin-pointer decode (fill, resolve, gather), the
// small-stream chain (path 4), the literal-only path (path 5) and the kernel that moves results to
// mapped host memory.  The in-order and fragment engines, which these paths fall back to, are in
// sm_decompress.hip; the window walk and the stage they share are in sm_dec_walk.h.
#include "sm_dec_walk.h"
#include "sm_internal.h"

namespace sm {

// ---- one large stream, decoded in parallel ------------------------
// Snappy.jl (src/Snappy.jl:29-33), libsnappy and this library compress 64 KiB blocks
// independently, so in their streams every output multiple of 65536 is a tag start and no copy
// reaches into an earlier block.  Finding those tags needs the tag boundaries, which the format
// does not index:
//  1. k_stream_index, one wave per 4 KiB chunk of the compressed body: the wave walks the tags
//     speculatively from the chunk's first byte (walk_window, 256 bytes per step: "lane 0's
//     path"), recording each visited position and the output before it; lanes l = 1..63 walk
//     from byte l (window-wise pointer doubling, the path's positions as stop nodes) until they
//     meet lane 0's path (tag walks resynchronise) or leave the chunk.  Each chunk then
//     knows, for entry offsets 0..63, where the walk leaves it and how much output it makes.
//  2. The host chains the true path (sm_api.hip) and locates each fragment's chunk.
//  3. k_decompress_frags, one wave per fragment: walk (window-parallel) from the chunk entry to
//     the tag at output F, then the batch engine with frag_lo = F and the output limit F + 65536.
// Anything unexpected (kErrCross, an error, a length mismatch) sends the caller to the in-order
// decode, which reproduces the reference's accept/reject exactly.

// Host tag walk (sm_api.hip host_walk) by one wave: where the tags from p leave [p, lim) and
// their output -- for chunk entries deeper than the index covers (lim - p <= kSmallChunk).  The
// bytes [p, lim + 256 + 32) are staged in stg (LDS, kDevWalkStage bytes) first; a 256-byte
// window of tags per step (walk_window, as k_origin_fill), a literal too long for a window by
// itself (its far end read from HBM).
template <uint32_t kC>  // (the chunk size: lim - p <= kC)
__device__ inline void dev_walk(const uint8_t* __restrict__ in, uint32_t N, uint64_t p, uint64_t lim, uint16_t* jt,
                                uint32_t lane, uint8_t* stg, uint64_t& exit_pos, uint64_t& produced) {
  constexpr uint32_t kStage = kC + kIdxPad;
  uint64_t o = 0;
  {  // Quick path: up to kQuickTags tags decoded one by one from a single load of the 256 bytes
     // at p's dword (zero past N, as the stage), no staging and no window walk.  A deep entry a
     // few bytes before its chunk's end, or one soon followed by a long literal, then costs one
     // round trip (most deep levels and walks of literal-heavy streams: paper-100k.pdf).
    constexpr uint32_t kQuickTags = 8;
    const uint32_t base = (uint32_t)p & ~3u;
    const uint32_t w = load_word(in, N, base + 4 * lane);
    uint64_t q = p, oq = 0;
    for (uint32_t k = 0; k < kQuickTags && q < lim; ++k) {
      const uint64_t rel = q - base;
      if (rel + 12 > 4 * kWave) break;
      const uint32_t i = (uint32_t)rel >> 2, sh = (uint32_t)rel & 3u;
      const uint32_t w0 = readlane(w, i), w1 = readlane(w, i + 1), w2 = readlane(w, i + 2);
      const uint32_t c = __builtin_amdgcn_alignbyte(w1, w0, sh) & 0xff;
      const uint32_t tr = __builtin_amdgcn_alignbyte(w2, w1, sh) << 24 | (__builtin_amdgcn_alignbyte(w1, w0, sh) >> 8);
      const Tag t = decode_tag(c, tr);
      q += t.size();
      oq += t.out_bytes();
    }
    p = q;  // (the window walk goes on from here when the quick path did not leave)
    o = oq;
  }
  const uint64_t sp = p;
  if (p < lim) {
    stage_bytes(stg, in, N, (uint32_t)sp, kStage, lane);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);  // (one wave: its LDS stores land before its loads)
  }
  auto rd8 = [&](uint64_t x) -> uint64_t {
    return x >= sp && x - sp + 8 <= kStage ? lds_ld64(stg, (uint32_t)(x - sp)) : load8z(in, N, (uint32_t)x);
  };
  while (p < lim) {
    const uint32_t rlim = (uint32_t)min((uint64_t)256, lim - p);
    uint32_t cpos, csz, sizes;
    const uint32_t ntok = walk_window(rd8(p + 4 * lane), rlim, jt, lane, cpos, csz, sizes);
    if (ntok == 0) {  // a literal too long for a window walk (or a wrapped length)
      const uint64_t hv = rd8(p);
      const Tag t = decode_tag(uniform((uint32_t)hv & 0xff), uniform((uint32_t)(hv >> 8)));
      p += t.size();
      o += t.out_bytes();
      continue;
    }
    const bool mine = lane < ntok;
    const uint32_t c = (uint32_t)rd8(p + (mine ? cpos : 0u)) & 0xff;
    const uint32_t ob = !mine ? 0u : window_out_bytes(c, csz);
    const uint32_t incl = scan_dpp(ob);
    o += readlane(incl, ntok - 1);
    p += readlane(cpos + csz, ntok - 1);
  }
  exit_pos = p;
  produced = o;
}

// kDeep (path 4): also deep[kDeepLevels (kDeepChains c + ch)] = (x, exit, output, 1) for entering
// the chunk where this one's entry walks leave it, x, when x lies kIdxEntries or more bytes into
// it (a long literal across the boundary): the entry the device chain needs there whenever its
// walk passed through this chunk from one of the entries (chain 0: lane 0's exit, chains 1..:
// other distinct entry exits).  Level k + 1 likewise enters where level k's walk leaves
// (consecutive long literals: the chunks between start inside a literal, and their own lane-0
// paths need not be the stream's).  .w = 0: no such level.
// kDeep: one wave per deep-record chain (kDeepChains waves): wave 0 indexes the chunk, then each
// wave walks its chain's levels (serial dev_walks) at the same time as the others.
constexpr uint32_t index_threads(bool deep) { return deep ? kDeepChains * kWave : kWave; }
// copy_to (path 4 from a host call, else null): `in` is the call's input in device-mapped pinned
// host memory, and chunk c's bytes (chunk 0: also the header before ip0) go on to copy_to, the
// device copy the later kernels read -- the upload folded into the index launch.
template <uint32_t kC, bool kDeep>  // compressed bytes per chunk (kIdxChunk; path 4: kSmallChunk)
__global__ __launch_bounds__(index_threads(kDeep)) void k_stream_index(const uint8_t* __restrict__ in, uint32_t N,
                                                                          uint32_t ip0, uint2* rec, uint4* deep,
                                                                          uint8_t* __restrict__ copy_to) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kC + kIdxPad];
  __shared__ __attribute__((aligned(16))) uint16_t jt[6 * 256];  // walk tables, then the entry walk's 3 KiB
  __shared__ uint32_t bm[kC / 32];  // positions on lane 0's path
  __shared__ uint32_t cum[kC];      // output before each such position
  constexpr uint32_t kXw = kDeep ? kDeepChains - 1 : 1;  // waves 1.. : their own walk stage and tables
  __shared__ __attribute__((aligned(16))) uint8_t xstg[kXw][kC + kIdxPad + 16];
  __shared__ __attribute__((aligned(16))) uint16_t xjt[kXw][kJt];
  __shared__ uint64_t xs[kDeepChains];  // each chain's first entry (~0: none)
  const uint32_t c = blockIdx.x, lane = lane_id(), wv = threadIdx.x / kWave;
  const uint32_t s = ip0 + c * kC;
  if (copy_to) {
    const uint32_t a = c == 0 ? 0u : s, e = min(s + kC, N);
    for (uint32_t k = a + threadIdx.x; k < e; k += blockDim.x) copy_to[k] = in[k];
  }
  if (wv == 0) {  // (one wave from here to the chain starts: LDS in order, signal fences only)
    stage_bytes(buf, in, N, s, kC + kIdxPad, lane);
    for (uint32_t k = lane; k < kC / 32; k += kWave) bm[k] = 0;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const uint64_t lim = min((uint64_t)s + kC, (uint64_t)N - 1);  // tags start below N-1 (:416)
    // lane 0's path: the tag walk from the chunk's first byte, a 256-byte window at a time
    uint64_t p = s, acc = 0;
    while (p < lim) {
      const uint32_t rel0 = (uint32_t)(p - s);
      uint32_t rel, next, ob, excl;
      const uint32_t ntok = window_tags(buf, rel0, (uint32_t)min(lim - p, (uint64_t)256), jt, lane, rel, next, ob, excl);
      if (ntok == 0) {  // long literal
        if (lane == 0) {
          bm[rel0 >> 5] |= 1u << (rel0 & 31);
          cum[rel0] = (uint32_t)acc;
        }
        const Tag t = tag_at(buf, rel0);
        acc += t.out_bytes();
        p += t.size();
        continue;
      }
      if (lane < ntok) {
        atomicOr(&bm[rel >> 5], 1u << (rel & 31));
        cum[rel] = (uint32_t)acc + excl;
      }
      acc += readlane(excl + ob, ntok - 1);
      p = s + readlane(next, ntok - 1);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const uint64_t exit0 = p;
    const uint32_t tot0 = (uint32_t)acc;
    // Lanes 1..63 (entries at chunk bytes 1..63) walk until they meet lane 0's path or leave the
    // chunk, a 256-byte window at a time, by pointer doubling with lane 0's path as stop nodes:
    // J0[x] = x + size(x), O0[x] = its output bytes; a path position, a long literal or a
    // position at/after the limit is a fixed point (O = 0).  Seven doublings give 128 steps --
    // more tags than 256 bytes hold -- so J7[x] is where the walk from x meets the path, stops or
    // leaves the window, and O7[x] the output on the way.  Long literals take a scalar step.
    const uint64_t rl = lim > s ? lim - s : 0;  // chunk-relative parse limit
    uint64_t x = lane, ex = exit0;
    uint32_t pre = 0, res = tot0;
    bool done = lane == 0;
    uint16_t* tj = jt;                                   // 2 x 256 u16
    uint32_t* to = reinterpret_cast<uint32_t*>(jt + 512);  // 2 x 256 u32 (jt holds 3 KiB here)
    while (true) {
      bool again = true;
      while (ballot(again)) {  // settle: out of the chunk, on the path, or a long literal
        again = false;
        if (!done) {
          if (x >= rl) {
            ex = s + x;
            res = pre;
            done = true;
          } else if ((bm[x >> 5] >> (x & 31)) & 1u) {  // met lane 0's path
            res = pre + (tot0 - cum[x]);
            done = true;
          } else {
            const Tag t = tag_at(buf, (uint32_t)x);
            if (walk_stop_literal(buf[x], t.out_bytes())) {
              pre += t.out_bytes();
              x += t.size();
              again = true;
            }
          }
        }
      }
      if (!ballot(!done)) break;
      uint32_t base = done ? 0xffffffffu : (uint32_t)x;
  #pragma unroll
      for (int d = 1; d < 64; d <<= 1) base = min(base, (uint32_t)__shfl_xor(base, d, 64));
      const uint32_t rlim = (uint32_t)min(rl - base, (uint64_t)256);
      const uint64_t cw = lds_ld64(buf, base + 4 * lane);
      const uint32_t sizes = pack_sizes((uint32_t)cw, (uint32_t)(cw >> 32));
      uint32_t J[4], O[4];
  #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t r = 4 * lane + j, a = base + r, sz = (sizes >> (8 * j)) & 0xff, cb = (uint32_t)(cw >> (8 * j)) & 0xff;
        const bool stop = r >= rlim || ((bm[a >> 5] >> (a & 31)) & 1u) || sz == 255;  // (bm read below rlim only)
        J[j] = stop ? r : r + sz;
        O[j] = stop ? 0u : window_out_bytes(cb, sz);
      }
  #pragma unroll
      for (int k = 0; k < 8; ++k) {  // k = 7: the final tables for the lanes' read
        uint16_t* bj = tj + (k & 1) * 256;
        uint32_t* bo = to + (k & 1) * 256;
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          bj[4 * lane + j] = (uint16_t)J[j];
          bo[4 * lane + j] = O[j];
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (k == 7) break;
  #pragma unroll
        for (int j = 0; j < 4; ++j)
          if (J[j] < 256) {
            O[j] += bo[J[j]];
            J[j] = bj[J[j]];
          }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
      }
      if (!done && x < base + 256) {
        const uint32_t r = (uint32_t)x - base;
        pre += to[256 + r];
        x = base + tj[256 + r];
      }
      __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the next window's stores follow these reads
    }
    // (exit, output) pairs side by side: the host's walk over the records reads one cache line
    rec[c * kIdxEntries + lane] = make_uint2((uint32_t)min(ex, (uint64_t)0xffffffffu), res);
    if constexpr (kDeep) {
      // chain 0 starts at lane 0's exit; chains 1.. at other distinct exits of the entry lanes that
      // land kIdxEntries or more bytes into a chunk (the records there do not cover them: a walk
      // that did not meet lane 0's path, e.g. one inside a long literal).  tools/chain_model.py
      // --distinct: paper-100k.pdf's fast stream 19 chain walks with one chain, 7 with four.
      auto deep_at = [&](uint64_t v) {
        const uint64_t db = ip0 + ((v - ip0) / kC) * kC;
        return v < (uint64_t)N - 1 && v - db >= kIdxEntries;
      };
      // (only exits inside the next chunk: the entry lanes that are not on the stream's path read
      // garbage as tags and often jump far -- chains for those cost alice29.txt 10 us, and the
      // model finds the same 7 walks on paper-100k.pdf without them)
      const uint32_t ex32 = (uint32_t)min(ex, (uint64_t)0xffffffffu);
      uint64_t more = ballot(ex != exit0 && ex < (uint64_t)s + 2 * kC && deep_at(ex));
      for (uint32_t ch = 0; ch < kDeepChains; ++ch) {
        uint64_t x = ~0ull;  // (no chain: zero records)
        if (ch == 0) {
          x = exit0;
        } else if (more) {
          x = readlane(ex32, ctz64(more));
          more &= ballot(ex32 != (uint32_t)x);
        }
        if (lane == 0) xs[ch] = x;
      }
    }
  }  // (wave 0)
  if constexpr (kDeep) {
    __syncthreads();
    const uint32_t ch = wv;
    uint64_t x = xs[ch];
    uint8_t* const stg = ch == 0 ? buf : xstg[ch - 1];  // (buf: free now)
    uint16_t* const wjt = ch == 0 ? jt : xjt[ch - 1];
    auto deep_at = [&](uint64_t v) {
      const uint64_t db = ip0 + ((v - ip0) / kC) * kC;
      return v < (uint64_t)N - 1 && v - db >= kIdxEntries;
    };
    uint4* const dc = deep + (size_t)(kDeepChains * c + ch) * kDeepLevels;
    for (uint32_t k = 0; k < kDeepLevels; ++k) {
      uint4 dr = make_uint4(0, 0, 0, 0);
      if (x != ~0ull && deep_at(x)) {
        const uint64_t db = ip0 + ((x - ip0) / kC) * kC;
        uint64_t dex, dot;
        dev_walk<kC>(in, N, x, min(db + kC, (uint64_t)N - 1), wjt, lane, stg, dex, dot);
        dr = make_uint4((uint32_t)x, (uint32_t)min(dex, (uint64_t)0xffffffffu),
                        (uint32_t)min(dot, (uint64_t)0xffffffffu), 1u);
        x = dex;
      }
      if (lane == 0) dc[k] = dr;
      if (!dr.w) {
        for (uint32_t j = k + 1; j < kDeepLevels; ++j)
          if (lane == 0) dc[j] = make_uint4(0, 0, 0, 0);
        break;
      }
    }
  }
}

// ---- any large stream, decoded in parallel by origin pointers ---------
// A stream whose copies reach into earlier 64 KiB blocks (not block-structured) cannot be cut
// into independent fragments.  Its output is still a pure function of the tags: output byte x
// is a literal byte in[i] or, inside a copy with offset d, the byte at x - d.  With the tag
// path of k_stream_index (host-chained: path element e = the tags starting in [y_e, ex_e),
// whose output starts at O_e):
//  1. k_origin_fill, one wave per path element: walk the element's tags (walk_window over
//     64-B-strided global words), apply the reference's checks (src/internal.jl:499,505,518),
//     and write P[x] for every output byte: 0x80000000 | i for a literal byte in[i], x - d for
//     a copy byte;
//  2. k_origin_resolve rounds: P[x] = P[P[x]] while P[x] names a copy byte.  Every value stays
//     an earlier byte of x's copy chain (in-place updates only move along it), and round k
//     moves an unresolved pointer at least 2^k steps, so ceil(log2(size)) rounds finish;
//  3. k_origin_gather: out[x] = in[P[x] & 0x7fffffff].
// The result is the plain LZ77 meaning of the tags -- decompress_all_tags!'s output for a valid
// stream (incremental_copy_slow!, internal.jl:477-481).  Any check that fails sends the caller
// to the in-order decode, which returns the reference's exact status.


// One path element's tags by one wave (window walks, internal.jl:411-466), with the reference's
// checks; kFill: the origin pointer of every output byte into P.  Returns the element's status.
// stg (optional): the stream bytes [sb, sb + sl) staged in LDS (stage_bytes), read instead of HBM
template <bool kFill>
__device__ __attribute__((always_inline)) inline int32_t origin_walk(const uint8_t* __restrict__ in, uint32_t N,
                                                                   uint32_t size, const OriginPath pe,
                                                                   uint32_t* __restrict__ P, uint16_t* jt,
                                                                   uint32_t lane, const uint8_t* stg = nullptr,
                                                                   uint32_t sb = 0, uint32_t sl = 0) {
  auto load8z = [&](const uint8_t* __restrict__ in_, uint32_t N_, uint32_t p) -> uint64_t {
    return (stg && p >= sb && p - sb + 8 <= sl) ? lds_ld64(stg, p - sb) : sm::load8z(in_, N_, p);
  };
  uint32_t ip = pe.y, op = pe.O;
  int32_t st = kOk;
  const uint32_t end = min(pe.ex, N - 1);  // a tag on the last byte is never parsed (internal.jl:416)
  while (ip < end) {
    const uint32_t rlim = min(256u, end - ip);  // tags that start before ex
    uint32_t cpos, csz, sizes;
    const uint32_t ntok = walk_window(load8z(in, N, ip + 4 * lane), rlim, jt, lane, cpos, csz, sizes);
    if (ntok == 0) {  // a literal too long for a window walk (or a wrapped length): whole wave
      const uint64_t hv = load8z(in, N, ip);
      const Tag t = decode_tag(uniform((uint32_t)hv & 0xff), uniform((uint32_t)(hv >> 8)));
      const uint32_t litlen = t.literal_len();
      const uint64_t lsrc = (uint64_t)ip + 1 + t.taglen;
      if (t.is_copy() || check_tag(t, op, size, lsrc, N) != kOk) {  // :518 (a copy here: bad path)
        st = t.is_copy() ? (kFill ? kErrInvalid : kErrCross) : kErrLiteral;
        break;
      }
      if (kFill)
        for (uint32_t i = lane; i < litlen; i += kWave) P[op + i] = 0x80000000u | (uint32_t)(lsrc + i);
      op += litlen;
      ip = (uint32_t)(lsrc + litlen);
      continue;
    }
    const bool mine = lane < ntok;
    const uint32_t tpos = ip + (mine ? cpos : 0u);
    const Tag t = decode_tag8(load8z(in, N, tpos));
    const bool iscopy = t.is_copy();
    const uint32_t offset = t.offset();
    const uint32_t olen = mine ? t.out_bytes() : 0u;
    const uint32_t incl = scan_dpp(olen);
    const uint32_t opt = op + incl - olen;
    const uint32_t lsrc = tpos + 1 + t.taglen;
    const int32_t code = mine ? check_tag(t, opt, size, lsrc, N) : kOk;  // :499, :505, :518
    const uint64_t bm = ballot(code != kOk);
    if (bm) {  // the first failing tag in stream order decides
      st = kFill ? kErrInvalid : (int32_t)readlane((uint32_t)code, ctz64(bm));
      break;
    }
    // every output byte of the window's tags: tag t's bytes by the whole wave.  A copy's byte i
    // points at o - f + (i mod f): for i >= f its source lies inside the same copy, whose byte
    // i - f is byte (i mod f) of the period (incremental_copy!, internal.jl:491-509) -- so a run
    // (offset 1, 2, ...) adds one chain step, not one per period.
    if (kFill) {  // each lane its own tag's pointers, four a store (P[o + i] = base + i')
      const uint32_t base = iscopy ? opt - offset : 0x80000000u | lsrc;
      const uint32_t f = iscopy && offset < olen ? offset : 0xffffffffu;  // a copy overlapping itself
      uint32_t* const dst = P + opt;
      uint32_t i = 0, r = 0;  // r = i mod f
      auto nx = [&]() { r = r + 1 == f ? 0u : r + 1; };
      while (ballot(i + 4 <= olen)) {
        if (i + 4 <= olen) {
          uint4 v;
          v.x = base + r;
          nx();
          v.y = base + r;
          nx();
          v.z = base + r;
          nx();
          v.w = base + r;
          nx();
          *reinterpret_cast<uint4 __attribute__((aligned(4)))*>(dst + i) = v;
          i += 4;
        }
      }
      while (ballot(i < olen)) {
        if (i < olen) {
          dst[i] = base + r;
          nx();
          ++i;
        }
      }
    }
    op += readlane(incl, ntok - 1);
    ip += readlane(cpos + csz, ntok - 1);
  }
  if (st == kOk && ip != pe.ex && !(ip >= end && pe.ex >= end)) st = kFill ? kErrInvalid : kErrCross;  // tags tile the path
  if (st == kOk && op != pe.O + pe.out) st = kFill ? kErrInvalid : kErrCross;
  return st;
}

// kFill = false (k_path_check): the same walk without P, recording the reference's exact status
// of the element's first failing tag (src/internal.jl:499, :505, :518) -- a stream's first error
// is then the first failing element in path order, found in parallel instead of by the in-order
// decode.  kErrCross marks an element whose tags do not tile it (the caller falls back).
template <bool kFill>
__global__ __launch_bounds__(64) void k_origin_fill(const uint8_t* __restrict__ in, uint32_t N, uint32_t size,
                                                    const OriginPath* path, uint32_t* __restrict__ P,
                                                    int32_t* status) {
  __shared__ __attribute__((aligned(16))) uint16_t jt[kJt];
  const int32_t st = origin_walk<kFill>(in, N, size, path[blockIdx.x], P, jt, lane_id());
  if (lane_id() == 0) status[blockIdx.x] = st;
}

// ---- a small stream, all on the device (sm_uncompress): the index records chained by one wave
// instead of the host, the origin pointers filled per path element, resolved in a fixed number of
// launches and gathered -- one synchronisation for the whole call.  Any stream (no block
// structure assumed); anything unexpected (an error, no progress, a length mismatch) is reported
// in ctl[1] and the caller decodes the old way, which also finds the first error.
// The chain's LDS pool (u32 words): the entry records of the first chunks, compact (below), then
// the deep records of as many chunks as still fit.  Everything else is read from HBM.
constexpr uint32_t kChainThreads = 1024;  // all of them load the pool and take part in the runs
constexpr uint32_t kChainPool = 96u * 1024 / 4;
constexpr uint32_t kChainPath = 1024;  // path elements kept in LDS until the end (more: straight to HBM)
constexpr uint32_t kDeepWords = kDeepChains * kDeepLevels * 4;  // a chunk's deep records
constexpr uint32_t kRecNone = 0xffffffffu;                       // compact record: not representable
constexpr uint32_t kChainNodes = kChainThreads;  // chunks the parallel runs cover, one thread each
constexpr uint32_t kLift = 10;                   // 2^kLift >= kChainNodes: jump tables J[0..kLift)
constexpr uint32_t kMinRun = 8;                  // links ahead that make a parallel run worth two barriers
constexpr uint32_t kRunDone = 0xffffffffu;
#ifndef SM_CHAIN_DEEPLINK
#define SM_CHAIN_DEEPLINK 1  // links through chain 0's deep records (0: entry records only)
#endif
static_assert((1u << kLift) >= kChainNodes, "the jump tables must reach every node");
// k_stream_chain's static LDS, summed against the 160 KiB a workgroup may declare (ADVICE round 5:
// at kC = 1024 the kernel uses ~159 KiB, so growing kChainPool, kChainPath, kLift, kIdxPad or
// OriginPath by a little fails here, where these constants are tuned, not in the compiler)
template <uint32_t kC>
constexpr uint32_t chain_lds_bytes() {
  return 4 * kChainPool + (uint32_t)sizeof(OriginPath) * kChainPath + 2 * kLift * kChainNodes +
         (5 * 4 + 1) * kChainNodes + 4 * 5 + 2 * kJt + (kC + kIdxPad + 16) + 64 /* alignment slack */;
}
static_assert(chain_lds_bytes<1024>() <= 160u * 1024 && chain_lds_bytes<512>() <= 160u * 1024 &&
                  chain_lds_bytes<kSmallChunkTiny>() <= 160u * 1024,
              "k_stream_chain's LDS arrays exceed 160 KiB");
// an entry record (exit, output) of chunk base `base`, compact: (output << 16) | (exit - base)
__device__ inline uint32_t rec_compact(uint2 r, uint64_t base) {
  const uint64_t d = (uint64_t)r.x - base;
  return r.x >= base && d < 0xffffu && r.y <= 0xffffu ? (r.y << 16) | (uint32_t)d : kRecNone;
}

// The chain, in parallel where it can be.  Chunk c's lane-0 walk exits at E(c); entered anywhere,
// its walk usually meets lane 0's path and exits there too.  The link c -> c' holds when E(c)
// enters c' at an entry the records cover (offset < kIdxEntries) AND that entry's walk exits at
// E(c') -- then the element after the one in c' is again decided by a link.  A link may also pass
// through chain 0's deep records of c first (E(c) deep in a later chunk, consecutive long
// literals: the deep elements the serial chain would take there).  Pointer jumping over the
// links (one thread per chunk, kLift rounds) gives every chunk its distance D to the end of its
// links, the elements and the output (SS) on the way, and the jump tables J[k] (2^k links).
// When the serial chain (wave 0) stands on an entry whose walk exits at E(c1) with D(c1) >=
// kMinRun links ahead, every chunk t tests in parallel whether it lies i = D(c1) - D(t) links
// along from c1 (J0 of the node i - 1 along is t) and writes its own path element and its link's
// deep elements; wave 0 continues after the last.  Every run element is one the serial chain
// would take (same record, same exit), so the path is identical; anything else (other deep
// entries, walks) stays serial.
__device__ inline uint4 chain_deep0(const uint4* sdeep, const uint4* __restrict__ deep, uint32_t nsdeep, uint32_t c,
                                    uint32_t k) {
  const uint32_t i = kDeepLevels * kDeepChains * c + k;
  uint4 v;
  if (i < nsdeep)
    v = sdeep[i];
  else
    v = deep[i];
  return v;
}

// ctl[0] = path elements, ctl[1] = 0 (the path covers exactly `size` bytes of output) or 1 (fall back)
template <uint32_t kC>  // bytes per index chunk
__global__ __launch_bounds__(kChainThreads) void k_stream_chain(const uint8_t* __restrict__ in, uint32_t N, uint32_t ip0,
                                                                uint32_t size, uint32_t nchunks,
                                                                const uint2* __restrict__ rec,
                                                                const uint4* __restrict__ deep, OriginPath* path,
                                                                uint32_t* ctl, uint32_t nrounds) {
  __shared__ __attribute__((aligned(16))) uint32_t pool[kChainPool];
  __shared__ __attribute__((aligned(16))) OriginPath spath[kChainPath];
  __shared__ uint16_t J[kLift][kChainNodes];
  // per chunk node: D (links to the end, low 16 bits) | elements before the end's (high 16), the
  // output on the way (saturating), E, the output of the linked element, of the deep elements
  // before it, and their count
  __shared__ uint32_t Dsh[kChainNodes], SSsh[kChainNodes], Esh[kChainNodes], Wsh[kChainNodes], Wdsh[kChainNodes];
  __shared__ uint8_t Lsh[kChainNodes];
  __shared__ uint32_t run[5];  // the run wave 0 asks for: c1 (kRunDone: finished), y, O, np, output of c1's element
  __shared__ __attribute__((aligned(16))) uint16_t jt[kJt];
  __shared__ __attribute__((aligned(16))) uint8_t stg[kC + kIdxPad + 16];
  // one round trip for the whole pool: every thread's loads are in flight before its stores
  const uint32_t nrec = min(nchunks, kChainPool / kIdxEntries);                    // chunks with LDS records
  const uint32_t ndeep = min(nchunks, (kChainPool - nrec * kIdxEntries) / kDeepWords);  // ... and LDS deep records
  uint32_t* const srec = pool;
  uint4* const sdeep = reinterpret_cast<uint4*>(pool + nrec * kIdxEntries);  // (16-B aligned: nrec * 64 words)
  const uint32_t t = threadIdx.x;
  {  // (clamped indices, no branches around the loads: they all issue before the first wait)
    const uint32_t nr = nrec * kIdxEntries, nd = ndeep * kDeepWords / 4;
    for (uint32_t k0 = t; k0 < nr; k0 += 8 * kChainThreads) {
      uint2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = rec[min(k0 + u * kChainThreads, nr - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t k = k0 + u * kChainThreads;
        if (k < nr) srec[k] = rec_compact(v[u], ip0 + (uint64_t)(k / kIdxEntries) * kC);
      }
    }
    for (uint32_t k0 = t; k0 < nd; k0 += 4 * kChainThreads) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = deep[min(k0 + u * kChainThreads, nd - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) sdeep[min(k0 + u * kChainThreads, nd - 1)] = v[u];  // (past nd: the last again)
    }
  }
  __syncthreads();
  const bool par = nchunks <= kChainNodes;
  // a compact entry record from LDS, or from HBM past the pool
  auto crec = [&](uint32_t cc, uint32_t l) {
    return cc < nrec ? srec[cc * kIdxEntries + l]
                     : rec_compact(rec[cc * kIdxEntries + l], ip0 + (uint64_t)cc * kC);
  };
  // chain 0's deep record k of chunk c (LDS, or HBM past the pool)
  const uint32_t nsdeep = ndeep * kDeepChains * kDeepLevels;
#define drec0(c, k) chain_deep0(sdeep, deep, nsdeep, (c), (k))
  if (par) {  // the links and their pointer jumping (a root links to itself)
    uint32_t link = t, w = 0, wd = 0, nd = 0, e = 0xffffffffu;
    if (t < nchunks) {
      const uint32_t v0 = crec(t, 0);
      if (v0 != kRecNone) {
        e = ip0 + t * kC + (v0 & 0xffffu);
        // from E(t): through chain 0's deep records while the exits land deep in later chunks
        // (the serial chain takes exactly those: level 0 from the chains of t's chunk, level k + 1
        // as the next level of the record it came from), then a recorded entry that exits at E
        uint32_t X = e;
        for (uint32_t k = 0; k <= kDeepLevels; ++k) {
          const uint32_t xr = X - ip0, cx = xr / kC, lx = xr % kC;
          if ((uint64_t)X >= (uint64_t)N - 1 || cx >= nchunks || cx <= t) break;
          if (lx < kIdxEntries) {
            const uint32_t v2 = crec(cx, lx), v20 = crec(cx, 0);
            if (v2 != kRecNone && v20 != kRecNone && (v2 & 0xffffu) == (v20 & 0xffffu) && (v2 & 0xffffu) > lx) {
              link = cx;
              w = v2 >> 16;
            }
            break;
          }
          if (!SM_CHAIN_DEEPLINK || k == kDeepLevels) break;
          const uint4 dr = drec0(t, k);
          if (!(dr.w && dr.x == X && dr.y > X && dr.z <= size)) break;
          ++nd;
          wd += dr.z;  // (<= kDeepLevels * size: no wrap for size < 2^30)
          X = dr.y;
        }
        if (link == t || wd > size) {
          link = t;
          w = wd = nd = 0;
        }
      }
    }
    Esh[t] = e;
    Wsh[t] = w;
    Wdsh[t] = wd;
    Lsh[t] = (uint8_t)nd;
    J[0][t] = (uint16_t)link;
    uint32_t d = link != t ? 1u | ((1u + nd) << 16) : 0u, ss = w + wd, p = link;
    Dsh[t] = d;
    SSsh[t] = ss;
    __syncthreads();
    for (uint32_t r = 1; r <= kLift; ++r) {  // d, ss: over 2^r links; J[r] = J[r-1] o J[r-1]
      const uint32_t dp = Dsh[p], sp = SSsh[p], pn = J[r - 1][p];
      __syncthreads();
      d += dp;  // (both halves: at most kChainNodes each)
      ss = ss + sp < ss ? 0xffffffffu : ss + sp;  // (saturating: a run then ends past `size`, rejected)
      Dsh[t] = d;
      SSsh[t] = ss;
      if (r < kLift) J[r][t] = (uint16_t)pn;
      p = pn;
      __syncthreads();
    }
  }
  auto lift = [&](uint32_t x, uint32_t n) {
#pragma unroll
    for (uint32_t k = 0; k < kLift; ++k)
      if ((n >> k) & 1u) x = J[k][x];
    return x;
  };
  auto put = [&](uint32_t k, const OriginPath& pe) {
    if (k < kChainPath)
      spath[k] = pe;
    else
      path[k] = pe;
  };
  const uint32_t lane = lane_id();
  const bool w0 = t < kWave;
  uint64_t y = ip0, O = 0;
  uint32_t np = 0, bad = 0, cprev = 0xffffffffu;  // the chunk of the previous element
  uint32_t dsrc = 0xffffffffu, dlev = 0;          // the deep record the previous element came from
  while (true) {
    if (w0) {
      uint32_t c1 = kRunDone, out1 = 0;
      while (y < (uint64_t)N - 1) {  // internal.jl:416
        {  // the common step, an entry record in LDS, in a tight 32-bit loop (the general step below
           // takes everything else, and re-checks what ended this loop)
          uint32_t yr = (uint32_t)(y - ip0);
          bool stop = false;
          while (true) {
            const uint32_t c = yr / kC, l = yr % kC;
            if (l >= kIdxEntries || c >= nchunks) break;
            const uint32_t v = uniform(crec(c, l)), d = v & 0xffffu;
            if (v == kRecNone || d <= l || np >= nchunks) break;
            const uint32_t ot = v >> 16, exr = c * kC + d, Oc = (uint32_t)O;  // (O <= size here)
            if (par && (uniform(Dsh[c]) & 0xffffu) >= kMinRun && ip0 + exr == uniform(Esh[c])) {  // a run from here
              c1 = c;
              out1 = ot;
              break;
            }
            const OriginPath pe = {ip0 + yr, ip0 + exr, Oc, ot < 0xffffffffu - Oc ? ot : 0xffffffffu - Oc};
            if (lane == 0) put(np, pe);
            ++np;
            O += ot;
            cprev = c;
            dsrc = 0xffffffffu;
            yr = exr;
            if (O > size || (uint64_t)ip0 + exr >= (uint64_t)N - 1) {
              stop = true;
              break;
            }
          }
          y = ip0 + (uint64_t)yr;
          if (stop || c1 != kRunDone) break;
        }
        const uint32_t c = (uint32_t)((y - ip0) / kC);
        const uint64_t base = ip0 + (uint64_t)c * kC, l = y - base;
        uint64_t ex, ot;
        if (l < kIdxEntries) {
          const uint32_t v = c < nrec ? srec[c * kIdxEntries + l] : kRecNone;
          if (v != kRecNone) {
            ex = base + (v & 0xffffu);
            ot = v >> 16;
          } else {
            const uint2 r = rec[c * kIdxEntries + l];
            ex = uniform(r.x);
            ot = uniform(r.y);
          }
          dsrc = 0xffffffffu;
        } else {
          // candidates, one lane each, read at once: lane 0 the next level of the deep record the
          // previous element came from, lanes 1..kDeepChains level 0 of the previous element's chunk's
          // chains (it left where one of that chunk's entry walks does); the first that starts at y
          // wins, else a walk
          uint32_t idx = 0xffffffffu;
          if (lane == 0 && dsrc != 0xffffffffu && dlev + 1 < kDeepLevels) idx = kDeepLevels * dsrc + dlev + 1;
          if (lane >= 1 && lane <= kDeepChains && cprev != 0xffffffffu) idx = kDeepLevels * (kDeepChains * cprev + lane - 1);
          uint4 dr = make_uint4(0, 0, 0, 0);
          if (idx != 0xffffffffu) dr = idx < ndeep * kDeepChains * kDeepLevels ? sdeep[idx] : deep[idx];
          const uint64_t hit = ballot(dr.w && dr.x == (uint32_t)y && y <= 0xffffffffull);
          if (hit) {
            const uint32_t h = ctz64(hit);
            ex = readlane(dr.y, h);
            ot = readlane(dr.z, h);
            const uint32_t i = readlane(idx, h);
            dsrc = i / kDeepLevels;
            dlev = i % kDeepLevels;
          } else {
            dev_walk<kC>(in, N, y, min(base + kC, (uint64_t)N - 1), jt, lane, stg, ex, ot);
            dsrc = 0xffffffffu;
          }
        }
        cprev = c;
        if (np >= nchunks || ex <= y) {  // (never for a well-formed index: every element leaves its chunk)
          bad = 1;
          break;
        }
        {  // (into LDS: a global store per element made every step wait for the previous one's)
          const uint32_t Oc = O < 0xffffffffull ? (uint32_t)O : 0xffffffffu;
          const uint32_t e32 = ex < 0xffffffffull ? (uint32_t)ex : 0xffffffffu;
          const uint32_t o32 = ot < (uint64_t)(0xffffffffu - Oc) ? (uint32_t)ot : 0xffffffffu - Oc;
          if (lane == 0) put(np, {(uint32_t)y, e32, Oc, o32});
        }
        ++np;
        O += ot;
        y = ex;
        if (O > size) break;
      }
      if (lane == 0) {
        run[0] = c1;
        run[1] = (uint32_t)y;
        run[2] = (uint32_t)O;  // (O <= size when c1 is set)
        run[3] = np;
        run[4] = out1;
      }
    }
    __syncthreads();
    const uint32_t c1 = run[0];
    if (c1 == kRunDone) break;
    {  // every chunk: is it i links along from c1?  Then its element is path element np + (the
       // elements between), followed by its link's deep elements.
      const uint32_t y1 = run[1], O1 = run[2], np1 = run[3], out1 = run[4];
      const uint32_t D1 = Dsh[c1] & 0xffffu, E1 = Dsh[c1] >> 16;
      if (t < nchunks && t >= c1 && (Dsh[t] & 0xffffu) <= D1) {
        const uint32_t i = D1 - (Dsh[t] & 0xffffu), et = np1 + E1 - (Dsh[t] >> 16);
        bool on = false;
        uint32_t Ot = O1, ot = out1;
        if (i == 0) {
          if (t == c1) {
            put(np1, {y1, Esh[c1], O1, out1});
            on = true;
          }
        } else {
          const uint32_t p = lift(c1, i - 1);
          if (J[0][p] == t && p != t) {
            const uint32_t np_ = Lsh[p];
            const uint32_t yt = np_ ? drec0(p, np_ - 1).y : Esh[p];
            Ot = O1 + out1 + SSsh[c1] - SSsh[p] + Wdsh[p];
            ot = Wsh[p];
            put(et, {yt, Esh[t], Ot, ot});
            on = true;
          }
        }
        if (on && J[0][t] != t) {  // (a root's deep elements are the serial chain's)
          uint32_t Ok = Ot + ot;
          for (uint32_t k = 0; k < Lsh[t]; ++k) {
            const uint4 dr = drec0(t, k);
            put(et + 1 + k, {dr.x, dr.y, Ok, dr.z});
            Ok += dr.z;
          }
        }
      }
      if (w0) {  // wave 0 goes on after the run's last element
        const uint32_t root = lift(c1, D1);
        np = np1 + E1 + 1;
        O = (uint64_t)O1 + out1 + SSsh[c1];
        y = Esh[root];
        cprev = root;
        dsrc = 0xffffffffu;
        if (O > size) {  // (the serial chain stops there too; the path is then rejected)
          y = N;
        }
      }
    }
    __syncthreads();  // (run[] is rewritten next round; the run's LDS path elements are in place)
  }
  if (!w0) return;
  if (O != size) bad = 1;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // (lane 0's LDS stores before the copy's reads; the runs': barrier)
  for (uint32_t k = lane; k < min(np, kChainPath); k += kWave) path[k] = spath[k];
  if (lane == 0) {
    ctl[0] = np;
    ctl[1] = bad;
  }
  if (lane >= 2 && lane < 4 + nrounds) ctl[lane] = 0;  // the fill's flag and the resolve counters
#undef drec0
}

// k_origin_fill for the device chain's path: elements past ctl[0] exit; a failing element sets ctl[2]
template <uint32_t kC>  // bytes per index chunk
__global__ __launch_bounds__(64) void k_origin_fill_dev(const uint8_t* __restrict__ in, uint32_t N, uint32_t size,
                                                        const OriginPath* path, uint32_t* __restrict__ P,
                                                        uint32_t* ctl) {
  __shared__ __attribute__((aligned(16))) uint16_t jt[kJt];
  __shared__ __attribute__((aligned(16))) uint8_t buf[kC + kIdxPad + 256 + 16];  // an element's tags and a window past them
  const uint32_t npath = __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t fail = __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (both in flight)
  if (blockIdx.x >= uniform(npath) || uniform(fail)) return;
  const OriginPath pe = path[blockIdx.x];
  stage_bytes(buf, in, N, pe.y, kC + kIdxPad + 256, lane_id());  // (zero past N, as load8z)
  __syncthreads();
  const int32_t st = origin_walk<true>(in, N, size, pe, P, jt, lane_id(), buf, pe.y, kC + kIdxPad + 256);
  if (st != kOk && lane_id() == 0) atomicOr(&ctl[2], 1u);
}

// Pointer jumping with up to `hops` chain steps per pointer per launch: after launch r every
// unresolved pointer has moved >= hops^(r+1) steps, so ceil(log_hops(size)) launches resolve
// all.  One pointer per thread (a pointer's hops are one dependent chain, so more threads hide
// more); a byte is written to out in the launch in which its pointer resolves (the gather folded
// in: a pointer resolved at the start of launch r > 0 was written before).  Launch r > 0 returns
// at once when launch r - 1 left nothing pending (pend[r] counts waves with unresolved pointers
// after launch r).  Launch 0's first thread publishes
// the call's verdict words (ctl[1], ctl[2]); nothing else runs when the chain or a fill failed (P
// is then not all written).  out and words may be device-mapped pinned host memory.
// (hops: kSmallHops, or up to kOneLaunchHops for a stream that small -- one launch then resolves
// every chain, whose length is at most size, without a second launch's dispatch)
__global__ __launch_bounds__(256) void k_small_resolve(const uint8_t* __restrict__ in, uint32_t* P, uint32_t size,
                                                       uint32_t* ctl, uint32_t r, uint32_t last, uint32_t hops,
                                                       uint8_t* __restrict__ out, uint32_t* words) {
  uint32_t* const pend = ctl + 4;
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x;
  // (the three control words in one round trip: later launches usually return here)
  const uint32_t f1 = __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t f2 = __hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t pprev = __hip_atomic_load(&pend[r > 0 ? r - 1 : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r == 0 && t0 == 0) {
    words[0] = f1;
    words[1] = f2;
  }
  if ((f1 | f2) != 0 || (r > 0 && pprev == 0)) return;
  uint32_t left = 0;
  for (uint32_t x = t0; x < size; x += gridDim.x * blockDim.x) {
    uint32_t v = P[x];
    if (v >> 31) {
      if (r == 0) out[x] = in[v & 0x7fffffffu];  // (r > 0: written by an earlier launch)
      continue;
    }
    // v < x: an earlier byte of the chain.  Every few hops the progress is published, so chains
    // through x jump over it (any value a thread stores or reads is a point of the same chain, so
    // stale or racing values are still correct): a run's chain then shrinks by doubling in
    // practice, while `hops` per launch bounds the work the round count assumes.
#pragma unroll 1
    for (uint32_t h = 0; h < hops && !(v >> 31); ++h) {
      v = P[v];
      if ((h & 3) == 3) P[x] = v;
    }
    P[x] = v;
    if (v >> 31)
      out[x] = in[v & 0x7fffffffu];
    else
      ++left;
  }
  const bool any_left = __builtin_amdgcn_ballot_w64(left != 0) != 0;
  if (any_left && lane_id() == 0) atomicAdd(&pend[r], 1u);
  // the last launch: a pointer still unresolved (the round count's bound broken) is reported in the
  // third verdict word (the host zeroes it before the call; every writer writes 1), so the host falls
  // back instead of returning bytes this call never wrote
  if (last && any_left && lane_id() == 0) words[2] = 1u;
}

__global__ __launch_bounds__(256) void k_origin_resolve(uint32_t* P, uint32_t size, uint32_t* pending) {
  uint32_t left = 0;
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < size; x += gridDim.x * blockDim.x) {
    const uint32_t v = P[x];
    if (!(v >> 31)) {
      const uint32_t w = P[v];  // v < x: an earlier byte of the chain
      P[x] = w;
      left += !(w >> 31);
    }
  }
  if (__builtin_amdgcn_ballot_w64(left != 0) && lane_id() == 0) atomicAdd(pending, 1u);
}

__global__ __launch_bounds__(256) void k_origin_gather(const uint8_t* __restrict__ in, const uint32_t* __restrict__ P,
                                                       uint32_t size, uint8_t* __restrict__ out) {
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < size; x += gridDim.x * blockDim.x)
    out[x] = in[P[x] & 0x7fffffffu];
}

// src[0, n) -> dst and nw control words -> words (dst / words: pinned host memory, device-mapped;
// sm_api.hip's upload_input runs it the other way, from mapped host pages into device memory),
// 16 bytes a thread; src and dst 16-byte aligned.
__global__ __launch_bounds__(256) void k_to_host(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ dst,
                                                 const uint32_t* wsrc, uint32_t nw, uint32_t* words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nw) words[t] = wsrc[t];
  const uint32_t n16 = n / 16;
  for (uint32_t i = t; i < n16; i += gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
  if (t < n - 16 * n16) dst[16 * n16 + t] = src[16 * n16 + t];
}

// path 5 (sm_uncompress): the literals of a literal-only stream to their output positions --
// copy_literal! (internal.jl:500-527) for every tag at once.  A thread takes 16 output bytes: one
// literal's bytes as five dword loads and four funnel shifts, one 16-byte store; a unit that
// straddles two literals or the end goes byte by byte.
__global__ __launch_bounds__(256) void k_literal_spans(const uint8_t* __restrict__ in, LitSpans sp,
                                                       uint8_t* __restrict__ out, uint32_t* words) {
  const uint32_t total = sp.dst[sp.n];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    words[0] = total;
    words[1] = 0;  // SM_OK
  }
  for (uint32_t x = 16 * t; x < total; x += 16 * blockDim.x * gridDim.x) {
    uint32_t s = 0;
    for (uint32_t k = 1; k < sp.n; ++k) s = sp.dst[k] <= x ? k : s;
    if (x + 16 <= sp.dst[s + 1]) {
      const uint32_t p = sp.src[s] + (x - sp.dst[s]);
      const uint32_t* w = reinterpret_cast<const uint32_t*>(in + (p & ~3u));
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
      *reinterpret_cast<uint4*>(out + x) =
          make_uint4(__builtin_amdgcn_alignbyte(w1, w0, p), __builtin_amdgcn_alignbyte(w2, w1, p),
                     __builtin_amdgcn_alignbyte(w3, w2, p), __builtin_amdgcn_alignbyte(w4, w3, p));
    } else {
      for (uint32_t y = x; y < min(x + 16, total); ++y) {
        while (s + 1 < sp.n && sp.dst[s + 1] <= y) ++s;
        out[y] = in[sp.src[s] + (y - sp.dst[s])];
      }
    }
  }
}

hipError_t launch_literal_spans(const uint8_t* in, const LitSpans& sp, uint8_t* out, uint32_t* words, hipStream_t s) {
  if (sp.n == 0 || sp.n > kLitSpans) return hipErrorInvalidValue;
  const uint32_t units = (sp.dst[sp.n] + 15) / 16;
  const uint32_t grid = min(1024u, max(1u, (units + 255) / 256));
  hipLaunchKernelGGL(k_literal_spans, dim3(grid), dim3(256), 0, s, in, sp, out, words);
  return hipGetLastError();
}

hipError_t launch_to_host(const uint8_t* src, uint32_t n, uint8_t* dst, const uint32_t* wsrc, uint32_t nw,
                          uint32_t* words, hipStream_t s) {
  if (nw > 256) return hipErrorInvalidValue;
  const uint32_t grid = min(1024u, max(1u, (n / 16 + 255) / 256));
  hipLaunchKernelGGL(k_to_host, dim3(grid), dim3(256), 0, s, src, n, dst, wsrc, nw, words);
  return hipGetLastError();
}

hipError_t launch_origin_fill(const uint8_t* in, uint32_t N, uint32_t size, const OriginPath* path, uint32_t npath,
                              uint32_t* P, int32_t* status, hipStream_t s) {
  if (npath == 0) return hipSuccess;
  hipLaunchKernelGGL(k_origin_fill<true>, dim3(npath), dim3(64), 0, s, in, N, size, path, P, status);
  return hipGetLastError();
}

hipError_t launch_path_check(const uint8_t* in, uint32_t N, uint32_t size, const OriginPath* path, uint32_t npath,
                             int32_t* status, hipStream_t s) {
  if (npath == 0) return hipSuccess;
  hipLaunchKernelGGL(k_origin_fill<false>, dim3(npath), dim3(64), 0, s, in, N, size, path, nullptr, status);
  return hipGetLastError();
}

static uint32_t origin_grid(uint32_t size) { return min(8192u, max(1u, (size + 1023) / 1024)); }

hipError_t launch_origin_resolve(uint32_t* P, uint32_t size, uint32_t* pending, hipStream_t s) {
  if (size == 0) return hipSuccess;
  hipLaunchKernelGGL(k_origin_resolve, dim3(origin_grid(size)), dim3(256), 0, s, P, size, pending);
  return hipGetLastError();
}

template <uint32_t kC>
static void launch_small_front(const uint8_t* in, const uint8_t* in_host, uint32_t N, uint32_t ip0, uint32_t size,
                               uint32_t nchunks, uint32_t* rec, OriginPath* path, uint32_t* ctl, uint32_t* P,
                               uint32_t rounds, hipStream_t s) {
  uint4* deep = reinterpret_cast<uint4*>(rec + (size_t)nchunks * kIdxEntries * 2);  // kDeepChains x kDeepLevels per chunk
  // (in_host: the index launch reads the input there and leaves its device copy at in)
  hipLaunchKernelGGL((k_stream_index<kC, true>), dim3(nchunks), dim3(index_threads(true)), 0, s, in_host ? in_host : in,
                     N, ip0, reinterpret_cast<uint2*>(rec), deep, in_host ? const_cast<uint8_t*>(in) : nullptr);
  hipLaunchKernelGGL(k_stream_chain<kC>, dim3(1), dim3(kChainThreads), 0, s, in, N, ip0, size, nchunks,
                     reinterpret_cast<const uint2*>(rec), deep, path, ctl, rounds);
  hipLaunchKernelGGL(k_origin_fill_dev<kC>, dim3(nchunks), dim3(64), 0, s, in, N, size, path, P, ctl);
}

hipError_t launch_small_decode(const uint8_t* in, const uint8_t* in_host, uint32_t N, uint32_t ip0, uint32_t size, uint32_t chunk,
                               uint32_t nchunks, uint32_t* rec, OriginPath* path, uint32_t* ctl, uint32_t* P,
                               uint32_t rounds, uint32_t hops, uint8_t* out, uint32_t* words, hipStream_t s) {
  if (nchunks == 0 || size == 0 || rounds == 0 || 4 + rounds > kWave || hops == 0 || hops > kOneLaunchHops)
    return hipErrorInvalidValue;
  if (chunk == kSmallChunk)
    launch_small_front<kSmallChunk>(in, in_host, N, ip0, size, nchunks, rec, path, ctl, P, rounds, s);
  else if (chunk == kSmallChunkFine)
    launch_small_front<kSmallChunkFine>(in, in_host, N, ip0, size, nchunks, rec, path, ctl, P, rounds, s);
  else if (chunk == kSmallChunkTiny)
    launch_small_front<kSmallChunkTiny>(in, in_host, N, ip0, size, nchunks, rec, path, ctl, P, rounds, s);
  else
    return hipErrorInvalidValue;
  // later launches usually find nothing pending and return at once: a small grid dispatches
  // faster, and strides over the pointers when some are left
  const uint32_t g1 = min(32768u, max(1u, (size + 255) / 256));
  for (uint32_t r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(k_small_resolve, dim3(r == 0 ? g1 : min(g1, 32u)), dim3(256), 0, s, in, P, size, ctl, r,
                       (uint32_t)(r + 1 == rounds), hops, out, words);
  return hipGetLastError();
}

hipError_t launch_origin_gather(const uint8_t* in, const uint32_t* P, uint32_t size, uint8_t* out, hipStream_t s) {
  if (size == 0) return hipSuccess;
  hipLaunchKernelGGL(k_origin_gather, dim3(origin_grid(size)), dim3(256), 0, s, in, P, size, out);
  return hipGetLastError();
}

hipError_t launch_stream_index(const uint8_t* in, uint32_t N, uint32_t ip0, uint32_t nchunks, uint32_t* rec,
                               hipStream_t s) {
  if (nchunks == 0) return hipSuccess;
  hipLaunchKernelGGL((k_stream_index<kIdxChunk, false>), dim3(nchunks), dim3(64), 0, s, in, N, ip0,
                     reinterpret_cast<uint2*>(rec), nullptr, nullptr);
  return hipGetLastError();
}

}  // namespace sm
