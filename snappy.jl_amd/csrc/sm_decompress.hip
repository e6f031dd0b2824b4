// sm_decompress.hip -- batched snappy decompression for gfx950 (MI355X).
//
// One wavefront per compressed stream.  Accept/reject semantics are Snappy.jl's
// (src/internal.jl:411-527, src/Snappy.jl:46-52), including its leniencies:
//   * `while ip < endof(input)` (internal.jl:416): a tag on the last byte is never parsed;
//   * the 4-byte lookahead is zero-padded past the end (internal.jl:426-430);
//   * literal length is len + trailer in UInt32 arithmetic (wraps);
//   * copy offset check `op-1 <= offset-1` with unsigned wrap (internal.jl:499);
//   * the copy-length check is skipped on the 2x8-byte fast path (internal.jl:500-505).
// The first error in stream order wins, as the reference throws at the first one.
//
// Batched tag engine (declared length <= 64 KiB -- every block the compressor produces):
//  * the compressed stream flows through a 1 KiB LDS ring (4 x 256-B slots + mirror), one
//    slot prefetched into registers a batch ahead;
//  * every lane computes, for its 4 positions of the current slot, the size a tag starting
//    there would have (packed u8, 255 = literal too long for a batch); a pointer-doubling walk
//    gives lane t the t-th tag directly;
//  * up to 64 tags per batch decode one per lane, output offsets from a wave scan; the
//    reference's length checks are settled by one uniform test per batch where that decides them
//    (a batch that ends inside the declared size and the input), else run per tag -- the lowest
//    failing lane decides the status;
//  * tags execute lane-parallel in 16-byte pieces into a linear LDS output window (sources in
//    the window or, older, in HBM), the few copies whose source overlaps the batch's own
//    output (or offset < 16) in stream order after them; whole 16-byte blocks go to HBM when
//    a batch ends;
//  * the first piece of every HBM source is loaded before the rest of the batch runs, and the next
//    batch's tag walk stands between that load and its use (it needs only where this batch ends).
// Literals longer than 64 bytes are copied by the whole wave.
// Streams declaring > 64 KiB use a simple per-tag engine (also straight into HBM).
//
// Also here, over the same window walk (sm_dec_walk.h): the fragment decode of one large stream
// (k_decompress_frags; its index and the other single-stream paths are in sm_dec_stream.hip),
// validation without output (k_validate) and the declared lengths (k_uncompressed_length).
#include "sm_dec_walk.h"
#include "sm_internal.h"

namespace sm {

constexpr uint32_t kRing = 1024;
constexpr uint32_t kRingMirror = 96;  // the ring's first bytes again past its end: a literal's
                                      // 16-byte pieces (<= 64 B) read at ring offset + 48 + 20

// ---------------------------------------------------------------------------------------
// batched tag engine

// ring slot write: stream bytes [base, base+256) (word per lane) at ring[(base & 1023)]
__device__ inline void ring_put(uint8_t* ring, uint32_t base, uint32_t word, uint32_t lane) {
  uint32_t r = base & (kRing - 1);
  reinterpret_cast<uint32_t*>(ring + r)[lane] = word;
  if (r == 0 && lane < kRingMirror / 4) reinterpret_cast<uint32_t*>(ring + kRing)[lane] = word;  // mirror
}

// 8 stream bytes at pos (aligned dword reads: the mirror covers the 12 bytes past kRing)
__device__ inline uint64_t ring_get8(const uint8_t* ring, uint32_t pos) { return lds_ld64(ring, pos & (kRing - 1)); }

// ring refill at wb: slots [wb, wb+768) and the two prefetch words, all five loads in flight
__device__ inline void ring_fill(const uint8_t* __restrict__ in, uint32_t N, uint32_t wb, uint8_t* ring, uint32_t& pre1,
                                 uint32_t& pre2, uint32_t lane) {
  uint32_t w[5];
  if ((((uintptr_t)(in + wb)) & 3) == 0 && wb + 1280 <= N) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(in + wb) + lane;
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = s[64 * i];
  } else {
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = load_word(in, N, wb + 256 * i + 4 * lane);
  }
  ring_put(ring, wb, w[0], lane);
  ring_put(ring, wb + 256, w[1], lane);
  ring_put(ring, wb + 512, w[2], lane);
  pre1 = w[3];
  pre2 = w[4];
}

// ---- LDS output window --------------------------------------------------------------------
// The recent output of the stream lives in a per-wave linear LDS window besides going to HBM:
// output position x at byte x - wbase (wbase a multiple of 16).  Every byte at or past the
// current output position op is zero when a batch starts, so tags write by or-ing whole 16-byte
// pieces (five aligned ds_or_b32, the bytes past the tag trimmed to 0) with no read-modify-write
// races between lanes.  When a batch would write past the window's end, the last kKeep+ bytes
// move to its start and the rest is zeroed (win_shift: a few 16-byte LDS ops per lane every
// couple of batches), so a copy source at distance <= op - wbase (>= kKeep right after a shift,
// growing until the next) is in LDS; older sources are read from HBM, which holds every byte
// before the window (only the last partial 16-byte block of a batch waits for the next flush,
// and it is inside the window).  No position ever wraps: reads and writes are plain offsets.
#ifndef SM_DEC_WIN
#define SM_DEC_WIN 2560
#endif
constexpr uint32_t kWin = SM_DEC_WIN;  // window bytes (a multiple of 16)
#ifndef SM_DEC_BOUT
#define SM_DEC_BOUT 512
#endif
constexpr uint32_t kBatchOut = SM_DEC_BOUT;  // most output bytes of one batch
#ifndef SM_DEC_KEEP
#define SM_DEC_KEEP 480
#endif
constexpr uint32_t kKeep = SM_DEC_KEEP;  // bytes a shift keeps (the least LDS source reach)
constexpr uint32_t kWinPad = 16;         // bytes before the window (the dword below a piece)
static_assert(kKeep + 15 + kBatchOut + 32 <= kWin && kKeep >= 80 && kWin % 16 == 0, "window bounds");
static_assert(kKeep + 15 <= 16 * kWave, "win_shift moves at most one 16-byte unit per lane");

typedef __attribute__((address_space(3))) uint32_t lds_u32;

// 16 bytes at LDS byte address a + k (k a compile-time multiple of 4): five aligned dword reads,
// four funnel shifts (v_alignbyte_b32 reads only the low 2 bits of the shift operand)
__device__ inline uint4 lds_get16(uint32_t a, uint32_t k) {
  const lds_u32* w = (const lds_u32*)(size_t)((a & ~3u) + k);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, a), __builtin_amdgcn_alignbyte(w2, w1, a),
                    __builtin_amdgcn_alignbyte(w3, w2, a), __builtin_amdgcn_alignbyte(w4, w3, a));
}

// v with the bytes from len (1..16) on cleared: two 64-bit right shifts of all-ones (amounts in
// 0..56 for len >= 1) and a select for the high half
__device__ inline uint4 trim16(uint4 v, uint32_t len) {
  uint32_t l8 = len << 3;
  asm("" : "+v"(l8));  // (else 128 - 8 len folds into a quarter-rate multiply)
  uint64_t mlo, mhi;   // (v_lshrrev_b64 of the inline constant -1: two shifts, not four)
  asm("v_lshrrev_b64 %0, %1, -1" : "=v"(mlo) : "v"(64 - min(l8, 64u)));
  asm("v_lshrrev_b64 %0, %1, -1" : "=v"(mhi) : "v"(128 - l8));
  const bool hi = len > 8;
  return make_uint4(v.x & (uint32_t)mlo, v.y & (uint32_t)(mlo >> 32), hi ? v.z & (uint32_t)mhi : 0u,
                    hi ? v.w & (uint32_t)(mhi >> 32) : 0u);
}

// or the 16 bytes v (zero past the piece) into the zeroed window at LDS byte address a + k (k a
// compile-time multiple of 4): the five dwords from (a - 1) & ~3 with t = -a, alignbyte(hi, lo,
// t) = (hi:lo) >> 8 (t & 3) -- an aligned a shifts the piece one dword up and ors a zero below
// it (the window's front pad), no selects
__device__ inline void lds_or16(uint32_t a, uint32_t k, uint4 v) {
  const uint32_t wa = ((a - 1u) & ~3u) + k, t = 0u - a;
  const uint32_t u0 = __builtin_amdgcn_alignbyte(v.x, 0u, t);
  const uint32_t u1 = __builtin_amdgcn_alignbyte(v.y, v.x, t);
  const uint32_t u2 = __builtin_amdgcn_alignbyte(v.z, v.y, t);
  const uint32_t u3 = __builtin_amdgcn_alignbyte(v.w, v.z, t);
  const uint32_t u4 = __builtin_amdgcn_alignbyte(0u, v.w, t);
  asm volatile("ds_or_b32 %0, %1\nds_or_b32 %0, %2 offset:4\nds_or_b32 %0, %3 offset:8\nds_or_b32 %0, %4 offset:12\n"
               "ds_or_b32 %0, %5 offset:16"
               : : "v"(wa), "v"(u0), "v"(u1), "v"(u2), "v"(u3), "v"(u4) : "memory");
}

// the window's first byte at output position wbase = op0 & ~15, all of it zero
__device__ inline void win_init(uint8_t* win, uint32_t lane) {
  for (uint32_t u = lane; u < kWin / 16; u += kWave) reinterpret_cast<uint4*>(win)[u] = make_uint4(0, 0, 0, 0);
}

// move the window so that it starts at nb = (op - kKeep) & ~15: bytes [nb, op) (rounded up to a
// 16-byte unit -- the bytes past op are zero) to its start, zeros after
__device__ inline void win_shift(uint8_t* win, uint32_t& wbase, uint32_t op, uint32_t lane) {
  const uint32_t nb = (op - kKeep) & ~15u;
  const uint32_t d = nb - wbase, n = (op - nb + 15) >> 4;
  uint4* w = reinterpret_cast<uint4*>(win);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (lane < n) v = w[(d >> 4) + lane];  // (every read is issued before the first write)
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  for (uint32_t u = lane; u < kWin / 16; u += kWave) w[u] = u < n ? v : make_uint4(0, 0, 0, 0);
  wbase = nb;
}

// HBM gets the window bytes of output positions [from, to): head bytes up to a 16-byte
// position boundary, 16-byte blocks, tail bytes
__device__ inline void win_flush(uint8_t* out, const uint8_t* win, uint32_t wbase, uint32_t from, uint32_t to,
                                 uint32_t lane) {
  if (to <= from) return;
  const uint32_t h = min((16u - (from & 15u)) & 15u, to - from);
  if (lane < h) out[from + lane] = win[from + lane - wbase];
  from += h;
  const uint32_t nb = (to - from) >> 4;
  for (uint32_t k = lane; k < nb; k += kWave) {
    const uint32_t x = from + 16 * k;
    st16u(out + x, *reinterpret_cast<const uint4*>(win + (x - wbase)));
  }
  from += nb << 4;
  if (lane < to - from) out[from + lane] = win[from + lane - wbase];
}

// Decodes the tags that start in [ip, ip_end) -- ip_end = N for a whole stream, whose loop
// stops at N-1 (internal.jl:416) -- into out[op0, ...).  Copy sources below frag_lo are
// refused with kErrCross: a fragment of a block-structured stream must not read output that
// other waves produce (the caller then decodes the whole stream in order instead).  Error
// checks use stream-global positions, so they are the reference's whatever the range.
// kLit: 16-byte loads per lane in flight in a long literal's bulk copy (4 in the batch kernels,
// whose VGPR budget sets their occupancy; 16 in the lone-stream kernel, where one wave's copy is
// latency-bound)
// kWhole: the whole stream from its first tag (ip_end = N, frag_lo = 0, no output limit; those
// three arguments are not read): no copy can cross a fragment and no batch is cut at a limit, so
// e_cross, every op_lim test and both kErrCross returns are not in the instantiation.
template <uint32_t kLit = 4, bool kWhole = false>
__device__ int32_t decode_stream_batch(const uint8_t* __restrict__ in, uint32_t N, uint32_t ip, uint32_t ip_end,
                                       uint32_t size, uint8_t* out, uint32_t op0, uint32_t frag_lo, uint8_t* ring,
                                       uint16_t* jt, uint8_t* win, uint32_t lane, uint32_t& op_end,
                                       uint32_t op_lim = 0xffffffffu) {
  if (kWhole) {
    ip_end = N;
    frag_lo = 0;
    op_lim = 0xffffffffu;
  }
  // ring holds stream bytes [wb, wb+768); pre1 = [wb+768, wb+1024) (loaded a batch ago),
  // pre2 = [wb+1024, wb+1280) issued at the end of the previous batch -- so a round's fence
  // (s_waitcnt vmcnt(0)) never waits for a freshly issued prefetch.
  uint32_t wb = ip & ~255u;
  uint32_t pre1, pre2;
  ring_fill(in, N, wb, ring, pre1, pre2, lane);
  bool issue_pre2 = false;
  uint32_t op = op0, flushed = op0;  // output produced / already in HBM
  const uint32_t wlo = op0 & ~15u;   // (the window never starts below the first output block)
  uint32_t wbase = wlo;              // output position of the window's first byte
  win_init(win, lane);
  const uint32_t winA = lds_addr(win), ringA = lds_addr(ring);
  const bool in_al = (((uintptr_t)in) & 3) == 0;
  // parse limit: tags start below min(N - 1, ip_end) (nothing for N = 0), a 32-bit value, so that the
  // uniform tests against it are scalar compares (a 64-bit `<` has no scalar form)
  const uint32_t Nm1 = min(N ? N - 1 : 0u, ip_end);

  // every batch consumes input (ip strictly increases): more than N batches means the wave is
  // not whole (a caller that split it) -- a status, never a hang
  uint32_t guard = N + 1;
  // streams of 2 GiB and more, and declared lengths within 64 KiB of 2^32, take every batch
  // through the full checks (no reasoning about wrap: a batch makes at most 64 * 200 bytes)
  const bool narrow = N < 0x80000000u && size <= 0xffff0000u;
  // the ring slot after the ring's three: pre1 into the ring, pre2 takes its place, and the slot
  // after that is asked for (fetch_pre2) once nothing freshly issued can be waited on
  auto ring_advance = [&]() {
    ring_put(ring, wb + 768, pre1, lane);
    pre1 = pre2;
    asm volatile("" : "+v"(pre1));  // (the move here: after the load into pre2 it would wait for that load)
    wb += 256;
    issue_pre2 = true;  // [wb+1024, wb+1280)
  };
  // (a whole slot inside the stream at a 4-aligned base: one plain load, the test uniform)
  auto fetch_pre2 = [&]() {
    pre2 = (in_al && wb + 1280 <= N) ? reinterpret_cast<const uint32_t*>(in + wb + 1024)[lane]
                                     : load_word(in, N, wb + 1024 + 4 * lane);
    issue_pre2 = false;
  };
  // The walk of the batch at ip: its tag count and, in lane t, tag t's window position and size.
  // A batch that will be followed by another batch walks that one while its own far copy sources
  // load (below), and hands the walk to the next trip: `walked` says that it is in hand.
  bool walked = false;
  uint32_t ntok = 0, cpos = 0, csz = 0, sizes = 0;
  while (ip < Nm1 && (kWhole || op < op_lim)) {
    if (__builtin_expect(--guard == 0, 0)) return kErrDevice;
    // the window [ip, ip+256) (inside the ring: ip < wb+256; a batch's literals end before
    // ip+256+200 < wb+768)
    const uint32_t wlim = ip + 256 < Nm1 ? ip + 256 : Nm1;
    if (!walked) {
      if (ip >= wb + 256) {
        if (__builtin_expect(ip < wb + 512, 1)) {
          ring_advance();  // (its load goes out after this batch's checks)
        } else {  // jumped (long literal): refill
          wb = ip & ~255u;
          ring_fill(in, N, wb, ring, pre1, pre2, lane);
          issue_pre2 = false;
        }
      }
      ntok = walk_window(ring_get8(ring, ip + 4 * lane), wlim - ip, jt, lane, cpos, csz, sizes);
    }
    walked = false;
    uint32_t tpos = 0, ipw = ip, tnext = 0;
    bool big = false;
    if (__builtin_expect(ntok != 0, 1)) {
      tpos = ip + cpos;
      tnext = cpos + csz;
      ipw = ip + readlane(tnext, ntok - 1);
    }
    if (ipw < wlim) {
      const uint32_t rel = ipw - ip;
      big = ((readlane(sizes, rel >> 2) >> ((rel & 3) * 8)) & 0xff) == 255;
    }

    if (__builtin_expect(ntok != 0, 1)) {
      const bool mine = lane < ntok;
      // one tag per lane: its fields and its output offset (wave scan).  A tag the walk hands to a
      // lane has size != 255, so it is a copy (<= 64 B) or a literal of <= kMaxBatchLit bytes
      // (tools/check_tag_lengths.c proves it for every (tag byte, next byte)): no length saturates,
      // and a batch makes at most 64 * kMaxBatchLit bytes.
      const uint64_t hv = ring_get8(ring, mine ? tpos : wb);
      const uint32_t c = (uint32_t)hv & 0xff;
      // The walk's size of the tag already fixes what char_entry's select tree would work out
      // again (the same check proves both): a copy has csz - 1 trailer bytes, and a batch literal,
      // whose tag has a length byte only as 0xf0, makes csz - 1 - (that byte) bytes -- its trailer
      // is not needed.  What is left of the table entry (a 512-byte table in global memory
      // instead: 1.510 against 1.455 ms) is a copy's length and the high offset bits of kind 1.
      const uint32_t kind = c & 3, hi = c >> 2;
      const bool iscopy = kind != 0, k1 = kind == 1;
      const uint32_t len = k1 ? 4 + (hi & 7) : hi + 1;     // (a copy's; a literal lane's is not read)
      const uint32_t offhi = k1 ? (c << 3) & 0x700u : 0u;
      const uint32_t tl = (c + 16) >> 8;                   // a batch literal's length bytes: 1 for 0xf0
      const uint32_t tr_raw = (uint32_t)(hv >> 8);
      // the low taglen bytes (0..4) of tr_raw: the low dword of ~0 << 8 taglen (64-bit: 0 for 4)
      // clears them in a mask, one v_bfi_b32 keeps them
      uint64_t hm;
      asm("v_lshlrev_b64 %0, %1, -1" : "=v"(hm) : "v"(8 * csz - 8));
      const uint32_t offset = offhi + (tr_raw & ~(uint32_t)hm);  // (a copy's)
      const uint32_t litlen = csz - 1 - tl;
      const uint32_t olen = mine ? (iscopy ? len : litlen) : 0u;
      const uint32_t incl = scan_dpp(olen);
      const uint32_t opt = op + incl - olen;
      const uint32_t lsrc = tpos + 1 + tl;                       // (a literal's)
      const uint64_t minem = ntok == 64 ? ~0ull : ((1ull << ntok) - 1);
      const uint64_t copya = ballot(iscopy) & minem;  // the batch's copies, over all ntok tags

      // The reference's checks (internal.jl:499-518), once per batch where that decides them.  With
      // X_all the output of all ntok tags and in_end the position after the last of them,
      //   clean = op + X_all <= size && in_end <= N
      // settles every length check of the batch, because the checks are monotone in stream order:
      //  * e_len (:500-505) is avail_out < len: its leniency clause needs avail_out >= 16 >= len,
      //    so it cannot clear the error when avail_out < len.  For every tag opt + olen = op + incl
      //    <= op + X_all <= size, so avail_out >= len for a copy and >= litlen for a literal;
      //  * a batch literal's lsrc + litlen is the next tag's position (its size is 1 + taglen +
      //    litlen), which is at most in_end <= N: avail_in >= litlen.
      // What is left per tag is the offset check (:499) as the 32-bit unsigned compare it is (both
      // sides are zero-extended 32-bit values; offset 0 wraps to 0xffffffff and fails, as there),
      // and for a fragment e_cross.  The capped batch (nt < ntok) is tested over all ntok tags, as
      // the full checks are.  A batch that is not clean, or has such a tag, takes the full per-tag
      // checks below, whose verdict alone decides: the test above only ever skips them.
      const uint32_t X_all = readlane(incl, ntok - 1);
      // (uniform 32-bit compares on the scalar unit -- as size - op they fold into a vector
      // subtract-with-borrow; op <= size holds after any checked batch, and is tested, not assumed:
      // with it and `narrow` the sum cannot wrap.  ipw is in_end here.)
      const bool clean = narrow && op <= size && op + X_all <= size && ipw <= N;
      uint64_t badm = ballot(opt <= offset - 1u);
      if (!kWhole) badm |= ballot(opt - offset < frag_lo);
      if (__builtin_expect(!clean || (badm & copya) != 0, 0)) {
        // the full checks as selects, in the reference's first-failing order; the lowest failing
        // lane decides the status
        const int64_t avail_out = (int64_t)size - (int64_t)opt;
        const int64_t avail_in = (int64_t)N - (int64_t)lsrc;
        const bool e_off = (int64_t)opt <= (int64_t)(uint32_t)(offset - 1u);                                // :499
        const bool e_cross = !kWhole && opt - offset < frag_lo;
        const bool e_len = !((len <= 16) & (offset >= 8) & (avail_out >= 16)) & (avail_out < (int64_t)len);  // :505
        const bool e_lit = (avail_out < (int64_t)litlen) | (avail_in < (int64_t)litlen);                     // :518
        const int32_t ec = e_off ? kErrCopyOffset : (e_cross ? kErrCross : (e_len ? kErrCopyLength : kOk));
        const int32_t err = !mine ? kOk : (iscopy ? ec : (e_lit ? kErrLiteral : kOk));
        const uint64_t em = ballot(err != kOk);
        if (em != 0) return (int32_t)readlane((uint32_t)err, ctz64(em));
      }
      // cap the batch output at kBatchOut bytes (the window bound; one tag is <= 200 B) and at
      // the output limit (a fragment ends where the next one starts)
      uint32_t nt = ntok;
      if (__builtin_expect(X_all > kBatchOut || (!kWhole && readlane(opt, ntok - 1) >= op_lim), 0)) {
        nt = (uint32_t)__builtin_popcountll(ballot(mine && incl <= kBatchOut && (kWhole || opt < op_lim)));
        ipw = ip + readlane(tnext, nt - 1);
        big = false;  // the next tag is a batch tag inside the window
      }
      const uint32_t X = readlane(incl, nt - 1);

      if (op - wbase + X + 32 > kWin) win_shift(win, wbase, op, lane);  // (uniform)
      const uint32_t O0 = op;
      const uint32_t slo = opt - offset;
      const uint32_t shi = slo + min(len, offset);
      // a source before the window comes from HBM, which holds it whole: the window starts at
      // least kKeep bytes before the output (after a shift or a big literal) or at the first
      // output block, a source ends at most 64 bytes after its start, and every byte before the
      // batch but the last partial 16-byte block is flushed
      // (lane sets as SGPR masks: a ballot of a compare is one v_cmp, and inverse_ballot turns a
      // mask back into a lane predicate for free -- a ballot of a combined bool costs two VALU)
      const uint64_t all = nt == 64 ? ~0ull : ((1ull << nt) - 1);
      const uint64_t copym = copya & all;
      const uint64_t longm = ballot(litlen > 64) & ~copym & all;
      const uint64_t gm = ballot(slo < wbase) & copym;
      uint64_t done = longm | ~all;
      // the tags one round runs (below), and those of them whose source is in HBM
      const uint64_t rm = ~done & (~copym | (ballot(shi <= O0) & ballot(offset >= 16)));
      const uint64_t fm = gm & rm;
      const uint32_t L = iscopy ? len : litlen;
      const uint32_t da = winA + (opt - wbase);
      const uint8_t* gs = out + slo;

      // Another batch follows this one in the ring's reach: its walk needs the position after this
      // batch (fixed above, cap included) and the input ring, nothing this batch's copies make, so
      // it runs between the far loads and their use.  Not when a big literal follows, the parse or
      // the fragment ends here, or the ring must be refilled: then the loop top walks as ever.
      const bool early = !big && ipw < Nm1 && (kWhole || O0 + X < op_lim) && ipw < wb + 512;
      // The ring moves before the far loads go out, and the slot asked for with it: the wait for the
      // far pieces is then a wait for the youngest loads, and covers no fresh prefetch.  (The slot
      // given up holds bytes before wb <= ip; this batch's literals read at and after ip.)
      if (issue_pre2) fetch_pre2();
      if (early && ipw >= wb + 256) {
        ring_advance();
        fetch_pre2();
      }

      // HBM sources: this wave's earlier flushes (and big literals) must have landed
      if (gm) __threadfence_block();
      // the far lanes' first 16-byte piece, in flight over the rest of the round and the walk (two
      // or three pieces ahead cost registers -- 6 waves per SIMD -- and measured slower)
      uint4 fv = make_uint4(0, 0, 0, 0);
      if (inverse_ballot(fm)) fv = ld16u(gs);

      // long literals (65..200 B, no dependencies, inside the input ring): whole-wave passes
      uint64_t lm = longm;
      while (lm) {
        const uint32_t t = ctz64(lm);
        lm &= lm - 1;
        const uint32_t o = readlane(opt, t), sr = readlane(lsrc, t), L = readlane(litlen, t);
        const uint32_t k = 16 * lane;
        if (k < L) lds_or16(winA + (o - wbase) + k, 0, trim16(lds_get16(ringA + ((sr + k) & (kRing - 1)), 0), min(16u, L - k)));
      }

      // One round (all in LDS, or HBM for sources before the window) runs every tag whose source
      // is final before the batch and whose bytes can be read straight: a literal (<= 64 B, from
      // the input ring) or a copy with offset >= 16 -- output byte j is S[j mod offset]
      // (incremental_copy_slow!, internal.jl:477-481), which for j >= offset is the copy's own
      // output byte j - offset = out[slo + j], written by an earlier 16-byte pass.  So every tag
      // reads out[slo + j] (or its literal bytes) in 16-byte pieces.  The writes never touch
      // bytes another ready tag reads.
      // The next batch's walk, while the far pieces arrive (the ring moved above).
      if (__builtin_expect(early, 1)) {
        const uint32_t wl2 = ipw + 256 < Nm1 ? ipw + 256 : Nm1;
        ntok = walk_window(ring_get8(ring, ipw + 4 * lane), wl2 - ipw, jt, lane, cpos, csz, sizes);
        walked = true;
      }
      // The round's pieces, every lane in one pass per 16 bytes: a far lane's first piece is the one
      // loaded above, its later ones (a copy longer than 16 bytes) a load and its use each.
      if (__builtin_expect(rm != 0, 1)) {
        const bool gsrc = inverse_ballot(fm);
        const uint32_t sa = iscopy ? winA + (slo - wbase) : ringA + (lsrc & (kRing - 1));
#pragma unroll
        for (uint32_t base = 0; base < 64; base += 16) {
          const uint64_t am = rm & ballot(L > base);
          if (!am) break;
          if (inverse_ballot(am)) {
            uint4 v;
            if (gsrc) v = base == 0 ? fv : ld16u(gs + base);
            else v = lds_get16(sa, base);
            lds_or16(da, base, trim16(v, min(L - base, 16u)));
          }
        }
      }
      done |= rm;
      // The copies left -- their source overlaps earlier tags of this batch, or offset < 16 --
      // run in stream order, one tag at a time, a byte per lane: byte k = S[k mod offset] with S
      // final by then (LDS accesses of a wave are serviced in order).
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      uint64_t rest = ~done;
      while (rest) {
        const uint32_t t = ctz64(rest);
        rest &= rest - 1;
        const uint32_t o = readlane(opt, t), sl = readlane(slo, t), L = readlane(len, t), off = readlane(offset, t);
        if (lane < L) {
          uint32_t k = lane;
          if (k >= off) {  // k mod off for k, off <= 64: exact through the f32 reciprocal
            const uint32_t q = (uint32_t)(((float)k + 0.5f) * __builtin_amdgcn_rcpf((float)off));
            k -= q * off;
          }
          win[o + lane - wbase] = win[sl + k - wbase];
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
      }
      op += X;
      if (!kWhole && __builtin_expect(op > op_lim, 0)) return kErrCross;  // a tag crosses the fragment end
      win_flush(out, win, wbase, flushed, op & ~15u, lane);  // whole 16-byte blocks to HBM
      flushed = max(flushed, op & ~15u);
      ip = ipw;
    }
    if (issue_pre2) fetch_pre2();  // (no batch at ip: the ring moved for a big literal alone)

    if (__builtin_expect(big && (kWhole || op < op_lim), 0)) {  // (at op_lim the literal opens the next fragment)
      // one literal too long for the batch path (or a wrapped length): straight to HBM
      const uint64_t hv = ring_get8(ring, ip);
      const Tag t = with_trailer(tag_head(uniform((uint32_t)hv & 0xff)), uniform((uint32_t)(hv >> 8)));  // decode_tag, in its two steps
      const uint32_t litlen = t.literal_len();
      const uint32_t lsrc = ip + 1 + t.taglen;
      const int64_t avail_out = (int64_t)size - (int64_t)op;
      const int64_t avail_in = (int64_t)N - (int64_t)lsrc;
      if (avail_out < (int64_t)litlen || avail_in < (int64_t)litlen) return kErrLiteral;  // :518
      if (!kWhole && (uint64_t)op + litlen > op_lim) return kErrCross;
      if (litlen <= kMaxBatchLit) {
        // a short literal with 2-4 length bytes (a non-minimal encoding, or a wrapped length): its
        // bytes are in the ring (the tag is in the batch window, ip < wb + 512, so lsrc + litlen <
        // wb + 717 < wb + 768), so the whole wave ors them into the window as the batch round does
        // its long literals, then flushes whole 16-byte blocks as a batch does -- no full flush and
        // window reload from HBM per such tag.  (Every byte before op & ~15 is in
        // HBM here, as after a batch: a shift drops only flushed bytes.)
        if (op - wbase + litlen + 32 > kWin) win_shift(win, wbase, op, lane);  // (uniform)
        const uint32_t k = 16 * lane;
        if (k < litlen)
          lds_or16(winA + (op - wbase) + k, 0, trim16(lds_get16(ringA + ((lsrc + k) & (kRing - 1)), 0), min(16u, litlen - k)));
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        op += litlen;
        win_flush(out, win, wbase, flushed, op & ~15u, lane);
        flushed = max(flushed, op & ~15u);
        ip = lsrc + litlen;
        continue;
      }
      win_flush(out, win, wbase, flushed, op, lane);  // HBM holds everything before the literal
      // bulk copy: head bytes to 16-B source alignment, then 16 B per lane, kLit in flight
      const uint8_t* s = in + lsrc;
      uint32_t head = (uint32_t)((16 - ((uintptr_t)s & 15)) & 15);
      if (head > litlen) head = litlen;
      if (lane < head) out[op + lane] = s[lane];
      const uint4* s16 = reinterpret_cast<const uint4*>(s + head);
      const uint32_t n16 = (litlen - head) >> 4;
      uint8_t* d = out + op + head;
      uint32_t k = lane;
      for (; k + (kLit - 1) * kWave < n16; k += kLit * kWave) {
        uint4 v[kLit];
#pragma unroll
        for (uint32_t j = 0; j < kLit; ++j) v[j] = s16[k + j * kWave];
#pragma unroll
        for (uint32_t j = 0; j < kLit; ++j) st16u(d + 16 * (k + j * kWave), v[j]);
      }
      for (; k < n16; k += kWave) st16u(d + 16 * k, s16[k]);
      const uint32_t done16 = head + (n16 << 4);
      if (lane < litlen - done16) out[op + done16 + lane] = s[done16 + lane];
      // the window restarts at nb = the 16-byte output boundary at or below op + litlen - kKeep
      // (not below the decode's first output block), filled from HBM -- which now holds all
      // output before op + litlen -- with zeros past op + litlen (any literal length, a wrapped
      // 0 included); older sources come from HBM
      const uint32_t opn = op + litlen;
      const uint32_t nb = (opn - min(opn - wlo, kKeep)) & ~15u;
      const uint32_t nk = opn - nb;
      __threadfence_block();  // (this wave's stores above land before the loads below)
      const uint8_t* q = out + nb;
      for (uint32_t u = lane; u < kWin / 16; u += kWave) {
        const uint32_t x = 16 * u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (x + 16 <= nk) {
          const du64u* g = reinterpret_cast<const du64u*>(q + x);
          const uint64_t a = g[0], b = g[1];
          v = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        } else if (x < nk) {  // the last bytes: never read past the output
          uint64_t lo = 0, hi = 0;
          for (uint32_t i = 0; i < nk - x; ++i) {
            const uint64_t bt = (uint64_t)q[x + i] << (8 * (i & 7));
            if (i < 8) lo |= bt;
            else hi |= bt;
          }
          v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
        reinterpret_cast<uint4*>(win)[u] = v;
      }
      wbase = nb;
      op += litlen;
      flushed = op;
      ip = lsrc + litlen;
    }
  }
  win_flush(out, win, wbase, flushed, op, lane);
  op_end = op;
  return kOk;
}

#ifndef SM_DEC_OCC
#define SM_DEC_OCC 7  // waves per SIMD: 70 VGPRs, 5.0 KB LDS per wave (6: 1.29 against 1.25 ms; 8 would spill)
#endif
// one stream of the batch (block b) by one wave
template <uint32_t kLit = 4>
__device__ inline void decompress_block(const DecompressArgs& a, uint32_t b, uint8_t* sring, uint16_t* sjt, uint8_t* swin,
                                        uint32_t lane) {
  const uint8_t* in = a.one_n ? a.in : a.in + a.in_off[b];
  const uint32_t N = a.one_n ? a.one_n : a.in_len[b];
  uint8_t* dst = a.one_n ? a.out : a.out + a.out_off[b];
  const uint32_t cap = a.one_n ? a.one_cap : a.out_cap[b];

  uint32_t size = cap, ip = 0;
  if (N >= kOutLenError) {  // a compressor error mark, not a length: the slot holds no stream
    if (lane == 0) {
      a.status[b] = kErrDevice;
      a.out_len[b] = 0;
    }
    return;
  }
  int32_t st = a.raw ? kOk : parse_header(in, N, lane, size, ip);
  if (st == kOk && size > cap) st = kBufferTooSmall;
  if (st == kOk) {
    uint32_t op_end = 0;
    st = decode_stream_batch<kLit, true>(in, N, ip, N, size, dst, 0, 0, sring, sjt, swin, lane, op_end);
    if (st == kOk && op_end != size) st = kErrInvalid;                                    // Snappy.jl:50
  }
  if (lane == 0) {
    a.status[b] = st;
    a.out_len[b] = st == kOk ? size : 0;
  }
}

__global__ __launch_bounds__(64, SM_DEC_OCC) void k_decompress(DecompressArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t sring[kRing + kRingMirror];
  __shared__ __attribute__((aligned(16))) uint16_t sjt[kJt];  // tag-walk jump tables
  __shared__ __attribute__((aligned(16))) uint8_t swin[kWinPad + kWin];  // output window
  decompress_block(a, blockIdx.x, sring, sjt, swin + kWinPad, lane_id());
}

// sm_uncompress's in-order path (a.one_n: one stream, one wave): the same engine with 16 loads a
// lane in flight in long literals -- a lone wave's bulk copy is bound by load latency, not by the
// VGPRs that set the batch kernel's occupancy (fireworks.jpeg's literal-only stream: see
// DESIGN.md section 3.4)
__global__ __launch_bounds__(64, 1) void k_decompress_one(DecompressArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t sring[kRing + kRingMirror];
  __shared__ __attribute__((aligned(16))) uint16_t sjt[kJt];
  __shared__ __attribute__((aligned(16))) uint8_t swin[kWinPad + kWin];
  decompress_block<16>(a, 0, sring, sjt, swin + kWinPad, lane_id());
}

// ---- one fragment of a large block-structured stream (step 3 of "one large stream",
// sm_dec_stream.hip): from the chunk entry the host's path gives to the tag at output F, then the
// batch engine over [F, lim)
__global__ __launch_bounds__(64, 4) void k_decompress_frags(const uint8_t* __restrict__ in, uint32_t N, uint32_t size,
                                                            uint8_t* out, const StreamFrag* frags, int32_t* status) {
  __shared__ __attribute__((aligned(16))) uint8_t sring[kRing + kRingMirror];
  __shared__ __attribute__((aligned(16))) uint16_t sjt[kJt];
  __shared__ __attribute__((aligned(16))) uint8_t swin[kWinPad + kWin];
  __shared__ __attribute__((aligned(16))) uint8_t sbuf[kIdxChunk + kIdxPad];
  const uint32_t f = blockIdx.x, lane = lane_id();
  const StreamFrag fr = frags[f];
  // walk from the chunk entry to the tag that starts at output F (inside that chunk), a
  // 256-byte window at a time: the first tag whose preceding output reaches F
  stage_bytes(sbuf, in, N, fr.y, kIdxChunk + kIdxPad, lane);
  __syncthreads();
  uint64_t p = fr.y, o = fr.O;
  int32_t st = kOk;
  while (o < fr.F) {
    const uint32_t rel0 = (uint32_t)(p - fr.y);
    if (rel0 >= kIdxChunk + 16) {
      st = kErrCross;
      break;
    }
    uint32_t rel, next, ob, excl;
    const uint32_t ntok = window_tags(sbuf, rel0, min(kIdxChunk + 16 - rel0, 256u), sjt, lane, rel, next, ob, excl);
    if (ntok == 0) {  // long literal
      const Tag t = tag_at(sbuf, rel0);
      o += t.out_bytes();
      p += t.size();
      continue;
    }
    const uint64_t hit = ballot(lane < ntok && o + excl >= fr.F);
    if (hit) {
      const uint32_t t = ctz64(hit);
      o += readlane(excl, t);
      p = fr.y + readlane(rel, t);
      break;
    }
    o += readlane(excl + ob, ntok - 1);
    p = fr.y + readlane(next, ntok - 1);
  }
  if (st == kOk && o != fr.F) st = kErrCross;  // no tag starts at F: not block-structured
  if (st == kOk) {
    uint32_t op_end = 0;
    st = decode_stream_batch(in, N, (uint32_t)p, N, size, out, fr.F, fr.F, sring, sjt, swin + kWinPad, lane, op_end, fr.lim);
    if (st == kOk && op_end != (fr.lim == 0xffffffffu ? size : fr.lim)) st = kErrCross;
  }
  if (lane == 0) status[f] = st;
}

// ---- validation and declared lengths, no output -----------------------
// k_validate: the decoder's tag walk and checks (decode_stream_batch, internal.jl:411-527)
// without moving data: a block's status is exactly what uncompress(block) returns with an
// unlimited output buffer (snappy-c.h snappy_validate_compressed_buffer).  One wave per block,
// a 256-byte window per step, staged from HBM into LDS.
__global__ __launch_bounds__(64) void k_validate(const uint8_t* __restrict__ d_in, const uint64_t* in_off,
                                                 const uint32_t* in_len, int32_t* status) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[320];
  __shared__ __attribute__((aligned(16))) uint16_t jt[kJt];
  const uint32_t b = blockIdx.x, lane = lane_id();
  const uint8_t* in = d_in + in_off[b];
  const uint32_t N = in_len[b];
  if (N >= kOutLenError) {  // a compressor error mark (k_decompress): no read of the slot
    if (lane == 0) status[b] = kErrDevice;
    return;
  }
  uint32_t size, ip;
  int32_t st = parse_header(in, N, lane, size, ip);
  uint64_t op = 0, p = ip;
  const uint64_t lim = N ? N - 1 : 0;  // tags start below N-1 (:416)
  while (st == kOk && p < lim) {
    stage_bytes(buf, in, N, (uint32_t)p, 320, lane);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    uint32_t rel, next, ob, excl;
    const uint32_t ntok = window_tags(buf, 0, (uint32_t)min(lim - p, (uint64_t)256), jt, lane, rel, next, ob, excl);
    const bool mine = lane < ntok || (ntok == 0 && lane == 0);  // ntok == 0: a long literal at p
    const Tag t = tag_at(buf, mine ? rel : 0u);
    const uint32_t taglen = t.taglen, litlen = t.literal_len();
    const uint64_t opt = op + (ntok ? excl : 0u);
    const int32_t err = mine ? check_tag(t, opt, size, p + (ntok ? rel : 0u) + 1 + taglen, N) : kOk;
    const uint64_t em = ballot(err != kOk);
    if (em) {
      st = (int32_t)readlane((uint32_t)err, ctz64(em));
      break;
    }
    if (ntok == 0) {
      op += readlane(litlen, 0);
      p += 1 + readlane(taglen, 0) + (uint64_t)readlane(litlen, 0);
    } else {
      op += readlane(excl + ob, ntok - 1);
      p += readlane(next, ntok - 1);
    }
  }
  if (st == kOk && op != size) st = kErrInvalid;  // Snappy.jl:50
  if (lane == 0) status[b] = st;
}

// k_uncompressed_length: the varint header of each block (length_uncompressed,
// src/Snappy.jl:90-92), one thread per block
__global__ __launch_bounds__(256) void k_uncompressed_length(const uint8_t* __restrict__ d_in, const uint64_t* in_off,
                                                             const uint32_t* in_len, uint32_t nblk, uint32_t* out_len,
                                                             int32_t* status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblk) return;
  const uint8_t* in = d_in + in_off[b];
  const uint32_t N = in_len[b];
  uint32_t v = 0, hv;
  int32_t st = kErrDevice;  // (N a compressor error mark: no read)
  if (N < kOutLenError) st = smc::parse_varint32([&](uint32_t i) { return (uint32_t)in[i]; }, N, v, hv);
  out_len[b] = st == kOk ? v : 0;
  status[b] = st;
}

hipError_t launch_validate(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nblk,
                           int32_t* status, hipStream_t s) {
  if (nblk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_validate, dim3(nblk), dim3(64), 0, s, in, in_off, in_len, status);
  return hipGetLastError();
}

hipError_t launch_uncompressed_length(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                      uint32_t nblk, uint32_t* out_len, int32_t* status, hipStream_t s) {
  if (nblk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_uncompressed_length, dim3((nblk + 255) / 256), dim3(256), 0, s, in, in_off, in_len, nblk,
                     out_len, status);
  return hipGetLastError();
}

hipError_t launch_decompress_frags(const uint8_t* in, uint32_t N, uint32_t size, uint8_t* out,
                                   const StreamFrag* frags, uint32_t nfrag, int32_t* status, hipStream_t s) {
  if (nfrag == 0) return hipSuccess;
  hipLaunchKernelGGL(k_decompress_frags, dim3(nfrag), dim3(64), 0, s, in, N, size, out, frags, status);
  return hipGetLastError();
}

hipError_t launch_decompress(const DecompressArgs& a, int /*large*/, hipStream_t s) {
  if (a.nblk == 0) return hipSuccess;
  if (a.one_n && a.nblk == 1)
    hipLaunchKernelGGL(k_decompress_one, dim3(1), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_decompress, dim3(a.nblk), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace sm
