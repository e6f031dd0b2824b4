// sm_internal.h -- launcher interfaces between the C-ABI layer (sm_api.hip) and the
// kernels (sm_compress.hip, sm_compress_fast.hip, sm_compress_sc.hip, sm_gather.hip;
// sm_decompress.hip, sm_dec_stream.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_host_rules.h"  // the HIP-free part: the types and constants the host rules share

namespace sm {

// Batch descriptor: block b is in[in_off[b] .. +in_len[b]) -> out[out_off[b] ..).
// All pointers are device pointers.
struct CompressArgs {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint8_t* out;
  const uint64_t* out_off;
  uint32_t* out_len;
  uint32_t nblk;
  uint32_t table_size;  // 0: per block from its length (internal.jl:107-113); else fixed (Q2)
  int header;           // 1: prefix each block with varint(len) (independent snappy stream)
  int screened;         // set by launch_compress_fast: out_len holds k_literal_screen's verdicts
  // plan_n != 0 (sm_compress, fast modes): the blocks are the 64 KiB fragments of one input of
  // plan_n bytes at slot pitch plan_slot, and k_literal_screen writes in_off / in_len / out_off
  // (instead of a k_frag_plan launch) before the kernels after it read them
  uint64_t plan_n = 0;
  uint64_t plan_slot = 0;
  // in_host != null (sm_compress, fast modes): the input in device-mapped pinned host memory; the
  // screen reads its block there and writes the device copy at `in`, which the parse reads
  const uint8_t* in_host = nullptr;
};

struct DecompressArgs {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* out_cap;
  uint32_t* out_len;
  int32_t* status;
  uint32_t nblk;
  int raw;  // 1: no varint header -- a fragment of one stream, declared length = out_cap[b]
  // one_n != 0 (sm_uncompress's in-order path): ONE stream of one_n bytes at in, output capacity
  // one_cap at out -- in_off / in_len / out_off / out_cap are not read (no upload for them)
  uint32_t one_n = 0;
  uint32_t one_cap = 0;
};

// out_len marks.  kNotABlock: a block longer than 64 KiB was refused (an error mark: it is above
// kOutLenError).  kScreenTodo: k_literal_screen's verdict "the parse compresses this block", read by
// the parse kernels of the same call and overwritten by them.
constexpr uint32_t kNotABlock = 0xffffffffu;
constexpr uint32_t kScreenTodo = 0xfffffffeu;

// mode 0 = reference (byte-identical to Snappy.jl), 1 = fast (wave-parallel parse), 2 = fast, denser
hipError_t launch_compress(const CompressArgs& a, int mode, hipStream_t s);
hipError_t launch_compress_fast(const CompressArgs& a, int mode, hipStream_t s);
hipError_t launch_compress_sc(const CompressArgs& a, int mode, hipStream_t s);  // sm_compress_sc.hip (after the screen)
hipError_t launch_decompress(const DecompressArgs& a, int large, hipStream_t s);

constexpr uint32_t kIdxPad = 288;     // staged bytes past a chunk: +16 entry slack, a 256-byte walk window + 16
hipError_t launch_validate(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nblk,
                           int32_t* status, hipStream_t s);
hipError_t launch_uncompressed_length(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                      uint32_t nblk, uint32_t* out_len, int32_t* status, hipStream_t s);
// rec: nchunks * kIdxEntries (exit, output) u32 pairs
hipError_t launch_stream_index(const uint8_t* in, uint32_t N, uint32_t ip0, uint32_t nchunks, uint32_t* rec,
                               hipStream_t s);
hipError_t launch_decompress_frags(const uint8_t* in, uint32_t N, uint32_t size, uint8_t* out,
                                   const StreamFrag* frags, uint32_t nfrag, int32_t* status, hipStream_t s);
hipError_t launch_origin_fill(const uint8_t* in, uint32_t N, uint32_t size, const OriginPath* path, uint32_t npath,
                              uint32_t* P, int32_t* status, hipStream_t s);
// The same walk without the pointers: per path element, the reference's exact status of its first
// failing tag (kErrCross: the element's tags do not tile it).
hipError_t launch_path_check(const uint8_t* in, uint32_t N, uint32_t size, const OriginPath* path, uint32_t npath,
                             int32_t* status, hipStream_t s);
hipError_t launch_origin_resolve(uint32_t* P, uint32_t size, uint32_t* pending, hipStream_t s);
// A small stream entirely on the device (index, chain, fill, `rounds` resolve launches, gather; no
// host synchronisation).  rec: nchunks * kIdxEntries u32 pairs, then nchunks * kDeepChains *
// kDeepLevels 16-byte deep-entry records; path: nchunks elements; ctl: 4 +
// rounds u32 (zeroed by the chain kernel) -- ctl[0] path elements, ctl[1] != 0: the chain found no exact path (fall
// back), ctl[2] != 0: an element failed its checks (fall back), ctl[4 + r] != 0: pointers still
// unresolved after round r.  P: size u32.  The resolve launches write the output (each quad of
// bytes in the launch that resolves it) and words[0..1] = ctl[1], ctl[2]; the last launch sets
// words[2] = 1 when a pointer is still unresolved after it (the caller zeroes words[2] first).  Any
// nonzero word: fall back.  out and words may be device-mapped pinned host memory.
// in_host (nullable): the input in device-mapped pinned host memory -- the index launch reads it
// there and writes the device copy at in, which the later launches read (no separate upload).
hipError_t launch_small_decode(const uint8_t* in, const uint8_t* in_host, uint32_t N, uint32_t ip0, uint32_t size, uint32_t chunk,
                               uint32_t nchunks, uint32_t* rec, OriginPath* path, uint32_t* ctl, uint32_t* P,
                               uint32_t rounds, uint32_t hops, uint8_t* out, uint32_t* words, hipStream_t s);
// src[0, n) to dst and wsrc[0, nw) to words by a kernel (dst, words: device-mapped pinned host
// memory; no copy engine behind the kernels -- or, for uploads, src mapped host memory and dst
// the device's).  src, dst 16-byte aligned; nw <= 256.
hipError_t launch_to_host(const uint8_t* src, uint32_t n, uint8_t* dst, const uint32_t* wsrc, uint32_t nw,
                          uint32_t* words, hipStream_t s);
// sm_uncompress path 5: the literals of sp (LitSpans) from in to out; words[0..1] = (length, SM_OK)
// behind the bytes.  in and out may be device-mapped host memory.
hipError_t launch_literal_spans(const uint8_t* in, const LitSpans& sp, uint8_t* out, uint32_t* words, hipStream_t s);
hipError_t launch_origin_gather(const uint8_t* in, const uint32_t* P, uint32_t size, uint8_t* out, hipStream_t s);
// sm_compress, small inputs (at most 64 fragments), without host round trips: the fragments'
// offsets and lengths (fragment f = input [64 KiB f, +64 KiB), output slot f at pitch `slot`);
// then, after the compress launch, the fragments gathered behind one another into dst (tot[0] =
// their total length, tot[1] = 1 on a bad length, when nothing is copied).
hipError_t launch_frag_plan(uint64_t n, uint32_t nfrag, uint64_t slot, uint64_t* in_off, uint32_t* in_len,
                            uint64_t* out_off, hipStream_t s);
// Fast modes, small inputs, for latency: each block parsed in `parts` parts of `span` 1 KiB
// super-chunks on their own workgroups (k_compress_sc_span; with launch_parts_gather, the same
// bytes as the whole-block parse).  Part j of block b writes at out + out_off[b] + j pitch (pitch >=
// span kSpanSlot) and its length to part_len[b parts + j]; parts * span >= 64.  Runs the screen
// first.
constexpr uint32_t kSpanSlot = 1088;  // a super-chunk's output bound (k_compress_sc's staging slot)
struct ScSpan {
  uint32_t parts, span;
  uint64_t pitch;
  uint32_t* part_len;
  // blk_pitch != 0 (the device batch calls' remainder blocks, launch_compress_batch_parts): block b's parts are
  // at out + b blk_pitch + j pitch (out_off is the caller's and is not read by the span kernel), and
  // a block the screen emitted as a literal -- it is in the caller's slot already -- has kPartScreened
  // as its part 0's length
  uint64_t blk_pitch = 0;
};
constexpr uint32_t kPartScreened = 0xffeffffdu;  // (below the error marks, above any length)
hipError_t launch_compress_span(const CompressArgs& a, int mode, const ScSpan& sp, hipStream_t s);
hipError_t launch_compress_sc_span(const CompressArgs& a, int mode, const ScSpan& sp, hipStream_t s);  // (no screen)
// the whole-block parse of a's blocks and, on workgroups behind the persistent ones in the same
// launch, r's blocks in sp.parts parts (sp.blk_pitch != 0; sp.parts == 0: none)
hipError_t launch_compress_sc_parts(const CompressArgs& a, const CompressArgs& r, const ScSpan& sp, int mode,
                                    hipStream_t s);
// The parts of nblk (<= 256 / parts) blocks behind one another into dst (a block whose parts sum to
// more than one literal of the block -- the whole-block parse's fallback -- as that literal, from
// in): tot[0] = the total, tot[1] = 1 on an error mark or an over-long part (nothing copied).
hipError_t launch_parts_gather(const uint8_t* src, const uint64_t* out_off, const ScSpan& sp, const uint8_t* in,
                               const uint64_t* in_off, const uint32_t* in_len, uint32_t nblk, uint64_t* tot,
                               uint8_t* dst, hipStream_t s);
// The device batch calls (sm_compress_batch_device, sm_compress_fragments_device; fast modes): the
// persistent whole-block kernel runs ceil(nblk / grid) rounds of blocks, the last of them on
// nblk % grid workgroups only.  When that remainder is at most half the grid, its blocks are parsed
// in `parts` parts each on workgroups of their own (span items of the same launch) and joined into the
// caller's slots (k_gather_parts_batch): the same bytes and lengths.
constexpr uint32_t kBlockScs = 64;       // 1 KiB super-chunks of a 64 KiB block
constexpr uint32_t kPartMinScs = 4;      // a part is at least this many super-chunks
struct BatchParts {
  uint32_t rem;    // the last `rem` blocks are parsed in parts (0: none, the whole-block kernel takes all)
  uint32_t parts;  // ... in this many parts each: the largest power of two with rem * parts <= grid
};
inline BatchParts batch_parts_rule(uint32_t nblk, uint32_t grid) {
  const uint32_t r = grid ? nblk % grid : 0u;  // (nblk < grid: every block)
  if (r == 0 || r > grid / 2) return {0u, 0u};
  uint32_t p = 2;
  while (p < kBlockScs / kPartMinScs && r * (2 * p) <= grid) p *= 2;
  return {r, p};
}
// the scratch launch_compress_batch_parts needs on a device of `grid` CUs: the parts' slots (16-byte
// aligned), then their lengths
inline size_t batch_parts_len_offset(uint32_t grid) { return (size_t)(grid / 2) * kBlockScs * kSpanSlot; }
inline size_t batch_parts_scratch(uint32_t grid) { return batch_parts_len_offset(grid) + 4 * (size_t)grid; }
// the current device's CU count (cached per device): the whole-block kernels' workgroup count for
// large batches, and reference mode's bound for one staged block per CU
inline uint32_t compress_grid() {
  static uint32_t ncu_cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  uint32_t ncu = __atomic_load_n(&ncu_cache[dev], __ATOMIC_RELAXED);
  if (!ncu) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    ncu = (uint32_t)v;
    __atomic_store_n(&ncu_cache[dev], ncu, __ATOMIC_RELAXED);
  }
  return ncu;
}
// launch_compress for modes 1 and 2 with the last bp.rem blocks in parts (bp from batch_parts_rule
// with compress_grid(); bp.rem != 0); scratch: batch_parts_scratch(compress_grid()) bytes, in use
// until the launches have run
hipError_t launch_compress_batch_parts(const CompressArgs& a, int mode, const BatchParts& bp, uint8_t* scratch,
                                       hipStream_t s);
hipError_t launch_batch_parts_gather(const CompressArgs& a, const uint8_t* src, const ScSpan& sp, hipStream_t s);
hipError_t launch_frag_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* out_len,
                              const uint32_t* in_len, uint32_t nfrag, uint64_t* tot, uint8_t* dst, hipStream_t s);
// a sharded stream's fragments at their global offsets (sm_place_fragments_device, k_place)
hipError_t launch_place(const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint64_t* dst_off,
                        uint32_t nfrag, uint64_t total, int header, uint64_t cap, uint8_t* dst, uint64_t* loc_off,
                        int32_t* status, hipStream_t s);
// concatenate per-fragment outputs into one stream after a varint header (single-buffer API)
hipError_t launch_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* len,
                         const uint64_t* dst_off, uint8_t* dst, uint32_t nblk, hipStream_t s);

}  // namespace sm
