// sm_api.hip -- C ABI (include/snappy_mi355x.h) over the gfx950 kernels.
// Host framing follows src/Snappy.jl:20-52: varint header, 64 KiB fragments sharing one
// table size derived from the total length (quirk Q2), final produced==declared check (the
// latter lives in the decode kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/snappy_mi355x.h"
#include "common/smc_hip_host.h"
#include "sm_device.h"
#include "sm_internal.h"

#ifndef SM_VERSION_STR
#define SM_VERSION_STR "dev"
#endif

// Host staging: page-aligned ordinary memory registered for DMA (hipHostRegister), so the CPU
// reads it through its caches -- the host walks the index records and scatters batch outputs
// from it.  (hipHostMalloc'd staging was read ~2x slower by those CPU loops.)  It is also mapped
// into the device (dp): the single-buffer calls' last kernel writes its result there directly,
// because a copy-engine transfer queued behind kernels waited up to ~120 us on this box
// (tools/probes/latency_probe.hip, profiles/r04_latency_probe.txt).
// Visibility: kernels store results into this memory and the host reads them only after
// hipStreamSynchronize on the launching stream; HIP makes a kernel's writes to host memory visible
// to the host at that synchronisation (the completion signal is a system-scope release), so the
// writers issue no fence of their own.  A __threadfence_system() in each writer
// was measured in round 5: every wave writes back the L2 (buffer_wbl2), and single calls took
// 20-45 us longer (alice29.txt compress 60 -> 104 us, urls.10K uncompress 296 -> 527 us, same box).
struct HostBuf {
  void* p = nullptr;
  void* dp = nullptr;  // the device's address of p (nullptr: not mapped)
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = ((n < (1u << 20) ? (1u << 20) : n) + 4095) & ~(size_t)4095;
    void* q = nullptr;
    if (posix_memalign(&q, 4096, want) != 0) return hipErrorOutOfMemory;
    const hipError_t e = hipHostRegister(q, want, hipHostRegisterMapped);
    if (e != hipSuccess) {
      free(q);
      return e;
    }
    p = q;
    cap = want;
    if (hipHostGetDevicePointer(&dp, q, 0) != hipSuccess) dp = nullptr;
    return hipSuccess;
  }
  void release() {
    if (p) {
      (void)hipHostUnregister(p);
      free(p);
    }
    p = nullptr;
    dp = nullptr;
    cap = 0;
  }
};

// A single-buffer call's result in that staging, by the convention above: the last kernel writes
// the bytes at 0 and its verdict words behind them at the next multiple of 256, and the host reads
// both after the stream's synchronisation, the words through a volatile pointer.
struct PinnedResult {
  HostBuf& st;
  size_t w_off = 0;
  bool ensure(size_t nbytes, size_t wbytes = 64) {  // false: no mapped staging of that size
    w_off = (nbytes + 255) / 256 * 256;
    return st.ensure(w_off + wbytes) == hipSuccess && st.dp;
  }
  uint8_t* d_bytes() const { return (uint8_t*)st.dp; }  // the launch's pointers
  template <typename T = uint32_t>
  T* d_words() const { return (T*)((uint8_t*)st.dp + w_off); }
  template <typename T = uint32_t>
  volatile T* words() const { return (volatile T*)((uint8_t*)st.p + w_off); }  // the host's
  const void* bytes() const { return st.p; }
};

struct sm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy = nullptr;     // host->device copies that overlap the kernels (sm_compress)
  std::vector<hipEvent_t> ev;     // their completion events
  DevBuf in, out, out2, meta, idx, gat, org;  // org: origin pointers of the general parallel decode
  HostBuf stage;
  HostBuf stage_in;              // small host inputs on their way up (upload_input)
  hipEvent_t in_ev = nullptr;    // recorded behind the last upload from stage_in
  int last_path = -1;  // sm_ctx_last_path
  bool small = true;   // sm_ctx_set_small_decode
  bool split = true;   // sm_ctx_set_split_compress
  bool last_split = false;  // the last sm_compress parsed its fragments in parts
  std::mutex mu;       // serialises the host-buffer entry points (they share the scratch above)
  // The device batch compress calls' part scratch (batch_parts_scratch), one per stream they were
  // given: calls on one stream run in order and share it, calls on different streams may overlap.
  // Allocated at full size on a stream's first call and never grown, so no later call frees or
  // synchronises; beyond kPartStreams streams a call takes the whole-block path.
  static constexpr int kPartStreams = 8;
  struct PartScratch {
    hipStream_t stream = nullptr;
    DevBuf buf;
  };
  PartScratch part[kPartStreams];
  int nparts = 0;
  std::mutex part_mu;  // the scratch table, and a call's launches that use a scratch (compress_device)
  std::atomic<int> last_parts{0};  // sm_ctx_last_batch_parts
};

namespace {

using sm::PathChunk;

#ifdef SM_HOST_TRACE  // diagnostic builds: phase times of the single-buffer entry points on stderr
#include <chrono>
#include <cstdio>
struct HostTrace {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(const char* what, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "  %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};
#define HT_DECL HostTrace ht_;
#define HT(what) ht_.mark(what, s);
#else
#define HT_DECL
#define HT(what)
#endif

constexpr size_t kOrgKeep = 256u << 20;  // origin-pointer scratch a context keeps after a decode
constexpr size_t kPipeMinInput = 32u << 20;  // sm_compress: inputs this large upload in pieces
constexpr size_t kSmallCompressMax = 4u << 20;  // sm_compress: inputs up to this size (64 fragments) synchronise once
constexpr uint32_t kPieceFrags = 256;        // 16 MiB per piece
#ifndef SM_OUT_PIECE
#define SM_OUT_PIECE 2048
#endif
constexpr uint32_t kOutPieceFrags = SM_OUT_PIECE;  // sm_uncompress: output pieces (128 MiB)

constexpr size_t kPinnedInMin = 32u << 10;  // host inputs from this size up (to sm::kPinnedInMax) go through stage_in

// A HIP failure behind launches that may read the pinned input staging: nothing stays queued
// when the call returns, so no later call can free pages the device still reads.
sm_status device_failure(hipStream_t s) {
  (void)hipStreamSynchronize(s);
  return SM_ERR_DEVICE;
}

// One call's use of the context's pinned, device-mapped input staging (ctx->stage_in): acquire()
// waits until the device is done with the previous contents (in_ev, recorded behind the last
// launch that read them) before the buffer may grow -- growing unregisters and frees the old
// pages -- and copies the caller's bytes in; finish() goes behind the last launch that reads the
// staging and records that event, once (an event between the launches costs each call ~4 us).
// When a launch or the record failed it synchronises the stream instead, and so does the
// destructor on any exit that did not reach finish(): no return leaves a reader queued.
struct StagedInput {
  sm_ctx* const ctx;
  const hipStream_t s;
  const uint8_t* dp = nullptr;  // the staged bytes for the device; null: nothing a launch may read
  StagedInput(sm_ctx* c, hipStream_t st) : ctx(c), s(st) {}
  StagedInput(const StagedInput&) = delete;
  ~StagedInput() {
    if (dp) (void)hipStreamSynchronize(s);
  }
  bool acquire(const void* src, size_t n) {  // false: no staging
    if (ctx->in_ev && hipEventSynchronize(ctx->in_ev) != hipSuccess) return false;
    if (ctx->stage_in.ensure(n + 16) != hipSuccess || !ctx->stage_in.dp) return false;
    memcpy(ctx->stage_in.p, src, n);
    dp = (const uint8_t*)ctx->stage_in.dp;
    return true;
  }
  hipError_t finish(hipError_t le) {  // le: the result of the launches that read the staging
    if (le == hipSuccess && !ctx->in_ev && (le = hipEventCreateWithFlags(&ctx->in_ev, hipEventDisableTiming)) != hipSuccess)
      ctx->in_ev = nullptr;
    if (le == hipSuccess) le = hipEventRecord(ctx->in_ev, s);
    if (le != hipSuccess) (void)hipStreamSynchronize(s);
    dp = nullptr;
    return le;
  }
  void drained() { dp = nullptr; }  // the caller synchronised the stream behind the readers
};

// A host input of a single-buffer call into ctx->in.  Inputs of 32 KiB to 16 MiB are copied on
// the host into the context's pinned, device-mapped staging and moved to the device by a copy
// kernel (k_to_host reading the mapped pages): fireworks.jpeg's uncompress 60 -> 50 us, html's
// 70 -> 67, 64 KiB compress 52 -> 48 (profiles/r06_upload_ab.txt).  Smaller inputs stay with the
// runtime's pageable copy, which is 2-4 us faster there than the staging (its event and the
// extra launch), and so does an upload through the copy engine from the staging at every size.
hipError_t upload_input(sm_ctx* ctx, const void* src, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  StagedInput in(ctx, s);
  if (n >= kPinnedInMin && n <= sm::kPinnedInMax && in.acquire(src, n))
    return in.finish(sm::launch_to_host(in.dp, (uint32_t)n, (uint8_t*)ctx->in.p, nullptr, 0, nullptr, s));
  return hipMemcpyAsync(ctx->in.p, src, n, hipMemcpyHostToDevice, s);
}

// What a decode path of sm_uncompress did.
struct PathResult {
  enum Kind { kTaken, kFallBack, kDeviceError, kStreamError } kind;
  int path = 0;             // kTaken, kStreamError: what sm_ctx_last_path reports
  int32_t status = SM_OK;   // kStreamError: the stream's first error (the reference throws: no output)
  bool in_ctx_out = false;  // kTaken: the output is in ctx->out (else already in the caller's buffer)
};
constexpr PathResult kFallBack{PathResult::kFallBack}, kDeviceError{PathResult::kDeviceError};

// path 5: the input into the pinned staging on the host, the literals to the pinned output by
// k_literal_spans reading and writing the mapped pages, then the bytes to the caller.  Falls back
// when there is no mapped staging.
PathResult literal_uncompress(sm_ctx* ctx, const uint8_t* comp, size_t n, uint32_t size, const sm::LitSpans& ls,
                              uint8_t* host_out) {
  hipStream_t s = ctx->stream;
  PinnedResult res{ctx->stage};
  StagedInput in(ctx, s);
  if (!res.ensure(size) || !in.acquire(comp, n)) return kFallBack;
  volatile uint32_t* const w = res.words();
  w[1] = 0xffffffffu;  // (the kernel writes SM_OK)
  if (sm::launch_literal_spans(in.dp, ls, res.d_bytes(), res.d_words(), s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  in.drained();
  if (w[1] != 0 || w[0] != size) return kDeviceError;
  memcpy(host_out, res.bytes(), size);
  return {PathResult::kTaken, 5};
}

// the context's copy stream and at least n events (created on first use)
hipError_t ensure_copy_stream(sm_ctx* ctx, size_t n) {
  if (!ctx->copy) {
    const hipError_t e = hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking);
    if (e != hipSuccess) {
      ctx->copy = nullptr;
      return e;
    }
  }
  while (ctx->ev.size() < n) {
    hipEvent_t e;
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    ctx->ev.push_back(e);
  }
  return hipSuccess;
}

// The first error of a stream whose tag path is known: one wave per path element checks its tags
// (k_path_check), and the first failing element in path order holds the reference's status.  With
// no failing tag the stream is short of its declared length (Snappy.jl:50).  Path 3 with that
// status, or a fall back to the in-order decode.
PathResult path_first_error(sm_ctx* ctx, uint32_t n, uint32_t size, const std::vector<PathChunk>& path) {
  if (n >= 0x80000000u || path.empty()) return kFallBack;
  hipStream_t s = ctx->stream;
  const size_t npath = path.size();
  const std::vector<sm::OriginPath> op = sm::origin_path(path, true);
  if (ctx->org.ensure(sm::carve_origin(nullptr, 0, npath).end) != hipSuccess) return kFallBack;
  const sm::OriginScratch sc = sm::carve_origin(ctx->org.p, 0, npath);
  if (hipMemcpyAsync(sc.path, op.data(), npath * sizeof(sm::OriginPath), hipMemcpyHostToDevice, s) != hipSuccess)
    return kDeviceError;
  if (sm::launch_path_check((const uint8_t*)ctx->in.p, n, size, sc.path, (uint32_t)npath, sc.st, s) != hipSuccess)
    return kDeviceError;
  std::vector<int32_t> st(npath);
  if (hipMemcpyAsync(st.data(), sc.st, npath * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  for (int32_t v : st) {
    if (v == sm::kOk) continue;
    if (v == sm::kErrCross) return kFallBack;  // the tags do not tile an element: let the in-order decode decide
    return {PathResult::kStreamError, 3, v};
  }
  const PathChunk& last = path.back();
  if (last.O + last.out == size) return kFallBack;  // no failing tag and the right length: not an error after all
  return {PathResult::kStreamError, 3, sm::kErrInvalid};  // Snappy.jl:50
}

// One large stream in parallel (sm_dec_stream.hip, "one large stream"; the fragment decode: sm_decompress.hip): index pass, true path
// on the host, one wave per 64 KiB fragment.  The compressed bytes are in ctx->in.  Path 1 (or 2,
// origin pointers) with the output in ctx->out, path 3 when the stream has an error (its first
// one in stream order), or a fall back to the in-order decode.  With host_out, a large output
// goes down in pieces on the copy stream as the fragment decode finishes them (then host_out
// holds the result of path 1).
PathResult parallel_uncompress(sm_ctx* ctx, const uint8_t* comp, uint32_t n, uint32_t ip0, uint32_t size,
                               uint8_t* host_out) {
  const uint32_t nchunks = (n - ip0 + sm::kIdxChunk - 1) / sm::kIdxChunk;
  const uint32_t nfrag = (uint32_t)(((uint64_t)size + 65535) / 65536);
  const size_t rec_bytes = sm::parallel_rec_words(nchunks) * 4;
  if (ctx->idx.ensure(sm::carve_parallel(nullptr, nchunks, nfrag).end) != hipSuccess) return kFallBack;  // (the in-order decode needs no scratch)
  hipStream_t s = ctx->stream;
  HT_DECL
  const sm::ParallelScratch sc = sm::carve_parallel(ctx->idx.p, nchunks, nfrag);
  const uint8_t* d_in = (const uint8_t*)ctx->in.p;
  if (sm::launch_stream_index(d_in, n, ip0, nchunks, sc.rec, s) != hipSuccess) return kDeviceError;
  HT("index kernel")
  // the index records (8 B per entry, ~9 MB per 64 MiB of stream) come back through the
  // context's pinned staging: one DMA, no page faults, no zero fill
  if (ctx->stage.ensure(rec_bytes) != hipSuccess) return kFallBack;
  if (hipMemcpyAsync(ctx->stage.p, sc.rec, rec_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  HT("index records D2H")
  std::vector<PathChunk> path;
  const sm::PathEnd end = sm::true_path(comp, n, ip0, size, (const uint32_t*)ctx->stage.p, path);
  if (end == sm::PathEnd::kFallBack) return kFallBack;
  if (end == sm::PathEnd::kFirstError) return path_first_error(ctx, n, size, path);
  const std::vector<sm::StreamFrag> frags = sm::path_frags(path, size);
  HT("host path + fragments")
  if (hipMemcpyAsync(sc.frags, frags.data(), frags.size() * sizeof(sm::StreamFrag), hipMemcpyHostToDevice, s) !=
      hipSuccess)
    return kDeviceError;
  const uint32_t nfp = (nfrag + kOutPieceFrags - 1) / kOutPieceFrags;
  const uint32_t npiece = (host_out && nfp > 1 && ensure_copy_stream(ctx, nfp) == hipSuccess) ? nfp : 1;
  uint8_t* out = (uint8_t*)ctx->out.p;
  for (uint32_t pc = 0; pc < npiece; ++pc) {
    const uint32_t f0 = pc * kOutPieceFrags, f1 = npiece == 1 ? nfrag : std::min(nfrag, f0 + kOutPieceFrags);
    if (sm::launch_decompress_frags(d_in, n, size, out, sc.frags + f0, f1 - f0, sc.st + f0, s) != hipSuccess)
      return kDeviceError;
    if (npiece > 1 && hipEventRecord(ctx->ev[pc], s) != hipSuccess) return kDeviceError;
  }
  if (npiece > 1) {  // each piece's output goes down while the later pieces decode
    for (uint32_t pc = 0; pc < npiece; ++pc) {
      const size_t b0 = (size_t)pc * kOutPieceFrags * 65536;
      const size_t b1 = std::min((size_t)size, b0 + (size_t)kOutPieceFrags * 65536);
      if (hipStreamWaitEvent(ctx->copy, ctx->ev[pc], 0) != hipSuccess) return kDeviceError;
      if (hipMemcpyAsync(host_out + b0, out + b0, b1 - b0, hipMemcpyDeviceToHost, ctx->copy) != hipSuccess)
        return kDeviceError;
    }
    if (hipStreamSynchronize(ctx->copy) != hipSuccess) return kDeviceError;
  }
  std::vector<int32_t> st(nfrag);
  if (hipMemcpyAsync(st.data(), sc.st, nfrag * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  HT("fragment decode")
  bool cross = false;
  for (int32_t v : st) {
    if (v == sm::kErrCross) cross = true;
    else if (v != sm::kOk) return path_first_error(ctx, n, size, path);  // the first error, in parallel
  }
  if (!cross) return {PathResult::kTaken, 1, SM_OK, npiece == 1};
  // Not block-structured (a copy reaches into an earlier block): origin pointers per output
  // byte, resolved by pointer jumping (sm_dec_stream.hip, "any large stream").
  if (n >= 0x80000000u || size >= 0x80000000u) return kFallBack;  // 31-bit positions
  const size_t npath = path.size();
  const std::vector<sm::OriginPath> op = sm::origin_path(path, false);
  if (ctx->org.ensure(sm::carve_origin(nullptr, size, npath).end) != hipSuccess) return kFallBack;  // (4 B per output byte: the in-order decode needs none)
  const sm::OriginScratch og = sm::carve_origin(ctx->org.p, size, npath);
  if (hipMemcpyAsync(og.path, op.data(), npath * sizeof(sm::OriginPath), hipMemcpyHostToDevice, s) != hipSuccess)
    return kDeviceError;
  if (sm::launch_origin_fill(d_in, n, size, og.path, (uint32_t)npath, og.P, og.st, s) != hipSuccess) return kDeviceError;
  std::vector<int32_t> st2(npath);
  if (hipMemcpyAsync(st2.data(), og.st, npath * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  for (int32_t v : st2)
    if (v != sm::kOk) return path_first_error(ctx, n, size, path);
  // round k moves every unresolved pointer >= 2^k chain steps: 32 rounds cover any size
  bool done = false;
  for (int round = 0; round < 32 && !done; ++round) {
    uint32_t pend = 0;
    if (hipMemsetAsync(og.pend, 0, 4, s) != hipSuccess) return kDeviceError;
    if (sm::launch_origin_resolve(og.P, size, og.pend, s) != hipSuccess) return kDeviceError;
    if (hipMemcpyAsync(&pend, og.pend, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
    if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
    done = pend == 0;
  }
  if (!done) return kFallBack;
  if (sm::launch_origin_gather(d_in, og.P, size, (uint8_t*)ctx->out.p, s) != hipSuccess) return kDeviceError;
  if (ctx->org.cap > kOrgKeep) {  // 4 B per output byte: do not keep gigabytes in the context
    if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
    ctx->org.release();
  }
  return {PathResult::kTaken, 2, SM_OK, true};
}

// A small stream entirely on the device (sm_dec_stream.hip, "a small stream"): index, chain,
// origin pointers, resolve, gather, then one synchronisation with the output's download.  Path 4
// with the output in host_out, or a fall back (an error or anything unexpected: the old paths
// find the reference's first error).  comp: the call's input on the host.  It goes to the device
// through the index launch (the pinned staging read there, the device copy written there); a fall
// back before any launch leaves ctx->in without it.
PathResult small_uncompress(sm_ctx* ctx, const uint8_t* comp, uint32_t n, uint32_t ip0, uint32_t size, uint8_t* host_out) {
  const sm::SmallPlan pl = sm::small_plan(n - ip0, size);
  if (ctx->idx.ensure(sm::carve_small(nullptr, pl.nchunks, pl.rounds).end) != hipSuccess) return kFallBack;
  if (ctx->org.ensure((size_t)size * 4) != hipSuccess) return kFallBack;
  // the output and the verdict words straight into the pinned staging (a large output: the words
  // only, the output by a copy into host_out)
  const bool pin_out = size <= sm::kPinnedOutMax;
  PinnedResult res{ctx->stage};
  if (!res.ensure(pin_out ? size : 0)) return kFallBack;
  hipStream_t s = ctx->stream;
  const sm::SmallScratch sc = sm::carve_small(ctx->idx.p, pl.nchunks, pl.rounds);
  StagedInput in(ctx, s);
  if (!in.acquire(comp, n)) return kFallBack;
  volatile uint32_t* const w = res.words();
  w[2] = 0;  // the third verdict word is written by the device only when a pointer stays unresolved
  if (in.finish(sm::launch_small_decode((const uint8_t*)ctx->in.p, in.dp, n, ip0, size, pl.chunk, pl.nchunks, sc.rec,
                                        sc.path, sc.ctl, (uint32_t*)ctx->org.p, pl.rounds, pl.hops,
                                        pin_out ? res.d_bytes() : (uint8_t*)ctx->out.p, res.d_words(), s)) != hipSuccess)
    return kDeviceError;
  if (!pin_out && hipMemcpyAsync(host_out, ctx->out.p, size, hipMemcpyDeviceToHost, s) != hipSuccess) return kDeviceError;
  if (hipStreamSynchronize(s) != hipSuccess) return kDeviceError;
  if (w[0] || w[1] || w[2]) return kFallBack;  // (w[2]: never, by the round count -- checked, not assumed)
  if (pin_out) memcpy(host_out, res.bytes(), size);
  return {PathResult::kTaken, 4};
}

using sm::Shard;

template <typename F>
sm_status run_shards(int nctx, F&& shard_fn) {
  std::vector<sm_status> st((size_t)nctx, SM_OK);
  std::vector<std::thread> th;
  th.reserve((size_t)nctx);
  for (int i = 0; i < nctx; ++i) th.emplace_back([&, i] { st[(size_t)i] = shard_fn(i); });
  for (auto& t : th) t.join();
  for (sm_status x : st)
    if (x != SM_OK) return x;
  return SM_OK;
}

// The blocks [d_src + src_off[b], +len[b]) of a device batch back to host + out_off[b]: one
// gather launch packs them back to back in ctx->out2, one D2H transfer brings them into the
// pinned staging buffer, and the host scatters them (instead of one small copy per block).
// len: host copy of the lengths (0 = nothing to copy); d_len: the same on the device.
sm_status gather_to_host(sm_ctx* ctx, const uint8_t* d_src, const uint64_t* d_src_off, const uint32_t* d_len,
                         const uint32_t* len, uint32_t nblk, const uint64_t* out_off, uint8_t* host) {
  hipStream_t s = ctx->stream;
  std::vector<uint64_t> dst(nblk);
  uint64_t total = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    dst[b] = total;
    total += len[b];
  }
  if (total == 0) return SM_OK;
  if (ctx->gat.ensure(8 * (size_t)nblk) != hipSuccess || ctx->out2.ensure(total + 16) != hipSuccess ||
      ctx->stage.ensure(total) != hipSuccess)
    return SM_ERR_DEVICE;
  uint64_t* d_dst = (uint64_t*)ctx->gat.p;
  if (hipMemcpyAsync(d_dst, dst.data(), 8 * (size_t)nblk, hipMemcpyHostToDevice, s) != hipSuccess) return SM_ERR_DEVICE;
  if (sm::launch_gather(d_src, d_src_off, d_len, d_dst, (uint8_t*)ctx->out2.p, nblk, s) != hipSuccess)
    return SM_ERR_DEVICE;
  if (hipMemcpyAsync(ctx->stage.p, ctx->out2.p, total, hipMemcpyDeviceToHost, s) != hipSuccess) return SM_ERR_DEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) return SM_ERR_DEVICE;
  const uint8_t* st = (const uint8_t*)ctx->stage.p;
  for (uint32_t b = 0; b < nblk; ++b)
    if (len[b]) memcpy(host + out_off[b], st + dst[b], len[b]);
  return SM_OK;
}

// A host batch on its way up: ctx->in, ctx->out and the tables *t in ctx->meta made large enough,
// then the input and the caller's tables copied (out_cap: the decode's; null for compress).
hipError_t upload_batch(sm_ctx* ctx, const uint8_t* in, size_t in_total, size_t out_total, const uint64_t* in_off,
                        const uint64_t* out_off, const uint32_t* in_len, const uint32_t* out_cap, uint32_t nblk,
                        sm::BatchTables* t) {
  hipStream_t s = ctx->stream;
  hipError_t e = ctx->in.ensure(in_total + 16);
  if (e == hipSuccess) e = ctx->out.ensure(out_total + 16);
  if (e == hipSuccess) e = ctx->meta.ensure(sm::carve_batch(nullptr, nblk, out_cap != nullptr).end);
  if (e != hipSuccess) return e;
  *t = sm::carve_batch(ctx->meta.p, nblk, out_cap != nullptr);
  e = hipMemcpyAsync(ctx->in.p, in, in_total, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(t->in_off, in_off, 8 * (size_t)nblk, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(t->out_off, out_off, 8 * (size_t)nblk, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(t->in_len, in_len, 4 * (size_t)nblk, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && out_cap) e = hipMemcpyAsync(t->out_cap, out_cap, 4 * (size_t)nblk, hipMemcpyHostToDevice, s);
  return e;
}

bool valid_ctxs(sm_ctx* const* ctxs, int nctx) {
  if (!ctxs || nctx <= 0) return false;
  for (int i = 0; i < nctx; ++i) {
    if (!ctxs[i]) return false;
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return false;  // two shards on one ctx would race on its scratch
  }
  return true;
}
}  // namespace

extern "C" {

int sm_ctx_last_path(sm_ctx* ctx) { return ctx ? ctx->last_path : -1; }

sm_status sm_ctx_set_small_decode(sm_ctx* ctx, int enable) {
  if (!ctx) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->small = enable != 0;
  return SM_OK;
}

sm_status sm_ctx_set_split_compress(sm_ctx* ctx, int enable) {
  if (!ctx) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->split = enable != 0;
  return SM_OK;
}

int sm_ctx_last_compress_split(sm_ctx* ctx) { return ctx ? (ctx->last_split ? 1 : 0) : -1; }

const char* sm_status_message(sm_status st) {
  switch (st) {
    case SM_OK: return "OK";
    case SM_INVALID_INPUT: return "Invalid input.";
    case SM_BUFFER_TOO_SMALL: return "Buffer too small.";
    case SM_ERR_INPUT_TOO_LARGE: return "Input too large.";
    case SM_ERR_INVALID: return "Invalid input.";
    case SM_ERR_VARINT: return "Could not decode varint32.";
    case SM_ERR_COPY_OFFSET: return "Invalid input: corrupt copy offset";
    case SM_ERR_COPY_LENGTH: return "Invalid input: corrupt copy length";
    case SM_ERR_LITERAL: return "Invalid input: corrupt literal";
    case SM_ERR_DEVICE: return "HIP device error.";
    case SM_ERR_ARGUMENT: return "Invalid argument.";
    default: return "Unknown status.";
  }
}

const char* sm_version(void) { return "snappy_mi355x gfx950 " SM_VERSION_STR; }

size_t sm_max_compressed_length(size_t n) { return smc::max_compressed_length(n); }

sm_status sm_parse32(const uint8_t* buf, size_t len, size_t off, uint32_t* value, size_t* next) {
  return sm::parse32(buf, len, off, value, next);
}

size_t sm_encode32(uint8_t* buf, uint32_t v) { return sm::encode32(buf, v); }

sm_status sm_find_match_length(const uint8_t* buf, size_t len, size_t i1, size_t i2, size_t limit,
                               size_t* matched) {
  if (!matched || (len && !buf)) return SM_ERR_ARGUMENT;
  // 8 bytes at a time while i2 + 7 <= limit, then bytes (internal.jl:356-386); every read
  // the reference makes must lie inside buf
  auto ld64 = [&](size_t i, uint64_t* v) {
    if (i + 8 > len) return false;
    memcpy(v, buf + i, 8);
    return true;
  };
  size_t m = 0;
  while (i2 + 7 <= limit) {
    uint64_t a, b;
    if (!ld64(i1 + m, &a) || !ld64(i2, &b)) return SM_ERR_ARGUMENT;
    if (a != b) {
      *matched = m + (__builtin_ctzll(a ^ b) >> 3);
      return SM_OK;
    }
    i2 += 8;
    m += 8;
  }
  while (i2 <= limit) {
    if (i2 >= len || i1 + m >= len) return SM_ERR_ARGUMENT;
    if (buf[i1 + m] != buf[i2]) break;
    ++i2;
    ++m;
  }
  *matched = m;
  return SM_OK;
}

sm_status sm_uncompressed_length(const char* compressed, size_t n, size_t* result) {
  uint32_t v = 0;
  sm_status st = sm_parse32((const uint8_t*)compressed, n, 0, &v, nullptr);
  if (st == SM_OK && result) *result = v;
  return st;
}

sm_ctx* sm_ctx_create(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return nullptr;
  sm_ctx* ctx = new (std::nothrow) sm_ctx();
  if (!ctx) return nullptr;
  ctx->device = device;
  DeviceGuard g(device);
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void sm_ctx_destroy(sm_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->in.release();
    ctx->out.release();
    ctx->out2.release();
    ctx->meta.release();
    ctx->idx.release();
    ctx->gat.release();
    ctx->org.release();
    for (int i = 0; i < ctx->nparts; ++i) ctx->part[i].buf.release();  // (the caller's streams are the caller's to drain)
    ctx->stage.release();
    ctx->stage_in.release();
    if (ctx->in_ev) (void)hipEventDestroy(ctx->in_ev);
    if (ctx->copy) {
      (void)hipStreamSynchronize(ctx->copy);
      (void)hipStreamDestroy(ctx->copy);
    }
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
}

void* sm_ctx_stream(sm_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

namespace {

// SM_BATCH_PARTS=0 in the environment (read once): the device batch calls parse every block with
// the whole-block kernel, as before the remainder rule -- the same bytes, for tests and A/Bs
bool batch_parts_enabled() {
  static const bool on = [] {
    const char* e = getenv("SM_BATCH_PARTS");
    return !(e && e[0] == '0' && e[1] == 0);
  }();
  return on;
}

// the part scratch of ctx for calls on stream s (nullptr: none to be had, take the whole-block
// path); ctx->part_mu is held.  Nothing is allocated while s is being captured into a graph (an
// allocation there fails or invalidates the capture): a scratch the stream already has is used,
// else the call takes the whole-block path.
uint8_t* batch_parts_buffer(sm_ctx* ctx, hipStream_t s) {
  for (int i = 0; i < ctx->nparts; ++i)
    if (ctx->part[i].stream == s) return (uint8_t*)ctx->part[i].buf.p;
  if (ctx->nparts == sm_ctx::kPartStreams) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return nullptr;
  }
  sm_ctx::PartScratch& ps = ctx->part[ctx->nparts];
  if (ps.buf.ensure(sm::batch_parts_scratch(sm::compress_grid())) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  ps.stream = s;
  ++ctx->nparts;
  return (uint8_t*)ps.buf.p;
}

// the device batch calls' compress launches (ctx's device is current).  A call that parses its
// remainder in parts holds ctx->part_mu from the scratch lookup to its last enqueue: the launches
// of two host threads on one stream must not interleave (screen, parse into the scratch, gather
// out of it), or the later call's parts would replace the earlier one's before its gather runs.
hipError_t compress_device(sm_ctx* ctx, const sm::CompressArgs& a, int mode, hipStream_t s) {
  if (mode != SM_MODE_REFERENCE && batch_parts_enabled()) {
    const sm::BatchParts bp = sm::batch_parts_rule(a.nblk, sm::compress_grid());
    if (bp.rem) {
      std::lock_guard<std::mutex> lk(ctx->part_mu);
      uint8_t* const scratch = batch_parts_buffer(ctx, s);
      if (scratch) {
        ctx->last_parts.store((int)bp.rem, std::memory_order_relaxed);
        return sm::launch_compress_batch_parts(a, mode, bp, scratch, s);
      }
    }
  }
  ctx->last_parts.store(0, std::memory_order_relaxed);
  return sm::launch_compress(a, mode, s);
}

}  // namespace

sm_status sm_compress_batch_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                   const uint32_t* d_in_len, uint32_t nblk, uint8_t* d_out,
                                   const uint64_t* d_out_off, uint32_t* d_out_len, int mode, void* stream) {
  if (!ctx || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  sm::CompressArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_len, nblk, 0, 1};
  SM_CHECK(compress_device(ctx, a, mode, (hipStream_t)stream));
  return SM_OK;
}

sm_status sm_compress_fragments_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                       const uint32_t* d_in_len, uint32_t nblk, uint8_t* d_out,
                                       const uint64_t* d_out_off, uint32_t* d_out_len, uint64_t total_len,
                                       int mode, void* stream) {
  if (!ctx || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (total_len > 0xffffffffull) return SM_ERR_INPUT_TOO_LARGE;        // src/Snappy.jl:21
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  sm::CompressArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_len, nblk, sm::hashtable_size(total_len), 0};
  SM_CHECK(compress_device(ctx, a, mode, (hipStream_t)stream));
  return SM_OK;
}

int sm_ctx_last_batch_parts(sm_ctx* ctx) { return ctx ? ctx->last_parts.load(std::memory_order_relaxed) : -1; }

void sm_batch_parts_plan(uint32_t nblk, uint32_t grid, uint32_t* rem, uint32_t* parts) {
  const sm::BatchParts bp = sm::batch_parts_rule(nblk, grid);
  if (rem) *rem = bp.rem;
  if (parts) *parts = bp.parts;
}

sm_status sm_place_fragments_device(sm_ctx* ctx, const uint8_t* d_src, const uint64_t* d_src_off,
                                    const uint32_t* d_len, uint32_t nfrag, const uint64_t* d_dst_off,
                                    uint64_t total_len, int write_header, uint8_t* d_dst, uint64_t dst_capacity,
                                    uint64_t* d_local_off, int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (total_len > 0xffffffffull) return SM_ERR_INPUT_TOO_LARGE;  // src/Snappy.jl:21
  if (nfrag == 0 && !write_header) return SM_OK;
  if (!d_dst || (nfrag && (!d_src || !d_src_off || !d_len || !d_dst_off))) return SM_ERR_ARGUMENT;
  if (write_header && dst_capacity < sm::varint_len((uint32_t)total_len)) return SM_BUFFER_TOO_SMALL;
  DeviceGuard g(ctx->device);
  SM_CHECK(sm::launch_place(d_src, d_src_off, d_len, d_dst_off, nfrag, total_len, write_header ? 1 : 0, dst_capacity,
                            d_dst, d_local_off, d_status, (hipStream_t)stream));
  return SM_OK;
}

sm_status sm_uncompress_batch_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                     const uint32_t* d_in_len, uint32_t nblk, uint8_t* d_out,
                                     const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                     uint32_t* d_out_len, int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  sm::DecompressArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, nblk};
  SM_CHECK(sm::launch_decompress(a, 0, (hipStream_t)stream));
  return SM_OK;
}

sm_status sm_compress_batch(sm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                            uint32_t nblk, uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int mode) {
  if (!ctx || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_len) return SM_ERR_ARGUMENT;
  size_t in_total = 0, out_total = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    if (in_len[b] > SM_BLOCK_SIZE) return SM_ERR_ARGUMENT;
    size_t ie = in_off[b] + in_len[b];
    size_t oe = out_off[b] + sm_max_compressed_length(in_len[b]);
    if (ie > in_total) in_total = ie;
    if (oe > out_total) out_total = oe;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  sm::BatchTables t;
  SM_CHECK(upload_batch(ctx, in, in_total, out_total, in_off, out_off, in_len, nullptr, nblk, &t));
  sm::CompressArgs a{(const uint8_t*)ctx->in.p, t.in_off, t.in_len, (uint8_t*)ctx->out.p, t.out_off, t.out_len,
                     nblk, 0, 1};
  SM_CHECK(sm::launch_compress(a, mode, s));
  SM_CHECK(hipMemcpyAsync(out_len, t.out_len, 4 * (size_t)nblk, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  SM_PASS(sm::check_compressed_lengths(out_len, in_len, nblk));
  // copy back only each block's bytes
  return gather_to_host(ctx, (const uint8_t*)ctx->out.p, t.out_off, t.out_len, out_len, nblk, out_off, out);
}

sm_status sm_uncompress_batch(sm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                              uint32_t nblk, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                              uint32_t* out_len, int32_t* status) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  size_t in_total = 0, out_total = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    size_t ie = in_off[b] + in_len[b];
    size_t oe = out_off[b] + out_cap[b];
    if (ie > in_total) in_total = ie;
    if (oe > out_total) out_total = oe;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  sm::BatchTables t;
  SM_CHECK(upload_batch(ctx, in, in_total, out_total, in_off, out_off, in_len, out_cap, nblk, &t));
  sm::DecompressArgs a{(const uint8_t*)ctx->in.p, t.in_off, t.in_len, (uint8_t*)ctx->out.p, t.out_off,
                       t.out_cap, t.out_len, t.status, nblk};
  SM_CHECK(sm::launch_decompress(a, 0, s));
  SM_CHECK(hipMemcpyAsync(out_len, t.out_len, 4 * (size_t)nblk, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(status, t.status, 4 * (size_t)nblk, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  for (uint32_t b = 0; b < nblk; ++b)
    if (status[b] != SM_OK) out_len[b] = 0;  // (the kernel already reports 0 for failed blocks)
  return gather_to_host(ctx, (const uint8_t*)ctx->out.p, t.out_off, t.out_len, out_len, nblk, out_off, out);
}

sm_status sm_validate_batch_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                   const uint32_t* d_in_len, uint32_t nblk, int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_status) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(sm::launch_validate(d_in, d_in_off, d_in_len, nblk, d_status, (hipStream_t)stream));
  return SM_OK;
}

sm_status sm_uncompressed_length_batch_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                              const uint32_t* d_in_len, uint32_t nblk, uint32_t* d_len,
                                              int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_len || !d_status) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(sm::launch_uncompressed_length(d_in, d_in_off, d_in_len, nblk, d_len, d_status, (hipStream_t)stream));
  return SM_OK;
}

sm_status sm_compress_batch_sharded(sm_ctx* const* ctxs, int nctx, const uint8_t* in, const uint64_t* in_off,
                                    const uint32_t* in_len, uint32_t nblk, uint8_t* out, const uint64_t* out_off,
                                    uint32_t* out_len, int mode) {
  if (!valid_ctxs(ctxs, nctx) || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_len) return SM_ERR_ARGUMENT;
  for (uint32_t b = 0; b < nblk; ++b)
    if (in_len[b] > SM_BLOCK_SIZE) return SM_ERR_ARGUMENT;
  const std::vector<Shard> sh = sm::make_shards(nctx, nblk, in_off, out_off);
  return run_shards(nctx, [&](int i) -> sm_status {
    const Shard& s = sh[(size_t)i];
    if (s.n == 0) return SM_OK;
    return sm_compress_batch(ctxs[i], in + s.in_base, s.in_off.data(), in_len + s.b0, s.n, out + s.out_base,
                             s.out_off.data(), out_len + s.b0, mode);
  });
}

sm_status sm_uncompress_batch_sharded(sm_ctx* const* ctxs, int nctx, const uint8_t* in, const uint64_t* in_off,
                                      const uint32_t* in_len, uint32_t nblk, uint8_t* out, const uint64_t* out_off,
                                      const uint32_t* out_cap, uint32_t* out_len, int32_t* status) {
  if (!valid_ctxs(ctxs, nctx)) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  const std::vector<Shard> sh = sm::make_shards(nctx, nblk, in_off, out_off);
  return run_shards(nctx, [&](int i) -> sm_status {
    const Shard& s = sh[(size_t)i];
    if (s.n == 0) return SM_OK;
    return sm_uncompress_batch(ctxs[i], in + s.in_base, s.in_off.data(), in_len + s.b0, s.n, out + s.out_base,
                               s.out_off.data(), out_cap + s.b0, out_len + s.b0, status + s.b0);
  });
}

sm_status sm_validate_compressed_buffer(sm_ctx* ctx, const char* compressed, size_t n) {
  if (!ctx || (n && !compressed)) return SM_ERR_ARGUMENT;
  if (n > 0xffffffffull) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  SM_CHECK(ctx->in.ensure(n + 16));
  SM_CHECK(ctx->meta.ensure(sm::carve_single(nullptr).end));
  const sm::SingleMeta m = sm::carve_single(ctx->meta.p);
  const uint64_t zero = 0;
  const uint32_t len32 = (uint32_t)n;
  int32_t st = SM_ERR_DEVICE;
  SM_CHECK(upload_input(ctx, compressed, n, s));
  SM_CHECK(hipMemcpyAsync(m.off, &zero, 8, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(m.in_len, &len32, 4, hipMemcpyHostToDevice, s));
  if (sm::launch_validate((const uint8_t*)ctx->in.p, m.off, m.in_len, 1, m.status, s) != hipSuccess) return device_failure(s);
  SM_CHECK(hipMemcpyAsync(&st, m.status, 4, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  return st;
}

// src/Snappy.jl:20-36 on the device: every 64 KiB fragment is one wave; fragments use the
// table size of the WHOLE input (Q2) and no per-fragment header; a gather kernel then
// concatenates them behind the varint header.
sm_status sm_compress(sm_ctx* ctx, const char* input, size_t n, char* compressed, size_t* compressed_length,
                      int mode) {
  if (!ctx || !compressed_length || (n && !input) || !compressed) return SM_ERR_ARGUMENT;
  if (!valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (n > 0xffffffffull) return SM_ERR_INPUT_TOO_LARGE;                  // Snappy.jl:21
  if (*compressed_length < sm_max_compressed_length(n)) return SM_BUFFER_TOO_SMALL;
  uint8_t hdr[5];
  size_t hl = sm_encode32(hdr, (uint32_t)n);                                // Snappy.jl:26
  memcpy(compressed, hdr, hl);
  if (n == 0) {
    *compressed_length = hl;
    return SM_OK;
  }
  const uint32_t nfrag = (uint32_t)((n + SM_BLOCK_SIZE - 1) / SM_BLOCK_SIZE);
  const size_t slot = smc::kMultiSlotPitch;  // a fragment's bound + 8, rounded up to 256
  std::vector<uint64_t> in_off(nfrag), out_off(nfrag), dst_off(nfrag);
  std::vector<uint32_t> in_len(nfrag), out_len(nfrag);
  for (uint32_t i = 0; i < nfrag; ++i) {
    in_off[i] = (uint64_t)i * SM_BLOCK_SIZE;
    size_t e = in_off[i] + SM_BLOCK_SIZE;
    in_len[i] = (uint32_t)((e < n ? e : n) - in_off[i]);
    out_off[i] = (uint64_t)i * slot;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  ctx->last_split = false;
  SM_CHECK(ctx->in.ensure(n + 16));
  SM_CHECK(ctx->out.ensure((size_t)nfrag * slot));
  SM_CHECK(ctx->out2.ensure(sm_max_compressed_length(n) + 16));
  SM_CHECK(ctx->meta.ensure(sm::carve_frags(nullptr, nfrag).end));
  const sm::FragTables t = sm::carve_frags(ctx->meta.p, nfrag);
  HT_DECL
  // Small inputs: one synchronisation -- the fragment table and the gather (with the lengths'
  // prefix sums) on the device; the gather kernel writes the stream body into the context's
  // pinned staging (device-mapped: no copy engine behind the kernels), copied out on the host.
  // The fast modes parse each fragment in parts on their own workgroups (k_compress_sc_span: the
  // same bytes, a fraction of one block's latency; up to 256 parts in all, one per CU).
  PinnedResult res{ctx->stage};  // the body, then (length, error) as two 64-bit words
  if (n <= kSmallCompressMax && res.ensure(sm_max_compressed_length(n) + 16, 16)) {
    uint32_t parts = 1;
    if (mode != SM_MODE_REFERENCE && ctx->split) {
      uint32_t p2 = 1;
      while (p2 < nfrag) p2 <<= 1;
      parts = std::min<uint32_t>(sm::kWave, sm::kMaxParts / p2);  // nfrag * parts <= 256 gather units
    }
    const uint32_t span = (uint32_t)((SM_BLOCK_SIZE / 1024 + parts - 1) / parts);
    const size_t sl = parts > 1 ? std::max<size_t>(slot, (size_t)parts * span * sm::kSpanSlot) : slot;
    SM_CHECK(ctx->out.ensure((size_t)nfrag * sl));
    sm::CompressArgs a{(const uint8_t*)ctx->in.p, t.in_off, t.in_len, (uint8_t*)ctx->out.p, t.out_off, t.out_len,
                       nfrag, sm::hashtable_size(n), 0};
    // fast modes: the screen (the first kernel) reads the input from the pinned staging and leaves
    // the device copy the parse reads -- no separate upload
    StagedInput in(ctx, s);
    if (mode != SM_MODE_REFERENCE && in.acquire(input, n)) {
      a.in_host = in.dp;
    } else {
      SM_CHECK(upload_input(ctx, input, n, s));
    }
    if (mode == SM_MODE_REFERENCE) {
      SM_CHECK(sm::launch_frag_plan(n, nfrag, sl, t.in_off, t.in_len, t.out_off, s));
    } else {  // (the screen, the fast modes' first kernel, writes the fragment table)
      a.plan_n = n;
      a.plan_slot = sl;
    }
    // the gather writes the body and its (length, error) pair straight into the pinned staging
    const sm::ScSpan sp{parts, span, (uint64_t)span * sm::kSpanSlot, t.part_len};
    hipError_t le = parts > 1 ? sm::launch_compress_span(a, mode, sp, s) : sm::launch_compress(a, mode, s);
    if (le == hipSuccess)
      le = parts > 1 ? sm::launch_parts_gather((const uint8_t*)ctx->out.p, t.out_off, sp, (const uint8_t*)ctx->in.p,
                                               t.in_off, t.in_len, nfrag, res.d_words<uint64_t>(), res.d_bytes(), s)
                     : sm::launch_frag_gather((const uint8_t*)ctx->out.p, t.out_off, t.out_len, t.in_len, nfrag,
                                              res.d_words<uint64_t>(), res.d_bytes(), s);
    // the staging's release behind the last launch; a failed launch synchronises instead (the
    // screen, the staging's only reader, may be queued)
    if (in.dp) le = in.finish(le);
    if (le != hipSuccess) return device_failure(s);
    SM_CHECK(hipStreamSynchronize(s));
    HT("compress (small): all")
    const volatile uint64_t* tot = res.words<uint64_t>();
    const uint64_t len = tot[0];
    if (tot[1]) return SM_ERR_DEVICE;  // a block's error mark (SM_OUT_LEN_ERROR), never expected
    if (hl + len > *compressed_length) return SM_BUFFER_TOO_SMALL;
    memcpy(compressed + hl, res.bytes(), len);
    *compressed_length = hl + len;
    ctx->last_split = parts > 1;
    return SM_OK;
  }
  SM_CHECK(hipMemcpyAsync(t.in_off, in_off.data(), 8 * (size_t)nfrag, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(t.out_off, out_off.data(), 8 * (size_t)nfrag, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(t.in_len, in_len.data(), 4 * (size_t)nfrag, hipMemcpyHostToDevice, s));
  // Large inputs go up in pieces on the copy stream, and each piece's fragments compress as
  // soon as it lands, so the kernels run under the rest of the upload.
  uint32_t npiece = n >= kPipeMinInput ? (nfrag + kPieceFrags - 1) / kPieceFrags : 1;
  if (npiece > 1 && ensure_copy_stream(ctx, npiece) != hipSuccess) npiece = 1;  // one upload then
  for (uint32_t pc = 0; pc < npiece; ++pc) {
    const uint32_t f0 = pc * kPieceFrags, f1 = npiece == 1 ? nfrag : std::min(nfrag, f0 + kPieceFrags);
    const size_t b0 = (size_t)f0 * SM_BLOCK_SIZE, b1 = std::min(n, (size_t)f1 * SM_BLOCK_SIZE);
    if (npiece == 1) {
      SM_CHECK(hipMemcpyAsync(ctx->in.p, input, n, hipMemcpyHostToDevice, s));
    } else {
      SM_CHECK(hipMemcpyAsync((uint8_t*)ctx->in.p + b0, input + b0, b1 - b0, hipMemcpyHostToDevice, ctx->copy));
      SM_CHECK(hipEventRecord(ctx->ev[pc], ctx->copy));
      SM_CHECK(hipStreamWaitEvent(s, ctx->ev[pc], 0));
    }
    sm::CompressArgs a{(const uint8_t*)ctx->in.p, t.in_off + f0, t.in_len + f0, (uint8_t*)ctx->out.p,
                       t.out_off + f0, t.out_len + f0, f1 - f0, sm::hashtable_size(n), 0};
    SM_CHECK(sm::launch_compress(a, mode, s));
  }
  HT("compress: H2D input + kernels")
  SM_CHECK(hipMemcpyAsync(out_len.data(), t.out_len, 4 * (size_t)nfrag, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  HT("compress: kernels + lengths")
  SM_PASS(sm::check_compressed_lengths(out_len.data(), in_len.data(), nfrag));
  size_t total = 0;
  for (uint32_t i = 0; i < nfrag; ++i) {
    dst_off[i] = total;
    total += out_len[i];
  }
  if (hl + total > *compressed_length) return SM_BUFFER_TOO_SMALL;
  SM_CHECK(hipMemcpyAsync(t.dst_off, dst_off.data(), 8 * (size_t)nfrag, hipMemcpyHostToDevice, s));
  SM_CHECK(sm::launch_gather((const uint8_t*)ctx->out.p, t.out_off, t.out_len, t.dst_off, (uint8_t*)ctx->out2.p,
                             nfrag, s));
  HT("compress: gather")
  SM_CHECK(hipMemcpyAsync(compressed + hl, ctx->out2.p, total, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  HT("compress: D2H output")
  *compressed_length = hl + total;
  return SM_OK;
}

// src/Snappy.jl:46-52: header parsed on the host (to size the output), the stream decoded by
// one wave (foreign streams carry no fragment index).
sm_status sm_uncompress(sm_ctx* ctx, const char* compressed, size_t n, char* uncompressed,
                        size_t* uncompressed_length) {
  if (!ctx || !uncompressed_length || (n && !compressed)) return SM_ERR_ARGUMENT;
  uint32_t size = 0;
  sm_status st = sm_parse32((const uint8_t*)compressed, n, 0, &size, nullptr);
  if (st != SM_OK) return st;
  if (n > 0xffffffffull) return SM_ERR_ARGUMENT;
  if (*uncompressed_length < size) return SM_BUFFER_TOO_SMALL;
  if (size && !uncompressed) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  SM_CHECK(ctx->in.ensure(n + 16));
  SM_CHECK(ctx->out.ensure((size_t)size + 16));
  SM_CHECK(ctx->meta.ensure(sm::carve_single(nullptr).end));
  const sm::SingleMeta m = sm::carve_single(ctx->meta.p);
  HT_DECL
  size_t hdr = 0;
  (void)sm_parse32((const uint8_t*)compressed, n, 0, &size, &hdr);
  const uint8_t* const comp = (const uint8_t*)compressed;
  uint8_t* const host_out = (uint8_t*)uncompressed;
  // The paths in turn, each falling back to the next.  Path 5: literal tags only (an
  // incompressible input) -- one copy kernel from the pinned input staging to the pinned output
  // staging, one synchronisation.  Path 4: a small stream entirely on the device.  Then a large
  // stream's fragments in parallel when it is block-structured (Snappy.jl, libsnappy and this
  // library all write such streams); otherwise, or on any error, the in-order decode (path 0).
  PathResult r = kFallBack;
  sm::LitSpans ls;
  if (ctx->small && size <= sm::kPinnedOutMax && n <= sm::kPinnedInMax && sm::literal_only(comp, n, hdr, size, ls))
    r = literal_uncompress(ctx, comp, n, size, ls, host_out);
  if (r.kind == PathResult::kFallBack && ctx->small && sm::small_candidate(n, hdr, size))
    r = small_uncompress(ctx, comp, (uint32_t)n, (uint32_t)hdr, size, host_out);
  if (r.kind == PathResult::kFallBack) {
    // (path 4 uploads through its index launch; every other path from here)
    SM_CHECK(upload_input(ctx, compressed, n, s));
    HT("uncompress: H2D input")
    if (sm::parallel_candidate(n, hdr, size)) r = parallel_uncompress(ctx, comp, (uint32_t)n, (uint32_t)hdr, size, host_out);
  }
  if (r.kind == PathResult::kDeviceError) return device_failure(s);
  ctx->last_path = r.path;  // (a fall back: 0, the in-order decode below)
  if (r.kind == PathResult::kStreamError) return r.status;
  if (r.kind == PathResult::kTaken) {
    if (r.in_ctx_out) {
      SM_CHECK(hipMemcpyAsync(uncompressed, ctx->out.p, size, hipMemcpyDeviceToHost, s));
      SM_CHECK(hipStreamSynchronize(s));
    }
    HT("uncompress: D2H output")
    *uncompressed_length = size;
    return SM_OK;
  }
  sm::DecompressArgs a{(const uint8_t*)ctx->in.p, m.off, m.in_len, (uint8_t*)ctx->out.p, m.off, m.cap, m.out_len,
                       m.status, 1};
  a.one_n = (uint32_t)n;  // (n >= 1 here: the header parsed) -- the stream's length and capacity as arguments
  a.one_cap = size;
  if (sm::launch_decompress(a, size > SM_BLOCK_SIZE, s) != hipSuccess) return device_failure(s);
  // the output (whatever the status) and (out_len, status) into the pinned staging by a kernel
  PinnedResult res{ctx->stage};
  if (size <= sm::kPinnedOutMax && res.ensure(size)) {
    SM_CHECK(sm::launch_to_host((const uint8_t*)ctx->out.p, size, res.d_bytes(), m.out_len, 2, res.d_words(), s));
    SM_CHECK(hipStreamSynchronize(s));
    const volatile uint32_t* w = res.words();
    const uint32_t dlen = w[0];
    const int32_t dst = (int32_t)w[1];
    if (dst != SM_OK) return dst;
    if (dlen > size) return SM_ERR_DEVICE;  // (never: the kernel's bound)
    if (dlen) memcpy(uncompressed, res.bytes(), dlen);  // (uncompressed may be NULL when dlen == 0)
    *uncompressed_length = dlen;
    return SM_OK;
  }
  int32_t dst = 0;
  uint32_t dlen = 0;
  SM_CHECK(hipMemcpyAsync(&dst, m.status, 4, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(&dlen, m.out_len, 4, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  if (dst != SM_OK) return dst;
  if (dlen) {
    SM_CHECK(hipMemcpyAsync(uncompressed, ctx->out.p, dlen, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipStreamSynchronize(s));
  }
  *uncompressed_length = dlen;
  return SM_OK;
}

sm_status sm_uncompress_fragments_device(sm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                         const uint32_t* d_in_len, uint32_t nblk, uint8_t* d_out,
                                         const uint64_t* d_out_off, const uint32_t* d_frag_len, uint32_t* d_out_len,
                                         int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_frag_len || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  sm::DecompressArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_frag_len, d_out_len, d_status, nblk, 1};
  SM_CHECK(sm::launch_decompress(a, 0, (hipStream_t)stream));
  return SM_OK;
}

// ---- snappy-c.h-shaped entry points on a process-wide default context --------------------
// The exact ccall shape of the reference's libsnappy helper (test/libsnappy.jl:5-30):
// (Ptr{UInt8}, Csize_t, Ptr{UInt8}, Ref{Csize_t}) -> Cint, so a binding rebinds by symbol name
// alone.  The default context lives on device SNAPPY_MI355X_DEVICE (default 0); its mutex
// serialises callers.

namespace {
std::mutex g_default_mu;
sm_ctx* g_default_ctx = nullptr;
// Dense by default: a drop-in caller gets stream sizes within 1.01x of Snappy.jl's on every
// corpus file, and a single call's fixed costs (PCIe, launches) hide dense's extra kernel time.
std::atomic<int> g_default_mode{SM_MODE_FAST_DENSE};  // set and read from any thread

sm_ctx* default_ctx() {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default_ctx) {
    const char* e = getenv("SNAPPY_MI355X_DEVICE");
    g_default_ctx = sm_ctx_create(e ? atoi(e) : 0);
  }
  return g_default_ctx;
}
}  // namespace

namespace {
// snappy-c.h knows three statuses: 0 OK, 1 INVALID_INPUT, 2 BUFFER_TOO_SMALL.  The detailed codes
// (the reference's messages 16-21, device and argument failures) stay on the ctx API.
sm_status snappy_c_status(sm_status st) {
  return st == SM_OK ? SM_OK : (st == SM_BUFFER_TOO_SMALL ? SM_BUFFER_TOO_SMALL : SM_INVALID_INPUT);
}
}  // namespace

sm_status sm_snappy_set_mode(int mode) {
  if (!valid_mode(mode)) return SM_ERR_ARGUMENT;
  g_default_mode.store(mode, std::memory_order_relaxed);
  return SM_OK;
}

sm_status sm_snappy_compress(const char* input, size_t input_length, char* compressed, size_t* compressed_length) {
  sm_ctx* ctx = default_ctx();
  if (!ctx) return SM_INVALID_INPUT;
  return snappy_c_status(sm_compress(ctx, input, input_length, compressed, compressed_length,
                                     g_default_mode.load(std::memory_order_relaxed)));
}

sm_status sm_snappy_uncompress(const char* compressed, size_t compressed_length, char* uncompressed,
                               size_t* uncompressed_length) {
  sm_ctx* ctx = default_ctx();
  if (!ctx) return SM_INVALID_INPUT;
  return snappy_c_status(sm_uncompress(ctx, compressed, compressed_length, uncompressed, uncompressed_length));
}

size_t sm_snappy_max_compressed_length(size_t source_length) { return sm_max_compressed_length(source_length); }

sm_status sm_snappy_uncompressed_length(const char* compressed, size_t compressed_length, size_t* result) {
  return snappy_c_status(sm_uncompressed_length(compressed, compressed_length, result));
}

sm_status sm_snappy_validate_compressed_buffer(const char* compressed, size_t compressed_length) {
  sm_ctx* ctx = default_ctx();
  if (!ctx) return SM_INVALID_INPUT;
  return snappy_c_status(sm_validate_compressed_buffer(ctx, compressed, compressed_length));
}

}  // extern "C"
