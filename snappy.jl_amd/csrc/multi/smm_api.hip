// smm_api.hip -- C ABI of the multi-stream library (include/snappy_mi355x_multi.h) over the raw
// codec's public batched device calls (libsnappy_mi355x.so, linked by name) and the kernels of
// smm_kernels.hip, smm_index.hip and smm_range.hip (the ranged decode of
// include/snappy_mi355x_multi_range.h).  The host-only entry points live in smm_host.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../common/smc_hip_host.h"
#include "smm_plan.h"
#include "smm_range.h"

#ifndef SMM_VERSION_STR
#define SMM_VERSION_STR "dev"
#endif

namespace {

// any total_len above 16,384 gives the fragment call the 16,384-entry table (src/Snappy.jl:27):
// the table of every fragment of a stream longer than 64 KiB
constexpr uint64_t kLongTotal = 2 * (uint64_t)smm::kBlock;

}  // namespace

struct smm_ctx {
  sm_ctx* sm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;  // the sm_ctx's: the host-buffer calls run on it
  DevBuf hdr;                    // smm::Header
  DevBuf meta, slots;            // the per-call arrays; compress: the fragments' output slots, ranges: the edge slots
  DevBuf io_in, io_out, io_meta; // the host-buffer calls' staging
  bool called = false;           // an uncompress call has been made (smm_ctx_last_indexed)
  std::mutex mu;                 // serialises the host-buffer entry points
};

extern "C" {

const char* smm_status_message(sm_status st) { return sm_status_message(st); }

const char* smm_version(void) { return "snappy_mi355x_multi gfx950 " SMM_VERSION_STR; }

smm_ctx* smm_ctx_create(int device) {
  sm_ctx* sm = sm_ctx_create(device);
  if (!sm) return nullptr;
  smm_ctx* ctx = new (std::nothrow) smm_ctx();
  if (!ctx) {
    sm_ctx_destroy(sm);
    return nullptr;
  }
  ctx->sm = sm;
  ctx->device = device;
  ctx->stream = (hipStream_t)sm_ctx_stream(sm);
  bool ok;
  {
    DeviceGuard g(device);
    ok = ctx->hdr.ensure(smm::kHeaderBytes) == hipSuccess && hipMemset(ctx->hdr.p, 0, smm::kHeaderBytes) == hipSuccess;
  }
  if (!ok) {
    smm_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smm_ctx_destroy(smm_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->hdr, &ctx->meta, &ctx->slots, &ctx->io_in, &ctx->io_out, &ctx->io_meta}) b->release();
  }
  sm_ctx_destroy(ctx->sm);
  delete ctx;
}

int smm_ctx_last_indexed(smm_ctx* ctx) {
  if (!ctx || !ctx->called) return -1;
  DeviceGuard g(ctx->device);
  smm::Header h;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&h, ctx->hdr.p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int)h.indexed;
}

// Launch sequence: plan scan, plan fill, the raw batch compressor over the streams (the long ones
// masked), the raw fragment compressor over the slots, pack scan, pack, finish.
sm_status smm_compress_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t nstreams, uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                              uint32_t* d_out_len, int32_t* d_status, uint32_t* d_frag_first, uint32_t* d_frag_pos,
                              int mode, void* stream) {
  if (!ctx || !valid_mode(mode) || (d_frag_first == nullptr) != (d_frag_pos == nullptr)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  if (nstreams == 0) {
    if (d_frag_first) SM_CHECK(hipMemsetAsync(d_frag_first, 0, 4, s));
    return SM_OK;
  }
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  const uint32_t n = nstreams, m = max_fragments;
  SM_CHECK(ctx->meta.ensure(smm::compress_meta_bytes(n, m)));
  SM_CHECK(ctx->slots.ensure((size_t)m * smm::kSlotPitch));
  smm::CompressPlan p{d_in,   d_in_off,     d_in_len,   n, m, d_out, d_out_off, d_out_len,
                      d_status, d_frag_first, d_frag_pos, (const uint8_t*)ctx->slots.p,
                      smm::carve_compress((uint8_t*)ctx->meta.p, n, m), (smm::Header*)ctx->hdr.p};
  SM_CHECK(smm::launch_compress_plan(p, s));
  SM_PASS(sm_compress_batch_device(ctx->sm, d_in, d_in_off, p.s.s_in_len, n, d_out, p.s.s_out_off, p.s.s_comp_len, mode,
                                   stream));
  if (m)
    SM_PASS(sm_compress_fragments_device(ctx->sm, d_in, p.s.f_in_off, p.s.f_in_len, m, (uint8_t*)ctx->slots.p,
                                         p.s.f_slot_off, p.s.f_comp_len, kLongTotal, mode, stream));
  SM_CHECK(smm::launch_pack(p, s));
  return SM_OK;
}

// Launch sequence without an index: the raw batch decoder.  With one: plan scan, plan fill, the raw
// fragment decoder over the slots, verdict, reduce, the raw batch decoder over the streams (the
// indexed ones masked), merge.
sm_status smm_uncompress_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                uint32_t nstreams, uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                                const uint32_t* d_frag_first, const uint32_t* d_frag_pos, void* stream) {
  if (!ctx || (d_frag_first == nullptr) != (d_frag_pos == nullptr)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  ctx->called = true;
  smm::Header* hdr = (smm::Header*)ctx->hdr.p;
  if (nstreams == 0 || !d_frag_first) {
    SM_CHECK(hipMemsetAsync(&hdr->indexed, 0, 4, s));
    if (nstreams == 0) return SM_OK;
    return sm_uncompress_batch_device(ctx->sm, d_in, d_in_off, d_in_len, nstreams, d_out, d_out_off, d_out_cap, d_out_len,
                                      d_status, stream);
  }
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  const uint32_t n = nstreams, m = max_fragments;
  SM_CHECK(ctx->meta.ensure(smm::decode_meta_bytes(n, m)));
  smm::DecodePlan p{d_in,     d_in_off, d_in_len,     n,          m, d_out_off, d_out_cap, d_out_len,
                    d_status, d_frag_first, d_frag_pos, smm::carve_decode((uint8_t*)ctx->meta.p, n, m), hdr};
  SM_CHECK(smm::launch_decode_plan(p, s));
  if (m)
    SM_PASS(sm_uncompress_fragments_device(ctx->sm, d_in, p.s.f_in_off, p.s.f_in_len, m, d_out, p.s.f_out_off, p.s.f_len,
                                           p.s.f_out_len, p.s.f_status, stream));
  SM_CHECK(smm::launch_reduce(p, s));
  SM_PASS(sm_uncompress_batch_device(ctx->sm, d_in, d_in_off, p.s.fb_in_len, n, d_out, d_out_off, p.s.fb_cap, d_out_len,
                                     d_status, stream));
  SM_CHECK(smm::launch_merge(p, s));
  return SM_OK;
}

// Launch sequence: the counts' scan (with the short streams' entries), the walk of the long streams.
sm_status smm_index_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                           uint32_t nstreams, uint32_t max_fragments, const uint32_t* d_out_cap, uint32_t* d_frag_first,
                           uint32_t* d_frag_pos, uint8_t* d_built, int32_t* d_status, void* stream) {
  if (!ctx || !d_frag_first) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  if (nstreams == 0) {
    SM_CHECK(hipMemsetAsync(d_frag_first, 0, 4, s));
    return SM_OK;
  }
  if (!d_in || !d_in_off || !d_in_len || !d_built || !d_status || (!d_frag_pos && max_fragments)) return SM_ERR_ARGUMENT;
  SM_CHECK(ctx->meta.ensure(smm::index_scratch_bytes(nstreams)));
  smm::IndexPlan p{d_in,         d_in_off,   d_in_len, nstreams, max_fragments, d_out_cap,
                   d_frag_first, d_frag_pos, d_built,  d_status, smm::carve_index((uint8_t*)ctx->meta.p, nstreams)};
  SM_CHECK(smm::launch_index(p, s));
  return SM_OK;
}

// Launch sequence: find, scan, slots, the raw fragment decoder once over all slots (its output base
// the edge slots: smm_range.hip, k_mrange_slots), trim, verdict, result.
sm_status smm_uncompress_ranges_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                       const uint32_t* d_in_len, uint32_t nstreams, const uint32_t* d_frag_first,
                                       const uint32_t* d_frag_pos, uint32_t nentries, const uint32_t* d_range_stream,
                                       const uint32_t* d_lo, const uint32_t* d_len, uint32_t nranges,
                                       uint32_t max_range_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                       uint32_t* d_out_len, int32_t* d_status, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nranges == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_frag_first || !d_frag_pos || !d_range_stream || !d_lo || !d_len || !d_out ||
      !d_out_off || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t n = nranges, m = max_range_fragments;
  SM_CHECK(ctx->meta.ensure(smm::range_arrays_bytes(n, m)));
  SM_CHECK(ctx->slots.ensure(smm::range_edge_slots(n, m) * (size_t)smm::kEdgePitch));
  const smm::RangeArgs a{d_in,  d_in_off, d_in_len, nstreams,  d_frag_first, d_frag_pos,
                         nentries, d_range_stream, d_lo, d_len, n, m,
                         d_out, d_out_off, d_out_len, d_status,  (uint8_t*)ctx->slots.p,
                         smm::carve_range((uint8_t*)ctx->meta.p, n, m)};
  SM_CHECK(smm::launch_range_plan(a, s));
  if (m)
    SM_PASS(sm_uncompress_fragments_device(ctx->sm, d_in, a.s.f_in_off, a.s.f_in_len, m, a.edge, a.s.f_out_off, a.s.f_len,
                                           a.s.f_out_len, a.s.f_status, stream));
  SM_CHECK(smm::launch_range_finish(a, s));
  return SM_OK;
}

// ---- host buffers ------------------------------------------------------------------------------

namespace {  // (its functions are static: inside extern "C" the unnamed namespace alone still exports them)

// the device copies of a host call's per-stream arrays, in ctx->io_meta
struct HostArrays {
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *cap, *out_len, *first, *pos;
  int32_t* status;
  uint8_t* built;  // (smm_index)
  uintptr_t end;
};
static HostArrays carve_host(uintptr_t base, size_t n, size_t entries) {
  smm::Carve c{base};
  HostArrays a;
  a.in_off = c.take<uint64_t>(n);
  a.out_off = c.take<uint64_t>(n);
  a.in_len = c.take<uint32_t>(n);
  a.cap = c.take<uint32_t>(n);
  a.out_len = c.take<uint32_t>(n);
  a.status = c.take<int32_t>(n);
  a.first = c.take<uint32_t>(n + 1);
  a.pos = c.take<uint32_t>(entries);
  a.built = c.take<uint8_t>(n);
  a.end = c.p;
  return a;
}

// A host call's staging: the arrays, room for the streams' bytes, and the uploads both calls make
// (the input up to in_total and the three per-stream arrays), on s.
static sm_status upload_streams(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                const uint64_t* out_off, size_t n, size_t entries, size_t in_total, size_t out_total,
                                HostArrays& a, hipStream_t s) {
  SM_CHECK(ctx->io_meta.ensure(carve_host(0, n, entries).end));
  a = carve_host((uintptr_t)ctx->io_meta.p, n, entries);
  SM_CHECK(ctx->io_in.ensure(in_total + 16));
  SM_CHECK(ctx->io_out.ensure(out_total + 16));
  if (in_total) SM_CHECK(hipMemcpyAsync(ctx->io_in.p, in, in_total, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.in_off, in_off, 8 * n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.out_off, out_off, 8 * n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.in_len, in_len, 4 * n, hipMemcpyHostToDevice, s));
  return SM_OK;
}

// Each stream's own bytes down from ctx->io_out, behind the results' read-back (s is idle).  The
// most a stream can have written: out_cap[i], or without out_cap the compressor's bound for
// in_len[i].  Synchronises s.
static sm_status copy_out(smm_ctx* ctx, uint8_t* out, const uint64_t* out_off, const uint32_t* out_len,
                          const int32_t* status, size_t n, const uint32_t* in_len, const uint32_t* out_cap,
                          hipStream_t s) {
  for (size_t i = 0; i < n; ++i) {
    if (status[i] != SM_OK || out_len[i] == 0) continue;
    if (out_len[i] > (out_cap ? out_cap[i] : smm::max_compressed_length(in_len[i]))) return SM_ERR_DEVICE;
    SM_CHECK(hipMemcpyAsync(out + out_off[i], (const uint8_t*)ctx->io_out.p + out_off[i], out_len[i],
                            hipMemcpyDeviceToHost, s));
  }
  SM_CHECK(hipStreamSynchronize(s));
  return SM_OK;
}

// the device copies of a ranged host call's arrays, in ctx->io_meta (n streams, k ranges)
struct RangeHostArrays {
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *first, *pos, *range_stream, *lo, *len, *out_len;
  int32_t* status;
  uintptr_t end;
};
static RangeHostArrays carve_range_host(uintptr_t base, size_t n, size_t entries, size_t k) {
  smm::Carve c{base};
  RangeHostArrays a;
  a.in_off = c.take<uint64_t>(n);
  a.out_off = c.take<uint64_t>(k);
  a.in_len = c.take<uint32_t>(n);
  a.first = c.take<uint32_t>(n + 1);
  a.pos = c.take<uint32_t>(entries);
  a.range_stream = c.take<uint32_t>(k);
  a.lo = c.take<uint32_t>(k);
  a.len = c.take<uint32_t>(k);
  a.out_len = c.take<uint32_t>(k);
  a.status = c.take<int32_t>(k);
  a.end = c.p;
  return a;
}

}  // namespace

sm_status smm_compress(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                       uint32_t nstreams, uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int32_t* status,
                       uint32_t* frag_first, uint32_t* frag_pos, int mode) {
  if (!ctx || !valid_mode(mode) || (frag_first == nullptr) != (frag_pos == nullptr)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) {
    if (frag_first) frag_first[0] = 0;
    return SM_OK;
  }
  if (!in_off || !in_len || !out || !out_off || !out_len || !status) return SM_ERR_ARGUMENT;
  const size_t n = nstreams;
  size_t in_total = 0, out_total = 0;
  uint64_t entries = 0;
  for (size_t i = 0; i < n; ++i) {
    if (in_len[i] > smm::kMaxInput) continue;  // (refused on the device, unread)
    entries += smm::fragment_count(in_len[i]);
    const size_t ie = in_off[i] + in_len[i], oe = out_off[i] + smm::max_compressed_length(in_len[i]);
    if (ie > in_total) in_total = ie;
    if (oe > out_total) out_total = oe;
  }
  if (entries > 0x7fffffffull) return SM_ERR_INPUT_TOO_LARGE;
  if (in_total && !in) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  HostArrays a;
  SM_PASS(upload_streams(ctx, in, in_off, in_len, out_off, n, entries, in_total, out_total, a, s));
  SM_PASS(smm_compress_device(ctx, (const uint8_t*)ctx->io_in.p, a.in_off, a.in_len, nstreams, (uint32_t)entries,
                              (uint8_t*)ctx->io_out.p, a.out_off, a.out_len, a.status, frag_first ? a.first : nullptr,
                              frag_first ? a.pos : nullptr, mode, s));
  SM_CHECK(hipMemcpyAsync(out_len, a.out_len, 4 * n, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(status, a.status, 4 * n, hipMemcpyDeviceToHost, s));
  if (frag_first) {
    SM_CHECK(hipMemcpyAsync(frag_first, a.first, 4 * (n + 1), hipMemcpyDeviceToHost, s));
    if (entries) SM_CHECK(hipMemcpyAsync(frag_pos, a.pos, 4 * (size_t)entries, hipMemcpyDeviceToHost, s));
  }
  SM_CHECK(hipStreamSynchronize(s));
  return copy_out(ctx, out, out_off, out_len, status, n, in_len, nullptr, s);
}

sm_status smm_uncompress(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                         uint32_t nstreams, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                         uint32_t* out_len, int32_t* status, const uint32_t* frag_first, const uint32_t* frag_pos) {
  if (!ctx || (frag_first == nullptr) != (frag_pos == nullptr)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  const size_t n = nstreams;
  size_t in_total = 0, out_total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (in_len[i] >= SM_OUT_LEN_ERROR) continue;  // (an error mark: refused on the device, unread)
    const size_t ie = in_off[i] + in_len[i], oe = out_off[i] + out_cap[i];
    if (ie > in_total) in_total = ie;
    if (oe > out_total) out_total = oe;
  }
  const size_t entries = frag_first ? frag_first[n] : 0;
  if (entries > 0x7fffffffull) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  HostArrays a;
  SM_PASS(upload_streams(ctx, in, in_off, in_len, out_off, n, entries, in_total, out_total, a, s));
  SM_CHECK(hipMemcpyAsync(a.cap, out_cap, 4 * n, hipMemcpyHostToDevice, s));
  if (frag_first) {
    SM_CHECK(hipMemcpyAsync(a.first, frag_first, 4 * (n + 1), hipMemcpyHostToDevice, s));
    if (entries) SM_CHECK(hipMemcpyAsync(a.pos, frag_pos, 4 * entries, hipMemcpyHostToDevice, s));
  }
  SM_PASS(smm_uncompress_device(ctx, (const uint8_t*)ctx->io_in.p, a.in_off, a.in_len, nstreams, (uint32_t)entries,
                                (uint8_t*)ctx->io_out.p, a.out_off, a.cap, a.out_len, a.status,
                                frag_first ? a.first : nullptr, frag_first ? a.pos : nullptr, s));
  SM_CHECK(hipMemcpyAsync(out_len, a.out_len, 4 * n, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(status, a.status, 4 * n, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i)
    if (status[i] != SM_OK) out_len[i] = 0;
  return copy_out(ctx, out, out_off, out_len, status, n, in_len, out_cap, s);
}

sm_status smm_index(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                    uint32_t max_fragments, const uint32_t* out_cap, uint32_t* frag_first, uint32_t* frag_pos,
                    uint8_t* built, int32_t* status) {
  if (!ctx || !frag_first) return SM_ERR_ARGUMENT;
  if (nstreams == 0) {
    frag_first[0] = 0;
    return SM_OK;
  }
  if (!in || !in_off || !in_len || !built || !status || (!frag_pos && max_fragments)) return SM_ERR_ARGUMENT;
  const size_t n = nstreams, m = max_fragments;
  size_t in_total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (in_len[i] >= SM_OUT_LEN_ERROR) continue;  // (an error mark: no entries, unread)
    const size_t ie = in_off[i] + in_len[i];
    if (ie > in_total) in_total = ie;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  SM_CHECK(ctx->io_meta.ensure(carve_host(0, n, m).end));
  const HostArrays a = carve_host((uintptr_t)ctx->io_meta.p, n, m);
  SM_CHECK(ctx->io_in.ensure(in_total + 16));
  if (in_total) SM_CHECK(hipMemcpyAsync(ctx->io_in.p, in, in_total, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.in_off, in_off, 8 * n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.in_len, in_len, 4 * n, hipMemcpyHostToDevice, s));
  if (out_cap) SM_CHECK(hipMemcpyAsync(a.cap, out_cap, 4 * n, hipMemcpyHostToDevice, s));
  SM_PASS(smm_index_device(ctx, (const uint8_t*)ctx->io_in.p, a.in_off, a.in_len, nstreams, max_fragments,
                           out_cap ? a.cap : nullptr, a.first, a.pos, a.built, a.status, s));
  SM_CHECK(hipMemcpyAsync(frag_first, a.first, 4 * (n + 1), hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(built, a.built, n, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(status, a.status, 4 * n, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  const size_t entries = frag_first[n];  // (at most max_fragments: the device's own scan)
  if (entries > m) return SM_ERR_DEVICE;
  if (entries) SM_CHECK(hipMemcpy(frag_pos, a.pos, 4 * entries, hipMemcpyDeviceToHost));
  return SM_OK;
}

// The stream-level rule runs here first (the device's own code, smm_range.h): it names the streams
// that some range can be served from -- those alone go up, whole, at their own offsets, with their
// index entries -- and counts the slots.  A range the rule refuses here is final, and the device
// reads no stream for it.  The ranges' outputs lie behind one another in ctx->io_out, each at a
// 16-byte boundary.
sm_status smm_uncompress_ranges(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                uint32_t nstreams, const uint32_t* frag_first, const uint32_t* frag_pos,
                                const uint32_t* range_stream, const uint32_t* lo, const uint32_t* len, uint32_t nranges,
                                uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int32_t* status) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nranges == 0) return SM_OK;
  if (!in || !in_off || !in_len || !frag_first || !frag_pos || !range_stream || !lo || !len || !out || !out_off ||
      !out_len || !status)
    return SM_ERR_ARGUMENT;
  const size_t n = nstreams, k = nranges;
  const size_t entries = frag_first[n];
  if (entries > 0x7fffffffull) return SM_ERR_ARGUMENT;
  std::vector<uint8_t> named(n, 0);
  std::vector<uint64_t> d_off(k, 0);
  std::vector<uint32_t> d_stream(range_stream, range_stream + k);
  uint64_t slots = 0, out_total = 0;
  size_t in_total = 0;
  for (size_t r = 0; r < k; ++r) {
    smm::Candidate c;
    const smm::RangeSpan sp =
        smm::range_span(in, in_off, in_len, nstreams, frag_first, (uint32_t)entries, range_stream[r], lo[r], len[r], c);
    // A range that failed here is settled: the device gets it with a stream number past the last,
    // which its rule refuses with the same status before it reads a byte -- so it never looks at
    // a stream that did not go up.
    if (sp.status != SM_OK) d_stream[r] = nstreams;
    if (sp.status != SM_OK || sp.count == 0) continue;
    const uint32_t s = range_stream[r];
    named[s] = 1;
    const size_t ie = in_off[s] + in_len[s];
    if (ie > in_total) in_total = ie;
    slots += sp.count;
    d_off[r] = out_total;
    out_total += ((uint64_t)len[r] + 15) / 16 * 16;
  }
  if (slots > 0x7fffffffull) return SM_ERR_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  SM_CHECK(ctx->io_meta.ensure(carve_range_host(0, n, entries, k).end));
  const RangeHostArrays a = carve_range_host((uintptr_t)ctx->io_meta.p, n, entries, k);
  SM_CHECK(ctx->io_in.ensure(in_total + 16));
  SM_CHECK(ctx->io_out.ensure((size_t)out_total + 16));
  for (size_t i = 0; i < n; ++i) {
    if (!named[i]) continue;
    if (in_len[i])
      SM_CHECK(hipMemcpyAsync((uint8_t*)ctx->io_in.p + in_off[i], in + in_off[i], in_len[i], hipMemcpyHostToDevice, s));
    const uint32_t e0 = frag_first[i], e1 = frag_first[i + 1];  // (in order and inside frag_pos: the rule passed)
    if (e1 > e0) SM_CHECK(hipMemcpyAsync(a.pos + e0, frag_pos + e0, 4 * (size_t)(e1 - e0), hipMemcpyHostToDevice, s));
  }
  SM_CHECK(hipMemcpyAsync(a.in_off, in_off, 8 * n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.in_len, in_len, 4 * n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.first, frag_first, 4 * (n + 1), hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.out_off, d_off.data(), 8 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.range_stream, d_stream.data(), 4 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.lo, lo, 4 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(a.len, len, 4 * k, hipMemcpyHostToDevice, s));
  SM_PASS(smm_uncompress_ranges_device(ctx, (const uint8_t*)ctx->io_in.p, a.in_off, a.in_len, nstreams, a.first, a.pos,
                                       (uint32_t)entries, a.range_stream, a.lo, a.len, nranges, (uint32_t)slots,
                                       (uint8_t*)ctx->io_out.p, a.out_off, a.out_len, a.status, s));
  SM_CHECK(hipMemcpyAsync(out_len, a.out_len, 4 * k, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipMemcpyAsync(status, a.status, 4 * k, hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));  // (also lets the pageable uploads above leave d_off and d_stream)
  for (size_t r = 0; r < k; ++r) {
    if (status[r] != SM_OK || out_len[r] == 0) continue;
    if (out_len[r] != len[r] || d_off[r] + len[r] > out_total) return SM_ERR_DEVICE;  // (never: the device's own rule)
    SM_CHECK(hipMemcpyAsync(out + out_off[r], (const uint8_t*)ctx->io_out.p + d_off[r], len[r], hipMemcpyDeviceToHost, s));
  }
  SM_CHECK(hipStreamSynchronize(s));
  return SM_OK;
}

}  // extern "C"
