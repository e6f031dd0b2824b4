// smm_api.hip -- C ABI of the multi-stream library (include/snappy_mi355x_multi.h) over the raw
// codec's public batched device calls (libsnappy_mi355x.so, linked by name) and the kernels of
// smm_kernels.hip and smm_index.hip.  The host-only entry points live in smm_host.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../common/smc_hip_host.h"
#include "smm_plan.h"

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
  DevBuf meta, slots;            // the per-call arrays; compress: the fragments' output slots
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

}  // extern "C"
