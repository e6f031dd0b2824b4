// smk_api.hip -- C ABI of the Kafka segment library (include/snappy_mi355x_kafka.h) over the blocks,
// multi and framing libraries' public device calls (libsnappy_mi355x_blocks.so,
// libsnappy_mi355x_multi.so and libsnappy_mi355x_framing.so, linked by name) and the kernels of
// smk_kernels.hip.  The host-only entry points live in smk_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../../include/snappy_mi355x_blocks.h"
#include "../../../include/snappy_mi355x_framing.h"
#include "../../../include/snappy_mi355x_multi.h"
#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "smk_format.h"
#include "smk_internal.h"

#ifndef SMK_VERSION_STR
#define SMK_VERSION_STR "dev"
#endif

struct smk_ctx {
  smb_ctx* smb = nullptr;  // the snappy-java streams, both ways
  smm_ctx* smm = nullptr;  // the raw batches
  smf_ctx* smf = nullptr;  // the batched CRC-32C
  int device = 0;
  bool decoded = false;          // a decode call has run (smk_ctx_last_indexed)
  hipStream_t stream = nullptr;  // the host-buffer calls run on it
  DevBuf meta;                   // a *_device call's arrays, the encoder's stage
  DevBuf io_in, io_out, sarg;    // the host-buffer calls' staging and their own arrays
  std::mutex mu;                 // serialises the host-buffer entry points
};

extern "C" {

const char* smk_status_message(sm_status st) {
  const char* m = smk::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* smk_version(void) { return "snappy_mi355x_kafka gfx950 " SMK_VERSION_STR; }

smk_ctx* smk_ctx_create(int device) {
  smk_ctx* ctx = new (std::nothrow) smk_ctx();
  if (!ctx) return nullptr;
  ctx->device = device;
  ctx->smb = smb_ctx_create(device);
  ctx->smm = ctx->smb ? smm_ctx_create(device) : nullptr;
  ctx->smf = ctx->smm ? smf_ctx_create(device) : nullptr;
  bool ok = ctx->smb && ctx->smm && ctx->smf;
  if (ok) {
    DeviceGuard g(device);
    ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) ctx->stream = nullptr;
  }
  if (!ok) {
    smk_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smk_ctx_destroy(smk_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->meta, &ctx->io_in, &ctx->io_out, &ctx->sarg}) b->release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  }
  if (ctx->smf) smf_ctx_destroy(ctx->smf);
  if (ctx->smm) smm_ctx_destroy(ctx->smm);
  if (ctx->smb) smb_ctx_destroy(ctx->smb);
  delete ctx;
}

int smk_ctx_last_indexed(smk_ctx* ctx) {
  if (!ctx || !ctx->decoded) return -1;
  const int x = smb_ctx_last_indexed(ctx->smb), r = smm_ctx_last_indexed(ctx->smm);
  return (x > 0 ? x : 0) + (r > 0 ? r : 0);
}

// Launch sequence: the counting walk, the scan, the storing walk; the heads; the blocks library's
// decoder over the snappy-java batches with no room (their sizes); the scan of the rewritten
// lengths, the segments' plans, the slots; that decoder again, with room; the gate; the multi
// library's index builder and decoder over the raw batches; the stored batches' copy, the headers;
// the framing library's CRC-32C over the stored bytes (verify_crc) and over the rewritten ones, the
// store of the latter; the verdicts, the results.
sm_status smk_uncompress_segments_device(smk_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                         uint32_t nsegments, uint32_t max_batches, uint32_t max_chunks, uint32_t max_fragments,
                                         int verify_crc, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                         uint64_t* d_out_len, int32_t* d_status, uint32_t* d_batch_first,
                                         uint64_t* d_batch_in_off, uint64_t* d_batch_out_off, uint64_t* d_batch_len,
                                         uint32_t* d_batch_codec, int32_t* d_batch_status, void* stream) {
  if (!ctx || nsegments > smk::kMaxCount || max_batches > smk::kMaxCount || max_chunks > smk::kMaxCount) return SM_ERR_ARGUMENT;
  if (nsegments == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_batches;
  SM_CHECK(ctx->meta.ensure(smk::decode_bytes(nsegments, m, max_fragments)));
  smk::DecodeArgs a{};
  a.s = smk::carve_decode((uint8_t*)ctx->meta.p, nsegments, m, max_fragments);
  a.w = smk::WalkArgs{d_in, d_in_off, d_in_len, nsegments, m, a.s.hdr, a.s.g, a.s.b, d_batch_first};
  a.verify = verify_crc ? 1u : 0u;
  a.out = d_out;
  a.out_off = d_out_off;
  a.out_cap = d_out_cap;
  a.out_len = d_out_len;
  a.status = d_status;
  a.batch_in_off = d_batch_in_off;
  a.batch_out_off = d_batch_out_off;
  a.batch_len = d_batch_len;
  a.batch_codec = d_batch_codec;
  a.batch_status = d_batch_status;
  ctx->decoded = true;
  SM_CHECK(smk::launch_walk(a.w, s));
  SM_CHECK(smk::launch_heads(a, s));
  if (m)
    SM_PASS(smb_uncompress_streams_device(ctx->smb, SMB_FORMAT_XERIAL, d_in, a.s.x_in_off, a.s.x_in_len, m, max_chunks, 0, d_out,
                                          a.s.x_out_off, a.s.x_cap, a.s.x_len, a.s.x_status, nullptr, nullptr, stream));
  SM_CHECK(smk::launch_decode_plan(a, s));
  if (m) {
    SM_PASS(smb_uncompress_streams_device(ctx->smb, SMB_FORMAT_XERIAL, d_in, a.s.x_in_off, a.s.x_in_len, m, max_chunks,
                                          max_fragments, d_out, a.s.x_out_off, a.s.x_cap, a.s.x_len, a.s.x_status, nullptr, nullptr,
                                          stream));
    SM_CHECK(smk::launch_gate(a, s));
    const bool index = max_fragments != 0;
    if (index)
      SM_PASS(smm_index_device(ctx->smm, d_in, a.s.r_in_off, a.s.r_in_len, m, max_fragments, a.s.r_cap, a.s.frag_first,
                               a.s.frag_pos, a.s.built, a.s.r_index_status, stream));
    SM_PASS(smm_uncompress_device(ctx->smm, d_in, a.s.r_in_off, a.s.r_in_len, m, max_fragments, d_out, a.s.r_out_off, a.s.r_cap,
                                  a.s.r_out_len, a.s.r_status, index ? a.s.frag_first : nullptr, index ? a.s.frag_pos : nullptr,
                                  stream));
    SM_CHECK(smk::launch_decode_pack(a, s));
    if (a.verify) SM_PASS(smf_crc32c_batch_device(ctx->smf, d_in, a.s.ci_off, a.s.ci_len, m, a.s.computed, 0, stream));
    SM_PASS(smf_crc32c_batch_device(ctx->smf, d_out, a.s.co_off, a.s.co_len, m, a.s.crc, 0, stream));
    SM_CHECK(smk::launch_crc_store(d_out, a.s.co_off, a.s.co_len, a.s.crc, m, s));
  }
  SM_CHECK(smk::launch_decode_result(a, s));
  return SM_OK;
}

// Launch sequence: the walks; the payloads against the bounds with the scan of the stage, the
// streams; the blocks library's encoder once over all payloads into the stage; the scan of the
// sizes, the pack; the framing library's CRC-32C once over the packed ranges; the checksum bytes,
// the results.
sm_status smk_compress_segments_device(smk_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t nsegments, uint32_t max_batches, uint32_t max_blocks, uint64_t stage_bytes,
                                       uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status,
                                       int mode, void* stream) {
  if (!ctx || nsegments > smk::kMaxCount || max_batches > smk::kMaxCount || max_blocks > smk::kMaxCount || !valid_mode(mode))
    return SM_ERR_ARGUMENT;
  if (nsegments == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_batches;
  const size_t stage = (size_t)stage_bytes + 64;  // (spare bytes behind the stage: the unused slots' empty streams)
  SM_CHECK(ctx->meta.ensure(smk::compress_bytes(nsegments, m, stage)));
  smk::CompressArgs a{};
  a.s = smk::carve_compress((uint8_t*)ctx->meta.p, nsegments, m, stage);
  a.w = smk::WalkArgs{d_in, d_in_off, d_in_len, nsegments, m, a.s.hdr, a.s.g, a.s.b, nullptr};
  a.max_blocks = max_blocks;
  a.stage_bytes = stage_bytes;
  a.out = d_out;
  a.out_off = d_out_off;
  a.out_len = d_out_len;
  a.status = d_status;
  SM_CHECK(smk::launch_walk(a.w, s));
  SM_CHECK(smk::launch_compress_plan(a, s));
  if (m)
    SM_PASS(smb_compress_streams_device(ctx->smb, SMB_FORMAT_XERIAL, d_in, a.s.c_in_off, a.s.c_in_len, m, max_blocks, a.s.stage,
                                        a.s.slot_off, a.s.c_len, a.s.c_status, mode, stream));
  SM_CHECK(smk::launch_compress_pack(a, s));
  if (m) {
    SM_PASS(smf_crc32c_batch_device(ctx->smf, d_out, a.s.co_off, a.s.co_len, m, a.s.crc, 0, stream));
    SM_CHECK(smk::launch_crc_store(d_out, a.s.co_off, a.s.co_len, a.s.crc, m, s));
  }
  SM_CHECK(smk::launch_compress_result(a, s));
  return SM_OK;
}

}  // extern "C"

// ---- host buffers (../common/smc_staging.h) ------------------------------------------------------
using smc::round16;

extern "C" {

// The segments' bytes packed behind one another in one staging block (one upload), and room for
// every segment's output at a 16-byte boundary of the device buffer (one download; each segment's
// own bytes then go to the caller's place).  The bounds come from the host plan.
sm_status smk_uncompress_segments(smk_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                  uint32_t nsegments, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                  const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t* batch_first,
                                  uint32_t max_entries, uint64_t* batch_in_off, uint64_t* batch_out_off, uint64_t* batch_len,
                                  uint32_t* batch_codec, int32_t* batch_status) {
  if (!ctx || nsegments > smk::kMaxCount) return SM_ERR_ARGUMENT;
  if (nsegments == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  const bool entries = batch_first != nullptr;
  if (entries != (batch_in_off != nullptr) || entries != (batch_out_off != nullptr) || entries != (batch_len != nullptr) ||
      entries != (batch_codec != nullptr) || entries != (batch_status != nullptr))
    return SM_ERR_ARGUMENT;
  for (uint32_t t = 0; t < nsegments; ++t)
    if ((in_len[t] && !in) || (out_cap[t] && !out)) return SM_ERR_ARGUMENT;
  uint64_t batches = 0, chunks = 0, fragments = 0;
  SM_PASS(smk_segments_plan(in, in_off, in_len, nsegments, out_cap, smk::kMaxCount, smk::kMaxCount, nullptr, nullptr, nullptr,
                            &batches, &chunks, &fragments));
  if (batches > smk::kMaxCount || chunks > smk::kMaxCount) return SM_ERR_INPUT_TOO_LARGE;
  if (fragments > smk::kMaxCount) fragments = 0;
  const StreamStaging h(in, in_off, in_len, nsegments, out_cap);
  const uint32_t m = (uint32_t)batches;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t n = nsegments, e8 = round16(8 * (size_t)m + 8), e4 = round16(4 * (size_t)m + 4);
  SM_PASS(ensure_staging(b, h.bytes.size(), (size_t)h.out_total, 5 * round16(8 * n) + 2 * round16(4 * (n + 1)) + 3 * e8 + 2 * e4));
  ArgUpload up{smc::Carve{(uintptr_t)ctx->sarg.p}, s};
  hipError_t e = hipSuccess;
  if (!h.bytes.empty()) e = hipMemcpyAsync(ctx->io_in.p, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice, s);
  const uint64_t* const d_in_off = up.put(h.in_off.data(), n, e);
  const uint64_t* const d_in_len = up.put(in_len, n, e);
  const uint64_t* const d_out_off = up.put(h.out_off.data(), n, e);
  const uint64_t* const d_out_cap = up.put(out_cap, n, e);
  uint64_t* const d_out_len = up.put((const uint64_t*)nullptr, n, e);
  int32_t* const d_status = up.put((const int32_t*)nullptr, n, e);
  uint32_t* const d_first = up.put((const uint32_t*)nullptr, n + 1, e);
  uint64_t* const d_bin = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint64_t* const d_bout = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint64_t* const d_blen = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint32_t* const d_bcodec = up.put((const uint32_t*)nullptr, (size_t)m + 1, e);
  int32_t* const d_bstatus = up.put((const int32_t*)nullptr, (size_t)m + 1, e);
  SM_CHECK(e);
  SM_PASS(smk_uncompress_segments_device(ctx, (const uint8_t*)ctx->io_in.p, d_in_off, d_in_len, nsegments, m, (uint32_t)chunks,
                                         (uint32_t)fragments, verify_crc, (uint8_t*)ctx->io_out.p, d_out_off, d_out_cap, d_out_len,
                                         d_status, d_first, d_bin, d_bout, d_blen, d_bcodec, d_bstatus, s));
  std::vector<uint8_t> decoded;
  std::vector<uint32_t> first(n + 1);
  SM_PASS(download_results(b, d_out_len, d_status, n, out_len, status));
  SM_CHECK(hipMemcpyAsync(first.data(), d_first, 4 * (n + 1), hipMemcpyDeviceToHost, s));
  SM_PASS(download_output(b, h.out_total, decoded));
  for (uint32_t t = 0; t < nsegments; ++t)
    if (status[t] != SM_ERR_ARGUMENT && out_len[t] && out_len[t] <= out_cap[t])
      memcpy(out + out_off[t], decoded.data() + h.out_off[t], (size_t)out_len[t]);
  if (!entries) return SM_OK;
  const uint32_t total = first[n];
  if (total > m) return SM_ERR_DEVICE;
  if (total > max_entries) return SM_BUFFER_TOO_SMALL;
  memcpy(batch_first, first.data(), 4 * (n + 1));
  if (total) {
    SM_CHECK(hipMemcpyAsync(batch_in_off, d_bin, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(batch_out_off, d_bout, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(batch_len, d_blen, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(batch_codec, d_bcodec, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(batch_status, d_bstatus, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipStreamSynchronize(s));
  }
  return SM_OK;
}

// the encoder's twin: the three bounds and every segment's room from the host plan
sm_status smk_compress_segments(smk_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t nsegments, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                uint64_t* out_len, int32_t* status, int mode) {
  if (!ctx || nsegments > smk::kMaxCount || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nsegments == 0) return SM_OK;
  if (!in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  for (uint32_t t = 0; t < nsegments; ++t)
    if (in_len[t] && !in) return SM_ERR_ARGUMENT;
  std::vector<uint64_t> room(nsegments);
  uint64_t batches = 0, blocks = 0, stage = 0;
  SM_PASS(smk_compress_plan(in, in_off, in_len, nsegments, smk::kMaxCount, nullptr, room.data(), nullptr, &batches, &blocks, &stage));
  if (batches > smk::kMaxCount || blocks > smk::kMaxCount) return SM_ERR_INPUT_TOO_LARGE;
  for (uint32_t t = 0; t < nsegments; ++t)
    if (out_cap[t] < room[t]) return SM_ERR_ARGUMENT;
  const StreamStaging h(in, in_off, in_len, nsegments, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d{};
  SM_PASS(upload_stream_call(b, h, in_len, nullptr, nsegments, d));
  SM_PASS(smk_compress_segments_device(ctx, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nsegments, (uint32_t)batches,
                                       (uint32_t)blocks, stage, (uint8_t*)ctx->io_out.p, d.out_off, d.out_len, d.status, mode,
                                       ctx->stream));
  std::vector<uint8_t> packed;
  SM_PASS(download_stream_call(b, h, d, nsegments, out_len, status, packed));
  for (uint32_t t = 0; t < nsegments; ++t) {
    if (out_len[t] > room[t]) return SM_ERR_DEVICE;
    if (status[t] == SM_OK && out_len[t]) memcpy(out + out_off[t], packed.data() + h.out_off[t], (size_t)out_len[t]);
  }
  return SM_OK;
}

}  // extern "C"
