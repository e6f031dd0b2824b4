// sma_api.hip -- C ABI of the Avro container library (include/snappy_mi355x_avro.h) over the multi
// library's and the Parquet library's public device calls (libsnappy_mi355x_multi.so and
// libsnappy_mi355x_parquet.so, linked by name) and the kernels of sma_kernels.hip.  The host-only
// entry points live in sma_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../../include/snappy_mi355x_multi.h"
#include "../../../include/snappy_mi355x_parquet.h"
#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "sma_format.h"
#include "sma_internal.h"

#ifndef SMA_VERSION_STR
#define SMA_VERSION_STR "dev"
#endif

struct sma_ctx {
  smm_ctx* smm = nullptr;
  smq_ctx* smq = nullptr;  // the batched CRC-32
  int device = 0;
  hipStream_t stream = nullptr;  // the host-buffer calls run on it
  DevBuf meta;                   // a *_device call's per-slot and per-stream arrays, the encoder's stage
  DevBuf io_in, io_out, sarg;    // the host-buffer calls' staging and their own arrays
  std::mutex mu;                 // serialises the host-buffer entry points
};

extern "C" {

const char* sma_status_message(sm_status st) {
  const char* m = sma::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* sma_version(void) { return "snappy_mi355x_avro gfx950 " SMA_VERSION_STR; }

sma_ctx* sma_ctx_create(int device) {
  sma_ctx* ctx = new (std::nothrow) sma_ctx();
  if (!ctx) return nullptr;
  ctx->device = device;
  ctx->smm = smm_ctx_create(device);
  ctx->smq = ctx->smm ? smq_ctx_create(device) : nullptr;
  bool ok = ctx->smm && ctx->smq;
  if (ok) {
    DeviceGuard g(device);
    ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) ctx->stream = nullptr;
  }
  if (!ok) {
    sma_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void sma_ctx_destroy(sma_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->meta, &ctx->io_in, &ctx->io_out, &ctx->sarg}) b->release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  }
  if (ctx->smq) smq_ctx_destroy(ctx->smq);
  if (ctx->smm) smm_ctx_destroy(ctx->smm);
  delete ctx;
}

int sma_ctx_last_indexed(sma_ctx* ctx) { return ctx ? smm_ctx_last_indexed(ctx->smm) : -1; }

// Launch sequence: the counting walk, the scan, the storing walk; the multi library's index builder
// and its decoder, once each over all slots; with verify_crc the Parquet library's CRC-32 once over
// the slots' output ranges; the slots' verdicts, the streams' results.
sm_status sma_uncompress_streams_device(sma_ctx* ctx, int kind, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, const uint8_t* d_sync, uint32_t nstreams,
                                        uint32_t max_blocks, uint32_t max_fragments, int verify_crc, uint8_t* d_out,
                                        const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                        int32_t* d_status, uint64_t* d_objects, uint32_t* d_block_first,
                                        const sma_blocks* d_blocks, int32_t* d_block_status, void* stream) {
  if (!ctx || !sma::valid_kind(kind) || nstreams > sma::kMaxStreams || max_blocks > sma::kMaxStreams) return SM_ERR_ARGUMENT;
  if (!d_block_first != !d_block_status) return SM_ERR_ARGUMENT;
  if (d_blocks && !sma::valid_blocks(*d_blocks)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  if (kind == SMA_INPUT_BLOCKS && !d_sync) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_blocks;
  SM_CHECK(ctx->meta.ensure(sma::decode_streams_bytes(nstreams, m, max_fragments)));
  const sma::DecodeStreamsArgs a{kind,      d_in,      d_in_off,  d_in_len, d_sync,    nstreams,      m,
                                 verify_crc ? 1u : 0u, d_out_off, d_out_cap, d_out_len, d_status,     d_objects,
                                 d_block_first, d_block_status, d_blocks != nullptr, d_blocks ? *d_blocks : sma_blocks{},
                                 sma::carve_decode_streams((uint8_t*)ctx->meta.p, nstreams, m, max_fragments)};
  SM_CHECK(sma::launch_decode_plan(a, s));
  if (m) {
    // the index of every slot that a block compressor wrote (over max_fragments: the empty index),
    // then the decode, by fragments where the index allows.  With no fragments allowed the index
    // would be the empty one, which decodes as no index does: it is not built.
    const bool index = max_fragments != 0;
    if (index)
      SM_PASS(smm_index_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.cap, a.s.frag_first,
                               a.s.frag_pos, a.s.built, a.s.index_status, stream));
    SM_PASS(smm_uncompress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, d_out, a.s.out_off, a.s.cap,
                                  a.s.out_len, a.s.dec_status, index ? a.s.frag_first : nullptr,
                                  index ? a.s.frag_pos : nullptr, stream));
    // the checksum of what was decoded: every slot's output range lies inside its stream's room
    if (verify_crc) SM_PASS(smq_crc32_device(ctx->smq, d_out, a.s.out_off, a.s.crc_len, m, a.s.computed, stream));
  }
  SM_CHECK(sma::launch_decode_result(a, s));
  return SM_OK;
}

sm_status sma_find_sync_device(sma_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                               const uint8_t* d_sync, uint32_t nstreams, const uint32_t* d_q_stream,
                               const uint64_t* d_q_from, uint32_t nqueries, uint64_t* d_pos, void* stream) {
  if (!ctx || nstreams > sma::kMaxStreams || nqueries > sma::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nqueries == 0) return SM_OK;
  if (nstreams == 0 || !d_in || !d_in_off || !d_in_len || !d_sync || !d_q_stream || !d_q_from || !d_pos) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(sma::launch_find_sync(sma::FindSyncArgs{d_in, d_in_off, d_in_len, d_sync, d_q_stream, d_q_from, nqueries, d_pos},
                                 (hipStream_t)stream));
  return SM_OK;
}

// Launch sequence: the blocks against the bounds with the scan of the stage, the slots; the multi
// library's compressor once over all blocks into the stage; the Parquet library's CRC-32 once over
// the input blocks; the scan of the block sizes, the pack, the streams' headers and results.
sm_status sma_compress_streams_device(sma_ctx* ctx, const uint8_t* d_in, const uint32_t* d_block_first,
                                      const uint64_t* d_block_off, const uint32_t* d_block_len,
                                      const uint64_t* d_block_count, const uint8_t* d_sync, const uint64_t* d_head_off,
                                      const uint64_t* d_head_len, uint32_t nstreams, uint32_t max_blocks,
                                      uint64_t stage_bytes, uint32_t max_fragments, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream) {
  if (!ctx || nstreams > sma::kMaxStreams || max_blocks > sma::kMaxStreams || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (!d_head_off != !d_head_len) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_block_first || !d_sync || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  if (max_blocks && (!d_block_off || !d_block_len || !d_block_count)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_blocks;
  // (spare bytes behind the stage: the unused slots' empty raw streams all go there)
  const size_t stage = (size_t)stage_bytes + 64;
  SM_CHECK(ctx->meta.ensure(sma::compress_streams_bytes(nstreams, m, stage)));
  const sma::CompressStreamsArgs a{d_in,       d_block_first, d_block_off, d_block_len,  d_block_count, d_sync,
                                   d_head_off, d_head_len,    nstreams,    m,            stage_bytes,   max_fragments,
                                   d_out,      d_out_off,     d_out_len,   d_status,
                                   sma::carve_compress_streams((uint8_t*)ctx->meta.p, nstreams, m, stage)};
  SM_CHECK(sma::launch_compress_plan(a, s));
  if (m) {
    SM_PASS(smm_compress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.stage, a.s.slot_off,
                                a.s.comp_len, a.s.comp_status, nullptr, nullptr, mode, stream));
    SM_PASS(smq_crc32_device(ctx->smq, d_in, a.s.in_off, a.s.crc_len, m, a.s.crc, stream));
  }
  SM_CHECK(sma::launch_compress_pack(a, s));
  return SM_OK;
}

}  // extern "C"

// ---- host buffers (../common/smc_staging.h) ------------------------------------------------------
using smc::round16;

extern "C" {

// The streams' bytes packed behind one another in one staging block (one upload), and room for
// every stream's output at a 16-byte boundary of the device buffer (one download; each stream's
// own bytes then go to the caller's place); the objects come back beside the lengths.
sm_status sma_uncompress_streams(sma_ctx* ctx, int kind, const uint8_t* in, const uint64_t* in_off,
                                 const uint64_t* in_len, const uint8_t* sync, uint32_t nstreams, int verify_crc,
                                 uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                 int32_t* status, uint64_t* objects) {
  if (!ctx || !sma::valid_kind(kind) || nstreams > sma::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  if (kind == SMA_INPUT_BLOCKS && !sync) return SM_ERR_ARGUMENT;
  // the plan on the host: the two bounds, and the room each decoded stream needs on the device
  std::vector<uint64_t> room(nstreams);
  uint64_t blocks = 0, fragments = 0;
  const sm_status planned = sma_streams_plan(in, in_off, in_len, nstreams, kind, sync, out_cap, sma::kMaxStreams, nullptr,
                                             room.data(), status, nullptr, &blocks, &fragments);
  if (planned != SM_OK) return planned == SM_BUFFER_TOO_SMALL ? (sm_status)SM_ERR_INPUT_TOO_LARGE : planned;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status[r] != SM_OK) room[r] = 0;  // (not decoded)
    if (room[r] && !out) return SM_ERR_ARGUMENT;
  }
  if (fragments > sma::kMaxStreams) fragments = 0;  // (a hint: such a batch decodes in stream order)
  const StreamStaging h(in, in_off, in_len, nstreams, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t n = nstreams;
  SM_PASS(ensure_staging(b, h.bytes.size(), (size_t)h.out_total, 6 * round16(8 * n) + round16(4 * n) + round16(16 * n)));
  ArgUpload up{smc::Carve{(uintptr_t)ctx->sarg.p}, s};
  hipError_t e = hipSuccess;
  if (!h.bytes.empty()) e = hipMemcpyAsync(ctx->io_in.p, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice, s);
  const uint64_t* const d_in_off = up.put(h.in_off.data(), n, e);
  const uint64_t* const d_in_len = up.put(in_len, n, e);
  const uint64_t* const d_out_off = up.put(h.out_off.data(), n, e);
  const uint64_t* const d_out_cap = up.put(out_cap, n, e);
  uint64_t* const d_out_len = up.put((const uint64_t*)nullptr, n, e);
  uint64_t* const d_objects = up.put((const uint64_t*)nullptr, n, e);
  int32_t* const d_status = up.put((const int32_t*)nullptr, n, e);
  const uint8_t* const d_sync = up.put(sync, sync ? 16 * n : 1, e);
  SM_CHECK(e);
  SM_PASS(sma_uncompress_streams_device(ctx, kind, (const uint8_t*)ctx->io_in.p, d_in_off, d_in_len, d_sync, nstreams,
                                        (uint32_t)blocks, (uint32_t)fragments, verify_crc, (uint8_t*)ctx->io_out.p, d_out_off,
                                        d_out_cap, d_out_len, d_status, d_objects, nullptr, nullptr, nullptr, s));
  std::vector<uint8_t> decoded;
  SM_PASS(download_results(b, d_out_len, d_status, n, out_len, status));
  if (objects) SM_CHECK(hipMemcpyAsync(objects, d_objects, 8 * n, hipMemcpyDeviceToHost, s));
  SM_PASS(download_output(b, h.out_total, decoded));
  for (uint32_t r = 0; r < nstreams; ++r)
    if (room[r]) memcpy(out + out_off[r], decoded.data() + h.out_off[r], (size_t)room[r]);
  return SM_OK;
}

// The encoder's twin: every header and every block packed behind one another (a block at a 16-byte
// boundary), the three bounds counted here, and per stream the room the bound promises.
sm_status sma_compress_streams(sma_ctx* ctx, const uint8_t* in, const uint32_t* block_first, const uint64_t* block_off,
                               const uint32_t* block_len, const uint64_t* block_count, const uint8_t* sync,
                               const uint64_t* head_off, const uint64_t* head_len, uint32_t nstreams, uint8_t* out,
                               const uint64_t* out_off, uint64_t* out_len, int32_t* status, int mode) {
  if (!ctx || nstreams > sma::kMaxStreams || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (!head_off != !head_len) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!block_first || !sync || !out || !out_off || !out_len || !status) return SM_ERR_ARGUMENT;
  const uint32_t m = block_first[nstreams];
  if (m > sma::kMaxStreams || (m && (!in || !block_off || !block_len || !block_count))) return SM_ERR_ARGUMENT;
  for (uint32_t r = 0; r < nstreams; ++r)
    if (block_first[r] > block_first[r + 1] || (head_len && head_len[r] && !in)) return SM_ERR_ARGUMENT;
  if (block_first[0] != 0) return SM_ERR_ARGUMENT;
  std::vector<uint64_t> h_block_off(m), h_head_off(nstreams), h_out_off(nstreams), room(nstreams);
  uint64_t in_total = 0, out_total = 0, stage = 0, fragments = 0;
  for (uint32_t r = 0; r < nstreams; ++r) {
    h_head_off[r] = in_total;
    room[r] = head_len ? head_len[r] : 0;
    in_total += room[r];
    for (uint32_t j = block_first[r]; j < block_first[r + 1]; ++j) {
      in_total = round16(in_total);
      h_block_off[j] = in_total;
      in_total += block_len[j];
      room[r] += sma::max_block_length(block_len[j]);
      stage += sma::stage_length(block_len[j]);
      fragments += sma::encode_fragments(block_len[j]);
    }
    h_out_off[r] = out_total;
    out_total += round16(room[r]);
  }
  if (fragments > sma::kMaxStreams) return SM_ERR_INPUT_TOO_LARGE;
  std::vector<uint8_t> bytes((size_t)in_total);
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (head_len && head_len[r]) memcpy(bytes.data() + h_head_off[r], in + head_off[r], (size_t)head_len[r]);
    for (uint32_t j = block_first[r]; j < block_first[r + 1]; ++j)
      if (block_len[j]) memcpy(bytes.data() + h_block_off[j], in + block_off[j], block_len[j]);
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t n = nstreams;
  SM_PASS(ensure_staging(b, bytes.size(), (size_t)out_total,
                         4 * round16(8 * n) + 2 * round16(4 * (n + 1)) + round16(16 * n) + 2 * round16(8 * (size_t)m) +
                             round16(4 * (size_t)m)));
  ArgUpload up{smc::Carve{(uintptr_t)ctx->sarg.p}, s};
  hipError_t e = hipSuccess;
  if (!bytes.empty()) e = hipMemcpyAsync(ctx->io_in.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s);
  const uint32_t* const d_first = up.put(block_first, n + 1, e);
  const uint64_t* const d_block_off = up.put(h_block_off.data(), m, e);
  const uint32_t* const d_block_len = up.put(block_len, m, e);
  const uint64_t* const d_block_count = up.put(block_count, m, e);
  const uint8_t* const d_sync = up.put(sync, 16 * n, e);
  const uint64_t* const d_head_off = up.put(h_head_off.data(), n, e);
  const uint64_t* const d_head_len = up.put(head_len, n, e);
  const uint64_t* const d_out_off = up.put(h_out_off.data(), n, e);
  uint64_t* const d_out_len = up.put((const uint64_t*)nullptr, n, e);
  int32_t* const d_status = up.put((const int32_t*)nullptr, n, e);
  SM_CHECK(e);
  SM_PASS(sma_compress_streams_device(ctx, (const uint8_t*)ctx->io_in.p, d_first, d_block_off, d_block_len, d_block_count, d_sync,
                                      head_len ? d_head_off : nullptr, head_len ? d_head_len : nullptr, nstreams, m, stage,
                                      (uint32_t)fragments, (uint8_t*)ctx->io_out.p, d_out_off, d_out_len, d_status, mode, s));
  std::vector<uint8_t> packed;
  SM_PASS(download_results(b, d_out_len, d_status, n, out_len, status));
  SM_PASS(download_output(b, out_total, packed));
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (out_len[r] > room[r]) return SM_ERR_DEVICE;
    if (status[r] == SM_OK && out_len[r]) memcpy(out + out_off[r], packed.data() + h_out_off[r], (size_t)out_len[r]);
  }
  return SM_OK;
}

}  // extern "C"
