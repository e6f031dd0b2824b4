// smq_api.hip -- C ABI of the Parquet page library (include/snappy_mi355x_parquet.h) over the multi
// library's public device calls (libsnappy_mi355x_multi.so, linked by name) and the kernels of
// smq_kernels.hip and smq_crc.hip.  The host-only entry points live in smq_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../../include/snappy_mi355x_multi.h"
#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "smq_chunks.h"
#include "smq_crc.h"
#include "smq_encode.h"
#include "smq_format.h"
#include "smq_internal.h"

#ifndef SMQ_VERSION_STR
#define SMQ_VERSION_STR "dev"
#endif

struct smq_ctx {
  smm_ctx* smm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;  // the host-buffer call runs on it
  DevBuf lut;                    // the CRC tables (smq::CrcLut)
  DevBuf meta;                   // a *_device call's per-slot and per-chunk arrays
  DevBuf io_in, io_out, sarg;    // the host-buffer call's staging and its own arrays
  std::mutex mu;                 // serialises the host-buffer entry point
};

extern "C" {

const char* smq_status_message(sm_status st) {
  const char* m = smq::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* smq_version(void) { return "snappy_mi355x_parquet gfx950 " SMQ_VERSION_STR; }

smq_ctx* smq_ctx_create(int device) {
  smm_ctx* smm = smm_ctx_create(device);
  if (!smm) return nullptr;
  smq_ctx* ctx = new (std::nothrow) smq_ctx();
  if (!ctx) {
    smm_ctx_destroy(smm);
    return nullptr;
  }
  ctx->smm = smm;
  ctx->device = device;
  bool ok;
  {
    DeviceGuard g(device);
    ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) ctx->stream = nullptr;
    std::unique_ptr<smq::CrcLut> lut(new (std::nothrow) smq::CrcLut);
    ok = ok && lut && ctx->lut.ensure(sizeof(smq::CrcLut)) == hipSuccess;
    if (ok) {
      smq::build_crc_lut(lut.get());
      ok = hipMemcpy(ctx->lut.p, lut.get(), sizeof(smq::CrcLut), hipMemcpyHostToDevice) == hipSuccess;
    }
  }
  if (!ok) {
    smq_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smq_ctx_destroy(smq_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->lut, &ctx->meta, &ctx->io_in, &ctx->io_out, &ctx->sarg}) b->release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  }
  smm_ctx_destroy(ctx->smm);
  delete ctx;
}

int smq_ctx_last_indexed(smq_ctx* ctx) { return ctx ? smm_ctx_last_indexed(ctx->smm) : -1; }

// Launch sequence: the counting walk, the scan, the storing walk (and the scan of the CRC
// segments); the multi library's index builder and its decoder, once each over all slots (a slot
// without a compressed section is an empty one to them); the copies, the CRC segments, the slots'
// verdicts, the chunks' results.
sm_status smq_uncompress_chunks_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t nchunks, uint32_t max_pages, uint32_t max_fragments, int verify_crc,
                                       uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, uint32_t* d_page_first,
                                       const smq_pages* d_pages, int32_t* d_page_status, void* stream) {
  if (!ctx || nchunks > smq::kMaxChunks || max_pages > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (!d_page_first != !d_page_status) return SM_ERR_ARGUMENT;
  if (d_pages && !smq::valid_pages(*d_pages)) return SM_ERR_ARGUMENT;
  if (nchunks == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_pages;
  SM_CHECK(ctx->meta.ensure(smq::decode_chunks_bytes(nchunks, m, max_fragments)));
  const smq::DecodeChunksArgs a{d_in,      d_in_off,  d_in_len,  nchunks,  m,            verify_crc ? 1u : 0u,
                                d_out,     d_out_off, d_out_cap, d_out_len, d_status,    d_page_first,
                                d_page_status, d_pages != nullptr, d_pages ? *d_pages : smq_pages{},
                                smq::carve_decode_chunks((uint8_t*)ctx->meta.p, nchunks, m, max_fragments)};
  SM_CHECK(smq::launch_decode_plan(a, s));
  if (m) {
    // the index of every compressed section that a block compressor wrote (over max_fragments: the
    // empty index), then the decode, by fragments where the index allows.  With no fragments allowed
    // the index would be the empty one, which decodes as no index does: it is not built.
    const bool index = max_fragments != 0;
    if (index)
      SM_PASS(smm_index_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.cap, a.s.frag_first, a.s.frag_pos,
                               a.s.built, a.s.index_status, stream));
    SM_PASS(smm_uncompress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, d_out, a.s.out_off, a.s.cap,
                                  a.s.out_len, a.s.dec_status, index ? a.s.frag_first : nullptr,
                                  index ? a.s.frag_pos : nullptr, stream));
  }
  SM_CHECK(smq::launch_decode_result(a, (const smq::CrcLut*)ctx->lut.p, s));
  return SM_OK;
}

sm_status smq_crc32_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_off, const uint64_t* d_len, uint32_t n,
                           uint32_t* d_crc, void* stream) {
  if (!ctx || n > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (n == 0) return SM_OK;
  if (!d_in || !d_off || !d_len || !d_crc) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(ctx->meta.ensure(smq::crc_ranges_bytes(n)));
  SM_CHECK(smq::launch_crc_ranges(d_in, d_off, d_len, n, d_crc, smq::carve_crc_ranges((uint8_t*)ctx->meta.p, n),
                                  (const smq::CrcLut*)ctx->lut.p, (hipStream_t)stream));
  return SM_OK;
}

// ---- the page encoder (include/snappy_mi355x_parquet_write.h) ----------------------------------------
// Launch sequence: the counting walk, the scan, the storing walk, the scan of the stage slots and
// the fragments; the multi library's compressor once over all slots (a slot without a section is an
// empty stream to it); the level bytes, the bodies' lengths and statuses, the CRC segments, the sizes
// with the chunks' results, the pack.
sm_status smqe_compress_chunks_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                      uint32_t nchunks, uint32_t max_pages, uint64_t stage_bytes, uint32_t max_fragments,
                                      uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                      int32_t* d_status, uint32_t* d_page_first, const smq_pages* d_pages,
                                      int32_t* d_page_status, int mode, void* stream) {
  if (!ctx || nchunks > smq::kMaxChunks || max_pages > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (mode != SM_MODE_REFERENCE && mode != SM_MODE_FAST && mode != SM_MODE_FAST_DENSE) return SM_ERR_ARGUMENT;
  if (!d_page_first != !d_page_status) return SM_ERR_ARGUMENT;
  if (d_pages && !smq::valid_pages(*d_pages)) return SM_ERR_ARGUMENT;
  if (nchunks == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_pages;
  SM_CHECK(ctx->meta.ensure(smq::encode_chunks_bytes(nchunks, m, (size_t)stage_bytes)));
  const smq::EncodeChunksArgs a{d_in,     d_in_off,     d_in_len,      nchunks,            m,
                                stage_bytes, max_fragments, d_out,      d_out_off,          d_out_cap,
                                d_out_len, d_status,     d_page_first,  d_page_status,      d_pages != nullptr,
                                d_pages ? *d_pages : smq_pages{},
                                smq::carve_encode_chunks((uint8_t*)ctx->meta.p, nchunks, m, (size_t)stage_bytes)};
  SM_CHECK(smq::launch_encode_plan(a, s));
  if (m)
    SM_PASS(smm_compress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.stage, a.s.comp_off, a.s.comp_len,
                                a.s.comp_status, nullptr, nullptr, mode, stream));
  SM_CHECK(smq::launch_encode_result(a, (const smq::CrcLut*)ctx->lut.p, s));
  return SM_OK;
}

// ---- host buffers --------------------------------------------------------------------------------
// The chunks' bytes packed behind one another in one staging block (one upload), and room for every
// chunk's output at a 16-byte boundary of the device buffer (one download; each chunk's own bytes
// then go to the caller's place): ../common/smc_staging.h.
sm_status smq_uncompress_chunks(smq_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t nchunks, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status) {
  if (!ctx || nchunks > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (nchunks == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  // the plan on the host: the two bounds, and the room each decoded chunk needs on the device
  std::vector<uint64_t> room(nchunks);
  uint64_t pages = 0, fragments = 0;
  const sm_status planned =
      smq_chunks_plan(in, in_off, in_len, nchunks, out_cap, smq::kMaxChunks, nullptr, room.data(), status, &pages, &fragments);
  if (planned != SM_OK) return planned == SM_BUFFER_TOO_SMALL ? (sm_status)SM_ERR_INPUT_TOO_LARGE : planned;
  for (uint32_t r = 0; r < nchunks; ++r) {
    if (status[r] != SM_OK) room[r] = 0;  // (not decoded)
    if (room[r] && !out) return SM_ERR_ARGUMENT;
  }
  if (fragments > smq::kMaxChunks) fragments = 0;  // (a hint: such a batch decodes in stream order)
  const StreamStaging h(in, in_off, in_len, nchunks, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, out_cap, nchunks, d));
  SM_PASS(smq_uncompress_chunks_device(ctx, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nchunks, (uint32_t)pages,
                                       (uint32_t)fragments, verify_crc, (uint8_t*)ctx->io_out.p, d.out_off, d.out_cap, d.out_len,
                                       d.status, nullptr, nullptr, nullptr, ctx->stream));
  std::vector<uint8_t> decoded;
  SM_PASS(download_stream_call(b, h, d, nchunks, out_len, status, decoded));
  for (uint32_t r = 0; r < nchunks; ++r)
    if (room[r]) memcpy(out + out_off[r], decoded.data() + h.out_off[r], (size_t)room[r]);
  return SM_OK;
}

// The encoder's twin: the plan on the host gives the three bounds and, per chunk, room that always
// suffices -- the smaller of the caller's room and the plan's bound.
sm_status smqe_compress_chunks(smq_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                               uint32_t nchunks, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                               uint64_t* out_len, int32_t* status, int mode) {
  if (!ctx || nchunks > smq::kMaxChunks) return SM_ERR_ARGUMENT;
  if (nchunks == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  std::vector<uint64_t> room(nchunks);
  uint64_t pages = 0, stage = 0, fragments = 0;
  const sm_status planned =
      smqe_chunks_plan(in, in_off, in_len, nchunks, smq::kMaxChunks, nullptr, status, room.data(), &pages, &stage, &fragments);
  if (planned != SM_OK) return planned == SM_BUFFER_TOO_SMALL ? (sm_status)SM_ERR_INPUT_TOO_LARGE : planned;
  if (fragments > smq::kMaxChunks) return SM_ERR_INPUT_TOO_LARGE;
  for (uint32_t r = 0; r < nchunks; ++r) {
    room[r] = std::min(room[r], out_cap[r]);
    if (room[r] && !out) return SM_ERR_ARGUMENT;
  }
  const StreamStaging h(in, in_off, in_len, nchunks, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, out_cap, nchunks, d));
  SM_PASS(smqe_compress_chunks_device(ctx, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nchunks, (uint32_t)pages, stage,
                                      (uint32_t)fragments, (uint8_t*)ctx->io_out.p, d.out_off, d.out_cap, d.out_len, d.status,
                                      nullptr, nullptr, nullptr, mode, ctx->stream));
  std::vector<uint8_t> packed;
  SM_PASS(download_stream_call(b, h, d, nchunks, out_len, status, packed));
  for (uint32_t r = 0; r < nchunks; ++r)
    if (status[r] == SM_OK && out_len[r]) memcpy(out + out_off[r], packed.data() + h.out_off[r], (size_t)out_len[r]);
  return SM_OK;
}

}  // extern "C"
