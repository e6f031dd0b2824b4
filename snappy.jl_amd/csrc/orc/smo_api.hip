// smo_api.hip -- C ABI of the ORC compression-stream format (include/snappy_mi355x_orc.h) over the
// multi library's public device calls (libsnappy_mi355x_multi.so, linked by name) and the kernels of
// smo_kernels.hip.  The host-only entry points live in smo_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../../include/snappy_mi355x_multi.h"
#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "smo_format.h"
#include "smo_internal.h"

#ifndef SMO_VERSION_STR
#define SMO_VERSION_STR "dev"
#endif

struct smo_ctx {
  smm_ctx* smm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;  // the host-buffer calls run on it
  DevBuf meta;                   // a *_device call's per-slot and per-stream arrays
  DevBuf slots;                  // compress: the raw compressor's output slots
  DevBuf io_in, io_out, sarg;    // the host-buffer calls' staging and their own arrays
  std::mutex mu;                 // serialises the host-buffer entry points
};

extern "C" {

const char* smo_status_message(sm_status st) {
  const char* m = smo::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* smo_version(void) { return "snappy_mi355x_orc gfx950 " SMO_VERSION_STR; }

smo_ctx* smo_ctx_create(int device) {
  smm_ctx* smm = smm_ctx_create(device);
  if (!smm) return nullptr;
  smo_ctx* ctx = new (std::nothrow) smo_ctx();
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
  }
  if (!ok) {
    ctx->stream = nullptr;
    smo_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smo_ctx_destroy(smo_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->meta, &ctx->slots, &ctx->io_in, &ctx->io_out, &ctx->sarg}) b->release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  }
  smm_ctx_destroy(ctx->smm);
  delete ctx;
}

int smo_ctx_last_indexed(smo_ctx* ctx) { return ctx ? smm_ctx_last_indexed(ctx->smm) : -1; }

// Launch sequence: the counting walk, the scan, the storing walk; the multi library's index builder
// and its decoder, once each over all slots (a stored chunk's is an empty one to them); the stored
// chunks' copies, the slots' verdicts, the streams' results.
sm_status smo_uncompress_streams_device(smo_ctx* ctx, uint32_t block_size, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_chunks,
                                        uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                        const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                        uint32_t* d_chunk_first, int32_t* d_chunk_status, void* stream) {
  if (!ctx || !smo::valid_block_size(block_size) || nstreams > smo::kMaxStreams || max_chunks > smo::kMaxStreams)
    return SM_ERR_ARGUMENT;
  if (!d_chunk_first != !d_chunk_status) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_chunks;
  SM_CHECK(ctx->meta.ensure(smo::decode_streams_bytes(nstreams, m, max_fragments)));
  const smo::DecodeStreamsArgs a{block_size, d_in,      d_in_off,  d_in_len,  nstreams, m,
                                 d_out,      d_out_off, d_out_cap, d_out_len, d_status, d_chunk_first,
                                 d_chunk_status, smo::carve_decode_streams((uint8_t*)ctx->meta.p, nstreams, m, max_fragments)};
  SM_CHECK(smo::launch_decode_plan(a, s));
  if (m) {
    // the index of every compressed slot that a block compressor wrote (over max_fragments: the
    // empty index), then the decode, by fragments where the index allows.  With no fragments allowed
    // the index would be the empty one, which decodes as no index does: it is not built.
    const bool index = max_fragments != 0;
    if (index)
      SM_PASS(smm_index_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.cap, a.s.frag_first,
                               a.s.frag_pos, a.s.built, a.s.index_status, stream));
    SM_PASS(smm_uncompress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, d_out, a.s.out_off, a.s.cap,
                                  a.s.out_len, a.s.dec_status, index ? a.s.frag_first : nullptr,
                                  index ? a.s.frag_pos : nullptr, stream));
  }
  SM_CHECK(smo::launch_decode_result(a, s));
  return SM_OK;
}

// Launch sequence: the scan of the piece counts, the pieces; the multi library's compressor, once
// over all pieces; the choice and the scan of the chunk sizes, the pack, the streams' results.
sm_status smo_compress_streams_device(smo_ctx* ctx, uint32_t block_size, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_pieces, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream) {
  if (!ctx || !smo::valid_block_size(block_size) || nstreams > smo::kMaxStreams || max_pieces > smo::kMaxStreams ||
      !valid_mode(mode))
    return SM_ERR_ARGUMENT;
  const uint64_t fragments = smo::piece_fragment_bound(max_pieces, block_size);
  if (fragments > smo::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_pieces;
  SM_CHECK(ctx->meta.ensure(smo::compress_streams_bytes(nstreams, m)));
  SM_CHECK(ctx->slots.ensure(smo::compress_streams_slot_bytes(m, block_size)));
  const smo::CompressStreamsArgs a{block_size, d_in,      d_in_off,  d_in_len, nstreams, m, (const uint8_t*)ctx->slots.p,
                                   d_out,      d_out_off, d_out_len, d_status, smo::carve_compress_streams((uint8_t*)ctx->meta.p, nstreams, m)};
  SM_CHECK(smo::launch_compress_plan(a, s));
  if (m)
    SM_PASS(smm_compress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, (uint32_t)fragments, (uint8_t*)ctx->slots.p,
                                a.s.slot_off, a.s.comp_len, a.s.comp_status, nullptr, nullptr, mode, stream));
  SM_CHECK(smo::launch_compress_pack(a, s));
  return SM_OK;
}

// ---- host buffers (../common/smc_staging.h) ------------------------------------------------------
sm_status smo_compress_streams(smo_ctx* ctx, uint32_t block_size, const uint8_t* in, const uint64_t* in_off,
                               const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                               uint64_t* out_len, int32_t* status, int mode) {
  if (!ctx || !smo::valid_block_size(block_size) || nstreams > smo::kMaxStreams || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in_off || !in_len || !out || !out_off || !out_len || !status) return SM_ERR_ARGUMENT;
  uint64_t pieces = 0;
  std::vector<uint64_t> room(nstreams);
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
    pieces += smo::stream_pieces(in_len[r], block_size);
    if (pieces > smo::kMaxStreams || smo::piece_fragment_bound(pieces, block_size) > smo::kMaxStreams)
      return SM_ERR_INPUT_TOO_LARGE;
    room[r] = smo::max_length(in_len[r], block_size);
  }
  const StreamStaging h(in, in_off, in_len, nstreams, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, nullptr, nstreams, d));
  SM_PASS(smo_compress_streams_device(ctx, block_size, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nstreams,
                                      (uint32_t)pieces, (uint8_t*)ctx->io_out.p, d.out_off, d.out_len, d.status, mode,
                                      ctx->stream));
  std::vector<uint8_t> packed;
  SM_PASS(download_stream_call(b, h, d, nstreams, out_len, status, packed));
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (out_len[r] > room[r]) return SM_ERR_DEVICE;
    if (out_len[r]) memcpy(out + out_off[r], packed.data() + h.out_off[r], (size_t)out_len[r]);
  }
  return SM_OK;
}

sm_status smo_uncompress_streams(smo_ctx* ctx, uint32_t block_size, const uint8_t* in, const uint64_t* in_off,
                                 const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                                 const uint64_t* out_cap, uint64_t* out_len, int32_t* status) {
  if (!ctx || !smo::valid_block_size(block_size) || nstreams > smo::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  // the plan on the host: the two bounds, and the room each decoded stream needs on the device
  std::vector<uint64_t> room(nstreams);
  uint64_t chunks = 0, fragments = 0;
  const sm_status planned = smo_streams_plan(in, in_off, in_len, nstreams, block_size, out_cap, smo::kMaxStreams, nullptr,
                                             room.data(), status, &chunks, &fragments);
  if (planned != SM_OK) return planned == SM_BUFFER_TOO_SMALL ? (sm_status)SM_ERR_INPUT_TOO_LARGE : planned;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status[r] != SM_OK) room[r] = 0;  // (not decoded)
    if (room[r] && !out) return SM_ERR_ARGUMENT;
  }
  if (fragments > smo::kMaxStreams) fragments = 0;  // (a hint: such a batch decodes in stream order)
  const StreamStaging h(in, in_off, in_len, nstreams, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, out_cap, nstreams, d));
  SM_PASS(smo_uncompress_streams_device(ctx, block_size, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nstreams,
                                        (uint32_t)chunks, (uint32_t)fragments, (uint8_t*)ctx->io_out.p, d.out_off,
                                        d.out_cap, d.out_len, d.status, nullptr, nullptr, ctx->stream));
  std::vector<uint8_t> decoded;
  SM_PASS(download_stream_call(b, h, d, nstreams, out_len, status, decoded));
  for (uint32_t r = 0; r < nstreams; ++r)
    if (room[r]) memcpy(out + out_off[r], decoded.data() + h.out_off[r], (size_t)room[r]);
  return SM_OK;
}

}  // extern "C"
