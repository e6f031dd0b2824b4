// smt_api.hip -- C ABI of the LevelDB table library (include/snappy_mi355x_table.h) over the multi
// library's and the framing library's public device calls (libsnappy_mi355x_multi.so and
// libsnappy_mi355x_framing.so, linked by name) and the kernels of smt_kernels.hip.  The host-only
// entry points live in smt_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../../include/snappy_mi355x_framing.h"
#include "../../../include/snappy_mi355x_multi.h"
#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "smt_format.h"
#include "smt_internal.h"

#ifndef SMT_VERSION_STR
#define SMT_VERSION_STR "dev"
#endif

struct smt_ctx {
  smm_ctx* smm = nullptr;
  smf_ctx* smf = nullptr;  // the batched masked CRC-32C
  int device = 0;
  hipStream_t stream = nullptr;  // the host-buffer calls run on it
  DevBuf meta;                   // a *_device call's arrays, the decoded index blocks, the encoder's stage
  DevBuf io_in, io_out, sarg;    // the host-buffer calls' staging and their own arrays
  std::mutex mu;                 // serialises the host-buffer entry points
};

namespace {

// The decode of the planned slots, shared by the tables call and the handle-level call: the index of
// every compressed slot and its decode (by fragments where the index allows), the stored slots'
// copy, the checksums of the stored bytes, the verdicts.
sm_status decode_slots(smt_ctx* ctx, const smt::DecodeArgs& a, uint32_t max_fragments, uint8_t* d_out, void* stream) {
  const uint32_t m = a.m;
  if (m) {
    const bool index = max_fragments != 0;
    if (index)
      SM_PASS(smm_index_device(ctx->smm, a.in, a.s.b_in_off, a.s.b_in_len, m, max_fragments, a.s.b_cap, a.s.frag_first,
                               a.s.frag_pos, a.s.built, a.s.b_index_status, stream));
    SM_PASS(smm_uncompress_device(ctx->smm, a.in, a.s.b_in_off, a.s.b_in_len, m, max_fragments, d_out, a.s.b_out_off, a.s.b_cap,
                                  a.s.b_out_len, a.s.b_dec, index ? a.s.frag_first : nullptr, index ? a.s.frag_pos : nullptr,
                                  stream));
    SM_CHECK(smt::launch_block_copy(a, d_out, (hipStream_t)stream));
    if (a.verify)
      SM_PASS(smf_crc32c_batch_device(ctx->smf, a.in, a.s.b_crc_off, a.s.b_crc_len, m, a.s.b_computed, 1, stream));
  }
  SM_CHECK(smt::launch_block_result(a, (hipStream_t)stream));
  return SM_OK;
}

// The index stage: footers and heads, the index blocks' checksums, their decode or copy into the
// scratch, the walks.
sm_status index_stage(smt_ctx* ctx, const smt::DecodeArgs& a, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  SM_CHECK(smt::launch_index_heads(a, s));
  if (a.verify)
    SM_PASS(smf_crc32c_batch_device(ctx->smf, a.in, a.s.ix_crc_off, a.s.ix_crc_len, a.nt, a.s.ix_computed, 1, stream));
  SM_PASS(smm_uncompress_device(ctx->smm, a.in, a.s.ix_in_off, a.s.ix_in_len, a.nt, 0, a.s.index, a.s.ix_out_off, a.s.ix_cap,
                                a.s.ix_out_len, a.s.ix_dec, nullptr, nullptr, stream));
  SM_CHECK(smt::launch_index_walk(a, s));
  return SM_OK;
}

}  // namespace

extern "C" {

const char* smt_status_message(sm_status st) {
  const char* m = smt::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* smt_version(void) { return "snappy_mi355x_table gfx950 " SMT_VERSION_STR; }

smt_ctx* smt_ctx_create(int device) {
  smt_ctx* ctx = new (std::nothrow) smt_ctx();
  if (!ctx) return nullptr;
  ctx->device = device;
  ctx->smm = smm_ctx_create(device);
  ctx->smf = ctx->smm ? smf_ctx_create(device) : nullptr;
  bool ok = ctx->smm && ctx->smf;
  if (ok) {
    DeviceGuard g(device);
    ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) ctx->stream = nullptr;
  }
  if (!ok) {
    smt_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smt_ctx_destroy(smt_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->meta, &ctx->io_in, &ctx->io_out, &ctx->sarg}) b->release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  }
  if (ctx->smf) smf_ctx_destroy(ctx->smf);
  if (ctx->smm) smm_ctx_destroy(ctx->smm);
  delete ctx;
}

int smt_ctx_last_indexed(smt_ctx* ctx) { return ctx ? smm_ctx_last_indexed(ctx->smm) : -1; }

// Launch sequence: the footers and the index blocks' heads, the scan that places the index blocks;
// the framing library's CRC-32C once over the index blocks; the multi library's decoder once over
// the compressed ones, the copy of the stored ones; the verdicts, the counting walk, the scan, the
// storing walk, the results.
sm_status smt_index_tables_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                  uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes, int verify_crc,
                                  uint32_t* d_block_first, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                  int32_t* d_status, void* stream) {
  if (!ctx || ntables > smt::kMaxCount || max_blocks > smt::kMaxCount) return SM_ERR_ARGUMENT;
  if (ntables == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_block_first || !d_status) return SM_ERR_ARGUMENT;
  if (max_blocks && (!d_handle_off || !d_handle_size)) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(ctx->meta.ensure(smt::decode_bytes(ntables, max_blocks, (size_t)max_index_bytes, 0)));
  smt::DecodeArgs a{};
  a.in = d_in;
  a.in_off = d_in_off;
  a.in_len = d_in_len;
  a.nt = ntables;
  a.m = max_blocks;
  a.index_bytes = max_index_bytes;
  a.verify = verify_crc ? 1u : 0u;
  a.decode = false;
  a.status = d_status;
  a.block_first = d_block_first;
  a.handle_off = d_handle_off;
  a.handle_size = d_handle_size;
  a.s = smt::carve_decode((uint8_t*)ctx->meta.p, ntables, max_blocks, (size_t)max_index_bytes, 0);
  return index_stage(ctx, a, stream);
}

// Launch sequence: the heads and the slots; then decode_slots.
sm_status smt_uncompress_blocks_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_blk_off,
                                       const uint64_t* d_blk_size, uint32_t nblocks, uint32_t max_fragments, int verify_crc,
                                       uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, void* stream) {
  if (!ctx || nblocks > smt::kMaxCount) return SM_ERR_ARGUMENT;
  if (nblocks == 0) return SM_OK;
  if (!d_in || !d_blk_off || !d_blk_size || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(ctx->meta.ensure(smt::decode_bytes(0, nblocks, 0, max_fragments)));
  smt::DecodeArgs a{};
  a.in = d_in;
  a.m = nblocks;
  a.verify = verify_crc ? 1u : 0u;
  a.decode = false;
  a.out_off = d_out_off;
  a.out_cap = d_out_cap;
  a.out_len = d_out_len;
  a.status = d_status;
  a.blk_off = d_blk_off;
  a.blk_size = d_blk_size;
  a.s = smt::carve_decode((uint8_t*)ctx->meta.p, 0, nblocks, 0, max_fragments);
  SM_CHECK(smt::launch_handle_plan(a, (hipStream_t)stream));
  return decode_slots(ctx, a, max_fragments, d_out, stream);
}

// Launch sequence: the index stage (smt_index_tables_device's); the heads, a thread per block, the
// scan of the declared lengths, the tables' plans, the slots; then decode_slots and the tables'
// results.
sm_status smt_uncompress_tables_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes,
                                       uint32_t max_fragments, int verify_crc, uint8_t* d_out, const uint64_t* d_out_off,
                                       const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                       uint32_t* d_block_first, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                       uint64_t* d_block_out_off, uint64_t* d_block_len, int32_t* d_block_status,
                                       void* stream) {
  if (!ctx || ntables > smt::kMaxCount || max_blocks > smt::kMaxCount) return SM_ERR_ARGUMENT;
  if (ntables == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(ctx->meta.ensure(smt::decode_bytes(ntables, max_blocks, (size_t)max_index_bytes, max_fragments)));
  smt::DecodeArgs a{};
  a.in = d_in;
  a.in_off = d_in_off;
  a.in_len = d_in_len;
  a.nt = ntables;
  a.m = max_blocks;
  a.index_bytes = max_index_bytes;
  a.verify = verify_crc ? 1u : 0u;
  a.decode = true;
  a.out_off = d_out_off;
  a.out_cap = d_out_cap;
  a.out_len = d_out_len;
  a.status = d_status;
  a.block_first = d_block_first;
  a.handle_off = d_handle_off;
  a.handle_size = d_handle_size;
  a.block_out_off = d_block_out_off;
  a.block_len = d_block_len;
  a.block_status = d_block_status;
  a.s = smt::carve_decode((uint8_t*)ctx->meta.p, ntables, max_blocks, (size_t)max_index_bytes, max_fragments);
  SM_PASS(index_stage(ctx, a, stream));
  SM_CHECK(smt::launch_block_plan(a, (hipStream_t)stream));
  return decode_slots(ctx, a, max_fragments, d_out, stream);
}

// Launch sequence: the blocks against the bounds with the scan of the stage, the slots; the multi
// library's compressor once over all blocks into the stage; the decision and the scan of the sizes,
// the pack; the framing library's CRC-32C once over the packed ranges; the checksum bytes, the results.
sm_status smt_compress_blocks_device(smt_ctx* ctx, const uint8_t* d_in, const uint32_t* d_block_first,
                                     const uint64_t* d_block_off, const uint32_t* d_block_len, uint32_t ntables,
                                     uint32_t max_blocks, uint64_t stage_bytes, uint32_t max_fragments, uint8_t* d_out,
                                     const uint64_t* d_out_off, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                     uint64_t* d_out_len, int32_t* d_status, int mode, void* stream) {
  if (!ctx || ntables > smt::kMaxCount || max_blocks > smt::kMaxCount || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (ntables == 0) return SM_OK;
  if (!d_in || !d_block_first || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  if (max_blocks && (!d_block_off || !d_block_len || !d_handle_off || !d_handle_size)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_blocks;
  const size_t stage = (size_t)stage_bytes + 64;  // (spare bytes behind the stage: the unused slots' empty raw streams)
  SM_CHECK(ctx->meta.ensure(smt::compress_bytes(ntables, m, stage)));
  const smt::CompressArgs a{d_in,  d_block_first, d_block_off, d_block_len,   ntables,   m,         stage_bytes, max_fragments,
                            d_out, d_out_off,     d_handle_off, d_handle_size, d_out_len, d_status,
                            smt::carve_compress((uint8_t*)ctx->meta.p, ntables, m, stage)};
  SM_CHECK(smt::launch_compress_plan(a, s));
  if (m)
    SM_PASS(smm_compress_device(ctx->smm, d_in, a.s.in_off, a.s.in_len, m, max_fragments, a.s.stage, a.s.slot_off, a.s.comp_len,
                                a.s.comp_status, nullptr, nullptr, mode, stream));
  SM_CHECK(smt::launch_compress_pack(a, s));
  if (m) SM_PASS(smf_crc32c_batch_device(ctx->smf, d_out, a.s.crc_off, a.s.crc_len, m, a.s.crc, 1, stream));
  SM_CHECK(smt::launch_compress_result(a, s));
  return SM_OK;
}

}  // extern "C"

// ---- host buffers (../common/smc_staging.h) ------------------------------------------------------
using smc::round16;

extern "C" {

// The tables' bytes packed behind one another in one staging block (one upload), and room for every
// table's output at a 16-byte boundary of the device buffer (one download; each table's own bytes
// then go to the caller's place).
sm_status smt_uncompress_tables(smt_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t ntables, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t* block_first,
                                uint32_t max_entries, uint64_t* handle_off, uint64_t* handle_size, uint64_t* block_len,
                                int32_t* block_status) {
  if (!ctx || ntables > smt::kMaxCount) return SM_ERR_ARGUMENT;
  if (ntables == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  const bool entries = block_first != nullptr;
  if (entries != (handle_off != nullptr) || entries != (handle_size != nullptr) || entries != (block_len != nullptr) ||
      entries != (block_status != nullptr))
    return SM_ERR_ARGUMENT;
  // the bounds on the host: each table's decoded index length, and the entries that many bytes hold
  uint64_t index_bytes = 0, blocks = 0;
  for (uint32_t t = 0; t < ntables; ++t) {
    if (in_len[t] && !in) return SM_ERR_ARGUMENT;
    if (out_cap[t] && !out) return SM_ERR_ARGUMENT;
    uint64_t ib = 0;
    if (smt_index_bound(in_len[t] ? in + in_off[t] : nullptr, (size_t)in_len[t], &ib) == SM_OK) {
      index_bytes += round16(ib);
      blocks += smt_max_blocks(ib);
    }
  }
  if (blocks > smt::kMaxCount) return SM_ERR_INPUT_TOO_LARGE;
  const StreamStaging h(in, in_off, in_len, ntables, out_cap);
  uint64_t fragments = blocks + h.out_total / 65536;  // (a hint: what the decoded tables' blocks can hold)
  if (fragments > smt::kMaxCount) fragments = 0;
  const uint32_t m = (uint32_t)blocks;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t n = ntables, e8 = round16(8 * (size_t)m + 8), e4 = round16(4 * (size_t)m + 4);
  SM_PASS(ensure_staging(b, h.bytes.size(), (size_t)h.out_total, 5 * round16(8 * n) + 2 * round16(4 * (n + 1)) + 3 * e8 + e4));
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
  uint64_t* const d_hoff = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint64_t* const d_hsize = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint64_t* const d_blen = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  int32_t* const d_bstatus = up.put((const int32_t*)nullptr, (size_t)m + 1, e);
  SM_CHECK(e);
  SM_CHECK(hipMemsetAsync(d_first, 0, 4 * (n + 1), s));  // (over a bound the call leaves it alone)
  SM_PASS(smt_uncompress_tables_device(ctx, (const uint8_t*)ctx->io_in.p, d_in_off, d_in_len, ntables, m, index_bytes,
                                       (uint32_t)fragments, verify_crc, (uint8_t*)ctx->io_out.p, d_out_off, d_out_cap, d_out_len,
                                       d_status, d_first, d_hoff, d_hsize, nullptr, d_blen, d_bstatus, s));
  std::vector<uint8_t> decoded;
  std::vector<uint32_t> first(n + 1);
  SM_PASS(download_results(b, d_out_len, d_status, n, out_len, status));
  SM_CHECK(hipMemcpyAsync(first.data(), d_first, 4 * (n + 1), hipMemcpyDeviceToHost, s));
  SM_PASS(download_output(b, h.out_total, decoded));
  for (uint32_t t = 0; t < ntables; ++t)
    if (status[t] != SM_ERR_ARGUMENT && out_len[t] && out_len[t] <= out_cap[t])
      memcpy(out + out_off[t], decoded.data() + h.out_off[t], (size_t)out_len[t]);
  if (!entries) return SM_OK;
  const uint32_t total = first[n];
  if (total > m) return SM_ERR_DEVICE;
  if (total > max_entries) return SM_BUFFER_TOO_SMALL;
  memcpy(block_first, first.data(), 4 * (n + 1));
  if (total) {
    SM_CHECK(hipMemcpyAsync(handle_off, d_hoff, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(handle_size, d_hsize, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(block_len, d_blen, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(block_status, d_bstatus, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipStreamSynchronize(s));
  }
  return SM_OK;
}

sm_status smt_uncompress_blocks(smt_ctx* ctx, const uint8_t* in, size_t n, const uint64_t* blk_off, const uint64_t* blk_size,
                                uint32_t nblocks, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status) {
  if (!ctx || nblocks > smt::kMaxCount) return SM_ERR_ARGUMENT;
  if (nblocks == 0) return SM_OK;
  if (!in || !blk_off || !blk_size || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  std::vector<uint64_t> h_out_off(nblocks);
  uint64_t out_total = 0, fragments = 0;
  for (uint32_t j = 0; j < nblocks; ++j) {  // (trusted, but a handle that leaves the buffer cannot be uploaded)
    if (blk_size[j] > smt::kMaxSize || blk_size[j] + smt::kTrailer > n || blk_off[j] > n - blk_size[j] - smt::kTrailer)
      return SM_ERR_ARGUMENT;
    if (out_cap[j] && !out) return SM_ERR_ARGUMENT;
    h_out_off[j] = out_total;
    out_total += round16(out_cap[j]);
    fragments += smt::decode_fragments(out_cap[j]);
  }
  if (fragments > smt::kMaxCount) fragments = 0;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t k = nblocks;
  SM_PASS(ensure_staging(b, n, (size_t)out_total, 5 * round16(8 * k) + round16(4 * k)));
  ArgUpload up{smc::Carve{(uintptr_t)ctx->sarg.p}, s};
  hipError_t e = hipMemcpyAsync(ctx->io_in.p, in, n, hipMemcpyHostToDevice, s);
  const uint64_t* const d_off = up.put(blk_off, k, e);
  const uint64_t* const d_size = up.put(blk_size, k, e);
  const uint64_t* const d_out_off = up.put(h_out_off.data(), k, e);
  const uint64_t* const d_out_cap = up.put(out_cap, k, e);
  uint64_t* const d_out_len = up.put((const uint64_t*)nullptr, k, e);
  int32_t* const d_status = up.put((const int32_t*)nullptr, k, e);
  SM_CHECK(e);
  SM_PASS(smt_uncompress_blocks_device(ctx, (const uint8_t*)ctx->io_in.p, d_off, d_size, nblocks, (uint32_t)fragments, verify_crc,
                                       (uint8_t*)ctx->io_out.p, d_out_off, d_out_cap, d_out_len, d_status, s));
  std::vector<uint8_t> decoded;
  SM_PASS(download_results(b, d_out_len, d_status, k, out_len, status));
  SM_PASS(download_output(b, out_total, decoded));
  for (uint32_t j = 0; j < nblocks; ++j)
    if (out_len[j] && out_len[j] <= out_cap[j]) memcpy(out + out_off[j], decoded.data() + h_out_off[j], (size_t)out_len[j]);
  return SM_OK;
}

// The encoder's twin: every block packed behind one another (each at a 16-byte boundary), the three
// bounds counted here, and per table the room the bound promises.
sm_status smt_compress_blocks(smt_ctx* ctx, const uint8_t* in, const uint32_t* block_first, const uint64_t* block_off,
                              const uint32_t* block_len, uint32_t ntables, uint8_t* out, const uint64_t* out_off,
                              uint64_t* handle_off, uint64_t* handle_size, uint64_t* out_len, int32_t* status, int mode) {
  if (!ctx || ntables > smt::kMaxCount || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (ntables == 0) return SM_OK;
  if (!block_first || !out || !out_off || !out_len || !status) return SM_ERR_ARGUMENT;
  const uint32_t m = block_first[ntables];
  if (m > smt::kMaxCount || (m && (!in || !block_off || !block_len || !handle_off || !handle_size))) return SM_ERR_ARGUMENT;
  for (uint32_t t = 0; t < ntables; ++t)
    if (block_first[t] > block_first[t + 1]) return SM_ERR_ARGUMENT;
  if (block_first[0] != 0) return SM_ERR_ARGUMENT;
  std::vector<uint64_t> h_block_off(m), h_out_off(ntables), room(ntables);
  uint64_t in_total = 0, out_total = 0, stage = 0, fragments = 0;
  for (uint32_t t = 0; t < ntables; ++t) {
    room[t] = 0;
    for (uint32_t j = block_first[t]; j < block_first[t + 1]; ++j) {
      in_total = round16(in_total);
      h_block_off[j] = in_total;
      in_total += block_len[j];
      room[t] += smt::max_block_length(block_len[j]);
      stage += smt::stage_length(block_len[j]);
      fragments += smt::encode_fragments(block_len[j]);
    }
    h_out_off[t] = out_total;
    out_total += round16(room[t]);
  }
  if (fragments > smt::kMaxCount) return SM_ERR_INPUT_TOO_LARGE;
  std::vector<uint8_t> bytes((size_t)in_total);
  for (uint32_t j = 0; j < m; ++j)
    if (block_len[j]) memcpy(bytes.data() + h_block_off[j], in + block_off[j], block_len[j]);
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  hipStream_t s = ctx->stream;
  const size_t n = ntables;
  SM_PASS(ensure_staging(b, bytes.size(), (size_t)out_total,
                         2 * round16(8 * n) + 2 * round16(4 * (n + 1)) + 3 * round16(8 * (size_t)m + 8) + round16(4 * (size_t)m + 4)));
  ArgUpload up{smc::Carve{(uintptr_t)ctx->sarg.p}, s};
  hipError_t e = hipSuccess;
  if (!bytes.empty()) e = hipMemcpyAsync(ctx->io_in.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s);
  const uint32_t* const d_first = up.put(block_first, n + 1, e);
  const uint64_t* const d_block_off = up.put(h_block_off.data(), m, e);
  const uint32_t* const d_block_len = up.put(block_len, m, e);
  const uint64_t* const d_out_off = up.put(h_out_off.data(), n, e);
  uint64_t* const d_out_len = up.put((const uint64_t*)nullptr, n, e);
  int32_t* const d_status = up.put((const int32_t*)nullptr, n, e);
  uint64_t* const d_hoff = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  uint64_t* const d_hsize = up.put((const uint64_t*)nullptr, (size_t)m + 1, e);
  SM_CHECK(e);
  SM_PASS(smt_compress_blocks_device(ctx, (const uint8_t*)ctx->io_in.p, d_first, d_block_off, d_block_len, ntables, m, stage,
                                     (uint32_t)fragments, (uint8_t*)ctx->io_out.p, d_out_off, d_hoff, d_hsize, d_out_len, d_status,
                                     mode, s));
  std::vector<uint8_t> packed;
  SM_PASS(download_results(b, d_out_len, d_status, n, out_len, status));
  if (m) {
    SM_CHECK(hipMemcpyAsync(handle_off, d_hoff, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
    SM_CHECK(hipMemcpyAsync(handle_size, d_hsize, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
  }
  SM_PASS(download_output(b, out_total, packed));
  for (uint32_t t = 0; t < ntables; ++t) {
    if (out_len[t] > room[t]) return SM_ERR_DEVICE;
    if (status[t] == SM_OK && out_len[t]) memcpy(out + out_off[t], packed.data() + h_out_off[t], (size_t)out_len[t]);
  }
  return SM_OK;
}

}  // extern "C"
