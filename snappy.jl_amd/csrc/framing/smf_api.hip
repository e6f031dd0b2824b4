// smf_api.hip -- C ABI of the framing format (include/snappy_mi355x_framing.h) over the raw
// codec's public batched device calls (libsnappy_mi355x.so, linked by name) and the kernels of
// smf_kernels.hip, smf_range.hip (the seek index and the ranged decode) and smf_streams.hip (a batch
// of streams per call).  The host-only entry points live in smf_host.cpp.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../common/smc_hip_host.h"
#include "../common/smc_layout.h"
#include "../common/smc_staging.h"
#include "smf_format.h"
#include "smf_internal.h"

#ifndef SMF_VERSION_STR
#define SMF_VERSION_STR "dev"
#endif

namespace {

constexpr uint64_t kSlotPitch = smc::kFramingSlotPitch;

// ---- scratch layouts: each is sized by its own carve from a null base (smc::Carve) ----------------
struct CompressMeta {  // per block (ctx->meta)
  uint64_t *in_off, *slot_off, *dst_off;
  uint32_t *in_len, *comp_len, *crc;
  uint8_t* type;
  uintptr_t end;
};
constexpr CompressMeta carve_compress(uintptr_t base, size_t n) {
  smc::Carve c{base};
  CompressMeta m{};
  m.in_off = c.take<uint64_t>(n);
  m.slot_off = c.take<uint64_t>(n);
  m.dst_off = c.take<uint64_t>(n);
  m.in_len = c.take<uint32_t>(n);
  m.comp_len = c.take<uint32_t>(n);
  m.crc = c.take<uint32_t>(n);
  m.type = c.take<uint8_t>(n);
  m.end = c.p;
  return m;
}
constexpr size_t compress_bytes(size_t n) { return carve_compress(0, n).end; }

// smf_uncompress_chunks_device's slots at base (ctx->meta): one group, the caller's index and
// d_chunk_status serve, so the call owns the plan's arrays and the stage's outputs.  Returns the bytes.
size_t carve_chunk_slots(uintptr_t base, size_t n, smf::Slots& sl) {
  smc::Carve c{base};
  sl = smf::carve_slots(c, n, 1, false, true, false);
  return c.p - base;
}

struct IndexMeta {  // a stream's index and the per-chunk status behind it (ctx->idx)
  smf_chunks ch;
  int32_t* chunk_status;
  uintptr_t end;
};
constexpr IndexMeta carve_index(uintptr_t base, size_t n) {
  smc::Carve c{base};
  IndexMeta m{};
  m.ch.pay_off = c.take<uint64_t>(n);
  m.ch.pay_len = c.take<uint32_t>(n);
  m.ch.crc = c.take<uint32_t>(n);
  m.ch.ulen = c.take<uint32_t>(n);
  m.chunk_status = c.take<int32_t>(n);
  m.ch.type = c.take<uint8_t>(n);
  m.end = c.p;
  return m;
}
constexpr size_t index_bytes(size_t n) { return carve_index(0, n).end; }

// A buffer of cap bytes holds cap / kIndexEntryBound entries, for every cap a DevBuf has (4096 at
// the least): index_bytes(e) <= e * index_bytes(16) / 16 + 15 * index_bytes(1) / 16, the bytes of
// an entry and under 16 of padding per array, and with e = cap / kIndexEntryBound the padding is
// at most e.
constexpr size_t kIndexEntryBound = 26;
static_assert(index_bytes(16) / 16 < kIndexEntryBound && 15 * (index_bytes(1) / 16) <= 4096 / kIndexEntryBound,
              "kIndexEntryBound does not cover an index entry of carve_index");

// ---- the small device results in ctx->res ---------------------------------------------------------
struct LenStatus {  // what a *_device call leaves in *d_out_len and *d_status
  uint64_t len;
  int32_t st, pad;
};
struct Results {
  smf_summary sum;  // smf_uncompress_device, smf_uncompressed_length_device: the walk's summary
  alignas(64) LenStatus io;  // smf_compress, smf_uncompress, smf_validate
  alignas(64) uint64_t range[3];  // smf_uncompress_range: lo, len, out_off
  alignas(32) LenStatus range_out;
};
static_assert(offsetof(Results, io) == 64 && offsetof(Results, range) == 128 && offsetof(Results, range_out) == 160 &&
                  sizeof(Results) <= 4096,
              "the layout of ctx->res");

}  // namespace

struct smf_ctx {
  sm_ctx* sm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;  // the sm_ctx's: the host-buffer calls run on it
  DevBuf lut;                    // smf::CrcLut
  DevBuf meta;                   // a *_device call's per-slot and per-group arrays
  DevBuf slots;                  // compress: the raw compressor's output slots
  DevBuf idx;                    // a stream's index (smf_uncompress_device, smf_uncompress)
  DevBuf io_in, io_out, res;     // the host-buffer calls' staging; small results
  DevBuf redge;                  // ranged decode: the edge slots
  DevBuf roff;                   // smf_uncompress_range: the index slice's chunk_off
  DevBuf sarg;                   // smf_compress_streams, smf_uncompress_streams: the calls' own arrays
  std::mutex mu;                 // serialises the host-buffer entry points
};

namespace {

// the index arrays of up to n chunks in ctx->idx, and the per-chunk status behind them
sm_status index_scratch(smf_ctx* ctx, size_t n, IndexMeta& m) {
  SM_CHECK(ctx->idx.ensure(index_bytes(n)));
  m = carve_index((uintptr_t)ctx->idx.p, n);
  return SM_OK;
}

// a host index's entries [first, first + count) to the device arrays
sm_status upload_chunks(const smf_chunks& dst, const smf_chunks& src, uint32_t first, uint32_t count, hipStream_t s) {
  if (count == 0) return SM_OK;
  const size_t k = count;
  SM_CHECK(hipMemcpyAsync(dst.type, src.type + first, k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(dst.pay_off, src.pay_off + first, 8 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(dst.pay_len, src.pay_len + first, 4 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(dst.crc, src.crc + first, 4 * k, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(dst.ulen, src.ulen + first, 4 * k, hipMemcpyHostToDevice, s));
  return SM_OK;
}

// The slot stage (smf_slots.h) behind a decode plan: the raw decoder over the m slots of `in`, the
// 0x01 slots' copies, the CRC-32C of every slot's output and the slots' verdicts.  Output offsets
// are relative to out_base.
sm_status slot_stage(smf_ctx* ctx, const uint8_t* in, uint8_t* out_base, const smf::Slots& sl, uint32_t m, hipStream_t s) {
  if (m == 0) return SM_OK;
  SM_PASS(sm_uncompress_batch_device(ctx->sm, in, sl.in_off, sl.dec_len, m, out_base, sl.out_off, sl.cap, sl.dec_out_len,
                                     sl.dec_status, s));
  SM_CHECK(smf::launch_slot_copy(in, out_base, sl, m, s));
  SM_CHECK(smf::launch_crc32c(out_base, sl.out_off, sl.cap, m, sl.crc_out, 1, (const smf::CrcLut*)ctx->lut.p, s));
  SM_CHECK(smf::launch_slot_verify(sl, m, s));
  return SM_OK;
}

// The end of a single-buffer host call: the pair its *_device call on s left at d, read back
// (synchronises s; a status in it is returned), the length checked (at most `most`, or exactly it),
// and, with dst, that many bytes of ctx->io_out to the caller.
sm_status finish(smf_ctx* ctx, const LenStatus* d, uint64_t most, bool exact, uint8_t* dst, size_t* length, hipStream_t s) {
  LenStatus r;
  SM_CHECK(hipMemcpyAsync(&r, d, sizeof(r), hipMemcpyDeviceToHost, s));
  SM_CHECK(hipStreamSynchronize(s));
  SM_PASS(r.st);
  if (r.len > most || (exact && r.len != most)) return SM_ERR_DEVICE;
  if (dst && r.len) SM_CHECK(hipMemcpy(dst, ctx->io_out.p, (size_t)r.len, hipMemcpyDeviceToHost));
  if (length) *length = (size_t)r.len;
  return SM_OK;
}

// A stream's index on the host, filled by smf_index; sum is its summary.
struct HostIndex {
  std::vector<uint8_t> type;
  std::vector<uint64_t> pay_off;
  std::vector<uint32_t> pay_len, crc, ulen;
  smf_summary sum{};
  smf_chunks view() { return smf_chunks{type.data(), pay_off.data(), pay_len.data(), crc.data(), ulen.data()}; }
  sm_status fill(const uint8_t* framed, size_t n, uint32_t nchunks) {
    type.resize(nchunks);
    pay_off.resize(nchunks);
    for (auto* v : {&pay_len, &crc, &ulen}) v->resize(nchunks);
    const smf_chunks h = view();
    return smf_index(framed, n, &h, nchunks, &sum);
  }
};

}  // namespace

extern "C" {

const char* smf_status_message(sm_status st) {
  const char* m = smf::host_message(st);
  return m ? m : sm_status_message(st);
}

const char* smf_version(void) { return "snappy_mi355x_framing gfx950 " SMF_VERSION_STR; }

smf_ctx* smf_ctx_create(int device) {
  sm_ctx* sm = sm_ctx_create(device);
  if (!sm) return nullptr;
  smf_ctx* ctx = new (std::nothrow) smf_ctx();
  smf::CrcLut* lut = new (std::nothrow) smf::CrcLut();
  if (!ctx || !lut) {
    delete ctx;
    delete lut;
    sm_ctx_destroy(sm);
    return nullptr;
  }
  ctx->sm = sm;
  ctx->device = device;
  ctx->stream = (hipStream_t)sm_ctx_stream(sm);
  smf::build_crc_lut(lut);
  bool ok;
  {
    DeviceGuard g(device);
    ok = ctx->lut.ensure(sizeof(smf::CrcLut)) == hipSuccess && ctx->res.ensure(4096) == hipSuccess &&
         hipMemcpy(ctx->lut.p, lut, sizeof(smf::CrcLut), hipMemcpyHostToDevice) == hipSuccess;
  }
  delete lut;
  if (!ok) {
    smf_ctx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void smf_ctx_destroy(smf_ctx* ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();  // (the *_device calls ran on the callers' streams)
    for (DevBuf* b : {&ctx->lut, &ctx->meta, &ctx->slots, &ctx->idx, &ctx->io_in, &ctx->io_out, &ctx->res, &ctx->redge,
                      &ctx->roff, &ctx->sarg})
      b->release();
  }
  sm_ctx_destroy(ctx->sm);
  delete ctx;
}

sm_status smf_crc32c_batch_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_off, const uint32_t* d_len,
                                  uint32_t nblk, uint32_t* d_crc, int masked, void* stream) {
  if (!ctx) return SM_ERR_ARGUMENT;
  if (nblk == 0) return SM_OK;
  if (!d_in || !d_off || !d_len || !d_crc) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(smf::launch_crc32c(d_in, d_off, d_len, nblk, d_crc, masked ? 1 : 0, (const smf::CrcLut*)ctx->lut.p,
                              (hipStream_t)stream));
  return SM_OK;
}

// smf_compress_device; with d_chunk_off also the encoder's index (smf_compress_indexed_device)
static sm_status compress_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_capacity,
                                 uint64_t* d_out_len, int32_t* d_status, int mode, const smf_chunks* d_chunks,
                                 uint64_t* d_chunk_off, uint32_t max_chunks, uint32_t* d_nchunks, void* stream) {
  if (!ctx || !d_out || !d_out_len || !d_status || (n && !d_in)) return SM_ERR_ARGUMENT;
  if (!valid_mode(mode)) return SM_ERR_ARGUMENT;
  const uint64_t nblk64 = (n + smf::kBlock - 1) / smf::kBlock;
  if (nblk64 > 0x7fffffffull) return SM_ERR_INPUT_TOO_LARGE;
  if (out_capacity < smf_max_framed_length(n)) return SM_BUFFER_TOO_SMALL;
  smf_chunks ich{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (d_chunk_off) {
    if (!d_nchunks) return SM_ERR_ARGUMENT;
    if (max_chunks < nblk64) return SM_BUFFER_TOO_SMALL;
    if (!smf::take_chunks(d_chunks, nblk64, ich)) return SM_ERR_ARGUMENT;
  }
  const uint32_t nblk = (uint32_t)nblk64;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  SM_CHECK(ctx->meta.ensure(compress_bytes(nblk)));
  SM_CHECK(ctx->slots.ensure((size_t)nblk * kSlotPitch));
  const CompressMeta m = carve_compress((uintptr_t)ctx->meta.p, nblk);
  uint8_t* slots = (uint8_t*)ctx->slots.p;
  SM_CHECK(smf::launch_frame_compress_plan(n, nblk, kSlotPitch, m.in_off, m.in_len, m.slot_off, s));
  SM_PASS(sm_compress_batch_device(ctx->sm, d_in, m.in_off, m.in_len, nblk, slots, m.slot_off, m.comp_len, mode, stream));
  SM_CHECK(smf::launch_crc32c(d_in, m.in_off, m.in_len, nblk, m.crc, 1, (const smf::CrcLut*)ctx->lut.p, s));
  const smf::PackArgs a{d_in, m.in_off, m.in_len, slots, m.slot_off, m.comp_len, m.crc, m.type, m.dst_off, nblk, d_out};
  SM_CHECK(smf::launch_frame_pack(a, d_out_len, d_status, s));
  if (d_chunk_off) SM_CHECK(smf::launch_frame_index_out(a, n, ich, d_chunk_off, d_nchunks, d_status, s));
  return SM_OK;
}

sm_status smf_compress_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_capacity,
                              uint64_t* d_out_len, int32_t* d_status, int mode, void* stream) {
  return compress_device(ctx, d_in, n, d_out, out_capacity, d_out_len, d_status, mode, nullptr, nullptr, 0, nullptr,
                         stream);
}

sm_status smf_compress_indexed_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out,
                                      uint64_t out_capacity, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      const smf_chunks* d_chunks, uint64_t* d_chunk_off, uint32_t max_chunks,
                                      uint32_t* d_nchunks, void* stream) {
  if (!d_chunk_off) return SM_ERR_ARGUMENT;
  return compress_device(ctx, d_in, n, d_out, out_capacity, d_out_len, d_status, mode, d_chunks, d_chunk_off, max_chunks,
                         d_nchunks, stream);
}

sm_status smf_chunk_offsets_device(smf_ctx* ctx, const uint32_t* d_ulen, uint32_t nchunks, uint64_t* d_chunk_off,
                                   void* stream) {
  if (!ctx || !d_chunk_off || (nchunks && !d_ulen)) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(smf::launch_chunk_offsets(d_ulen, nchunks, d_chunk_off, (hipStream_t)stream));
  return SM_OK;
}

sm_status smf_uncompress_ranges_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, const smf_chunks* d_chunks,
                                       const uint64_t* d_chunk_off, uint32_t nchunks, const uint64_t* d_lo,
                                       const uint64_t* d_len, uint32_t nranges, uint32_t max_range_chunks,
                                       uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                       int32_t* d_range_status, void* stream) {
  if (!ctx || nchunks > smf::kMaxIndexChunks || nranges > smf::kMaxIndexChunks) return SM_ERR_ARGUMENT;
  if (nranges == 0) return SM_OK;
  if (!d_chunk_off || !d_lo || !d_len || !d_out_off || !d_out_len || !d_range_status) return SM_ERR_ARGUMENT;
  smf_chunks ch;
  if (nchunks && (!d_in || !d_out)) return SM_ERR_ARGUMENT;
  if (!smf::take_chunks(d_chunks, nchunks, ch)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_range_chunks;
  SM_CHECK(ctx->meta.ensure(smf::range_meta_bytes(nranges, m)));
  SM_CHECK(ctx->redge.ensure(smf::range_edge_bytes(nranges)));
  const smf::RangeArgs a{d_in,  n,       ch, d_chunk_off, nchunks,   d_lo,
                         d_len, nranges, m,  d_out,       d_out_off, (uint8_t*)ctx->redge.p,
                         smf::carve_range((uint8_t*)ctx->meta.p, nranges, m)};
  SM_CHECK(smf::launch_range_plan(a, s));
  // every slot's output offset is relative to the edge slots (smf_range.hip, k_range_slots)
  SM_PASS(slot_stage(ctx, d_in ? d_in : a.edge, a.edge, a.s.slots, m, s));
  SM_CHECK(smf::launch_range_trim(a, s));
  SM_CHECK(smf::launch_group_result(a.s.slots,
                                    smf::Groups{nranges, a.s.hdr, a.s.rpre, d_len, false, d_out_len, d_range_status}, s));
  return SM_OK;
}

sm_status smf_uncompress_streams_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_chunks, uint8_t* d_out,
                                        const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                        int32_t* d_status, uint32_t* d_chunk_first, int32_t* d_chunk_status,
                                        void* stream) {
  if (!ctx || nstreams > smf::kMaxStreams || max_chunks > smf::kMaxStreams) return SM_ERR_ARGUMENT;
  if (!d_chunk_first != !d_chunk_status) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_chunks;
  SM_CHECK(ctx->meta.ensure(smf::decode_streams_bytes(nstreams, m)));
  smf::DecodeStreamsArgs a{d_in,  d_in_off,  d_in_len,  nstreams,      m,
                           d_out, d_out_off, d_out_cap, d_chunk_first,
                           smf::carve_decode_streams((uint8_t*)ctx->meta.p, nstreams, m)};
  if (d_chunk_status) a.s.slots.slot_status = d_chunk_status;  // (the verdicts, where the caller wants them)
  SM_CHECK(smf::launch_streams_plan(a, s));
  SM_PASS(slot_stage(ctx, d_in, d_out, a.s.slots, m, s));
  SM_CHECK(smf::launch_group_result(a.s.slots, smf::Groups{nstreams, a.s.hdr, a.s.pre, a.s.length, true, d_out_len, d_status},
                                    s));
  return SM_OK;
}

sm_status smf_compress_streams_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_blocks, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream) {
  if (!ctx || nstreams > smf::kMaxStreams || max_blocks > smf::kMaxStreams || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  const uint32_t m = max_blocks;
  SM_CHECK(ctx->meta.ensure(smf::compress_streams_bytes(nstreams, m)));
  SM_CHECK(ctx->slots.ensure(smf::compress_streams_slot_bytes(m)));
  const smf::CompressStreamsArgs a{d_in,  d_in_off,  d_in_len,  nstreams, m, (const uint8_t*)ctx->slots.p,
                                   d_out, d_out_off, d_out_len, d_status,
                                   smf::carve_compress_streams((uint8_t*)ctx->meta.p, nstreams, m)};
  SM_CHECK(smf::launch_cstreams_plan(a, s));
  if (m) {
    SM_PASS(sm_compress_batch_device(ctx->sm, d_in, a.s.in_off, a.s.in_len, m, (uint8_t*)ctx->slots.p, a.s.slot_off,
                                     a.s.comp_len, mode, stream));
    SM_CHECK(smf::launch_crc32c(d_in, a.s.in_off, a.s.in_len, m, a.s.crc, 1, (const smf::CrcLut*)ctx->lut.p, s));
  }
  SM_CHECK(smf::launch_cstreams_pack(a, s));
  return SM_OK;
}

sm_status smf_index_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, const smf_chunks* d_chunks,
                           uint32_t max_chunks, smf_summary* d_summary, void* stream) {
  if (!ctx || !d_summary || (n && !d_in)) return SM_ERR_ARGUMENT;
  smf_chunks none{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (d_chunks && max_chunks == 0) d_chunks = &none;  // (nothing is stored; more than 0 chunks is still too small)
  if (d_chunks && max_chunks && !smf::valid_chunks(*d_chunks)) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  SM_CHECK(smf::launch_frame_index(d_in, n, d_chunks, max_chunks, d_summary, (hipStream_t)stream));
  return SM_OK;
}

sm_status smf_uncompressed_length_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint64_t* d_len,
                                         int32_t* d_status, void* stream) {
  if (!ctx || !d_len || !d_status || (n && !d_in)) return SM_ERR_ARGUMENT;
  DeviceGuard g(ctx->device);
  smf_summary* sum = &((Results*)ctx->res.p)->sum;
  SM_CHECK(smf::launch_frame_index(d_in, n, nullptr, 0, sum, (hipStream_t)stream));
  SM_CHECK(smf::launch_frame_result(d_len, 0, sum, d_status, 0, (hipStream_t)stream));
  return SM_OK;
}

sm_status smf_uncompress_chunks_device(smf_ctx* ctx, const uint8_t* d_in, const smf_chunks* d_chunks,
                                       uint32_t nchunks, uint8_t* d_out, uint64_t out_capacity,
                                       int32_t* d_chunk_status, uint64_t* d_out_len, int32_t* d_status, void* stream) {
  if (!ctx || !d_out_len || !d_status) return SM_ERR_ARGUMENT;
  smf_chunks ch;
  if (nchunks && (!d_in || !d_out || !d_chunk_status)) return SM_ERR_ARGUMENT;
  if (!smf::take_chunks(d_chunks, nchunks, ch)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  smf::Slots sl;
  SM_CHECK(ctx->meta.ensure(carve_chunk_slots(0, nchunks, sl)));
  carve_chunk_slots((uintptr_t)ctx->meta.p, nchunks, sl);
  // the caller's index is the slots' (a chunk that is not decoded has no room, so its copy moves nothing)
  sl.type = ch.type;
  sl.in_off = ch.pay_off;
  sl.crc_want = ch.crc;
  sl.slot_status = d_chunk_status;
  SM_CHECK(smf::launch_frame_plan(ch, nchunks, out_capacity, sl, d_out_len, s));
  SM_PASS(slot_stage(ctx, d_in, d_out, sl, nchunks, s));
  SM_CHECK(smf::launch_group_result(sl, smf::Groups{1, nullptr, nullptr, nullptr, false, nullptr, d_status}, s));
  return SM_OK;
}

sm_status smf_uncompress_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_capacity,
                                uint64_t* d_out_len, int32_t* d_status, void* stream) {
  if (!ctx || !d_out_len || !d_status || (n && !d_in)) return SM_ERR_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(ctx->device);
  smf_summary* d_sum = &((Results*)ctx->res.p)->sum;
  smf_summary sum;
  IndexMeta ix;
  // entries for a stream whose chunks average 1 KiB or more, or all the buffer already holds; a
  // stream of smaller chunks walks twice
  size_t entries = std::max<size_t>(ctx->idx.cap / kIndexEntryBound, n / 1024 + 64);
  entries = std::min<size_t>(entries, 0xffffffffu);
  for (int pass = 0;; ++pass) {
    SM_PASS(index_scratch(ctx, entries, ix));
    SM_CHECK(smf::launch_frame_index(d_in, n, &ix.ch, (uint32_t)entries, d_sum, s));
    SM_CHECK(hipMemcpyAsync(&sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s));
    SM_CHECK(hipStreamSynchronize(s));  // the documented synchronisation
    if (sum.status != SM_BUFFER_TOO_SMALL || pass) break;
    entries = sum.nchunks;
  }
  sm_status st = sum.status;
  if (st == SM_OK && sum.total_length > out_capacity) st = SM_BUFFER_TOO_SMALL;
  if (st != SM_OK) {
    SM_CHECK(smf::launch_frame_result(d_out_len, sum.total_length, nullptr, d_status, st, s));
    return st;
  }
  if (sum.nchunks && !d_out) return SM_ERR_ARGUMENT;
  return smf_uncompress_chunks_device(ctx, d_in, &ix.ch, sum.nchunks, d_out, out_capacity, ix.chunk_status, d_out_len,
                                      d_status, stream);
}

sm_status smf_compress(smf_ctx* ctx, const uint8_t* input, size_t n, uint8_t* framed, size_t* framed_length, int mode) {
  if (!ctx || !framed || !framed_length || (n && !input)) return SM_ERR_ARGUMENT;
  const size_t need = smf_max_framed_length(n);
  if (*framed_length < need) return SM_BUFFER_TOO_SMALL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  SM_CHECK(ctx->io_in.ensure(n));
  SM_CHECK(ctx->io_out.ensure(need));
  if (n) SM_CHECK(hipMemcpyAsync(ctx->io_in.p, input, n, hipMemcpyHostToDevice, s));
  LenStatus* d = &((Results*)ctx->res.p)->io;
  SM_PASS(smf_compress_device(ctx, (const uint8_t*)ctx->io_in.p, n, (uint8_t*)ctx->io_out.p, need, &d->len, &d->st, mode,
                              s));
  return finish(ctx, d, need, false, framed, framed_length, s);
}

// host index, upload, decode; output == null validates only (the decode goes to scratch)
static sm_status uncompress_host(smf_ctx* ctx, const uint8_t* framed, size_t n, uint8_t* output, size_t* length) {
  smf_summary sum;
  SM_PASS(smf_index(framed, n, nullptr, 0, &sum));
  if (length && sum.total_length > *length) {
    *length = (size_t)sum.total_length;
    return SM_BUFFER_TOO_SMALL;
  }
  const uint32_t nc = sum.nchunks;
  HostIndex hx;
  SM_PASS(hx.fill(framed, n, nc));
  const smf_chunks h = hx.view();
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  IndexMeta ix;
  SM_PASS(index_scratch(ctx, nc, ix));
  SM_CHECK(ctx->io_in.ensure(n));
  SM_CHECK(ctx->io_out.ensure((size_t)sum.total_length));
  SM_CHECK(hipMemcpyAsync(ctx->io_in.p, framed, n, hipMemcpyHostToDevice, s));
  SM_PASS(upload_chunks(ix.ch, h, 0, nc, s));
  LenStatus* d = &((Results*)ctx->res.p)->io;
  SM_PASS(smf_uncompress_chunks_device(ctx, (const uint8_t*)ctx->io_in.p, &ix.ch, nc, (uint8_t*)ctx->io_out.p,
                                       sum.total_length, ix.chunk_status, &d->len, &d->st, s));
  return finish(ctx, d, sum.total_length, false, output, length, s);
}

sm_status smf_uncompress(smf_ctx* ctx, const uint8_t* framed, size_t n, uint8_t* output, size_t* length) {
  if (!ctx || !length || (n && !framed) || (*length && !output)) return SM_ERR_ARGUMENT;
  return uncompress_host(ctx, framed, n, output, length);
}

sm_status smf_validate(smf_ctx* ctx, const uint8_t* framed, size_t n) {
  if (!ctx || (n && !framed)) return SM_ERR_ARGUMENT;
  return uncompress_host(ctx, framed, n, nullptr, nullptr);
}

sm_status smf_uncompress_range(smf_ctx* ctx, const uint8_t* framed, size_t n, uint64_t lo, uint64_t len,
                               uint8_t* output, size_t* out_len) {
  if (!ctx || !out_len || (n && !framed) || (*out_len && !output)) return SM_ERR_ARGUMENT;
  smf_summary sum;
  SM_PASS(smf_index(framed, n, nullptr, 0, &sum));
  if (lo + len < lo || lo + len > sum.total_length) return SM_ERR_ARGUMENT;
  if (len > *out_len) {
    *out_len = (size_t)len;
    return SM_BUFFER_TOO_SMALL;
  }
  *out_len = 0;
  if (len == 0) return SM_OK;
  const uint32_t nc = sum.nchunks;
  HostIndex hx;
  SM_PASS(hx.fill(framed, n, nc));
  const smf_chunks h = hx.view();
  std::vector<uint64_t>& pay_off = hx.pay_off;
  const std::vector<uint32_t>& pay_len = hx.pay_len;
  std::vector<uint64_t> chunk_off((size_t)nc + 1);
  SM_PASS(smf_chunk_offsets(hx.ulen.data(), nc, chunk_off.data()));
  // the touched chunks [f, f + k), their bytes in the stream, and the index slice rebased to them
  const smf::RangeChunks rc = smf::range_chunks(chunk_off.data(), nc, lo, len);
  if (rc.status != SM_OK || rc.count == 0) return SM_ERR_ARGUMENT;
  const uint32_t f = rc.first, k = rc.count;
  const uint64_t span0 = pay_off[f], span = pay_off[f + k - 1] + pay_len[f + k - 1] - span0, base = chunk_off[f];
  for (uint32_t c = f; c < f + k; ++c) pay_off[c] -= span0;
  for (uint32_t c = f; c <= f + k; ++c) chunk_off[c] -= base;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  IndexMeta ix;
  SM_PASS(index_scratch(ctx, k, ix));
  SM_CHECK(ctx->roff.ensure(8 * ((size_t)k + 1)));
  SM_CHECK(ctx->io_in.ensure((size_t)span));
  SM_CHECK(ctx->io_out.ensure((size_t)len));
  SM_CHECK(hipMemcpyAsync(ctx->io_in.p, framed + span0, (size_t)span, hipMemcpyHostToDevice, s));
  SM_PASS(upload_chunks(ix.ch, h, f, k, s));
  SM_CHECK(hipMemcpyAsync(ctx->roff.p, chunk_off.data() + f, 8 * ((size_t)k + 1), hipMemcpyHostToDevice, s));
  Results* res = (Results*)ctx->res.p;
  const uint64_t arg[3] = {lo - base, len, 0};  // lo, len, out_off
  uint64_t* d_arg = res->range;
  LenStatus* d = &res->range_out;
  SM_CHECK(hipMemcpyAsync(d_arg, arg, sizeof(arg), hipMemcpyHostToDevice, s));
  SM_PASS(smf_uncompress_ranges_device(ctx, (const uint8_t*)ctx->io_in.p, span, &ix.ch, (const uint64_t*)ctx->roff.p, k,
                                       d_arg, d_arg + 1, 1, k, (uint8_t*)ctx->io_out.p, d_arg + 2, &d->len, &d->st, s));
  // (the read-back's synchronisation also lets the pageable uploads above leave their host buffers)
  return finish(ctx, d, len, true, output, out_len, s);
}

// ---- a batch of streams from host buffers (../common/smc_staging.h) ------------------------------
sm_status smf_compress_streams(smf_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                               uint32_t nstreams, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                               int32_t* status, int mode) {
  if (!ctx || nstreams > smf::kMaxStreams || !valid_mode(mode)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in_off || !in_len || !out || !out_off || !out_len || !status) return SM_ERR_ARGUMENT;
  uint64_t blocks = 0;
  std::vector<uint64_t> room(nstreams);
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (in_len[r] && !in) return SM_ERR_ARGUMENT;
    blocks += smf::stream_blocks(in_len[r]);
    if (blocks > smf::kMaxStreams) return SM_ERR_INPUT_TOO_LARGE;
    room[r] = smf_max_framed_length((size_t)in_len[r]);
  }
  const StreamStaging h(in, in_off, in_len, nstreams, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, nullptr, nstreams, d));
  SM_PASS(smf_compress_streams_device(ctx, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nstreams, (uint32_t)blocks,
                                      (uint8_t*)ctx->io_out.p, d.out_off, d.out_len, d.status, mode, ctx->stream));
  std::vector<uint8_t> framed;
  SM_PASS(download_stream_call(b, h, d, nstreams, out_len, status, framed));
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (out_len[r] > room[r]) return SM_ERR_DEVICE;
    memcpy(out + out_off[r], framed.data() + h.out_off[r], (size_t)out_len[r]);
  }
  return SM_OK;
}

sm_status smf_uncompress_streams(smf_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                 uint32_t nstreams, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                 uint64_t* out_len, int32_t* status) {
  if (!ctx || nstreams > smf::kMaxStreams) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return SM_ERR_ARGUMENT;
  // the plan on the host: the slots, and the room each decoded stream needs on the device
  std::vector<uint64_t> room(nstreams);
  uint64_t chunks = 0;
  const sm_status planned = smf_streams_plan(in, in_off, in_len, nstreams, out_cap, smf::kMaxStreams, nullptr, room.data(),
                                             status, &chunks);
  if (planned != SM_OK) return planned == SM_BUFFER_TOO_SMALL ? (sm_status)SM_ERR_INPUT_TOO_LARGE : planned;
  for (uint32_t r = 0; r < nstreams; ++r) {
    if (status[r] != SM_OK) room[r] = 0;  // (not decoded)
    if (room[r] && !out) return SM_ERR_ARGUMENT;
  }
  const StreamStaging h(in, in_off, in_len, nstreams, room.data());
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const StagingBufs b{ctx->io_in, ctx->io_out, ctx->sarg, ctx->stream};
  StreamCallArrays d;
  SM_PASS(upload_stream_call(b, h, in_len, out_cap, nstreams, d));
  SM_PASS(smf_uncompress_streams_device(ctx, (const uint8_t*)ctx->io_in.p, d.in_off, d.in_len, nstreams, (uint32_t)chunks,
                                        (uint8_t*)ctx->io_out.p, d.out_off, d.out_cap, d.out_len, d.status, nullptr,
                                        nullptr, ctx->stream));
  std::vector<uint8_t> decoded;
  SM_PASS(download_stream_call(b, h, d, nstreams, out_len, status, decoded));
  for (uint32_t r = 0; r < nstreams; ++r)
    if (room[r]) memcpy(out + out_off[r], decoded.data() + h.out_off[r], (size_t)room[r]);
  return SM_OK;
}

}  // extern "C"
