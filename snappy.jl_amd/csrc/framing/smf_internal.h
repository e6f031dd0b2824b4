// smf_internal.h -- launcher interfaces between the framing C ABI (smf_api.hip) and its kernels
// (smf_kernels.hip, smf_range.hip, smf_streams.hip; their shared device helpers: smf_device.h).
// Not part of the public ABI.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smf_format.h"
#include "smf_range.h"
#include "smf_slots.h"
#include "smf_streams.h"

namespace smf {

hipError_t launch_crc32c(const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t nblk, uint32_t* crc,
                         int masked, const CrcLut* T, hipStream_t s);

// compress: the blocks of an n-byte input and their slots; then, behind the raw compressor and the
// CRC pass, the chunk types and places (*out_len, *status) and the packed stream
hipError_t launch_frame_compress_plan(uint64_t n, uint32_t nblk, uint64_t pitch, uint64_t* in_off, uint32_t* in_len,
                                      uint64_t* slot_off, hipStream_t s);
struct PackArgs {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  const uint8_t* slots;
  const uint64_t* slot_off;
  const uint32_t* comp_len;
  const uint32_t* crc;
  uint8_t* type;
  uint64_t* dst_off;
  uint32_t nblk;
  uint8_t* dst;
};
hipError_t launch_frame_pack(const PackArgs& a, uint64_t* out_len, int32_t* status, hipStream_t s);

// index: ch == null counts only
hipError_t launch_frame_index(const uint8_t* in, uint64_t n, const smf_chunks* ch, uint32_t max_chunks, smf_summary* sum,
                              hipStream_t s);
// *d_len / *d_status = (len, status), or with sum the walk's total and status
hipError_t launch_frame_result(uint64_t* d_len, uint64_t len, const smf_summary* sum, int32_t* d_status, int32_t status,
                               hipStream_t s);

// smf_uncompress_chunks_device's plan: places, the raw decoder's arguments and pre; *sl.fail = none
hipError_t launch_frame_plan(const smf_chunks& ch, uint32_t nchunks, uint64_t out_capacity, const Slots& sl,
                             uint64_t* out_len, hipStream_t s);
// the slot stage's own kernels (m > 0): the 0x01 slots' copies, the slots' verdicts; then the groups'
hipError_t launch_slot_copy(const uint8_t* in, uint8_t* out_base, const Slots& sl, uint32_t m, hipStream_t s);
hipError_t launch_slot_verify(const Slots& sl, uint32_t m, hipStream_t s);
hipError_t launch_group_result(const Slots& sl, const Groups& g, hipStream_t s);

// ---- smf_range.hip: the seek index and the ranged decode ------------------------------------
// chunk_off[0, nchunks] = the exclusive scan of ulen
hipError_t launch_chunk_offsets(const uint32_t* ulen, uint32_t nchunks, uint64_t* chunk_off, hipStream_t s);
// behind launch_frame_pack: the encoder's index of the stream it packed
hipError_t launch_frame_index_out(const PackArgs& a, uint64_t n, const smf_chunks& ch, uint64_t* chunk_off,
                                  uint32_t* nchunks, const int32_t* status, hipStream_t s);

struct RangeArgs {
  const uint8_t* in;
  uint64_t n;
  smf_chunks ch;
  const uint64_t* chunk_off;
  uint32_t nchunks;
  const uint64_t* lo;
  const uint64_t* len;
  uint32_t nranges, m;  // m = max_range_chunks: the slots
  uint8_t* out;
  const uint64_t* out_off;
  uint8_t* edge;  // 2 nranges edge slots of kEdgePitch bytes: the raw decoder's and the CRC pass's base
  RangeScratch s;
};
// per range its chunks, the scan of the counts against m, per slot the raw decoder's arguments
hipError_t launch_range_plan(const RangeArgs& a, hipStream_t s);
// behind the slot stage: the edge slots' covered bytes
hipError_t launch_range_trim(const RangeArgs& a, hipStream_t s);

// ---- smf_streams.hip: a batch of framed streams per call -------------------------------------
struct DecodeStreamsArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nstreams, m;  // m = max_chunks: the slots
  uint8_t* out;
  const uint64_t *out_off, *out_cap;
  uint32_t* chunk_first;  // optional
  DecodeStreams s;
};
// the counting walk, the scan of the slots against m, the storing walk and the unused slots
hipError_t launch_streams_plan(const DecodeStreamsArgs& a, hipStream_t s);

struct CompressStreamsArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nstreams, m;  // m = max_blocks: the slots
  const uint8_t* slots;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  int32_t* status;
  CompressStreams s;
};
// the scan of the streams' block counts against m, then per block its stream, input and slot
hipError_t launch_cstreams_plan(const CompressStreamsArgs& a, hipStream_t s);
// behind the raw compressor and the CRC pass: types and places, the packed chunks, then per stream
// the identifier, the length and the status
hipError_t launch_cstreams_pack(const CompressStreamsArgs& a, hipStream_t s);

}  // namespace smf
