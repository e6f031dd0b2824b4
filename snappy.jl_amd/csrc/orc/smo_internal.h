// smo_internal.h -- launcher interfaces between the ORC C ABI (smo_api.hip) and its kernels
// (smo_kernels.hip).  Not part of the public ABI.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smo_format.h"
#include "smo_streams.h"

namespace smo {

struct DecodeStreamsArgs {
  uint32_t block_size;
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nstreams, m;  // m = max_chunks: the slots
  uint8_t* out;
  const uint64_t *out_off, *out_cap;
  uint64_t* out_len;
  int32_t* status;
  uint32_t* chunk_first;  // optional
  int32_t* chunk_status;  // optional
  DecodeStreams s;
};
// the counting walk, the scan of the slots against m, the storing walk with the slots no chunk took
hipError_t launch_decode_plan(const DecodeStreamsArgs& a, hipStream_t s);
// behind the two smm calls: the stored chunks' copies and the slots' verdicts (m > 0), then the
// streams' results
hipError_t launch_decode_result(const DecodeStreamsArgs& a, hipStream_t s);

struct CompressStreamsArgs {
  uint32_t block_size;
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nstreams, m;  // m = max_pieces: the slots
  const uint8_t* slots;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  int32_t* status;
  CompressStreams s;
};
// the scan of the streams' piece counts against m, then per piece its stream, input and slot
hipError_t launch_compress_plan(const CompressStreamsArgs& a, hipStream_t s);
// behind smm_compress_device: the choice and the scan of the chunk sizes, the packed chunks, then
// per stream the length and the status
hipError_t launch_compress_pack(const CompressStreamsArgs& a, hipStream_t s);

}  // namespace smo
