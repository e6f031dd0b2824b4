// sma_internal.h -- launcher interfaces between the Avro library's C ABI (sma_api.hip) and its
// kernels (sma_kernels.hip).  Not part of the public ABI.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sma_format.h"
#include "sma_streams.h"

namespace sma {

struct DecodeStreamsArgs {
  int kind;
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  const uint8_t* sync;   // SMA_INPUT_BLOCKS: 16 bytes per stream
  uint32_t nstreams, m;  // m = max_blocks: the slots
  uint32_t verify_crc;
  const uint64_t *out_off, *out_cap;
  uint64_t* out_len;
  int32_t* status;
  uint64_t* objects;      // optional
  uint32_t* block_first;  // optional
  int32_t* block_status;  // optional
  bool table;             // blocks is given
  sma_blocks blocks;
  DecodeStreams s;
};
// the counting walk, the scan of the slots against m, the storing walk with the slots no block took
hipError_t launch_decode_plan(const DecodeStreamsArgs& a, hipStream_t s);
// behind the two smm calls and the CRC call: the slots' verdicts (m > 0), then the streams' results
hipError_t launch_decode_result(const DecodeStreamsArgs& a, hipStream_t s);

struct FindSyncArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  const uint8_t* sync;
  const uint32_t* q_stream;
  const uint64_t* q_from;
  uint32_t nqueries;
  uint64_t* pos;
};
// every answer set to its stream's length, then the tiles' bids
hipError_t launch_find_sync(const FindSyncArgs& a, hipStream_t s);

struct CompressStreamsArgs {
  const uint8_t* in;
  const uint32_t* block_first;
  const uint64_t* block_off;
  const uint32_t* block_len;
  const uint64_t* block_count;
  const uint8_t* sync;
  const uint64_t *head_off, *head_len;  // both or neither
  uint32_t nstreams, m;                 // m = max_blocks: the slots
  uint64_t stage_bytes;
  uint32_t max_fragments;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  int32_t* status;
  CompressStreams s;
};
// the blocks against the three bounds with the scan of the stage, then per slot its arguments
hipError_t launch_compress_plan(const CompressStreamsArgs& a, hipStream_t s);
// behind smm_compress_device and smq_crc32_device: the scan of the block sizes, the packed blocks,
// then per stream its header, the length and the status
hipError_t launch_compress_pack(const CompressStreamsArgs& a, hipStream_t s);

}  // namespace sma
