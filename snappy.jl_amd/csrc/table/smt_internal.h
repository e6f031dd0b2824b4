// smt_internal.h -- launcher interfaces between the table library's C ABI (smt_api.hip) and its
// kernels (smt_kernels.hip).  Not part of the public ABI.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smt_format.h"

namespace smt {

// smt_index_tables_device and smt_uncompress_tables_device (decode set) and, with nt == 0,
// smt_uncompress_blocks_device, whose m blocks come by the caller's handles
struct DecodeArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;  // per table
  uint32_t nt, m;                   // m = max_blocks: the entries
  uint64_t index_bytes;
  uint32_t verify;
  bool decode;  // the tables call: blocks are decoded behind the index stage
  const uint64_t *out_off, *out_cap;  // per table (per block for the handle-level call)
  uint64_t* out_len;
  int32_t* status;
  uint32_t* block_first;                   // optional
  uint64_t *handle_off, *handle_size;      // optional
  uint64_t *block_out_off, *block_len;     // optional
  int32_t* block_status;                   // optional
  const uint64_t *blk_off, *blk_size;      // the handle-level call's trusted handles
  Decode s;
};

// the footers with the index blocks' heads, the scan that places the index blocks in the scratch
hipError_t launch_index_heads(const DecodeArgs& a, hipStream_t s);
// behind the index blocks' decode and checksum: the stored index blocks' copy, the verdicts, the
// counting walk, the scan against m, the storing walk; the index call's results (decode not set)
hipError_t launch_index_walk(const DecodeArgs& a, hipStream_t s);
// the tables call: the blocks' heads, the scan of the declared lengths, the tables' plans, the slots
hipError_t launch_block_plan(const DecodeArgs& a, hipStream_t s);
// the handle-level call: the blocks' heads and slots
hipError_t launch_handle_plan(const DecodeArgs& a, hipStream_t s);
// the stored blocks' tiled copy
hipError_t launch_block_copy(const DecodeArgs& a, uint8_t* out, hipStream_t s);
// behind the decode and the checksums: the blocks' verdicts and (tables call) the tables' results
hipError_t launch_block_result(const DecodeArgs& a, hipStream_t s);

struct CompressArgs {
  const uint8_t* in;
  const uint32_t* block_first;
  const uint64_t* block_off;
  const uint32_t* block_len;
  uint32_t nt, m;
  uint64_t stage_bytes;
  uint32_t max_fragments;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t *handle_off, *handle_size;
  uint64_t* out_len;
  int32_t* status;
  Compress s;
};
// the blocks against the three bounds with the scan of the stage, then per slot its arguments
hipError_t launch_compress_plan(const CompressArgs& a, hipStream_t s);
// behind smm_compress_device: the 12.5 % decision with the scan of the sizes, the pack
hipError_t launch_compress_pack(const CompressArgs& a, hipStream_t s);
// behind smf_crc32c_batch_device: the checksum bytes, the tables' results
hipError_t launch_compress_result(const CompressArgs& a, hipStream_t s);

}  // namespace smt
