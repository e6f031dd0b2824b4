// smk_internal.h -- launcher interfaces between the Kafka segment library's C ABI (smk_api.hip) and
// its kernels (smk_kernels.hip).  Not part of the public ABI.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smk_format.h"

namespace smk {

// what both calls' walks take: the segments, the bound on the batches and the walks' arrays
struct WalkArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;  // per segment
  uint32_t ns, m;                   // m = max_batches
  Header* hdr;
  Segments g;
  Batches b;
  uint32_t* batch_first;  // optional
};
// the counting walk, the scan against m, the storing walk
hipError_t launch_walk(const WalkArgs& w, hipStream_t s);

struct DecodeArgs {
  WalkArgs w;
  uint32_t verify;
  uint8_t* out;
  const uint64_t *out_off, *out_cap;  // per segment
  uint64_t* out_len;
  int32_t* status;
  uint64_t *batch_in_off, *batch_out_off, *batch_len;  // optional
  uint32_t* batch_codec;                               // optional
  int32_t* batch_status;                               // optional
  Decode s;
};
// the heads, a thread per batch, with the snappy-java batches as streams of no room
hipError_t launch_heads(const DecodeArgs& a, hipStream_t s);
// behind the sizing call: the scan of the rewritten lengths, the segments' plans, the slots
hipError_t launch_decode_plan(const DecodeArgs& a, hipStream_t s);
// behind the snappy-java decode: more chunks than the bound takes every other slot's work away
hipError_t launch_gate(const DecodeArgs& a, hipStream_t s);
// the stored batches' tiled copy and the 61 header bytes of every written batch
hipError_t launch_decode_pack(const DecodeArgs& a, hipStream_t s);
// m batches: the four bytes of crc[j] in front of out[crc_off[j]], big-endian, where crc_len[j] is not 0
hipError_t launch_crc_store(uint8_t* out, const uint64_t* crc_off, const uint32_t* crc_len, const uint32_t* crc, uint32_t m,
                            hipStream_t s);
// the batches' verdicts and the segments' results
hipError_t launch_decode_result(const DecodeArgs& a, hipStream_t s);

struct CompressArgs {
  WalkArgs w;
  uint32_t max_blocks;
  uint64_t stage_bytes;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  int32_t* status;
  Compress s;
};
// the payloads against the bounds with the scan of the stage, then per batch its stream
hipError_t launch_compress_plan(const CompressArgs& a, hipStream_t s);
// behind smb_compress_streams_device: the scan of the sizes, the pack
hipError_t launch_compress_pack(const CompressArgs& a, hipStream_t s);
// behind the checksums (launch_crc_store): the segments' results
hipError_t launch_compress_result(const CompressArgs& a, hipStream_t s);

}  // namespace smk
