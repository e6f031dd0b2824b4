// smq_internal.h -- launcher interfaces between the Parquet page library's C ABI (smq_api.hip) and
// its kernels (smq_kernels.hip, smq_crc.hip).  Not part of the public ABI.  All pointers are device
// pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smq_chunks.h"
#include "smq_crc.h"
#include "smq_format.h"

namespace smq {

struct DecodeChunksArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nchunks, m;  // m = max_pages: the slots
  uint32_t verify_crc;
  uint8_t* out;
  const uint64_t *out_off, *out_cap;
  uint64_t* out_len;
  int32_t* status;
  uint32_t* page_first;  // optional
  int32_t* page_status;  // optional
  bool table;            // pages is given
  smq_pages pages;
  DecodeChunks s;
};
// the counting walk, the scan of the slots against m, the storing walk with the slots no page took,
// and with verify_crc the scan of the slots' CRC segments
hipError_t launch_decode_plan(const DecodeChunksArgs& a, hipStream_t s);
// behind the two smm calls: the copies, the CRC segments and the slots' verdicts (m > 0), then the
// chunks' results
hipError_t launch_decode_result(const DecodeChunksArgs& a, const CrcLut* T, hipStream_t s);

// ---- the encoder (smq_encode.hip) ----------------------------------------------------------------------
struct EncodeChunksArgs {
  const uint8_t* in;
  const uint64_t *in_off, *in_len;
  uint32_t nchunks, m;   // m = max_pages: the slots
  uint64_t stage_bytes;  // the caller's bound on the stage
  uint32_t max_fragments;
  uint8_t* out;
  const uint64_t *out_off, *out_cap;
  uint64_t* out_len;
  int32_t* status;
  uint32_t* page_first;  // optional
  int32_t* page_status;  // optional
  bool table;            // pages is given
  smq_pages pages;
  EncodeChunks s;
};
// the counting walk, the scan of the slots against m, the storing walk with the slots no page took,
// the scan of the stage slots and the fragments against their bounds
hipError_t launch_encode_plan(const EncodeChunksArgs& a, hipStream_t s);
// behind smm_compress_device: the level bytes to their slots' fronts, the new bodies' lengths and the
// pages' statuses, the CRC segments, the sizes with the chunks' results, the pack
hipError_t launch_encode_result(const EncodeChunksArgs& a, const CrcLut* T, hipStream_t s);

// CRC-32 of jobs (ranges or slots): job j is in[off[j] .. +len[j]) with its segments numbered from
// seg_first[j]; hdr->segments = seg_first[njobs].  Adds every segment's share to acc[j] (zero before).
struct CrcJobs {
  const uint8_t* in;
  const uint64_t* off;
  const uint32_t* len;      // u32 lengths (the slots'), or NULL
  const uint64_t* len64;    // u64 lengths (smq_crc32_device's), when len is NULL
  const uint32_t* seg_first;
  uint32_t njobs;
  const Header* hdr;
  uint32_t* acc;
};
hipError_t launch_crc_segments(const CrcJobs& j, const CrcLut* T, hipStream_t s);
// smq_crc32_device: the scan of the ranges' segments, the segments, the complement
hipError_t launch_crc_ranges(const uint8_t* in, const uint64_t* off, const uint64_t* len, uint32_t n, uint32_t* crc,
                             const CrcRanges& r, const CrcLut* T, hipStream_t s);

}  // namespace smq
