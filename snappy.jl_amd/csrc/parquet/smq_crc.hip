// smq_crc.hip -- CRC-32 (IEEE) of byte ranges of any length on gfx950: the page checksum pass of
// smq_uncompress_chunks_device and smq_crc32_device (smq_internal.h).  The rules and the table
// arithmetic are smq_crc.h's; here are the kernels: a range is cut into segments of kCrcSegment
// bytes, the short one first, one workgroup a segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smq_chunks.h"
#include "smq_crc.h"
#include "smq_internal.h"

namespace smq {

namespace {

using smc::kWave;

constexpr uint32_t kCrcGroups = 2048;  // 256 CUs x 8 workgroups (20.5 KiB of LDS each)

__device__ inline uint32_t job_len(const CrcJobs& j, uint32_t i) {
  if (j.len) return j.len[i];
  const uint64_t n = j.len64[i];
  return n > 0x7fffffffull ? 0x7fffffffu : (uint32_t)n;
}

}  // namespace

// Segment g of the call (grid-strided, so the tables are staged in LDS once per workgroup) belongs
// to job i = smc::slot_owner(seg_first, g) and is its segment g - seg_first[i].  Within the segment, as
// in the framing library's CRC-32C: lane t takes the 16-byte granules at distance t, t + 256, ...
// from the last one as coalesced 16-byte loads -- a lane's register, 256 granules old, is advanced
// by four lookups and the new granule enters by sixteen, all independent -- and moves its register
// to the granules' end (crc_lane_granules); the lane with the fewest granules runs the segment's
// init through the head bytes (crc_head); the registers add up (xor) over the workgroup; the tail
// runs bytewise behind the sum.  The segment's register is then moved over the whole segments behind
// it (crc_shift_segments) and added to its job's by an atomic xor: the order of the segments does
// not matter, and a job's register is complete when the kernel is.
__global__ __launch_bounds__(kCrcThreads) void k_crc32_segments(CrcJobs j, const CrcLut* __restrict__ T) {
  __shared__ uint32_t tab[kCrcTabs * 256];
  __shared__ uint32_t red[kCrcThreads / kWave];
  const uint32_t nseg_all = j.hdr->segments, njobs = j.hdr->total;
  if (blockIdx.x >= nseg_all) return;  // (the whole workgroup: no barrier is left behind)
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t i = t; i < kCrcTabs * 256; i += kCrcThreads) tab[i] = (&T->tab[0][0])[i];
  __syncthreads();
  for (uint32_t g = blockIdx.x; g < nseg_all; g += gridDim.x) {
    const uint32_t i = smc::slot_owner(j.seg_first, njobs, g), k = g - j.seg_first[i];
    const uint32_t n = job_len(j, i), nseg = crc_segments(n);
    const uint32_t len = crc_segment_len(n, k);
    const uint8_t* p = j.in + j.off[i] + crc_segment_start(n, k);
    const CrcSplit sp = crc_split(p, len);
    uint32_t s = t < sp.G ? crc_lane_granules(tab, T, p + sp.head, sp.G, t) : 0u;
    if (t == kCrcThreads - 1) s ^= crc_head(tab, T, p, sp, k == 0 ? 0xffffffffu : 0u);
    for (uint32_t d = 1; d < kWave; d <<= 1) s ^= (uint32_t)__shfl_xor((int)s, (int)d, kWave);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (t == 0) {
      const uint32_t c = crc_tail(tab, p, len, sp, red[0] ^ red[1] ^ red[2] ^ red[3]);
      atomicXor(&j.acc[i], crc_shift_segments(T, c, nseg - 1 - k));
    }
    __syncthreads();  // (red is read before the next segment's sums land)
  }
}

hipError_t launch_crc_segments(const CrcJobs& j, const CrcLut* T, hipStream_t s) {
  // the number of segments is the device's: workgroups beyond it return at once
  hipLaunchKernelGGL(k_crc32_segments, dim3(kCrcGroups), dim3(kCrcThreads), 0, s, j, T);
  return hipGetLastError();
}

// ---- smq_crc32_device ------------------------------------------------------------------------------
// the scan of the ranges' segments, by one workgroup, and the registers' zeros
__global__ __launch_bounds__(256) void k_crc32_plan(CrcJobs j, CrcRanges r) {
  __shared__ uint64_t sh[4];
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < j.njobs; b0 += 256) {  // (uniform: every thread takes every tile)
    const uint32_t i = b0 + threadIdx.x;
    const uint64_t v = i < j.njobs ? crc_segments(job_len(j, i)) : 0u;
    uint64_t total;
    const uint64_t ex = smc::block_scan(v, sh, total);
    if (i < j.njobs) {
      r.seg_first[i] = smc::sat32(carry + ex);
      r.acc[i] = 0;
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    r.seg_first[j.njobs] = smc::sat32(carry);
    r.hdr->total = j.njobs;
    r.hdr->over = 0;
    r.hdr->segments = smc::sat32(carry);
  }
}

__global__ __launch_bounds__(256) void k_crc32_finish(CrcJobs j, uint32_t* __restrict__ crc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= j.njobs) return;
  crc[i] = job_len(j, i) ? ~j.acc[i] : 0u;  // (the CRC of nothing is 0)
}

hipError_t launch_crc_ranges(const uint8_t* in, const uint64_t* off, const uint64_t* len, uint32_t n, uint32_t* crc,
                             const CrcRanges& r, const CrcLut* T, hipStream_t s) {
  const CrcJobs j{in, off, nullptr, len, r.seg_first, n, r.hdr, r.acc};
  hipLaunchKernelGGL(k_crc32_plan, dim3(1), dim3(256), 0, s, j, r);
  hipLaunchKernelGGL(k_crc32_segments, dim3(kCrcGroups), dim3(kCrcThreads), 0, s, j, T);
  hipLaunchKernelGGL(k_crc32_finish, dim3((n + 255) / 256), dim3(256), 0, s, j, crc);
  return hipGetLastError();
}

}  // namespace smq
