// smm_index.hip -- the fragment index of a batch of raw streams, built on the device
// (smm_index_device; the rule: smm_plan.h index_count / index_walk).
//
// k_index_count: one workgroup scans the streams' entry counts into d_frag_first and finishes every
// stream that needs no walk (no entries, or at most 64 KiB: its one entry is the varint's length).
// k_index_walk: one workgroup of two waves per stream that declares more than 64 KiB.  Wave 0 walks
// the tag sizes out of LDS, a 256-byte window at a time, with the decoder's own window walk
// (../sm_dec_walk.h); wave 1 stages the stream into LDS in pieces of kIndexStage bytes, the next
// piece while wave 0 walks the current one, so that the serial chain waits for HBM once per stream
// and not once per window.  Nothing is copied and no offset is checked: the index is a hint that
// smm_uncompress_device verifies by decoding.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "../sm_dec_walk.h"
#include "smm_plan.h"

namespace smm {

namespace {

using smc::block_scan;
using smc::sat32;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWalkThreads = 128;  // wave 0 walks, wave 1 stages
// A window that starts below kIndexStage reads its 256 bytes and a tag's 8 behind them, in aligned
// dwords (lds_ld64: 12 bytes from the dword below): under kIndexStage + 268.
constexpr uint32_t kPiecePad = 320;
constexpr uint32_t kPiece = kIndexStage + kPiecePad;
static_assert(kIndexStage % 16 == 0 && kIndexStage >= 1024, "a piece is a multi-KiB run of whole dwords");

enum : uint32_t { kWalking = 0, kBuilt = 1, kFailed = 2 };

}  // namespace

// Thread i serves stream i of each tile of 256.  The total is known only behind the last tile, so
// the per-stream results follow in a second sweep, each thread over the streams it scanned.
__global__ __launch_bounds__(kThreads) void k_index_count(IndexPlan p) {
  __shared__ uint64_t sh[4];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < p.n; base += kThreads) {  // (uniform: every thread takes every tile)
    const uint32_t s = base + threadIdx.x;
    uint32_t cnt = 0;
    if (s < p.n) {
      const IndexCount c = index_count(p.in + p.in_off[s], p.in_len[s], p.out_cap ? p.out_cap[s] : 0xffffffffu);
      p.s.D[s] = c.D;
      p.s.hv[s] = c.hv;
      cnt = c.count;
    }
    uint64_t t;
    const uint64_t ex = block_scan(cnt, sh, t);
    if (s < p.n) p.frag_first[s] = sat32(carry + ex);
    carry += t;
  }
  const bool stop = carry > p.m;  // (every thread holds the total)
  if (threadIdx.x == 0) {
    p.frag_first[p.n] = stop ? 0u : (uint32_t)carry;
    *p.s.stop = stop;
  }
  for (uint32_t s = threadIdx.x; s < p.n; s += kThreads) {
    p.status[s] = stop ? SM_ERR_ARGUMENT : SM_OK;
    p.built[s] = 0;
    if (stop) {
      p.frag_first[s] = 0;
    } else {
      const uint32_t D = p.s.D[s];
      if (D != 0 && D <= kBlock) p.frag_pos[p.frag_first[s]] = p.s.hv[s];  // (its own store above)
    }
  }
}

// blockIdx.x = the stream.  Every branch around a barrier is uniform over the workgroup: it depends
// on the arguments, or on what wave 0 left in LDS before the barrier in front of it.
__global__ __launch_bounds__(kWalkThreads) void k_index_walk(IndexPlan p) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[2][kPiece];
  __shared__ __attribute__((aligned(16))) uint16_t jt[sm::kJt];
  __shared__ uint64_t s_x[2];      // wave 0's position and verdict behind a piece, by the round's parity:
  __shared__ uint32_t s_state[2];  // a slot is written again two barriers after it was read
  const uint32_t s = blockIdx.x, lane = sm::lane_id(), w = threadIdx.x >> 6;
  if (*p.s.stop) return;
  const uint32_t D = p.s.D[s];
  if (D <= kBlock) return;
  const uint8_t* const in = p.in + p.in_off[s];
  const uint32_t N = p.in_len[s], count = fragment_count(D);
  uint32_t* const pos = p.frag_pos + p.frag_first[s];  // count entries: the scan's total is at most p.m

  uint64_t start = p.s.hv[s];  // buf[cur] holds the stream's bytes [start, start + kPiece), zero past N
  uint64_t x = start, o = 0;   // the next tag and the output before it (wave 0's; x is shared behind a round)
  uint32_t f = 0, cur = 0, state = kWalking;
  if (w == 1) sm::stage_bytes(buf[0], in, N, (uint32_t)start, kPiece, lane);  // (start <= 5, N >= 1: the header parsed)
  __syncthreads();
  for (uint32_t round = 0;; ++round) {
    if (w == 1) {
      // the next piece, while wave 0 walks this one (no tag starts at or past N: then nobody reads it)
      if (start + kIndexStage < N) sm::stage_bytes(buf[cur ^ 1], in, N, (uint32_t)(start + kIndexStage), kPiece, lane);
    } else {
      const uint8_t* const b = buf[cur];
      for (;;) {
        if (x >= N) {
          state = kFailed;
          break;
        }
        if (x - start >= kIndexStage) break;  // behind this piece
        const uint32_t rel0 = (uint32_t)(x - start);
        const uint64_t at = (uint64_t)kBlock * f;  // the output at which fragment f's first tag must start
        uint32_t rel, next, ob, excl;
        const uint32_t ntok = sm::window_tags(b, rel0, (uint32_t)min((uint64_t)N - x, (uint64_t)256), jt, lane, rel, next, ob, excl);
        if (ntok == 0) {  // a literal the window walk leaves alone: one scalar step, any length
          if (o > at) {
            state = kFailed;
            break;
          }
          if (o == at) {
            if (lane == 0) pos[f] = (uint32_t)x;
            if (++f == count) {
              state = kBuilt;
              break;
            }
          }
          const sm::Tag t = sm::tag_at(b, rel0);
          const uint64_t size = t.size();
          o += sm::uniform(t.out_bytes());
          x += ((uint64_t)sm::uniform((uint32_t)(size >> 32)) << 32) | sm::uniform((uint32_t)size);
          continue;
        }
        // At most one multiple of 65536 lies inside a window's output (64 tags of at most 200 bytes),
        // and the first tag at or behind it must start on it.
        const uint64_t hit = sm::ballot(lane < ntok && o + excl >= at);
        if (hit) {
          const uint32_t t = sm::ctz64(hit);
          if (o + sm::readlane(excl, t) != at) {
            state = kFailed;
            break;
          }
          if (lane == 0) pos[f] = (uint32_t)(start + sm::readlane(rel, t));
          if (++f == count) {
            state = kBuilt;
            break;
          }
        }
        o += sm::readlane(excl + ob, ntok - 1);
        x = start + sm::readlane(next, ntok - 1);
      }
      if (lane == 0) {
        s_x[round & 1] = x;
        s_state[round & 1] = state;
      }
    }
    __syncthreads();
    const uint64_t xs = s_x[round & 1];
    x = ((uint64_t)sm::uniform((uint32_t)(xs >> 32)) << 32) | sm::uniform((uint32_t)xs);
    state = sm::uniform(s_state[round & 1]);
    if (state != kWalking) break;
    if (x - start < 2 * (uint64_t)kIndexStage) {  // inside the piece wave 1 has just staged (x < N here)
      start += kIndexStage;
      cur ^= 1;
    } else {  // a long literal went past it: stage again where it ended
      start = x;
      if (w == 1) sm::stage_bytes(buf[cur], in, N, (uint32_t)start, kPiece, lane);
      __syncthreads();
    }
  }
  if (w != 0) return;
  if (state == kBuilt) {
    if (lane == 0) p.built[s] = 1;
    return;
  }
  __threadfence();  // the zeros below land behind lane 0's positions
  for (uint32_t k = lane; k < count; k += smc::kWave) pos[k] = 0;
}

hipError_t launch_index(const IndexPlan& p, hipStream_t st) {
  hipLaunchKernelGGL(k_index_count, dim3(1), dim3(kThreads), 0, st, p);
  hipLaunchKernelGGL(k_index_walk, dim3(p.n), dim3(kWalkThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace smm
