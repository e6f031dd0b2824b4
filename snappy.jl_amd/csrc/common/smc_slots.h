// smc_slots.h -- the slot rules the container libraries' batched calls share (framing, blocks, orc,
// parquet, avro, table): a call has groups (streams, chunks, tables) whose items (chunks, pages,
// blocks) take slots up to the caller's bound.  Here: the plan's two words, the owner of a slot in
// the scan of the groups' counts, a group's verdict over its slots, and the tiling of the copies.
// Plain functions, compiled for the host and the device alike, so the host checkers test the code
// the kernels run.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../../include/snappy_mi355x.h"
#include "smc_layout.h"

namespace smc {

constexpr uint32_t kNoSlot = 0xffffffffu;  // a slot of no group; a group without a failing slot

struct PlanHeader {  // a plan's words for the kernels behind it
  uint32_t total;    // slots in use (0 over the bound: nothing is decoded or packed)
  uint32_t over;     // the groups need more slots than the caller's bound
};

SMC_HD constexpr uint64_t round16(uint64_t n) { return (n + 15) / 16 * 16; }

// The owner of slot j in the exclusive scan first[0, n]: first[r] <= j < first[r + 1] (of equal
// entries the last one, so owners without slots are passed over).  j < first[n].
SMC_HD inline uint32_t slot_owner(const uint32_t* first, uint32_t n, uint32_t j) {
  uint32_t lo = 0, hi = n;  // first[lo] <= j < first[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A group's status: SM_ERR_ARGUMENT over the caller's bound, else the plan's, else its first
// failing slot's (fail == kNoSlot: none failed).
SMC_HD inline int32_t plan_verdict(bool over, int32_t pre, uint32_t fail, int32_t fail_status) {
  if (over) return SM_ERR_ARGUMENT;
  if (pre != SM_OK) return pre;
  return fail != kNoSlot ? fail_status : (int32_t)SM_OK;
}

// ---- the copies' grid -----------------------------------------------------------------------------
// A slot's bytes are copied in tiles of kCopyTile bytes, tile t by the workgroups of row t mod rows
// (copy_tiled in smc_device.h).  With many slots one row does (a workgroup a slot); with few, a
// long slot is spread over as many rows as fill the device (kCopyGroups workgroups), at most one
// per tile of the longest slot the caller expects (a longer one is strided).
constexpr uint32_t kCopyTile = 16384;
constexpr uint32_t kCopyGroups = 2048;  // 256 CUs x 8 workgroups

SMC_HD inline uint32_t copy_rows(uint32_t slots, uint32_t longest) {
  const uint32_t tiles = longest / kCopyTile + (longest % kCopyTile ? 1 : 0);
  const uint32_t want = slots ? kCopyGroups / slots : kCopyGroups;
  const uint32_t rows = tiles < want ? tiles : want;
  return rows ? rows : 1;
}

}  // namespace smc
