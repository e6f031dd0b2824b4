// smf_slots.h -- the slot stage of the three decode entry points (smf_uncompress_chunks_device,
// smf_uncompress_ranges_device, smf_uncompress_streams_device): behind its plan each of them has m
// slots, a chunk to decode or to copy each, in groups (the one stream, the ranges, the streams).
// The stage (slot_stage in smf_api.hip) runs the raw decoder over the slots, copies the 0x01
// payloads, takes the CRC-32C of every slot's output and gives each slot its verdict; a group's
// result is its plan's status, else its first failing slot's.  Here: the layout, its carve and the
// two verdict rules -- plain functions, compiled for the host and the device alike, so the host
// checker tests the code the kernels run.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common/smc_slots.h"
#include "smf_format.h"

namespace smf {

using smc::kNoSlot;  // a slot of no group; a group without a failing slot
using GroupHeader = smc::PlanHeader;

// A slot's status: why it was not decoded, else the raw decoder's status (a 0x00 chunk), else the
// CRC's verdict.
SMC_HD inline int32_t slot_verdict(int32_t pre, uint32_t type, int32_t dec_status, uint32_t crc_out, uint32_t crc_want) {
  if (pre != SM_OK) return pre;
  if (type == SMF_CHUNK_COMPRESSED && dec_status != SM_OK) return dec_status;
  return crc_out != crc_want ? (int32_t)SMF_ERR_CRC : (int32_t)SM_OK;
}

// A group's status: the shared rule, under the name the slot stage and its checker know it by.
SMC_HD inline int32_t group_verdict(bool over, int32_t pre, uint32_t fail, int32_t fail_status) {
  return smc::plan_verdict(over, pre, fail, fail_status);
}

struct Slots {
  // per slot, what the stage reads.  A slot that is not decoded has cap == 0 and dec_len == 0: the
  // raw decoder returns at once on an empty stream, and the copy and the CRC pass move nothing.
  uint8_t* type;       // 0x00: decoded, 0x01: copied
  uint64_t* in_off;    // the payload, relative to the stage's input
  uint32_t* crc_want;
  uint64_t* out_off;   // relative to the stage's output base
  uint32_t *dec_len, *cap;  // the raw decoder's input length (0 for a 0x01 chunk) and capacity = the declared length
  int32_t* pre;        // optional (null: SM_OK): why the slot is not decoded
  uint32_t* group;     // optional (null: all in group 0); kNoSlot: an unused slot, its verdict SM_OK
  // per slot, what it writes
  uint32_t *dec_out_len, *crc_out;
  int32_t *dec_status, *slot_status;
  // per group: its first failing slot (the plan sets kNoSlot)
  uint32_t* fail;
};

// The arrays a call owns, from its scratch.  index: type, in_off and crc_want (else the caller's
// index serves); pre; grouped: group and slot_status (else one group, the verdicts go to the caller).
inline Slots carve_slots(smc::Carve& c, size_t m, size_t ngroups, bool index, bool pre, bool grouped) {
  Slots s{};
  if (index) s.in_off = c.take<uint64_t>(m);
  s.out_off = c.take<uint64_t>(m);
  if (index) s.crc_want = c.take<uint32_t>(m);
  s.dec_len = c.take<uint32_t>(m);
  s.cap = c.take<uint32_t>(m);
  s.dec_out_len = c.take<uint32_t>(m);
  s.crc_out = c.take<uint32_t>(m);
  s.dec_status = c.take<int32_t>(m);
  if (pre) s.pre = c.take<int32_t>(m);
  if (grouped) s.group = c.take<uint32_t>(m);
  if (grouped) s.slot_status = c.take<int32_t>(m);
  if (index) s.type = c.take<uint8_t>(m);
  s.fail = c.take<uint32_t>(ngroups);
  return s;
}

// The groups' results, behind the slots' verdicts.
struct Groups {
  uint32_t n;
  const GroupHeader* hdr;  // optional (null: not over)
  const int32_t* pre;      // optional (null: SM_OK): the plan's status per group
  const uint64_t* len;     // the length a group reports
  bool len_on_error;       // also with a status (the batched decode: the walked length), else 0 then
  uint64_t* out_len;       // optional
  int32_t* status;
};

}  // namespace smf
