// smm_host.cpp -- the host-only part of the multi-stream library (include/snappy_mi355x_multi.h):
// the size helpers and the index rules over host arrays.  No HIP and no call into the raw codec,
// so this file also builds alone (the sanitizer driver, smm_host_check.cpp).
#include "smm_plan.h"

extern "C" {

uint32_t smm_fragment_count(uint64_t len) { return smm::fragment_count(len); }

size_t smm_scratch_bytes(uint32_t nstreams, uint32_t max_fragments) {
  return smm::scratch_bytes(nstreams, max_fragments);
}

// the device plan in stream order: k_dplan_scan's rules, then k_dplan_fill's for every fragment
sm_status smm_index_check(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                          uint32_t max_fragments, const uint32_t* out_cap, const uint32_t* frag_first,
                          const uint32_t* frag_pos, uint8_t* indexed) {
  if ((frag_first == nullptr) != (frag_pos == nullptr)) return SM_ERR_ARGUMENT;
  if (nstreams == 0) return SM_OK;
  if (!in || !in_off || !in_len || !out_cap || !indexed) return SM_ERR_ARGUMENT;
  for (uint32_t s = 0; s < nstreams; ++s) indexed[s] = 0;
  if (!frag_first) return SM_OK;
  for (uint32_t s = 0; s < nstreams; ++s)
    if (!smm::first_rule(frag_first, s, nstreams, max_fragments)) return SM_OK;
  for (uint32_t s = 0; s < nstreams; ++s) {
    smm::Candidate c;
    if (!smm::stream_candidate(in + in_off[s], in_len[s], out_cap[s], frag_first[s], frag_first[s + 1], max_fragments, c))
      continue;
    bool ok = true;
    for (uint32_t f = 0; f < c.count; ++f) {
      uint32_t lo, hi;
      ok = smm::fragment_range(frag_pos + c.e0, f, c.count, c.hv, in_len[s], lo, hi) && ok;  // (every fragment is looked at)
    }
    indexed[s] = ok;
  }
  return SM_OK;
}

}  // extern "C"
