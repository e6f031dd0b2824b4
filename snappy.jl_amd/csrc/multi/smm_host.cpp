// smm_host.cpp -- the host-only part of the multi-stream library (include/snappy_mi355x_multi.h):
// the size helpers, the index rules and the plan of the ranged decode
// (include/snappy_mi355x_multi_range.h) over host arrays.  No HIP and no call into the raw codec,
// so this file also builds alone (the sanitizer driver, smm_host_check.cpp).
#include "smm_plan.h"
#include "smm_range.h"

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

// smm_index_device in stream order: k_index_count's counts and scan, then the walk of every stream
// that declares more than 64 KiB as the scalar loop (smm_plan.h index_walk)
sm_status smm_index_host(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                         uint32_t max_fragments, const uint32_t* out_cap, uint32_t* frag_first, uint32_t* frag_pos,
                         uint8_t* built, int32_t* status) {
  if (!frag_first) return SM_ERR_ARGUMENT;
  frag_first[0] = 0;
  if (nstreams == 0) return SM_OK;
  if (!in || !in_off || !in_len || !built || !status || (!frag_pos && max_fragments)) return SM_ERR_ARGUMENT;
  uint64_t total = 0;
  for (uint32_t s = 0; s < nstreams; ++s)
    total += smm::index_count(in + in_off[s], in_len[s], out_cap ? out_cap[s] : 0xffffffffu).count;
  const bool stop = total > max_fragments;
  uint32_t e = 0;
  for (uint32_t s = 0; s < nstreams; ++s) {
    status[s] = stop ? SM_ERR_ARGUMENT : SM_OK;
    built[s] = 0;
    frag_first[s] = e;
    if (stop) continue;
    const uint8_t* p = in + in_off[s];
    const smm::IndexCount c = smm::index_count(p, in_len[s], out_cap ? out_cap[s] : 0xffffffffu);
    if (c.D > smm::kBlock)
      built[s] = smm::index_walk(p, in_len[s], c.hv, c.count, frag_pos + e);
    else if (c.count)
      frag_pos[e] = c.hv;
    e += c.count;
  }
  frag_first[nstreams] = e;
  return SM_OK;
}

uint32_t smm_range_fragment_count(uint32_t lo, uint32_t len) { return smm::range_fragment_count(lo, len); }

size_t smm_range_scratch_bytes(uint32_t nranges, uint32_t max_range_fragments) {
  return smm::range_scratch_bytes(nranges, max_range_fragments);
}

// the device plan in range order: k_mrange_find's rule, the total k_mrange_scan compares, then
// k_mrange_slots' entry check of every touched fragment
sm_status smm_range_plan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                         const uint32_t* frag_first, const uint32_t* frag_pos, uint32_t nentries,
                         const uint32_t* range_stream, const uint32_t* lo, const uint32_t* len, uint32_t nranges,
                         uint32_t max_range_fragments, uint32_t* first, uint32_t* count, int32_t* status,
                         uint64_t* total) {
  if (total) *total = 0;
  if (nranges == 0) return SM_OK;
  if (!in || !in_off || !in_len || !frag_first || !frag_pos || !range_stream || !lo || !len) return SM_ERR_ARGUMENT;
  uint64_t sum = 0;
  for (uint32_t r = 0; r < nranges; ++r) {
    smm::Candidate c;
    sum += smm::range_span(in, in_off, in_len, nstreams, frag_first, nentries, range_stream[r], lo[r], len[r], c).count;
  }
  if (total) *total = sum;
  const bool stop = sum > max_range_fragments;
  for (uint32_t r = 0; r < nranges; ++r) {
    smm::Candidate c;
    const smm::RangeSpan sp =
        smm::range_span(in, in_off, in_len, nstreams, frag_first, nentries, range_stream[r], lo[r], len[r], c);
    int32_t failed = SM_OK;
    for (uint32_t k = 0; k < sp.count && failed == SM_OK && !stop; ++k)
      failed = smm::slot_verdict(
          smm::slot_args(frag_pos + c.e0, c, in_len[range_stream[r]], sp.first + k, lo[r], len[r]).status, SM_OK);
    if (first) first[r] = sp.first;
    if (count) count[r] = sp.count;
    if (status) status[r] = smm::range_verdict(stop, sp.status, failed);
  }
  return stop ? SM_BUFFER_TOO_SMALL : SM_OK;
}

}  // extern "C"
