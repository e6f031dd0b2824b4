// smc_staging.h -- the host side of the container libraries' host-buffer calls: the groups' bytes
// packed behind one another in one staging block (one upload), room for every group's output at a
// 16-byte boundary of the device buffer (one download; each group's own bytes then go to the
// caller's place), and the per-group arrays the device call takes.  The layout part is plain C++
// (a host checker runs it under sanitizers), the rest needs HIP; all of it follows smc_hip_host.h:
// an unnamed namespace, so internal linkage throughout and no library exports any of it.  Not part
// of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "smc_layout.h"
#include "smc_slots.h"

namespace {

struct StreamCallArrays {  // per group, what a host-buffer call hands the device call (the ctx's sarg)
  uint64_t *in_off, *in_len, *out_off, *out_cap, *out_len;
  int32_t* status;
  uintptr_t end;
};
constexpr StreamCallArrays carve_stream_call(uintptr_t base, size_t n) {
  smc::Carve c{base};
  StreamCallArrays m{};
  m.in_off = c.take<uint64_t>(n);
  m.in_len = c.take<uint64_t>(n);
  m.out_off = c.take<uint64_t>(n);
  m.out_cap = c.take<uint64_t>(n);
  m.out_len = c.take<uint64_t>(n);
  m.status = c.take<int32_t>(n);
  m.end = c.p;
  return m;
}
constexpr size_t stream_call_bytes(size_t n) { return carve_stream_call(0, n).end; }

// The inputs in[off[r], off[r] + len[r]) behind one another, and room[r] bytes of output each from a
// 16-byte boundary.
struct StreamStaging {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> in_off, out_off;
  uint64_t out_total = 0;
  StreamStaging(const uint8_t* in, const uint64_t* off, const uint64_t* len, uint32_t n, const uint64_t* room)
      : in_off(n), out_off(n) {
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; ++r) {
      in_off[r] = total;
      total += len[r];
      out_off[r] = out_total;
      out_total += smc::round16(room[r]);
    }
    bytes.resize((size_t)total);
    for (uint32_t r = 0; r < n; ++r)
      if (len[r]) memcpy(bytes.data() + in_off[r], in + off[r], (size_t)len[r]);
  }
};

}  // namespace

#if defined(__HIPCC__)
#include "smc_hip_host.h"

namespace {

struct StagingBufs {  // a ctx's staging buffers, its argument scratch and the stream its host-buffer calls run on
  DevBuf &io_in, &io_out, &sarg;
  hipStream_t stream;
};

// room for the staged input, the output and the call's arrays (a byte of each staging buffer at the
// least: the device calls want both pointers)
inline sm_status ensure_staging(const StagingBufs& b, size_t in_bytes, size_t out_bytes, size_t arg_bytes) {
  SM_CHECK(b.io_in.ensure(in_bytes ? in_bytes : 1));
  SM_CHECK(b.io_out.ensure(out_bytes ? out_bytes : 1));
  SM_CHECK(b.sarg.ensure(arg_bytes));
  return SM_OK;
}

// uploads the staging and the arrays; out_cap may be null (compress)
inline sm_status upload_stream_call(const StagingBufs& b, const StreamStaging& h, const uint64_t* in_len,
                                    const uint64_t* out_cap, uint32_t n, StreamCallArrays& d) {
  hipStream_t s = b.stream;
  SM_PASS(ensure_staging(b, h.bytes.size(), (size_t)h.out_total, stream_call_bytes(n)));
  d = carve_stream_call((uintptr_t)b.sarg.p, n);
  if (!h.bytes.empty()) SM_CHECK(hipMemcpyAsync(b.io_in.p, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(d.in_off, h.in_off.data(), 8 * (size_t)n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(d.in_len, in_len, 8 * (size_t)n, hipMemcpyHostToDevice, s));
  SM_CHECK(hipMemcpyAsync(d.out_off, h.out_off.data(), 8 * (size_t)n, hipMemcpyHostToDevice, s));
  if (out_cap) SM_CHECK(hipMemcpyAsync(d.out_cap, out_cap, 8 * (size_t)n, hipMemcpyHostToDevice, s));
  return SM_OK;
}

// the lengths and the statuses, on their way back to the host
inline sm_status download_results(const StagingBufs& b, const uint64_t* d_out_len, const int32_t* d_status, size_t n,
                                  uint64_t* out_len, int32_t* status) {
  SM_CHECK(hipMemcpyAsync(out_len, d_out_len, 8 * n, hipMemcpyDeviceToHost, b.stream));
  SM_CHECK(hipMemcpyAsync(status, d_status, 4 * n, hipMemcpyDeviceToHost, b.stream));
  return SM_OK;
}

// out_total bytes of the device output buffer, back on the host (synchronises)
inline sm_status download_output(const StagingBufs& b, uint64_t out_total, std::vector<uint8_t>& out) {
  out.resize((size_t)out_total);
  if (!out.empty()) SM_CHECK(hipMemcpyAsync(out.data(), b.io_out.p, out.size(), hipMemcpyDeviceToHost, b.stream));
  SM_CHECK(hipStreamSynchronize(b.stream));
  return SM_OK;
}

// both, for a call with nothing else to fetch
inline sm_status download_stream_call(const StagingBufs& b, const StreamStaging& h, const StreamCallArrays& d,
                                      uint32_t n, uint64_t* out_len, int32_t* status, std::vector<uint8_t>& out) {
  SM_PASS(download_results(b, d.out_len, d.status, n, out_len, status));
  return download_output(b, h.out_total, out);
}

// uploads n elements of a host array behind one another in the ctx's argument scratch (a null host
// array: room for the device call's results)
struct ArgUpload {
  smc::Carve c;
  hipStream_t s;
  template <typename T>
  T* put(const T* host, size_t n, hipError_t& e) {
    T* const d = c.take<T>(n);
    if (e == hipSuccess && host && n) e = hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s);
    return d;
  }
};

}  // namespace
#endif  // __HIPCC__
