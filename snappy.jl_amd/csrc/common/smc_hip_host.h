// smc_hip_host.h -- the HIP host helpers of the three C ABIs (sm_api.hip, smf_api.hip,
// smm_api.hip): a growing device buffer, the device guard, the mode check and the two early-return
// macros.  Internal linkage throughout: no library exports any of it.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../../include/snappy_mi355x.h"

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {  // (growing frees the old buffer: hipFree waits for the device)
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = n < 4096 ? 4096 : n;
    const hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

inline bool valid_mode(int m) { return m == SM_MODE_REFERENCE || m == SM_MODE_FAST || m == SM_MODE_FAST_DENSE; }

}  // namespace

// in a function that returns sm_status: a failed HIP call is SM_ERR_DEVICE, a failed sm call itself
#define SM_CHECK(x)                               \
  do {                                            \
    if ((x) != hipSuccess) return SM_ERR_DEVICE;  \
  } while (0)
#define SM_PASS(x)                 \
  do {                             \
    const sm_status st_ = (x);     \
    if (st_ != SM_OK) return st_;  \
  } while (0)
