// Plumbing shared by the C-ABI files (capi.hip, flock_comm.hip, cov_capi.hip, shepherd.hip,
// graph_utils.hip): the error report, the HIP status check, typed device allocation and
// the opening of every *_create. The helpers are static: none becomes a symbol of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "device_alloc.h"
#include "gymflock.h"

namespace gf {

// Sets the calling thread's error message (fe_last_error) and returns `code`. One
// thread-local string for the whole library, defined in capi.hip.
int set_error(int code, const std::string& msg);

static inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

static inline int fail_hip(const char* what, hipError_t e) {
  return set_error(GF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Returns GF_EHIP ("<expression>: <hipGetErrorString>") from the enclosing function
// unless the HIP call succeeds.
#define GF_HIP(expr)                                        \
  do {                                                      \
    hipError_t e_ = (expr);                                 \
    if (e_ != hipSuccess) return gf::fail_hip(#expr, e_);   \
  } while (0)

// `count` elements of device memory (device_alloc.h; count 0: nullptr).
template <class T>
static int dalloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) return GF_OK;
  hipError_t e = device_alloc(reinterpret_cast<void**>(p), count * sizeof(T));
  if (e != hipSuccess) return fail(GF_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return GF_OK;
}

// The same, zero-filled.
template <class T>
static int dalloc_zero(T** p, size_t count) {
  if (int rc = dalloc(p, count)) return rc;
  if (!*p) return GF_OK;
  GF_HIP(hipMemset(*p, 0, count * sizeof(T)));
  // hipMemset may still be running on the null stream, which the handle's non-blocking
  // stream does not order against: finish it before any kernel writes the buffer
  GF_HIP(hipDeviceSynchronize());
  return GF_OK;
}

// The opening of every *_create: a device exists, `device` names one, and it becomes the
// calling thread's current device.
static inline int select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(GF_EHIP, "no HIP device available (libgymflock needs an MI355X)");
  if (device < 0 || device >= ndev) return fail(GF_EINVAL, "device ordinal out of range");
  GF_HIP(hipSetDevice(device));
  return GF_OK;
}

}  // namespace gf
