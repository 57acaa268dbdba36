// Plumbing shared by the C-ABI files (capi.hip, flock_comm.hip, cov_capi.hip,
// cov_maps_capi.hip, cov_step_capi.hip, shepherd.hip, graph_utils.hip): the error report,
// the HIP status checks, typed device allocation, the owner of a handle's device buffers
// and the opening of every *_create. The helpers are static or hidden: none becomes a
// symbol of the library.
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

// The same for a kernel launch, named `what` ("<what>: <hipGetErrorString>").
#define GF_LAUNCH(what, expr)                                    \
  do {                                                           \
    hipError_t e_ = (expr);                                      \
    if (e_ != hipSuccess) return gf::fail_hip(what, e_);         \
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

// The owner of a handle's device memory: what it hands out stays on its list until
// free_one or free_all, so a handle's release names no buffer. Hidden, like the static
// helpers above: no member becomes a symbol of the library.
#pragma GCC visibility push(hidden)
struct DeviceBuffers {
  static constexpr int kMax = 128;  // a handle's pointer fields, each on the list at most once
  void* ptrs[kMax];
  int n = 0;

  // dalloc_zero, remembered (also when the fill failed: free_all returns the memory).
  template <class T>
  int zeroed(T** p, size_t count) {
    if (n == kMax) return fail(GF_ENOMEM, "device buffer list full");
    const int rc = dalloc_zero(p, count);
    if (*p) ptrs[n++] = *p;
    return rc;
  }
  // `bytes` of hipMalloc, not filled, remembered.
  template <class T>
  hipError_t plain(T** p, size_t bytes) {
    *p = nullptr;
    if (n == kMax) return hipErrorOutOfMemory;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
    if (e == hipSuccess) ptrs[n++] = *p;
    return e;
  }
  // Frees *p and forgets it.
  template <class T>
  hipError_t free_one(T** p) {
    if (!*p) return hipSuccess;
    for (int k = 0; k < n; ++k)
      if (ptrs[k] == *p) {
        ptrs[k] = ptrs[--n];
        break;
      }
    const hipError_t e = hipFree(*p);
    *p = nullptr;
    return e;
  }
  // The buffers that are reallocated when they must grow: *p holds at least `need`
  // zero-filled elements, *have of them before the call.
  template <class T>
  int grow_zeroed(T** p, size_t* have, size_t need) {
    if (need <= *have) return GF_OK;
    GF_HIP(free_one(p));
    *have = 0;
    if (int rc = zeroed(p, need)) return rc;
    *have = need;
    return GF_OK;
  }
  void free_all() {
    while (n > 0) hipFree(ptrs[--n]);
  }
};
#pragma GCC visibility pop

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
