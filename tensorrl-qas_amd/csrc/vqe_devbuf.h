// vqe_devbuf.h - the host layer's one owning device buffer and its one HIP error macro.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include "../../include/vqe_hip.h"

namespace vqe {

// Grows by re-allocation (the content is not kept), never shrinks.  SLACK: a quarter more than asked for, so that a
// batch that grows call by call re-allocates rarely (the buffers of vqe_handle); without it exactly what was asked for
// (StreamWork: the states alone are gigabytes at n = 20 and batch 256).
template <class T, bool SLACK = true>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const size_t want = SLACK ? n + n / 4 + 16 : n;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
};
template <class T>
using DevBufExact = DevBuf<T, false>;

// where a failed call leaves its message: the caller's error string here, the handle in vqe_api.hip's overload
inline int fail(std::string& err, int code, const std::string& msg) {
  err = msg;
  return code;
}

}  // namespace vqe

// ctx: what fail() takes first (a handle, or the string that receives the message)
#define HIP_TRY(ctx, expr)                                                             \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(ctx, _e == hipErrorOutOfMemory ? VQE_ENOMEM : VQE_EHIP,              \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                  \
  } while (0)
// the same for a call that returns one of the VQE_* codes itself
#define VQE_TRY(expr)                                                                  \
  do {                                                                                 \
    if (const int _rc = (expr)) return _rc;                                            \
  } while (0)
