// dtk_own.h -- the owners of the host units' HIP resources: device arrays, page-locked buffers, streams and events.
// What they hold is released by their destructors and nowhere else (dtk_pinned_free aside: the caller's memory).  None
// can be copied or moved: the objects they are members of live on the heap and stay where they are.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/datok_gpu.h"

#pragma GCC visibility push(hidden)

int hip_fail(hipError_t e, const char *what);
#define HIP_TRY(call)                                   \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return hip_fail(e_, #call);   \
  } while (0)

struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy &) = delete;
  NoCopy &operator=(const NoCopy &) = delete;
};

// Device array of T with its capacity in elements.
template <class T>
struct DevArray : NoCopy {
  T *p = nullptr;
  uint64_t cap = 0;
  ~DevArray() { if (p) (void)hipFree(p); }
  operator T *() const { return p; }
  // Room for n elements: no HIP call if they fit, else the array is freed and made anew with cap_if_grown elements
  // (its contents are lost; the caller chooses the slack).  A failure leaves {nullptr, 0}.
  int fit(uint64_t n, uint64_t cap_if_grown) {
    if (n <= cap) return DTK_OK;
    T *old = p;
    p = nullptr; cap = 0;
    if (old) HIP_TRY(hipFree(old));
    const hipError_t e = hipMalloc((void **)&p, cap_if_grown * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc"); }
    cap = cap_if_grown;
    return DTK_OK;
  }
};

// Page-locked host memory with its capacity in bytes.
struct PinBuf : NoCopy {
  void *p = nullptr;
  size_t cap = 0;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  template <class T> T *as() const { return static_cast<T *>(p); }
  int fit(size_t n, size_t cap_if_grown) {
    if (n <= cap && p) return DTK_OK;
    void *old = p;
    p = nullptr; cap = 0;
    if (old) HIP_TRY(hipHostFree(old));
    const hipError_t e = hipHostMalloc(&p, cap_if_grown, hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipHostMalloc"); }
    cap = cap_if_grown;
    return DTK_OK;
  }
  // (grown with a quarter of slack: allocation costs milliseconds)
  int fit(size_t n) { return fit(n, std::max<size_t>(n + n / 4, 256)); }
};

// A stream of the object's own (non-blocking), or one lent by the caller, which is left alone.
struct Stream : NoCopy {
  hipStream_t s = nullptr;
  bool mine = false;
  ~Stream() { if (s && mine) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
  int create() {
    const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { s = nullptr; return hip_fail(e, "hipStreamCreateWithFlags"); }
    mine = true;
    return DTK_OK;
  }
  int lend(hipStream_t h) {
    if (s && mine) HIP_TRY(hipStreamDestroy(s));
    s = h; mine = false;
    return DTK_OK;
  }
};

// An event created with its first use.
struct Event : NoCopy {
  hipEvent_t e = nullptr;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
  int ensure(unsigned flags) {
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, flags));
    return DTK_OK;
  }
};

#pragma GCC visibility pop
