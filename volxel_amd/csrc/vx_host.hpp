// vx_host.hpp -- host-only helpers of vx_api.hip: the error macros and the three owners of device resources (a device
// buffer, the carve of one allocation into typed arrays, a stage timer).  No device code.
//
// The owners release with hipFree / hipEventDestroy, which act on the calling thread's current device.  They are only ever
// released from inside an entry point that made the context's device current first: VxContext::Volume is reset by free_volume
// (vx_upload_volume behind its VX_DEV, vx_destroy behind its hipSetDevice), everything else by the `delete` at the end of
// vx_destroy, which sets the device of each context -- each member of a device group included -- before anything is released.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/volxel_hip.h"

// what the owners need of a context (VxContext derives from it)
struct VxCore {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
};

#define VX_FAIL(ctx, code, ...)                       \
  do {                                                \
    char buf_[512];                                   \
    snprintf(buf_, sizeof buf_, __VA_ARGS__);         \
    (ctx)->err = buf_;                                \
    return (code);                                    \
  } while (0)

#define VX_HIP(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) VX_FAIL(ctx, VX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace vx {

// A device buffer that owns its memory; cap counts elements (bytes for DevBuf<void>).  Reads as its pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // exactly n elements, whatever was there: freed first, null / 0 when the allocation fails
  int alloc(VxCore* c, size_t n) {
    reset();
    VX_HIP(c, hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(std::conditional_t<std::is_void_v<T>, char, T>)));
    cap = n;
    return VX_OK;
  }
  // at least n elements: grows, never shrinks
  int ensure(VxCore* c, size_t n) { return n > cap ? alloc(c, n) : VX_OK; }
};

// One allocation carved into typed arrays.  `layout` is called twice with a Carve and takes its arrays in order, take<T>(n):
// the first pass (no base) only adds up the bytes, the second hands out the pointers, so the size and the carve cannot disagree.
struct Carve {
  uintptr_t base = 0;
  size_t off = 0;
  template <class T>
  T* take(size_t n = 1) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;   // (null while measuring: what a failed allocation leaves)
    off += n * sizeof(T);
    return r;
  }
};
template <class F>
int carve(VxCore* c, DevBuf<void>& buf, F&& layout) {
  Carve measure;
  layout(measure);
  if (int rc = buf.alloc(c, measure.off)) return rc;
  Carve k{reinterpret_cast<uintptr_t>(buf.p)};
  layout(k);
  return VX_OK;
}

// The timer of N stages of a call: N + 1 events, created by the first mark.  mark(c, i) records event i on the context's
// stream; read(c) fills ms[k] with the time from event k to event k + 1 (every event recorded and complete).
template <int N>
struct StageTimer {
  hipEvent_t ev[N + 1] = {};
  double ms[N] = {};   // what the last read found
  StageTimer() = default;
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int mark(VxCore* c, int i) {
    for (hipEvent_t& e : ev)
      if (!e) VX_HIP(c, hipEventCreate(&e));
    VX_HIP(c, hipEventRecord(ev[i], c->stream));
    return VX_OK;
  }
  int read(VxCore* c) {
    for (int k = 0; k < N; ++k) {
      float f = 0.0f;
      VX_HIP(c, hipEventElapsedTime(&f, ev[k], ev[k + 1]));
      ms[k] = f;
    }
    return VX_OK;
  }
};

}  // namespace vx
