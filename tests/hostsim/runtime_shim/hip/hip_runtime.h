// TEST INFRASTRUCTURE ONLY - a heap-backed <hip/hip_runtime.h> for the host staging of the C-ABI
// (fbstab_amd/csrc/fb_host_stage.h), beside shim/ (the device twin of the kernels' arithmetic).
//
// tests/test_host_stage.py compiles fb_host_stage.h and a driver with g++ against THIS directory: the runtime
// surface that header uses, and nothing else.  Device memory is the heap - hipMalloc returns exactly the bytes asked
// for, so the address sanitizer sees a copy that overruns a staging buffer by one double - copies are memcpy (row by
// row for the 2-D form), and everything is synchronous.  The shim counts live allocations and runtime calls
// (fb_shim::state()), so that a test can ask whether a handle leaks and whether a refusal made any device call, and
// it can make the n-th hipMalloc fail.
//
// What it CANNOT show: a missing synchronisation (nothing here is asynchronous) and a wrong copy direction (host and
// device are one address space; the hipMemcpyKind is not looked at).  Those stay with the GPU tests
// (tests/test_gpu_placement.py).
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2,
                     hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
constexpr unsigned hipStreamDefault = 0;

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct hipDeviceProp_t {
  int multiProcessorCount;
};
// streams and events are heap objects of their own, so that one that is never destroyed is a leak the sanitizer reports
struct fb_shim_stream { int unused; };
struct fb_shim_event { int unused; };
typedef fb_shim_stream* hipStream_t;
typedef fb_shim_event* hipEvent_t;

namespace fb_shim {
struct State {
  long live = 0;           // allocations of hipMalloc not yet freed
  long mallocs = 0;        // hipMalloc calls so far
  long calls = 0;          // runtime calls so far, of any kind
  long fail_malloc_at = 0; // > 0: the hipMalloc call of this number (counted from `mallocs`) fails, once
  size_t last_bytes = 0;   // size of the last allocation
};
inline State& state() {
  static State s;
  return s;
}
inline hipError_t called() {
  state().calls++;
  return hipSuccess;
}
}  // namespace fb_shim

inline const char* hipGetErrorString(hipError_t e) {
  return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value";
}
inline hipError_t hipGetLastError() { return fb_shim::called(); }

template <class T>
inline hipError_t hipMalloc(T** p, size_t bytes) {
  fb_shim::State& st = fb_shim::state();
  st.calls++;
  st.mallocs++;
  *p = nullptr;
  if (st.fail_malloc_at > 0 && st.mallocs == st.fail_malloc_at) {
    st.fail_malloc_at = 0;
    return hipErrorOutOfMemory;
  }
  if (bytes == 0) return hipSuccess;  // (as the runtime: a null pointer, and nothing to free)
  *p = static_cast<T*>(malloc(bytes));
  if (!*p) return hipErrorOutOfMemory;
  st.live++;
  st.last_bytes = bytes;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  fb_shim::called();
  if (p) {
    fb_shim::state().live--;
    free(p);
  }
  return hipSuccess;
}

inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  memcpy(dst, src, bytes);
  return fb_shim::called();
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  return hipMemcpy(dst, src, bytes, kind);
}
inline hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                                   size_t height, hipMemcpyKind, hipStream_t) {
  if (width > dpitch || width > spitch) return hipErrorInvalidValue;  // (as the runtime)
  for (size_t r = 0; r < height; r++)
    memcpy(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
  return fb_shim::called();
}
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  memset(dst, value, bytes);
  return fb_shim::called();
}

inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = new fb_shim_stream{0};
  return fb_shim::called();
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  delete s;
  return fb_shim::called();
}
inline hipError_t hipStreamSynchronize(hipStream_t) { return fb_shim::called(); }
inline hipError_t hipEventCreate(hipEvent_t* e) {
  *e = new fb_shim_event{0};
  return fb_shim::called();
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  return fb_shim::called();
}
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return fb_shim::called(); }
inline hipError_t hipEventSynchronize(hipEvent_t) { return fb_shim::called(); }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.f;
  return fb_shim::called();
}

inline hipError_t hipSetDevice(int) { return fb_shim::called(); }
inline hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return fb_shim::called();
}
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
  prop->multiProcessorCount = 1;
  return fb_shim::called();
}
inline hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return fb_shim::called(); }
inline hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* blocks, const void*, int, size_t) {
  *blocks = 1;
  return fb_shim::called();
}
// (no kernel exists on the host: the driver passes host lambdas where fbstab_hip.hip passes launches, and an entry
// launched through launch_entry only counts)
inline hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return fb_shim::called(); }
