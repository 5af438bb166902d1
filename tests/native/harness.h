// tests/native/harness.h -- what every *_harness.cpp of this directory shares: the device buffer, the error and export macros, the
// argument checks and the device queries.  Test infrastructure only: each harness is one translation unit built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_<stem>_harness.so with hidden visibility, so nothing here is exported but what
// H_EXPORT marks.  It includes nothing of the product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define H_EXPORT extern "C" __attribute__((visibility("default")))
#define H_BAD_ARGS (-1)
// return off + the first hipError_t (k1 / k1p: off = 1000, their entry points also return lcpc status codes)
#define H_TRY_OFF(expr, off) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (off) + (int)e_; } while (0)
#define H_TRY(expr) H_TRY_OFF(expr, 0)
// <prefix>device_count / <prefix>cu_count of a harness
#define H_DEVICE_COUNT(prefix) \
  H_EXPORT int prefix##device_count() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
#define H_CU_COUNT(prefix) \
  H_EXPORT int prefix##cu_count() { hipDeviceProp_t prop; return hipGetDeviceProperties(&prop, 0) == hipSuccess ? prop.multiProcessorCount : 0; }

namespace {

struct DevBuf {
  uint32_t* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc((void**)&p, bytes ? bytes : 16); }
  hipError_t put(const void* src, size_t bytes) {
    hipError_t e = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t get(void* dst, size_t bytes) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};

constexpr uint64_t MAX_WORDS = (uint64_t)1 << 28;   // what a test may ask for of one buffer (the launchers take more)
bool nl_ok(int nl) { return nl == 2 || nl == 4 || nl == 6 || nl == 8; }
// an element array's alignment
bool off_ok(uint64_t off_words, int nl) { return (off_words * 4) % (nl % 4 == 0 ? 16 : 8) == 0; }
// `words` words from off on lie inside a buffer of buf_words
bool span_ok(uint64_t words, uint64_t buf_words, uint64_t off, int nl) {
  return words <= MAX_WORDS && buf_words <= MAX_WORDS && off <= buf_words && words <= buf_words - off && off_ok(off, nl);
}

}  // namespace
