// What the host side of every HIP translation unit here shares (pairhmm_api.hip through pairhmm_ctx.h, pdhmm_api.hip
// ahead of pdhmm_ctx.h and the launch paths it includes, sw_api.hip): the error plumbing behind each library's *_last_error and the grow-and-trim device / pinned buffers of a
// context.  Everything sits in an anonymous namespace: each library keeps its own thread_local message.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <exception>
#include <new>
#include <string>

#include "../../include/gkl_hip_pairhmm.h"  // status codes

// ------------------------------------------------------------------ errors
namespace {
thread_local std::string g_err;

[[maybe_unused]] int fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return status;
}

// No C++ exception leaves the C ABI or a helper thread of these libraries (a std::bad_alloc from a plan vector inside a
// JVM would otherwise be std::terminate): entry points and thread bodies run their work through guarded().
[[maybe_unused]] int fail_noexcept(int status, const char* msg) noexcept {
  try { g_err = msg; } catch (...) {}
  return status;
}
template <typename F>
int guarded(F&& body) noexcept {
  try { return body(); }
  catch (const std::bad_alloc&) { return fail_noexcept(GKLHIP_ERR_OOM, "host memory allocation failed"); }
  catch (const std::exception& e) { return fail_noexcept(GKLHIP_ERR_HIP, e.what()); }
  catch (...) { return fail_noexcept(GKLHIP_ERR_HIP, "unexpected C++ exception"); }
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      (void)hipGetLastError();                                                               \
      return fail(e__ == hipErrorOutOfMemory ? GKLHIP_ERR_OOM : GKLHIP_ERR_HIP, "%s: %s",    \
                  #expr, hipGetErrorString(e__));                                            \
    }                                                                                        \
  } while (0)

// ------------------------------------------------------------------ buffers
// Device / pinned-host buffers of a context: they grow with the biggest call and shrink again when the calls stay small --
// a buffer above kTrimFloor that the last kTrimCalls calls each needed less than a quarter of is given back and re-made at
// the size in use (one 1.28 M-pair PairHMM call must not pin ~100 MB per slot for the life of the JVM; a 424k-pair PDHMM
// call holds ~3 GB of streams and tables).  hipFree / hipHostFree wait for the device to finish with the memory, exactly
// as on the grow path.
constexpr size_t kTrimFloor = (size_t)32 << 20;
constexpr int kTrimCalls = 16;
// Hysteresis (r05 advisor): hipFree / hipHostFree synchronise the whole device -- every other context's work in flight
// waits -- so a buffer that GREW less than kTrimQuiet calls ago is left alone: a workload that alternates one big call with
// sixteen small ones keeps its buffers instead of freeing and re-making 100 MB every round.  `small_uses` counts the small
// calls in a row, `since_grow` the calls since the buffer last grew.
constexpr int kTrimQuiet = 64;
inline bool trim_due(size_t n, size_t cap, int* small_uses, int* since_grow) {
  if (*since_grow < kTrimQuiet) ++*since_grow;
  if (cap <= kTrimFloor || n >= cap / 4) { *small_uses = 0; return false; }
  if (*small_uses < kTrimCalls) ++*small_uses;
  return *small_uses >= kTrimCalls && *since_grow >= kTrimQuiet;
}
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int small_uses = 0, since_grow = kTrimQuiet;
  int reserve(size_t n) {
    if (n <= cap && !trim_due(n, cap, &small_uses, &since_grow)) return GKLHIP_OK;
    if (n > cap) since_grow = 0;
    small_uses = 0;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const size_t want = n + n / 4 + 256;
    HIP_TRY(hipMalloc(&p, want));
    cap = want;
    return GKLHIP_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
struct PinBuf {  // page-locked host memory
  void* p = nullptr;
  size_t cap = 0;
  int small_uses = 0, since_grow = kTrimQuiet;
  int reserve(size_t n) {
    if (n <= cap && !trim_due(n, cap, &small_uses, &since_grow)) return GKLHIP_OK;
    if (n > cap) since_grow = 0;
    small_uses = 0;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const size_t want = n + n / 4 + 256;
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return GKLHIP_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
}  // namespace
