// JNI_OnLoad device probe shared by the JNI drop-in libraries.
//
// The reference has no JNI_OnLoad: System.load succeeding is all that IntelPairHmm.load() checks
// (NativeLibraryLoader.java:99-140), and a machine without the required ISA is filtered earlier by the
// libgkl_utils.so AVX gate.  A GPU library needs the equivalent for "no usable gfx950 device": returning JNI_ERR
// makes System.load throw UnsatisfiedLinkError, NativeLibraryLoader.load() returns false, and GATK falls back to its
// Java implementation instead of failing later in initNative.  GKL_HIP_LOAD_WITHOUT_DEVICE=1 keeps the load
// succeeding (initNative then raises RuntimeException).  Include once per shared library.
// GKL_JNI_SERVER_PROBE (libgkl_pairhmm.so): with GKL_HIP_SERVER=PATH set the library is a client of the PairHMM server
// on PATH, and the probe asks that server instead of the device -- no HIP call; a server that cannot be reached fails
// the load the same way (GATK falls back to its Java PairHMM).
// GKL_JNI_PDHMM_SERVER_PROBE (libgkl_pdhmm.so): the same for the PDHMM library, through gklhip_pdhmm_server_stats.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

#ifdef GKL_JNI_SERVER_PROBE
// (weak: the JNI layer's CPU test build links the shim against a stub of the C ABI that has no client mode)
extern "C" int gklhip_server_stats(const char* socket_path, gklhip_server_info* out) __attribute__((weak));
#endif
#ifdef GKL_JNI_PDHMM_SERVER_PROBE
// (weak for the same reason: a CPU test build of the shim against a stub of the C ABI has no client mode)
extern "C" int gklhip_pdhmm_server_stats(const char* socket_path, gklhip_pdhmm_server_info* out) __attribute__((weak));
#endif

extern "C" JNIEXPORT jint JNICALL JNI_OnLoad(JavaVM*, void*) {
  const char* force = getenv("GKL_HIP_LOAD_WITHOUT_DEVICE");
  if (force && *force == '1') return JNI_VERSION_1_8;
#ifdef GKL_JNI_SERVER_PROBE
  const char* server = getenv("GKL_HIP_SERVER");
  if (server && *server) {
    gklhip_server_info info;
    return gklhip_server_stats && gklhip_server_stats(server, &info) == GKLHIP_OK ? JNI_VERSION_1_8 : JNI_ERR;
  }
#endif
#ifdef GKL_JNI_PDHMM_SERVER_PROBE
  const char* pd_server = getenv("GKL_HIP_SERVER");
  if (pd_server && *pd_server) {
    gklhip_pdhmm_server_info info;
    return gklhip_pdhmm_server_stats && gklhip_pdhmm_server_stats(pd_server, &info) == GKLHIP_OK ? JNI_VERSION_1_8 : JNI_ERR;
  }
#endif
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return JNI_ERR; }
  for (int d = 0; d < n; d++) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) return JNI_VERSION_1_8;
  }
  return JNI_ERR;
}
