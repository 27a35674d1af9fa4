// Test infrastructure (CPU): what gkl_amd/csrc/pairhmm_server.cpp needs of the C ABI beyond tests/native/stub_gklhip.cpp,
// so that the server can be linked against the stub (tests/test_server_cpu.py) -- no device, no PairHMM arithmetic.
//   STUB_REGISTER=0     gklhip_host_register fails: the server takes its copy path
//   STUB_DELAY_US=n     every gklhip_compute sleeps n microseconds first (calls that are "in flight" long enough to
//                       kill a client or the server in the middle of one)
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/gkl_hip_pairhmm.h"

extern "C" void stub_delay_us(long us);

namespace {
struct FromEnv {
  FromEnv() { if (const char* v = getenv("STUB_DELAY_US")) stub_delay_us(atol(v)); }
} from_env;
}  // namespace

extern "C" {

int gklhip_host_register(void* p, size_t bytes) {
  const char* v = getenv("STUB_REGISTER");
  return p && bytes && !(v && v[0] == '0') ? GKLHIP_OK : GKLHIP_ERR_HIP;
}
int gklhip_host_unregister(void*) { return GKLHIP_OK; }
int gklhip_small_call_counts(int device, int64_t out[3], int reset) {
  if (!out || device < 0) return GKLHIP_ERR_INVALID_ARG;
  out[0] = out[1] = out[2] = 0;
  return GKLHIP_OK;
}
int gklhip_get_stats(gklhip_ctx* c, gklhip_stats* out) {
  if (!c || !out) return GKLHIP_ERR_INVALID_ARG;
  memset(out, 0, sizeof *out);
  return GKLHIP_OK;
}
int gklhip_num_devices(gklhip_ctx* c) { return c ? 1 : 0; }

}  // extern "C"
