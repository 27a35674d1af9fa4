// C-ABI implementation (include/gkl_hip_pdhmm.h) of the MI355X PDHMM path.  Compiled WITHOUT the
// fp64 flush-to-zero flag of the PairHMM translation unit: the reference's PDHMM never touches
// MXCSR (no _MM_SET_FLUSH_ZERO_MODE anywhere under src/main/native/pdhmm).
//
// This file: the argument checks and every extern "C" entry.  What a call decides is pdhmm_call_plan.h (no HIP in it);
// the context pdhmm_ctx.h; a single call pdhmm_single_call.h; several regions in one set of launches pdhmm_multi_call.h;
// concurrent callers sharing such a set pdhmm_combine.h.
#include <hip/hip_runtime.h>
#include <sys/sysinfo.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <vector>

#include "../../include/gkl_hip_pairhmm.h"  // status codes
#include "../../include/gkl_hip_pdhmm.h"
#include "pdhmm_kernel.h"
#include "pdhmm_remote.h"
#include "hip_host_common.h"      // g_err / fail / guarded / HIP_TRY, DevBuf, PinBuf
#include "pairhmm_host_finalize.h"   // gklhip::WorkerPool: persistent threads for the host log10

#include "pdhmm_ctx.h"
#include "pdhmm_single_call.h"
#include "pdhmm_multi_call.h"
#include "pdhmm_combine.h"

extern "C" {

const char* gklhip_pdhmm_last_error(void) { return g_err.c_str(); }

int64_t gklhip_pdhmm_get_table(int which, double* dst, int64_t cap) {
  const PdTables& t = pd_tables();
  const std::vector<double>* v = which == 0 ? &t.q2err : which == 1 ? &t.mm : nullptr;
  if (!v) return -1;
  if (dst) memcpy(dst, v->data(), sizeof(double) * (size_t)std::min<int64_t>(cap, (int64_t)v->size()));
  return (int64_t)v->size();
}

namespace {
// "reference" (default) | "vector": read by the process that makes the context, a client included
int pd_tail_mode_from_env() {
  const char* tm = getenv("GKL_HIP_PDHMM_TAIL");
  return (tm && (strcmp(tm, "vector") == 0 || strcmp(tm, "0") == 0)) ? 0 : 1;
}
}  // namespace

int gklhip_pdhmm_connect(const char* socket_path, int device, gklhip_pdhmm_ctx** out_ctx) {
  if (!out_ctx) return fail(GKLHIP_ERR_INVALID_ARG, "out_ctx is NULL");
  *out_ctx = nullptr;
  gklhip_pdhmm_ctx* c = new (std::nothrow) gklhip_pdhmm_ctx();
  if (!c) return fail(GKLHIP_ERR_OOM, "context allocation failed");
  std::string err;
  int rc;
  try { rc = gklhip_pd_remote::connect(socket_path, device, &c->remote, &err); }
  catch (...) { rc = GKLHIP_ERR_OOM; err = "host memory allocation failed"; }
  if (rc != GKLHIP_OK) { delete c; return fail(rc, "%s", err.c_str()); }
  c->device = device;
  c->tail_mode = pd_tail_mode_from_env();
  *out_ctx = c;
  return GKLHIP_OK;
}

int gklhip_pdhmm_is_remote(gklhip_pdhmm_ctx* c) { return c && c->remote ? 1 : 0; }

int gklhip_pdhmm_server_stats(const char* socket_path, gklhip_pdhmm_server_info* out) {
  if (!out) return fail(GKLHIP_ERR_INVALID_ARG, "NULL argument");
  std::string err;
  int rc;
  try { rc = gklhip_pd_remote::server_stats(socket_path, out, &err); }
  catch (...) { rc = GKLHIP_ERR_OOM; err = "host memory allocation failed"; }
  return rc == GKLHIP_OK ? rc : fail(rc, "%s", err.c_str());
}

int gklhip_pdhmm_init(int device, gklhip_pdhmm_ctx** out_ctx) {
  // GKL_HIP_SERVER=PATH: every context of the process is a client context of the server on PATH
  if (const char* path = getenv("GKL_HIP_SERVER"))
    if (*path) return gklhip_pdhmm_connect(path, device, out_ctx);
  if (!out_ctx) return fail(GKLHIP_ERR_INVALID_ARG, "out_ctx is NULL");
  *out_ctx = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(GKLHIP_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU compute path)");
  }
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= ndev) return fail(GKLHIP_ERR_INVALID_ARG, "device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GKLHIP_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  gklhip_pdhmm_ctx* c = new (std::nothrow) gklhip_pdhmm_ctx();
  if (!c) return fail(GKLHIP_ERR_OOM, "context allocation failed");
  c->device = device;
  auto bail = [&](int st) { gklhip_pdhmm_done(c); return st; };
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipStreamCreate failed"));
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&c->dev_ev, hipEventDisableTiming) != hipSuccess)
    return bail(fail(GKLHIP_ERR_HIP, "hipEventCreate failed"));
  if (hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipStreamCreate failed"));
  for (int k = 0; k < gklhip_pdhmm_ctx::kMaxSlices; k++)
    if (hipEventCreateWithFlags(&c->up_ev[k], hipEventDisableTiming) != hipSuccess || hipEventCreate(&c->sl_ev0[k]) != hipSuccess ||
        hipEventCreate(&c->sl_ev1[k]) != hipSuccess)
      return bail(fail(GKLHIP_ERR_HIP, "hipEventCreate failed"));
  const PdTables& t = pd_tables();
  int rc = c->tables.reserve((t.q2err.size() + t.mm.size()) * sizeof(double));
  if (rc) return bail(rc);
  if (hipMemcpy(c->tables.p, t.q2err.data(), t.q2err.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->tables.as<double>() + t.q2err.size(), t.mm.data(), t.mm.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(GKLHIP_ERR_HIP, "table upload failed"));
  {
    c->tail_mode = pd_tail_mode_from_env();
    const char* tb = getenv("GKL_HIP_PDHMM_TABLE");
    c->use_table = (tb && tb[0] == '0') ? 0 : 1;
    const char* pl = getenv("GKL_HIP_PDHMM_PIPELINE");
    c->pipeline = (pl && pl[0] == '0') ? 0 : 1;
  }
  if (c->use_table) {
    // once per process and device: does a DS read beyond the workgroup's LDS allocation return 0 here?  The table
    // kernel's idle entries depend on it (pdhmm_kernel.h: kPdTabIdle); if not, every haplotype takes the other kernels.
    static std::mutex mu;
    static std::vector<int> checked;   // 0 unknown, 1 good, -1 bad
    std::lock_guard<std::mutex> l(mu);
    if ((int)checked.size() <= device) checked.resize((size_t)device + 1, 0);
    if (checked[(size_t)device] == 0) {
      uint32_t* d_out = nullptr;
      uint32_t h_out = 1u;
      if (hipMalloc(reinterpret_cast<void**>(&d_out), 4) != hipSuccess) return bail(fail(GKLHIP_ERR_OOM, "hipMalloc failed"));
      bool ok = hipMemsetAsync(d_out, 0, 4, c->stream) == hipSuccess;
      hipLaunchKernelGGL(pdhmm_idle_class_selftest_kernel, dim3(64), dim3(64), 0, c->stream, d_out);
      ok = ok && hipMemcpyAsync(&h_out, d_out, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
      (void)hipFree(d_out);
      checked[(size_t)device] = ok && h_out == 0u ? 1 : -1;
      if (checked[(size_t)device] < 0)
        fprintf(stderr, "[gklhip] pdhmm: LDS reads beyond the allocation do not return 0 on device %d (%08x): the table kernel is off\n", device, h_out);
    }
    if (checked[(size_t)device] < 0) c->use_table = 0;
  }
  *out_ctx = c;
  return GKLHIP_OK;
}

int gklhip_pdhmm_set_tail_mode(gklhip_pdhmm_ctx* c, int mode) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
  if (mode != 0 && mode != 1) return fail(GKLHIP_ERR_INVALID_ARG, "tail mode %d (0 or 1)", mode);
  std::lock_guard<std::mutex> lock(c->mu);
  c->tail_mode = mode;
  return GKLHIP_OK;
}

int gklhip_pdhmm_done(gklhip_pdhmm_ctx* c) {
  if (!c) return GKLHIP_OK;
  if (c->remote) {
    gklhip_pd_remote::close(c->remote);
    delete c;
    return GKLHIP_OK;
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
  for (int k = 0; k < gklhip_pdhmm_ctx::kMaxSlices; k++)
    for (hipEvent_t e : {c->up_ev[k], c->sl_ev0[k], c->sl_ev1[k]})
      if (e) (void)hipEventDestroy(e);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  for (DevBuf* b : {&c->tables, &c->inputs, &c->entries, &c->entries_tab, &c->sums, &c->misc, &c->carry, &c->jobs, &c->tabx}) b->release();
  for (PinBuf* b : {&c->stage_in, &c->stage_jobs, &c->sums_pin}) b->release();
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->dev_ev) (void)hipEventDestroy(c->dev_ev);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return GKLHIP_OK;
}

int gklhip_pdhmm_set_fma_mode(gklhip_pdhmm_ctx* c, int fma_mode) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
  if (fma_mode != 0 && fma_mode != 1) return fail(GKLHIP_ERR_INVALID_ARG, "fma_mode %d (0 or 1)", fma_mode);
  std::lock_guard<std::mutex> lock(c->mu);
  c->fma_mode = fma_mode;
  return GKLHIP_OK;
}

float gklhip_pdhmm_last_kernel_ms(gklhip_pdhmm_ctx* c) { return c ? c->last_ms : 0.f; }
int64_t gklhip_pdhmm_buffer_bytes(gklhip_pdhmm_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lock(c->mu);
  if (c->remote) return (int64_t)gklhip_pd_remote::arena_bytes(c->remote);
  size_t total = 0;
  for (const DevBuf* b : {&c->tables, &c->inputs, &c->entries, &c->entries_tab, &c->sums, &c->misc, &c->carry, &c->jobs, &c->tabx}) total += b->cap;
  for (const PinBuf* b : {&c->stage_in, &c->stage_jobs, &c->sums_pin}) total += b->cap;
  return (int64_t)total;
}
int gklhip_pdhmm_last_routing(gklhip_pdhmm_ctx* c, int32_t out[3]) {
  if (!c || !out) return fail(GKLHIP_ERR_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(c->mu);
  for (int i = 0; i < 3; i++) out[i] = c->last_routing[i];
  return GKLHIP_OK;
}

namespace {
int pd_validate(const PdProblem& q, const double* out_host) {
  if (q.max_hap_len <= 0 || q.max_read_len <= 0)
    return fail(GKLHIP_ERR_INVALID_ARG, "maxHapLength / maxReadLength must be greater than 0");
  if (!q.hap_bases || !q.hap_pdbases || !q.read_bases || !q.read_qual || !q.read_ins_qual || !q.read_del_qual ||
      !q.gcp || !q.hap_lengths || !q.read_lengths || !out_host)
    return fail(GKLHIP_ERR_INVALID_ARG, "Input arrays aren't valid.");
  if (q.n_pairs > 0x7fffffffLL) return fail(GKLHIP_ERR_INVALID_ARG, "more than 2^31 pairs");
  for (int i = 0; i < q.n_hap_items; i++)
    if (q.hap_lengths[i] < 1 || q.hap_lengths[i] > q.max_hap_len)
      return fail(GKLHIP_ERR_INVALID_ARG, "hap_lengths[%d] = %lld outside 1..%d", i, (long long)q.hap_lengths[i], q.max_hap_len);
  for (int i = 0; i < q.n_read_items; i++)
    if (q.read_lengths[i] < 1 || q.read_lengths[i] > q.max_read_len)
      return fail(GKLHIP_ERR_INVALID_ARG, "read_lengths[%d] = %lld outside 1..%d", i, (long long)q.read_lengths[i], q.max_read_len);
  return GKLHIP_OK;
}

// One cross call's arguments (gklhip_pdhmm_compute_cross_batched; a region of _compute_cross_multi) as a checked problem.
int pd_cross_problem(const gklhip_pdhmm_cross* x, int64_t ref_batch_pairs, const double* out_host, PdProblem* q) {
  if (ref_batch_pairs < 0) return fail(GKLHIP_ERR_INVALID_ARG, "ref_batch_pairs must not be negative");
  if (!x) return fail(GKLHIP_ERR_INVALID_ARG, "batch is NULL");
  if (x->n_reads <= 0 || x->n_haps <= 0) return fail(GKLHIP_ERR_INVALID_ARG, "no pairs to process");
  *q = PdProblem{(int64_t)x->n_reads * x->n_haps, x->n_reads, x->n_haps, x->n_haps, x->max_hap_len, x->max_read_len,
                 x->hap_bases, x->hap_pdbases, x->read_bases, x->read_qual, x->read_ins_qual, x->read_del_qual, x->gcp,
                 x->hap_lengths, x->read_lengths, ref_batch_pairs};
  return pd_validate(*q, out_host);
}

// One paired call's arguments (gklhip_pdhmm_compute, _compute_device) as a checked problem.
int pd_paired_problem(const gklhip_pdhmm_batch* b, const double* out, PdProblem* q) {
  if (!b) return fail(GKLHIP_ERR_INVALID_ARG, "batch is NULL");
  // IntelPDHMM.java:163-173
  if (b->batch <= 0) return fail(GKLHIP_ERR_INVALID_ARG, "batchSize must be greater than 0");
  *q = PdProblem{b->batch, b->batch, b->batch, 0, b->max_hap_len, b->max_read_len, b->hap_bases, b->hap_pdbases,
                 b->read_bases, b->read_qual, b->read_ins_qual, b->read_del_qual, b->gcp, b->hap_lengths, b->read_lengths, 0};
  return pd_validate(*q, out);
}

// A client context: the checked call goes to the server, which answers with its context's kernel time and routing.
int pd_run_remote(gklhip_pdhmm_ctx* c, const PdProblem& q, double* out_host) {
  const gklhip_pd_remote::Call call{q.cross_haps ? 1 : 0, q.n_read_items, q.n_hap_items, q.max_hap_len, q.max_read_len,
                                    (c->fma_mode ? 1 : 0) | (c->tail_mode ? 2 : 0), q.ref_batch_pairs, q.n_pairs,
                                    q.hap_bases, q.hap_pdbases, q.read_bases, q.read_qual, q.read_ins_qual, q.read_del_qual,
                                    q.gcp, q.hap_lengths, q.read_lengths};
  gklhip_wire::PdComputeReply rep{};
  std::string err;
  int rc;
  try { rc = gklhip_pd_remote::compute(c->remote, call, out_host, &rep, &err); }
  catch (...) { rc = GKLHIP_ERR_OOM; err = "host memory allocation failed"; }
  if (rc != GKLHIP_OK) return fail(rc, "%s", err.c_str());
  c->last_ms = rep.kernel_ms;
  for (int i = 0; i < 3; i++) c->last_routing[i] = rep.routing[i];
  return GKLHIP_OK;
}

int pd_run(gklhip_pdhmm_ctx* c, const PdProblem& q, double* out_host) {
  std::lock_guard<std::mutex> lock(c->mu);
  if (c->remote) return pd_run_remote(c, q, out_host);
  return pd_fenced(c, [&] { return pd_run_locked(c, q, out_host); });
}

// Does the cross call fit a multi-region launch set on its own?
bool pd_fits_multi(const PdProblem& q) { return q.cross_haps && PdMultiFit().fits_with(q); }

// a cross call on a context of this process, counted (gklhip_pdhmm_combine_counts); with the combiner on, through it
int pd_run_cross(gklhip_pdhmm_ctx* c, const PdProblem& q, double* out_host) {
  if (!c->remote && pd_combine_config()->on && c->device >= 0 && c->device < kPdCountDevices && pd_fits_multi(q)) {
    std::lock_guard<std::mutex> lock(c->mu);
    return pd_run_combined(c, q, out_host);
  }
  if (!c->remote) pd_count(c->device, 1, 0, 1);
  return pd_run(c, q, out_host);
}
}  // namespace

int gklhip_pdhmm_compute(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_batch* b, double* out_host) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  PdProblem q;
  const int rc = pd_paired_problem(b, out_host, &q);
  return rc ? rc : pd_run(c, q, out_host);
}

int gklhip_pdhmm_compute_cross(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_cross* x, double* out_host) {
  return gklhip_pdhmm_compute_cross_batched(c, x, 0, out_host);
}

int32_t gklhip_pdhmm_available_memory_mb(int32_t max_memory_mb) {
  // pdhmm-implementation.h:204-235 (getMaxMemoryAvailable): min(maxMemoryInMB, free RAM of the host) -- taken ONCE, by
  // initNative, like the reference does; the batch cut of every later call then depends on its arguments only
  if (max_memory_mb <= 0) return 0;
  int64_t mb = max_memory_mb;
  struct sysinfo info;
  if (sysinfo(&info) == 0) mb = std::min<int64_t>(mb, (int64_t)info.freeram * (int64_t)info.mem_unit / (1024 * 1024));
  return (int32_t)std::max<int64_t>(mb, 0);
}

int64_t gklhip_pdhmm_reference_batch_pairs(int32_t max_memory_mb, int32_t max_read_len, int32_t max_hap_len, int64_t total_pairs) {
  // JavaData.h:86-101: min(totalPairs, maxMemory / memoryPerPair), maxMemory = what initNative kept (above)
  if (max_memory_mb <= 0 || max_read_len <= 0 || max_hap_len <= 0 || total_pairs <= 0) return 0;
  const int64_t per_pair = ((int64_t)max_read_len * 5 + (int64_t)max_hap_len * 2) + 8 + 16;
  return std::min(total_pairs, (int64_t)max_memory_mb * 1024 * 1024 / per_pair);
}

int gklhip_pdhmm_compute_cross_batched(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_cross* x, int64_t ref_batch_pairs, double* out_host) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  PdProblem q;
  const int rc = pd_cross_problem(x, ref_batch_pairs, out_host, &q);
  return rc ? rc : pd_run_cross(c, q, out_host);
}

// ---- device-resident calls: byte arrays and results in HBM, synchronous ----
namespace {
constexpr const char* kPdDeviceRemoteText = "device-resident batches cannot go to the PDHMM server (client context)";

// The checked problem on the context's own stream and buffers: never through the combiner, never counted
// (gklhip_pdhmm_combine_counts).
int pd_run_device(gklhip_pdhmm_ctx* c, PdProblem q, double* out_dev, double* sums_dev, void* hip_stream) {
  q.in_hbm = true;
  const PdDeviceOut dev{out_dev, sums_dev, static_cast<hipStream_t>(hip_stream)};
  std::lock_guard<std::mutex> lock(c->mu);
  return pd_fenced(c, [&] { return pd_run_locked(c, q, nullptr, &dev); });
}
}  // namespace

int gklhip_pdhmm_compute_device(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_batch* b, double* out_dev, double* sums_dev, void* hip_stream) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  if (c->remote) return fail(GKLHIP_ERR_UNSUPPORTED, "gklhip_pdhmm_compute_device: %s", kPdDeviceRemoteText);
  PdProblem q;
  const int rc = pd_paired_problem(b, out_dev, &q);
  return rc ? rc : pd_run_device(c, q, out_dev, sums_dev, hip_stream);
}

int gklhip_pdhmm_compute_cross_device(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_cross* x, int64_t ref_batch_pairs, double* out_dev,
                                      double* sums_dev, void* hip_stream) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  if (c->remote) return fail(GKLHIP_ERR_UNSUPPORTED, "gklhip_pdhmm_compute_cross_device: %s", kPdDeviceRemoteText);
  PdProblem q;
  const int rc = pd_cross_problem(x, ref_batch_pairs, out_dev, &q);
  return rc ? rc : pd_run_device(c, q, out_dev, sums_dev, hip_stream);
}

int gklhip_pdhmm_finalise_host(const double* sums, int64_t n, double* out) {
  if (n < 0 || (n > 0 && (!sums || !out))) return fail(GKLHIP_ERR_INVALID_ARG, "gklhip_pdhmm_finalise_host: NULL array or negative count");
  const double scale_log10 = pd_tables().initial_condition_log10;
  for (int64_t i = 0; i < n; i++) out[i] = std::log10(sums[i]) - scale_log10;   // exactly pd_finalise's expression
  return GKLHIP_OK;
}

namespace {
// The two multi-region entry points.  after == NULL: the host form (out: host arrays, no sums_out); else the device form
// (the regions' byte arrays, out[k] and sums_out[k] in HBM; never on a client context), behind *after.
int pd_cross_multi(gklhip_pdhmm_ctx* c, int32_t n_regions, const gklhip_pdhmm_cross* regions, const int64_t* ref_batch_pairs,
                   double* const* out, double* const* sums_out, int32_t* status_out, const hipStream_t* after) {
  if (n_regions <= 0) return fail(GKLHIP_ERR_INVALID_ARG, "no regions to process");
  if (!regions || !out) return fail(GKLHIP_ERR_INVALID_ARG, "regions / out_host is NULL");
  int first_rc = GKLHIP_OK, first_k = n_regions;   // the failing region with the lowest index
  std::string first_err;
  auto note = [&](int k, int rc) {   // (g_err holds region k's message)
    if (status_out) status_out[k] = rc;
    if (rc != GKLHIP_OK && k < first_k) { first_k = k; first_rc = rc; first_err = g_err; }
  };
  try {
    // the argument checks of gklhip_pdhmm_compute_cross_batched, region by region, before anything touches the device
    std::vector<PdMultiRegion> R;
    std::vector<int32_t> index;
    R.reserve((size_t)n_regions);
    for (int32_t k = 0; k < n_regions; k++) {
      PdMultiRegion r;
      r.out = out[k];
      r.sums_out = after && sums_out ? sums_out[k] : nullptr;
      const int rc = pd_cross_problem(&regions[k], ref_batch_pairs ? ref_batch_pairs[k] : 0, r.out, &r.q);
      r.q.in_hbm = after != nullptr;
      note(k, rc);
      if (rc == GKLHIP_OK) { R.push_back(r); index.push_back(k); }
    }
    if (R.empty()) return fail(first_rc, "%s", first_err.c_str());
    PdMultiFit fit;
    for (const PdMultiRegion& r : R) fit.take(r.q);
    const bool fits = !c->remote && R.size() <= (size_t)kPdMaxRegions && fit.fits();
    if (!fits) {
      // a client context, or a call over the limits: region by region through the single-call path (same results).
      // last_routing: the sums, last_kernel_ms: the sum of the calls' kernel times
      int32_t routing[3] = {0, 0, 0};
      float ms = 0.f;
      for (size_t i = 0; i < R.size(); i++) {
        if (!c->remote) pd_count(c->device, 1, 0, 1);
        note(index[i], after ? pd_run_device(c, R[i].q, R[i].out, R[i].sums_out, *after) : pd_run(c, R[i].q, R[i].out));
        std::lock_guard<std::mutex> lock(c->mu);
        ms += c->last_ms;
        for (int j = 0; j < 3; j++) routing[j] += c->last_routing[j];
      }
      std::lock_guard<std::mutex> lock(c->mu);
      c->last_ms = ms;
      for (int j = 0; j < 3; j++) c->last_routing[j] = routing[j];
    } else {
      std::lock_guard<std::mutex> lock(c->mu);
      const int rc = pd_fenced(c, [&] { return pd_run_multi_locked(c, R, after); });
      pd_count(c->device, (int64_t)R.size(), R.size() > 1 ? (int64_t)R.size() : 0, 1);
      for (size_t i = 0; i < R.size(); i++) {
        if (rc != GKLHIP_OK) { note(index[i], rc); continue; }   // (g_err: the launch set's message)
        note(index[i], R[i].flag != 0 ? fail(GKLHIP_ERR_INVALID_ARG, "%s", kPdInputErrorText) : GKLHIP_OK);
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(GKLHIP_ERR_OOM, "host memory allocation failed");
  } catch (...) {
    return fail(GKLHIP_ERR_HIP, "unexpected C++ exception");
  }
  return first_rc == GKLHIP_OK ? GKLHIP_OK : fail(first_rc, "%s", first_err.c_str());
}
}  // namespace

int gklhip_pdhmm_compute_cross_multi(gklhip_pdhmm_ctx* c, int32_t n_regions, const gklhip_pdhmm_cross* regions, const int64_t* ref_batch_pairs,
                                     double* const* out_host, int32_t* status_out) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  return pd_cross_multi(c, n_regions, regions, ref_batch_pairs, out_host, nullptr, status_out, nullptr);
}

int gklhip_pdhmm_compute_cross_multi_device(gklhip_pdhmm_ctx* c, int32_t n_regions, const gklhip_pdhmm_cross* dev_regions,
                                            const int64_t* ref_batch_pairs, double* const* out_dev, double* const* sums_dev,
                                            int32_t* status_out, void* hip_stream) {
  if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL (initNative not called)");
  if (c->remote) return fail(GKLHIP_ERR_UNSUPPORTED, "gklhip_pdhmm_compute_cross_multi_device: %s", kPdDeviceRemoteText);
  const hipStream_t after = static_cast<hipStream_t>(hip_stream);
  return pd_cross_multi(c, n_regions, dev_regions, ref_batch_pairs, out_dev, sums_dev, status_out, &after);
}

int gklhip_pdhmm_combine_counts(int device, int64_t out[3], int reset) {
  if (!out) return fail(GKLHIP_ERR_INVALID_ARG, "NULL argument");
  if (device >= kPdCountDevices) return fail(GKLHIP_ERR_INVALID_ARG, "device %d", device);
  out[0] = out[1] = out[2] = 0;
  for (int d = device < 0 ? 0 : device; d < (device < 0 ? kPdCountDevices : device + 1); d++)
    for (int i = 0; i < 3; i++) out[i] += reset ? g_pd_counts[d][i].exchange(0) : g_pd_counts[d][i].load();
  return GKLHIP_OK;
}

}  // extern "C"
