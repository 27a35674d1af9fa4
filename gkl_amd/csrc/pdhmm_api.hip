// C-ABI implementation (include/gkl_hip_pdhmm.h) of the MI355X PDHMM path.  Compiled WITHOUT the
// fp64 flush-to-zero flag of the PairHMM translation unit: the reference's PDHMM never touches
// MXCSR (no _MM_SET_FLUSH_ZERO_MODE anywhere under src/main/native/pdhmm).
#include <hip/hip_runtime.h>
#include <immintrin.h>
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
#include "pairhmm_plan.h"
#include "pdhmm_job_layout.h"      // pd_up, PdInputLayout, PdJobOffsets / PdJobLayout, PdTabxLayout
#include "hip_host_common.h"      // g_err / fail / guarded / HIP_TRY, DevBuf, PinBuf
#include "pairhmm_host_finalize.h"   // gklhip::WorkerPool: persistent threads for the host log10

using namespace gklhip;

namespace {
// ---- host tables: ProbabilityCache of pdhmm-common.h:139-192 (exact 1/ln10 here, unlike PairHMM) ----
constexpr int kPdMaxQual = 254;
constexpr int kPdMmSize = ((kPdMaxQual + 1) * (kPdMaxQual + 2)) >> 1;

struct PdTables {
  std::vector<double> q2err, mm;
  double initial_condition, initial_condition_log10;
};

const PdTables& pd_tables() {
  static const PdTables t = [] {
    PdTables r;
    std::vector<double> jac(80001);
    for (int k = 0; k < 80001; k++) jac[k] = std::log10(1.0 + std::pow(10.0, -k * 0.0001));  // MathUtils.cc:84-87
    auto round_half_away = [](double d) { return d > 0.0 ? (int)(d + 0.5) : (int)(d - 0.5); };
    auto log10_sum = [&](double a, double b) {  // MathUtils.cc:91-109 (a <= b after the swap)
      if (a > b) std::swap(a, b);
      if (a == -1e10) return b;
      const double diff = b - a;
      return b + (diff < 8.0 ? jac[round_half_away(diff * (1.0 / 0.0001))] : 0.0);
    };
    const double inv_ln10 = 1.0 / std::log(10);
    r.mm.resize(kPdMmSize);
    for (int i = 0, offset = 0; i <= kPdMaxQual; offset += ++i)
      for (int j = 0; j <= i; j++) {
        const double l10 = std::log1p(-std::min(1.0, std::pow(10, log10_sum(-0.1 * i, -0.1 * j)))) * inv_ln10;
        r.mm[offset + j] = std::pow(10, l10);
      }
    r.q2err.resize(kPdMaxQual + 1);
    for (int q = 0; q <= kPdMaxQual; q++) r.q2err[q] = std::pow(10.0, (double)q / -10.0);
    r.initial_condition = std::pow(2, 1020);                       // MathUtils.cc:31
    r.initial_condition_log10 = std::log10(r.initial_condition);  // :32
    return r;
  }();
  return t;
}

}  // namespace

struct gklhip_pdhmm_ctx {
  // a client context of the server (gklhip_pdhmm_connect, GKL_HIP_SERVER): no stream, no event, no buffer -- no HIP
  // call is made for it; fma_mode / tail_mode travel with every call, last_ms / last_routing come back with the reply
  gklhip_pd_remote::Client* remote = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t dev_ev = nullptr;          // device-resident calls: recorded on the caller's stream, waited for by `stream`
  // big paired calls are cut into slices of pairs whose kernels run while later slices still cross PCIe (pd_run_locked)
  static constexpr int kMaxSlices = 8;
  hipStream_t up_stream = nullptr;
  gklhip::WorkerPool workers;           // host log10 of the sums: three helpers from 4096 pairs on
  std::vector<uint32_t> class_stamp;    // cross layout's class discovery: last haplotype that showed a (base, flags) pair
  uint32_t class_stamp_id = 0;
  hipEvent_t up_ev[kMaxSlices] = {}, sl_ev0[kMaxSlices] = {}, sl_ev1[kMaxSlices] = {};
  int pipeline = 1;                     // GKL_HIP_PDHMM_PIPELINE=0: one slice whatever the size
  std::mutex mu;
  DevBuf tables, inputs, entries, entries_tab, sums, misc, carry, jobs, tabx;
  PackScratch pack_scratch;
  PinBuf stage_in, stage_jobs, sums_pin;   // small calls: ONE copy per device buffer instead of one per array (9 + 17 of them)
  float last_ms = 0.f;
  int32_t last_routing[3] = {0, 0, 0};  // last cross call: haplotype items by kernel (table / predicate / byte-comparing); last paired call: packed jobs by kernel
  int use_table = 1;                    // GKL_HIP_PDHMM_TABLE=0: never route to the table kernel
  int fma_mode = 1;  // 1 = arithmetic of GKL's AVX-512 object (default), 0 = of its AVX2 object
  int tail_mode = 1; // 1 (default) = the last `batch mod SIMD width` pairs of every reference batch take the scalar engine's arithmetic, like GKL; 0 = vector arithmetic everywhere
};

namespace {
// The fence around a launch path (pd_run_locked, pd_run_multi_locked; c->mu is held).  No C++ exception leaves the C ABI
// (a host vector that cannot grow, a helper thread that cannot start): it becomes a status like any other error.  An error
// return must not leave asynchronous copies from the call's host vectors (or the caller's arrays) in flight when those go
// out of scope: both streams are drained first (a multi-region call never uses up_stream: idle there, the wait returns at once).
template <typename F>
int pd_fenced(gklhip_pdhmm_ctx* c, F&& launch_path) {
  const int rc = guarded(launch_path);
  if (rc != GKLHIP_OK) {
    const std::string keep = g_err;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    (void)hipGetLastError();
    g_err = keep;
  }
  return rc;
}
}  // namespace

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
// Shared by the two entry points.  Paired layout: n_read_items == n_hap_items == n_pairs, cross_haps = 0.
// Cross layout: n_pairs == n_read_items * n_hap_items, cross_haps = n_hap_items, pair p = (p / n_haps, p % n_haps).
struct PdProblem {
  int64_t n_pairs;
  int32_t n_read_items, n_hap_items, cross_haps, max_hap_len, max_read_len;
  const int8_t *hap_bases, *hap_pdbases, *read_bases, *read_qual, *read_ins_qual, *read_del_qual, *gcp;
  const int64_t *hap_lengths, *read_lengths;
  // cross layout, reference-tail mode: the reference cuts the read-major pair list into batches of this many pairs
  // (JavaData.h:83-101) and each batch has its own scalar tail; 0 = the whole cross product is one batch
  int64_t ref_batch_pairs;
  // a device-resident call (gklhip_pdhmm_compute_device / _cross_device): the seven byte arrays are HBM addresses on the
  // context's device -- no host code reads through them; the two length arrays are host arrays as always
  bool in_hbm = false;
};

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

// Where a device-resident call leaves its results (HBM of the context's device) and the caller's stream, behind whose
// work the call is ordered.
struct PdDeviceOut {
  double* out;        // [n_pairs] log10 likelihoods
  double* sums;       // [n_pairs] raw sums, or NULL
  hipStream_t after;  // NULL: HIP's default stream
};

// dev == NULL: a host call, results to out_host; else a device-resident call (q.in_hbm), results to *dev.
int pd_run_locked(gklhip_pdhmm_ctx* c, const PdProblem& q, double* out_host, const PdDeviceOut* dev = nullptr);

// Does the haplotype hold a base outside ACGTN?  (Such columns need the byte-comparing step: the job goes to the full kernel.)
bool has_odd_base_scalar(const int8_t* b, int64_t n) {
  unsigned ok = 1;
  for (int64_t j = 0; j < n; j++)
    ok &= (unsigned)(b[j] == 'A') | (unsigned)(b[j] == 'C') | (unsigned)(b[j] == 'G') | (unsigned)(b[j] == 'T') | (unsigned)(b[j] == 'N');
  return !ok;
}
__attribute__((target("avx2"))) bool has_odd_base_avx2(const int8_t* b, int64_t n) {
  const __m256i cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'), cG = _mm256_set1_epi8('G'), cT = _mm256_set1_epi8('T'),
                cN = _mm256_set1_epi8('N');
  __m256i all = _mm256_set1_epi8((char)0xff);
  int64_t j = 0;
  for (; j + 32 <= n; j += 32) {
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(b + j));
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, cA), _mm256_cmpeq_epi8(v, cC)),
                                                       _mm256_or_si256(_mm256_cmpeq_epi8(v, cG), _mm256_cmpeq_epi8(v, cT))),
                                       _mm256_cmpeq_epi8(v, cN));
    all = _mm256_and_si256(all, ok);
  }
  if (_mm256_movemask_epi8(all) != -1) return true;
  return has_odd_base_scalar(b + j, n - j);
}
bool has_odd_base(const int8_t* b, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  return avx2 ? has_odd_base_avx2(b, n) : has_odd_base_scalar(b, n);
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

constexpr size_t kPdStageBytes = (size_t)4 << 20;
// misc: 64 int32 of flags and job counters (the first 256 bytes, cleared by every call), then the per-region input-error
// flags of a multi-region call
constexpr size_t kPdMiscBytes = 256 + 4 * (size_t)kPdMaxRegions;
// Up to this many pairs (1 MB of sums) the kernels store the sums straight into pinned host memory (pd_plan_counts:
// sums_direct).  The host form of a multi-region call has no other way to return them, so this is also the most pairs a
// shared launch set takes (the device form, whose sums stay in HBM, keeps the same limit): both paths depend on the
// one constant.
constexpr size_t kPdMultiMaxPairs = 131072;
// Padded input bytes (haplotype bases + the five read arrays) from which a paired call of 65 536 pairs or more is cut
// into upload slices (pd_plan_slices), and from which a call too big to stage leaves its copies to a helper thread
// (PdUploads::start).
constexpr size_t kPdSliceMinBytes = (size_t)64 << 20, kPdHelperUploadBytes = (size_t)8 << 20;
static_assert(kPdLaneRowBytes == kLanes * sizeof(PlanLane), "pdhmm_job_layout.h sizes a lane row for this wavefront");
// The int32 words of `misc` that a call uses (the first 64 are cleared by every call; a GKL_PD_PROF build keeps its
// cycle counts in words 32-63).  kPdMiscNext*: job counters of the persistent launches (PdArgs::next).
enum PdMiscWord : int {
  kPdMiscInputError = 0,     // single call: PDHMM_INPUT_DATA_ERROR (PdArgs::status)
  kPdMiscNext = 1,           // the predicate launch that is not a slice's
  kPdMiscNextTail = 2,
  kPdMiscNextFull = 3,
  kPdMiscNextTab = 4,        // cross layout's table launch
  kPdMiscFullCount = 5,      // length of the full launch's job list (PdArgs::full_count)
  kPdMiscHotCount = 6,       // paired table route: length of the closing predicate launch's list
  kPdMiscNextSliceTab = 8,   // + k: paired layout, slice k's table launch
  kPdMiscNextSliceHot = 16,  // + k: ... its predicate launch
  kPdMiscRegionFlags = 64,   // + k: multi-region call, region k's input-error flag
};
constexpr int kPdMiscStatusWords = 8;   // what a single call reads back
static_assert(kPdMiscNextSliceTab + gklhip_pdhmm_ctx::kMaxSlices <= kPdMiscNextSliceHot &&
              kPdMiscNextSliceHot + gklhip_pdhmm_ctx::kMaxSlices <= 32, "the slices' job counters stay clear of each other");
static_assert(kPdMiscHotCount < kPdMiscStatusWords && 4 * kPdMiscRegionFlags == 256, "status read-back; the flags follow the cleared words");

// The nine input arrays of a problem, in the order they are sent.  The layout's rows are the problem's own in a single
// call and the common, possibly longer ones in a multi-region call.
struct PdInputArray {
  size_t offset;            // of the array in the layout
  const char* src;
  size_t src_row, dst_row;  // bytes per item in the caller's array / in the layout
  size_t n_items;
  bool hap;                 // one item per haplotype item (else: per read item)
  bool on_host;             // src is host memory: the lengths always, the byte arrays unless the problem's inputs are in HBM
};
struct PdInputArrays {
  PdInputArray v[9];
  const PdInputArray* begin() const { return v; }
  const PdInputArray* end() const { return v + 9; }
};
PdInputArrays pd_input_arrays(const PdInputLayout& in, const PdProblem& q) {
  const size_t qh = (size_t)q.max_hap_len, qr = (size_t)q.max_read_len, nh = (size_t)q.n_hap_items, nr = (size_t)q.n_read_items;
  auto bytes = [](const void* p) { return static_cast<const char*>(p); };
  const bool host = !q.in_hbm;
  return {{{in.o_hl, bytes(q.hap_lengths), 8, 8, nh, true, true}, {in.o_rl, bytes(q.read_lengths), 8, 8, nr, false, true},
           {in.o_hb, bytes(q.hap_bases), qh, in.hap_row, nh, true, host}, {in.o_hp, bytes(q.hap_pdbases), qh, in.hap_row, nh, true, host},
           {in.o_rb, bytes(q.read_bases), qr, in.read_row, nr, false, host}, {in.o_rq, bytes(q.read_qual), qr, in.read_row, nr, false, host},
           {in.o_ri, bytes(q.read_ins_qual), qr, in.read_row, nr, false, host}, {in.o_rd, bytes(q.read_del_qual), qr, in.read_row, nr, false, host},
           {in.o_gc, bytes(q.gcp), qr, in.read_row, nr, false, host}}};
}
// Cross layout: reads are packed into 64-lane chunks by best fit within windows of this many reads.  The chunks are reused
// for every haplotype, so a fuller chunk pays off nh times: 2048 fills 99.2 % of the lanes on the reference's fixture
// (192, the paired layout's window: 97.7 %).
constexpr int kPdCrossWindow = 2048;
// The cross layout's plan of ONE region call (one computeLikelihoods cross product): the packing of its reads, the
// order and routing of its haplotypes, its striped reads and its tail pairs -- everything in the call's own indices.
// pd_run_locked launches one plan; pd_run_multi_locked (below) concatenates several.
struct PdCrossPlan {
  std::vector<int32_t> job_pair, job_steps;    // listed jobs: one per (read that needs more than 64 lanes, haplotype)
  std::vector<uint8_t> job_striped;
  std::vector<PlanLane> cross_lanes;           // [chunk][64] = {read item, block}
  std::vector<int32_t> hap_order, chunk_steps, chunk_rep;
  size_t n_tail = 0;
  std::vector<PlanLane> tail_lanes;
  std::vector<int32_t> tail_pair, tail_steps;
  std::vector<uint8_t> tail_striped;
  std::vector<uint8_t> hap_ncls;
  std::vector<uint32_t> class_codes;
  size_t n_clean_haps = 0, n_tab_haps = 0;
};

// Appends the reference-tail job of one pair: a job of its own for the scalar-arithmetic launch (a lane row of the pair's
// row blocks, or a striped job when the read needs more than 64 lanes).
void pd_push_tail_job(PdCrossPlan* plan, int32_t pair, int read_len, int hap_len) {
  const int nb = blocks_for(read_len, kPdRpl);
  plan->tail_pair.push_back(pair);
  plan->tail_striped.push_back(nb > kLanes ? 1 : 0);
  plan->tail_steps.push_back(hap_len + std::min(nb, kLanes) - 1);
  plan->tail_lanes.resize(plan->tail_lanes.size() + kLanes, PlanLane{-1, 0});
  if (nb <= kLanes)
    for (int b = 0; b < nb; b++) plan->tail_lanes[plan->tail_lanes.size() - kLanes + (size_t)b] = PlanLane{pair, b};
  plan->n_tail = plan->tail_pair.size();
}

void pd_plan_cross_jobs(gklhip_pdhmm_ctx* c, const PdProblem& q, PdCrossPlan* plan) {
  const size_t n = (size_t)q.n_pairs, nh = (size_t)q.n_hap_items, nr = (size_t)q.n_read_items;
  const int cross = q.cross_haps;
  auto read_len_of = [&](size_t p) { return (int)q.read_lengths[p / (size_t)cross]; };
  auto hap_len_of = [&](size_t p) { return (int)q.hap_lengths[p % (size_t)cross]; };
  auto &job_pair = plan->job_pair, &job_steps = plan->job_steps, &hap_order = plan->hap_order, &chunk_steps = plan->chunk_steps,
       &chunk_rep = plan->chunk_rep;
  auto& job_striped = plan->job_striped;
  auto& cross_lanes = plan->cross_lanes;
  // reads are packed into 64-lane chunks ONCE; every chunk meets every haplotype (longest haplotypes first).
  std::vector<int64_t> read_off(nr + 1, 0);
  for (size_t r = 0; r < nr; r++) read_off[r + 1] = read_off[r] + q.read_lengths[r];
  std::vector<int32_t> shorts;
  shorts.reserve(nr);
  for (size_t r = 0; r < nr; r++) {
    if (blocks_for((int)q.read_lengths[r], kPdRpl) <= kLanes) { shorts.push_back((int32_t)r); continue; }
    for (size_t h = 0; h < nh; h++) {  // a read that needs more than 64 lanes (64 x kPdRpl = 384 bases or more): one striped job per haplotype
      job_pair.push_back((int32_t)(r * nh + h)); job_striped.push_back(1); job_steps.push_back(0);
    }
  }
  const int made = pack_reads_windowed(shorts.data(), (int)shorts.size(), read_off.data(), kPdRpl, kPdCrossWindow, &cross_lanes, nullptr);
  chunk_steps.assign((size_t)made, 0);
  chunk_rep.assign((size_t)made, 0);
  for (int k = 0; k < made; k++) {
    const PlanLane* row = cross_lanes.data() + (size_t)k * kLanes;
    int32_t rep = -1, top = 0;
    for (int l = 0; l < kLanes; l++) {
      if (row[l].read < 0) continue;
      if (rep < 0) rep = row[l].read;
      top = std::max(top, row[l].block);
    }
    chunk_steps[(size_t)k] = top;
    chunk_rep[(size_t)k] = rep;
  }
  hap_order.resize(nh);
  for (size_t h = 0; h < nh; h++) hap_order[h] = (int32_t)h;
  std::stable_sort(hap_order.begin(), hap_order.end(),
                   [&](int32_t x, int32_t y) { return q.hap_lengths[x] > q.hap_lengths[y]; });
  // "Reference tail" of the cross product: computeLikelihoods expands it into read-major pairs, batch by batch
  // (JavaData.h:177-242), and computePDHMM finishes the last `batch mod SIMD width` pairs of EVERY batch with the
  // scalar engine (pdhmm.h:1264-1268).  The main launch computes all pairs with the vector arithmetic; the pairs at
  // those positions are then recomputed by the scalar-arithmetic instantiation and overwrite their sums.
  if (c->tail_mode == 1) {
    const size_t width = c->fma_mode ? 8 : 4;
    const size_t per = q.ref_batch_pairs > 0 ? (size_t)std::min<int64_t>(q.ref_batch_pairs, (int64_t)n) : n;
    for (size_t start = 0; start < n; start += per) {
      const size_t nb_pairs = std::min(per, n - start);
      for (size_t i = start + nb_pairs / width * width; i < start + nb_pairs; i++)
        pd_push_tail_job(plan, (int32_t)i, read_len_of(i), hap_len_of(i));
    }
  }
}

void pd_plan_cross_routing(gklhip_pdhmm_ctx* c, const PdProblem& q, PdCrossPlan* plan) {
  const size_t nh = (size_t)q.n_hap_items;
  const int cross = q.cross_haps;
  auto& hap_order = plan->hap_order;
  auto& hap_ncls = plan->hap_ncls;
  auto& class_codes = plan->class_codes;
  size_t &n_clean_haps = plan->n_clean_haps, &n_tab_haps = plan->n_tab_haps;
  std::vector<uint8_t> hap_odd;
  if (cross) {
    hap_odd.assign(nh, 0);
    for (size_t h = 0; h < nh; h++) hap_odd[h] = has_odd_base(q.hap_bases + h * (size_t)q.max_hap_len, q.hap_lengths[h]) ? 1 : 0;
  }
  n_clean_haps = nh; n_tab_haps = 0;
  // cross layout: a clean haplotype whose columns fall into at most kPdTabClasses classes of (base, SNP alleles, 'N')
  // goes to the table kernel (pdhmm_fwd_tab_kernel); class c of haplotype h has the match bits class_codes[8 h + c]
  if (cross) {
    hap_ncls.assign(nh, 0);
    class_codes.assign(nh * 8, 0u);
    for (size_t h = 0; h < nh && c->use_table; h++) {
      if (hap_odd[h]) continue;
      const int8_t* hb = q.hap_bases + h * (size_t)q.max_hap_len;
      const int8_t* pd = q.hap_pdbases + h * (size_t)q.max_hap_len;
      uint32_t* codes = class_codes.data() + h * 8;
      int ncls = 0;
      // (a column's class is a function of its (base, flags) pair: 2^15 of them, a haplotype shows a handful -- a stamp
      //  per pair and haplotype skips the columns whose pair has been seen; this loop was 0.06 of a region call's 0.33 ms)
      if (c->class_stamp.empty()) c->class_stamp.assign(1u << 15, 0u);
      if (++c->class_stamp_id == 0u) { std::fill(c->class_stamp.begin(), c->class_stamp.end(), 0u); c->class_stamp_id = 1u; }
      const uint32_t stamp_id = c->class_stamp_id;
      uint32_t* const stamp = c->class_stamp.data();
      for (int64_t j = 0; j < q.hap_lengths[h] && ncls <= kPdTabClasses; j++) {
        // (as pdhmm_entries_kernel builds the entry's match bits)
        const uint32_t yb = (uint32_t)hb[j] & 0xffu, flags = (uint32_t)pd[j] & 0x7fu;
        uint32_t& seen = stamp[(yb << 7) | flags];
        if (seen == stamp_id) continue;
        seen = stamp_id;
        const uint32_t hot = yb == (uint32_t)'A' ? 1u : yb == (uint32_t)'C' ? 2u : yb == (uint32_t)'G' ? 4u : yb == (uint32_t)'T' ? 8u : 0u;
        const uint32_t allele = (flags & kPdSnp) ? ((flags >> 3) & 0xfu) : 0u;
        const uint32_t code = (hot << 20) | (allele << 24) | (1u << 28) | (yb == (uint32_t)'N' ? 1u << 29 : 0u);
        int k = 0;
        while (k < ncls && codes[k] != code) k++;
        if (k == ncls) {
          if (ncls < kPdTabClasses) codes[ncls] = code;
          ncls++;
        }
      }
      hap_ncls[h] = ncls <= kPdTabClasses ? (uint8_t)ncls : 0;
    }
    // order: table haplotypes, then the other clean ones, then those with odd bases (each group longest first)
    std::stable_partition(hap_order.begin(), hap_order.end(), [&](int32_t h) { return hap_odd[(size_t)h] == 0; });
    n_clean_haps = 0;
    for (size_t h = 0; h < nh; h++) n_clean_haps += hap_odd[h] == 0;
    std::stable_partition(hap_order.begin(), hap_order.begin() + (ptrdiff_t)n_clean_haps, [&](int32_t h) { return hap_ncls[(size_t)h] != 0; });
    for (size_t h = 0; h < nh; h++) n_tab_haps += hap_ncls[h] != 0;
    // The haplotypes of one region share their variant sites, hence their column classes: when the union of the table
    // haplotypes' classes still fits the table, every one of them gets the union as its list -- a wavefront that takes
    // several haplotypes with the same chunk of reads (tab_group_start below) then builds the table once.
    {
      uint32_t uni[kPdTabClasses + 1];
      int n_uni = 0;
      for (size_t h = 0; h < nh && n_uni <= kPdTabClasses; h++)
        for (int k = 0; k < (int)hap_ncls[h] && n_uni <= kPdTabClasses; k++) {
          const uint32_t code = class_codes[h * 8 + (size_t)k];
          int at = 0;
          while (at < n_uni && uni[at] != code) at++;
          if (at == n_uni) { if (n_uni < kPdTabClasses) uni[n_uni] = code; n_uni++; }
        }
      if (n_uni <= kPdTabClasses)
        for (size_t h = 0; h < nh; h++)
          if (hap_ncls[h]) { for (int k = 0; k < n_uni; k++) class_codes[h * 8 + (size_t)k] = uni[k]; hap_ncls[h] = (uint8_t)n_uni; }
    }
  }
}

// Table launch: a unit of work is (a group of consecutive table haplotypes of ONE region, a chunk of reads) -- the wavefront
// sets the chunk's rows up once per group (a twelfth of a job's time otherwise).  Groups of up to six while the launch has at
// least six units per wavefront -- sized by the units of the WHOLE launch: many small regions together fill the device, so
// they get the full groups a single one would not -- shrinking to single haplotypes over the last part of the launch's list
// (they run last and even the load out).  n_tab_haps[k]: the table haplotypes of region k (a single call: one count);
// n_cross_tab: the launch's (haplotype, chunk) jobs.  Fills tab_group_start (`start`, empty before) -- group g = entries
// [start[g], start[g + 1]) of the launch's haplotype list -- and groups[k], when asked for: the number of region k's groups.
void pd_size_tab_groups(const size_t* n_tab_haps, int K, int64_t n_cross_tab, std::vector<int32_t>* start, int32_t* groups) {
  const int64_t per_wave = n_cross_tab / (256 * 8);
  const size_t group_max = (size_t)std::max<int64_t>(1, std::min<int64_t>(6, per_wave / 6));
  size_t left = 0, at = 0;
  for (int k = 0; k < K; k++) left += n_tab_haps[k];
  for (int k = 0; k < K; k++) {
    const size_t mine = n_tab_haps[k];
    int32_t made = 0;
    for (size_t i = 0; i < mine; made++) {
      const size_t g = std::max<size_t>(1, std::min(std::min(group_max, left / 7), mine - i));
      start->push_back((int32_t)(at + i));
      i += g; left -= g;
    }
    at += mine;
    if (groups) groups[k] = made;
  }
  start->push_back((int32_t)at);
}

// The kernel arguments that a single call and a multi-region call set the same way: the input arrays, the tables, the
// entry streams, the carry rows and the job tables of PdJobOffsets (but the tail jobs': pd_launch_tail).  Everything
// else is 0 / NULL for the caller to set.
PdArgs pd_common_args(gklhip_pdhmm_ctx* c, const PdInputLayout& in, const PdJobOffsets& o, size_t n_hap_items, int32_t max_hap,
                      int32_t max_read, int entry_stride, bool table_haps) {
  unsigned char *d = c->inputs.as<unsigned char>(), *dj = c->jobs.as<unsigned char>();
  PdArgs a;
  memset(&a, 0, sizeof a);
  a.hap_bases = reinterpret_cast<const int8_t*>(d + in.o_hb);
  a.hap_pdbases = reinterpret_cast<const int8_t*>(d + in.o_hp);
  a.read_bases = reinterpret_cast<const int8_t*>(d + in.o_rb);
  a.read_qual = reinterpret_cast<const int8_t*>(d + in.o_rq);
  a.read_ins = reinterpret_cast<const int8_t*>(d + in.o_ri);
  a.read_del = reinterpret_cast<const int8_t*>(d + in.o_rd);
  a.gcp = reinterpret_cast<const int8_t*>(d + in.o_gc);
  a.hap_len = reinterpret_cast<const int64_t*>(d + in.o_hl);
  a.read_len = reinterpret_cast<const int64_t*>(d + in.o_rl);
  a.max_hap = max_hap; a.max_read = max_read;
  a.n_hap_items = (int32_t)n_hap_items;
  a.q2err = c->tables.as<double>();
  a.mm_prob = c->tables.as<double>() + pd_tables().q2err.size();
  a.entries = c->entries.as<uint32_t>();
  a.entry_stride = entry_stride;
  a.next = c->misc.as<int32_t>() + kPdMiscNext;
  a.carry = c->carry.as<double>();
  a.carry_len = entry_stride;
  a.lanes = reinterpret_cast<const LaneSlot*>(dj + o.jl);
  a.job_pair = reinterpret_cast<const int32_t*>(dj + o.jp);
  a.job_steps = reinterpret_cast<const int32_t*>(dj + o.jn);
  a.job_striped = dj + o.js;
  a.cross_lanes = reinterpret_cast<const LaneSlot*>(dj + o.cl);
  a.chunk_steps = reinterpret_cast<const int32_t*>(dj + o.cs);
  a.chunk_rep = reinterpret_cast<const int32_t*>(dj + o.cr);
  a.hap_ncls = table_haps ? dj + o.nc : nullptr;
  a.class_codes = reinterpret_cast<const uint32_t*>(dj + o.cc);
  a.entries_tab = c->entries_tab.as<uint32_t>();
  a.next_special = table_haps ? reinterpret_cast<int32_t*>(c->entries_tab.as<uint32_t>() + n_hap_items * (size_t)entry_stride) : nullptr;
  a.tab_group_start = reinterpret_cast<const int32_t*>(dj + o.tg);
  a.job_flags = dj + o.jf;
  a.full_jobs = reinterpret_cast<const int32_t*>(dj + o.fj);
  a.sb_stride = entry_stride / 64; a.ns_stride = entry_stride;
#ifdef GKL_PD_PROF
  a.prof = reinterpret_cast<unsigned long long*>(c->misc.as<char>() + 128);
#endif
  return a;
}

// One forward launch of 64-lane blocks in the context's arithmetic: the FMA instantiation of a kernel or its plain twin.
using PdFwdKernel = void (*)(PdArgs, double);
void pd_launch_fwd(const gklhip_pdhmm_ctx* c, PdFwdKernel k_fma, PdFwdKernel k_plain, int blocks, hipStream_t s, const PdArgs& a) {
  const PdFwdKernel k = c->fma_mode ? k_fma : k_plain;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64), 0, s, a, pd_tables().initial_condition);
}

// log10 of the sums with the HOST libm, like the reference (pdhmm.h:846) -- a region's 13 248 pairs are 0.13 ms of it on
// one thread, three quarters of what the call costs beyond its kernels: four threads from 4096 pairs on (persistent
// workers: a thread per call would cost more than it saves).  The pairs of K regions (a single call: one) lie behind one
// another in `sums`, region k from regions[k].pair_base on (regions[K]: the total); its values go to out[k], unless
// flags[k] says that its inputs were bad: that output stays untouched.
int pd_finalise(gklhip_pdhmm_ctx* c, const double* sums, const PdRegion* regions, int K, double* const* out, const int32_t* flags) {
  const double scale_log10 = pd_tables().initial_condition_log10;
  const std::function<void(int64_t, int64_t)> finalise = [&](int64_t lo, int64_t hi) {
    for (int k = pd_region_of_pair(regions, K, (int)lo); lo < hi; k++) {   // region by region: the inner loop is a plain one
      const int64_t base = regions[k].pair_base, end = std::min<int64_t>(hi, regions[k + 1].pair_base);
      double* const dst = out[k];
      if (flags[k] == 0)
        for (int64_t i = lo; i < end; i++) dst[i - base] = std::log10(sums[i]) - scale_log10;
      lo = end;
    }
  };
  static const int fin_threads = std::max(1, std::min(4, (int)std::thread::hardware_concurrency()));
  try {
    c->workers.parallel_for((int64_t)regions[K].pair_base, fin_threads, finalise, 4096);
  } catch (const std::bad_alloc&) {
    return fail(GKLHIP_ERR_OOM, "out of memory in the host finalisation");
  }
  return GKLHIP_OK;
}

// ==== a single call (pd_run_locked, at the end): plan, uploads, job tables, launches, finish ====

// ---- step 1: the plan.  Everything the call decides before anything of it touches the stream, on the caller's stack. ----
struct PdCallPlan {
  // A big PAIRED call (computePDHMMNative: ~1.2 KB of padded input per pair -- the x32 fixture is 498 MB, 9.5 ms of PCIe
  // against 5 ms of kernels) is cut into slices of consecutive pairs, biggest first: the helper thread sends slice after
  // slice on the upload stream and records an event behind each; the kernels of a slice -- its pairs are packed among
  // themselves -- wait for that event only, so they run while the later slices still cross the bus, and the last,
  // smallest slice leaves little to do once the bus is done.  Everything else about the call is one problem: one set of
  // device arrays, one job list (slice k = a range of listed jobs), the rare striped / odd-base / tail jobs at the end.
  int n_slices = 1;
  size_t slice_lo[gklhip_pdhmm_ctx::kMaxSlices + 1] = {};        // slice k = pairs [slice_lo[k], slice_lo[k + 1])
  int32_t slice_chunk0[gklhip_pdhmm_ctx::kMaxSlices + 1] = {};   // ... = chunks [slice_chunk0[k], slice_chunk0[k + 1]) = listed jobs n_striped + those
  // A call of the fixture's size (276 reads x 48 haplotypes) spent half its time in two dozen small copies from
  // pageable memory (~10 us each): up to kPdStageBytes the arrays are gathered in a pinned block and travel in ONE copy.
  bool staged = false;
  std::vector<int32_t> place_chunk;            // paired layout: compact packing of the pairs (pack_reads_place)
  std::vector<uint8_t> place_lane, chunk_used;
  size_t n_striped = 0;                        // paired layout: the first listed jobs are the striped ones
  PdCrossPlan x;                               // cross layout: pd_plan_cross_jobs / _routing; paired layout: its listed and tail jobs (pd_plan_paired_jobs)
  std::vector<int32_t> tab_group_start;        // (table launch; see pd_size_tab_groups)
  // the full launch's list of listed jobs: the striped ones (the first n_striped in the paired layout, all of them in
  // the cross layout) from here, flagged packed jobs appended by pdhmm_collect_kernel; its length lives in misc[kPdMiscFullCount]
  std::vector<int32_t> full_first;
  int32_t n_striped_listed = 0;                // (lives, like the vectors, until the stream is drained)
  // the counts (pd_plan_counts)
  size_t n_clean_haps = 0, n_packed = 0;       // haplotypes without an odd base (paired: every item); paired layout's packed jobs
  int n_chunks_cross = 0, n_general = 0, n_cross_jobs = 0, n_cross_tab = 0, n_tab_units = 0, n_cross_hot = 0, n_jobs = 0;
  int entry_stride = 0, n_blocks = 0;
  bool tab_paired = false, tab_paired_asm = false;
  bool sums_direct = false;                    // the kernels store the sums straight into pinned host memory
  bool paired_packed() const { return !chunk_used.empty(); }   // a paired call with at least one packed chunk: pd_launch_paired
  PdJobCounts job_counts() const {
    return PdJobCounts{(size_t)n_general, (size_t)n_chunks_cross, x.hap_order.size(), x.n_tail, place_chunk.size(), chunk_used.size(), tab_group_start.size()};
  }
};

void pd_plan_slices(const gklhip_pdhmm_ctx* c, const PdProblem& q, const PdInputLayout& in, PdCallPlan* p) {
  const size_t n = (size_t)q.n_pairs;
  p->staged = !q.in_hbm && in.total <= kPdStageBytes;   // (inputs in HBM: never through host memory, and no bus to hide: one slice)
  p->n_slices = 1;
  p->slice_lo[0] = 0; p->slice_lo[1] = n;
  if (!q.in_hbm && !q.cross_haps && c->pipeline && n >= 65536 && in.hap_bytes + 5 * in.read_bytes >= kPdSliceMinBytes) {
    static const double kShare[] = {0.28, 0.24, 0.19, 0.13, 0.09, 0.05, 0.02};
    p->n_slices = (int)(sizeof kShare / sizeof kShare[0]);
    double acc = 0.0;
    for (int k = 0; k < p->n_slices; k++) { p->slice_lo[k] = (size_t)(acc * (double)n) / 64 * 64; acc += kShare[k]; }
    p->slice_lo[p->n_slices] = n;
  }
}

// The paired layout's jobs: the tail pairs, the striped pairs, then the packed chunks slice by slice.
void pd_plan_paired_jobs(gklhip_pdhmm_ctx* c, const PdProblem& q, PdCallPlan* p) {
  const size_t n = (size_t)q.n_pairs;
  auto read_len_of = [&](size_t i) { return (int)q.read_lengths[i]; };
  auto hap_len_of = [&](size_t i) { return (int)q.hap_lengths[i]; };
  PdCrossPlan& x = p->x;
  // "Reference tail": GKL finishes the last `batch mod SIMD width` pairs of every vector batch with its SCALAR
  // engine (pdhmm.h:1264-1270; 8 doubles per AVX-512 vector, 4 per AVX2 vector), whose arithmetic differs in the
  // last bits (and, with deletions at a haplotype's end, by more).  In that mode those pairs get jobs of their own,
  // run by the scalar-arithmetic instantiation of the kernel.
  const size_t n_vec = n - (c->tail_mode == 1 ? n % (size_t)(c->fma_mode ? 8 : 4) : 0);
  for (size_t i = n_vec; i < n; i++) pd_push_tail_job(&x, (int32_t)i, read_len_of(i), hap_len_of(i));
  // short pairs, ordered by haplotype length so that wavefront mates finish together, are packed best-fit
  // into 64-lane chunks; a read that needs more than 64 lanes becomes a striped job
  std::vector<int64_t> pair_off(n + 1, 0);  // pack_reads_windowed() addresses reads through offsets
  for (size_t i = 0; i < n; i++) pair_off[i + 1] = pair_off[i] + read_len_of(i);
  for (size_t i = 0; i < n_vec; i++) {
    if (blocks_for(read_len_of(i), kPdRpl) <= kLanes) continue;
    x.job_pair.push_back((int32_t)i); x.job_striped.push_back(1); x.job_steps.push_back(0);  // (a striped job's lane row stays unused)
  }
  // compact packing (5 bytes per pair); pdhmm_expand_kernel turns it into the lane rows on the device.  Slice by slice
  // (one slice: the whole batch): the pairs of a slice share chunks among themselves only, chunk numbers run on.
  const size_t n_striped = p->n_striped = x.job_pair.size();
  p->place_chunk.assign(n, -1);
  p->place_lane.assign(n, 0);
  std::vector<int32_t> shorts, cnt;
  shorts.reserve(n);
  for (int k = 0; k < p->n_slices; k++) {
    const size_t lo = std::min(p->slice_lo[k], n_vec), hi = std::min(p->slice_lo[k + 1], n_vec);
    p->slice_chunk0[k] = (int32_t)p->chunk_used.size();
    // counting sort by haplotype length, longest first (the big jobs start first)
    cnt.assign((size_t)q.max_hap_len + 2, 0);
    size_t n_short = 0;
    for (size_t i = lo; i < hi; i++)
      if (blocks_for(read_len_of(i), kPdRpl) <= kLanes) { cnt[(size_t)hap_len_of(i)]++; n_short++; }
    int32_t acc = 0;
    for (int64_t h = q.max_hap_len; h >= 0; h--) { const int32_t m = cnt[(size_t)h]; cnt[(size_t)h] = acc; acc += m; }
    shorts.resize(n_short);
    for (size_t i = lo; i < hi; i++)
      if (blocks_for(read_len_of(i), kPdRpl) <= kLanes) shorts[(size_t)cnt[(size_t)hap_len_of(i)]++] = (int32_t)i;
    const int made = pack_reads_place(shorts.data(), (int)shorts.size(), pair_off.data(), kPdRpl, 192, p->place_chunk.data(),
                                      p->place_lane.data(), &p->chunk_used, nullptr, &c->pack_scratch);
    const size_t j0 = n_striped + (size_t)p->slice_chunk0[k];
    x.job_pair.resize(j0 + (size_t)made, -1);
    x.job_steps.resize(j0 + (size_t)made, 0);
    x.job_striped.resize(j0 + (size_t)made, 0);
    for (const int32_t i : shorts) {
      const size_t j = n_striped + (size_t)p->place_chunk[(size_t)i];
      if (x.job_pair[j] < 0) x.job_pair[j] = i;
      x.job_steps[j] = std::max(x.job_steps[j], (int32_t)(hap_len_of((size_t)i) + blocks_for(read_len_of((size_t)i), kPdRpl) - 1));
    }
  }
  p->slice_chunk0[p->n_slices] = (int32_t)p->chunk_used.size();
}

// The figures that follow from the jobs and the routing: what every launch is sized by.
int pd_plan_counts(gklhip_pdhmm_ctx* c, const PdProblem& q, PdCallPlan* p) {
  const int cross = q.cross_haps;
  const size_t n = (size_t)q.n_pairs, nh = (size_t)q.n_hap_items, n_tab_haps = p->x.n_tab_haps;
  p->n_clean_haps = cross ? p->x.n_clean_haps : nh;
  p->n_chunks_cross = (int)p->x.chunk_steps.size();
  const int64_t n_cross_jobs64 = (int64_t)p->n_chunks_cross * (int64_t)(cross ? nh : 0);
  if (n_cross_jobs64 + (int64_t)p->x.job_pair.size() > 0x7fffffffLL) return fail(GKLHIP_ERR_INVALID_ARG, "too many jobs");
  p->n_cross_jobs = (int)n_cross_jobs64;
  p->n_cross_tab = cross ? (int)((int64_t)p->n_chunks_cross * (int64_t)n_tab_haps) : 0;
  if (p->n_cross_tab > 0) pd_size_tab_groups(&n_tab_haps, 1, p->n_cross_tab, &p->tab_group_start, nullptr);
  p->n_tab_units = p->tab_group_start.empty() ? 0 : (int)((int64_t)p->n_chunks_cross * (int64_t)(p->tab_group_start.size() - 1));
  p->n_cross_hot = cross ? (int)((int64_t)p->n_chunks_cross * (int64_t)(p->n_clean_haps - n_tab_haps)) : 0;
  p->n_general = (int)p->x.job_pair.size();
  p->n_jobs = p->n_cross_jobs + p->n_general;
  p->entry_stride = (q.max_hap_len + 2 * kLanes + 4 + 63) / 64 * 64;   // 64 idle, the columns, 63 skew + 4 look-ahead
  p->n_blocks = std::max(1, std::min(std::max(p->n_jobs, (int)p->x.n_tail), 256 * 8));
  // Paired layout through the table kernel (pdhmm_fwd_tab_paired_kernel): classes, special columns and the routing of the
  // jobs are found on the device.  Needs the program's 32-bit entry offsets to reach every item's stream and the step
  // marks of a job to fit the special kernel's LDS.
  p->n_packed = cross ? 0 : (size_t)p->n_general - p->n_striped;
  p->tab_paired = !cross && c->use_table && p->n_packed > 0 && nh * (size_t)p->entry_stride * 4 < ((size_t)1 << 32) && p->entry_stride <= 12 * 1024;
  p->tab_paired_asm = p->tab_paired && c->fma_mode == 1 && GKL_PD_ASM == 2;   // (the C++ step loops ballot on the lanes' own entries)
  // A region-sized call (up to kPdMultiMaxPairs = 1 MB of sums): the kernels store the sums -- write-only, one store per pair --
  // straight into the pinned host block (posted writes over PCIe) instead of a device array that a copy then fetches: one
  // copy launch (~15 us of a 0.28 ms call) less.
  p->sums_direct = !q.in_hbm && n <= kPdMultiMaxPairs;   // (a device-resident call: the sums stay in c->sums for pdhmm_finalise_kernel)
  p->n_striped_listed = cross ? p->n_general : (int32_t)p->n_striped;
  p->full_first.resize((size_t)p->n_striped_listed);
  for (int32_t k = 0; k < p->n_striped_listed; k++) p->full_first[(size_t)k] = k;
  return GKLHIP_OK;
}

// ---- step 2: the nine input arrays go to the device ----
// The nine input copies (the paired layout of a big batch is hundreds of MB of padded [pair][maxLen] arrays: the
// calls alone -- pinning the caller's pages -- take milliseconds): a helper thread issues them while the caller builds
// the jobs; both meet before anything else goes onto the stream (a sliced call: slice by slice, see PdCallPlan).
struct PdUploads {
  hipError_t err = hipSuccess;
  std::thread th;
  std::atomic<int> recorded{0};   // slices whose upload event has been recorded (or given up on)
  ~PdUploads() { if (th.joinable()) th.join(); }   // (an early error return of the call)

  // one pinned block and one copy (staged), the copies inline, or the helper thread
  int start(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdInputLayout& in, const PdCallPlan& p) {
    int rc;
    if ((rc = c->inputs.reserve(in.total))) return rc;
    if (p.staged) {
      if ((rc = c->stage_in.reserve(in.total))) return rc;
      unsigned char* h = c->stage_in.as<unsigned char>();
      for (const PdInputArray& v : pd_input_arrays(in, q)) memcpy(h + v.offset, v.src, v.n_items * v.src_row);
      HIP_TRY(hipMemcpyAsync(c->inputs.p, h, in.total, hipMemcpyHostToDevice, c->stream));
    } else if (!q.in_hbm && (p.n_slices > 1 || in.hap_bytes + 5 * in.read_bytes >= kPdHelperUploadBytes)) {
      // (inputs in HBM: the byte arrays are copied device to device into the context's layout -- a fraction of a
      //  millisecond for the largest call, no pages to pin: the copies are enqueued inline below)
      th = std::thread([this, c, &q, &in, &p] { send(c, q, in, p); });
    } else {
      send(c, q, in, p);
    }
    return GKLHIP_OK;
  }
  int wait_all() {
    if (th.joinable()) th.join();
    HIP_TRY(err);
    return GKLHIP_OK;
  }
  int wait_slice(int k) {   // until slice k's upload event is recorded: the stream can then be told to wait for it
    while (recorded.load(std::memory_order_acquire) <= k) std::this_thread::yield();
    HIP_TRY(err);
    return GKLHIP_OK;
  }

 private:
  void send(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdInputLayout& in, const PdCallPlan& p) {
    (void)hipSetDevice(c->device);
    unsigned char* const d = c->inputs.as<unsigned char>();
    const hipStream_t us = p.n_slices > 1 ? c->up_stream : c->stream;
    for (int k = 0; k < p.n_slices; k++) {
      // (paired layout: item i of every array belongs to pair i; cross layout: one slice, all items)
      for (const PdInputArray& v : pd_input_arrays(in, q)) {
        const size_t i0 = p.n_slices > 1 ? p.slice_lo[k] : 0, i1 = p.n_slices > 1 ? p.slice_lo[k + 1] : v.n_items;
        if (err != hipSuccess || i1 == i0) continue;
        err = hipMemcpyAsync(d + v.offset + i0 * v.src_row, v.src + i0 * v.src_row, (i1 - i0) * v.src_row,
                             v.on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, us);
      }
      if (p.n_slices > 1) {
        if (err == hipSuccess) err = hipEventRecord(c->up_ev[k], us);
        recorded.store(k + 1, std::memory_order_release);
      }
    }
  }
};

// ---- step 3: the device buffers and the job tables ----
int pd_reserve_buffers(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdCallPlan& p, const PdTabxLayout& X) {
  const size_t stream_bytes = (size_t)q.n_hap_items * (size_t)p.entry_stride * 4;   // one entry stream per haplotype item
  int rc;
  if ((rc = c->entries.reserve(stream_bytes))) return rc;
  if (p.x.n_tab_haps && (rc = c->entries_tab.reserve(2 * stream_bytes))) return rc;   // + the next-special-column table
  if (p.tab_paired && ((rc = c->entries_tab.reserve(stream_bytes)) || (rc = c->tabx.reserve(X.total)))) return rc;
  if ((rc = c->sums.reserve((size_t)q.n_pairs * 8))) return rc;
  if ((rc = c->misc.reserve(kPdMiscBytes))) return rc;
  return c->carry.reserve((size_t)p.n_blocks * 2 * (6 * (size_t)p.entry_stride + 64) * 8);   // (carry_len = entry_stride)
}

// The single call's job tables, laid out by PdJobLayout: through the pinned block in one copy while they fit it, else
// table by table.  Clears the status words and sets the full launch's list up.
int pd_stage_tables(gklhip_pdhmm_ctx* c, const PdCallPlan& p, const PdJobLayout& L) {
  const hipStream_t s = c->stream;
  const PdCrossPlan& x = p.x;
  const size_t n_general = (size_t)p.n_general;
  int rc;
  if ((rc = c->jobs.reserve(L.total + 256))) return rc;
  unsigned char* dj = c->jobs.as<unsigned char>();
  const bool staged_jobs = L.total <= kPdStageBytes;
  if (staged_jobs && (rc = c->stage_jobs.reserve(L.total + 256))) return rc;
  unsigned char* hj = c->stage_jobs.as<unsigned char>();
  size_t staged_hi = 0;  // bytes of the staging block in use
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    if (staged_jobs) { memcpy(hj + off, src, bytes); staged_hi = std::max(staged_hi, off + bytes); return hipSuccess; }
    return hipMemcpyAsync(dj + off, src, bytes, hipMemcpyHostToDevice, s);
  };
  HIP_TRY(put(L.jp, x.job_pair.data(), n_general * 4));
  HIP_TRY(put(L.jn, x.job_steps.data(), n_general * 4));
  HIP_TRY(put(L.js, x.job_striped.data(), n_general));
  HIP_TRY(put(L.cl, x.cross_lanes.data(), x.cross_lanes.size() * sizeof(PlanLane)));
  HIP_TRY(put(L.ho, x.hap_order.data(), x.hap_order.size() * 4));
  HIP_TRY(put(L.cs, x.chunk_steps.data(), x.chunk_steps.size() * 4));
  HIP_TRY(put(L.cr, x.chunk_rep.data(), x.chunk_rep.size() * 4));
  HIP_TRY(put(L.tl, x.tail_lanes.data(), x.tail_lanes.size() * sizeof(PlanLane)));
  HIP_TRY(put(L.tp, x.tail_pair.data(), x.n_tail * 4));
  HIP_TRY(put(L.tn, x.tail_steps.data(), x.n_tail * 4));
  HIP_TRY(put(L.ts, x.tail_striped.data(), x.n_tail));
  HIP_TRY(put(L.nc, x.hap_ncls.data(), x.hap_ncls.size()));
  HIP_TRY(put(L.cc, x.class_codes.data(), x.class_codes.size() * 4));
  HIP_TRY(put(L.pc, p.place_chunk.data(), p.place_chunk.size() * 4));
  HIP_TRY(put(L.pl, p.place_lane.data(), p.place_lane.size()));
  HIP_TRY(put(L.cu, p.chunk_used.data(), p.chunk_used.size()));
  HIP_TRY(put(L.tg, p.tab_group_start.data(), p.tab_group_start.size() * 4));
  if (n_general > 0) {
    if (staged_jobs) { memset(hj + L.jf, 0, n_general); staged_hi = std::max(staged_hi, L.jf + n_general); }
    else HIP_TRY(hipMemsetAsync(dj + L.jf, 0, n_general, s));
  }
  HIP_TRY(hipMemsetAsync(c->misc.p, 0, 256, s));
#ifdef GKL_PD_PROF
  HIP_TRY(hipMemsetAsync(c->misc.as<char>() + 128 + 13 * 8, 0xff, 8, s));
  HIP_TRY(hipMemsetAsync(c->misc.as<char>() + 128 + 15 * 8, 0xff, 8, s));
#endif
  HIP_TRY(put(L.fj, p.full_first.data(), p.full_first.size() * 4));
  if (staged_jobs && staged_hi > 0) HIP_TRY(hipMemcpyAsync(dj, hj, staged_hi, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->misc.as<int32_t>() + kPdMiscFullCount, &p.n_striped_listed, 4, hipMemcpyHostToDevice, s));
  return GKLHIP_OK;
}

// What every launch of the call is given; the launches below copy it and change what is theirs.
int pd_call_args(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdInputLayout& in, const PdCallPlan& p, const PdJobLayout& L,
                 const PdTabxLayout& X, PdArgs* out) {
  const size_t n = (size_t)q.n_pairs;
  PdArgs a = pd_common_args(c, in, L, (size_t)q.n_hap_items, q.max_hap_len, q.max_read_len, p.entry_stride, p.x.n_tab_haps != 0);
  a.batch = (int32_t)n;
  a.cross_haps = q.cross_haps;
  a.sums = c->sums.as<double>();
  int rc;
  if ((rc = c->sums_pin.reserve((q.in_hbm ? 0 : n * 8) + 64))) return rc;   // (a device-resident call: the status words alone come back)
  if (p.sums_direct) {
    void* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, c->sums_pin.p, 0));
    a.sums = static_cast<double*>(dp);
  }
  a.status = c->misc.as<int32_t>() + kPdMiscInputError;
  a.n_jobs = p.n_jobs;
  a.n_cross_jobs = p.n_cross_jobs; a.n_chunks_cross = std::max(p.n_chunks_cross, 1);
  a.hap_order = reinterpret_cast<const int32_t*>(c->jobs.as<unsigned char>() + L.ho);
  a.full_count = c->misc.as<int32_t>() + kPdMiscFullCount;
  if (p.tab_paired) {
    unsigned char* dx = c->tabx.as<unsigned char>();
    a.hap_ncls_out = dx + X.nc;
    a.class_codes_out = reinterpret_cast<uint32_t*>(dx + X.cc);
    a.special_bits = p.tab_paired_asm ? reinterpret_cast<uint64_t*>(dx + X.sb) : nullptr;
    a.job_notab = dx + X.nt;
    a.job_ns = reinterpret_cast<const int32_t*>(dx + X.ns);
    HIP_TRY(hipMemsetAsync(dx + X.nt, 0, (size_t)p.n_general, c->stream));
  }
  *out = a;
  return GKLHIP_OK;
}

// ---- step 4: the launches ----
// Paired layout with packed chunks: slice by slice (one slice unless the call is big, see PdCallPlan), then the closing
// launches over the lists that pdhmm_collect_kernel made.
int pd_launch_paired(gklhip_pdhmm_ctx* c, const PdCallPlan& p, const PdJobLayout& L, const PdTabxLayout& X, const PdArgs& a, PdUploads* up) {
  const hipStream_t s = c->stream;
  unsigned char *dj = c->jobs.as<unsigned char>(), *dx = c->tabx.as<unsigned char>();
  int32_t* const misc = c->misc.as<int32_t>();
  const int n_slices = p.n_slices, n_blocks = p.n_blocks;
  PdExpandArgs x;
  x.place_chunk = reinterpret_cast<const int32_t*>(dj + L.pc);
  x.place_lane = dj + L.pl;
  x.chunk_used = dj + L.cu;
  x.read_len = a.read_len;
  x.entries = a.entries; x.entry_stride = p.entry_stride;
  x.lanes = reinterpret_cast<LaneSlot*>(dj + L.jl);
  x.job_flags = dj + L.jf;
  x.hap_ncls = p.tab_paired ? dx + X.nc : nullptr;
  x.job_notab = p.tab_paired ? dx + X.nt : nullptr;
  x.n_striped = (int32_t)p.n_striped; x.rpl = kPdRpl;
  for (int k = 0; k < n_slices; k++) {
    const size_t lo = p.slice_lo[k], hi = p.slice_lo[k + 1];
    const int c0 = p.slice_chunk0[k], c1 = p.slice_chunk0[k + 1];
    const int j0 = (int)p.n_striped + c0, j1 = (int)p.n_striped + c1;
    if (n_slices > 1) {
      if (int rc = up->wait_slice(k)) return rc;
      HIP_TRY(hipStreamWaitEvent(s, c->up_ev[k], 0));
    }
    PdArgs ae = a;
    ae.item_base = (int32_t)lo;
    hipLaunchKernelGGL(pdhmm_entries_kernel, dim3((unsigned)(hi - lo)), dim3(kLanes), 0, s, ae);   // one wavefront per haplotype item
    x.pair_base = (int32_t)lo; x.n_pairs = (int32_t)hi; x.chunk_base = c0; x.n_chunks = c1;
    hipLaunchKernelGGL(pdhmm_expand_kernel, dim3((unsigned)((std::max<size_t>(hi - lo, (size_t)(c1 - c0)) + 255) / 256)), dim3(256), 0, s, x);
    if (j1 > j0)
      hipLaunchKernelGGL(pdhmm_collect_kernel, dim3((unsigned)((j1 - j0 + 255) / 256)), dim3(256), 0, s, dj + L.jf, dj + L.js, j1,
                         reinterpret_cast<int32_t*>(dj + L.fj), misc + kPdMiscFullCount, p.tab_paired ? dx + X.nt : nullptr,
                         reinterpret_cast<int32_t*>(dx + X.hj), misc + kPdMiscHotCount, j0);
    HIP_TRY(hipEventRecord(n_slices > 1 ? c->sl_ev0[k] : c->ev0, s));
    if (j1 <= j0) { if (n_slices > 1) HIP_TRY(hipEventRecord(c->sl_ev1[k], s)); continue; }
    if (p.tab_paired) {
      // table launch: the jobs' next-special-step tables first (part of the timed region: work only this route does),
      // then every listed job of the slice that is clean and whose haplotypes all have at most kPdTabClasses classes
      if (p.tab_paired_asm) {
        PdJobNsArgs na;
        na.lanes = a.lanes; na.job_steps = a.job_steps; na.job_striped = a.job_striped; na.job_flags = a.job_flags; na.job_notab = a.job_notab;
        na.read_len = a.read_len; na.hap_len = a.hap_len; na.special_bits = a.special_bits; na.sb_stride = p.entry_stride / 64;
        na.job_ns = reinterpret_cast<int32_t*>(dx + X.ns); na.ns_stride = p.entry_stride; na.rpl = kPdRpl; na.job_base = j0; na.job_end = j1;
        hipLaunchKernelGGL(pdhmm_job_special_kernel, dim3((unsigned)((j1 - j0 + kPdNsJobsPerBlock - 1) / kPdNsJobsPerBlock)), dim3(kLanes * kPdNsJobsPerBlock),
                           (size_t)p.entry_stride * kPdNsJobsPerBlock, s, na);
      }
      PdArgs at = a;
      at.n_cross_jobs = 0; at.job_base = j0; at.n_jobs = j1;
      at.class_codes = a.class_codes_out;
      at.next = misc + kPdMiscNextSliceTab + k;
      pd_launch_fwd(c, pdhmm_fwd_tab_paired_kernel<true>, pdhmm_fwd_tab_paired_kernel<false>, std::min(j1 - j0, n_blocks), s, at);
    } else {
      // predicate launch: walks the slice's listed jobs and skips the flagged ones
      PdArgs ah = a;
      ah.n_cross_jobs = 0; ah.job_base = j0; ah.n_jobs = j1;
      ah.full_jobs = nullptr;
      ah.next = misc + kPdMiscNextSliceHot + k;
      pd_launch_fwd(c, pdhmm_fwd_kernel<true, false, true>, pdhmm_fwd_kernel<false, false, true>, std::min(j1 - j0, n_blocks), s, ah);
    }
    if (n_slices > 1) HIP_TRY(hipEventRecord(c->sl_ev1[k], s));
  }
  if (n_slices > 1) HIP_TRY(hipEventRecord(c->ev0, s));
  if (p.tab_paired) {
    // predicate launch: the (rare) clean packed jobs with an ineligible haplotype, from the list pdhmm_collect_kernel made
    PdArgs ah = a;
    ah.n_cross_jobs = 0; ah.n_jobs = 0;
    ah.full_jobs = reinterpret_cast<const int32_t*>(dx + X.hj);
    ah.full_count = misc + kPdMiscHotCount;
    pd_launch_fwd(c, pdhmm_fwd_kernel<true, false, true>, pdhmm_fwd_kernel<false, false, true>, std::min((int)p.n_packed, n_blocks), s, ah);
  }
  PdArgs af = a;   // full launch: striped reads and haplotypes with odd bases (the list: striped jobs from the host, flagged ones from pdhmm_collect_kernel)
  af.n_cross_jobs = 0; af.n_jobs = p.n_general;
  af.next = misc + kPdMiscNextFull;
  pd_launch_fwd(c, pdhmm_fwd_kernel<true>, pdhmm_fwd_kernel<false>, std::min(p.n_general, n_blocks), s, af);
  return GKLHIP_OK;
}

// The three launches over cross jobs (a chunk of reads x a haplotype, or a group of table haplotypes), of a single call
// and of a multi-region call: the same walk with the kernels' single-region or multi-region instantiations.
struct PdCrossLaunches {
  PdFwdKernel tab[2], hot[2], full[2];     // {FMA, plain}
  bool multi;                              // the kernels find their region through PdArgs::multi_launch
  const int32_t* hap_order;                // [the table launch's haplotypes | the predicate launch's | the full launch's]
  size_t n_tab_haps, n_hot_haps;
  int tab_units, hot_units, full_units;    // cross jobs (table launch: haplotype group x chunk)
  int hot_listed, full_listed;             // listed jobs that the launch walks on top
};
void pd_launch_cross_jobs(gklhip_pdhmm_ctx* c, const PdCrossLaunches& l, const PdArgs& a, int n_blocks) {
  const hipStream_t s = c->stream;
  // table launch: cross jobs over the haplotypes with few column classes
  if (l.tab_units > 0) {
    PdArgs at = a;
    at.hap_order = l.hap_order;
    at.n_cross_jobs = at.n_jobs = l.tab_units;
    if (l.multi) at.multi_launch = kPdLaunchTab;
    at.next = c->misc.as<int32_t>() + kPdMiscNextTab;
    pd_launch_fwd(c, l.tab[0], l.tab[1], std::min(l.tab_units, n_blocks), s, at);
  }
  // predicate ("hot") launch: cross jobs over the other clean haplotypes + the listed jobs the device routes to it
  PdArgs ah = a;
  ah.hap_order = l.hap_order + l.n_tab_haps;
  ah.n_cross_jobs = l.hot_units;
  ah.n_jobs = l.hot_units + l.hot_listed;
  if (l.multi) ah.multi_launch = kPdLaunchHot;
  ah.full_jobs = nullptr;   // walks every listed job and skips the flagged ones
  if (ah.n_jobs > 0) pd_launch_fwd(c, l.hot[0], l.hot[1], std::min(ah.n_jobs, n_blocks), s, ah);
  // full launch: cross jobs over the haplotypes with odd bases + the listed jobs with a striped read or an odd haplotype
  PdArgs af = a;
  af.hap_order = l.hap_order + l.n_tab_haps + l.n_hot_haps;
  af.n_cross_jobs = l.full_units;
  af.n_jobs = l.full_units + l.full_listed;
  if (l.multi) af.multi_launch = kPdLaunchFull;
  af.next = c->misc.as<int32_t>() + kPdMiscNextFull;
  if (af.n_jobs > 0) pd_launch_fwd(c, l.full[0], l.full[1], std::min(af.n_jobs, n_blocks), s, af);
}

// Cross layout (and a paired call that holds striped reads only).
int pd_launch_cross(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdCallPlan& p, const PdArgs& a, PdUploads* up) {
  const hipStream_t s = c->stream;
  if (p.n_slices > 1) {
    // A sliced call without one packed chunk (every read striped): nothing here waits slice by slice, and the helper
    // thread may still be sending -- meet ALL the uploads before the first kernel reads the arrays.
    if (int rc = up->wait_all()) return rc;
    for (int k = 0; k < p.n_slices; k++) HIP_TRY(hipStreamWaitEvent(s, c->up_ev[k], 0));
  }
  hipLaunchKernelGGL(pdhmm_entries_kernel, dim3((unsigned)q.n_hap_items), dim3(kLanes), 0, s, a);   // one wavefront per haplotype item
  HIP_TRY(hipEventRecord(c->ev0, s));
  const PdCrossLaunches l{{pdhmm_fwd_tab_kernel<true>, pdhmm_fwd_tab_kernel<false>},
                          {pdhmm_fwd_kernel<true, false, true>, pdhmm_fwd_kernel<false, false, true>},
                          {pdhmm_fwd_kernel<true>, pdhmm_fwd_kernel<false>},
                          false, a.hap_order, p.x.n_tab_haps, p.n_clean_haps - p.x.n_tab_haps,
                          p.n_tab_units, p.n_cross_hot, p.n_cross_jobs - p.n_cross_hot - p.n_cross_tab,
                          q.cross_haps ? 0 : p.n_general,   // (cross layout: the listed jobs are striped reads, all the full kernel's)
                          p.n_general};
  pd_launch_cross_jobs(c, l, a, p.n_blocks);
  return GKLHIP_OK;
}

// The tail pairs: jobs of their own, scalar-engine arithmetic (same stream: the carry rows are free again).  `tail`: the
// scalar-arithmetic instantiation of pdhmm_fwd_kernel for the call (single or multi-region); persistent: one carry slab per block.
void pd_launch_tail(gklhip_pdhmm_ctx* c, PdFwdKernel tail, const PdArgs& a, const PdJobOffsets& o, size_t n_tail, int n_blocks) {
  unsigned char* dj = c->jobs.as<unsigned char>();
  PdArgs at = a;
  at.lanes = reinterpret_cast<const LaneSlot*>(dj + o.tl);
  at.job_pair = reinterpret_cast<const int32_t*>(dj + o.tp);
  at.job_steps = reinterpret_cast<const int32_t*>(dj + o.tn);
  at.job_striped = dj + o.ts;
  at.n_jobs = (int32_t)n_tail;
  at.n_cross_jobs = 0;
  at.job_flags = nullptr;   // every tail job is this launch's
  at.full_jobs = nullptr;
  at.next = c->misc.as<int32_t>() + kPdMiscNextTail;
  hipLaunchKernelGGL(tail, dim3((unsigned)std::min<size_t>(n_tail, (size_t)n_blocks)), dim3(64), 0, c->stream, at, pd_tables().initial_condition);
}

// ---- step 5: finish ----
// The call's clock (GKLHIP_TIMING): milliseconds since it began, at four points on the way.
struct PdCallClock {
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  double uploads = 0, jobs = 0, routing = 0, launched = 0;
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
};

// last_routing of a paired call, from the status words it read back: packed jobs by kernel (the full launch's list, the
// striped jobs included; the predicate launch's)
void pd_paired_routing(gklhip_pdhmm_ctx* c, const PdCallPlan& p, const int32_t* status) {
  const int32_t n_full_packed = status[kPdMiscFullCount] - (int32_t)p.n_striped,
                n_hot = p.tab_paired ? status[kPdMiscHotCount] : (int32_t)p.n_packed - n_full_packed;
  c->last_routing[0] = p.tab_paired ? (int32_t)p.n_packed - n_hot - n_full_packed : 0;
  c->last_routing[1] = n_hot;
  c->last_routing[2] = n_full_packed;
}

// Behind the last launch: the sums and the status words come back, the stream drains, the helper thread is met, the
// kernel time and the paired routing counts are read, the sums become the caller's log10 values.
int pd_finish(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdCallPlan& p, PdUploads* up, PdCallClock* clock, double* out_host) {
  static const bool timing = getenv("GKLHIP_TIMING") != nullptr;
  const hipStream_t s = c->stream;
  const size_t n = (size_t)q.n_pairs;
  HIP_TRY(hipEventRecord(c->ev1, s));
  HIP_TRY(hipGetLastError());
  double* sums = c->sums_pin.as<double>();
  int32_t* status = reinterpret_cast<int32_t*>(sums + n);
  if (!p.sums_direct) HIP_TRY(hipMemcpyAsync(sums, c->sums.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(status, c->misc.p, 4 * kPdMiscStatusWords, hipMemcpyDeviceToHost, s));
  clock->launched = clock->ms();
  HIP_TRY(hipStreamSynchronize(s));
  if (int rc = up->wait_all()) return rc;   // (a sliced call: the stream has waited for every upload event by now)
  HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  if (p.paired_packed() && p.n_slices > 1)   // kernel time of a sliced call: its slices' launches plus the closing ones (the waits for the bus lie between them)
    for (int k = 0; k < p.n_slices; k++) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, c->sl_ev0[k], c->sl_ev1[k]));
      c->last_ms += ms;
    }
#ifdef GKL_PD_PROF
  {  // development build: where the table kernel's wavefronts spent their cycles (s_memtime)
    unsigned long long pr[16];
    HIP_TRY(hipMemcpy(pr, c->misc.as<char>() + 128, sizeof pr, hipMemcpyDeviceToHost));
    const double tot = (double)(pr[0] + pr[1] + pr[2] + pr[3] + pr[4] + pr[5]);
    fprintf(stderr, "[pd prof] setup+table %.3f  asm runs %.3f (%llu steps)  plain x2 loop %.3f (%llu)  plain x1 loop %.3f (%llu)  general %.3f (%llu)  other %.3f  | jobs %llu, total %.3e ticks; first wavefront done at %.3f of the launch, last at 1\n",
            pr[0] / tot, pr[1] / tot, pr[8], pr[2] / tot, pr[9], pr[3] / tot, pr[10], pr[4] / tot, pr[11], pr[5] / tot, pr[12], tot, (double)(pr[13] - pr[15]) / (double)(pr[14] - pr[15]));
  }
#endif
  if (timing)
    fprintf(stderr, "[gklhip] pdhmm call: uploads enqueued %.2f ms, jobs built %.2f, routed %.2f, launched %.2f, synchronised %.2f (kernels %.2f ms), %zu pairs\n",
            clock->uploads, clock->jobs, clock->routing, clock->launched, clock->ms(), (double)c->last_ms, n);
  if (!q.cross_haps) pd_paired_routing(c, p, status);
  if (status[kPdMiscInputError] != 0)  // PDHMM_INPUT_DATA_ERROR (pdhmm-serial.cc:183-199): negative ins / del / gcp quality
    return fail(GKLHIP_ERR_INVALID_ARG, "Error while calculating pdhmm. Input arrays aren't valid.");
  PdRegion one[2] = {};   // the call as ONE region of n pairs
  one[1].pair_base = (int32_t)n;
  return pd_finalise(c, sums, one, 1, &out_host, status);   // (status[0] == 0 here)
}

// pd_finish of a device-resident call: behind the last forward or tail launch (and behind ev1: the kernel time stays the
// forward launches') pdhmm_finalise_kernel turns c->sums into the caller's log10 values in HBM -- and copies the sums
// themselves when asked to -- unless the status word reports an input error: then it writes nothing.  Only the status
// words cross the bus; one synchronisation; no host log10.
int pd_finish_device(gklhip_pdhmm_ctx* c, const PdProblem& q, const PdCallPlan& p, PdUploads* up, PdCallClock* clock, const PdDeviceOut& dev) {
  static const bool timing = getenv("GKLHIP_TIMING") != nullptr;
  const hipStream_t s = c->stream;
  const int64_t n = q.n_pairs;
  HIP_TRY(hipEventRecord(c->ev1, s));
  hipLaunchKernelGGL(pdhmm_finalise_kernel, dim3((unsigned)std::min<int64_t>((n + kPdFinaliseBlock - 1) / kPdFinaliseBlock, 2048)),
                     dim3(kPdFinaliseBlock), 0, s, c->sums.as<double>(), c->misc.as<int32_t>() + kPdMiscInputError, n,
                     pd_tables().initial_condition_log10, dev.out, dev.sums);
  HIP_TRY(hipGetLastError());
  int32_t* status = c->sums_pin.as<int32_t>();
  HIP_TRY(hipMemcpyAsync(status, c->misc.p, 4 * kPdMiscStatusWords, hipMemcpyDeviceToHost, s));
  clock->launched = clock->ms();
  HIP_TRY(hipStreamSynchronize(s));
  if (int rc = up->wait_all()) return rc;
  HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  if (timing)
    fprintf(stderr, "[gklhip] pdhmm device-resident call: copies enqueued %.2f ms, jobs built %.2f, routed %.2f, launched %.2f, synchronised %.2f (kernels %.2f ms), %lld pairs\n",
            clock->uploads, clock->jobs, clock->routing, clock->launched, clock->ms(), (double)c->last_ms, (long long)n);
  if (!q.cross_haps) pd_paired_routing(c, p, status);
  if (status[kPdMiscInputError] != 0) return fail(GKLHIP_ERR_INVALID_ARG, "Error while calculating pdhmm. Input arrays aren't valid.");
  return GKLHIP_OK;
}

// Cross layout of a device-resident call: the planners (pd_plan_cross_routing, has_odd_base) read haplotype bytes on the
// host, so hap_bases and hap_pdbases -- n_haps * max_hap_len bytes each, the small side of a cross product -- come back
// into the context's pinned block first (free here: such a call never stages its inputs), behind the caller's work, and
// the call waits for them: its one early wait.  *plan_q: the problem as the planners may read it.
int pd_fetch_haps(gklhip_pdhmm_ctx* c, const PdProblem& q, PdProblem* plan_q) {
  const size_t hap_bytes = (size_t)q.n_hap_items * (size_t)q.max_hap_len;
  if (int rc = c->stage_in.reserve(2 * hap_bytes)) return rc;
  int8_t* h = c->stage_in.as<int8_t>();
  HIP_TRY(hipMemcpyAsync(h, q.hap_bases, hap_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h + hap_bytes, q.hap_pdbases, hap_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  plan_q->hap_bases = h;
  plan_q->hap_pdbases = h + hap_bytes;
  return GKLHIP_OK;
}

int pd_run_locked(gklhip_pdhmm_ctx* c, const PdProblem& q_call, double* out_host, const PdDeviceOut* dev) {
  PdCallClock clock;
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  // q_call: the caller's arrays, what the uploads copy from; q: what the host reads while it plans -- the same, but the
  // two haplotype arrays of a device-resident cross call (pd_fetch_haps)
  PdProblem q = q_call;
  if (dev) {
    // everything the call enqueues is ordered behind what the caller's stream already holds
    HIP_TRY(hipEventRecord(c->dev_ev, dev->after));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->dev_ev, 0));
    if (q.cross_haps && (rc = pd_fetch_haps(c, q_call, &q))) return rc;
  }
  const int cross = q.cross_haps;
  const PdInputLayout in((size_t)q.n_hap_items, (size_t)q.n_read_items, (size_t)q.max_hap_len, (size_t)q.max_read_len);
  PdCallPlan plan;
  pd_plan_slices(c, q, in, &plan);
  PdUploads up;
  if ((rc = up.start(c, q_call, in, plan))) return rc;
  clock.uploads = clock.ms();
  if (cross) pd_plan_cross_jobs(c, q, &plan.x); else pd_plan_paired_jobs(c, q, &plan);
  clock.jobs = clock.ms();
  // ---- routing: the hot launch (only the two in-place step loops, see pdhmm_fwd_kernel) takes every job without a
  // striped read and without a haplotype that has a base outside ACGTN (such columns need the byte-comparing step);
  // the rest -- rare -- go to a second launch of the full kernel.  Cross layout: the host looks at the (few)
  // haplotypes and orders them by kernel.  Listed jobs (paired layout: every job): routed on the device
  // (PdArgs::job_flags) -- a host scan of a haplotype per PAIR is ~100 MB for 400k pairs.
  if (cross) pd_plan_cross_routing(c, q, &plan.x);
  const int32_t n_haps = q.n_hap_items, n_tab = (int32_t)plan.x.n_tab_haps, n_clean = (int32_t)plan.x.n_clean_haps;
  c->last_routing[0] = cross ? n_tab : 0; c->last_routing[1] = cross ? n_clean - n_tab : 0; c->last_routing[2] = cross ? n_haps - n_clean : 0;
  clock.routing = clock.ms();
  if ((rc = pd_plan_counts(c, q, &plan))) return rc;
  const PdJobLayout L(plan.job_counts());
  const PdTabxLayout X((size_t)n_haps, (size_t)plan.n_general, (size_t)plan.entry_stride, plan.tab_paired_asm);
  if ((rc = pd_reserve_buffers(c, q, plan, X))) return rc;
  if (plan.n_slices == 1 && (rc = up.wait_all())) return rc;   // (sliced call: the kernels of slice k wait for slice k's upload event)
  if ((rc = pd_stage_tables(c, plan, L))) return rc;
  PdArgs a;
  if ((rc = pd_call_args(c, q, in, plan, L, X, &a))) return rc;
  if ((rc = plan.paired_packed() ? pd_launch_paired(c, plan, L, X, a, &up) : pd_launch_cross(c, q, plan, a, &up))) return rc;
  if (plan.x.n_tail > 0) pd_launch_tail(c, pdhmm_fwd_kernel<false, true>, a, L, plan.x.n_tail, plan.n_blocks);
  return dev ? pd_finish_device(c, q, plan, &up, &clock, *dev) : pd_finish(c, q, plan, &up, &clock, out_host);
}

// ==== several region calls in one set of launches (pd_run_multi_locked, at the end): the host form
// (gklhip_pdhmm_compute_cross_multi: arrays and results on the host) and the device form (_cross_multi_device: the byte
// arrays and the results in HBM).  Plan, stage the inputs, stage the job tables, launch, finish: the two forms differ in
// how the inputs are staged and in the finish only ====
struct PdMultiRegion {
  PdProblem q;
  double* out;                          // host form: a host array; device form: HBM
  double* sums_out = nullptr;           // device form: HBM, or NULL
  int32_t flag = 0;                     // out: the region's input-error flag (PDHMM_INPUT_DATA_ERROR)
  int32_t routing[3] = {0, 0, 0};       // out: its haplotypes by kernel
};

// The set's totals and its input layout: one common row stride per side.
struct PdMultiShape {
  size_t NH = 0, NR = 0, NP = 0, mh = 0, mr = 0;
  explicit PdMultiShape(const std::vector<PdMultiRegion>& R) {
    for (const PdMultiRegion& r : R) {
      NH += (size_t)r.q.n_hap_items; NR += (size_t)r.q.n_read_items; NP += (size_t)r.q.n_pairs;
      mh = std::max(mh, (size_t)r.q.max_hap_len); mr = std::max(mr, (size_t)r.q.max_read_len);
    }
  }
  PdInputLayout layout() const { return PdInputLayout(NH, NR, mh, mr); }
};
// Bytes of the regions' inputs in the layout of a multi-region call.
size_t pd_multi_input_bytes(const std::vector<PdMultiRegion>& R) { return PdMultiShape(R).layout().total; }

// ---- step 1: the plan.  Every region planned exactly as pd_run_locked plans a single call, then the region table. ----
struct PdMultiPlan {
  std::vector<PdCrossPlan> plans;
  std::vector<PdRegion> regions;          // K + 1 (pd_build_regions)
  std::vector<int32_t> tab_group_start;
  size_t n_tab_haps = 0, n_hot_haps = 0, n_full_haps = 0, n_chunks = 0, n_general = 0, n_tail = 0;
  int n_tab_units = 0, n_hot_units = 0, n_full_units = 0, entry_stride = 0, n_blocks = 0;
};
// Q[k]: region k's problem as the planners may read it (the device form: its haplotype arrays are the pinned copies).
void pd_multi_plan(gklhip_pdhmm_ctx* c, const std::vector<PdProblem>& Q, const PdMultiShape& sh, PdMultiPlan* p) {
  const int K = (int)Q.size();
  p->plans.resize((size_t)K);
  std::vector<PdRegionShape> shapes((size_t)K);
  std::vector<size_t> tab_haps((size_t)K);
  std::vector<int32_t> groups((size_t)K);
  int64_t n_cross_tab = 0;   // (haplotype, chunk) jobs of the table launch
  for (int k = 0; k < K; k++) {
    const PdProblem& q = Q[(size_t)k];
    pd_plan_cross_jobs(c, q, &p->plans[(size_t)k]);
    pd_plan_cross_routing(c, q, &p->plans[(size_t)k]);
    const PdCrossPlan& pl = p->plans[(size_t)k];
    tab_haps[(size_t)k] = pl.n_tab_haps;
    p->n_tab_haps += pl.n_tab_haps; p->n_hot_haps += pl.n_clean_haps - pl.n_tab_haps; p->n_full_haps += (size_t)q.n_hap_items - pl.n_clean_haps;
    p->n_chunks += pl.chunk_steps.size(); p->n_general += pl.job_pair.size(); p->n_tail += pl.n_tail;
    n_cross_tab += (int64_t)pl.chunk_steps.size() * (int64_t)pl.n_tab_haps;
  }
  pd_size_tab_groups(tab_haps.data(), K, n_cross_tab, &p->tab_group_start, groups.data());
  for (int k = 0; k < K; k++) {
    const PdProblem& q = Q[(size_t)k];
    const PdCrossPlan& pl = p->plans[(size_t)k];
    shapes[(size_t)k] = PdRegionShape{q.n_read_items, q.n_hap_items, (int32_t)pl.chunk_steps.size(),
                                      {groups[(size_t)k], (int32_t)(pl.n_clean_haps - pl.n_tab_haps), (int32_t)((size_t)q.n_hap_items - pl.n_clean_haps)}};
  }
  p->regions.resize((size_t)K + 1);
  pd_build_regions(shapes.data(), K, p->regions.data());
  p->n_tab_units = p->regions[(size_t)K].unit_start[kPdLaunchTab];
  p->n_hot_units = p->regions[(size_t)K].unit_start[kPdLaunchHot];
  p->n_full_units = p->regions[(size_t)K].unit_start[kPdLaunchFull];
  p->entry_stride = ((int)sh.mh + 2 * kLanes + 4 + 63) / 64 * 64;
  const int n_jobs_max = std::max(std::max(p->n_tab_units, p->n_hot_units), p->n_full_units + (int)p->n_general);
  p->n_blocks = std::max(1, std::min(std::max(n_jobs_max, (int)p->n_tail), 256 * 8));
}

// ---- step 2: the inputs go to the device, every region's rows at the common strides ----
// Host form: one pinned block, one copy.
int pd_multi_stage_inputs_host(gklhip_pdhmm_ctx* c, const std::vector<PdMultiRegion>& R, const PdInputLayout& in, const PdRegion* regions) {
  int rc;
  if ((rc = c->inputs.reserve(in.total)) || (rc = c->stage_in.reserve(in.total))) return rc;
  unsigned char* h = c->stage_in.as<unsigned char>();
  for (size_t k = 0; k < R.size(); k++) {
    const PdRegion& rg = regions[k];
    for (const PdInputArray& v : pd_input_arrays(in, R[k].q)) {   // the region's rows at the common strides
      unsigned char* dst = h + v.offset + (size_t)(v.hap ? rg.hap_base : rg.read_base) * v.dst_row;
      if (v.dst_row == v.src_row) { memcpy(dst, v.src, v.n_items * v.src_row); continue; }
      for (size_t i = 0; i < v.n_items; i++) memcpy(dst + i * v.dst_row, v.src + i * v.src_row, v.src_row);
    }
  }
  HIP_TRY(hipMemcpyAsync(c->inputs.p, h, in.total, hipMemcpyHostToDevice, c->stream));
  return GKLHIP_OK;
}

// Device form.  `inputs` and `stage_in` hold the set's layout with the gather table behind it (PdGatherTable), at the same
// offsets in both.  Behind the caller's stream: ONE copy up -- the regions' host length arrays into o_hl / o_rl, the
// descriptors and the result pointers behind the layout, contiguous in both blocks --, pdhmm_gather_regions_kernel, ONE
// copy back of [o_hb, o_rb): both haplotype arrays of all regions, at the common stride, for the planners
// (pd_plan_cross_routing, has_odd_base read haplotype bytes on the host); the call's one early wait.  Q[k]: region k's
// problem with its haplotype arrays in that pinned copy.
int pd_multi_stage_inputs_device(gklhip_pdhmm_ctx* c, const std::vector<PdMultiRegion>& R, const PdInputLayout& in, hipStream_t after,
                                 std::vector<PdProblem>* Q) {
  const int K = (int)R.size();
  const hipStream_t s = c->stream;
  const PdGatherTable T(in, K);
  int rc;
  if ((rc = c->inputs.reserve(T.total)) || (rc = c->stage_in.reserve(T.total))) return rc;
  unsigned char *d = c->inputs.as<unsigned char>(), *h = c->stage_in.as<unsigned char>();
  PdGatherRegion G[kPdMaxRegions];
  PdRegionResults* results = reinterpret_cast<PdRegionResults*>(h + T.o_results);
  size_t hap_base = 0, read_base = 0;
  for (int k = 0; k < K; k++) {
    const PdProblem& q = R[(size_t)k].q;
    G[k] = PdGatherRegion{{q.hap_bases, q.hap_pdbases, q.read_bases, q.read_qual, q.read_ins_qual, q.read_del_qual, q.gcp},
                          q.n_hap_items, q.n_read_items, q.max_hap_len, q.max_read_len};
    results[k] = PdRegionResults{R[(size_t)k].out, R[(size_t)k].sums_out};
    memcpy(h + in.o_hl + hap_base * 8, q.hap_lengths, (size_t)q.n_hap_items * 8);
    memcpy(h + in.o_rl + read_base * 8, q.read_lengths, (size_t)q.n_read_items * 8);
    PdProblem& pq = (*Q)[(size_t)k];   // the planners' view: the haplotype rows at the common stride
    pq.hap_bases = reinterpret_cast<const int8_t*>(h + in.o_hb + hap_base * in.hap_row);
    pq.hap_pdbases = reinterpret_cast<const int8_t*>(h + in.o_hp + hap_base * in.hap_row);
    pq.max_hap_len = (int32_t)in.hap_row;
    hap_base += (size_t)q.n_hap_items; read_base += (size_t)q.n_read_items;
  }
  PdGatherDesc* descs = reinterpret_cast<PdGatherDesc*>(h + T.o_desc);
  pd_build_gather(G, K, in, descs);
  uint32_t most = 1;   // bytes of the largest array
  for (int i = 0; i < K * kPdGatherArrays; i++) most = std::max(most, descs[i].n_items * descs[i].src_row);
  // everything the call enqueues is ordered behind what the caller's stream already holds
  HIP_TRY(hipEventRecord(c->dev_ev, after));
  HIP_TRY(hipStreamWaitEvent(s, c->dev_ev, 0));
  HIP_TRY(hipMemcpyAsync(d + in.o_hl, h + in.o_hl, T.total - in.o_hl, hipMemcpyHostToDevice, s));
  const unsigned per_block = kPdGatherBlock * 16;
  hipLaunchKernelGGL(pdhmm_gather_regions_kernel, dim3(std::min((most + per_block - 1) / per_block, 64u), (unsigned)(K * kPdGatherArrays)),
                     dim3(kPdGatherBlock), 0, s, reinterpret_cast<const PdGatherDesc*>(d + T.o_desc), d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h + in.o_hb, d + in.o_hb, in.o_rb - in.o_hb, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GKLHIP_OK;
}

// ---- step 3: the device buffers and the job tables ----
// `sums_pin` holds the host form's sums (the kernels store them straight into it) and, in both forms, the status words
// that come back behind them; the device form's sums stay in `sums`.
int pd_multi_reserve(gklhip_pdhmm_ctx* c, const PdMultiShape& sh, const PdMultiPlan& p, bool device) {
  int rc;
  if ((rc = c->entries.reserve(sh.NH * (size_t)p.entry_stride * 4))) return rc;
  if (p.n_tab_haps && (rc = c->entries_tab.reserve(2 * sh.NH * (size_t)p.entry_stride * 4))) return rc;
  if ((rc = c->misc.reserve(kPdMiscBytes))) return rc;
  if ((rc = c->carry.reserve((size_t)p.n_blocks * 2 * (6 * (size_t)p.entry_stride + 64) * 8))) return rc;   // (carry_len = entry_stride)
  if (device && (rc = c->sums.reserve(sh.NP * 8))) return rc;
  return c->sums_pin.reserve((device ? 0 : sh.NP * 8) + 4 * ((size_t)kPdMiscRegionFlags + (size_t)kPdMaxRegions));
}

// A multi-region call's block in `jobs`: the region table (rg), the launches' haplotype lists (ho), the length of the
// full launch's list (fc) and the tables of PdJobOffsets; everything but the lane rows of the listed jobs (jl: striped
// jobs, their rows stay unused) is staged in one pinned block.
struct PdMultiJobLayout : PdJobOffsets {
  size_t rg, ho, fc, staged_total, total;
  PdMultiJobLayout(size_t K, size_t NH, const PdMultiPlan& p) {
    const size_t n_chunks = p.n_chunks, n_general = p.n_general, n_tail = p.n_tail;
    rg = 0; cl = rg + pd_up((K + 1) * sizeof(PdRegion)); cs = cl + pd_up(n_chunks * kLanes * sizeof(PlanLane));
    cr = cs + pd_up(n_chunks * 4); ho = cr + pd_up(n_chunks * 4); tg = ho + pd_up(NH * 4);
    nc = tg + pd_up(p.tab_group_start.size() * 4); cc = nc + pd_up(NH); jp = cc + pd_up(NH * 32); jn = jp + pd_up(n_general * 4);
    js = jn + pd_up(n_general * 4); jf = js + pd_up(n_general); fj = jf + pd_up(n_general); fc = fj + pd_up(n_general * 4);
    tl = fc + 256; tp = tl + pd_up(n_tail * kLanes * sizeof(PlanLane)); tn = tp + pd_up(n_tail * 4);
    ts = tn + pd_up(n_tail * 4); staged_total = ts + pd_up(n_tail);
    jl = staged_total; total = jl + pd_up(n_general * kLanes * sizeof(PlanLane));
  }
};

// The regions' plans, shifted to the concatenated indices, in one pinned block and one copy; clears the status words.
int pd_multi_stage_tables(gklhip_pdhmm_ctx* c, const PdMultiPlan& p, const PdMultiJobLayout& L) {
  const int K = (int)p.plans.size();
  const size_t n_general = p.n_general;
  int rc;
  if ((rc = c->jobs.reserve(L.total + 256)) || (rc = c->stage_jobs.reserve(L.staged_total + 256))) return rc;
  {
    unsigned char* hj = c->stage_jobs.as<unsigned char>();
    memcpy(hj + L.rg, p.regions.data(), ((size_t)K + 1) * sizeof(PdRegion));
    memcpy(hj + L.tg, p.tab_group_start.data(), p.tab_group_start.size() * 4);
    PlanLane* cl = reinterpret_cast<PlanLane*>(hj + L.cl);
    int32_t *cs = reinterpret_cast<int32_t*>(hj + L.cs), *cr = reinterpret_cast<int32_t*>(hj + L.cr);
    int32_t* ho = reinterpret_cast<int32_t*>(hj + L.ho);   // [table launch's list | predicate launch's | byte-comparing launch's]
    int32_t *ho_tab = ho, *ho_hot = ho + p.n_tab_haps, *ho_full = ho + p.n_tab_haps + p.n_hot_haps;
    uint8_t* nc = hj + L.nc;
    uint32_t* cc = reinterpret_cast<uint32_t*>(hj + L.cc);
    int32_t *jp = reinterpret_cast<int32_t*>(hj + L.jp), *fj = reinterpret_cast<int32_t*>(hj + L.fj);
    PlanLane* tl = reinterpret_cast<PlanLane*>(hj + L.tl);
    int32_t *tp = reinterpret_cast<int32_t*>(hj + L.tp), *tn = reinterpret_cast<int32_t*>(hj + L.tn);
    uint8_t* ts = hj + L.ts;
    memset(hj + L.js, 1, n_general);
    memset(hj + L.jf, 0, n_general);
    memset(hj + L.jn, 0, n_general * 4);   // (job_steps: unused by striped jobs)
    for (size_t j = 0; j < n_general; j++) fj[j] = (int32_t)j;
    *reinterpret_cast<int32_t*>(hj + L.fc) = (int32_t)n_general;
    for (int k = 0; k < K; k++) {
      const PdCrossPlan& pl = p.plans[(size_t)k];
      const PdRegion& rg = p.regions[(size_t)k];
      for (const PlanLane& l : pl.cross_lanes) *cl++ = PlanLane{l.read < 0 ? -1 : l.read + rg.read_base, l.block};
      for (const int32_t v : pl.chunk_steps) *cs++ = v;
      for (const int32_t v : pl.chunk_rep) *cr++ = v + rg.read_base;
      const size_t nh = (size_t)rg.n_haps;
      for (size_t i = 0; i < nh; i++) {
        int32_t*& dst = i < pl.n_tab_haps ? ho_tab : i < pl.n_clean_haps ? ho_hot : ho_full;
        *dst++ = pl.hap_order[i] + rg.hap_base;
      }
      memcpy(nc, pl.hap_ncls.data(), nh); nc += nh;
      memcpy(cc, pl.class_codes.data(), nh * 32); cc += nh * 8;
      for (const int32_t v : pl.job_pair) *jp++ = v + rg.pair_base;
      for (const PlanLane& l : pl.tail_lanes) *tl++ = PlanLane{l.read < 0 ? -1 : l.read + rg.pair_base, l.block};
      for (const int32_t v : pl.tail_pair) *tp++ = v + rg.pair_base;
      for (const int32_t v : pl.tail_steps) *tn++ = v;
      for (const uint8_t v : pl.tail_striped) *ts++ = v;
    }
    HIP_TRY(hipMemcpyAsync(c->jobs.p, hj, L.staged_total, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemsetAsync(c->misc.p, 0, kPdMiscBytes, c->stream));
  return GKLHIP_OK;
}

// ---- step 4: the launches.  One pdhmm_entries_kernel, at most one launch each of the table, predicate and full kernels and
// one tail launch, in their multi-region instantiations; `sums`: where they store the set's sums (a device address). ----
int pd_multi_launch(gklhip_pdhmm_ctx* c, const PdMultiShape& sh, const PdInputLayout& in, const PdMultiPlan& p, const PdMultiJobLayout& L, double* sums) {
  const hipStream_t s = c->stream;
  const unsigned char* dj = c->jobs.as<unsigned char>();
  PdArgs a = pd_common_args(c, in, L, sh.NH, (int32_t)sh.mh, (int32_t)sh.mr, p.entry_stride, p.n_tab_haps != 0);
  a.batch = (int32_t)sh.NP;
  a.cross_haps = 1;   // (cross layout; the pair index comes from the region table)
  a.sums = sums;
  a.status = c->misc.as<int32_t>() + kPdMiscRegionFlags;   // one flag per region
  a.n_chunks_cross = 1;
  a.full_count = reinterpret_cast<const int32_t*>(dj + L.fc);
  a.regions = reinterpret_cast<const PdRegion*>(dj + L.rg);
  a.n_regions = (int32_t)p.plans.size();
  const int32_t* d_ho = reinterpret_cast<const int32_t*>(dj + L.ho);

  hipLaunchKernelGGL(pdhmm_entries_kernel, dim3((unsigned)sh.NH), dim3(kLanes), 0, s, a);   // one wavefront per haplotype item
  HIP_TRY(hipEventRecord(c->ev0, s));
  const PdCrossLaunches l{{pdhmm_fwd_tab_kernel<true, true>, pdhmm_fwd_tab_kernel<false, true>},
                          {pdhmm_fwd_kernel<true, false, true, true>, pdhmm_fwd_kernel<false, false, true, true>},
                          {pdhmm_fwd_kernel<true, false, false, true>, pdhmm_fwd_kernel<false, false, false, true>},
                          true, d_ho, p.n_tab_haps, p.n_hot_haps, p.n_tab_units, p.n_hot_units, p.n_full_units,
                          0, (int)p.n_general};   // the listed jobs: the striped reads, all from the host's list
  pd_launch_cross_jobs(c, l, a, p.n_blocks);
  if (p.n_tail > 0) pd_launch_tail(c, pdhmm_fwd_kernel<false, true, false, true>, a, L, p.n_tail, p.n_blocks);   // every region's tail pairs
  HIP_TRY(hipEventRecord(c->ev1, s));
  HIP_TRY(hipGetLastError());
  return GKLHIP_OK;
}

// ---- step 5: finish.  Behind the last launch (and behind ev1: the kernel time is the forward launches'), the device form
// first: pdhmm_finalise_multi_kernel turns every good region's part of c->sums into its log10 values in HBM -- no host
// log10.  Both forms: the status words with the regions' flags come back to `status`, the stream drains, the routing and
// the flags are noted.  Host form: one finalisation over all pairs of the pinned sums.  A region with an input error
// keeps its results untouched in either. ----
int pd_multi_finish(gklhip_pdhmm_ctx* c, std::vector<PdMultiRegion>& R, const PdInputLayout& in, const PdMultiPlan& p, const PdMultiJobLayout& L,
                    bool device, int32_t* status) {
  const hipStream_t s = c->stream;
  const int K = (int)R.size();
  if (device) {
    int32_t most = 1;   // pairs of the largest region
    for (int k = 0; k < K; k++) most = std::max(most, p.regions[(size_t)k + 1].pair_base - p.regions[(size_t)k].pair_base);
    const unsigned char* d = c->inputs.as<unsigned char>();
    hipLaunchKernelGGL(pdhmm_finalise_multi_kernel, dim3((unsigned)std::min((most + kPdFinaliseBlock - 1) / kPdFinaliseBlock, 512), (unsigned)K),
                       dim3(kPdFinaliseBlock), 0, s, c->sums.as<double>(), reinterpret_cast<const PdRegion*>(c->jobs.as<unsigned char>() + L.rg),
                       c->misc.as<int32_t>() + kPdMiscRegionFlags, pd_tables().initial_condition_log10,
                       reinterpret_cast<const PdRegionResults*>(d + PdGatherTable(in, K).o_results));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(status, c->misc.p, 4 * ((size_t)kPdMiscRegionFlags + (size_t)K), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  c->last_routing[0] = (int32_t)p.n_tab_haps; c->last_routing[1] = (int32_t)p.n_hot_haps; c->last_routing[2] = (int32_t)p.n_full_haps;
  for (int k = 0; k < K; k++) {
    PdMultiRegion& r = R[(size_t)k];
    const PdCrossPlan& pl = p.plans[(size_t)k];
    r.flag = status[kPdMiscRegionFlags + k];
    r.routing[0] = (int32_t)pl.n_tab_haps; r.routing[1] = (int32_t)(pl.n_clean_haps - pl.n_tab_haps);
    r.routing[2] = (int32_t)((size_t)r.q.n_hap_items - pl.n_clean_haps);
  }
  if (device) return GKLHIP_OK;
  double* out[kPdMaxRegions];
  for (int k = 0; k < K; k++) out[k] = R[(size_t)k].out;
  return pd_finalise(c, c->sums_pin.as<double>(), p.regions.data(), K, out, status + kPdMiscRegionFlags);
}

// The regions of R (all valid, same context settings; at most kPdMaxRegions, kPdMultiMaxPairs pairs, kPdStageBytes of
// inputs) as ONE problem.  after == NULL: the host form; else the device form (R[k].q.in_hbm), ordered behind *after (a
// NULL stream: HIP's default stream).  The device form stages its inputs before it plans: the planners read the haplotype
// bytes that come back with them.  The return value is the status of the launch set (a HIP failure fails every region);
// R[k].flag != 0: region k had a negative quality (PDHMM_INPUT_DATA_ERROR), its results are not written.
int pd_run_multi_locked(gklhip_pdhmm_ctx* c, std::vector<PdMultiRegion>& R, const hipStream_t* after = nullptr) {
  HIP_TRY(hipSetDevice(c->device));
  const bool device = after != nullptr;
  const PdMultiShape sh(R);
  const PdInputLayout in = sh.layout();
  std::vector<PdProblem> Q(R.size());
  for (size_t k = 0; k < R.size(); k++) Q[k] = R[k].q;
  PdMultiPlan plan;
  int rc;
  if (device && (rc = pd_multi_stage_inputs_device(c, R, in, *after, &Q))) return rc;
  pd_multi_plan(c, Q, sh, &plan);
  if (!device && (rc = pd_multi_stage_inputs_host(c, R, in, plan.regions.data()))) return rc;
  if ((rc = pd_multi_reserve(c, sh, plan, device))) return rc;
  const PdMultiJobLayout L(R.size(), sh.NH, plan);
  if ((rc = pd_multi_stage_tables(c, plan, L))) return rc;
  // the sums: the device form's stay in HBM for its finalise kernel; the host form's go straight into pinned memory,
  // the status words behind them
  double* sums = c->sums.as<double>();
  int32_t* status = c->sums_pin.as<int32_t>();
  if (!device) {
    void* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, c->sums_pin.p, 0));
    sums = static_cast<double*>(dp);
    status = reinterpret_cast<int32_t*>(c->sums_pin.as<double>() + sh.NP);
  }
  if ((rc = pd_multi_launch(c, sh, in, plan, L, sums))) return rc;
  return pd_multi_finish(c, R, in, plan, L, device, status);
}

// process-wide, per device (gklhip_pdhmm_combine_counts): region calls computed, region calls that shared a launch set
// with another, launch sets
constexpr int kPdCountDevices = 64;
std::atomic<int64_t> g_pd_counts[kPdCountDevices][3];
void pd_count(int device, int64_t calls, int64_t shared, int64_t sets) {
  if (device < 0 || device >= kPdCountDevices) return;
  g_pd_counts[device][0] += calls; g_pd_counts[device][1] += shared; g_pd_counts[device][2] += sets;
}

constexpr const char* kPdInputErrorText = "Error while calculating pdhmm. Input arrays aren't valid.";

// Does the cross call fit a multi-region launch set on its own?
bool pd_fits_multi(const PdProblem& q) {
  return q.cross_haps && (size_t)q.n_pairs <= kPdMultiMaxPairs &&
         PdInputLayout((size_t)q.n_hap_items, (size_t)q.n_read_items, (size_t)q.max_hap_len, (size_t)q.max_read_len).total <= kPdStageBytes;
}

// ---- concurrent cross calls share launches (GKL_HIP_PDHMM_COMBINE=1; off by default) ----
// One combiner per device, like SmallCombiner of pairhmm_host_call.h: a call queues a ticket; the first thread that finds
// the combiner free leads -- it takes every queued ticket with its own fma and tail mode, up to the limits of a multi-region
// call, runs them as one on ITS context (stream, buffers) and hands every follower its status, error text, routing and the
// kernel time; the followers' doubles are written by the leader's finalisation.  Every thread holds its own context's lock
// throughout and never another's.
struct PdTicket {
  PdProblem q;
  double* out;
  int fma_mode, tail_mode;
  bool done = false;
  int rc = GKLHIP_OK;
  char err[256] = {0};
  int32_t routing[3] = {0, 0, 0};
  float ms = 0.f;
  PdTicket* next = nullptr;   // the queue: a list through the tickets, no allocation
};
struct PdCombiner {
  std::mutex mu;
  std::condition_variable cv;
  PdTicket *head = nullptr, *tail = nullptr;
  bool busy = false;   // a leader is collecting or running
};
PdCombiner g_pd_combiners[kPdCountDevices];
struct PdCombineConfig { bool on; int min; int64_t wait_us; };
const PdCombineConfig* pd_combine_config() {
  static const PdCombineConfig cfg = [] {
    PdCombineConfig r{false, 1, 0};
    const char* v = getenv("GKL_HIP_PDHMM_COMBINE");
    r.on = v && *v && strcmp(v, "0") != 0;
    if (const char* m = getenv("GKL_HIP_PDHMM_COMBINE_MIN")) r.min = std::max(1, std::min(kPdMaxRegions, atoi(m)));
    if (const char* w = getenv("GKL_HIP_PDHMM_COMBINE_WAIT_US")) r.wait_us = std::max<int64_t>(0, std::min<int64_t>(atoll(w), 60ll * 1000 * 1000));
    return r;
  }();
  return &cfg;
}

// c->mu is held.  The call's own result: status (and g_err), c->last_ms, c->last_routing.
int pd_run_combined(gklhip_pdhmm_ctx* c, const PdProblem& q, double* out_host) {
  const PdCombineConfig& cfg = *pd_combine_config();
  PdCombiner& cb = g_pd_combiners[c->device];
  PdTicket me;
  me.q = q; me.out = out_host; me.fma_mode = c->fma_mode; me.tail_mode = c->tail_mode;
  auto mine = [&](const PdTicket* t) { return t->fma_mode == me.fma_mode && t->tail_mode == me.tail_mode; };
  PdTicket* taken[kPdMaxRegions];
  int n_taken = 0;
  {
    std::unique_lock<std::mutex> lk(cb.mu);
    (cb.tail ? cb.tail->next : cb.head) = &me;
    cb.tail = &me;
    cb.cv.notify_all();   // (a leader that waits for company counts the queue)
    while (!me.done && cb.busy) cb.cv.wait(lk);
    if (!me.done) {
      cb.busy = true;   // lead
      if (cfg.min > 1 && cfg.wait_us > 0) {   // bounded: company that does not arrive in time is not waited for
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(cfg.wait_us);
        cb.cv.wait_until(lk, deadline, [&] {
          int have = 0;
          for (const PdTicket* t = cb.head; t; t = t->next) have += mine(t);
          return have >= cfg.min;
        });
      }
      // its own ticket first, then the queue in order while the set still fits
      size_t pairs = 0, nh = 0, nr = 0, mh = 0, mr = 0;
      auto fits_with = [&](const PdTicket* t) {
        const size_t p2 = pairs + (size_t)t->q.n_pairs, nh2 = nh + (size_t)t->q.n_hap_items, nr2 = nr + (size_t)t->q.n_read_items,
                     mh2 = std::max(mh, (size_t)t->q.max_hap_len), mr2 = std::max(mr, (size_t)t->q.max_read_len);
        return p2 <= kPdMultiMaxPairs && PdInputLayout(nh2, nr2, mh2, mr2).total <= kPdStageBytes;
      };
      auto take = [&](PdTicket* t) {
        pairs += (size_t)t->q.n_pairs; nh += (size_t)t->q.n_hap_items; nr += (size_t)t->q.n_read_items;
        mh = std::max(mh, (size_t)t->q.max_hap_len); mr = std::max(mr, (size_t)t->q.max_read_len);
        taken[n_taken++] = t;
      };
      take(&me);
      PdTicket *prev = nullptr, *t = cb.head;
      while (t) {
        PdTicket* nx = t->next;
        const bool go = t == &me || (n_taken < kPdMaxRegions && mine(t) && fits_with(t));
        if (go) {
          if (t != &me) take(t);
          (prev ? prev->next : cb.head) = nx;
          if (cb.tail == t) cb.tail = prev;
          t->next = nullptr;
        } else {
          prev = t;
        }
        t = nx;
      }
    }
  }
  if (n_taken > 0) {
    // the launch set, on this context; whatever happens every taken ticket gets an answer
    int rc;
    std::string err;
    try {
      std::vector<PdMultiRegion> R((size_t)n_taken);
      for (int k = 0; k < n_taken; k++) { R[(size_t)k].q = taken[k]->q; R[(size_t)k].out = taken[k]->out; }
      rc = pd_fenced(c, [&] { return pd_run_multi_locked(c, R); });
      if (rc != GKLHIP_OK) err = g_err;
      for (int k = 0; k < n_taken; k++) {
        PdTicket* t = taken[k];
        t->rc = rc != GKLHIP_OK ? rc : (R[(size_t)k].flag != 0 ? GKLHIP_ERR_INVALID_ARG : GKLHIP_OK);
        snprintf(t->err, sizeof t->err, "%s", rc != GKLHIP_OK ? err.c_str() : (R[(size_t)k].flag != 0 ? kPdInputErrorText : ""));
        for (int i = 0; i < 3; i++) t->routing[i] = R[(size_t)k].routing[i];
        t->ms = c->last_ms;
      }
    } catch (...) {
      for (int k = 0; k < n_taken; k++) { taken[k]->rc = GKLHIP_ERR_OOM; snprintf(taken[k]->err, sizeof taken[k]->err, "host memory allocation failed"); }
    }
    pd_count(c->device, n_taken, n_taken > 1 ? n_taken : 0, 1);
    std::lock_guard<std::mutex> lk(cb.mu);
    for (int k = 0; k < n_taken; k++) taken[k]->done = true;   // (a follower's ticket lives on its stack: not touched after this)
    cb.busy = false;
    cb.cv.notify_all();
  }
  c->last_ms = me.ms;
  for (int i = 0; i < 3; i++) c->last_routing[i] = me.routing[i];
  return me.rc == GKLHIP_OK ? GKLHIP_OK : fail(me.rc, "%s", me.err);
}

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
  if (!b) return fail(GKLHIP_ERR_INVALID_ARG, "batch is NULL");
  // IntelPDHMM.java:163-173
  if (b->batch <= 0) return fail(GKLHIP_ERR_INVALID_ARG, "batchSize must be greater than 0");
  PdProblem q{b->batch, b->batch, b->batch, 0, b->max_hap_len, b->max_read_len, b->hap_bases, b->hap_pdbases,
              b->read_bases, b->read_qual, b->read_ins_qual, b->read_del_qual, b->gcp, b->hap_lengths, b->read_lengths, 0};
  const int rc = pd_validate(q, out_host);
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
  if (!b) return fail(GKLHIP_ERR_INVALID_ARG, "batch is NULL");
  if (b->batch <= 0) return fail(GKLHIP_ERR_INVALID_ARG, "batchSize must be greater than 0");
  PdProblem q{b->batch, b->batch, b->batch, 0, b->max_hap_len, b->max_read_len, b->hap_bases, b->hap_pdbases,
              b->read_bases, b->read_qual, b->read_ins_qual, b->read_del_qual, b->gcp, b->hap_lengths, b->read_lengths, 0};
  const int rc = pd_validate(q, out_dev);
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
    size_t pairs = 0;
    for (const PdMultiRegion& r : R) pairs += (size_t)r.q.n_pairs;
    const bool fits = !c->remote && R.size() <= (size_t)kPdMaxRegions && pairs <= kPdMultiMaxPairs && pd_multi_input_bytes(R) <= kPdStageBytes;
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
