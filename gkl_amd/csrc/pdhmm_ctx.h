// The PDHMM context and what every launch path of pdhmm_api.hip shares: the host tables, the fence around a launch
// path, the words of `misc`.  Part of the one HIP translation unit pdhmm_api.hip (included there, not compiled alone).
#pragma once
#include "pdhmm_call_plan.h"      // PdPlanSettings, PdPlanScratch, kPdMaxSlices

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
  static constexpr int kMaxSlices = kPdMaxSlices;
  hipStream_t up_stream = nullptr;
  gklhip::WorkerPool workers;           // host log10 of the sums: three helpers from 4096 pairs on
  PdPlanScratch plan_scratch;           // the planner's stamp table and packing scratch (pdhmm_call_plan.h)
  hipEvent_t up_ev[kMaxSlices] = {}, sl_ev0[kMaxSlices] = {}, sl_ev1[kMaxSlices] = {};
  int pipeline = 1;                     // GKL_HIP_PDHMM_PIPELINE=0: one slice whatever the size
  std::mutex mu;
  DevBuf tables, inputs, entries, entries_tab, sums, misc, carry, jobs, tabx;
  PinBuf stage_in, stage_jobs, sums_pin;   // small calls: ONE copy per device buffer instead of one per array (9 + 17 of them)
  float last_ms = 0.f;
  int32_t last_routing[3] = {0, 0, 0};  // last cross call: haplotype items by kernel (table / predicate / byte-comparing); last paired call: packed jobs by kernel
  int use_table = 1;                    // GKL_HIP_PDHMM_TABLE=0: never route to the table kernel
  int fma_mode = 1;  // 1 = arithmetic of GKL's AVX-512 object (default), 0 = of its AVX2 object
  int tail_mode = 1; // 1 (default) = the last `batch mod SIMD width` pairs of every reference batch take the scalar engine's arithmetic, like GKL; 0 = vector arithmetic everywhere
  // what the planner is handed of the above (c->mu is held)
  PdPlanSettings plan_settings() const { return PdPlanSettings{fma_mode, tail_mode, use_table, pipeline, GKL_PD_ASM == 2}; }
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

// misc: 64 int32 of flags and job counters (the first 256 bytes, cleared by every call), then the per-region input-error
// flags of a multi-region call
constexpr size_t kPdMiscBytes = 256 + 4 * (size_t)kPdMaxRegions;
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

// PDHMM_INPUT_DATA_ERROR (pdhmm-serial.cc:183-199) as the C ABI reports it: a negative ins / del / gcp quality
constexpr const char* kPdInputErrorText = "Error while calculating pdhmm. Input arrays aren't valid.";
}  // namespace
