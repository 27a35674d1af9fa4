// Process-wide switches and DevCtx: one device's engine state (error plumbing and the grow-and-trim device / pinned
// buffers: hip_host_common.h, shared with the PDHMM and Smith-Waterman libraries).
// Part of the ONE translation unit gkl_amd/csrc/pairhmm_api.hip, which includes it in the order it needs; not a stand-alone header.
#pragma once

using namespace gklhip;

// Development / A-B switches, read from the environment ONCE -- when the library is loaded -- and never on a call path
// (getenv is not safe against a concurrent setenv in the host JVM).  Context-level settings (GKL_HIP_DEVICES, GKL_HIP_GATHER,
// GKL_HIP_HOST_SHARDS, GKLHIP_ASM_GENERAL, ...) are read by the init functions; the test hooks GKL_HIP_RCCL_FAIL /
// GKLHIP_SELFTEST_FAIL where a context or a communicator is made.
namespace {
struct EnvSwitches {
  static bool on_unless_zero(const char* name) { const char* v = getenv(name); return !v || atoi(v) != 0; }
  static int integer(const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; }
  const bool wide_long = on_unless_zero("GKLHIP_WIDE_LONG");        // long reads: workgroups of several wavefronts (0: one-wavefront stripes)
  const bool super_long = on_unless_zero("GKLHIP_SUPER_LONG");      // reads beyond a workgroup: super-stripes
  const bool fused_pairs = on_unless_zero("GKLHIP_FUSED_PAIRS");    // small calls: fp32 + policy + fp64 of a pair in one wavefront
  const int64_t fused_max = [] { const char* v = getenv("GKLHIP_FUSED_MAX_PAIRS"); return v ? atoll(v) : -1LL; }();
  const bool xcd_aware = on_unless_zero("GKLHIP_XCD_AWARE");
  const bool timing = getenv("GKLHIP_TIMING") != nullptr;
  const int combine_load = integer("GKL_HIP_COMBINE_LOAD");
  const int target_cols = integer("GKLHIP_TARGET_COLS");
  const int fb_wanted_jobs = integer("GKLHIP_FB_WANTED_JOBS");
  const int plan_blocks = integer("GKLHIP_PLAN_BLOCKS");
  const int finalize_threads = integer("GKL_HIP_FINALIZE_THREADS");
  const int finalize_min = integer("GKL_HIP_FINALIZE_MIN");   // one-pass host log10: pairs from which it is spread over the workers (0: the built-in 8192)
  const bool combine = [] { const char* v = getenv("GKL_HIP_COMBINE"); return !(v && v[0] == '0'); }();
  // concurrent callers' mid-size calls (2049 - 65 536 pairs) enter the small-call combiner, for contexts made from here
  // on: off unless set to a non-zero number (gklhip_set_mid_combine changes it per context)
  const bool combine_mid = integer("GKL_HIP_COMBINE_MID") != 0;
  const bool quiet = getenv("GKL_HIP_QUIET") != nullptr;
  const bool one_device_engine = integer("GKL_HIP_DEVICE_ENGINES") == 1;
  // the longest read of a region that takes the small-call path, for contexts made from here on: 511 when set to exactly
  // that, 383 otherwise (gklhip_set_small_read_limit changes it per context)
  const int small_read_limit = integer("GKL_HIP_SMALL_READ_LIMIT") == 511 ? 511 : 383;
};
const EnvSwitches g_env;
}  // namespace

#include "hip_host_common.h"   // g_err / fail / guarded / HIP_TRY, trim_due, DevBuf, PinBuf

// ------------------------------------------------------------------ context
// One device's engine: streams, tables, grow-only scratch.  The public gklhip_ctx owns one of these per
// device of its list (one for the usual single-device context).
struct DevCtx {
  gklhip_config cfg;
  int device = 0;
  bool multi_device = false;   // one of several engines of a multi-device context (set by gklhip_init_devices): its shards of a double-precision call keep the general pass
  int n_cus = 256;
  int n_xcds = 8;   // hipDeviceAttributeNumberOfXccs: workgroups go to the XCDs round-robin by index
  // development / cross-check switches, read from the environment ONCE per context (dev_init), never on a call path
  // (getenv is not safe against a concurrent setenv in the host JVM): GKLHIP_ASM_GENERAL=0 (round-3 arrangement: C++
  // general steps), GKLHIP_SPECULATE_FP64=1 (fp64 beside fp32 for a lone tiny call)
  int asm_general = 1;
  int speculate_fp64 = 0;
  int small_read_limit = g_env.small_read_limit;   // 383 or 511 (gklhip_set_small_read_limit; a staging lane follows its parent)
  int mid_combine = g_env.combine_mid ? 1 : 0;     // gklhip_set_mid_combine (mid_call_combines; twins and staging lanes follow their parent)
  int lds_oob_zero = 1;   // dev_init's self-test: a DS read beyond the allocation returns 0 here (the fp32 programs' separator priors)
  hipStream_t stream = nullptr;
  // tables
  DevBuf tab32, tab64;
  DevTables<float> dt32;
  DevTables<double> dt64;
  // per-call plan uploads (pinned staging -> device)
  // Two slots alternate from call to call: the plan of call k+1 is staged and uploaded (own stream) while the
  // kernels of call k still read theirs -- back-to-back batches then never wait for the plan block.
  PinBuf stage_slot[2];
  DevBuf plan_dev_slot[2];
  hipEvent_t stage_free_slot[2] = {nullptr, nullptr};   // the slot's upload has left the staging buffer
  hipEvent_t plan_unused_slot[2] = {nullptr, nullptr};  // the last call that used the slot's device copy has finished
  hipStream_t upload_stream = nullptr;
  bool upload_eager = false;          // opened with the context (the first one of the process: see dev_init) -- trim_streams keeps it
  hipStream_t pad_stream = nullptr;   // never used: keeps the context's stream count at four once copy_stream exists (aux_streams)
  int plan_slot = 0;
  // per-call device scratch
  DevBuf raw32, raw64, used64, counters, stream_buf, out_dev;
  DevBuf lanes_main;  // the main pass's lane map, expanded by prep_kernel from the plan's compact read packing
  DevBuf read_fail, lanes2, jobs, jobs_long, fail_order, fail_hist, hap_flags;
  // host-API device copies of the batch, packed results (device + pinned), finalisation workers
  DevBuf batch_dev;
  PinBuf res_pin;
  WorkerPool workers;
  hipStream_t copy_stream = nullptr;  // early D2H of the fp32 results / device log10 of the kept pairs while the fp64 pass runs
  hipEvent_t policy_done = nullptr, early_copy_done = nullptr;
  // scratch is per context and ordered by the stream of the call that uses it: a call on a different stream than
  // the previous one first waits for that one's end
  hipEvent_t call_done = nullptr;
  bool have_call_done = false;
  // events: kEventRing sets of 6 (call start, main begin/end, fallback begin/end, call end); record_events == 1 uses
  // set 0 and synchronises every call, record_events == 2 rotates through the ring and never synchronises
  // (gklhip_get_step_times reads a set later)
  static constexpr int kEventRing = 64;
  hipEvent_t ev_ring[kEventRing][6] = {};
  hipEvent_t* ev = ev_ring[0];
  int64_t calls = 0;
  bool ring_double[kEventRing] = {};
  // last call
  gklhip_stats stats;
  int64_t last_pairs = 0;
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  Plan plan;
  std::vector<PlanLane> long_lanes;
  std::vector<FwdJob> long_jobs;
  DevBuf carry;
  // gklhip_compute_multi_device (an engine, not its lanes): the event that orders a set behind the caller's stream, and the
  // fallback counts of a set's regions as finalize_words_multi_kernel leaves them (kMultiMax words of pinned memory)
  hipEvent_t multi_in = nullptr;
  PinBuf multi_fallbacks;
};
