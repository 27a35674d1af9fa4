// One pass of the hot path on one device: table upload, plan block layout, kernel launch helpers, and the pass in steps -- plan_call (host
// only), stage_call (the block and its way to the device), the kernels' argument builders, one launch function per shape of call (prep ->
// fp32 forward -> policy + device-side planning -> fp64 recomputation -> finalisation), describe_small_call (the deferred exit) -- which
// run_device and the host-buffer calls (pairhmm_host_call.h) compose.
// Part of the ONE translation unit gkl_amd/csrc/pairhmm_api.hip, which includes it in the order it needs; not a stand-alone header.
#pragma once

namespace {

// The context's third stream, made on first use together with a padding stream (see dev_init: how many streams a process
// holds decides how the device's scheduler treats it next to other processes; two and four are good numbers, three is not).
int aux_streams(DevCtx* c) {
  if (!c->upload_stream) HIP_TRY(hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking));
  if (!c->copy_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->pad_stream) HIP_TRY(hipStreamCreateWithFlags(&c->pad_stream, hipStreamNonBlocking));
  }
  return GKLHIP_OK;
}

template <typename T>
int upload_tables(DevCtx* c, const HostTables<T>& h, DevBuf* buf, DevTables<T>* dt) {
  const size_t n = (size_t)kQuals * 2 + kMmEntries;
  int st = buf->reserve(n * sizeof(T));
  if (st) return st;
  T* base = buf->as<T>();
  // (on the context's own stream -- the null stream would be one more hardware queue per process -- and pulled by a kernel
  //  from a pinned block instead of copied: no copy-engine queue either)
  {
    T* pin = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pin), n * sizeof(T), hipHostMallocDefault));
    memcpy(pin, h.ph2pr.data(), kQuals * sizeof(T));
    memcpy(pin + kQuals, h.div3.data(), kQuals * sizeof(T));
    memcpy(pin + 2 * kQuals, h.mm.data(), kMmEntries * sizeof(T));
    void* pin_dev = nullptr;
    hipError_t e = hipHostGetDevicePointer(&pin_dev, pin, 0);
    if (e == hipSuccess) {
      static_assert(sizeof(T) % 4 == 0, "whole words");
      hipLaunchKernelGGL(pull_words_kernel, dim3(64), dim3(256), 0, c->stream, static_cast<const uint32_t*>(pin_dev),
                         reinterpret_cast<uint32_t*>(base), (int)(n * sizeof(T) / 4));
      e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    (void)hipHostFree(pin);
    HIP_TRY(e);
  }
  dt->ph2pr = base;
  dt->div3 = base + kQuals;
  dt->mm = base + 2 * kQuals;
  return GKLHIP_OK;
}

size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Layout of the per-call plan block (identical in pinned staging and on the device).  A small host-buffer call
// appends its six input arrays (`batch`: 5 read arrays at `batch_stride`, then the haplotype bases), so that plan
// and inputs travel in ONE copy.
struct PlanLayout {
  size_t place_chunk, place_lane, chunk_used, groups, hap_len, hap_pos, hap_pos_flat, hap_orig, hap_sidx, hap_group, hap_src, y0_32, y0_64, read_off, long_lanes, long_jobs, long_count,
      batch, batch_stride, stream, stream_flat, has_n, desc, total;
};
// Where a call's six byte arrays live -- what decides the block's layout and whether the small-call path is offered.
enum class Arrays {
  kHostInline,   // HOST arrays that travel inside the plan block (a host call no larger than kSmallBatchBytes)
  kDevice,       // on the device: a device-resident call, or a host call whose arrays were copied there
  kRegionInHbm,  // in HBM, no larger than kSmallBatchBytes, as a region of gklhip_compute_multi_device
};
PlanLayout layout_for(const Plan& p, int n_reads, int n_haps, size_t n_long_lanes, size_t n_long_jobs, size_t read_bytes, size_t hap_bytes, Arrays where) {
  PlanLayout l;
  const size_t inline_read_bytes = where == Arrays::kHostInline ? read_bytes : 0, inline_hap_bytes = where == Arrays::kHostInline ? hap_bytes : 0;
  size_t o = 0;
  l.place_chunk = o; o = align_up(o + (size_t)n_reads * 4);
  l.place_lane = o; o = align_up(o + (size_t)n_reads);
  l.chunk_used = o; o = align_up(o + (size_t)p.n_chunks);
  l.groups = o; o = align_up(o + p.groups.size() * sizeof(PlanGroup));
  l.hap_len = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_pos = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_pos_flat = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_orig = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_sidx = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_group = o; o = align_up(o + (size_t)n_haps * 4);
  l.hap_src = o; o = align_up(o + (size_t)n_haps * 4);
  l.y0_32 = o; o = align_up(o + (size_t)n_haps * 4);
  l.y0_64 = o; o = align_up(o + (size_t)n_haps * 8);
  l.read_off = o; o = align_up(o + (size_t)(n_reads + 1) * 8);
  l.long_lanes = o; o = align_up(o + n_long_lanes * sizeof(PlanLane));
  l.long_jobs = o; o = align_up(o + n_long_jobs * sizeof(FwdJob));
  l.long_count = o; o = align_up(o + 16);
  l.batch = o;
  l.batch_stride = align_up(inline_read_bytes);
  if (inline_read_bytes) o = o + 5 * l.batch_stride + align_up(inline_hap_bytes);
  // ... and, when the host holds the haplotype bases anyway, the two haplotype streams and the 'N' flags, built on
  // the host: the first kernel then only pulls the block (its wavefronts would otherwise chase three dependent reads
  // of pinned host memory per haplotype before the first forward kernel can start)
  l.stream = o; if (inline_read_bytes) o = align_up(o + (size_t)p.n_stream * 4);
  l.stream_flat = o; if (inline_read_bytes) o = align_up(o + (size_t)p.n_stream_flat * 4);
  l.has_n = o; if (inline_read_bytes) o = align_up(o + (size_t)n_haps);
  // ... and the call's descriptor for the combined launches of several small calls (SmallCombiner); a region of the
  // device-resident multi call (kRegionInHbm) has one too, behind a block without inputs and host-built streams
  l.desc = o; if (inline_read_bytes || where == Arrays::kRegionInHbm) o = align_up(o + sizeof(SmallCall));
  l.total = o;
  return l;
}

int validate(const gklhip_batch* b) {
  if (!b) return fail(GKLHIP_ERR_INVALID_ARG, "batch is NULL");
  if (b->n_reads < 0 || b->n_haps < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative batch size");
  if (b->n_reads == 0 || b->n_haps == 0) return GKLHIP_OK;
  if (!b->read_off || !b->hap_off) return fail(GKLHIP_ERR_INVALID_ARG, "offset arrays are NULL");
  if (!b->read_bases || !b->read_quals || !b->ins_gop || !b->del_gop || !b->gcp || !b->hap_bases)
    return fail(GKLHIP_ERR_INVALID_ARG, "a batch byte array is NULL");
  if (b->read_off[0] != 0 || b->hap_off[0] != 0)
    return fail(GKLHIP_ERR_INVALID_ARG, "offset arrays must start at 0");
  // The reference does not guard empty reads/haplotypes (division by zero / negative index,
  // SURVEY appendix A.10); this boundary rejects them.
  for (int r = 0; r < b->n_reads; r++)
    if (b->read_off[r + 1] <= b->read_off[r])
      return fail(GKLHIP_ERR_INVALID_ARG, "read %d is empty or offsets are not increasing", r);
  for (int h = 0; h < b->n_haps; h++)
    if (b->hap_off[h + 1] <= b->hap_off[h])
      return fail(GKLHIP_ERR_INVALID_ARG, "haplotype %d is empty or offsets are not increasing", h);
  if ((int64_t)b->n_reads * b->n_haps >= (int64_t)1 << 31)
    return fail(GKLHIP_ERR_UNSUPPORTED, "more than 2^31 pairs in one call");
  if (b->hap_off[b->n_haps] + b->n_haps + 4096 >= (int64_t)1 << 31)
    return fail(GKLHIP_ERR_UNSUPPORTED, "haplotype bases exceed 2^31");
  return GKLHIP_OK;
}

template <typename T, int RPL>
void launch_stream(const FwdArgs<T>& a, int fma, int n_blocks, hipStream_t s) {
  if (fma) hipLaunchKernelGGL((pairhmm_fwd_stream_kernel<T, RPL, true>), dim3(n_blocks), dim3(64), 0, s, a);
  else     hipLaunchKernelGGL((pairhmm_fwd_stream_kernel<T, RPL, false>), dim3(n_blocks), dim3(64), 0, s, a);
}
template <typename T, int RPL>
void launch_jobs(const FwdArgs<T>& a, int fma, int n_blocks, hipStream_t s) {
  if (fma) hipLaunchKernelGGL((pairhmm_fwd_jobs_kernel<T, RPL, true>), dim3(n_blocks), dim3(64), 0, s, a);
  else     hipLaunchKernelGGL((pairhmm_fwd_jobs_kernel<T, RPL, false>), dim3(n_blocks), dim3(64), 0, s, a);
}

template <typename T, int RPL>
void launch_long(const FwdArgs<T>& a, int fma, int n_blocks, T* carry, int carry_len, hipStream_t s) {
  if (fma) hipLaunchKernelGGL((pairhmm_fwd_long_kernel<T, RPL, true>), dim3(n_blocks), dim3(64), 0, s, a, carry, carry_len);
  else     hipLaunchKernelGGL((pairhmm_fwd_long_kernel<T, RPL, false>), dim3(n_blocks), dim3(64), 0, s, a, carry, carry_len);
}

// long reads: workgroups of kWideWaves wavefronts per (read, haplotype run) job (pairhmm_fwd_wide_kernel: the asm programs'
// arithmetic only); the unfused arithmetic keeps the one-wavefront striped kernel
// compute wavefronts of a super-stripe workgroup (+ 1 helper): 7 + 1 in both precisions = 512 threads, two wavefronts per
// SIMD (amdgpu_waves_per_eu(4): 128 VGPRs) -- the first version's 5 + 1 put four compute wavefronts on SIMD 0 and two on SIMDs
// 2, 3, and a pipeline of wavefronts advances at the speed of its slowest (docs/NOTES.md 44).  LDS: ~78 KB per fp32
// workgroup (two fit a CU's 160 KB), fp64 with its 16 KB tables one per CU; super_blocks_max = the workgroups that can be
// resident at once (256 CUs x 2 / x 1): the carry rows (two per workgroup) are sized for that many.
template <typename T> constexpr int super_waves() { return 7; }
template <typename T> constexpr int super_blocks_max() { return sizeof(T) == 8 ? 256 : 512; }
// carry rows of the super-stripe kernel: two per workgroup, one 32-byte slot per step of the deepest array's longest stream
inline int64_t super_steps(int carry_len, int max_read_len, int rpl) { return (int64_t)carry_len + 64 * (int64_t)((blocks_for(max_read_len, rpl) + kLanes - 1) / kLanes); }
template <typename T, int RPL, int RPL_STRIPED>
void launch_long_jobs(const FwdArgs<T>& a, int fma, int n_blocks, int max_read_len, T* carry, int carry_len, hipStream_t s,
                      unsigned char* xcarry = nullptr, int64_t xsteps = 0, int32_t* next2 = nullptr) {
  const bool wide_env = g_env.wide_long, super_env = g_env.super_long;
  if (!wide_env) { launch_long<T, RPL_STRIPED>(a, fma, n_blocks, carry, carry_len, s); return; }
  // a read that needs more wavefronts than a wide workgroup holds: super-stripes of super_waves<T>() wavefronts, the carry row through HBM
  if (super_env && xcarry && next2 && (blocks_for(max_read_len, RPL) + kLanes - 1) / kLanes > kWideWavesMax) {
    static_assert(RPL == kRplSuper, "the super-stripe kernel's array depth");
    FwdArgs<T> sa = a;
    sa.super_steps = xsteps;
    if (fma) hipLaunchKernelGGL((pairhmm_fwd_super_kernel<T, RPL, super_waves<T>(), true>), dim3(std::min(n_blocks, super_blocks_max<T>())), dim3(64 * (super_waves<T>() + 1)), 0, s, sa, xcarry);
    else     hipLaunchKernelGGL((pairhmm_fwd_super_kernel<T, RPL, super_waves<T>(), false>), dim3(std::min(n_blocks, super_blocks_max<T>())), dim3(64 * (super_waves<T>() + 1)), 0, s, sa, xcarry);
    // ... and the jobs it leaves (a haplotype no longer than a wavefront is deep, fp64: an N haplotype): one-wavefront stripes
    sa.long_filter = 2;
    sa.job_next = next2;
    launch_long<T, RPL_STRIPED>(sa, fma, n_blocks, carry, carry_len, s);
    return;
  }
  // wavefronts per workgroup: what the call's longest read needs, at most kWideWavesMax (longer reads are striped in-kernel)
  const int waves = std::max(2, std::min(kWideWavesMax, (blocks_for(max_read_len, RPL) + kLanes - 1) / kLanes));
  if (fma) {
    if (waves == 2)      hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, true, 2>), dim3(n_blocks), dim3(128), 0, s, a, carry, carry_len);
    else if (waves == 3) hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, true, 3>), dim3(n_blocks), dim3(192), 0, s, a, carry, carry_len);
    else                 hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, true, 4>), dim3(n_blocks), dim3(256), 0, s, a, carry, carry_len);
  } else {   // the unfused arithmetic (fma_mode 0): the same kernels over the "...n" programs
    if (waves == 2)      hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, false, 2>), dim3(n_blocks), dim3(128), 0, s, a, carry, carry_len);
    else if (waves == 3) hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, false, 3>), dim3(n_blocks), dim3(192), 0, s, a, carry, carry_len);
    else                 hipLaunchKernelGGL((pairhmm_fwd_wide_kernel<T, RPL, false, 4>), dim3(n_blocks), dim3(256), 0, s, a, carry, carry_len);
  }
}

// A small host-buffer call, planned and staged but not launched (describe_small_call): SmallCombiner decides how it
// reaches the device (on its own, or in one set of launches with the calls of other threads).
struct SmallLaunch {
  SmallCall call;                          // the descriptor
  const SmallCall* desc_pinned = nullptr;  // ... as the device sees it in the pinned staging block (the prep kernel reads this one)
  const SmallCall* desc_dev = nullptr;     // ... in the device copy of the plan block (which the prep kernel pulls)
};

// Rows per lane.  fp32 main pass: 8 (4 or 2 for small batches).  fp64: 10 in the streaming and job-list kernels, 6 (kRplF64) in the
// one-pair-per-wavefront and striped long-read kernels.  A read of length R needs R+1 rows; reads that exceed 64*RPL rows go to the
// striped long-read kernel.
#ifndef GKL_RPL_F64
#define GKL_RPL_F64 6
#endif
constexpr int kRplF64 = GKL_RPL_F64;
// The streaming and job-list fp64 kernels run two wavefronts per SIMD (256 VGPRs, 8 x 20 KB of LDS): 10 rows per lane
// (20 spilled registers, none in the unrolled loop) -- fewer hand-offs per cell and shorter general-step windows than 6
// or 8: the packed fp64 pass of the precision policy takes 3.23 (6 rows) / 2.91 (8) / 2.77 ms (10), the all-fp64 mode
// 18.2 / 17.8 / 17.1 ms (A/B on one box; 12 rows would leave LDS for three wavefronts per CU pair only).  kRplF64 (6)
// remains the row count of the one-pair-per-wavefront kernel (three wavefronts per SIMD) and of the striped long-read kernel.
#ifndef GKL_RPL_F64_JOBS
#define GKL_RPL_F64_JOBS 10
#endif
constexpr int kRplF64Jobs = GKL_RPL_F64_JOBS;
// The wide long-read kernel (several wavefronts of a workgroup per read) runs fp64 at 8 rows per lane: 16 KB of prior planes
// per wavefront instead of 20 -- four / three / two workgroups per CU at two / three / four wavefronts each instead of three / two / one.
constexpr int kRplF64Wide = 8;
constexpr size_t kSmallBatchBytes = 1 << 20;  // host-buffer calls up to this size send their inputs inside the plan block
constexpr int64_t kDirectPairs = 65536;        // calls up to this many pairs: policy + fp64 recomputation of one pair per wavefront (host calls of 24k / 38k / 50k pairs: 0.64 / 0.74 / 0.96 ms against 0.81 / 0.82 / 1.09 through the planned fp64 pass; equal at 80k)
constexpr int64_t kTwoStepFrom = 2048;         // ... from this many pairs in two launches: policy + list of the failing pairs, then their recomputation (10k / 16k / 32k pairs: 0.37 / 0.45-0.48 / 0.72-0.84 ms against 0.43 / 0.49-0.54 / 0.76-0.97 in one)
constexpr int64_t kSmallDoublePairs = kTwoStepFrom;   // a small call of a double-precision context (kSmallDouble: every pair through pairhmm_pair_f64_kernel): at most this many pairs
constexpr int kPlanBlocks = 64;                // 1024-thread blocks of the packing / run-detection launches of the fp64 plan
constexpr int kFallbackWantedJobs = 12288;     // the packed fp64 pass is cut into about this many jobs (4 per wavefront slot)
constexpr int64_t kHostShardPairs = 400000;    // single-device host-buffer calls from this many pairs run as two half-batches (see gklhip_ctx::host_dev)
constexpr int64_t kOnePassPairs = 65536;      // host-buffer calls up to this many pairs finalise in one pass after the last kernel
constexpr int kTargetCols = 2048;  // columns of a full-size haplotype group (sweep 1024..4096: flat within 2 %, optimum 1800..2600)
#ifndef GKL_RPL_F32
#define GKL_RPL_F32 8
#endif
constexpr int kRplF32 = GKL_RPL_F32;
std::atomic<int> g_host_calls_in_flight{0};  // host-buffer calls inside the library right now, process-wide
// fp32 main pass: which kernel.  rows_per_lane of the config: 0 = choose, 8 / 4 / 2 = that many rows per lane.
// Choosing: a small batch (one GATK active region) gives the 8-row kernel fewer jobs than the chip has wavefront
// slots worth filling (< 2 per SIMD), and a lone wavefront issues one instruction per ~6 cycles; fewer rows per
// lane mean more chunks and a shorter step (2 rows: reads of up to 127 bases).  `load`: small host calls in flight in
// this process -- they share the chip (and leave in combined launches, SmallCombiner), so their jobs count together
// and the wider, cheaper-per-cell kernels pay from fewer jobs per call.
int pick_f32_rpl(int forced, int n_reads, int n_haps, const int64_t* read_off, const int64_t* hap_off, int load = 1) {
  int max_len = 0;
  for (int r = 0; r < n_reads; r++) max_len = std::max(max_len, (int)(read_off[r + 1] - read_off[r]));
  if (forced == 2 && max_len <= 2 * kLanes - 1) return 2;
  if (forced == 4 || forced == -4 || forced == 2) return 4;
  if (forced == 8) return kRplF32;
  const int64_t total_cols = hap_off[n_haps] + n_haps;
  auto jobs_at = [&](int rpl) {
    int64_t blocks = 0;
    for (int r = 0; r < n_reads; r++) {
      const int nb = blocks_for((int)(read_off[r + 1] - read_off[r]), rpl);
      if (nb <= kLanes) blocks += nb;
    }
    const int64_t chunks = std::max<int64_t>(1, (blocks + kLanes - 1) / kLanes);
    const int64_t groups = std::min<int64_t>(n_haps, std::max<int64_t>((total_cols + kTargetCols - 1) / kTargetCols,
                                                                        (4096 + chunks - 1) / chunks));
    return chunks * groups;
  };
  // (a read of 256 bases or more does not fit 64 lanes x 4 rows: it would take the striped long-read kernel)
  if (jobs_at(kRplF32) * load >= 2048 || max_len > 4 * kLanes - 1) return kRplF32;
  if (jobs_at(4) * load >= 1024 || max_len > 2 * kLanes - 1) return 4;
  return 2;
}

void launch_main_f32(const FwdArgs<float>& a, int rpl_main, int fma, int n_blocks, hipStream_t s) {
  if (rpl_main == 2)      launch_stream<float, 2>(a, fma, n_blocks, s);
  else if (rpl_main == 4) launch_stream<float, 4>(a, fma, n_blocks, s);
  else                    launch_stream<float, kRplF32>(a, fma, n_blocks, s);
}

// ---- the one-pair-per-wavefront kernels: a call of `rows` (by its longest read: pair_rows_for), or a set of calls whose
// widest has them, launches the form pairhmm_pair_forms.h names.  Forms...: the instantiations the family has. ----
static_assert(kRplF64 == kPairTiers[2] && kRplPair8 == kPairTiers[3], "the third and fourth tier by the names the kernels' comments use");
template <int... Forms, typename F>
int launch_pair_form(PairFamily family, bool is_set, int rows, int fma, F launch) {
  if (dispatch_pair_form<Forms...>(pair_form(family, is_set, rows), fma != 0, launch)) return GKLHIP_OK;
  return fail(GKLHIP_ERR_UNSUPPORTED, "no per-pair kernel of family %d for %d rows per lane", (int)family, rows);
}
// the policy on the fp32 sums + the fp64 recomputation of the pairs that fail it, one launch
int launch_pair_policy(const FwdArgs<double>& d, const PairPolicyArgs& q, int rows, int fma, int64_t n_pairs, hipStream_t s) {
  const dim3 grid((unsigned)n_pairs), block(64);
  return launch_pair_form<2, 4, kRplF64, kRplPair8>(PairFamily::kPolicy, false, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pairhmm_pair_policy_kernel<maxr.value, fused_mul.value>), grid, block, 0, s, d, q); });
}
// the per-pair policy of a mid-size call in two launches (pairhmm_pair_flag_kernel): `list` holds n_pairs entries
int launch_pair_policy_two_step(const FwdArgs<double>& d, const PairPolicyArgs& q, int rows, int fma, int64_t n_pairs, int32_t* list, hipStream_t s) {
  hipLaunchKernelGGL(pairhmm_pair_flag_kernel, dim3((unsigned)multi_flag_blocks((int)n_pairs)), dim3(kFlagBlock), 0, s, q, (int32_t)n_pairs, list);
  const dim3 grid((unsigned)multi_recompute_blocks((int)n_pairs)), block(64);
  return launch_pair_form<2, 4, kRplF64, kRplPair8>(PairFamily::kRecompute, false, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pairhmm_pair_recompute_kernel<maxr.value, fused_mul.value>), grid, block, 0, s, d, q, list); });
}
// tiny calls: fp32 + policy + fp64 of ONE pair per wavefront in one launch (pairhmm_pair_fused_kernel)
// `speculate`: nothing else is on the device -- the fp64 recomputation of every pair runs beside its fp32 recurrence
// (pairhmm_pair_spec_kernel) and the call takes max(fp32, fp64) instead of fp32 + fp64
int launch_pair_fused(const FwdArgs<float>& f, const FwdArgs<double>& d, const PairPolicyArgs& q, int rows, int fma, int64_t n_pairs,
                      hipStream_t s, bool speculate = false) {
  // Opt-in (GKLHIP_SPECULATE_FP64=1, read when the context is made, and only for a call that is alone on the device): it pays when a good share of the pairs fails the policy (100 x 10 with
  // 16 % failing: 0.151 -> 0.130 ms per call) and costs when none does (0.100 -> 0.130: the fp64 wavefront of a pair takes
  // twice as long as its fp32 one) -- and real active regions are mostly of the second kind.
  const dim3 grid((unsigned)n_pairs);
  if (const int spec = speculate ? pair_spec_form(rows) : 0) {   // (0: the speculating kernel has no 8-row form)
    const bool found = dispatch_pair_form<kRplF64>(spec, fma != 0, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pairhmm_pair_spec_kernel<maxr.value, fused_mul.value>), grid, dim3(128), 0, s, f, d, q); });
    return found ? GKLHIP_OK : fail(GKLHIP_ERR_UNSUPPORTED, "no speculating per-pair kernel for %d rows per lane", rows);
  }
  return launch_pair_form<4, kRplF64, kRplPair8>(PairFamily::kFused, false, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pairhmm_pair_fused_kernel<maxr.value, fused_mul.value>), grid, dim3(64), 0, s, f, d, q); });
}
// small calls of a double-precision context: every pair in fp64, ONE pair per wavefront (pairhmm_pair_f64_kernel)
int launch_pair_f64(const FwdArgs<double>& d, const PairPolicyArgs& q, int rows, int fma, int64_t n_pairs, hipStream_t s) {
  const dim3 grid((unsigned)n_pairs), block(64);
  return launch_pair_form<4, kRplF64, kRplPair8>(PairFamily::kF64, false, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pairhmm_pair_f64_kernel<maxr.value, fused_mul.value>), grid, block, 0, s, d, q); });
}
// ---- ... and the launches of a SET of small calls (SmallCombiner::launch_multi; pairhmm_aux_kernels.h: the *_multi_kernel
// forms).  `m` holds the calls and where each call's blocks begin in this launch; `rows`: of the set's widest call. ----
dim3 set_grid(const MultiArgs& m) { return dim3((unsigned)m.begin[m.n]); }
int launch_pair_set(PairFamily family, const MultiArgs& m, int rows, int fma, hipStream_t s) {
  const dim3 grid = set_grid(m), block(64);
  switch (family) {
    case PairFamily::kPolicy:
      return launch_pair_form<kRplF64, kRplPair8>(family, true, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pair_policy_multi_kernel<fused_mul.value, maxr.value>), grid, block, 0, s, m); });
    case PairFamily::kRecompute:
      return launch_pair_form<2, 4, kRplF64, kRplPair8>(family, true, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pair_recompute_multi_kernel<fused_mul.value, maxr.value>), grid, block, 0, s, m); });
    case PairFamily::kFused:
      return launch_pair_form<4, kRplF64, kRplPair8>(family, true, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pair_fused_multi_kernel<fused_mul.value, maxr.value>), grid, block, 0, s, m); });
    default:   // PairFamily::kF64
      return launch_pair_form<4, kRplF64, kRplPair8>(family, true, rows, fma, [&](auto maxr, auto fused_mul) { hipLaunchKernelGGL((pair_f64_multi_kernel<fused_mul.value, maxr.value>), grid, block, 0, s, m); });
  }
}
// the packed fp32 pass of a set (each call at its own rpl_main), and the packed fp64 pass of a set of mid-size regions of
// double-precision contexts
void launch_stream_f32_set(const MultiArgs& m, int fma, hipStream_t s) {
  if (fma) hipLaunchKernelGGL((fwd_stream_multi_kernel<true, kRplF32>), set_grid(m), dim3(64), 0, s, m);
  else     hipLaunchKernelGGL((fwd_stream_multi_kernel<false, kRplF32>), set_grid(m), dim3(64), 0, s, m);
}
void launch_stream_f64_set(const MultiArgs& m, int fma, hipStream_t s) {
  if (fma) hipLaunchKernelGGL((fwd_stream_f64_multi_kernel<true, kRplF64Jobs>), set_grid(m), dim3(64), 0, s, m);
  else     hipLaunchKernelGGL((fwd_stream_f64_multi_kernel<false, kRplF64Jobs>), set_grid(m), dim3(64), 0, s, m);
}

// A small plan (GATK-sized call) is PULLED from the pinned staging block by the prep kernel itself: no copy-engine hop at all.
bool plan_pulled(size_t plan_bytes) { return plan_bytes < (1u << 20); }  // (256 KB .. 2 MB measure within 2 % on calls of 4k-50k pairs, 1 MB best)
bool finalizes_on_device(int mode) { return mode == GKLHIP_FINALIZE_DEVICE_F64 || mode == GKLHIP_FINALIZE_DEVICE_REF32; }

// The six byte arrays of a batch in ONE buffer: the five read arrays `stride` apart, then the haplotype bases.
size_t six_arrays_bytes(const gklhip_batch* b) { return 5 * align_up((size_t)b->read_off[b->n_reads]) + align_up((size_t)b->hap_off[b->n_haps]); }
// a GATK-sized host call: the six arrays travel inside the plan block (ONE copy or pull for plan + inputs)
bool inputs_inline(const gklhip_batch* hb) { return six_arrays_bytes(hb) <= kSmallBatchBytes; }
// ... `b` with its array pointers into such a buffer at `base`
gklhip_batch batch_at(const gklhip_batch& b, const unsigned char* base, size_t stride) {
  gklhip_batch v = b;
  v.read_bases = base; v.read_quals = base + stride; v.ins_gop = base + 2 * stride;
  v.del_gop = base + 3 * stride; v.gcp = base + 4 * stride; v.hap_bases = base + 5 * stride;
  return v;
}
// ... and the arrays of `b` on their way there: put(offset in the buffer, source, bytes) is the copy (memcpy, H2D, peer)
template <typename F>
int copy_six_arrays(const gklhip_batch& b, size_t stride, F put) {
  const size_t rl = (size_t)b.read_off[b.n_reads], hl = (size_t)b.hap_off[b.n_haps];
  const uint8_t* srcs[5] = {b.read_bases, b.read_quals, b.ins_gop, b.del_gop, b.gcp};
  for (int i = 0; i < 5; i++)
    if (int rc = put(i * stride, srcs[i], rl)) return rc;
  return put(5 * stride, b.hap_bases, hl);
}

// ---- step 1: the plan.  Everything a call decides before it touches the device, on the caller's stack. ----
struct CallPlan {
  int n_reads, n_haps;
  int64_t n_pairs;               // 0: an empty call -- nothing else is set, and nothing is staged or launched
  size_t rl, hl;                 // read / haplotype bases
  int finalize_mode, fma, rpl_main, carry_len;
  Arrays where;                  // where the batch's byte arrays live
  bool inline_host() const { return where == Arrays::kHostInline; }
  bool use_double;
  int n_long_main, n_long64;     // reads too long for a chunk of the main pass / of the packed fp64 pass
  PlanLayout L;
  bool pull;                     // the prep kernel pulls the block from pinned memory (plan_pulled)
  bool per_pair, fused;          // policy + fp64 of one pair per wavefront; ... with the fp32 recurrence in the same wavefront and launch
  bool pair_double;              // a double-precision single-device context's call that fits the fp64 per-pair kernel (no read beyond small_read_len_max)
  int rows;                      // rows per lane of the per-pair kernels, by the longest read
  bool defers;                   // planned and staged, then handed to the small-call combiner (small_call_defers)
  int n_hist, chunk_stride, n_main_blocks, n_long_waves;   // grids and sizes that follow from the plan
  size_t striped_carry_bytes;
  int64_t xsteps;                // steps of a super-stripe carry row (0: no read needs super-stripes)
  std::chrono::steady_clock::time_point t0;   // (GKLHIP_TIMING)
};

// Which host-buffer calls are deferred -- planned and staged, then launched by the small-call combiner, alone or in one
// set of launches with others (concurrent callers' calls, the regions of one gklhip_compute_multi).  What a host call
// knows before it is planned (whether to offer deferral at all): inputs inline, not switched off (GKL_HIP_COMBINE=0) ...
// -- or a region of gklhip_compute_multi_device: its arrays in HBM stand where "inputs inline" stands (the same size
// limit: MultiCallOps::plan says kRegionInHbm only within it).
bool deferral_offered(Arrays where) { return g_env.combine && where != Arrays::kDevice; }
// ... and of a planned call that was offered it, what the three rules below have in common: plan block pulled, no event
// recording, no long read, host-exact packed finalisation, something to compute.
bool launches_shareable(const DevCtx* c, const CallPlan& P) {
  return deferral_offered(P.where) && P.pull && c->cfg.record_events == 0 && c->plan.long_reads.empty() && P.finalize_mode == kModePacked && c->plan.n_chunks > 0;
}
bool mid_size(const CallPlan& P) { return P.n_pairs > kTwoStepFrom && P.n_pairs <= kDirectPairs; }
// A small call (plan_call asks, nowhere else): a per-pair call of at most kTwoStepFrom pairs.  A double-precision
// context's call (kSmallDouble) likewise: its per-pair kernel holds reads of up to 383 bases, or 511 with the context's
// small_read_limit (pair_double), and its size limit has a name of its own (kSmallDoublePairs).
bool small_call_defers(const DevCtx* c, const CallPlan& P) {
  return launches_shareable(c, P) && (P.per_pair || P.pair_double) && P.n_pairs <= (P.pair_double ? kSmallDoublePairs : kTwoStepFrom);
}
// A mid-size region of a gklhip_compute_multi call shares a set with others of its kind (multi_call_drive): its policy in
// two launches (per-pair, not fused).  Asked of a plan that small_call_defers turned down; a SINGLE call asks through
// mid_call_combines only.
bool mid_call_shares(const DevCtx* c, const CallPlan& P) { return launches_shareable(c, P) && P.per_pair && !P.fused && mid_size(P); }
// ... and a mid-size region of a double-precision context (kSmallDoubleStream): the same of the all-fp64 pass.  No read
// too long for a chunk of the packed fp64 pass (639 bases at kRplF64Jobs rows per lane: the limit is the chunk, not the
// per-pair kernel's 383), a single-device context (a multi-device one keeps the general pass, as for kSmallDouble).
bool double_mid_shares(const DevCtx* c, const CallPlan& P) { return launches_shareable(c, P) && P.use_double && !c->multi_device && mid_size(P); }
// A SINGLE call's mid-size region enters the combiner -- staged as a multi call stages one, launched in a set with the
// like regions of concurrent callers or as a set of one -- where the context's switch says so (gklhip_set_mid_combine /
// GKL_HIP_COMBINE_MID; off by default) and one of the two rules above holds.  Asked by dev_compute_host_impl of a plan that
// was offered deferral and that small_call_defers turned down; the shards of a multi-device context keep the general pass.
bool mid_call_combines(const DevCtx* c, const CallPlan& P) {
  return c->mid_combine != 0 && !c->multi_device && (mid_call_shares(c, P) || double_mid_shares(c, P));
}
// The longest read of a call that may take the per-pair kernels: 383 bases (64 lanes x kRplF64 rows - 1), or 511 (x kRplPair8)
// where the context's small_read_limit says so AND the call is one the small-call path is offered at all -- a host call
// with its inputs inline, combining not switched off, a single-device context without event recording.  Everything else
// (device-resident calls, multi-device contexts, record_events, GKL_HIP_COMBINE=0) keeps the general pass for such reads.
// The regions of gklhip_compute_multi_device (kRegionInHbm) are offered the small-call path but not the fourth tier:
// their limit is 383 bases whatever the context's small_read_limit says.
static_assert(kRplPair8 == kRplF32 && kRplPair8 == kRplF64Wide, "the fourth tier: one wavefront at 8 rows per lane in both precisions");
int small_read_len_max(const DevCtx* c, Arrays where) {
  const bool fourth_tier = where == Arrays::kHostInline && c->small_read_limit == pair_tier_len_max(kRplPair8) && deferral_offered(where) && !c->multi_device && c->cfg.record_events == 0;
  return pair_tier_len_max(fourth_tier ? kRplPair8 : kRplF64);
}
// `load` of pick_f32_rpl: 1 for a call that is not offered deferral.  (About half of the calls inside the library are on
// the device at any moment, the others are being staged or finalised: 16 callers of 100 x 10 regions keep the 4-row
// kernel -- the 8-row one needs three wavefronts per SIMD to pay, tools/small_scaling.py -- and 32 callers get the 8-row one.)
int call_load(bool deferral) {
  return !deferral ? 1 : g_env.combine_load > 0 ? g_env.combine_load : std::max(1, g_host_calls_in_flight.load(std::memory_order_relaxed) / 2);
}

// Host only: no HIP call, no stream.  Fills c->plan, c->long_lanes, c->long_jobs and the statistics a plan decides.
// `db` holds host offsets; the byte arrays are not read.
void plan_call(DevCtx* c, const gklhip_batch* db, int finalize_mode, Arrays where, bool deferral, int load, CallPlan* out) {
  CallPlan& P = *out;
  const int n_reads = P.n_reads = db->n_reads, n_haps = P.n_haps = db->n_haps;
  P.n_pairs = (int64_t)n_reads * n_haps;
  P.defers = false;
  gklhip_stats& st = c->stats;
  memset(&st, 0, sizeof st);
  st.n_pairs = P.n_pairs;
  c->have_last = false;
  if (P.n_pairs == 0) return;
  P.finalize_mode = finalize_mode;
  P.where = where;
  P.use_double = c->cfg.use_double != 0;
  P.fma = c->cfg.fma_mode != 0;
  P.t0 = std::chrono::steady_clock::now();
  Plan& plan = c->plan;
  P.rpl_main = P.use_double ? kRplF64Jobs : pick_f32_rpl(c->cfg.rows_per_lane, n_reads, n_haps, db->read_off, db->hap_off, load);
  build_plan(n_reads, n_haps, db->read_off, db->hap_off, P.rpl_main, g_env.target_cols > 0 ? g_env.target_cols : kTargetCols, &plan);
  // Long reads: pseudo-chunks (lane 0 names the read) + one striped job per (read, stream group)
  // for the main pass; for the fp64 fallback the same pseudo-chunks feed the run detection.
  std::vector<PlanLane>& long_lanes = c->long_lanes;
  std::vector<FwdJob>& long_jobs = c->long_jobs;
  long_lanes.clear(); long_jobs.clear();
  P.n_long_main = (int)plan.long_reads.size();
  // pseudo-chunk index space: [0, n_long_main) main-pass reads, then [n_long_main, +n_long64) fp64-pass reads
  auto pseudo_chunk = [&](int32_t r) { long_lanes.resize(long_lanes.size() + kLanes, PlanLane{-1, 0}); long_lanes[long_lanes.size() - kLanes] = PlanLane{r, 0}; };
  for (int32_t r : plan.long_reads) pseudo_chunk(r);
  P.n_long64 = 0;  // reads too long for the packed fp64 pass
  if (!P.use_double && plan.max_read_len > kLanes * kRplF64Jobs - 1)
    for (int r = 0; r < n_reads; r++)
      if (blocks_for((int)(db->read_off[r + 1] - db->read_off[r]), kRplF64Jobs) > kLanes) { pseudo_chunk(r); P.n_long64++; }
  for (int i = 0; i < P.n_long_main; i++)
    for (const PlanGroup& g : plan.groups) long_jobs.push_back(FwdJob{i, g.hap_begin, g.hap_end, 0});
  int carry_len = 0;
  for (const PlanGroup& g : plan.groups) {
    const int last = g.hap_end - 1;
    carry_len = std::max(carry_len, plan.hap_pos[last] + plan.hap_len[last] - plan.hap_pos[g.hap_begin] + 3 * kLanes);
  }
  P.carry_len = (carry_len + 63) / 64 * 64;
  P.rl = (size_t)db->read_off[n_reads]; P.hl = (size_t)db->hap_off[n_haps];
  P.L = layout_for(plan, n_reads, n_haps, long_lanes.size(), long_jobs.size(), P.rl, P.hl, where);
  P.pull = plan_pulled(P.L.total);
  // policy + fp64 recomputation of one pair per wavefront (the kernel holds at most 64 x kRplF64 - 1 rows, or 64 x
  // kRplPair8 - 1 where the context's small_read_limit admits the fourth tier: small_read_len_max)
  const int pair_len_max = small_read_len_max(c, where);
  P.per_pair = !P.use_double && P.n_pairs <= kDirectPairs && P.n_long64 == 0 && plan.max_read_len <= pair_len_max;
  // ... the tiny ones (one GATK active region) with the fp32 recurrence in the same wavefront and launch as the policy
  const int64_t fused_max = g_env.fused_max >= 0 ? g_env.fused_max : (int64_t)kTwoStepFrom;
  P.fused = P.per_pair && g_env.fused_pairs && P.n_pairs <= fused_max && P.n_long_main == 0 && c->cfg.rows_per_lane == 0;
  P.rows = pair_rows_for(plan.max_read_len);
  // a double-precision context: every pair through the same fp64 per-pair code, when the call's reads fit it (the shards
  // of a multi-device context keep the general pass: that mode is as it was)
  P.pair_double = P.use_double && !c->multi_device && plan.max_read_len <= pair_len_max;
  P.defers = deferral && small_call_defers(c, P);

  P.n_hist = P.use_double ? 0 : 2 * (n_haps + 2);
  // XCD-aware grid of the streaming kernels (fwd_stream_block): a chunk's jobs all land on one XCD
  // (c->n_xcds: what the device reports -- 8 on an MI355X in SPX mode; a partitioned device shows fewer and gets no padding it cannot use)
  const int xq = c->n_xcds;
  P.chunk_stride = (g_env.xcd_aware && xq > 1 && plan.n_chunks >= 64) ? (plan.n_chunks + xq - 1) / xq * xq : plan.n_chunks;
  P.n_main_blocks = P.chunk_stride * (int)plan.groups.size();
  // persistent wavefronts of the striped long-read kernel: one per job up to two per SIMD (each owns two carry rows of
  // the longest stream group: ~110 KB)
  P.n_long_waves = (int)std::min<size_t>(2048, std::max<size_t>(512, std::max(long_jobs.size(), (size_t)P.n_long64 * plan.groups.size())));
  // ... and, when a read needs more wavefronts than a wide workgroup holds, the super-stripe kernel's carry rows behind them
  P.striped_carry_bytes = (size_t)P.n_long_waves * 2 * (3 * (size_t)P.carry_len + 64) * sizeof(double);
  const bool super_long = (blocks_for(plan.max_read_len, kRplF32) + kLanes - 1) / kLanes > kWideWavesMax;
  P.xsteps = super_long ? super_steps(P.carry_len, plan.max_read_len, kRplF32) : 0;   // (fp32 and fp64 both run the long reads at 8 rows per lane)
  static_assert(kRplF32 == kRplF64Wide, "one array depth for the long reads of both precisions");

  st.n_long_pairs = (int32_t)std::min<int64_t>((int64_t)P.n_long_main * n_haps, 0x7fffffff);
  st.n_chunks = plan.n_chunks;
  st.n_hap_groups = (int)plan.groups.size();
  st.rows_per_lane = P.rpl_main;
  st.lane_fill = plan.n_chunks ? (float)((double)plan.useful_rows / ((double)plan.n_chunks * 64 * P.rpl_main)) : 0.f;
  st.cells = (int64_t)P.rl * (int64_t)P.hl;
}

// ---- step 2: the plan block and its way to the device ----
// the haplotype streams and 'N' flags of a host call (what prep_kernel builds on the device for resident batches)
void build_host_streams(unsigned char* hs, const PlanLayout& L, const Plan& plan, const uint8_t* hap_bases, int n_haps) {
  uint32_t* sg = reinterpret_cast<uint32_t*>(hs + L.stream);
  uint32_t* sf = reinterpret_cast<uint32_t*>(hs + L.stream_flat);
  uint8_t* hn = hs + L.has_n;
  for (int k = 0; k < n_haps; k++) {
    const uint8_t* src = hap_bases + plan.hap_src[k];
    const int len = plan.hap_len[k], pg = plan.hap_pos[k], pf = plan.hap_pos_flat[k];
    bool has_n = false;
    for (int col = 0; col < len; col++) {
      const uint8_t bb = src[col];  // pairhmm_common.h:57-61: A0 C1 T2 G3 N4, anything else 0
      const uint32_t e = bb == 'C' ? 1u : bb == 'T' ? 2u : bb == 'G' ? 3u : bb == 'N' ? 4u : 0u;
      sg[pg + col] = e; sf[pf + col] = e;
      has_n |= bb == 'N';
    }
    sg[pg + len] = kEntSep | (uint32_t)k;
    sf[pf + len] = kEntSep | (uint32_t)k;
    hn[k] = has_n ? 1 : 0;
    if (k + 1 == n_haps || plan.hap_group[k + 1] != plan.hap_group[k])
      for (int i = 0; i < kLanes; i++) sg[pg + len + 1 + i] = kEntIdle;
    if (k + 1 == n_haps)
      for (int i = 0; i < kLanes; i++) sf[pf + len + 1 + i] = kEntIdle;
  }
}
// Writes the block at `hs` (P.L.total bytes of plain memory; no HIP object is touched).
void fill_plan_block(unsigned char* hs, const CallPlan& P, const Plan& plan, const std::vector<PlanLane>& long_lanes,
                     const std::vector<FwdJob>& long_jobs, const gklhip_batch* db) {
  const PlanLayout& L = P.L;
  const int n_reads = P.n_reads, n_haps = P.n_haps;
  memcpy(hs + L.place_chunk, plan.place_chunk.data(), (size_t)n_reads * 4);
  memcpy(hs + L.place_lane, plan.place_lane.data(), (size_t)n_reads);
  memcpy(hs + L.chunk_used, plan.chunk_used.data(), (size_t)plan.n_chunks);
  memcpy(hs + L.groups, plan.groups.data(), plan.groups.size() * sizeof(PlanGroup));
  memcpy(hs + L.hap_len, plan.hap_len.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_pos, plan.hap_pos.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_pos_flat, plan.hap_pos_flat.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_orig, plan.hap_orig.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_sidx, plan.hap_sidx.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_group, plan.hap_group.data(), (size_t)n_haps * 4);
  memcpy(hs + L.hap_src, plan.hap_src.data(), (size_t)n_haps * 4);
  {
    // Y[0][j] = INITIAL_CONSTANT / (NUMBER)haplen, divided on the host (template.h:110,176)
    float* y32 = reinterpret_cast<float*>(hs + L.y0_32);
    double* y64 = reinterpret_cast<double*>(hs + L.y0_64);
    const float i32 = host_tables_f32().initial_constant;
    const double i64 = host_tables_f64().initial_constant;
    for (int k = 0; k < n_haps; k++) {
      y32[k] = i32 / (float)plan.hap_len[k];
      y64[k] = i64 / (double)plan.hap_len[k];
    }
  }
  memcpy(hs + L.read_off, db->read_off, (size_t)(n_reads + 1) * 8);
  if (!long_lanes.empty()) memcpy(hs + L.long_lanes, long_lanes.data(), long_lanes.size() * sizeof(PlanLane));
  if (!long_jobs.empty()) memcpy(hs + L.long_jobs, long_jobs.data(), long_jobs.size() * sizeof(FwdJob));
  {
    int32_t lc[4] = {(int32_t)long_jobs.size(), P.n_long_main, P.n_long64, 0};
    memcpy(hs + L.long_count, lc, sizeof lc);
  }
  if (P.inline_host()) {
    unsigned char* dst = hs + L.batch;
    copy_six_arrays(*db, L.batch_stride, [dst](size_t at, const uint8_t* src, size_t n) { memcpy(dst + at, src, n); return 0; });
    build_host_streams(hs, L, plan, db->hap_bases, n_haps);
  }
}

// A call whose block is on its way to the device and whose scratch is reserved: what the argument builders point at.
struct StagedCall {
  hipStream_t s;
  double* out;
  int slot;
  unsigned char* hs;            // the pinned staging block
  const unsigned char* hs_dev;  // ... as the device sees it (pulled plans only)
  unsigned char* dp;            // the device copy of the block
  DevBatch b;                   // the batch as the forward kernels see it
  const uint8_t* hap_bases;     // ... and its haplotype bases as the prep kernel does
  uint32_t *stream_grouped, *stream_flat;
  uint8_t *hap_has_n, *xcarry;  // xcarry: carry rows of the super-stripe kernel (reserve_carry)
};

// `db` holds host offsets and DEVICE byte arrays -- or, with P.inline_host(), HOST byte arrays that travel inside the plan
// block (small host-buffer calls: one copy for plan and inputs).  Flips c->plan_slot.
int stage_call(DevCtx* c, const gklhip_batch* db, const CallPlan& P, double* out_dev, hipStream_t s, StagedCall* out) {
  const PlanLayout& L = P.L;
  const Plan& plan = c->plan;
  StagedCall& S = *out;
  int rc;
  const int slot = c->plan_slot ^= 1;
  PinBuf& stage = c->stage_slot[slot];
  DevBuf& plan_dev = c->plan_dev_slot[slot];
  HIP_TRY(hipEventSynchronize(c->stage_free_slot[slot]));
  if (L.total > stage.cap || L.total > plan_dev.cap) HIP_TRY(hipEventSynchronize(c->plan_unused_slot[slot]));  // about to reallocate
  if ((rc = stage.reserve(L.total))) return rc;
  if ((rc = plan_dev.reserve(L.total))) return rc;
  unsigned char* hs = stage.as<unsigned char>();
  fill_plan_block(hs, P, plan, c->long_lanes, c->long_jobs, db);
  unsigned char* dp = plan_dev.as<unsigned char>();
  // scratch is shared by the calls of a context: one on another stream than the last one waits for that one's end
  if (c->have_call_done && c->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->call_done, 0));
  // Big plans ride the upload stream (the copy overlaps the previous call's kernels); a small one is pulled (plan_pulled).
  S.hs_dev = nullptr;
  if (P.pull) {
    void* p = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&p, hs, 0));
    S.hs_dev = static_cast<const unsigned char*>(p);
    // (a deferred call is launched by the combiner, maybe on another stream: a lane's slot events are never recorded)
    if (!P.defers) HIP_TRY(hipStreamWaitEvent(s, c->plan_unused_slot[slot], 0));
  } else {
    if ((rc = aux_streams(c))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->upload_stream, c->plan_unused_slot[slot], 0));  // readers of the old contents are done
    HIP_TRY(hipMemcpyAsync(dp, hs, L.total, hipMemcpyHostToDevice, c->upload_stream));
    HIP_TRY(hipEventRecord(c->stage_free_slot[slot], c->upload_stream));
    HIP_TRY(hipStreamWaitEvent(s, c->stage_free_slot[slot], 0));                    // kernels below read the new plan
  }
  if (g_env.timing)
    fprintf(stderr, "[gklhip] host plan + staging: %.3f ms (%d chunks, %d stream entries, %zu plan bytes)\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - P.t0).count(),
            plan.n_chunks, plan.n_stream, L.total);

  // ---- scratch ----
  if ((rc = c->raw32.reserve((size_t)P.n_pairs * 4))) return rc;
  if ((rc = c->raw64.reserve((size_t)P.n_pairs * 8))) return rc;
  if ((rc = c->used64.reserve((size_t)P.n_pairs))) return rc;
  if ((rc = c->counters.reserve(128))) return rc;
  if ((rc = c->read_fail.reserve((size_t)P.n_reads * 4))) return rc;
  if ((rc = c->stream_buf.reserve(((size_t)plan.n_stream + (size_t)plan.n_stream_flat) * 4))) return rc;
  if (!P.use_double && (rc = c->fail_hist.reserve((size_t)P.n_hist * 4))) return rc;
  if ((rc = c->hap_flags.reserve((size_t)P.n_haps))) return rc;
  if ((rc = c->lanes_main.reserve((size_t)std::max(plan.n_chunks, 1) * kLanes * sizeof(LaneSlot)))) return rc;

  S.s = s; S.out = out_dev; S.slot = slot; S.hs = hs; S.dp = dp; S.xcarry = nullptr;
  // the six byte arrays as the device reads them: inside the block, or where the caller put them
  const gklhip_batch dbi = P.inline_host() ? batch_at(*db, dp + L.batch, L.batch_stride) : *db;
  S.b = DevBatch{dbi.read_bases, dbi.read_quals, dbi.ins_gop, dbi.del_gop, dbi.gcp, reinterpret_cast<const int64_t*>(dp + L.read_off), P.n_reads, P.n_haps};
  // (pulling: the prep kernel reads the HOST copy of the block)
  S.hap_bases = (P.pull && P.inline_host()) ? batch_at(*db, S.hs_dev + L.batch, L.batch_stride).hap_bases : dbi.hap_bases;
  // (host-built streams arrive with the block; the prep kernel then only pulls and clears)
  S.stream_grouped = P.inline_host() ? reinterpret_cast<uint32_t*>(dp + L.stream) : c->stream_buf.as<uint32_t>();
  S.stream_flat = P.inline_host() ? reinterpret_cast<uint32_t*>(dp + L.stream_flat) : c->stream_buf.as<uint32_t>() + plan.n_stream;
  S.hap_has_n = P.inline_host() ? dp + L.has_n : c->hap_flags.as<uint8_t>();
  return GKLHIP_OK;
}

// ---- step 3: the kernels' arguments, each a function of (context, plan, staged call) ----
// haplotype streams + clears + the pull of the block: one launch
PrepArgs prep_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const PlanLayout& L = P.L;
  PrepArgs pa;
  const unsigned char* pb = P.pull ? S.hs_dev : S.dp;  // pulling: this kernel reads the HOST copy of the plan
  pa.hap_bases = S.hap_bases;
  pa.hap_src = reinterpret_cast<const int32_t*>(pb + L.hap_src);
  pa.hap_len = reinterpret_cast<const int32_t*>(pb + L.hap_len);
  pa.hap_pos = reinterpret_cast<const int32_t*>(pb + L.hap_pos);
  pa.hap_group = reinterpret_cast<const int32_t*>(pb + L.hap_group);
  pa.stream = S.stream_grouped;
  // the flat stream (no gaps between groups): the fp64 recomputation's jobs are arbitrary runs of it
  // (a double-precision context's general pass has none; its per-pair kernel does, and a region of
  //  gklhip_compute_multi_device that takes it has its streams built here, not on the host)
  const bool flat = !P.use_double || (P.where == Arrays::kRegionInHbm && P.pair_double);
  pa.hap_pos_flat = flat ? reinterpret_cast<const int32_t*>(pb + L.hap_pos_flat) : nullptr;
  pa.stream_flat = S.stream_flat;
  pa.hap_has_n = S.hap_has_n;
  pa.n_haps = P.inline_host() ? 0 : P.n_haps;   // (host-built streams)
  pa.clear_a = c->counters.as<int32_t>(); pa.n_a = 32;
  pa.clear_b = c->read_fail.as<int32_t>(); pa.n_b = P.use_double ? 0 : P.n_reads;
  pa.clear_c = c->fail_hist.as<int32_t>(); pa.n_c = P.n_hist;
  pa.place_chunk = reinterpret_cast<const int32_t*>(pb + L.place_chunk);
  pa.place_lane = pb + L.place_lane;
  pa.chunk_used = pb + L.chunk_used;
  pa.read_off = reinterpret_cast<const int64_t*>(pb + L.read_off);
  pa.lanes_out = c->lanes_main.as<LaneSlot>();
  pa.n_reads = P.n_reads; pa.n_chunks = c->plan.n_chunks; pa.rpl = P.rpl_main;
  const int threads_needed = std::max({pa.n_haps * 64, 32, pa.n_b, pa.n_c, P.n_reads});
  pa.hap_blocks = (threads_needed + kPrepBlock - 1) / kPrepBlock;
  pa.pull_src = reinterpret_cast<const uint4*>(S.hs_dev);
  pa.pull_dst = reinterpret_cast<uint4*>(S.dp);
  pa.pull_n16 = P.pull ? (int32_t)(L.total / 16) : 0;
  return pa;
}
int prep_grid(const PrepArgs& pa, const CallPlan& P) {
  return pa.hap_blocks + (P.pull ? (int)std::min<size_t>(64, (P.L.total / 16 + kPrepBlock * 4 - 1) / (kPrepBlock * 4)) : 0);
}

// The main pass in precision T (fp32 of the policy mode, fp64 of the all-fp64 mode).
template <typename T>
FwdArgs<T> fwd_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  constexpr bool is_f32 = std::is_same<T, float>::value;
  const PlanLayout& L = P.L;
  unsigned char* dp = S.dp;
  FwdArgs<T> a{};
  a.b = S.b;
  a.stream = S.stream_grouped;
  a.hap_len = reinterpret_cast<const int32_t*>(dp + L.hap_len);
  a.hap_pos = reinterpret_cast<const int32_t*>(dp + L.hap_pos);
  a.hap_orig = reinterpret_cast<const int32_t*>(dp + L.hap_orig);
  a.hap_has_n = S.hap_has_n;
  a.groups = reinterpret_cast<const HapGroup*>(dp + L.groups);
  a.n_groups = (int)c->plan.groups.size();
  a.chunk_lanes = c->lanes_main.as<LaneSlot>();
  a.n_chunks = c->plan.n_chunks;
  a.chunk_stride = P.chunk_stride;
  a.jobs = c->jobs.as<FwdJob>();
  a.job_count = c->counters.as<int32_t>() + 2;
  a.job_next = c->counters.as<int32_t>() + 3;
  // the fp32 programs fetch a separator lane's priors from beyond the LDS allocation: only where that reads 0 (dev_init)
  a.asm_general = (c->asm_general && (!is_f32 || c->lds_oob_zero)) ? 1 : 0;
  if constexpr (is_f32) {
    a.tab = c->dt32;
    a.y0 = reinterpret_cast<const float*>(dp + L.y0_32);
    a.raw = c->raw32.as<float>();
    // host-exact packed words straight from the forward kernels (the per-pair path applies the policy per pair and
    // writes the words itself)
    a.packed_out = (P.finalize_mode == kModePacked && !P.per_pair) ? reinterpret_cast<uint64_t*>(S.out) : nullptr;
  } else {
    a.tab = c->dt64;
    a.y0 = reinterpret_cast<const double*>(dp + L.y0_64);
    a.raw = c->raw64.as<double>();
  }
  return a;
}
// ... its long reads: the pseudo-chunks and jobs that came with the plan block
template <typename T>
FwdArgs<T> long_main_args(const DevCtx* c, const CallPlan& P, const StagedCall& S, const FwdArgs<T>& a) {
  FwdArgs<T> la = a;
  la.chunk_lanes = reinterpret_cast<const LaneSlot*>(S.dp + P.L.long_lanes);
  la.jobs = reinterpret_cast<const FwdJob*>(S.dp + P.L.long_jobs);
  la.job_count = reinterpret_cast<const int32_t*>(S.dp + P.L.long_count);
  la.job_next = c->counters.as<int32_t>() + 7;
  return la;
}
// fp64 arguments shared by the two ways of recomputing (the flat stream: a job may run across stream groups)
FwdArgs<double> recompute_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  FwdArgs<double> d = fwd_args<double>(c, P, S);
  d.stream = S.stream_flat;
  d.hap_pos = reinterpret_cast<const int32_t*>(S.dp + P.L.hap_pos_flat);
  // (the planned fp64 pass leaves the packed words of the recomputed pairs to finalize64_kernel: its jobs run as whole-job
  //  asm programs that store the raw sums only)
  d.packed_out = nullptr;
  d.packed_only_flagged = c->used64.as<uint8_t>();
  return d;
}
FinalizeArgs finalize_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  FinalizeArgs fa;
  fa.raw32 = c->raw32.as<float>(); fa.raw64 = c->raw64.as<double>(); fa.out = S.out;
  fa.used64 = c->used64.as<uint8_t>();
  fa.count = c->counters.as<int32_t>(); fa.n = P.n_pairs; fa.mode = P.finalize_mode;
  fa.read_fail = c->read_fail.as<int32_t>(); fa.n_haps = P.n_haps;
  fa.log10_init_f = host_tables_f32().log10_initial; fa.log10_init32_as_f64 = std::log10(std::ldexp(1.0, 120)); fa.log10_init_d = host_tables_f64().log10_initial;
  return fa;
}
PairPolicyArgs pair_policy_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  PairPolicyArgs q;
  q.raw32 = c->raw32.as<float>(); q.out = S.out; q.used64 = c->used64.as<uint8_t>(); q.count = c->counters.as<int32_t>();
  q.hap_sidx = reinterpret_cast<const int32_t*>(S.dp + P.L.hap_sidx);
  q.mode = P.finalize_mode;
  q.log10_init_f = host_tables_f32().log10_initial; q.log10_init32_as_f64 = std::log10(std::ldexp(1.0, 120)); q.log10_init_d = host_tables_f64().log10_initial;
  return q;
}
// precision policy + device-side planning of the fp64 recomputation (buffers: launch_planned_fp64 reserves them)
size_t planned_max_jobs(const CallPlan& P) { return (size_t)P.n_reads * (size_t)P.n_haps; }  // a job holds at least one haplotype and the jobs of a chunk do not overlap
PlanArgs plan_args(const DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const PlanLayout& L = P.L;
  unsigned char* dp = S.dp;
  const int n_reads = P.n_reads, n_haps = P.n_haps;
  PlanArgs pa;
  pa.fa = finalize_args(c, P, S);
  pa.n_reads = n_reads; pa.n_haps = n_haps; pa.n_pairs_i = (int32_t)P.n_pairs;
  pa.read_off = S.b.read_off;
  pa.rpl = kRplF64Jobs; pa.max_len = kLanes * kRplF64Jobs - 1;
  pa.cnts = c->counters.as<int32_t>();
  pa.hist = c->fail_hist.as<int32_t>();
  pa.pos = pa.hist + (n_haps + 2);
  pa.order = c->fail_order.as<int32_t>();
  pa.lanes2 = c->lanes2.as<LaneSlot>();
  pa.hap_orig = reinterpret_cast<const int32_t*>(dp + L.hap_orig);
  pa.hap_group = reinterpret_cast<const int32_t*>(dp + L.hap_group);
  pa.hap_pos = reinterpret_cast<const int32_t*>(dp + L.hap_pos_flat);
  pa.hap_len = reinterpret_cast<const int32_t*>(dp + L.hap_len);
  pa.jobs = c->jobs.as<FwdJob>();
  pa.sorted = c->jobs.as<FwdJob>() + planned_max_jobs(P);
  pa.long_lanes = reinterpret_cast<const LaneSlot*>(dp + L.long_lanes) + (size_t)P.n_long_main * kLanes;
  pa.n_long = P.n_long64;
  pa.jobs_long = c->jobs_long.as<FwdJob>();
  pa.long_chunk_jobs = c->fail_order.as<int32_t>() + n_reads;
  pa.total_cols = (int32_t)std::min<int64_t>((int64_t)P.hl + n_haps, 0x7fffffff);
  // (a shard of the batch wants fewer, longer jobs: 4096 for an eighth, measured on the 1250 x 128 shard)
  pa.wanted_jobs = g_env.fb_wanted_jobs > 0 ? g_env.fb_wanted_jobs : (int)std::min<int64_t>(kFallbackWantedJobs, std::max<int64_t>(4096, P.n_pairs / 100));
  pa.min_job_cols = 256;
  pa.packed_by_kernels = (P.finalize_mode == kModePacked && !P.per_pair) ? 1 : 0;
  return pa;
}

// ---- step 4: the launches on S.s, one function per shape, each with its event records; no host synchronisation
// before finish_call.  In the policy mode a big call is 7 launches (prep, fp32 forward, the three launches of policy +
// planning of the fp64 pass, fp64 forward over the job list, log10 / packed words of the recomputed pairs; + the log10
// of the kept pairs on a side stream in the device finalisation modes), a call of up to 65 536 pairs 3-4 (prep, fp32
// forward, per-pair policy in one or two launches), one of up to 2048 pairs 2 (prep, the fused per-pair kernel).  A
// double-precision context's call is 3 (prep, fp64 forward, log10 / packed words) -- or, deferred (kSmallDouble), 2 from
// the combiner (prep, pairhmm_pair_f64_kernel); its mid-size regions of one multi call (kSmallDoubleStream) take the same 3
// once per set of up to 64 (SmallCombiner::launch_multi). ----
int launch_prep(DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const bool ev = c->cfg.record_events != 0;
  if (ev) {
    const bool deferred = c->cfg.record_events == 2;
    c->ev = c->ev_ring[deferred ? c->calls % DevCtx::kEventRing : 0];
    c->ring_double[deferred ? c->calls % DevCtx::kEventRing : 0] = P.use_double;
    c->calls++;
    HIP_TRY(hipEventRecord(c->ev[0], S.s));
  }
  const PrepArgs pa = prep_args(c, P, S);
  hipLaunchKernelGGL(prep_kernel, dim3((unsigned)prep_grid(pa, P)), dim3(kPrepBlock), 0, S.s, pa);
  if (P.pull) HIP_TRY(hipEventRecord(c->stage_free_slot[S.slot], S.s));
  return GKLHIP_OK;
}
// the carry rows of the long-read kernels (a call without long reads reserves none)
int reserve_carry(DevCtx* c, const CallPlan& P, StagedCall* S) {
  if (P.n_long_main == 0 && P.n_long64 == 0) return GKLHIP_OK;
  if (int rc = c->carry.reserve(P.striped_carry_bytes + (size_t)super_blocks_max<float>() * 2 * (size_t)P.xsteps * 32)) return rc;
  if (P.xsteps > 0) S->xcarry = c->carry.as<unsigned char>() + P.striped_carry_bytes;
  return GKLHIP_OK;
}
int launch_all_double(DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const bool ev = c->cfg.record_events != 0;
  hipStream_t s = S.s;
  const FwdArgs<double> a = fwd_args<double>(c, P, S);
  if (P.n_main_blocks > 0) launch_stream<double, kRplF64Jobs>(a, P.fma, P.n_main_blocks, s);
  if (P.n_long_main > 0)
    launch_long_jobs<double, kRplF64Wide, kRplF64>(long_main_args(c, P, S, a), P.fma, P.n_long_waves, c->plan.max_read_len, c->carry.as<double>(), P.carry_len, s,
                                                   S.xcarry, P.xsteps, c->counters.as<int32_t>() + 12);
  if (ev) HIP_TRY(hipEventRecord(c->ev[2], s));
  hipLaunchKernelGGL(finalize64_kernel, dim3((unsigned)((P.n_pairs + 255) / 256)), dim3(256), 0, s, finalize_args(c, P, S), 1);
  if (ev) { HIP_TRY(hipEventRecord(c->ev[3], s)); HIP_TRY(hipEventRecord(c->ev[4], s)); }
  HIP_TRY(hipEventRecord(c->policy_done, s));  // (host path: "results are final from here")
  return GKLHIP_OK;
}
// the fp32 main pass (a fused call's runs inside its per-pair kernel) and its long reads
int launch_main_pass_f32(DevCtx* c, const CallPlan& P, const StagedCall& S, const FwdArgs<float>& a) {
  hipStream_t s = S.s;
  if (P.n_main_blocks > 0 && !P.fused) launch_main_f32(a, P.rpl_main, P.fma, P.n_main_blocks, s);
  if (P.n_long_main > 0) {
    const FwdArgs<float> la = long_main_args(c, P, S, a);
    if (P.rpl_main <= 4) launch_long<float, 4>(la, P.fma, P.n_long_waves, c->carry.as<float>(), P.carry_len, s);  // (2 is only chosen without long reads)
    else                 launch_long_jobs<float, kRplF32, kRplF32>(la, P.fma, P.n_long_waves, c->plan.max_read_len, c->carry.as<float>(), P.carry_len, s, S.xcarry, P.xsteps, c->counters.as<int32_t>() + 12);
  }
  if (c->cfg.record_events != 0) HIP_TRY(hipEventRecord(c->ev[2], s));
  return GKLHIP_OK;
}
// Small calls (one GATK region): policy + fp64 recomputation + finalisation of one pair per wavefront -- fused with the
// fp32 recurrence, in ONE launch (pairhmm_pair_policy_kernel), or from kTwoStepFrom pairs in two.
int launch_per_pair(DevCtx* c, const CallPlan& P, const StagedCall& S, const FwdArgs<float>& a) {
  const bool ev = c->cfg.record_events != 0;
  hipStream_t s = S.s;
  const FwdArgs<double> d = recompute_args(c, P, S);
  const PairPolicyArgs q = pair_policy_args(c, P, S);
  if (ev) HIP_TRY(hipEventRecord(c->ev[3], s));
  if (P.fused) {
    if (int rc = launch_pair_fused(a, d, q, P.rows, P.fma, P.n_pairs, s, c->speculate_fp64 && g_host_calls_in_flight.load(std::memory_order_relaxed) <= 1)) return rc;
  } else if (P.n_pairs > kTwoStepFrom) {
    if (int rc = c->fail_order.reserve((size_t)P.n_pairs * 4)) return rc;
    if (int rc = launch_pair_policy_two_step(d, q, P.rows, P.fma, P.n_pairs, c->fail_order.as<int32_t>(), s)) return rc;
  } else {
    if (int rc = launch_pair_policy(d, q, P.rows, P.fma, P.n_pairs, s)) return rc;
  }
  if (ev) HIP_TRY(hipEventRecord(c->ev[4], s));
  HIP_TRY(hipEventRecord(c->policy_done, s));
  return GKLHIP_OK;
}
// Precision policy + device-side planning of the fp64 recomputation (three launches, no host round trip), the fp64
// recomputation of the underflowed pairs and their finalisation.
int launch_planned_fp64(DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const bool ev = c->cfg.record_events != 0;
  hipStream_t s = S.s;
  const int n_reads = P.n_reads;
  const int64_t n_pairs = P.n_pairs;
  const size_t max_jobs = planned_max_jobs(P);
  int rc;
  if ((rc = c->fail_order.reserve(((size_t)n_reads + (size_t)P.n_long64) * 4))) return rc;
  if ((rc = c->lanes2.reserve((size_t)n_reads * kLanes * sizeof(LaneSlot)))) return rc;
  if ((rc = c->jobs.reserve(2 * max_jobs * sizeof(FwdJob)))) return rc;  // as built + sorted by length
  if (P.n_long64 > 0 && (rc = c->jobs_long.reserve((size_t)P.n_long64 * (size_t)P.n_haps * sizeof(FwdJob)))) return rc;
  const PlanArgs pa = plan_args(c, P, S);
  // Three stream-ordered launches (pairhmm_aux_kernels.h): no block waits for another, so nothing limits how many
  // of these are in flight per device or process.  The policy takes a block per 4096 pairs (up to one per CU), the
  // packing a wavefront per window of affected reads, the run detection a wavefront per chunk (grid-stride).
  const int blocks_env = g_env.plan_blocks;
  const int policy_grid = std::max(1, blocks_env > 0 ? blocks_env : (int)std::min<int64_t>(c->n_cus, std::max<int64_t>(16, n_pairs / 4096)));
  const int64_t max_windows = ((int64_t)n_reads + kPackWindow - 1) / kPackWindow;
  const int pack_grid = (int)std::max<int64_t>(1, std::min<int64_t>(kPlanBlocks, (max_windows + kPlanBlock / 64 - 1) / (kPlanBlock / 64)));
  const int jobs_grid = std::max(1, std::min(c->n_cus, blocks_env > 0 ? blocks_env : (int)std::min<int64_t>(kPlanBlocks, std::max<int64_t>(16, n_pairs / 8192))));
  hipLaunchKernelGGL(plan_policy_kernel, dim3((unsigned)policy_grid), dim3(kPlanBlock), 0, s, pa);
  // The policy's flags and the kept pairs' words are final here: the log10 of the kept pairs (side stream below; the
  // host's early pass in host-buffer calls) starts now and overlaps the two small planning launches -- behind them it
  // would queue up against the fp64 pass, whose persistent wavefronts leave it no registers until they drain.
  HIP_TRY(hipEventRecord(c->policy_done, s));
  hipLaunchKernelGGL(plan_pack_kernel, dim3((unsigned)pack_grid), dim3(kPlanBlock), 0, s, pa);
  hipLaunchKernelGGL(plan_jobs_kernel, dim3((unsigned)jobs_grid), dim3(kPlanBlock), 0, s, pa);
  const bool side_finalize = finalizes_on_device(P.finalize_mode);
  if (side_finalize) {
    if ((rc = aux_streams(c))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->policy_done, 0));
    hipLaunchKernelGGL(finalize32_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, c->copy_stream, pa.fa);
    HIP_TRY(hipEventRecord(c->early_copy_done, c->copy_stream));
  }
  // ---- fp64 recomputation of the underflowed pairs: persistent wavefronts stream the job list -- same WaveJob
  // template as the main pass, T = double (no jobs: the kernel's wavefronts leave at once) ----
  FwdArgs<double> d = recompute_args(c, P, S);
  d.chunk_lanes = c->lanes2.as<LaneSlot>();
  d.n_chunks = n_reads;  // upper bound; the job list only names packed chunks
  d.jobs = c->jobs.as<FwdJob>() + max_jobs;
  if (ev) HIP_TRY(hipEventRecord(c->ev[3], s));
  launch_jobs<double, kRplF64Jobs>(d, P.fma, (int)std::min<int64_t>(n_pairs, (int64_t)c->n_cus * 16), s);
  if (P.n_long64 > 0) {
    // reads too long for a chunk: one pseudo-chunk each, same run detection, striped kernel
    int32_t* cnts = c->counters.as<int32_t>();
    FwdArgs<double> ld = d;
    ld.chunk_lanes = pa.long_lanes;
    ld.jobs = c->jobs_long.as<FwdJob>();
    ld.job_count = cnts + 8;
    ld.job_next = cnts + 9;
    launch_long_jobs<double, kRplF64Wide, kRplF64>(ld, P.fma, P.n_long_waves, c->plan.max_read_len, c->carry.as<double>(), P.carry_len, s, S.xcarry, P.xsteps, cnts + 13);
  }
  if (ev) HIP_TRY(hipEventRecord(c->ev[4], s));
  // (log10 of the recomputed pairs / host-buffer calls: their packed words)
  hipLaunchKernelGGL(finalize64_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, pa.fa, 0);
  if (side_finalize) HIP_TRY(hipStreamWaitEvent(s, c->early_copy_done, 0));  // join the side stream
  return GKLHIP_OK;
}
// The end of a launched call: its events, and -- record_events == 1 -- the statistics read back.
int finish_call(DevCtx* c, const CallPlan& P, const StagedCall& S) {
  const bool ev = c->cfg.record_events != 0;
  hipStream_t s = S.s;
  gklhip_stats& st = c->stats;
  if (ev) HIP_TRY(hipEventRecord(c->ev[5], s));
  HIP_TRY(hipGetLastError());

  HIP_TRY(hipEventRecord(c->plan_unused_slot[S.slot], s));
  HIP_TRY(hipEventRecord(c->call_done, s));
  c->have_call_done = true;
  c->last_pairs = P.n_pairs;
  c->last_stream = s;
  c->have_last = true;

  if (ev && c->cfg.record_events != 2) {
    HIP_TRY(hipEventSynchronize(c->ev[5]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); st.ms_fwd_main = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[3], c->ev[4])); st.ms_fwd_fallback = P.use_double ? 0.f : ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[5])); st.ms_total_device = ms;
    int32_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, c->counters.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.n_fallback = P.use_double ? P.n_pairs : cnt[0];
    if (g_env.timing && !P.use_double) {
      int32_t k[32];
      HIP_TRY(hipMemcpy(k, c->counters.p, sizeof k, hipMemcpyDeviceToHost));
      fprintf(stderr, "[gklhip] policy+plan phases, each from the start of its own launch (us): hist %.1f scan %.1f scatter %.1f pack %.1f jobs %.1f sort %.1f | "
              "%d affected reads, %d chunks, %d jobs | window 0: loaded %.1f ranked %.1f fitted %.1f cleared %.1f written %.1f\n",
              k[16] * 0.01, k[17] * 0.01, k[18] * 0.01, k[19] * 0.01, k[20] * 0.01, k[21] * 0.01,
              k[4], k[5], k[2], k[22] * 0.01, k[23] * 0.01, k[24] * 0.01, k[25] * 0.01, k[26] * 0.01);
    }
  } else {
    st.n_fallback = P.use_double ? P.n_pairs : -1;  // unknown without a sync; gklhip_get_raw fills it in
  }
  return GKLHIP_OK;
}

// The kind of a call that is staged for the combiner (SmallCall::kind; the multi call cuts its sets by it): one place
// for the descriptor and the cut.
int32_t small_call_kind(const CallPlan& P) {
  if (P.use_double && P.n_pairs > kSmallDoublePairs) return kSmallDoubleStream;
  return P.pair_double ? kSmallDouble : P.fused ? kSmallFused : P.n_pairs > kTwoStepFrom ? kSmallTwoStep : kSmallOneLaunch;
}
// ... the two kinds of mid-size regions (the combiner's caps on their sets: pairhmm_multi_sets.h)
bool small_kind_is_mid(int32_t kind) { return kind == kSmallTwoStep || kind == kSmallDoubleStream; }

// ---- step 5: the deferred exit.  Nothing is launched: the call's descriptor, from the same builders, goes into the
// staging block (still ours to write) and to the combiner. ----
void describe_small_call(DevCtx* c, const CallPlan& P, const StagedCall& S, SmallLaunch* out) {
  SmallCall& k = out->call;
  k.prep = prep_args(c, P, S);
  k.prep_grid = prep_grid(k.prep, P);
  k.kind = small_call_kind(P);
  // (kSmallDoubleStream: the grouped stream of the general all-fp64 pass, not the flat one of the per-pair kernels)
  const bool all_double = k.kind == kSmallDouble || k.kind == kSmallDoubleStream;
  k.f = all_double ? FwdArgs<float>{} : fwd_args<float>(c, P, S);
  k.d = k.kind == kSmallDoubleStream ? fwd_args<double>(c, P, S) : recompute_args(c, P, S);
  k.q = pair_policy_args(c, P, S);
  if (all_double) k.q.raw32 = nullptr;   // (no fp32 buffer is read or written)
  k.rpl_main = P.rpl_main; k.main_blocks = P.n_main_blocks; k.rows = P.rows; k.n_pairs = (int32_t)P.n_pairs; k.fma = P.fma;
  k.fused = P.fused ? 1 : 0;
  k.speculate = c->speculate_fp64;
  // (a mid-size region: its list is the lane's fail_order, reserved for n_pairs entries by whoever staged it)
  const bool two_step = k.kind == kSmallTwoStep;
  k.flag_grid = two_step || k.kind == kSmallDoubleStream ? multi_flag_blocks(k.n_pairs) : 0;
  k.recompute_grid = two_step ? multi_recompute_blocks(k.n_pairs) : 0;
  k.list = two_step ? c->fail_order.as<int32_t>() : nullptr;
  memcpy(S.hs + P.L.desc, &k, sizeof k);
  out->desc_pinned = reinterpret_cast<const SmallCall*>(S.hs_dev + P.L.desc);
  out->desc_dev = reinterpret_cast<const SmallCall*>(S.dp + P.L.desc);
  c->last_pairs = P.n_pairs;
  c->last_stream = S.s;
  c->have_last = true;
  c->stats.n_fallback = -1;
}

// ---- step 6: the callers compose.  A planned call that does not defer: staged, launched on `s`, finished. ----
int launch_call(DevCtx* c, const gklhip_batch* db, const CallPlan& P, double* out_dev, hipStream_t s) {
  if (P.n_pairs == 0) return GKLHIP_OK;
  StagedCall S;
  int rc;
  if ((rc = stage_call(c, db, P, out_dev, s, &S))) return rc;
  if ((rc = launch_prep(c, P, S))) return rc;
  if ((rc = reserve_carry(c, P, &S))) return rc;
  if (c->cfg.record_events != 0) HIP_TRY(hipEventRecord(c->ev[1], s));
  if (P.use_double) {
    rc = launch_all_double(c, P, S);
  } else {
    const FwdArgs<float> a = fwd_args<float>(c, P, S);
    if ((rc = launch_main_pass_f32(c, P, S, a))) return rc;
    rc = P.per_pair ? launch_per_pair(c, P, S, a) : launch_planned_fp64(c, P, S);
  }
  return rc ? rc : finish_call(c, P, S);
}
// The whole pass of a call that is never deferred (device-resident and multi-device callers, host calls with device
// finalisation) on stream `s`: `db` as for stage_call.
int run_device(DevCtx* c, const gklhip_batch* db, double* out_dev, int finalize_mode, hipStream_t s, Arrays where) {
  CallPlan P;
  plan_call(c, db, finalize_mode, where, false, call_load(false), &P);
  return launch_call(c, db, P, out_dev, s);
}

}  // namespace
