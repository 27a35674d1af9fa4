// Several PDHMM region calls in one set of launches (pd_run_multi_locked, at the end): the host form
// (gklhip_pdhmm_compute_cross_multi: arrays and results on the host) and the device form (_cross_multi_device: the byte
// arrays and the results in HBM).  Plan (pdhmm_call_plan.h: PdMultiPlan), stage the inputs, stage the job tables, launch,
// finish: the two forms differ in how the inputs are staged and in the finish only.  Part of the one HIP translation unit
// pdhmm_api.hip (included there behind pdhmm_single_call.h, not compiled alone).
#pragma once
#include "pdhmm_single_call.h"   // pd_input_arrays, pd_common_args, pd_launch_cross_jobs, pd_launch_tail, pd_finalise

namespace {
struct PdMultiRegion {
  PdProblem q;
  double* out;                          // host form: a host array; device form: HBM
  double* sums_out = nullptr;           // device form: HBM, or NULL
  int32_t flag = 0;                     // out: the region's input-error flag (PDHMM_INPUT_DATA_ERROR)
  int32_t routing[3] = {0, 0, 0};       // out: its haplotypes by kernel
};

// ---- step 1 is the plan (pd_multi_plan).  Step 2: the inputs go to the device, every region's rows at the common strides ----
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

// The regions' plans, shifted to the concatenated indices (pd_multi_fill_tables), in one pinned block and one copy;
// clears the status words.
int pd_multi_stage_tables(gklhip_pdhmm_ctx* c, const PdMultiPlan& p, const PdMultiJobLayout& L) {
  int rc;
  if ((rc = c->jobs.reserve(L.total + 256)) || (rc = c->stage_jobs.reserve(L.staged_total + 256))) return rc;
  unsigned char* hj = c->stage_jobs.as<unsigned char>();
  pd_multi_fill_tables(p, L, hj);
  HIP_TRY(hipMemcpyAsync(c->jobs.p, hj, L.staged_total, hipMemcpyHostToDevice, c->stream));
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
// inputs: PdMultiFit) as ONE problem.  after == NULL: the host form; else the device form (R[k].q.in_hbm), ordered behind
// *after (a NULL stream: HIP's default stream).  The device form stages its inputs before it plans: the planners read the
// haplotype bytes that come back with them.  The return value is the status of the launch set (a HIP failure fails every
// region); R[k].flag != 0: region k had a negative quality (PDHMM_INPUT_DATA_ERROR), its results are not written.
int pd_run_multi_locked(gklhip_pdhmm_ctx* c, std::vector<PdMultiRegion>& R, const hipStream_t* after = nullptr) {
  HIP_TRY(hipSetDevice(c->device));
  const bool device = after != nullptr;
  std::vector<PdProblem> Q(R.size());
  for (size_t k = 0; k < R.size(); k++) Q[k] = R[k].q;
  const PdMultiShape sh(Q);
  const PdInputLayout in = sh.layout();
  PdMultiPlan plan;
  int rc;
  if (device && (rc = pd_multi_stage_inputs_device(c, R, in, *after, &Q))) return rc;
  pd_multi_plan(c->plan_settings(), &c->plan_scratch, Q, sh, &plan);
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
}  // namespace
