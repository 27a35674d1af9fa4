// A single PDHMM call on the context's stream (pd_run_locked, at the end): uploads, job tables, launches, finish -- of
// the plan that pdhmm_call_plan.h made.  Host call or device-resident call, paired or cross layout.  Part of the one HIP
// translation unit pdhmm_api.hip (included there behind pdhmm_ctx.h, not compiled alone).
#pragma once
#include "pdhmm_ctx.h"

namespace {
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

// Where a device-resident call leaves its results (HBM of the context's device) and the caller's stream, behind whose
// work the call is ordered.
struct PdDeviceOut {
  double* out;        // [n_pairs] log10 likelihoods
  double* sums;       // [n_pairs] raw sums, or NULL
  hipStream_t after;  // NULL: HIP's default stream
};

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

// ---- step 1 is the plan (pdhmm_call_plan.h: PdCallPlan).  Step 2: the nine input arrays go to the device ----
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

// The single call's job tables, laid out by PdJobLayout (pd_table_copies lists them): through the pinned block in one
// copy while they fit it, else table by table.  Clears the status words and sets the full launch's list up.
int pd_stage_tables(gklhip_pdhmm_ctx* c, const PdCallPlan& p, const PdJobLayout& L) {
  const hipStream_t s = c->stream;
  const size_t n_general = (size_t)p.n_general;
  int rc;
  if ((rc = c->jobs.reserve(L.total + 256))) return rc;
  unsigned char* dj = c->jobs.as<unsigned char>();
  const bool staged_jobs = L.total <= kPdStageBytes;
  if (staged_jobs && (rc = c->stage_jobs.reserve(L.total + 256))) return rc;
  unsigned char* hj = c->stage_jobs.as<unsigned char>();
  size_t staged_hi = 0;  // bytes of the staging block in use
  auto put = [&](const PdTableCopy& t) {
    if (!t.bytes) return hipSuccess;
    if (staged_jobs) { memcpy(hj + t.offset, t.src, t.bytes); staged_hi = std::max(staged_hi, t.offset + t.bytes); return hipSuccess; }
    return hipMemcpyAsync(dj + t.offset, t.src, t.bytes, hipMemcpyHostToDevice, s);
  };
  const PdTableCopies tables = pd_table_copies(p, L);
  for (auto t = tables.begin(); t != tables.end() - 1; t++) HIP_TRY(put(*t));
  if (n_general > 0) {
    if (staged_jobs) { memset(hj + L.jf, 0, n_general); staged_hi = std::max(staged_hi, L.jf + n_general); }
    else HIP_TRY(hipMemsetAsync(dj + L.jf, 0, n_general, s));
  }
  HIP_TRY(hipMemsetAsync(c->misc.p, 0, 256, s));
#ifdef GKL_PD_PROF
  HIP_TRY(hipMemsetAsync(c->misc.as<char>() + 128 + 13 * 8, 0xff, 8, s));
  HIP_TRY(hipMemsetAsync(c->misc.as<char>() + 128 + 15 * 8, 0xff, 8, s));
#endif
  HIP_TRY(put(tables.back()));   // (the head of the full launch's list)
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
    return fail(GKLHIP_ERR_INVALID_ARG, "%s", kPdInputErrorText);
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
  if (status[kPdMiscInputError] != 0) return fail(GKLHIP_ERR_INVALID_ARG, "%s", kPdInputErrorText);
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

// dev == NULL: a host call, results to out_host; else a device-resident call (q.in_hbm), results to *dev.
int pd_run_locked(gklhip_pdhmm_ctx* c, const PdProblem& q_call, double* out_host, const PdDeviceOut* dev = nullptr) {
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
  const PdPlanSettings set = c->plan_settings();
  const PdInputLayout in((size_t)q.n_hap_items, (size_t)q.n_read_items, (size_t)q.max_hap_len, (size_t)q.max_read_len);
  PdCallPlan plan;
  pd_plan_slices(set, q, in, &plan);
  PdUploads up;
  if ((rc = up.start(c, q_call, in, plan))) return rc;
  clock.uploads = clock.ms();
  if (cross) pd_plan_cross_jobs(set, q, &plan.x); else pd_plan_paired_jobs(set, &c->plan_scratch, q, &plan);
  clock.jobs = clock.ms();
  // ---- routing: the hot launch (only the two in-place step loops, see pdhmm_fwd_kernel) takes every job without a
  // striped read and without a haplotype that has a base outside ACGTN (such columns need the byte-comparing step);
  // the rest -- rare -- go to a second launch of the full kernel.  Cross layout: the host looks at the (few)
  // haplotypes and orders them by kernel.  Listed jobs (paired layout: every job): routed on the device
  // (PdArgs::job_flags) -- a host scan of a haplotype per PAIR is ~100 MB for 400k pairs.
  if (cross) pd_plan_cross_routing(set, &c->plan_scratch, q, &plan.x);
  const int32_t n_haps = q.n_hap_items, n_tab = (int32_t)plan.x.n_tab_haps, n_clean = (int32_t)plan.x.n_clean_haps;
  c->last_routing[0] = cross ? n_tab : 0; c->last_routing[1] = cross ? n_clean - n_tab : 0; c->last_routing[2] = cross ? n_haps - n_clean : 0;
  clock.routing = clock.ms();
  if (!pd_plan_counts(set, q, &plan)) return fail(GKLHIP_ERR_INVALID_ARG, "too many jobs");
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
}  // namespace
