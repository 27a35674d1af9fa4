// The host-buffer call of one device (dev_compute_host: H2D, device pass, reference-exact host log10), the small-call combiner that launches
// the GATK-sized calls of several threads together, and the multi-region call that hands it whole sets (dev_compute_multi).
// Part of the ONE translation unit gkl_amd/csrc/pairhmm_api.hip, which includes it in the order it needs; not a stand-alone header.
#pragma once

namespace {

// Host threads of the reference-exact finalisation.  maxNumberOfThreads caps the OpenMP compute threads of the
// reference's OMP build (IntelPairHmm.cc:72-89; 1 is the default of PairHMMNativeArguments, IntelPairHmm.java:86-90);
// here the compute is on the device and the only host work it can cap is log10f/log10 over the results.  It IS a cap:
// a value >= 1 is honoured as given -- an explicit 1 means ONE finalisation thread per call (bench.py reports what
// that costs a 1.28 M-pair call in host_path.max_threads_1).  Only <= 0 (C ABI: "not set") picks a number here: the
// host-buffer calls in flight in this process then SHARE a budget of min(cores, 8) threads -- one call alone takes all
// of it, the two engines of a pipelined or twin-engine call half each, eight concurrent slots one each.
// GKL_HIP_FINALIZE_THREADS overrides both (per call).
struct HostCallInFlight {
  int share;
  HostCallInFlight() : share(g_host_calls_in_flight.fetch_add(1) + 1) {}
  ~HostCallInFlight() { g_host_calls_in_flight.fetch_sub(1); }
};
int finalize_threads(const DevCtx* c, int share) {
  const int env = g_env.finalize_threads;
  if (env > 0) return env;
  const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
  int threads = c->cfg.max_threads;
  if (threads <= 0) threads = std::max(1, std::min(hw, 8) / std::max(1, share));
  return std::max(1, std::min(threads, 64));
}

// ---- small host-buffer calls of several threads: combined launches ----
// The device executes the kernels of about four hardware queues at a time (tools/ubench_launch.hip: 16 threads with a
// stream each get 4 x the kernel rate of one, not 16 x), so GATK-sized calls from many threads queue up behind each
// other however many streams they use.  A call that arrives while others are in flight therefore waits for a flight
// slot, and the thread that gets the slot launches ALL waiting calls in one set of three kernels (prep_multi_kernel,
// fwd_stream_multi_kernel, pair_policy_multi_kernel: a block finds its call through block offsets in the kernel
// arguments).  A call that finds a free slot and nobody waiting goes out on its own stream exactly as before.
constexpr int kFlightSlots = 4;
// A set of gklhip_compute_multi_device, whose regions' arrays and outputs lie in HBM: what its launches wait for, and its
// way out (finalize_words_multi_kernel behind the last launch).  NULL everywhere else.
struct ResidentSet {
  hipEvent_t after;     // recorded on the caller's stream: the set's stream waits for it before prep_multi_kernel
  int mode;             // GKLHIP_FINALIZE_DEVICE_F64 or GKLHIP_FINALIZE_DEVICE_REF32
  int32_t* fallbacks;   // [kMultiMax], as the device sees them: each region's number of fp64 words
};
struct SmallCombiner {
  struct Ticket {
    const SmallLaunch* sl = nullptr;
    int state = 0;  // 0 queued, 4 taken by a leader, 1 launched (wait for `ev`), 2 failed
    hipEvent_t ev = nullptr;
    int rc = GKLHIP_OK;
    std::string err;
    int64_t t_in = 0;
  };
  struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    bool busy = false;
  };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Ticket*> queue;
  Slot slot[kFlightSlots];
  int device = 0;
  bool streams_made = false;       // the flight streams are created by the first COMBINED launch (make_streams)
  int flights = 0;
  int mid_flights = 0;             // ... of which sets of mid-size calls (at most kMidFlights from the queue: combine_admits)
  int max_flights = 4;   // (r05, alternating on one box: 4 callers 698-723 -> 740-757 GCUPS, 16 callers 1941-2010 -> 2127-2133 with four instead of three)
  int min_batch = 0;               // 0: by load (see run())
  int64_t batch_wait_ns = 50000;
  int64_t n_calls = 0, n_combined = 0, n_launch_sets = 0;  // diagnostics (gklhip_small_call_counts)
  int64_t ns_queued = 0, ns_launch = 0, ns_sync = 0;
  std::atomic<int64_t> ns_stage{0}, ns_run{0}, ns_finalize{0};  // per call, outside the lock
  static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  // The flight streams, created together -- the runtime deals streams round-robin onto the process's hardware queues, so
  // consecutive ones land on different queues and the sets in flight really run side by side -- but only when two calls
  // first meet: a process with ONE caller (a HaplotypeCaller JVM) never needs them, and every stream it does not create is a
  // hardware queue the device's scheduler does not have to rotate in -- with sixteen such processes on one GPU that is the
  // difference between 0.9 and 1.5 TCUPS (docs/NOTES.md 48).  Called with the combiner's lock held.
  int64_t last_made_or_used_ns = 0;   // when the flight streams were made / last carried a set
  // The flight streams go again when nothing has been combined for `idle_ns` and nothing is in the air (an idle process
  // should not hold their hardware queues: gklhip_release_idle); the next two calls that meet make them again.
  int release_streams(int64_t idle_ns) {
    std::lock_guard<std::mutex> l(mu);
    if (!streams_made || flights > 0 || !queue.empty() || now_ns() - last_made_or_used_ns < idle_ns) return 0;
    for (auto& sl : slot) if (sl.busy) return 0;
    int prev = 0, n = 0;
    const bool have_dev = hipGetDevice(&prev) == hipSuccess;
    if (hipSetDevice(device) == hipSuccess) {
      for (auto& sl : slot) {
        if (sl.stream) { (void)hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); sl.stream = nullptr; n++; }
        if (sl.ev) { (void)hipEventDestroy(sl.ev); sl.ev = nullptr; }
      }
      streams_made = false;
    }
    if (have_dev) (void)hipSetDevice(prev);
    return n;
  }
  void make_streams() {
    last_made_or_used_ns = now_ns();
    if (streams_made) return;
    streams_made = true;
    int prev = 0;
    const bool have_dev = hipGetDevice(&prev) == hipSuccess;
    if (hipSetDevice(device) == hipSuccess) {
      for (auto& sl : slot)
        if (hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) {
          sl.stream = nullptr;  // (a set that gets this slot reports the failure)
          (void)hipGetLastError();
        }
    }
    if (have_dev) (void)hipSetDevice(prev);
  }

  int launch_single(const SmallCall& k, hipStream_t s, bool alone) {
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)k.prep_grid), dim3(kPrepBlock), 0, s, k.prep);
    int rc;
    if (k.kind == kSmallDouble) {
      rc = launch_pair_f64(k.d, k.q, k.rows, k.fma, k.n_pairs, s);
    } else if (k.fused) {
      rc = launch_pair_fused(k.f, k.d, k.q, k.rows, k.fma, k.n_pairs, s, alone && k.speculate);
    } else {
      launch_main_f32(k.f, k.rpl_main, k.fma, k.main_blocks, s);
      rc = launch_pair_policy(k.d, k.q, k.rows, k.fma, k.n_pairs, s);
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return GKLHIP_OK;
  }
  // One set of launches for calls[0 .. n) (every call of a set is of one kind: a leader only takes calls like its own, a
  // multi call cuts its sets by kind).  The kernel forms are the launchers' business (pairhmm_device_pass.h).  On stream `s`;
  // `done` (may be NULL) is recorded behind the last launch.
  int launch_multi(const SmallLaunch* const* calls, int n, int fma, hipStream_t s, hipEvent_t done, const ResidentSet* resident = nullptr) {
    // a launch's table: each call's descriptor (prep reads the pinned one) and where its `blocks` blocks begin
    auto set_of = [&](const SmallCall* SmallLaunch::*desc, int32_t SmallCall::*blocks) {
      MultiArgs m{};
      int32_t per_call[kMultiMax];
      for (int i = 0; i < n; i++) { m.call[i] = calls[i]->*desc; per_call[i] = calls[i]->call.*blocks; }
      m.n = n;
      multi_begin(per_call, n, m.begin);
      return m;
    };
    const auto dev = &SmallLaunch::desc_dev;
    int rows = kPairTiers[0];   // of the set's widest call
    for (int i = 0; i < n; i++) rows = std::max(rows, calls[i]->call.rows);
    const MultiArgs mp = set_of(&SmallLaunch::desc_pinned, &SmallCall::prep_grid);
    if (resident) HIP_TRY(hipStreamWaitEvent(s, resident->after, 0));
    hipLaunchKernelGGL(prep_multi_kernel, set_grid(mp), dim3(kPrepBlock), 0, s, mp);
    int rc = GKLHIP_OK;
    switch (calls[0]->call.kind) {
      case kSmallTwoStep: {   // mid-size regions (of a multi call, or of concurrent callers with the mid-size switch on): the packed fp32 pass, then the policy in two launches
        launch_stream_f32_set(set_of(dev, &SmallCall::main_blocks), fma, s);
        const MultiArgs mg = set_of(dev, &SmallCall::flag_grid);
        hipLaunchKernelGGL(pair_flag_multi_kernel, set_grid(mg), dim3(kFlagBlock), 0, s, mg);
        rc = launch_pair_set(PairFamily::kRecompute, set_of(dev, &SmallCall::recompute_grid), rows, fma, s);
      } break;
      case kSmallDoubleStream: {   // mid-size regions of a double-precision context: the packed fp64 pass, then its packed words
        launch_stream_f64_set(set_of(dev, &SmallCall::main_blocks), fma, s);
        const MultiArgs mg = set_of(dev, &SmallCall::flag_grid);
        hipLaunchKernelGGL(finalize64_multi_kernel, set_grid(mg), dim3(kFlagBlock), 0, s, mg);
      } break;
      case kSmallDouble:   // calls of double-precision contexts: one launch, a block per pair, every pair in fp64
        rc = launch_pair_set(PairFamily::kF64, set_of(dev, &SmallCall::n_pairs), rows, fma, s);
        break;
      case kSmallFused:    // (exactly the calls with `fused` set: small_call_kind)
        rc = launch_pair_set(PairFamily::kFused, set_of(dev, &SmallCall::n_pairs), rows, fma, s);
        break;
      default:             // kSmallOneLaunch: the one-launch policy behind the packed fp32 pass
        launch_stream_f32_set(set_of(dev, &SmallCall::main_blocks), fma, s);
        rc = launch_pair_set(PairFamily::kPolicy, set_of(dev, &SmallCall::n_pairs), rows, fma, s);
    }
    if (rc) return rc;
    if (resident) {   // the regions' packed words, in their own output arrays, become doubles there: a thread per pair
      MultiArgs mf = set_of(dev, &SmallCall::n_pairs);
      int32_t blocks[kMultiMax];
      for (int i = 0; i < n; i++) blocks[i] = multi_flag_blocks(calls[i]->call.n_pairs);
      multi_begin(blocks, n, mf.begin);
      hipLaunchKernelGGL(finalize_words_multi_kernel, set_grid(mf), dim3(kFlagBlock), 0, s, mf, resident->mode, resident->fallbacks);
    }
    HIP_TRY(hipGetLastError());
    if (done) HIP_TRY(hipEventRecord(done, s));
    return GKLHIP_OK;
  }

  // One set into the air and back: takes a free flight slot (the caller holds the lock and has found flights < max_flights),
  // launches calls[0 .. n) -- one call on the caller's own stream exactly as a lone call always went, several in one set of
  // launches on the slot's stream --, reports the launch to the owners of calls[1 ..] (`others`; NULL: all n are the
  // caller's own, the regions of a multi call) and waits for the end.  Returns with the lock released.
  // ONE mid-size call has no single-call launch form here: it leaves as a set of one through launch_multi, on the caller's
  // own stream like any lone call -- on the slot's stream it made the four flight streams at a lone caller's first call, which
  // a one-caller process should never hold (make_streams), and 100 x 10 callers that came later ran a quarter slower
  // (docs/NOTES.md 75).
  // A `resident` set (gklhip_compute_multi_device) of one region leaves through launch_multi as well: its way out is the
  // set's.
  int fly(std::unique_lock<std::mutex>& l, const SmallLaunch* const* calls, int n, hipStream_t own_stream, Ticket* const* others, int64_t t_lead,
          const ResidentSet* resident = nullptr) {
    int si = 0;
    while (slot[si].busy) si++;
    Slot& sl = slot[si];
    sl.busy = true;
    const bool alone = flights == 0 && queue.empty() && n == 1;   // no other small call on the device or waiting for it
    const bool mid = small_kind_is_mid(calls[0]->call.kind);
    const bool own = n == 1;                                      // on the caller's own stream
    flights++;
    if (mid) mid_flights++;
    n_launch_sets++;
    if (n > 1) n_combined += n;
    int rc = GKLHIP_OK;
    if (!own) make_streams();
    if (!own && !sl.stream) rc = fail(GKLHIP_ERR_HIP, "no stream for combined small calls");
    l.unlock();
    if (rc == GKLHIP_OK)
      rc = !own ? launch_multi(calls, n, calls[0]->call.fma, sl.stream, sl.ev, resident)
           : mid || resident ? launch_multi(calls, 1, calls[0]->call.fma, own_stream, nullptr, resident) : launch_single(calls[0]->call, own_stream, alone);
    const std::string err = rc == GKLHIP_OK ? std::string() : g_err;
    const int64_t t_launched = now_ns();
    // a launch that failed part-way may have left kernels on the stream that still read the calls' staging blocks and
    // write their result buffers: drain it BEFORE any of the calls is told about the failure (and returns to a caller
    // that is free to reuse those buffers)
    if (rc != GKLHIP_OK) { (void)(own ? hipStreamSynchronize(own_stream) : hipStreamSynchronize(sl.stream)); (void)hipGetLastError(); }
    if (n > 1 && others) {
      l.lock();
      // (the others wait on the set's event themselves; letting them sleep until this thread has seen the end
      //  measured the same)
      for (int i = 1; i < n; i++) {
        Ticket* o = others[i - 1];
        o->rc = rc; o->err = err; o->ev = sl.ev;
        o->state = rc == GKLHIP_OK ? 1 : 2;
      }
      cv.notify_all();
      l.unlock();
    }
    hipError_t e = hipSuccess;
    if (rc == GKLHIP_OK) e = own ? hipStreamSynchronize(own_stream) : hipEventSynchronize(sl.ev);
    l.lock();
    {
      const int64_t t_end = now_ns();
      ns_launch += t_launched - t_lead; ns_sync += t_end - t_launched;
    }
    sl.busy = false;  // (the event is recorded again only from here on: a late waiter of this flight then waits a little longer)
    flights--;
    if (mid) mid_flights--;
    cv.notify_all();
    l.unlock();
    if (rc != GKLHIP_OK) { g_err = err; return rc; }
    if (e != hipSuccess) return fail(GKLHIP_ERR_HIP, "%s (combined small calls)", hipGetErrorString(e));
    return GKLHIP_OK;
  }

  // The staged regions of one gklhip_compute_multi call that share a set (at most kMultiMax, of one kind and arithmetic
  // mode), to completion: the set waits for a flight slot like any leader and leaves through the same launches, but it is
  // the caller's own from end to end -- it never enters the queue, so no other leader sees its regions, it takes nobody
  // else's tickets, and it never waits for company.  One region alone goes out on `own_stream` as a lone call does.
  int run_set(const SmallLaunch* const* calls, int n, hipStream_t own_stream, const ResidentSet* resident = nullptr) {
    const int64_t t_in = now_ns();
    std::unique_lock<std::mutex> l(mu);
    n_calls += n;
    cv.wait(l, [&] { return flights < max_flights; });
    const int64_t t_lead = now_ns();
    ns_queued += (t_lead - t_in) * n;
    return fly(l, calls, n, own_stream, nullptr, t_lead, resident);
  }

  // Runs one staged call to completion (its packed words are in the caller's pinned result buffer on return).
  int run(const SmallLaunch& mine, hipStream_t own_stream) {
    Ticket t;
    t.sl = &mine;
    const int64_t t_in = t.t_in = now_ns();
    const auto as_combine_call = [](const SmallLaunch& x) { return CombineCall{x.call.kind, x.call.fma, (int64_t)x.call.n_pairs}; };
    const bool mid = small_kind_is_mid(mine.call.kind);
    std::unique_lock<std::mutex> l(mu);
    n_calls++;
    queue.push_back(&t);
    while (t.state == 0 || t.state == 4) {
      // (a mid-size call also waits while kMidFlights mid-size sets are in the air, whatever slots are free)
      if (t.state == 4 || !combine_admits(mid, flights, mid_flights, max_flights)) { cv.wait(l); continue; }
      // Under load (other sets are in the air) a set is worth more the more calls it carries -- its kernels take as long
      // as their slowest pair whatever their size -- so a would-be leader that finds fewer than `min_batch` calls waiting
      // gives the others `batch_wait_ns` to arrive (GKL_HIP_COMBINE_MIN / GKL_HIP_COMBINE_WAIT_US; 1 / 0 = lead at once).
      // The number to wait for follows the load: a quarter of the host calls inside the library right now, at most 4
      // (16 callers: 4, 8: 2, up to 7: none -- with few callers the wait only adds latency; measured with 50 us: 16 callers
      // 1.42 -> 2.14 TCUPS, while a fixed minimum of 4 cost 4 callers 0.90 -> 0.71).
      // `queue.size()` counts every waiting call, of whatever kind: with the mid-size switch on, the mid-size tickets
      // that combine_admits holds back count too, so a small would-be leader may then leave with less company of its own
      // kind than without them (not measured apart; the mixed run of docs/NOTES.md 75 has both kinds waiting).
      {
        const int want = min_batch > 0 ? min_batch : std::min(4, g_host_calls_in_flight.load(std::memory_order_relaxed) / 4);
        if (flights > 0 && (int)queue.size() < want && now_ns() - t_in < batch_wait_ns) {
          cv.wait_for(l, std::chrono::microseconds(5));
          continue;
        }
      }
      // lead: this call first, then the waiting calls of the same arithmetic mode and kind (a set never mixes the fused
      // and the one-launch fp32 calls, nor either with the calls of a double-precision context, nor small calls with
      // mid-size ones), a set of mid-size calls within its pair cap: the rule is CombinePick's (pairhmm_multi_sets.h)
      const int64_t t_lead = now_ns();
      ns_queued += t_lead - t_in;
      const SmallLaunch* calls[kCombineMax];
      Ticket* others[kCombineMax];   // the owners of calls[1 ..]
      static thread_local std::vector<CombineCall> waiting;   // (what the rule reads of the queue, in arrival order)
      waiting.clear();
      int me = 0;
      for (Ticket* o : queue) {
        if (o == &t) me = (int)waiting.size();
        waiting.push_back(as_combine_call(*o->sl));
      }
      int32_t picked[kCombineMax];
      const int n = combine_pick(waiting.data(), (int)waiting.size(), me, mid, picked);
      calls[0] = &mine;
      for (int i = 1; i < n; i++) {
        Ticket* o = queue[(size_t)picked[i]];
        o->state = 4;  // taken: its owner keeps sleeping until this thread reports the launch (or the end)
        ns_queued += t_lead - o->t_in;
        others[i - 1] = o;
        calls[i] = o->sl;
      }
      // (this call and the taken ones leave the queue; the rest keep their order)
      queue.erase(std::remove_if(queue.begin(), queue.end(), [&](const Ticket* o) { return o == &t || o->state == 4; }), queue.end());
      return fly(l, calls, n, own_stream, others, t_lead);
    }
    l.unlock();
    if (t.state == 2) { g_err = t.err; return t.rc; }
    if (t.state == 1) HIP_TRY(hipEventSynchronize(t.ev));
    return GKLHIP_OK;
  }
};
SmallCombiner* small_combiner(int device) {
  static std::mutex mu;
  static std::vector<SmallCombiner*> all;
  std::lock_guard<std::mutex> l(mu);
  if ((int)all.size() <= device) all.resize((size_t)device + 1, nullptr);
  if (!all[(size_t)device]) {
    SmallCombiner* k = all[(size_t)device] = new SmallCombiner();  // lives as long as the process (a handful of streams and events)
    k->device = device;   // (its flight streams: SmallCombiner::make_streams, when two calls first meet)
    if (const char* v = getenv("GKL_HIP_EAGER_STREAMS")) if (atoi(v) >= 7) k->make_streams();   // A/B: the r04 arrangement
    if (const char* v = getenv("GKL_HIP_COMBINE_FLIGHTS")) all[(size_t)device]->max_flights = std::max(1, std::min(kFlightSlots, atoi(v)));
    if (const char* v = getenv("GKL_HIP_COMBINE_MIN")) all[(size_t)device]->min_batch = std::max(0, std::min(kCombineMax, atoi(v)));
    if (const char* v = getenv("GKL_HIP_COMBINE_WAIT_US")) all[(size_t)device]->batch_wait_ns = (int64_t)std::max(0, atoi(v)) * 1000;
  }
  return all[(size_t)device];
}
int64_t one_pass_min() { return g_env.finalize_min > 0 ? g_env.finalize_min : 8192; }
int dev_compute_host_impl(DevCtx* c, const gklhip_batch* hb, double* out_host) {
  const int64_t n_pairs = (int64_t)hb->n_reads * hb->n_haps;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int rc;
  const Arrays where = inputs_inline(hb) ? Arrays::kHostInline : Arrays::kDevice;
  gklhip_batch db = *hb;
  if (where == Arrays::kDevice) {
    // H2D of the six byte arrays (one allocation, 256-byte aligned sub-buffers)
    if ((rc = c->batch_dev.reserve(six_arrays_bytes(hb)))) return rc;
    unsigned char* d = c->batch_dev.as<unsigned char>();
    if (c->have_call_done && c->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->call_done, 0));
    const size_t stride = align_up((size_t)hb->read_off[hb->n_reads]);
    if ((rc = copy_six_arrays(*hb, stride, [d, s](size_t at, const uint8_t* src, size_t n) -> int { HIP_TRY(hipMemcpyAsync(d + at, src, n, hipMemcpyHostToDevice, s)); return GKLHIP_OK; }))) return rc;
    db = batch_at(*hb, d, stride);
  }
  const int mode = c->cfg.finalize;
  // The kernels store their results straight into pinned host memory (posted writes over PCIe, 8 bytes per pair):
  // a copy-engine transfer behind the last kernel costs a small call ~15 us of queue hand-offs, and in a big call
  // the runtime's copy kernel for the early results slowed the fp64 pass it was meant to overlap with by a third.
  if ((rc = c->res_pin.reserve((size_t)n_pairs * 8))) return rc;
  double* pin_out = nullptr;
  {
    void* p = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&p, c->res_pin.p, 0));
    pin_out = static_cast<double*>(p);
  }
  if (finalizes_on_device(mode)) {
    if ((rc = run_device(c, &db, pin_out, mode, s, where))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(out_host, c->res_pin.p, (size_t)n_pairs * 8);
    return GKLHIP_OK;
  }
  // Reference-exact finalisation on the host: one packed 8-byte word per pair.  The fp32 results are final as soon
  // as the policy has run, so in a big call the host finalises them WHILE the fp64 recomputation pass runs; only the
  // recomputed pairs are left for after the last kernel (their words are rewritten in place by finalize64_kernel;
  // the early pass skips every word that is not fp32-tagged, whatever it holds at that moment).
  const HostCallInFlight in_flight;
  const int threads = finalize_threads(c, in_flight.share);
  HostFinalizer fin;
  // (a context with an asynchronous device-resident call still in flight keeps the stream-ordered path)
  const bool may_defer = deferral_offered(where) && (!c->have_call_done || hipEventQuery(c->call_done) == hipSuccess);
  (void)hipGetLastError();  // (hipErrorNotReady of the query)
  const int64_t t_call = SmallCombiner::now_ns();
  CallPlan P;
  plan_call(c, &db, kModePacked, where, may_defer, call_load(may_defer), &P);
  // a mid-size region of a context with the mid-size switch on: staged as a multi call stages one (MultiCallOps::stage), and into the
  // combiner with the like regions of whoever else is calling right now
  const bool mid = !P.defers && may_defer && mid_call_combines(c, P);
  if (mid) P.defers = true;
  if (P.defers) {   // staged and described here, launched by the combiner
    StagedCall S;
    SmallLaunch small;
    if ((rc = stage_call(c, &db, P, pin_out, s, &S))) return rc;
    if (mid && !P.use_double && (rc = c->fail_order.reserve((size_t)P.n_pairs * 4))) return rc;   // the list of its flagged pairs
    describe_small_call(c, P, S, &small);
    SmallCombiner* k = small_combiner(c->device);
    const int64_t t_staged = SmallCombiner::now_ns();
    if ((rc = k->run(small, s))) return rc;
    const int64_t t_done = SmallCombiner::now_ns();
    c->stats.n_fallback = fin.all(&c->workers, c->res_pin.as<uint64_t>(), out_host, n_pairs, threads, one_pass_min());
    k->ns_stage.fetch_add(t_staged - t_call, std::memory_order_relaxed);
    k->ns_run.fetch_add(t_done - t_staged, std::memory_order_relaxed);
    k->ns_finalize.fetch_add(SmallCombiner::now_ns() - t_done, std::memory_order_relaxed);
    return GKLHIP_OK;
  }
  if ((rc = launch_call(c, &db, P, pin_out, s))) return rc;  // records policy_done
  if (c->cfg.use_double || n_pairs <= kOnePassPairs) {
    // all-fp64 mode, or a GATK-sized call (the fp64 stage of a region without underflowed pairs -- the usual case --
    // is two launches that find nothing to do): one pass over the words once the last kernel is done
    // (from 8192 pairs on spread over the workers: a region of 400 reads x 40 haplotypes is 16 000 log10's = 0.08 ms on one
    //  thread, a fifth of the call -- 400 x 40: 0.416 -> 0.378 ms; at 4096 the hand-off costs a 150 x 30 call more than it
    //  saves: 0.236 -> 0.245; tools/mid_finalize_ab.py)
    HIP_TRY(hipStreamSynchronize(s));
    c->stats.n_fallback = fin.all(&c->workers, c->res_pin.as<uint64_t>(), out_host, n_pairs, threads, one_pass_min());
    return GKLHIP_OK;
  }
  HIP_TRY(hipEventSynchronize(c->policy_done));
  fin.early(&c->workers, c->res_pin.as<uint64_t>(), out_host, n_pairs, threads);
  HIP_TRY(hipStreamSynchronize(s));
  c->stats.n_fallback = fin.late(&c->workers, c->res_pin.as<uint64_t>(), out_host, threads);
  return GKLHIP_OK;
}

// Host buffers in, host doubles out on one device.  An error return must not leave copies from the caller's
// arrays (or into them) in flight: drain the streams first.
int dev_compute_host(DevCtx* c, const gklhip_batch* hb, double* out_host) {
  // ... and neither must a C++ exception on its way to the entry point's guarded() (bad_alloc from a plan vector, a
  // finalisation worker's rethrow): the same drain, then the exception goes on
  auto drain = [c]() noexcept {
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->upload_stream) (void)hipStreamSynchronize(c->upload_stream);
    (void)hipGetLastError();
  };
  int rc;
  try {
    rc = dev_compute_host_impl(c, hb, out_host);
  } catch (...) {
    drain();
    throw;
  }
  if (rc != GKLHIP_OK) {
    const std::string keep = g_err;
    drain();
    g_err = keep;
  }
  return rc;
}

// ---- several region calls in one set of launches (gklhip_compute_multi, gklhip_compute_multi_device) ----
// A region of a multi call: checked by the caller (validate, at least one pair, an output array).
struct MultiRegion {
  const gklhip_batch* hb = nullptr;
  double* out = nullptr;
  int index = 0;            // its place in the caller's arrays
  int rc = GKLHIP_OK;
  std::string err;
  bool alone = false;       // does not qualify for a shared set: the caller runs it through the single-call path
  int lane = -1;            // the staging lane that holds its raw sums after the call (-1: none)
  gklhip_stats stats;
};

// The device side of multi_call_drive (pairhmm_multi_call.h, which decides everything): a region is planned, staged and
// described on a lane of the context exactly as a single call stages itself (plan_call, stage_call, describe_small_call),
// a set leaves through the combiner's launches (run_set), and each region's packed words are finalised on the host as a
// single call's are.  The regions that qualify are the ones the single call would defer, and the mid-size ones
// (mid_call_shares; a double-precision context's: double_mid_shares).
// `resident` (gklhip_compute_multi_device: the regions' arrays and outputs lie in HBM) differs in three places: a region's
// arrays are kRegionInHbm (within kSmallBatchBytes they stand where "inputs inline" stands, and the context's device
// finalisation does not turn the region away); its packed words go into its own output array; and the set waits for the
// caller's stream and ends with finalize_words_multi_kernel, which also leaves the region's fallback count -- no host
// log10, no res_pin.
struct MultiCallOps {
  DevCtx* c;
  std::vector<DevCtx*>& lanes;
  std::vector<MultiRegion>& R;
  const ResidentSet* resident;
  int threads;                      // of the host finalisation
  std::vector<SmallLaunch> staged;  // by lane
  CallPlan last, held;
  bool last_mid = false, held_mid = false;

  MultiPlanned plan(int i, int li) {
    const gklhip_batch* hb = R[(size_t)i].hb;
    // (inputs_inline: the size limit, of host arrays and of arrays in HBM alike)
    const Arrays where = !inputs_inline(hb) ? Arrays::kDevice : resident ? Arrays::kRegionInHbm : Arrays::kHostInline;
    if (!deferral_offered(where) || (!resident && finalizes_on_device(c->cfg.finalize))) return {GKLHIP_OK, kMultiNone, 0, false};
    while ((int)lanes.size() <= li) {   // lanes are made on first use
      DevCtx* ln = nullptr;
      if (const int rc = lane_init(c, &ln)) return {rc, kMultiNone, 0, false};
      lanes.push_back(ln);
    }
    DevCtx* ln = lanes[(size_t)li];
    plan_call(ln, hb, kModePacked, where, true, call_load(true), &last);
    last_mid = !last.defers && (mid_call_shares(ln, last) || double_mid_shares(ln, last));
    if (!last.defers && !last_mid) return {GKLHIP_OK, kMultiNone, 0, false};
    last.defers = true;   // (a mid-size region too is staged for the combiner: see stage_call)
    return {GKLHIP_OK, last_mid ? kMultiMid : kMultiSmall, (uint8_t)small_call_kind(last), last.use_double};
  }
  void hold() { held = last; held_mid = last_mid; }
  int stage(int i, int li, bool from_held) {
    MultiRegion& r = R[(size_t)i];
    DevCtx* ln = lanes[(size_t)li];
    const CallPlan& P = from_held ? held : last;
    int rc;
    void* pin_out = r.out;   // (resident: the packed words go where the doubles will be)
    if (!resident) {
      if ((rc = ln->res_pin.reserve((size_t)r.hb->n_reads * (size_t)r.hb->n_haps * 8))) return rc;
      if (hipHostGetDevicePointer(&pin_out, ln->res_pin.p, 0) != hipSuccess) { (void)hipGetLastError(); return ::fail(GKLHIP_ERR_HIP, "hipHostGetDevicePointer failed"); }
    }
    StagedCall S;   // (the regions of a multi call are staged on lanes that have no stream of their own)
    if ((rc = stage_call(ln, r.hb, P, static_cast<double*>(pin_out), c->stream, &S))) return rc;
    if ((from_held ? held_mid : last_mid) && !P.use_double && (rc = ln->fail_order.reserve((size_t)P.n_pairs * 4))) return rc;   // the list of its flagged pairs
    describe_small_call(ln, P, S, &staged[(size_t)li]);
    return GKLHIP_OK;
  }
  int run(const int* members, int m) {
    const SmallLaunch* calls[kMultiMax];
    for (int j = 0; j < m; j++) calls[j] = &staged[(size_t)R[(size_t)members[j]].lane];
    if (resident) std::fill_n(c->multi_fallbacks.as<int32_t>(), kMultiMax, -1);
    return small_combiner(c->device)->run_set(calls, m, c->stream, resident);
  }
  void take(int i, int j) {
    MultiRegion& r = R[(size_t)i];
    DevCtx* ln = lanes[(size_t)r.lane];
    if (resident) ln->stats.n_fallback = c->multi_fallbacks.as<int32_t>()[j];
    else ln->stats.n_fallback = HostFinalizer().all(&c->workers, ln->res_pin.as<uint64_t>(), r.out, ln->stats.n_pairs, threads, one_pass_min());
    r.stats = ln->stats;
  }
  void fail(int i, int rc) { R[(size_t)i].rc = rc; R[(size_t)i].err = g_err; }
};

// The return value is for what stops the whole call before any region is touched; a failure later is a region's own (`rc`,
// `err`).  `resident_stream`: NULL for host regions; else the caller's stream, which every set waits for (an event on it).
int dev_compute_multi(DevCtx* c, std::vector<DevCtx*>& lanes, std::vector<MultiRegion>& R, const hipStream_t* resident_stream) {
  HIP_TRY(hipSetDevice(c->device));
  const HostCallInFlight in_flight;
  ResidentSet rset{};
  if (resident_stream) {
    if (!c->multi_in) HIP_TRY(hipEventCreateWithFlags(&c->multi_in, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->multi_in, *resident_stream));
    if (const int rc = c->multi_fallbacks.reserve(kMultiMax * sizeof(int32_t))) return rc;
    void* p = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&p, c->multi_fallbacks.p, 0));
    rset.after = c->multi_in;
    rset.mode = c->cfg.finalize == GKLHIP_FINALIZE_DEVICE_REF32 ? GKLHIP_FINALIZE_DEVICE_REF32 : GKLHIP_FINALIZE_DEVICE_F64;
    rset.fallbacks = static_cast<int32_t*>(p);
  }
  MultiCallOps ops{c, lanes, R, resident_stream ? &rset : nullptr, finalize_threads(c, in_flight.share), std::vector<SmallLaunch>((size_t)kMultiMax), {}, {}};
  int32_t owner[kMultiMax];   // by lane: the region whose raw sums it holds
  std::fill_n(owner, kMultiMax, -1);
  multi_call_drive(R.data(), (int)R.size(), owner, ops);
  return GKLHIP_OK;
}

}  // namespace
