// Concurrent PDHMM cross calls share launches (GKL_HIP_PDHMM_COMBINE=1; off by default), and the process-wide counts of
// region calls and launch sets.  Part of the one HIP translation unit pdhmm_api.hip (included there behind
// pdhmm_multi_call.h, not compiled alone).
#pragma once
#include "pdhmm_multi_call.h"   // PdMultiRegion, pd_run_multi_locked

namespace {
// process-wide, per device (gklhip_pdhmm_combine_counts): region calls computed, region calls that shared a launch set
// with another, launch sets
constexpr int kPdCountDevices = 64;
std::atomic<int64_t> g_pd_counts[kPdCountDevices][3];
void pd_count(int device, int64_t calls, int64_t shared, int64_t sets) {
  if (device < 0 || device >= kPdCountDevices) return;
  g_pd_counts[device][0] += calls; g_pd_counts[device][1] += shared; g_pd_counts[device][2] += sets;
}

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
  PdMultiFit fit;   // of the tickets taken: taken[0 .. fit.count)
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
      auto take = [&](PdTicket* t) {
        taken[fit.count] = t;
        fit.take(t->q);
      };
      take(&me);
      PdTicket *prev = nullptr, *t = cb.head;
      while (t) {
        PdTicket* nx = t->next;
        const bool go = t == &me || (fit.count < kPdMaxRegions && mine(t) && fit.fits_with(t->q));
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
  if (const int n_taken = fit.count) {
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
}  // namespace
