// Test infrastructure (CPU): the nine functions of include/gkl_hip_pdhmm.h that gkl_amd/csrc/pairhmm_server.cpp resolves
// at run time, WITHOUT a device and without any PDHMM arithmetic, as a shared library of its own that the server is
// pointed to with GKL_HIP_PDHMM_LIB (tests/test_pdhmm_server_cpu.py).
//
// "Likelihood" of a pair = position-weighted checksum of its read's five arrays * 2^-20 + a checksum of its haplotype's
// two arrays, both up to their lengths, both lengths, fma_mode, tail_mode and, in the cross layout, ref_batch_pairs and
// the pair's index: a wrong offset, stride, mode or layout changes the value (Python twin: stub_pd_expected in the test).
//   STUB_DELAY_US=n   every compute call sleeps n microseconds first
// A negative gcp byte inside a read's length fails the call like the product does.
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <thread>

#include "../../include/gkl_hip_pairhmm.h"
#include "../../include/gkl_hip_pdhmm.h"

namespace {
thread_local const char* t_err = "";
constexpr const char* kInvalid = "Error while calculating pdhmm. Input arrays aren't valid.";

void delay() {
  static const long us = [] { const char* v = getenv("STUB_DELAY_US"); return v ? atol(v) : 0L; }();
  if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

uint64_t read_sum(const int8_t* const a[5], int64_t row, int32_t stride, int64_t n, bool* negative_gcp) {
  uint64_t s = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t at = row * stride + i;
    if (a[4][at] < 0) *negative_gcp = true;
    s += (uint64_t)(i + 1) * ((uint8_t)a[0][at] + 3u * (uint8_t)a[1][at] + 5u * (uint8_t)a[2][at] + 7u * (uint8_t)a[3][at] + 11u * (uint8_t)a[4][at]);
  }
  return s;
}
uint64_t hap_sum(const int8_t* hb, const int8_t* hp, int64_t row, int32_t stride, int64_t n) {
  uint64_t s = 0;
  for (int64_t i = 0; i < n; i++) s += (uint64_t)(i + 1) * ((uint8_t)hb[row * stride + i] + 13u * (uint8_t)hp[row * stride + i]);
  return s;
}
}  // namespace

struct gklhip_pdhmm_ctx {
  int fma_mode = 1, tail_mode = 1;
  int32_t routing[3] = {0, 0, 0};
  float ms = 0.f;
};

namespace {
int run(gklhip_pdhmm_ctx* c, int cross, int32_t n_reads, int32_t n_haps, int32_t max_hap, int32_t max_read, const int8_t* hb,
        const int8_t* hp, const int8_t* const rd[5], const int64_t* hl, const int64_t* rl, int64_t ref_batch_pairs, double* out) {
  delay();
  if (!c || !hb || !hp || !hl || !rl || !out || n_reads <= 0 || n_haps <= 0) { t_err = "bad argument (stub)"; return GKLHIP_ERR_INVALID_ARG; }
  bool negative = false;
  const int64_t n_pairs = cross ? (int64_t)n_reads * n_haps : n_reads;
  for (int64_t p = 0; p < n_pairs; p++) {
    const int64_t r = cross ? p / n_haps : p, h = cross ? p % n_haps : p;
    const uint64_t hr = read_sum(rd, r, max_read, rl[r], &negative);
    uint64_t k = hap_sum(hb, hp, h, max_hap, hl[h]) + 1000003u * (uint64_t)hl[h] + 999983u * (uint64_t)rl[r] + 17u * (uint64_t)c->fma_mode +
                 31u * (uint64_t)c->tail_mode;
    if (cross) k += 7919u * (uint64_t)(ref_batch_pairs % 1000) + 104729u * (uint64_t)(p % 1000) + 5u;
    out[p] = (double)hr * (1.0 / 1048576.0) + (double)k;
  }
  if (negative) { t_err = kInvalid; return GKLHIP_ERR_INVALID_ARG; }
  c->routing[0] = n_reads; c->routing[1] = n_haps; c->routing[2] = cross;
  c->ms = 1.25f + (float)n_pairs;
  return GKLHIP_OK;
}
}  // namespace

extern "C" {

int gklhip_pdhmm_init(int device, gklhip_pdhmm_ctx** out) {
  if (!out) { t_err = "out_ctx is NULL"; return GKLHIP_ERR_INVALID_ARG; }
  *out = new gklhip_pdhmm_ctx();
  return GKLHIP_OK;
}
int gklhip_pdhmm_set_fma_mode(gklhip_pdhmm_ctx* c, int m) {
  if (!c || (m != 0 && m != 1)) { t_err = "fma_mode (stub)"; return GKLHIP_ERR_INVALID_ARG; }
  c->fma_mode = m;
  return GKLHIP_OK;
}
int gklhip_pdhmm_set_tail_mode(gklhip_pdhmm_ctx* c, int m) {
  if (!c || (m != 0 && m != 1)) { t_err = "tail mode (stub)"; return GKLHIP_ERR_INVALID_ARG; }
  c->tail_mode = m;
  return GKLHIP_OK;
}
int gklhip_pdhmm_compute(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_batch* b, double* out) {
  if (!b) { t_err = "batch is NULL"; return GKLHIP_ERR_INVALID_ARG; }
  const int8_t* const rd[5] = {b->read_bases, b->read_qual, b->read_ins_qual, b->read_del_qual, b->gcp};
  return run(c, 0, b->batch, b->batch, b->max_hap_len, b->max_read_len, b->hap_bases, b->hap_pdbases, rd, b->hap_lengths, b->read_lengths, 0, out);
}
int gklhip_pdhmm_compute_cross_batched(gklhip_pdhmm_ctx* c, const gklhip_pdhmm_cross* x, int64_t ref_batch_pairs, double* out) {
  if (!x || ref_batch_pairs < 0) { t_err = "batch is NULL"; return GKLHIP_ERR_INVALID_ARG; }
  const int8_t* const rd[5] = {x->read_bases, x->read_qual, x->read_ins_qual, x->read_del_qual, x->gcp};
  return run(c, 1, x->n_reads, x->n_haps, x->max_hap_len, x->max_read_len, x->hap_bases, x->hap_pdbases, rd, x->hap_lengths, x->read_lengths,
             ref_batch_pairs, out);
}
float gklhip_pdhmm_last_kernel_ms(gklhip_pdhmm_ctx* c) { return c ? c->ms : 0.f; }
int gklhip_pdhmm_last_routing(gklhip_pdhmm_ctx* c, int32_t out[3]) {
  if (!c || !out) { t_err = "NULL argument"; return GKLHIP_ERR_INVALID_ARG; }
  for (int i = 0; i < 3; i++) out[i] = c->routing[i];
  return GKLHIP_OK;
}
int gklhip_pdhmm_done(gklhip_pdhmm_ctx* c) { delete c; return GKLHIP_OK; }
const char* gklhip_pdhmm_last_error(void) { return t_err; }

}  // extern "C"
