// C-ABI implementation (include/inflate/gkl_hip_inflate.h) of the MI355X batch inflate: validation, device layout of a batch of
// raw-deflate streams, one persistent-wavefront launch, read-back of the bytes and the per-stream results; the BGZF
// member walk (bgzf_scan.h, host only) and the whole-file call on top of the two.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/gkl_hip_pairhmm.h"  // status codes
#include "../../include/inflate/gkl_hip_inflate.h"
#include "inflate_kernel.h"
#include "bgzf_scan.h"
#include "hip_host_common.h"   // g_err / fail / HIP_TRY / DevBuf / PinBuf

using namespace gklhip;

struct gklhip_inflate_ctx {
  int device = 0;
  int n_cus = 1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mu;
  PinBuf stage_in, stage_out;   // pinned: input bytes + descriptors up, output bytes + results down
  DevBuf dev_in, dev_out, meta;
  float last_ms = 0.f;
};

namespace {
size_t up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The streams of one call: where each lies in the source and destination images, and the order the wavefronts take them.
struct Job {
  std::vector<InflateStream> streams;
  std::vector<int32_t> order;
  // longest input first, so that the persistent wavefronts finish together: a counting sort on 4096 length classes
  void sort_longest_first() {
    const size_t n = streams.size();
    order.resize(n);
    int64_t max_len = 1;
    for (const InflateStream& s : streams) max_len = std::max<int64_t>(max_len, s.src_len);
    constexpr int kClasses = 4096;
    const auto cls = [&](size_t k) { return (int)(kClasses - 1 - (int64_t)streams[k].src_len * (kClasses - 1) / max_len); };
    std::vector<int32_t> start(kClasses + 1, 0);
    for (size_t k = 0; k < n; k++) start[(size_t)cls(k) + 1]++;
    for (int q = 0; q < kClasses; q++) start[(size_t)q + 1] += start[(size_t)q];
    for (size_t k = 0; k < n; k++) order[(size_t)start[(size_t)cls(k)]++] = (int32_t)k;
  }
};

// n + 1 non-decreasing offsets, each span at most 2^31 - 1
int check_offsets(const int64_t* off, int32_t n, const char* what) {
  if (off[0] < 0) return fail(GKLHIP_ERR_INVALID_ARG, "%s offsets start below 0", what);
  for (int32_t k = 0; k < n; k++) {
    const int64_t d = off[k + 1] - off[k];
    if (d < 0) return fail(GKLHIP_ERR_INVALID_ARG, "%s offsets decrease at stream %d", what, k);
    if (d > INT32_MAX) return fail(GKLHIP_ERR_INVALID_ARG, "stream %d: %s span exceeds 2^31 - 1 bytes", k, what);
  }
  return GKLHIP_OK;
}

int job_from_offsets(Job& job, int32_t n, const int64_t* src_off, const int64_t* dst_off) {
  int rc;
  if ((rc = check_offsets(src_off, n, "source"))) return rc;
  if ((rc = check_offsets(dst_off, n, "destination"))) return rc;
  job.streams.resize((size_t)n);
  for (int32_t k = 0; k < n; k++) {
    InflateStream& s = job.streams[(size_t)k];
    s.src_off = src_off[k];
    s.dst_off = dst_off[k];
    s.src_len = (int32_t)(src_off[k + 1] - src_off[k]);
    s.cap = (int32_t)(dst_off[k + 1] - dst_off[k]);
  }
  job.sort_longest_first();
  return GKLHIP_OK;
}

// Uploads the descriptors and launches on s; every pointer but the job is device memory.  Does not wait.
int launch(gklhip_inflate_ctx* c, hipStream_t s, const Job& job, const uint8_t* d_src, uint8_t* d_dst, int32_t* d_out_len,
           int32_t* d_consumed, uint32_t* d_crc, int32_t* d_status, unsigned char* stage /* pinned, meta_bytes(n) */) {
  const size_t n = job.streams.size();
  const size_t o_desc = 256, o_order = o_desc + up(n * sizeof(InflateStream)), total = o_order + up(n * 4);
  int rc;
  if ((rc = c->meta.reserve(total))) return rc;
  memset(stage, 0, o_desc);   // the counter
  memcpy(stage + o_desc, job.streams.data(), n * sizeof(InflateStream));
  memcpy(stage + o_order, job.order.data(), n * 4);
  HIP_TRY(hipMemcpyAsync(c->meta.p, stage, total, hipMemcpyHostToDevice, s));
  unsigned char* dm = c->meta.as<unsigned char>();
  InflateArgs a;
  a.src = d_src;
  a.dst = d_dst;
  a.streams = reinterpret_cast<const InflateStream*>(dm + o_desc);
  a.order = reinterpret_cast<const int32_t*>(dm + o_order);
  a.n = (int32_t)n;
  a.want_crc = d_crc != nullptr;
  a.out_len = d_out_len;
  a.consumed = d_consumed;
  a.crc32 = d_crc;
  a.status = d_status;
  a.next = reinterpret_cast<int32_t*>(dm);
  // persistent wavefronts: kInflateWavesPerCu per CU at the most, each pulls streams until the counter runs out
  const int n_waves = (int)std::min<size_t>(n, (size_t)c->n_cus * kInflateWavesPerCu);
  HIP_TRY(hipEventRecord(c->ev0, s));
  hipLaunchKernelGGL(inflate_kernel, dim3(n_waves), dim3(64), 0, s, a);
  HIP_TRY(hipEventRecord(c->ev1, s));
  HIP_TRY(hipGetLastError());
  return GKLHIP_OK;
}
size_t meta_bytes(size_t n) { return 256 + up(n * sizeof(InflateStream)) + up(n * 4); }

// Host call over a job whose source offsets index src[0, src_bytes) and whose destinations lie in dst[dst_lo, dst_hi).
int run_host(gklhip_inflate_ctx* c, const Job& job, const uint8_t* src, size_t src_bytes, uint8_t* dst, int64_t dst_lo,
             int64_t dst_hi, int32_t* out_len, int32_t* consumed, uint32_t* crc32, int32_t* status) {
  const size_t n = job.streams.size();
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t dst_bytes = (size_t)(dst_hi - dst_lo);
  const size_t o_meta = up(src_bytes), in_total = o_meta + meta_bytes(n);
  const size_t o_res = up(dst_bytes), out_total = o_res + 4 * up(n * 4);
  int rc;
  if ((rc = c->stage_in.reserve(in_total))) return rc;
  if ((rc = c->dev_in.reserve(std::max<size_t>(src_bytes, 1)))) return rc;
  if ((rc = c->dev_out.reserve(out_total))) return rc;
  if ((rc = c->stage_out.reserve(out_total))) return rc;
  unsigned char* hs = c->stage_in.as<unsigned char>();
  if (src_bytes) {
    memcpy(hs, src, src_bytes);
    HIP_TRY(hipMemcpyAsync(c->dev_in.p, hs, src_bytes, hipMemcpyHostToDevice, s));
  }
  unsigned char* dout = c->dev_out.as<unsigned char>();
  int32_t* d_res = reinterpret_cast<int32_t*>(dout + o_res);
  const size_t stride = up(n * 4) / 4;
  // the kernel addresses dst by the caller's offsets: shift the base so that dst_lo lands on the buffer's first byte
  if ((rc = launch(c, s, job, c->dev_in.as<uint8_t>(), dout - dst_lo, d_res, d_res + stride, crc32 ? reinterpret_cast<uint32_t*>(d_res + 2 * stride) : nullptr,
                   d_res + 3 * stride, hs + o_meta)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->stage_out.p, c->dev_out.p, out_total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  const unsigned char* ho = c->stage_out.as<unsigned char>();
  const int32_t* res = reinterpret_cast<const int32_t*>(ho + o_res);
  memcpy(out_len, res, n * 4);
  if (consumed) memcpy(consumed, res + stride, n * 4);
  if (crc32) memcpy(crc32, res + 2 * stride, n * 4);
  memcpy(status, res + 3 * stride, n * 4);
  // only what a stream wrote goes back: the caller's bytes behind a valid prefix stay as they were
  for (size_t k = 0; k < n; k++) {
    const InflateStream& st = job.streams[k];
    const int32_t len = std::min(std::max(out_len[k], 0), st.cap);
    if (len) memcpy(dst + st.dst_off, ho + (st.dst_off - dst_lo), (size_t)len);
  }
  return GKLHIP_OK;
}
}  // namespace

extern "C" {

const char* gklhip_inflate_last_error(void) { return g_err.c_str(); }

int gklhip_inflate_init(int device, gklhip_inflate_ctx** out_ctx) {
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
  gklhip_inflate_ctx* c = new (std::nothrow) gklhip_inflate_ctx();
  if (!c) return fail(GKLHIP_ERR_OOM, "context allocation failed");
  c->device = device;
  c->n_cus = std::max(prop.multiProcessorCount, 1);
  auto bail = [&](int st) { gklhip_inflate_done(c); return st; };
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipStreamCreate failed"));
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipEventCreate failed"));
  *out_ctx = c;
  return GKLHIP_OK;
}

int gklhip_inflate_done(gklhip_inflate_ctx* c) {
  if (!c) return GKLHIP_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->stage_in.release(); c->stage_out.release();
  c->dev_in.release(); c->dev_out.release(); c->meta.release();
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return GKLHIP_OK;
}

float gklhip_inflate_last_kernel_ms(gklhip_inflate_ctx* c) { return c ? c->last_ms : 0.f; }

int gklhip_inflate_batch(gklhip_inflate_ctx* c, int32_t n, const uint8_t* src, const int64_t* src_off, uint8_t* dst,
                         const int64_t* dst_off, int32_t* out_len, int32_t* consumed, uint32_t* crc32, int32_t* status) {
  return guarded([&]() -> int {
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (n < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative stream count");
    if (n == 0) return GKLHIP_OK;
    if (!src_off || !dst_off || !out_len || !status) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    Job job;
    int rc;
    if ((rc = job_from_offsets(job, n, src_off, dst_off))) return rc;
    if ((src_off[n] > src_off[0] && !src) || (dst_off[n] > dst_off[0] && !dst)) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    // the device image of the source starts at src_off[0]
    for (InflateStream& s : job.streams) s.src_off -= src_off[0];
    return run_host(c, job, src ? src + src_off[0] : nullptr, (size_t)(src_off[n] - src_off[0]), dst, dst_off[0], dst_off[n], out_len, consumed, crc32, status);
  });
}

int gklhip_inflate_batch_device(gklhip_inflate_ctx* c, int32_t n, const uint8_t* src, const int64_t* src_off, uint8_t* dst,
                                const int64_t* dst_off, int32_t* out_len, int32_t* consumed, uint32_t* crc32, int32_t* status,
                                void* hip_stream) {
  return guarded([&]() -> int {
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (n < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative stream count");
    if (n == 0) return GKLHIP_OK;
    if (!src_off || !dst_off || !out_len || !status) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    Job job;
    int rc;
    if ((rc = job_from_offsets(job, n, src_off, dst_off))) return rc;
    if ((src_off[n] > src_off[0] && !src) || (dst_off[n] > dst_off[0] && !dst)) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((rc = c->stage_in.reserve(meta_bytes((size_t)n)))) return rc;
    int32_t* d_consumed = consumed;
    if (!d_consumed) {   // the kernel always writes the counts
      if ((rc = c->dev_out.reserve((size_t)n * 4))) return rc;
      d_consumed = c->dev_out.as<int32_t>();
    }
    if ((rc = launch(c, s, job, src, dst, out_len, d_consumed, crc32, status, c->stage_in.as<unsigned char>()))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return GKLHIP_OK;
  });
}

int gklhip_bgzf_scan(const uint8_t* file, int64_t len, int32_t max_members, int64_t* payload_off, int32_t* payload_len,
                     uint32_t* crc32, uint32_t* isize, int32_t* n_members, int64_t* bytes_used) {
  if (!n_members || !bytes_used) return fail(GKLHIP_ERR_INVALID_ARG, "NULL output");
  *n_members = 0; *bytes_used = 0;
  if (len < 0 || (len > 0 && !file)) return fail(GKLHIP_ERR_INVALID_ARG, "no file image");
  const bool arrays = payload_off || payload_len || crc32 || isize;
  if (arrays && (!payload_off || !payload_len || !crc32 || !isize)) return fail(GKLHIP_ERR_INVALID_ARG, "all four arrays or none");
  if (arrays && max_members < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative max_members");
  const int r = gklinf::bgzf_scan(file, len, max_members, payload_off, payload_len, crc32, isize, n_members, bytes_used);
  if (r != gklinf::BGZF_OK) return fail(GKLHIP_ERR_INVALID_ARG, "member %d at offset %lld: %s", *n_members, (long long)*bytes_used, gklinf::bgzf_scan_message(r));
  return GKLHIP_OK;
}

int gklhip_bgzf_inflate(gklhip_inflate_ctx* c, const uint8_t* file, int64_t len, uint8_t* out, int64_t out_cap,
                        int64_t* out_len, int32_t* bad_member) {
  return guarded([&]() -> int {
    if (!out_len || !bad_member) return fail(GKLHIP_ERR_INVALID_ARG, "NULL output");
    *out_len = 0; *bad_member = -1;
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (out_cap < 0 || (out_cap > 0 && !out)) return fail(GKLHIP_ERR_INVALID_ARG, "no output buffer");
    int32_t n = 0;
    int64_t used = 0;
    int rc = gklhip_bgzf_scan(file, len, 0, nullptr, nullptr, nullptr, nullptr, &n, &used);
    if (rc) { *bad_member = n; return rc; }
    if (n == 0) return GKLHIP_OK;
    std::vector<int64_t> poff((size_t)n);
    std::vector<int32_t> plen((size_t)n), olen((size_t)n), status((size_t)n);
    std::vector<uint32_t> crc((size_t)n), isize((size_t)n), got_crc((size_t)n);
    if ((rc = gklhip_bgzf_scan(file, len, n, poff.data(), plen.data(), crc.data(), isize.data(), &n, &used))) return rc;
    Job job;
    job.streams.resize((size_t)n);
    int64_t at = 0;
    for (int32_t k = 0; k < n; k++) {
      if (isize[(size_t)k] > (uint32_t)INT32_MAX) { *bad_member = k; return fail(GKLHIP_ERR_INVALID_ARG, "member %d: ISIZE exceeds 2^31 - 1", k); }
      InflateStream& s = job.streams[(size_t)k];
      s.src_off = poff[(size_t)k]; s.src_len = plen[(size_t)k];
      s.dst_off = at; s.cap = (int32_t)isize[(size_t)k];
      at += s.cap;
    }
    if (at > out_cap) return fail(GKLHIP_ERR_INVALID_ARG, "the members' ISIZE fields add up to %lld bytes, out_cap is %lld", (long long)at, (long long)out_cap);
    job.sort_longest_first();
    if ((rc = run_host(c, job, file, (size_t)len, out, 0, at, olen.data(), nullptr, got_crc.data(), status.data()))) return rc;
    for (int32_t k = 0; k < n; k++) {
      const size_t i = (size_t)k;
      if (status[i] == 0 && (uint32_t)olen[i] == isize[i] && got_crc[i] == crc[i]) { *out_len += olen[i]; continue; }
      *bad_member = k;
      if (status[i]) return fail(GKLHIP_ERR_INVALID_ARG, "member %d: inflate status %d", k, status[i]);
      if ((uint32_t)olen[i] != isize[i]) return fail(GKLHIP_ERR_INVALID_ARG, "member %d: %d bytes, ISIZE says %u", k, olen[i], isize[i]);
      return fail(GKLHIP_ERR_INVALID_ARG, "member %d: CRC-32 %08x, the member says %08x", k, got_crc[i], crc[i]);
    }
    return GKLHIP_OK;
  });
}

}  // extern "C"
