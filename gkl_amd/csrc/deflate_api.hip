// C-ABI implementation (include/deflate/gkl_hip_deflate.h) of the MI355X batch deflate: validation, device layout of a
// batch of inputs, one persistent-wavefront launch, read-back of the streams and the per-stream results; the BGZF
// framing (bgzf_frame.h, host only) and the whole-buffer call on top.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/gkl_hip_pairhmm.h"  // status codes
#include "../../include/deflate/gkl_hip_deflate.h"
#include "deflate_kernel.h"
#include "bgzf_frame.h"
#include "hip_host_common.h"   // g_err / fail / HIP_TRY / DevBuf / PinBuf

using namespace gklhip;

struct gklhip_deflate_ctx {
  int device = 0;
  int n_waves = 1;              // the grid at the most; the token area is sized by it
  int32_t strategy = 0, types = gkldef::BT_ALL;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mu;
  PinBuf stage_in, stage_out;   // pinned: input bytes + descriptors up, streams + results down
  DevBuf dev_in, dev_out, meta;
  void* tokens = nullptr;       // n_waves x kTokensPerWave words, allocated once
  float last_ms = 0.f;
};

namespace {
size_t up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The inputs of one call: where each lies in the source and destination images, and the order the wavefronts take them.
struct Job {
  std::vector<DeflateStream> streams;
  std::vector<int32_t> order;
  // longest input first, so that the persistent wavefronts finish together: a counting sort on 4096 length classes
  void sort_longest_first() {
    const size_t n = streams.size();
    order.resize(n);
    int64_t max_len = 1;
    for (const DeflateStream& s : streams) max_len = std::max<int64_t>(max_len, s.src_len);
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
    DeflateStream& s = job.streams[(size_t)k];
    s.src_off = src_off[k];
    s.dst_off = dst_off[k];
    s.src_len = (int32_t)(src_off[k + 1] - src_off[k]);
    s.cap = (int32_t)(dst_off[k + 1] - dst_off[k]);
  }
  job.sort_longest_first();
  return GKLHIP_OK;
}

int check_level(int32_t level) {
  if (level == 0 || level == 1 || (level >= 3 && level <= 8)) return GKLHIP_OK;
  return fail(GKLHIP_ERR_UNSUPPORTED, "compression level %d is not built: 0 (stored), 1 and 3 to 8 are", level);
}

size_t meta_bytes(size_t n) { return 256 + up(n * sizeof(DeflateStream)) + up(n * 4); }

// Uploads the descriptors and launches on s; every pointer but the job is device memory.  Does not wait.
int launch(gklhip_deflate_ctx* c, hipStream_t s, const Job& job, int32_t level, const uint8_t* d_src, uint8_t* d_dst, int32_t* d_out_len,
           uint32_t* d_crc, int32_t* d_status, unsigned char* stage /* pinned, meta_bytes(n) */) {
  const size_t n = job.streams.size();
  const size_t o_desc = 256, o_order = o_desc + up(n * sizeof(DeflateStream)), total = o_order + up(n * 4);
  int rc;
  if ((rc = c->meta.reserve(total))) return rc;
  memset(stage, 0, o_desc);   // the counter
  memcpy(stage + o_desc, job.streams.data(), n * sizeof(DeflateStream));
  memcpy(stage + o_order, job.order.data(), n * 4);
  HIP_TRY(hipMemcpyAsync(c->meta.p, stage, total, hipMemcpyHostToDevice, s));
  unsigned char* dm = c->meta.as<unsigned char>();
  DeflateArgs a;
  a.src = d_src;
  a.dst = d_dst;
  a.streams = reinterpret_cast<const DeflateStream*>(dm + o_desc);
  a.order = reinterpret_cast<const int32_t*>(dm + o_order);
  a.n = (int32_t)n;
  a.level = level;
  a.strategy = c->strategy;
  a.types = c->types;
  a.out_len = d_out_len;
  a.crc32 = d_crc;
  a.status = d_status;
  a.next = reinterpret_cast<int32_t*>(dm);
  a.tokens = static_cast<uint32_t*>(c->tokens);
  // persistent wavefronts: each pulls inputs until the counter runs out, each owns one slice of the token area
  const int n_waves = (int)std::min<size_t>(n, (size_t)c->n_waves);
  HIP_TRY(hipEventRecord(c->ev0, s));
  // levels 0 and 1 launch the kernel they always had; the chain search of levels 3-8 is a kernel of its own
  if (level >= 3) hipLaunchKernelGGL(deflate_kernel<gkldef::SEARCH_CHAINS>, dim3(n_waves), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(deflate_kernel<gkldef::SEARCH_TABLE>, dim3(n_waves), dim3(64), 0, s, a);
  HIP_TRY(hipEventRecord(c->ev1, s));
  HIP_TRY(hipGetLastError());
  return GKLHIP_OK;
}

// Host call over a job whose source offsets index src[0, src_bytes) and whose destinations lie in dst[dst_lo, dst_hi).
// The caller holds the context's lock.
int run_host(gklhip_deflate_ctx* c, const Job& job, int32_t level, const uint8_t* src, size_t src_bytes, uint8_t* dst, int64_t dst_lo,
             int64_t dst_hi, int32_t* out_len, uint32_t* crc32, int32_t* status) {
  const size_t n = job.streams.size();
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t dst_bytes = (size_t)(dst_hi - dst_lo);
  const size_t o_meta = up(src_bytes), in_total = o_meta + meta_bytes(n);
  const size_t o_res = up(dst_bytes), out_total = o_res + 3 * up(n * 4);
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
  if ((rc = launch(c, s, job, level, c->dev_in.as<uint8_t>(), dout - dst_lo, d_res, crc32 ? reinterpret_cast<uint32_t*>(d_res + stride) : nullptr,
                   d_res + 2 * stride, hs + o_meta)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->stage_out.p, c->dev_out.p, out_total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  const unsigned char* ho = c->stage_out.as<unsigned char>();
  const int32_t* res = reinterpret_cast<const int32_t*>(ho + o_res);
  memcpy(out_len, res, n * 4);
  if (crc32) memcpy(crc32, res + stride, n * 4);
  memcpy(status, res + 2 * stride, n * 4);
  // only a stream's bytes go back: the caller's bytes behind it stay as they were
  for (size_t k = 0; k < n; k++) {
    const DeflateStream& st = job.streams[k];
    const int32_t len = std::min(std::max(out_len[k], 0), st.cap);
    if (len) memcpy(dst + st.dst_off, ho + (st.dst_off - dst_lo), (size_t)len);
  }
  return GKLHIP_OK;
}
}  // namespace

extern "C" {

const char* gklhip_deflate_last_error(void) { return g_err.c_str(); }

int64_t gklhip_deflate_bound(int64_t len) { return gkldef::deflate_bound(len); }

int64_t gklhip_bgzf_bound(int64_t len, int32_t block_size) {
  if (block_size == 0) block_size = gkldef::kBgzfDefaultBlock;
  if (block_size < 1 || block_size > gkldef::kBgzfMaxBlock) return -1;
  return gkldef::bgzf_bound(len, block_size);
}

int gklhip_deflate_init(int device, gklhip_deflate_ctx** out_ctx) {
  return guarded([&]() -> int {
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
    gklhip_deflate_ctx* c = new (std::nothrow) gklhip_deflate_ctx();
    if (!c) return fail(GKLHIP_ERR_OOM, "context allocation failed");
    c->device = device;
    c->n_waves = std::max(prop.multiProcessorCount, 1) * kDeflateWavesPerCu;
    auto bail = [&](int st) { gklhip_deflate_done(c); return st; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipStreamCreate failed"));
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return bail(fail(GKLHIP_ERR_HIP, "hipEventCreate failed"));
    if (hipMalloc(&c->tokens, (size_t)c->n_waves * gkldef::kTokensPerWave * sizeof(uint32_t)) != hipSuccess) {
      (void)hipGetLastError();
      c->tokens = nullptr;
      return bail(fail(GKLHIP_ERR_OOM, "the token area (%d wavefronts x 256 KB) could not be allocated", c->n_waves));
    }
    *out_ctx = c;
    return GKLHIP_OK;
  });
}

int gklhip_deflate_done(gklhip_deflate_ctx* c) {
  if (!c) return GKLHIP_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->stage_in.release(); c->stage_out.release();
  c->dev_in.release(); c->dev_out.release(); c->meta.release();
  if (c->tokens) (void)hipFree(c->tokens);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return GKLHIP_OK;
}

float gklhip_deflate_last_kernel_ms(gklhip_deflate_ctx* c) { return c ? c->last_ms : 0.f; }

int gklhip_deflate_set_strategy(gklhip_deflate_ctx* c, int32_t strategy, int32_t block_types) {
  return guarded([&]() -> int {
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (strategy != 0 && strategy != 1) return fail(GKLHIP_ERR_INVALID_ARG, "strategy %d: 0 (default) or 1 (Huffman only)", strategy);
    if (block_types < 0 || block_types > 7) return fail(GKLHIP_ERR_INVALID_ARG, "block type mask %d: stored = 1, fixed = 2, dynamic = 4", block_types);
    std::lock_guard<std::mutex> lock(c->mu);
    c->strategy = strategy;
    c->types = block_types ? block_types : (int32_t)gkldef::BT_ALL;
    return GKLHIP_OK;
  });
}

int gklhip_deflate_batch(gklhip_deflate_ctx* c, int32_t n, const uint8_t* src, const int64_t* src_off, uint8_t* dst,
                         const int64_t* dst_off, int32_t level, int32_t* out_len, uint32_t* crc32, int32_t* status) {
  return guarded([&]() -> int {
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (n < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative stream count");
    int rc;
    if ((rc = check_level(level))) return rc;
    if (n == 0) return GKLHIP_OK;
    if (!src_off || !dst_off || !out_len || !status) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    Job job;
    if ((rc = job_from_offsets(job, n, src_off, dst_off))) return rc;
    if ((src_off[n] > src_off[0] && !src) || (dst_off[n] > dst_off[0] && !dst)) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    // the device image of the source starts at src_off[0]
    for (DeflateStream& s : job.streams) s.src_off -= src_off[0];
    std::lock_guard<std::mutex> lock(c->mu);
    return run_host(c, job, level, src ? src + src_off[0] : nullptr, (size_t)(src_off[n] - src_off[0]), dst, dst_off[0], dst_off[n], out_len, crc32, status);
  });
}

int gklhip_deflate_batch_device(gklhip_deflate_ctx* c, int32_t n, const uint8_t* src, const int64_t* src_off, uint8_t* dst,
                                const int64_t* dst_off, int32_t level, int32_t* out_len, uint32_t* crc32, int32_t* status,
                                void* hip_stream) {
  return guarded([&]() -> int {
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (n < 0) return fail(GKLHIP_ERR_INVALID_ARG, "negative stream count");
    int rc;
    if ((rc = check_level(level))) return rc;
    if (n == 0) return GKLHIP_OK;
    if (!src_off || !dst_off || !out_len || !status) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    Job job;
    if ((rc = job_from_offsets(job, n, src_off, dst_off))) return rc;
    if ((src_off[n] > src_off[0] && !src) || (dst_off[n] > dst_off[0] && !dst)) return fail(GKLHIP_ERR_INVALID_ARG, "NULL array");
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((rc = c->stage_in.reserve(meta_bytes((size_t)n)))) return rc;
    if ((rc = launch(c, s, job, level, src, dst, out_len, crc32, status, c->stage_in.as<unsigned char>()))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return GKLHIP_OK;
  });
}

int gklhip_bgzf_deflate(gklhip_deflate_ctx* c, const uint8_t* data, int64_t len, int32_t block_size, int32_t level,
                        int32_t append_eof, uint8_t* out, int64_t out_cap, int64_t* out_len, int32_t* n_members) {
  return guarded([&]() -> int {
    if (!out_len || !n_members) return fail(GKLHIP_ERR_INVALID_ARG, "NULL output");
    *out_len = 0; *n_members = 0;
    if (!c) return fail(GKLHIP_ERR_INVALID_ARG, "context is NULL");
    if (len < 0 || (len > 0 && !data)) return fail(GKLHIP_ERR_INVALID_ARG, "no data");
    if (out_cap < 0 || (out_cap > 0 && !out)) return fail(GKLHIP_ERR_INVALID_ARG, "no output buffer");
    if (block_size == 0) block_size = gkldef::kBgzfDefaultBlock;
    if (block_size < 1 || block_size > gkldef::kBgzfMaxBlock) return fail(GKLHIP_ERR_INVALID_ARG, "block_size %d: 1 .. %d, 0 = %d", block_size, gkldef::kBgzfMaxBlock, gkldef::kBgzfDefaultBlock);
    int rc;
    if ((rc = check_level(level))) return rc;
    const int64_t m64 = gkldef::bgzf_members(len, block_size);
    if (m64 > INT32_MAX) return fail(GKLHIP_ERR_INVALID_ARG, "%lld members exceed 2^31 - 1", (long long)m64);
    const size_t m = (size_t)m64;
    int64_t at = 0;
    if (m) {
      // every member's stream lands kBgzfHeader bytes into a slot of the stored size + the frame
      const int64_t slot = gkldef::kBgzfHeader + gkldef::deflate_bound(block_size) + gkldef::kBgzfTrailer;
      std::vector<uint8_t> image((size_t)slot * m);
      std::vector<int32_t> clen(m), status(m);
      std::vector<uint32_t> crc(m);
      Job job;
      job.streams.resize(m);
      for (size_t k = 0; k < m; k++) {
        DeflateStream& s = job.streams[k];
        s.src_off = (int64_t)k * block_size;
        s.src_len = (int32_t)std::min<int64_t>(block_size, len - s.src_off);
        s.dst_off = (int64_t)k * slot + gkldef::kBgzfHeader;
        s.cap = (int32_t)gkldef::deflate_bound(s.src_len);
      }
      job.sort_longest_first();
      std::lock_guard<std::mutex> lock(c->mu);
      if ((rc = run_host(c, job, level, data, (size_t)len, image.data(), 0, slot * (int64_t)m, clen.data(), crc.data(), status.data()))) return rc;
      for (size_t k = 0; k < m; k++) {
        if (status[k]) return fail(GKLHIP_ERR_INVALID_ARG, "member %zu does not fit 64 KB under the block-type mask in force", k);
        uint8_t* p = image.data() + k * (size_t)slot;
        const uint32_t total = gkldef::bgzf_frame(p, (uint32_t)clen[k], crc[k], (uint32_t)job.streams[k].src_len);
        if (at + total > out_cap) return fail(GKLHIP_ERR_INVALID_ARG, "out_cap %lld is too small: gklhip_bgzf_bound gives %lld", (long long)out_cap, (long long)gkldef::bgzf_bound(len, block_size));
        memcpy(out + at, p, total);
        at += total;
      }
    }
    if (append_eof) {
      if (at + gkldef::kBgzfEof > out_cap) return fail(GKLHIP_ERR_INVALID_ARG, "out_cap %lld has no room for the end-of-file member", (long long)out_cap);
      gkldef::bgzf_eof(out + at);
      at += gkldef::kBgzfEof;
    }
    *out_len = at;
    *n_members = (int32_t)m + (append_eof ? 1 : 0);
    return GKLHIP_OK;
  });
}

}  // extern "C"
