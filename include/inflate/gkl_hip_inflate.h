/*
 * gkl_hip_inflate.h -- C ABI of the MI355X-native batch inflate (raw deflate, RFC 1951, and BGZF members),
 * row f5: the inflate half of GKL's compression component.
 *
 * The reference (com.intel.gkl.compression.IntelInflater, IntelInflater.cc) inflates ONE stream per call, which is a
 * serial dependent chain a GPU loses on.  A BAM file is tens of thousands of independent BGZF members of at most
 * 64 KB, so the entry point here is a batch, which the reference has no counterpart for.  Outputs are bit-exact
 * (acceptance rules: zlib's inflate with windowBits = -15); every malformed input becomes a per-stream status.
 * The header has a directory of its own under include/: the headers directly in include/ are the set whose libraries
 * tests/test_cabi_cpu.py enumerates; tests/test_inflate_core_cpu.py checks this one's symbols.
 * The deflater is include/deflate/gkl_hip_deflate.h.
 * Not here: a libgkl_compression drop-in, JNI, the zlib and gzip wrappers other than BGZF members.
 */
#ifndef GKL_HIP_INFLATE_H
#define GKL_HIP_INFLATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gklhip_inflate_ctx gklhip_inflate_ctx;

/* The calls return gklhip_status of gkl_hip_pairhmm.h (0 ok, 1 invalid argument, 2 no device, 3 out of memory,
 * 4 HIP error, 5 unsupported): GKLHIP_OK whenever the call ran.  A bad stream is a per-stream status: */
enum {
  GKLHIP_INFLATE_OK = 0,               /* the final block's end-of-block symbol was reached */
  GKLHIP_INFLATE_INVALID_BLOCK = 1,    /* block type 3, stored lengths, a dynamic header zlib rejects */
  GKLHIP_INFLATE_INVALID_SYMBOL = 2,   /* invalid literal/length or distance code */
  GKLHIP_INFLATE_INVALID_LOOKBACK = 3, /* a distance that reaches before the stream's first output byte */
  GKLHIP_INFLATE_END_INPUT = 4,        /* the input ends before the final end-of-block symbol */
  GKLHIP_INFLATE_OUT_OVERFLOW = 5      /* the stream would write byte capacity + 1 */
};
/* The first condition met in stream order decides.  Input behind the final end-of-block is no error. */

int gklhip_inflate_init(int device /* -1 = current */, gklhip_inflate_ctx** out_ctx);
int gklhip_inflate_done(gklhip_inflate_ctx* ctx);

/* n independent raw-deflate streams.  Stream k is src[src_off[k] .. src_off[k+1]); its output goes to
 * dst[dst_off[k] ..) with capacity dst_off[k+1] - dst_off[k] (n + 1 non-decreasing offsets each; a stream is at most
 * 2^31 - 1 bytes in and out).  out_len[k] = bytes written, on every status: the valid prefix.  consumed[k] = input
 * bytes used up to and including the one with the final end-of-block (all of them on END_INPUT; unspecified on the
 * other statuses).  crc32[k] = CRC-32 (zlib / BGZF polynomial) of the out_len[k] bytes, computed on the device.
 * Nothing outside [dst_off[k], dst_off[k] + out_len[k]) is written.  n == 0 succeeds and touches nothing. */
int gklhip_inflate_batch(gklhip_inflate_ctx* ctx, int32_t n, const uint8_t* src, const int64_t* src_off,
                         uint8_t* dst, const int64_t* dst_off, int32_t* out_len, int32_t* consumed /* or NULL */,
                         uint32_t* crc32 /* or NULL */, int32_t* status);

/* The same with src, dst, out_len, consumed, crc32 and status in HBM on the context's device; the two offset arrays
 * on the host.  The work is ordered behind hip_stream (a hipStream_t, NULL = the default stream).  SYNCHRONOUS: the
 * results are complete when the call returns. */
int gklhip_inflate_batch_device(gklhip_inflate_ctx* ctx, int32_t n, const uint8_t* src, const int64_t* src_off,
                                uint8_t* dst, const int64_t* dst_off, int32_t* out_len, int32_t* consumed /* or NULL */,
                                uint32_t* crc32 /* or NULL */, int32_t* status, void* hip_stream);

/* Host only, no HIP call: walk the BGZF members of a file image (magic 1f 8b 08 04, the BC subfield, BSIZE, CRC32,
 * ISIZE).  Stops at the end of the file, after max_members, or at the first malformed member (GKLHIP_ERR_INVALID_ARG;
 * *n_members then counts the well-formed members in front of it).  *bytes_used = offset behind the last member taken.
 * The four arrays may all be NULL to count the members. */
int gklhip_bgzf_scan(const uint8_t* file, int64_t len, int32_t max_members, int64_t* payload_off, int32_t* payload_len,
                     uint32_t* crc32, uint32_t* isize, int32_t* n_members, int64_t* bytes_used);

/* scan + batch + check of every member's CRC32 and ISIZE; the members' outputs are concatenated into out.
 * GKLHIP_ERR_INVALID_ARG with *bad_member set (the first such member) for a malformed header, a non-zero stream
 * status, a CRC or an ISIZE mismatch; *bad_member = -1 otherwise.  *out_len = bytes written to out. */
int gklhip_bgzf_inflate(gklhip_inflate_ctx* ctx, const uint8_t* file, int64_t len, uint8_t* out, int64_t out_cap,
                        int64_t* out_len, int32_t* bad_member);

/* HIP-event time of the kernel of the last call, milliseconds. */
float gklhip_inflate_last_kernel_ms(gklhip_inflate_ctx* ctx);
const char* gklhip_inflate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GKL_HIP_INFLATE_H */
