/*
 * gkl_hip_deflate.h -- C ABI of the MI355X-native batch deflate (raw deflate, RFC 1951, and BGZF members),
 * row f6: the deflate half of GKL's compression component.
 *
 * The reference (com.intel.gkl.compression.IntelDeflater, IntelDeflater.cc) deflates ONE stream per call; every tool
 * that writes a BAM runs each 64 KB BGZF block through it at level 1 or 2.  The entry point here is a batch of
 * independent streams, one wavefront per stream, as in gkl_hip_inflate.h.  The output is a valid raw-deflate stream
 * that any inflater reads; it is NOT the byte sequence of zlib or ISA-L (no two deflaters agree on that).  The bytes of
 * a stream depend on its input, the level, the strategy and the block-type mask only.
 * The header has a directory of its own under include/ (see gkl_hip_inflate.h).
 *
 * Levels: 0 = stored blocks only; 1 = a one-entry hash table of 4-byte keys, greedy selection (the fast one); 3 to 8 =
 * hash chains of 3-byte keys searched to a depth, minimum match 3 (a 3-byte match farther back than 4096 is dropped),
 * lazy selection from level 4 on, a walk over once a match of `nice` bytes is found:
 *     level   3    4    5    6    7    8
 *     depth   4    8   16   32   64  128
 *     nice   32   32   64  128  258  258
 *     lazy   no  yes  yes  yes  yes  yes
 * The reference sends every level but 1 and 2 to zlib; 5 is htsjdk's default.  Huffman only gives the same bytes at
 * every level from 1 to 8.  Levels 2, 9 and -1 (zlib's default) are left for a later change and are refused.
 * Not here: levels 2, 9 and -1, a libgkl_compression drop-in, JNI, the zlib and gzip wrappers other than BGZF members.
 */
#ifndef GKL_HIP_DEFLATE_H
#define GKL_HIP_DEFLATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gklhip_deflate_ctx gklhip_deflate_ctx;

/* The calls return gklhip_status of gkl_hip_pairhmm.h (0 ok, 1 invalid argument, 2 no device, 3 out of memory,
 * 4 HIP error, 5 unsupported): GKLHIP_OK whenever the call ran.  A stream that does not fit is a per-stream status: */
enum {
  GKLHIP_DEFLATE_OK = 0,
  GKLHIP_DEFLATE_OUT_OVERFLOW = 1      /* the stream's exact size exceeds its capacity; its out_len is 0 */
};
enum { GKLHIP_DEFLATE_DEFAULT_STRATEGY = 0, GKLHIP_DEFLATE_HUFFMAN_ONLY = 1 };
enum { GKLHIP_DEFLATE_STORED = 1, GKLHIP_DEFLATE_FIXED = 2, GKLHIP_DEFLATE_DYNAMIC = 4 };

/* init allocates the token area of the context once: 320 KB per resident wavefront (8 per compute unit) -- 256 KB of
 * tokens and the 64 KB ring of chain links of levels 3 to 8 -- which is 640 MB on an MI355X's 256 compute units. */
int gklhip_deflate_init(int device /* -1 = current */, gklhip_deflate_ctx** out_ctx);
int gklhip_deflate_done(gklhip_deflate_ctx* ctx);

/* Host arithmetic, no HIP call: the size of `len` bytes in stored blocks, len + 5 * max(1, ceil(len / 65535)).  A stream
 * given this capacity never overflows while stored blocks are allowed. */
int64_t gklhip_deflate_bound(int64_t len);

/* strategy: 0 default, 1 Huffman only (no match search, zlib's Z_HUFFMAN_ONLY).  block_types: a mask of the block
 * types the encoder may choose from, stored = 1, fixed = 2, dynamic = 4; 0 and 7 mean all (2 is zlib's Z_FIXED).
 * Holds for the context's later calls. */
int gklhip_deflate_set_strategy(gklhip_deflate_ctx* ctx, int32_t strategy, int32_t block_types);

/* n independent inputs.  Input k is src[src_off[k] .. src_off[k+1]); its stream goes to dst[dst_off[k] ..) with
 * capacity dst_off[k+1] - dst_off[k] (n + 1 non-decreasing offsets each; an input and a capacity are at most
 * 2^31 - 1 bytes).  level 0, 1 or 3 to 8 (above); other levels: GKLHIP_ERR_UNSUPPORTED.
 * out_len[k] = bytes of the stream (0 on OUT_OVERFLOW).  crc32[k] = CRC-32 (zlib / BGZF polynomial) of INPUT k.
 * Nothing outside [dst_off[k], dst_off[k+1]) is written for stream k.  n == 0 succeeds and touches nothing. */
int gklhip_deflate_batch(gklhip_deflate_ctx* ctx, int32_t n, const uint8_t* src, const int64_t* src_off, uint8_t* dst,
                         const int64_t* dst_off, int32_t level, int32_t* out_len, uint32_t* crc32 /* of the input, or NULL */,
                         int32_t* status);

/* The same with src, dst, out_len, crc32 and status in HBM on the context's device; the two offset arrays on the host.
 * The work is ordered behind hip_stream (a hipStream_t, NULL = the default stream).  SYNCHRONOUS. */
int gklhip_deflate_batch_device(gklhip_deflate_ctx* ctx, int32_t n, const uint8_t* src, const int64_t* src_off,
                                uint8_t* dst, const int64_t* dst_off, int32_t level, int32_t* out_len,
                                uint32_t* crc32 /* or NULL */, int32_t* status, void* hip_stream);

/* Host arithmetic: an out_cap that gklhip_bgzf_deflate never exceeds (every member stored, plus the EOF member). */
int64_t gklhip_bgzf_bound(int64_t len, int32_t block_size);

/* Cuts data into members of block_size input bytes (1 .. 65498, 0 = 65280), deflates them as one batch, frames each
 * with the 18-byte BGZF header (1f 8b 08 04, XLEN 6, BC, BSIZE), CRC32 and ISIZE, and packs them back to back into
 * out; append_eof adds the standard 28-byte empty member.  Every member is at most 65536 bytes.  Empty data yields
 * the EOF member only, or nothing. */
int gklhip_bgzf_deflate(gklhip_deflate_ctx* ctx, const uint8_t* data, int64_t len, int32_t block_size, int32_t level,
                        int32_t append_eof, uint8_t* out, int64_t out_cap, int64_t* out_len, int32_t* n_members);

/* HIP-event time of the kernel of the last call, milliseconds. */
float gklhip_deflate_last_kernel_ms(gklhip_deflate_ctx* ctx);
const char* gklhip_deflate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GKL_HIP_DEFLATE_H */
