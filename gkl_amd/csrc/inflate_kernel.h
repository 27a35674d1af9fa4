// Batch inflate for gfx950: one wavefront owns one raw-deflate stream from its first bit to its status word; persistent
// wavefronts pull streams, longest input first, from a counter (the launch form of sw_align_kernel).  The decoder is
// inflate_core.h, instantiated here for 64 lanes: the bit reader and the symbol loop are wave-uniform, the lanes share
// the table fill, the match copy, the literal stores and the CRC chunks.
//
// Window scheme: a match reads the stream's own output back from global memory.  WaveExec::sync() is __syncthreads() of
// a one-wavefront workgroup -- a workgroup-scope release/acquire pair, which on gfx950 is a wait for the wavefront's
// outstanding stores and loads (the CU's L1 is write-through and shared by the workgroup), so visibility holds by the
// memory model and not by timing.  No LDS ring: the tables take 7.6 KB a wavefront, so occupancy stays a choice
// (docs/NOTES.md, "Inflate").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GKL_INF_FN __device__ __forceinline__
#include "inflate_core.h"

namespace gklhip {

struct InflateStream {
  int64_t src_off, dst_off;
  int32_t src_len, cap;
};

struct InflateArgs {
  const uint8_t* src;
  uint8_t* dst;
  const InflateStream* streams;
  const int32_t* order;   // stream indices, longest input first
  int32_t n;
  int32_t want_crc;
  int32_t* out_len;
  int32_t* consumed;
  uint32_t* crc32;
  int32_t* status;
  int32_t* next;          // the counter the wavefronts pull from (0 at launch)
};

struct WaveExec {
  static constexpr int kLanes = 64;
  static __device__ __forceinline__ int lane() { return (int)threadIdx.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// The grid: 16 wavefronts per CU (four per SIMD; the registers allow five, the 7.6 KB of LDS twenty per CU).  A batch
// with more streams than that is worked off by the pull loop; the wavefronts never wait for each other.
constexpr int kInflateWavesPerCu = 16;

__global__ __launch_bounds__(64) void inflate_kernel(InflateArgs a) {
  __shared__ gklinf::Scratch S;
  const int lane = threadIdx.x;
  for (;;) {
    // Every lane takes part in the pull (lane 0 adds 1, the others 0), so no branch on the lane stands between the
    // result stores of the last stream and the readfirstlane below.  With `if (lane == 0) k = atomicAdd(...)` here the
    // compiler joined that branch with the `if (lane == 0)` of the stores across the back edge, took lane 0 out of the
    // loop for both and let lanes 1..63 run on: readfirstlane then read their k = 0 for ever.
    int k = atomicAdd(a.next, lane == 0 ? 1 : 0);
    k = __builtin_amdgcn_readfirstlane(k);
    if (k >= a.n) break;
    const int si = a.order[k];
    const InflateStream s = a.streams[si];
    uint8_t* out = a.dst + s.dst_off;
    int32_t out_len = 0, consumed = 0;
    const int st = gklinf::inflate_stream<WaveExec>(S, a.src + s.src_off, s.src_len, out, s.cap, &out_len, &consumed);
    uint32_t crc = 0;
    if (a.want_crc) crc = gklinf::crc32_stream<WaveExec>(S, out, (uint32_t)out_len);
    if (lane == 0) {
      a.status[si] = st;
      a.out_len[si] = out_len;
      a.consumed[si] = consumed;
      if (a.want_crc) a.crc32[si] = crc;
    }
  }
}

}  // namespace gklhip
