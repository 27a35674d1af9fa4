// Batch deflate for gfx950: one wavefront owns one input from its CRC-32 to its status word; persistent wavefronts pull
// inputs, longest first, from a counter (the launch form of inflate_kernel).  The encoder is deflate_core.h,
// instantiated here for 64 lanes: lane i of a chunk looks up, extends and inserts position i, the selection is
// wave-uniform over a ballot of the candidates, the histograms and the bit packing are LDS atomics.
//
// LDS: 20 160 B a wavefront (16 KB of it the match table, which the code construction, the CRC and the emission
// reuse), so eight
// workgroups fit a CU's 160 KB; the grid is kDeflateWavesPerCu per CU.  Tokens go to the wavefront's own 320 KB of
// the context's token area in global memory (256 KB of tokens, then the 64 KB ring of chain links that levels 3-8 use)
// and are read back by the same wavefront behind WaveExec::sync() (__syncthreads() of a one-wavefront workgroup: see
// inflate_kernel.h on why that is visibility by the memory model).  At levels 3-8 lane i also walks the chain of
// position i; the walk's bound is the level's depth, whatever the ring holds (deflate_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GKL_INF_FN __device__ __forceinline__
#define GKL_DEF_FN __device__ __forceinline__
#include "deflate_core.h"

namespace gklhip {

struct DeflateStream {
  int64_t src_off, dst_off;
  int32_t src_len, cap;
};

struct DeflateArgs {
  const uint8_t* src;
  uint8_t* dst;
  const DeflateStream* streams;
  const int32_t* order;   // stream indices, longest input first
  int32_t n;
  int32_t level, strategy, types;
  int32_t* out_len;
  uint32_t* crc32;        // of the input, or NULL
  int32_t* status;
  int32_t* next;          // the counter the wavefronts pull from (0 at launch)
  uint32_t* tokens;       // gkldef::kTokensPerWave words per wavefront of the grid
};

struct DeflateWaveExec {
  static constexpr int kLanes = 64;
  static __device__ __forceinline__ int lane() { return (int)threadIdx.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
  static __device__ __forceinline__ uint32_t excl_scan64(uint32_t* a) {
    __syncthreads();
    const int l = (int)threadIdx.x;
    const uint32_t v = a[l];
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d);
      if (l >= d) inc += t;
    }
    a[l] = inc - v;
    const uint32_t total = __shfl(inc, 63);
    __syncthreads();
    return total;
  }
  static __device__ __forceinline__ uint64_t which64(const uint16_t* a) { return __ballot(a[threadIdx.x] != 0); }
  static __device__ __forceinline__ void atomic_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
  static __device__ __forceinline__ void atomic_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
  // LDS has no 16-bit atomic: a compare-and-swap on the word that holds the entry
  static __device__ __forceinline__ void atomic_max16(uint16_t* p, uint16_t v) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    uint32_t* w = reinterpret_cast<uint32_t*>(addr & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(addr & 2u) * 8u;
    uint32_t old = *w;
    for (;;) {
      if (((old >> sh) & 0xFFFFu) >= v) break;
      const uint32_t want = (old & ~(0xFFFFu << sh)) | ((uint32_t)v << sh);
      const uint32_t seen = atomicCAS(w, old, want);
      if (seen == old) break;
      old = seen;
    }
  }
};

// The grid: 8 wavefronts per CU, what 20 160 B of LDS each leave room for.  A batch with more inputs is worked off by
// the pull loop; the wavefronts never wait for each other.
constexpr int kDeflateWavesPerCu = 8;

// Two instantiations: SEARCH_TABLE for levels 0 and 1, SEARCH_CHAINS for levels 3-8 (and for their Huffman-only
// streams, which search nothing).  Neither carries the other's search, so level 1 pays nothing for the chains.
template <int kSearches>
__global__ __launch_bounds__(64) void deflate_kernel(DeflateArgs a) {
  __shared__ gkldef::Scratch S;
  const int lane = threadIdx.x;
  uint32_t* toks = a.tokens + (size_t)blockIdx.x * gkldef::kTokensPerWave;
  for (;;) {
    // every lane takes part in the pull, as in inflate_kernel (a branch on the lane here once merged with the one
    // around the result stores across the back edge, and the wavefront looped for ever)
    int k = atomicAdd(a.next, lane == 0 ? 1 : 0);
    k = __builtin_amdgcn_readfirstlane(k);
    if (k >= a.n) break;
    const int si = a.order[k];
    const DeflateStream s = a.streams[si];
    const uint8_t* in = a.src + s.src_off;
    uint32_t crc = 0;
    if (a.crc32) crc = gklinf::crc32_stream<DeflateWaveExec>(S.u.inf, in, (uint32_t)s.src_len);
    int32_t out_len = 0;
    const int st = gkldef::deflate_stream<DeflateWaveExec, kSearches>(S, in, s.src_len, a.dst + s.dst_off, s.cap, toks, a.level, a.strategy, a.types, &out_len);
    if (lane == 0) {
      a.status[si] = st;
      a.out_len[si] = out_len;
      if (a.crc32) a.crc32[si] = crc;
    }
  }
}

}  // namespace gklhip
