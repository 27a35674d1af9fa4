// Multi-region cross launches of the PDHMM kernels: the region table and the index mappings, for the host and the device.
//
// One launch runs the units of K regions (K computeLikelihoods cross products) whose read items and haplotype items lie
// concatenated in the same device arrays (one common max_read / max_hap stride).  Region k owns
//   read items      [read_base, read_base + n_reads)          haplotype items [hap_base, hap_base + n_haps)
//   output pairs    [pair_base, pair_base + n_reads * n_haps), read-major like a single call's
//   chunks of reads [chunk_base, chunk_base + n_chunks)
// and, in each of the three launches (table, predicate, byte-comparing), a slice of the launch's lists and a range of its
// units: unit u of region k is (item list_start + (u - unit_start) / n_chunks, chunk chunk_base + (u - unit_start) % n_chunks).
// An item is a haplotype GROUP in the table launch (tab_group_start[item] .. tab_group_start[item + 1] of that launch's
// hap_order; groups never straddle regions) and an entry of the launch's hap_order in the other two.
// The table holds K + 1 entries: entry K carries the totals, so every *_base / *_start column is a prefix sum of K + 1
// values and a unit (or a pair index) finds its region by a binary search over it -- uniform over a wavefront, once per unit.
//
// Plain C++ (tests/native/pdhmm_multi_plan_check.cpp compiles it for the host alone, under the sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GKL_PD_HD __host__ __device__ __forceinline__
#else
#define GKL_PD_HD inline
#endif

namespace gklhip {

constexpr int kPdMaxRegions = 64;
constexpr int kPdLaunchTab = 0, kPdLaunchHot = 1, kPdLaunchFull = 2;

struct PdRegion {
  int32_t read_base, hap_base, n_haps, pair_base;
  int32_t chunk_base, n_chunks;
  int32_t list_start[3];   // per launch: first group (table launch) / first hap_order entry (the other two) of the region
  int32_t unit_start[3];   // per launch: first unit of the region
};

// What the host's per-region planning yields.
struct PdRegionShape {
  int32_t n_reads, n_haps;
  int32_t n_chunks;        // chunks of packed reads (0: every read is striped)
  int32_t n_items[3];      // table launch: haplotype groups; predicate / byte-comparing launch: haplotypes
};

// out[0 .. K]: the table (entry K = the totals).
inline void pd_build_regions(const PdRegionShape* s, int K, PdRegion* out) {
  PdRegion acc = {};
  for (int k = 0; k <= K; k++) {
    out[k] = acc;
    if (k == K) break;
    out[k].n_haps = s[k].n_haps;
    out[k].n_chunks = s[k].n_chunks;
    acc.read_base += s[k].n_reads;
    acc.hap_base += s[k].n_haps;
    acc.pair_base += s[k].n_reads * s[k].n_haps;
    acc.chunk_base += s[k].n_chunks;
    for (int l = 0; l < 3; l++) {
      acc.list_start[l] += s[k].n_items[l];
      acc.unit_start[l] += s[k].n_items[l] * s[k].n_chunks;
    }
  }
}

// The region of unit u of a launch, 0 <= u < t[K].unit_start[launch]: the LAST k with unit_start <= u (regions without
// units in this launch share their start with the next one).
GKL_PD_HD int pd_region_of_unit(const PdRegion* __restrict__ t, int K, int launch, int u) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (u >= t[mid].unit_start[launch]) lo = mid; else hi = mid;
  }
  return lo;
}
GKL_PD_HD void pd_unit_split(const PdRegion& r, int launch, int u, int* item, int* chunk) {
  const int local = u - r.unit_start[launch], q = local / r.n_chunks;
  *item = r.list_start[launch] + q;
  *chunk = r.chunk_base + (local - q * r.n_chunks);
}

// (region, read item, haplotype item) -> output pair, and back.  The items are indices into the concatenated arrays.
GKL_PD_HD int pd_pair_index(const PdRegion& r, int ri, int hi) { return r.pair_base + (ri - r.read_base) * r.n_haps + (hi - r.hap_base); }
GKL_PD_HD int pd_region_of_pair(const PdRegion* __restrict__ t, int K, int p) {   // 0 <= p < t[K].pair_base
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p >= t[mid].pair_base) lo = mid; else hi = mid;
  }
  return lo;
}
GKL_PD_HD void pd_pair_split(const PdRegion& r, int p, int* ri, int* hi) {
  const int local = p - r.pair_base, q = local / r.n_haps;
  *ri = r.read_base + q;
  *hi = r.hap_base + (local - q * r.n_haps);
}

}  // namespace gklhip
