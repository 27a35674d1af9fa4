// Several small PairHMM calls in one set of launches: which calls share a set, where each call's blocks begin in a
// launch, and how a block finds its call -- for the host (SmallCombiner, gklhip_compute_multi) and the kernels
// (pairhmm_aux_kernels.h: the *_multi_kernel families).
//
// A launch of a set runs the blocks of its n calls back to back: call k owns blocks [begin[k], begin[k + 1]) and runs
// local block (block - begin[k]) exactly as its single-call kernel would.  begin[] is a prefix sum of n + 1 values, so a
// block finds its call by a binary search over it -- uniform over the wavefront, once per block.
//
// The rules only: what a multi call does with them -- lanes, order, failures -- is pairhmm_multi_call.h, which includes
// this file.  Plain C++ (tests/native/pairhmm_multi_sets_check.cpp, pairhmm_multi_mid_check.cpp, pairhmm_mid_combine_check.cpp
// and pairhmm_multi_call_check.cpp compile it for the host alone, under the sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GKL_MS_HD __host__ __device__ __forceinline__
#else
#define GKL_MS_HD inline
#endif

namespace gklhip {

constexpr int kMultiMax = 64;     // calls per set of launches (what MultiArgs holds: a set of gklhip_compute_multi)
constexpr int kCombineMax = 16;   // ... of which a leader of concurrent callers takes at most this many (SmallCombiner::run)

// The set-cutting rule of gklhip_compute_multi (multi_call_drive applies it).  The regions that qualify for a shared set (the single call would defer
// them: small_call_defers) form runs in input order: a run ends where the next qualifying region is of another kind
// (`kind`: any values -- the fused per-pair kernel, the one-launch policy, the all-fp64 per-pair kernel of a
// double-precision context); regions that do not qualify run alone and do not interrupt a run.  A run of m regions
// is cut into ceil(m / kMultiMax) sets of consecutive regions whose sizes differ by at most one -- 65 regions leave as
// 33 + 32, not as 64 and one region that pays a set of launches alone.
// set_of[k]: the set of region k, numbered from 0 in input order, or -1 for a region that does not qualify.  Returns the
// number of sets.
inline int multi_cut_sets(const uint8_t* qualifies, const uint8_t* kind, int n, int32_t* set_of) {
  int n_sets = 0;
  for (int k = 0; k < n;) {
    if (!qualifies[k]) { set_of[k++] = -1; continue; }
    int m = 0, end = k;
    for (; end < n && (!qualifies[end] || kind[end] == kind[k]); end++) m += qualifies[end] ? 1 : 0;
    const int sets = (m + kMultiMax - 1) / kMultiMax;
    for (int j = k, i = 0; j < end; j++) {
      if (!qualifies[j]) { set_of[j] = -1; continue; }
      set_of[j] = n_sets + (int)((int64_t)i * sets / m);
      i++;
    }
    n_sets += sets;
    k = end;
  }
  return n_sets;
}

// ---- which waiting calls a leader of concurrent callers takes (SmallCombiner::run) ----
// A leader takes itself first, then the waiting calls of its own kind and arithmetic mode in arrival order, at most
// kCombineMax in all.  A set of MID-SIZE calls (2049 - 65 536 pairs; concurrent callers' only enter with the context's
// mid-size switch on: gklhip_set_mid_combine) has two limits more, both conditions and not measurements:
//   kCombineMidPairs  the pairs of one set, twice the largest region.  A set ends when its slowest member does: the cap
//                     bounds how long a 2049-pair call can be held by its company to about two largest regions' work.
//                     A waiting call that does not fit is PASSED OVER, not a stop: later, smaller ones are still
//                     considered (first fit in arrival order).  The passed-over call loses nothing by it -- its own thread
//                     leads it as soon as it is admitted.  The leader always goes, whatever its size.
//   kMidFlights       mid-size sets in the air at a time, of the combiner's four flight slots.  A mid-size set holds its
//                     slot for milliseconds, a GATK-sized one for tens of microseconds: those must always find a slot.  A
//                     mid-size call that finds kMidFlights mid-size sets in the air waits in the queue -- where it gains
//                     company -- even when a slot is free.  With fewer slots than four (GKL_HIP_COMBINE_FLIGHTS) mid-size
//                     sets leave one of them to the small calls: at most min(kMidFlights, slots - 1), combine_mid_flights.
//                     ONE slot is shared by whoever comes first: the promise to the small calls does not hold there.
constexpr int64_t kCombineMidPairs = 131072;
constexpr int kMidFlights = 2;
constexpr int combine_mid_flights(int max_flights) {
  return max_flights <= 1 ? 1 : (kMidFlights < max_flights - 1 ? kMidFlights : max_flights - 1);
}

// What the rule reads of a call.
struct CombineCall {
  int32_t kind, fma;
  int64_t pairs;
};
// The set of one leader, filled call by call in arrival order: takes(c) says whether waiting call c rides along (and
// counts it in).  `mid`: the leader's kind is a mid-size one.
struct CombinePick {
  CombineCall lead;
  bool mid;
  int n = 1;
  int64_t pairs;
  CombinePick(const CombineCall& leader, bool leader_is_mid) : lead(leader), mid(leader_is_mid), pairs(leader.pairs) {}
  bool takes(const CombineCall& c) {
    if (n >= kCombineMax || c.fma != lead.fma || c.kind != lead.kind) return false;
    if (mid && pairs + c.pairs > kCombineMidPairs) return false;
    n++;
    pairs += c.pairs;
    return true;
  }
};
// ... over a whole queue, as SmallCombiner::run calls it: picked[0] = leader, then the queue positions that ride along,
// ascending; returns their number (picked holds kCombineMax entries).
inline int combine_pick(const CombineCall* queue, int n_queue, int leader, bool mid, int32_t* picked) {
  CombinePick pick(queue[leader], mid);
  picked[0] = leader;
  for (int i = 0; i < n_queue; i++)
    if (i != leader && pick.takes(queue[i])) picked[pick.n - 1] = i;
  return pick.n;
}
// May a waiting call lead now?  `flights` sets are in the air, `mid_flights` of them mid-size.
inline bool combine_admits(bool mid, int flights, int mid_flights, int max_flights) {
  return flights < max_flights && (!mid || mid_flights < combine_mid_flights(max_flights));
}

// Mid-size regions (two-launch per-pair policy: more than kTwoStepFrom pairs, pairhmm_device_pass.h) share sets of their
// own kind only, and are cut apart from the small ones: for the small regions' cut they are regions that do not qualify
// (they do not interrupt a run of small regions), and here the small ones do not interrupt them.  The mid-size regions of
// the call, in input order, are cut by the rule above -- at most kMultiMax per set, sizes differing by at most one -- and a
// set of ONE region is no set: that region runs alone through the single-call path (set_of -1).  Sets are numbered from 0.
inline int multi_cut_mid_sets(const uint8_t* mid, int n, int32_t* set_of) {
  int m = 0;
  for (int k = 0; k < n; k++) m += mid[k] ? 1 : 0;
  const int sets = m < 2 ? 0 : (m + kMultiMax - 1) / kMultiMax;
  for (int k = 0, i = 0; k < n; k++) {
    if (!mid[k] || sets == 0) { set_of[k] = -1; continue; }
    set_of[k] = (int)((int64_t)i * sets / m);
    i++;
  }
  return sets;
}

// The two launches of a mid-size region's policy, as the single call sizes them (launch_pair_policy_two_step) and as the
// region's share of a set's launches: a thread per pair flags, then `multi_recompute_blocks` one-wavefront blocks walk the
// list of the flagged pairs -- local block b takes entries b, b + g, b + 2 g, ... of the region's count.
constexpr int kFlagBlock = 256;
GKL_MS_HD int multi_flag_blocks(int n_pairs) { return (n_pairs + kFlagBlock - 1) / kFlagBlock; }
GKL_MS_HD int multi_recompute_blocks(int n_pairs) { return n_pairs / 2 > 256 ? n_pairs / 2 : 256; }

// begin[0 .. n]: first block of each call in a launch of `blocks[k]` blocks per call (begin[n] = the grid).
inline void multi_begin(const int32_t* blocks, int n, int32_t* begin) {
  begin[0] = 0;
  for (int k = 0; k < n; k++) begin[k + 1] = begin[k] + blocks[k];
}

// The call of block `block`, 0 <= block < begin[n], n >= 1: the LAST k with begin[k] <= block (a call without blocks in
// this launch shares its start with the next one).
GKL_MS_HD int multi_find(const int32_t* __restrict__ begin, int n, int block) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block >= begin[mid]) lo = mid; else hi = mid;
  }
  return lo;
}
// ... and its index inside that call, and back.
GKL_MS_HD int multi_local(const int32_t* __restrict__ begin, int call, int block) { return block - begin[call]; }
GKL_MS_HD int multi_block(const int32_t* __restrict__ begin, int call, int local) { return begin[call] + local; }

}  // namespace gklhip
