// What a PDHMM call DECIDES before anything of it touches a stream: the packing of its reads into 64-lane chunks, its
// striped and tail jobs, the order and routing of its haplotypes, the table groups, the slices of a big paired call, the
// counts that size every launch -- for one call (PdCallPlan) and for several region calls that share one set of launches
// (PdMultiPlan) -- and the host-memory side of staging the job tables (pd_table_copies, pd_multi_fill_tables).  The
// launch paths (pdhmm_single_call.h, pdhmm_multi_call.h) hand it the context's settings and scratch and enqueue what it planned.
//
// Plain C++17, header-only: no device runtime, no context, no error state (tests/native/pdhmm_call_plan_check.cpp
// compiles it for the host alone, under the sanitizers, and re-derives every plan naively).
#pragma once
#include <immintrin.h>

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pairhmm_pair_forms.h"   // kPairLanes
#include "pairhmm_plan.h"         // PlanLane, blocks_for, pack_reads_windowed / _place, PackScratch
#include "pdhmm_job_layout.h"     // kPdRpl, kPdTabClasses, kPdSnp; pd_up, PdInputLayout, PdJobOffsets / PdJobLayout
#include "pdhmm_multi_plan.h"     // kPdMaxRegions, PdRegion, PdRegionShape, pd_build_regions

namespace gklhip {

// Shared by the two entry points.  Paired layout: n_read_items == n_hap_items == n_pairs, cross_haps = 0.
// Cross layout: n_pairs == n_read_items * n_hap_items, cross_haps = n_hap_items, pair p = (p / n_haps, p % n_haps).
struct PdProblem {
  int64_t n_pairs;
  int32_t n_read_items, n_hap_items, cross_haps, max_hap_len, max_read_len;
  const int8_t *hap_bases, *hap_pdbases, *read_bases, *read_qual, *read_ins_qual, *read_del_qual, *gcp;
  const int64_t *hap_lengths, *read_lengths;
  // cross layout, reference-tail mode: the reference cuts the read-major pair list into batches of this many pairs
  // (JavaData.h:83-101) and each batch has its own scalar tail; 0 = the whole cross product is one batch
  int64_t ref_batch_pairs;
  // a device-resident call (the C ABI's _compute_device / _cross_device): the seven byte arrays are HBM addresses on the
  // context's device -- no host code reads through them; the two length arrays are host arrays as always
  bool in_hbm = false;
};

// What the planner reads of the context's settings.
struct PdPlanSettings {
  int fma_mode, tail_mode, use_table, pipeline;
  bool asm_table;   // the whole-job asm table program is compiled in (GKL_PD_ASM == 2)
};
// What it keeps from call to call: a member of the context, so the vectors keep their capacity.
struct PdPlanScratch {
  std::vector<uint32_t> class_stamp;    // cross layout's class discovery: last haplotype that showed a (base, flags) pair
  uint32_t class_stamp_id = 0;
  PackScratch pack_scratch;
};

constexpr size_t kPdStageBytes = (size_t)4 << 20;
// Up to this many pairs (1 MB of sums) the kernels store the sums straight into pinned host memory (pd_plan_counts:
// sums_direct).  The host form of a multi-region call has no other way to return them, so this is also the most pairs a
// shared launch set takes (the device form, whose sums stay in HBM, keeps the same limit): both paths depend on the
// one constant.
constexpr size_t kPdMultiMaxPairs = 131072;
// Padded input bytes (haplotype bases + the five read arrays) from which a paired call of 65 536 pairs or more is cut
// into upload slices (pd_plan_slices), and from which a call too big to stage leaves its copies to a helper thread
// (PdUploads::start).
constexpr size_t kPdSliceMinBytes = (size_t)64 << 20, kPdHelperUploadBytes = (size_t)8 << 20;
// big paired calls are cut into slices of pairs whose kernels run while later slices still cross PCIe (pd_run_locked)
constexpr int kPdMaxSlices = 8;
static_assert(kPdLaneRowBytes == kPairLanes * sizeof(PlanLane), "pdhmm_job_layout.h sizes a lane row for this wavefront");

// Does a set of regions fit ONE multi-region launch set?  At most kPdMultiMaxPairs pairs and kPdStageBytes of inputs at
// the common row strides (and at most kPdMaxRegions regions: `count`, the caller's to compare).
struct PdMultiFit {
  size_t pairs = 0, nh = 0, nr = 0, mh = 0, mr = 0;
  int count = 0;
  void take(const PdProblem& q) {
    pairs += (size_t)q.n_pairs; nh += (size_t)q.n_hap_items; nr += (size_t)q.n_read_items;
    mh = std::max(mh, (size_t)q.max_hap_len); mr = std::max(mr, (size_t)q.max_read_len);
    count++;
  }
  bool fits() const { return pairs <= kPdMultiMaxPairs && PdInputLayout(nh, nr, mh, mr).total <= kPdStageBytes; }
  bool fits_with(const PdProblem& q) const { PdMultiFit with = *this; with.take(q); return with.fits(); }
};

// Does the haplotype hold a base outside ACGTN?  (Such columns need the byte-comparing step: the job goes to the full kernel.)
inline bool has_odd_base_scalar(const int8_t* b, int64_t n) {
  unsigned ok = 1;
  for (int64_t j = 0; j < n; j++)
    ok &= (unsigned)(b[j] == 'A') | (unsigned)(b[j] == 'C') | (unsigned)(b[j] == 'G') | (unsigned)(b[j] == 'T') | (unsigned)(b[j] == 'N');
  return !ok;
}
__attribute__((target("avx2"))) inline bool has_odd_base_avx2(const int8_t* b, int64_t n) {
  const __m256i cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'), cG = _mm256_set1_epi8('G'), cT = _mm256_set1_epi8('T'),
                cN = _mm256_set1_epi8('N');
  __m256i all = _mm256_set1_epi8((char)0xff);
  int64_t j = 0;
  for (; j + 32 <= n; j += 32) {
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(b + j));
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, cA), _mm256_cmpeq_epi8(v, cC)),
                                                       _mm256_or_si256(_mm256_cmpeq_epi8(v, cG), _mm256_cmpeq_epi8(v, cT))),
                                       _mm256_cmpeq_epi8(v, cN));
    all = _mm256_and_si256(all, ok);
  }
  if (_mm256_movemask_epi8(all) != -1) return true;
  return has_odd_base_scalar(b + j, n - j);
}
inline bool has_odd_base(const int8_t* b, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  return avx2 ? has_odd_base_avx2(b, n) : has_odd_base_scalar(b, n);
}

// Cross layout: reads are packed into 64-lane chunks by best fit within windows of this many reads.  The chunks are reused
// for every haplotype, so a fuller chunk pays off nh times: 2048 fills 99.2 % of the lanes on the reference's fixture
// (192, the paired layout's window: 97.7 %).
constexpr int kPdCrossWindow = 2048;
// The cross layout's plan of ONE region call (one computeLikelihoods cross product): the packing of its reads, the
// order and routing of its haplotypes, its striped reads and its tail pairs -- everything in the call's own indices.
// pd_run_locked launches one plan; pd_run_multi_locked concatenates several.
struct PdCrossPlan {
  std::vector<int32_t> job_pair, job_steps;    // listed jobs: one per (read that needs more than 64 lanes, haplotype)
  std::vector<uint8_t> job_striped;
  std::vector<PlanLane> cross_lanes;           // [chunk][64] = {read item, block}
  std::vector<int32_t> hap_order, chunk_steps, chunk_rep;
  size_t n_tail = 0;
  std::vector<PlanLane> tail_lanes;
  std::vector<int32_t> tail_pair, tail_steps;
  std::vector<uint8_t> tail_striped;
  std::vector<uint8_t> hap_ncls;
  std::vector<uint32_t> class_codes;
  size_t n_clean_haps = 0, n_tab_haps = 0;
};

// Appends the reference-tail job of one pair: a job of its own for the scalar-arithmetic launch (a lane row of the pair's
// row blocks, or a striped job when the read needs more than 64 lanes).
inline void pd_push_tail_job(PdCrossPlan* plan, int32_t pair, int read_len, int hap_len) {
  const int nb = blocks_for(read_len, kPdRpl);
  plan->tail_pair.push_back(pair);
  plan->tail_striped.push_back(nb > kPairLanes ? 1 : 0);
  plan->tail_steps.push_back(hap_len + std::min(nb, kPairLanes) - 1);
  plan->tail_lanes.resize(plan->tail_lanes.size() + kPairLanes, PlanLane{-1, 0});
  if (nb <= kPairLanes)
    for (int b = 0; b < nb; b++) plan->tail_lanes[plan->tail_lanes.size() - kPairLanes + (size_t)b] = PlanLane{pair, b};
  plan->n_tail = plan->tail_pair.size();
}

inline void pd_plan_cross_jobs(const PdPlanSettings& set, const PdProblem& q, PdCrossPlan* plan) {
  const size_t n = (size_t)q.n_pairs, nh = (size_t)q.n_hap_items, nr = (size_t)q.n_read_items;
  const int cross = q.cross_haps;
  auto read_len_of = [&](size_t p) { return (int)q.read_lengths[p / (size_t)cross]; };
  auto hap_len_of = [&](size_t p) { return (int)q.hap_lengths[p % (size_t)cross]; };
  auto &job_pair = plan->job_pair, &job_steps = plan->job_steps, &hap_order = plan->hap_order, &chunk_steps = plan->chunk_steps,
       &chunk_rep = plan->chunk_rep;
  auto& job_striped = plan->job_striped;
  auto& cross_lanes = plan->cross_lanes;
  // reads are packed into 64-lane chunks ONCE; every chunk meets every haplotype (longest haplotypes first).
  std::vector<int64_t> read_off(nr + 1, 0);
  for (size_t r = 0; r < nr; r++) read_off[r + 1] = read_off[r] + q.read_lengths[r];
  std::vector<int32_t> shorts;
  shorts.reserve(nr);
  for (size_t r = 0; r < nr; r++) {
    if (blocks_for((int)q.read_lengths[r], kPdRpl) <= kPairLanes) { shorts.push_back((int32_t)r); continue; }
    for (size_t h = 0; h < nh; h++) {  // a read that needs more than 64 lanes (64 x kPdRpl = 384 bases or more): one striped job per haplotype
      job_pair.push_back((int32_t)(r * nh + h)); job_striped.push_back(1); job_steps.push_back(0);
    }
  }
  const int made = pack_reads_windowed(shorts.data(), (int)shorts.size(), read_off.data(), kPdRpl, kPdCrossWindow, &cross_lanes, nullptr);
  chunk_steps.assign((size_t)made, 0);
  chunk_rep.assign((size_t)made, 0);
  for (int k = 0; k < made; k++) {
    const PlanLane* row = cross_lanes.data() + (size_t)k * kPairLanes;
    int32_t rep = -1, top = 0;
    for (int l = 0; l < kPairLanes; l++) {
      if (row[l].read < 0) continue;
      if (rep < 0) rep = row[l].read;
      top = std::max(top, row[l].block);
    }
    chunk_steps[(size_t)k] = top;
    chunk_rep[(size_t)k] = rep;
  }
  hap_order.resize(nh);
  for (size_t h = 0; h < nh; h++) hap_order[h] = (int32_t)h;
  std::stable_sort(hap_order.begin(), hap_order.end(),
                   [&](int32_t x, int32_t y) { return q.hap_lengths[x] > q.hap_lengths[y]; });
  // "Reference tail" of the cross product: computeLikelihoods expands it into read-major pairs, batch by batch
  // (JavaData.h:177-242), and computePDHMM finishes the last `batch mod SIMD width` pairs of EVERY batch with the
  // scalar engine (pdhmm.h:1264-1268).  The main launch computes all pairs with the vector arithmetic; the pairs at
  // those positions are then recomputed by the scalar-arithmetic instantiation and overwrite their sums.
  if (set.tail_mode == 1) {
    const size_t width = set.fma_mode ? 8 : 4;
    const size_t per = q.ref_batch_pairs > 0 ? (size_t)std::min<int64_t>(q.ref_batch_pairs, (int64_t)n) : n;
    for (size_t start = 0; start < n; start += per) {
      const size_t nb_pairs = std::min(per, n - start);
      for (size_t i = start + nb_pairs / width * width; i < start + nb_pairs; i++)
        pd_push_tail_job(plan, (int32_t)i, read_len_of(i), hap_len_of(i));
    }
  }
}

inline void pd_plan_cross_routing(const PdPlanSettings& set, PdPlanScratch* scratch, const PdProblem& q, PdCrossPlan* plan) {
  const size_t nh = (size_t)q.n_hap_items;
  const int cross = q.cross_haps;
  auto& hap_order = plan->hap_order;
  auto& hap_ncls = plan->hap_ncls;
  auto& class_codes = plan->class_codes;
  size_t &n_clean_haps = plan->n_clean_haps, &n_tab_haps = plan->n_tab_haps;
  std::vector<uint8_t> hap_odd;
  if (cross) {
    hap_odd.assign(nh, 0);
    for (size_t h = 0; h < nh; h++) hap_odd[h] = has_odd_base(q.hap_bases + h * (size_t)q.max_hap_len, q.hap_lengths[h]) ? 1 : 0;
  }
  n_clean_haps = nh; n_tab_haps = 0;
  // cross layout: a clean haplotype whose columns fall into at most kPdTabClasses classes of (base, SNP alleles, 'N')
  // goes to the table kernel (pdhmm_fwd_tab_kernel); class c of haplotype h has the match bits class_codes[8 h + c]
  if (cross) {
    hap_ncls.assign(nh, 0);
    class_codes.assign(nh * 8, 0u);
    for (size_t h = 0; h < nh && set.use_table; h++) {
      if (hap_odd[h]) continue;
      const int8_t* hb = q.hap_bases + h * (size_t)q.max_hap_len;
      const int8_t* pd = q.hap_pdbases + h * (size_t)q.max_hap_len;
      uint32_t* codes = class_codes.data() + h * 8;
      int ncls = 0;
      // (a column's class is a function of its (base, flags) pair: 2^15 of them, a haplotype shows a handful -- a stamp
      //  per pair and haplotype skips the columns whose pair has been seen; this loop was 0.06 of a region call's 0.33 ms)
      if (scratch->class_stamp.empty()) scratch->class_stamp.assign(1u << 15, 0u);
      if (++scratch->class_stamp_id == 0u) { std::fill(scratch->class_stamp.begin(), scratch->class_stamp.end(), 0u); scratch->class_stamp_id = 1u; }
      const uint32_t stamp_id = scratch->class_stamp_id;
      uint32_t* const stamp = scratch->class_stamp.data();
      for (int64_t j = 0; j < q.hap_lengths[h] && ncls <= kPdTabClasses; j++) {
        // (as pdhmm_entries_kernel builds the entry's match bits)
        const uint32_t yb = (uint32_t)hb[j] & 0xffu, flags = (uint32_t)pd[j] & 0x7fu;
        uint32_t& seen = stamp[(yb << 7) | flags];
        if (seen == stamp_id) continue;
        seen = stamp_id;
        const uint32_t hot = yb == (uint32_t)'A' ? 1u : yb == (uint32_t)'C' ? 2u : yb == (uint32_t)'G' ? 4u : yb == (uint32_t)'T' ? 8u : 0u;
        const uint32_t allele = (flags & kPdSnp) ? ((flags >> 3) & 0xfu) : 0u;
        const uint32_t code = (hot << 20) | (allele << 24) | (1u << 28) | (yb == (uint32_t)'N' ? 1u << 29 : 0u);
        int k = 0;
        while (k < ncls && codes[k] != code) k++;
        if (k == ncls) {
          if (ncls < kPdTabClasses) codes[ncls] = code;
          ncls++;
        }
      }
      hap_ncls[h] = ncls <= kPdTabClasses ? (uint8_t)ncls : 0;
    }
    // order: table haplotypes, then the other clean ones, then those with odd bases (each group longest first)
    std::stable_partition(hap_order.begin(), hap_order.end(), [&](int32_t h) { return hap_odd[(size_t)h] == 0; });
    n_clean_haps = 0;
    for (size_t h = 0; h < nh; h++) n_clean_haps += hap_odd[h] == 0;
    std::stable_partition(hap_order.begin(), hap_order.begin() + (ptrdiff_t)n_clean_haps, [&](int32_t h) { return hap_ncls[(size_t)h] != 0; });
    for (size_t h = 0; h < nh; h++) n_tab_haps += hap_ncls[h] != 0;
    // The haplotypes of one region share their variant sites, hence their column classes: when the union of the table
    // haplotypes' classes still fits the table, every one of them gets the union as its list -- a wavefront that takes
    // several haplotypes with the same chunk of reads (tab_group_start below) then builds the table once.
    {
      uint32_t uni[kPdTabClasses + 1];
      int n_uni = 0;
      for (size_t h = 0; h < nh && n_uni <= kPdTabClasses; h++)
        for (int k = 0; k < (int)hap_ncls[h] && n_uni <= kPdTabClasses; k++) {
          const uint32_t code = class_codes[h * 8 + (size_t)k];
          int at = 0;
          while (at < n_uni && uni[at] != code) at++;
          if (at == n_uni) { if (n_uni < kPdTabClasses) uni[n_uni] = code; n_uni++; }
        }
      if (n_uni <= kPdTabClasses)
        for (size_t h = 0; h < nh; h++)
          if (hap_ncls[h]) { for (int k = 0; k < n_uni; k++) class_codes[h * 8 + (size_t)k] = uni[k]; hap_ncls[h] = (uint8_t)n_uni; }
    }
  }
}

// Table launch: a unit of work is (a group of consecutive table haplotypes of ONE region, a chunk of reads) -- the wavefront
// sets the chunk's rows up once per group (a twelfth of a job's time otherwise).  Groups of up to six while the launch has at
// least six units per wavefront -- sized by the units of the WHOLE launch: many small regions together fill the device, so
// they get the full groups a single one would not -- shrinking to single haplotypes over the last part of the launch's list
// (they run last and even the load out).  n_tab_haps[k]: the table haplotypes of region k (a single call: one count);
// n_cross_tab: the launch's (haplotype, chunk) jobs.  Fills tab_group_start (`start`, empty before) -- group g = entries
// [start[g], start[g + 1]) of the launch's haplotype list -- and groups[k], when asked for: the number of region k's groups.
inline void pd_size_tab_groups(const size_t* n_tab_haps, int K, int64_t n_cross_tab, std::vector<int32_t>* start, int32_t* groups) {
  const int64_t per_wave = n_cross_tab / (256 * 8);
  const size_t group_max = (size_t)std::max<int64_t>(1, std::min<int64_t>(6, per_wave / 6));
  size_t left = 0, at = 0;
  for (int k = 0; k < K; k++) left += n_tab_haps[k];
  for (int k = 0; k < K; k++) {
    const size_t mine = n_tab_haps[k];
    int32_t made = 0;
    for (size_t i = 0; i < mine; made++) {
      const size_t g = std::max<size_t>(1, std::min(std::min(group_max, left / 7), mine - i));
      start->push_back((int32_t)(at + i));
      i += g; left -= g;
    }
    at += mine;
    if (groups) groups[k] = made;
  }
  start->push_back((int32_t)at);
}

// ==== a single call: the plan.  Everything the call decides before anything of it touches the stream, on the caller's stack. ====
struct PdCallPlan {
  // A big PAIRED call (computePDHMMNative: ~1.2 KB of padded input per pair -- the x32 fixture is 498 MB, 9.5 ms of PCIe
  // against 5 ms of kernels) is cut into slices of consecutive pairs, biggest first: the helper thread sends slice after
  // slice on the upload stream and records an event behind each; the kernels of a slice -- its pairs are packed among
  // themselves -- wait for that event only, so they run while the later slices still cross the bus, and the last,
  // smallest slice leaves little to do once the bus is done.  Everything else about the call is one problem: one set of
  // device arrays, one job list (slice k = a range of listed jobs), the rare striped / odd-base / tail jobs at the end.
  int n_slices = 1;
  size_t slice_lo[kPdMaxSlices + 1] = {};        // slice k = pairs [slice_lo[k], slice_lo[k + 1])
  int32_t slice_chunk0[kPdMaxSlices + 1] = {};   // ... = chunks [slice_chunk0[k], slice_chunk0[k + 1]) = listed jobs n_striped + those
  // A call of the fixture's size (276 reads x 48 haplotypes) spent half its time in two dozen small copies from
  // pageable memory (~10 us each): up to kPdStageBytes the arrays are gathered in a pinned block and travel in ONE copy.
  bool staged = false;
  std::vector<int32_t> place_chunk;            // paired layout: compact packing of the pairs (pack_reads_place)
  std::vector<uint8_t> place_lane, chunk_used;
  size_t n_striped = 0;                        // paired layout: the first listed jobs are the striped ones
  PdCrossPlan x;                               // cross layout: pd_plan_cross_jobs / _routing; paired layout: its listed and tail jobs (pd_plan_paired_jobs)
  std::vector<int32_t> tab_group_start;        // (table launch; see pd_size_tab_groups)
  // the full launch's list of listed jobs: the striped ones (the first n_striped in the paired layout, all of them in
  // the cross layout) from here, flagged packed jobs appended by pdhmm_collect_kernel; its length lives in misc[kPdMiscFullCount]
  std::vector<int32_t> full_first;
  int32_t n_striped_listed = 0;                // (lives, like the vectors, until the stream is drained)
  // the counts (pd_plan_counts)
  size_t n_clean_haps = 0, n_packed = 0;       // haplotypes without an odd base (paired: every item); paired layout's packed jobs
  int n_chunks_cross = 0, n_general = 0, n_cross_jobs = 0, n_cross_tab = 0, n_tab_units = 0, n_cross_hot = 0, n_jobs = 0;
  int entry_stride = 0, n_blocks = 0;
  bool tab_paired = false, tab_paired_asm = false;
  bool sums_direct = false;                    // the kernels store the sums straight into pinned host memory
  bool paired_packed() const { return !chunk_used.empty(); }   // a paired call with at least one packed chunk: pd_launch_paired
  PdJobCounts job_counts() const {
    return PdJobCounts{(size_t)n_general, (size_t)n_chunks_cross, x.hap_order.size(), x.n_tail, place_chunk.size(), chunk_used.size(), tab_group_start.size()};
  }
};

inline void pd_plan_slices(const PdPlanSettings& set, const PdProblem& q, const PdInputLayout& in, PdCallPlan* p) {
  const size_t n = (size_t)q.n_pairs;
  p->staged = !q.in_hbm && in.total <= kPdStageBytes;   // (inputs in HBM: never through host memory, and no bus to hide: one slice)
  p->n_slices = 1;
  p->slice_lo[0] = 0; p->slice_lo[1] = n;
  if (!q.in_hbm && !q.cross_haps && set.pipeline && n >= 65536 && in.hap_bytes + 5 * in.read_bytes >= kPdSliceMinBytes) {
    static const double kShare[] = {0.28, 0.24, 0.19, 0.13, 0.09, 0.05, 0.02};
    p->n_slices = (int)(sizeof kShare / sizeof kShare[0]);
    double acc = 0.0;
    for (int k = 0; k < p->n_slices; k++) { p->slice_lo[k] = (size_t)(acc * (double)n) / 64 * 64; acc += kShare[k]; }
    p->slice_lo[p->n_slices] = n;
  }
}

// The paired layout's jobs: the tail pairs, the striped pairs, then the packed chunks slice by slice.
inline void pd_plan_paired_jobs(const PdPlanSettings& set, PdPlanScratch* scratch, const PdProblem& q, PdCallPlan* p) {
  const size_t n = (size_t)q.n_pairs;
  auto read_len_of = [&](size_t i) { return (int)q.read_lengths[i]; };
  auto hap_len_of = [&](size_t i) { return (int)q.hap_lengths[i]; };
  PdCrossPlan& x = p->x;
  // "Reference tail": GKL finishes the last `batch mod SIMD width` pairs of every vector batch with its SCALAR
  // engine (pdhmm.h:1264-1270; 8 doubles per AVX-512 vector, 4 per AVX2 vector), whose arithmetic differs in the
  // last bits (and, with deletions at a haplotype's end, by more).  In that mode those pairs get jobs of their own,
  // run by the scalar-arithmetic instantiation of the kernel.
  const size_t n_vec = n - (set.tail_mode == 1 ? n % (size_t)(set.fma_mode ? 8 : 4) : 0);
  for (size_t i = n_vec; i < n; i++) pd_push_tail_job(&x, (int32_t)i, read_len_of(i), hap_len_of(i));
  // short pairs, ordered by haplotype length so that wavefront mates finish together, are packed best-fit
  // into 64-lane chunks; a read that needs more than 64 lanes becomes a striped job
  std::vector<int64_t> pair_off(n + 1, 0);  // pack_reads_windowed() addresses reads through offsets
  for (size_t i = 0; i < n; i++) pair_off[i + 1] = pair_off[i] + read_len_of(i);
  for (size_t i = 0; i < n_vec; i++) {
    if (blocks_for(read_len_of(i), kPdRpl) <= kPairLanes) continue;
    x.job_pair.push_back((int32_t)i); x.job_striped.push_back(1); x.job_steps.push_back(0);  // (a striped job's lane row stays unused)
  }
  // compact packing (5 bytes per pair); pdhmm_expand_kernel turns it into the lane rows on the device.  Slice by slice
  // (one slice: the whole batch): the pairs of a slice share chunks among themselves only, chunk numbers run on.
  const size_t n_striped = p->n_striped = x.job_pair.size();
  p->place_chunk.assign(n, -1);
  p->place_lane.assign(n, 0);
  std::vector<int32_t> shorts, cnt;
  shorts.reserve(n);
  for (int k = 0; k < p->n_slices; k++) {
    const size_t lo = std::min(p->slice_lo[k], n_vec), hi = std::min(p->slice_lo[k + 1], n_vec);
    p->slice_chunk0[k] = (int32_t)p->chunk_used.size();
    // counting sort by haplotype length, longest first (the big jobs start first)
    cnt.assign((size_t)q.max_hap_len + 2, 0);
    size_t n_short = 0;
    for (size_t i = lo; i < hi; i++)
      if (blocks_for(read_len_of(i), kPdRpl) <= kPairLanes) { cnt[(size_t)hap_len_of(i)]++; n_short++; }
    int32_t acc = 0;
    for (int64_t h = q.max_hap_len; h >= 0; h--) { const int32_t m = cnt[(size_t)h]; cnt[(size_t)h] = acc; acc += m; }
    shorts.resize(n_short);
    for (size_t i = lo; i < hi; i++)
      if (blocks_for(read_len_of(i), kPdRpl) <= kPairLanes) shorts[(size_t)cnt[(size_t)hap_len_of(i)]++] = (int32_t)i;
    const int made = pack_reads_place(shorts.data(), (int)shorts.size(), pair_off.data(), kPdRpl, 192, p->place_chunk.data(),
                                      p->place_lane.data(), &p->chunk_used, nullptr, &scratch->pack_scratch);
    const size_t j0 = n_striped + (size_t)p->slice_chunk0[k];
    x.job_pair.resize(j0 + (size_t)made, -1);
    x.job_steps.resize(j0 + (size_t)made, 0);
    x.job_striped.resize(j0 + (size_t)made, 0);
    for (const int32_t i : shorts) {
      const size_t j = n_striped + (size_t)p->place_chunk[(size_t)i];
      if (x.job_pair[j] < 0) x.job_pair[j] = i;
      x.job_steps[j] = std::max(x.job_steps[j], (int32_t)(hap_len_of((size_t)i) + blocks_for(read_len_of((size_t)i), kPdRpl) - 1));
    }
  }
  p->slice_chunk0[p->n_slices] = (int32_t)p->chunk_used.size();
}

// The figures that follow from the jobs and the routing: what every launch is sized by.  false: too many jobs for the
// kernels' 32-bit job numbers (nothing else of the plan is then filled in).
inline bool pd_plan_counts(const PdPlanSettings& set, const PdProblem& q, PdCallPlan* p) {
  const int cross = q.cross_haps;
  const size_t n = (size_t)q.n_pairs, nh = (size_t)q.n_hap_items, n_tab_haps = p->x.n_tab_haps;
  p->n_clean_haps = cross ? p->x.n_clean_haps : nh;
  p->n_chunks_cross = (int)p->x.chunk_steps.size();
  const int64_t n_cross_jobs64 = (int64_t)p->n_chunks_cross * (int64_t)(cross ? nh : 0);
  if (n_cross_jobs64 + (int64_t)p->x.job_pair.size() > 0x7fffffffLL) return false;
  p->n_cross_jobs = (int)n_cross_jobs64;
  p->n_cross_tab = cross ? (int)((int64_t)p->n_chunks_cross * (int64_t)n_tab_haps) : 0;
  if (p->n_cross_tab > 0) pd_size_tab_groups(&n_tab_haps, 1, p->n_cross_tab, &p->tab_group_start, nullptr);
  p->n_tab_units = p->tab_group_start.empty() ? 0 : (int)((int64_t)p->n_chunks_cross * (int64_t)(p->tab_group_start.size() - 1));
  p->n_cross_hot = cross ? (int)((int64_t)p->n_chunks_cross * (int64_t)(p->n_clean_haps - n_tab_haps)) : 0;
  p->n_general = (int)p->x.job_pair.size();
  p->n_jobs = p->n_cross_jobs + p->n_general;
  p->entry_stride = (q.max_hap_len + 2 * kPairLanes + 4 + 63) / 64 * 64;   // 64 idle, the columns, 63 skew + 4 look-ahead
  p->n_blocks = std::max(1, std::min(std::max(p->n_jobs, (int)p->x.n_tail), 256 * 8));
  // Paired layout through the table kernel (pdhmm_fwd_tab_paired_kernel): classes, special columns and the routing of the
  // jobs are found on the device.  Needs the program's 32-bit entry offsets to reach every item's stream and the step
  // marks of a job to fit the special kernel's LDS.
  p->n_packed = cross ? 0 : (size_t)p->n_general - p->n_striped;
  p->tab_paired = !cross && set.use_table && p->n_packed > 0 && nh * (size_t)p->entry_stride * 4 < ((size_t)1 << 32) && p->entry_stride <= 12 * 1024;
  p->tab_paired_asm = p->tab_paired && set.fma_mode == 1 && set.asm_table;   // (the C++ step loops ballot on the lanes' own entries)
  // A region-sized call (up to kPdMultiMaxPairs = 1 MB of sums): the kernels store the sums -- write-only, one store per pair --
  // straight into the pinned host block (posted writes over PCIe) instead of a device array that a copy then fetches: one
  // copy launch (~15 us of a 0.28 ms call) less.
  p->sums_direct = !q.in_hbm && n <= kPdMultiMaxPairs;   // (a device-resident call: the sums stay in the device array for pdhmm_finalise_kernel)
  p->n_striped_listed = cross ? p->n_general : (int32_t)p->n_striped;
  p->full_first.resize((size_t)p->n_striped_listed);
  for (int32_t k = 0; k < p->n_striped_listed; k++) p->full_first[(size_t)k] = k;
  return true;
}

// The single call's job tables as copies into its block of PdJobLayout, in the order they are made; the last one, the
// head of the full launch's list, goes behind the clears of pd_stage_tables.  The sources live in the plan.
struct PdTableCopy {
  size_t offset;     // of the table in the block
  const void* src;
  size_t bytes;      // 0: nothing to copy
};
using PdTableCopies = std::array<PdTableCopy, 18>;
inline PdTableCopies pd_table_copies(const PdCallPlan& p, const PdJobLayout& L) {
  const PdCrossPlan& x = p.x;
  const size_t n_general = (size_t)p.n_general;
  return {{{L.jp, x.job_pair.data(), n_general * 4}, {L.jn, x.job_steps.data(), n_general * 4}, {L.js, x.job_striped.data(), n_general},
           {L.cl, x.cross_lanes.data(), x.cross_lanes.size() * sizeof(PlanLane)}, {L.ho, x.hap_order.data(), x.hap_order.size() * 4},
           {L.cs, x.chunk_steps.data(), x.chunk_steps.size() * 4}, {L.cr, x.chunk_rep.data(), x.chunk_rep.size() * 4},
           {L.tl, x.tail_lanes.data(), x.tail_lanes.size() * sizeof(PlanLane)}, {L.tp, x.tail_pair.data(), x.n_tail * 4},
           {L.tn, x.tail_steps.data(), x.n_tail * 4}, {L.ts, x.tail_striped.data(), x.n_tail},
           {L.nc, x.hap_ncls.data(), x.hap_ncls.size()}, {L.cc, x.class_codes.data(), x.class_codes.size() * 4},
           {L.pc, p.place_chunk.data(), p.place_chunk.size() * 4}, {L.pl, p.place_lane.data(), p.place_lane.size()},
           {L.cu, p.chunk_used.data(), p.chunk_used.size()}, {L.tg, p.tab_group_start.data(), p.tab_group_start.size() * 4},
           {L.fj, p.full_first.data(), p.full_first.size() * 4}}};
}

// ==== several region calls in one set of launches: the plan ====
// The set's totals and its input layout: one common row stride per side.
struct PdMultiShape {
  size_t NH = 0, NR = 0, NP = 0, mh = 0, mr = 0;
  explicit PdMultiShape(const std::vector<PdProblem>& Q) {
    for (const PdProblem& q : Q) {
      NH += (size_t)q.n_hap_items; NR += (size_t)q.n_read_items; NP += (size_t)q.n_pairs;
      mh = std::max(mh, (size_t)q.max_hap_len); mr = std::max(mr, (size_t)q.max_read_len);
    }
  }
  PdInputLayout layout() const { return PdInputLayout(NH, NR, mh, mr); }
};

// Every region planned exactly as a single call is planned, then the region table.
struct PdMultiPlan {
  std::vector<PdCrossPlan> plans;
  std::vector<PdRegion> regions;          // K + 1 (pd_build_regions)
  std::vector<int32_t> tab_group_start;
  size_t n_tab_haps = 0, n_hot_haps = 0, n_full_haps = 0, n_chunks = 0, n_general = 0, n_tail = 0;
  int n_tab_units = 0, n_hot_units = 0, n_full_units = 0, entry_stride = 0, n_blocks = 0;
};
// Q[k]: region k's problem as the planners may read it (the device form: its haplotype arrays are the pinned copies).
inline void pd_multi_plan(const PdPlanSettings& set, PdPlanScratch* scratch, const std::vector<PdProblem>& Q, const PdMultiShape& sh, PdMultiPlan* p) {
  const int K = (int)Q.size();
  p->plans.resize((size_t)K);
  std::vector<PdRegionShape> shapes((size_t)K);
  std::vector<size_t> tab_haps((size_t)K);
  std::vector<int32_t> groups((size_t)K);
  int64_t n_cross_tab = 0;   // (haplotype, chunk) jobs of the table launch
  for (int k = 0; k < K; k++) {
    const PdProblem& q = Q[(size_t)k];
    pd_plan_cross_jobs(set, q, &p->plans[(size_t)k]);
    pd_plan_cross_routing(set, scratch, q, &p->plans[(size_t)k]);
    const PdCrossPlan& pl = p->plans[(size_t)k];
    tab_haps[(size_t)k] = pl.n_tab_haps;
    p->n_tab_haps += pl.n_tab_haps; p->n_hot_haps += pl.n_clean_haps - pl.n_tab_haps; p->n_full_haps += (size_t)q.n_hap_items - pl.n_clean_haps;
    p->n_chunks += pl.chunk_steps.size(); p->n_general += pl.job_pair.size(); p->n_tail += pl.n_tail;
    n_cross_tab += (int64_t)pl.chunk_steps.size() * (int64_t)pl.n_tab_haps;
  }
  pd_size_tab_groups(tab_haps.data(), K, n_cross_tab, &p->tab_group_start, groups.data());
  for (int k = 0; k < K; k++) {
    const PdProblem& q = Q[(size_t)k];
    const PdCrossPlan& pl = p->plans[(size_t)k];
    shapes[(size_t)k] = PdRegionShape{q.n_read_items, q.n_hap_items, (int32_t)pl.chunk_steps.size(),
                                      {groups[(size_t)k], (int32_t)(pl.n_clean_haps - pl.n_tab_haps), (int32_t)((size_t)q.n_hap_items - pl.n_clean_haps)}};
  }
  p->regions.resize((size_t)K + 1);
  pd_build_regions(shapes.data(), K, p->regions.data());
  p->n_tab_units = p->regions[(size_t)K].unit_start[kPdLaunchTab];
  p->n_hot_units = p->regions[(size_t)K].unit_start[kPdLaunchHot];
  p->n_full_units = p->regions[(size_t)K].unit_start[kPdLaunchFull];
  p->entry_stride = ((int)sh.mh + 2 * kPairLanes + 4 + 63) / 64 * 64;
  const int n_jobs_max = std::max(std::max(p->n_tab_units, p->n_hot_units), p->n_full_units + (int)p->n_general);
  p->n_blocks = std::max(1, std::min(std::max(n_jobs_max, (int)p->n_tail), 256 * 8));
}

// A multi-region call's block in `jobs`: the region table (rg), the launches' haplotype lists (ho), the length of the
// full launch's list (fc) and the tables of PdJobOffsets; everything but the lane rows of the listed jobs (jl: striped
// jobs, their rows stay unused) is staged in one pinned block.
struct PdMultiJobLayout : PdJobOffsets {
  size_t rg, ho, fc, staged_total, total;
  PdMultiJobLayout(size_t K, size_t NH, const PdMultiPlan& p) {
    const size_t n_chunks = p.n_chunks, n_general = p.n_general, n_tail = p.n_tail;
    rg = 0; cl = rg + pd_up((K + 1) * sizeof(PdRegion)); cs = cl + pd_up(n_chunks * kPairLanes * sizeof(PlanLane));
    cr = cs + pd_up(n_chunks * 4); ho = cr + pd_up(n_chunks * 4); tg = ho + pd_up(NH * 4);
    nc = tg + pd_up(p.tab_group_start.size() * 4); cc = nc + pd_up(NH); jp = cc + pd_up(NH * 32); jn = jp + pd_up(n_general * 4);
    js = jn + pd_up(n_general * 4); jf = js + pd_up(n_general); fj = jf + pd_up(n_general); fc = fj + pd_up(n_general * 4);
    tl = fc + 256; tp = tl + pd_up(n_tail * kPairLanes * sizeof(PlanLane)); tn = tp + pd_up(n_tail * 4);
    ts = tn + pd_up(n_tail * 4); staged_total = ts + pd_up(n_tail);
    jl = staged_total; total = jl + pd_up(n_general * kPairLanes * sizeof(PlanLane));
  }
};

// The regions' plans, shifted to the concatenated indices, into the staged part of the block: `hj` holds
// L.staged_total bytes, and nothing beyond them is written.
inline void pd_multi_fill_tables(const PdMultiPlan& p, const PdMultiJobLayout& L, unsigned char* hj) {
  const int K = (int)p.plans.size();
  const size_t n_general = p.n_general;
  memcpy(hj + L.rg, p.regions.data(), ((size_t)K + 1) * sizeof(PdRegion));
  memcpy(hj + L.tg, p.tab_group_start.data(), p.tab_group_start.size() * 4);
  PlanLane* cl = reinterpret_cast<PlanLane*>(hj + L.cl);
  int32_t *cs = reinterpret_cast<int32_t*>(hj + L.cs), *cr = reinterpret_cast<int32_t*>(hj + L.cr);
  int32_t* ho = reinterpret_cast<int32_t*>(hj + L.ho);   // [table launch's list | predicate launch's | byte-comparing launch's]
  int32_t *ho_tab = ho, *ho_hot = ho + p.n_tab_haps, *ho_full = ho + p.n_tab_haps + p.n_hot_haps;
  uint8_t* nc = hj + L.nc;
  uint32_t* cc = reinterpret_cast<uint32_t*>(hj + L.cc);
  int32_t *jp = reinterpret_cast<int32_t*>(hj + L.jp), *fj = reinterpret_cast<int32_t*>(hj + L.fj);
  PlanLane* tl = reinterpret_cast<PlanLane*>(hj + L.tl);
  int32_t *tp = reinterpret_cast<int32_t*>(hj + L.tp), *tn = reinterpret_cast<int32_t*>(hj + L.tn);
  uint8_t* ts = hj + L.ts;
  memset(hj + L.js, 1, n_general);
  memset(hj + L.jf, 0, n_general);
  memset(hj + L.jn, 0, n_general * 4);   // (job_steps: unused by striped jobs)
  for (size_t j = 0; j < n_general; j++) fj[j] = (int32_t)j;
  *reinterpret_cast<int32_t*>(hj + L.fc) = (int32_t)n_general;
  for (int k = 0; k < K; k++) {
    const PdCrossPlan& pl = p.plans[(size_t)k];
    const PdRegion& rg = p.regions[(size_t)k];
    for (const PlanLane& l : pl.cross_lanes) *cl++ = PlanLane{l.read < 0 ? -1 : l.read + rg.read_base, l.block};
    for (const int32_t v : pl.chunk_steps) *cs++ = v;
    for (const int32_t v : pl.chunk_rep) *cr++ = v + rg.read_base;
    const size_t nh = (size_t)rg.n_haps;
    for (size_t i = 0; i < nh; i++) {
      int32_t*& dst = i < pl.n_tab_haps ? ho_tab : i < pl.n_clean_haps ? ho_hot : ho_full;
      *dst++ = pl.hap_order[i] + rg.hap_base;
    }
    memcpy(nc, pl.hap_ncls.data(), nh); nc += nh;
    memcpy(cc, pl.class_codes.data(), nh * 32); cc += nh * 8;
    for (const int32_t v : pl.job_pair) *jp++ = v + rg.pair_base;
    for (const PlanLane& l : pl.tail_lanes) *tl++ = PlanLane{l.read < 0 ? -1 : l.read + rg.pair_base, l.block};
    for (const int32_t v : pl.tail_pair) *tp++ = v + rg.pair_base;
    for (const int32_t v : pl.tail_steps) *tn++ = v;
    for (const uint8_t v : pl.tail_striped) *ts++ = v;
  }
}

}  // namespace gklhip
