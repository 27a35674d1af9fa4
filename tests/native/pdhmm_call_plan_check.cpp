// Stand-alone check of gkl_amd/csrc/pdhmm_call_plan.h (tests/test_pdhmm_call_plan_cpu.py builds it, with
// gkl_amd/csrc/pairhmm_plan.cpp, under -fsanitize=address,undefined and expects exit 0).  Every fact below is re-derived
// naively -- no stamp table, no counting sort, no best-fit packer -- and compared with what the planner made, for
// fma_mode 0 and 1 (SIMD width 4 and 8) and tail_mode 0 and 1:
//   odd bases     has_odd_base against the scalar form and a plain scan, lengths 0..70, one foreign byte at every position
//   cross plan    every short read in exactly one chunk on consecutive lanes, chunk_steps / chunk_rep, one striped job per
//                 (long read, haplotype); read lengths 1, kPdRpl - 1, kPdRpl, 64 kPdRpl - 1 (packed), 64 kPdRpl (striped);
//                 regions of striped reads only; 2049 short reads (one packing window crossed)
//   routing       hap_order = [table | other clean | odd], each longest first and stable; class lists against a column by
//                 column recount; the union rule both ways; use_table = 0; the same plan twice from one scratch, across
//                 the wrap of class_stamp_id
//   tail jobs     the last `batch mod width` pairs of every reference batch, both layouts; lane rows, steps, striped flags
//   paired plan   placement, chunk_used, job_steps / job_pair, slices kept apart; pd_plan_slices through its inputs
//   table groups  pd_size_tab_groups: cover, sizes 1..6, no group across a region, the counts; K = 1 as pd_plan_counts
//   multi plan    PdMultiJobLayout's blocks; pd_multi_fill_tables into a block of exactly staged_total bytes, then every
//                 launch's work enumerated with the kernel's index functions against the K single-region plans; K = 1
//                 field by field; pd_table_copies executed into a block of exactly PdJobLayout::total bytes
// Every buffer a fill function writes into is a heap block of exactly the layout's size: one byte beyond is ASan's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "../../gkl_amd/csrc/pdhmm_call_plan.h"

using namespace gklhip;

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed: ", __func__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      return false;                                                          \
    }                                                                        \
  } while (0)

namespace {
constexpr int kLongRead = kPairLanes * kPdRpl;   // the shortest striped read (384); one base less still fits 64 lanes

struct Counts {
  long long regions = 0, striped_reads = 0, table_haps = 0, odd_haps = 0, tail_jobs = 0, striped_tails = 0, sliced_plans = 0,
            union_shared = 0, union_kept = 0, paired_plans = 0, multi_sets = 0, grouped = 0;
} g;

std::mt19937 rng(20250311u);
int pick(int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); }

// One region's (or one paired batch's) planner inputs: the haplotype bytes and both length arrays, each a heap block of
// exactly its size.  The planner reads nothing else.
struct Inputs {
  int nr = 0, nh = 0, mh = 0, mr = 0;
  std::unique_ptr<int8_t[]> hb, pd;
  std::unique_ptr<int64_t[]> hl, rl;
  PdProblem cross(int64_t ref_batch_pairs) const {
    return PdProblem{(int64_t)nr * nh, nr, nh, nh, mh, mr, hb.get(), pd.get(), nullptr, nullptr, nullptr, nullptr, nullptr, hl.get(), rl.get(), ref_batch_pairs};
  }
  PdProblem paired() const {   // nr == nh
    return PdProblem{nr, nr, nr, 0, mh, mr, hb.get(), pd.get(), nullptr, nullptr, nullptr, nullptr, nullptr, hl.get(), rl.get(), 0};
  }
};
// hap_kind: 0 the four bases; 1 up to kPdTabClasses classes ('N', a SNP allele); 2 more than kPdTabClasses classes;
// 3 a base outside ACGTN; -1 any.  read_len(r): the length of read r.
template <typename ReadLen>
Inputs make_inputs(int nr, int nh, int mh, ReadLen read_len, int hap_kind = -1, bool same_len_haps = false) {
  Inputs in;
  in.nr = nr; in.nh = nh; in.mh = mh;
  in.rl.reset(new int64_t[(size_t)nr]);
  for (int r = 0; r < nr; r++) { in.rl[r] = read_len(r); in.mr = std::max(in.mr, (int)in.rl[r]); }
  in.hl.reset(new int64_t[(size_t)nh]);
  in.hb.reset(new int8_t[(size_t)nh * mh]);
  in.pd.reset(new int8_t[(size_t)nh * mh]);
  const int alleles = pick(1, 15);   // the region's SNP alleles (haplotypes of one region share their variant sites)
  for (int h = 0; h < nh; h++) {
    const int len = same_len_haps ? mh : pick(1, mh), kind = hap_kind >= 0 ? hap_kind : pick(0, 3);
    in.hl[h] = len;
    for (int j = 0; j < mh; j++) {
      int8_t base = "ACGT"[pick(0, 3)];
      int flags = pick(0, 3) == 0 ? (pick(0, 1) ? kPdDelStart : kPdDelEnd) : 0;   // (same class, another (base, flags) pair)
      if (kind >= 1 && pick(0, 9) == 0) base = 'N';
      if (kind == 1 && base == 'A' && pick(0, 4) == 0) flags |= kPdSnp | (alleles << 3);   // A C G T N and A with the alleles: six
      if (kind == 2 && pick(0, 3) == 0) flags |= kPdSnp | (pick(1, 15) << 3);
      if (kind == 3 && (j == len - 1 || pick(0, 19) == 0)) base = (int8_t)"XRYacgt*\x00\xff"[pick(0, 9)];
      in.hb[(size_t)h * mh + j] = base;
      in.pd[(size_t)h * mh + j] = (int8_t)flags;
    }
  }
  return in;
}

bool naive_odd(const int8_t* b, int64_t n) {
  for (int64_t j = 0; j < n; j++)
    if (!std::strchr("ACGTN", b[j]) || b[j] == 0) return true;
  return false;
}
// The match bits of one column, as pdhmm_entries_kernel builds them.
uint32_t naive_code(int8_t base, int8_t pdflags) {
  const uint32_t yb = (uint8_t)base, flags = (uint8_t)pdflags & 0x7fu;
  uint32_t code = 1u << 28;
  if (yb == 'A') code |= 1u << 20;
  if (yb == 'C') code |= 2u << 20;
  if (yb == 'G') code |= 4u << 20;
  if (yb == 'T') code |= 8u << 20;
  if (yb == 'N') code |= 1u << 29;
  if (flags & kPdSnp) code |= ((flags >> 3) & 0xfu) << 24;
  return code;
}
std::set<uint32_t> naive_classes(const PdProblem& q, int h) {
  std::set<uint32_t> s;
  for (int64_t j = 0; j < q.hap_lengths[h]; j++) s.insert(naive_code(q.hap_bases[(size_t)h * q.max_hap_len + j], q.hap_pdbases[(size_t)h * q.max_hap_len + j]));
  return s;
}
// The tail pairs of a problem: the last `batch mod width` pairs of every reference batch.
std::vector<int32_t> naive_tails(const PdPlanSettings& set, const PdProblem& q) {
  std::vector<int32_t> t;
  if (set.tail_mode != 1) return t;
  const int64_t n = q.n_pairs, width = set.fma_mode ? 8 : 4;
  const int64_t per = q.cross_haps && q.ref_batch_pairs > 0 ? std::min(q.ref_batch_pairs, n) : n;
  for (int64_t p = 0; p < n; p++) {
    const int64_t start = p / per * per, size = std::min(per, n - start);
    if (p - start >= size - size % width) t.push_back((int32_t)p);
  }
  return t;
}

bool check_odd_bases() {
  const char foreign[] = {'X', 'a', 'n', '\0', (char)0xff, '@', 'B', 'U'};
  for (int len = 0; len <= 70; len++)
    for (int pos = -1; pos < len; pos++) {
      std::unique_ptr<int8_t[]> b(new int8_t[(size_t)len]);
      for (int j = 0; j < len; j++) b[j] = "ACGTN"[(j + len) % 5];
      if (pos >= 0) b[pos] = foreign[(pos + len) % 8];
      const bool want = pos >= 0;
      CHECK(has_odd_base(b.get(), len) == want && has_odd_base_scalar(b.get(), len) == want && naive_odd(b.get(), len) == want,
            "length %d, foreign byte at %d", len, pos);
      if (__builtin_cpu_supports("avx2")) CHECK(has_odd_base_avx2(b.get(), len) == want, "avx2: length %d, foreign byte at %d", len, pos);
    }
  return true;
}

bool check_tails(const PdPlanSettings& set, const PdProblem& q, const PdCrossPlan& x) {
  const std::vector<int32_t> want = naive_tails(set, q);
  CHECK(x.n_tail == want.size() && x.tail_pair == want, "%zu tail jobs, %zu expected (n %lld, batches of %lld)", x.n_tail, want.size(),
        (long long)q.n_pairs, (long long)q.ref_batch_pairs);
  CHECK(x.tail_steps.size() == x.n_tail && x.tail_striped.size() == x.n_tail && x.tail_lanes.size() == x.n_tail * kPairLanes, "tail tables of %zu jobs", x.n_tail);
  for (size_t t = 0; t < x.n_tail; t++) {
    const int32_t p = x.tail_pair[t];
    const int rlen = (int)q.read_lengths[q.cross_haps ? p / q.cross_haps : p], hlen = (int)q.hap_lengths[q.cross_haps ? p % q.cross_haps : p];
    const int nb = blocks_for(rlen, kPdRpl);
    CHECK(x.tail_striped[t] == (nb > kPairLanes ? 1 : 0), "tail job %zu: read of %d bases", t, rlen);
    CHECK(x.tail_steps[t] == hlen + std::min(nb, kPairLanes) - 1, "tail job %zu: %d steps", t, x.tail_steps[t]);
    for (int l = 0; l < kPairLanes; l++) {
      const PlanLane& s = x.tail_lanes[t * kPairLanes + (size_t)l];
      if (nb <= kPairLanes && l < nb) CHECK(s.read == p && s.block == l, "tail job %zu lane %d: {%d, %d}", t, l, s.read, s.block);
      else CHECK(s.read == -1, "tail job %zu lane %d is not idle", t, l);
    }
    g.tail_jobs++;
    g.striped_tails += nb > kPairLanes;
  }
  return true;
}

bool check_cross_jobs(const PdProblem& q, const PdCrossPlan& x) {
  const int nr = q.n_read_items, nh = q.n_hap_items;
  const size_t n_chunks = x.chunk_steps.size();
  CHECK(x.cross_lanes.size() == n_chunks * kPairLanes && x.chunk_rep.size() == n_chunks, "%zu chunks, %zu lanes", n_chunks, x.cross_lanes.size());
  std::vector<int> chunk_of((size_t)nr, -1), blocks_seen((size_t)nr, 0);
  for (size_t k = 0; k < n_chunks; k++) {
    int top = 0;
    bool rep_inside = false;
    for (int l = 0; l < kPairLanes; l++) {
      const PlanLane& s = x.cross_lanes[k * kPairLanes + (size_t)l];
      if (s.read < 0) continue;
      CHECK(s.read < nr, "chunk %zu lane %d: read %d of %d", k, l, s.read, nr);
      CHECK(chunk_of[(size_t)s.read] < 0 || chunk_of[(size_t)s.read] == (int)k, "read %d sits in chunks %d and %zu", s.read, chunk_of[(size_t)s.read], k);
      CHECK(s.block == blocks_seen[(size_t)s.read], "read %d: block %d on lane %d, %d expected", s.read, s.block, l, blocks_seen[(size_t)s.read]);
      if (s.block > 0) CHECK(l > 0 && x.cross_lanes[k * kPairLanes + (size_t)l - 1].read == s.read, "read %d: its lanes are not consecutive", s.read);
      chunk_of[(size_t)s.read] = (int)k;
      blocks_seen[(size_t)s.read]++;
      top = std::max(top, s.block);
      rep_inside |= s.read == x.chunk_rep[k];
    }
    CHECK(x.chunk_steps[k] == top, "chunk %zu: steps %d, highest block %d", k, x.chunk_steps[k], top);
    CHECK(rep_inside, "chunk %zu: its representative %d is not in it", k, x.chunk_rep[k]);
  }
  std::set<int32_t> listed(x.job_pair.begin(), x.job_pair.end());
  size_t n_long = 0;
  for (int r = 0; r < nr; r++) {
    const int nb = blocks_for((int)q.read_lengths[r], kPdRpl);
    if (nb <= kPairLanes) { CHECK(blocks_seen[(size_t)r] == nb, "read %d: %d of its %d blocks are placed", r, blocks_seen[(size_t)r], nb); continue; }
    CHECK(blocks_seen[(size_t)r] == 0, "striped read %d is in a chunk", r);
    for (int h = 0; h < nh; h++) CHECK(listed.count(r * nh + h) == 1, "striped read %d, haplotype %d: no listed job", r, h);
    n_long++;
  }
  CHECK(x.job_pair.size() == n_long * (size_t)nh && listed.size() == x.job_pair.size() && x.job_striped.size() == x.job_pair.size() &&
            x.job_steps.size() == x.job_pair.size(), "%zu listed jobs for %zu striped reads", x.job_pair.size(), n_long);
  for (const uint8_t s : x.job_striped) CHECK(s == 1, "a listed job of the cross layout is not striped");
  if (n_long == (size_t)nr) CHECK(n_chunks == 0, "every read is striped, yet there are %zu chunks", n_chunks);
  g.striped_reads += (long long)n_long;
  return true;
}

bool check_routing(const PdPlanSettings& set, const PdProblem& q, const PdCrossPlan& x) {
  const int nh = q.n_hap_items;
  CHECK((int)x.hap_order.size() == nh && (int)x.hap_ncls.size() == nh && (int)x.class_codes.size() == 8 * nh, "routing tables of %d haplotypes", nh);
  std::vector<int> odd((size_t)nh);
  std::vector<std::set<uint32_t>> cls((size_t)nh);
  std::set<uint32_t> uni;
  size_t n_clean = 0, n_tab = 0;
  for (int h = 0; h < nh; h++) {
    odd[(size_t)h] = naive_odd(q.hap_bases + (size_t)h * q.max_hap_len, q.hap_lengths[h]);
    cls[(size_t)h] = naive_classes(q, h);
    const bool tab = set.use_table && !odd[(size_t)h] && (int)cls[(size_t)h].size() <= kPdTabClasses;
    n_clean += !odd[(size_t)h];
    n_tab += tab;
    CHECK((x.hap_ncls[(size_t)h] != 0) == tab, "haplotype %d: %d classes listed, %zu counted, odd %d", h, x.hap_ncls[(size_t)h], cls[(size_t)h].size(), odd[(size_t)h]);
    if (tab) uni.insert(cls[(size_t)h].begin(), cls[(size_t)h].end());
  }
  CHECK(x.n_clean_haps == n_clean && x.n_tab_haps == n_tab, "%zu clean / %zu table haplotypes, %zu / %zu expected", x.n_clean_haps, x.n_tab_haps, n_clean, n_tab);
  if (!set.use_table) CHECK(n_tab == 0, "table haplotypes without the table kernel");
  // [table | other clean | odd], each longest first, ties in index order
  std::vector<int32_t> want;
  for (int group = 0; group < 3; group++) {
    std::vector<int32_t> mine;
    for (int h = 0; h < nh; h++)
      if ((odd[(size_t)h] ? 2 : x.hap_ncls[(size_t)h] ? 0 : 1) == group) mine.push_back(h);
    for (size_t i = 1; i < mine.size(); i++)   // insertion sort: stable, nothing shared with the planner's
      for (size_t j = i; j > 0 && q.hap_lengths[mine[j - 1]] < q.hap_lengths[mine[j]]; j--) std::swap(mine[j - 1], mine[j]);
    want.insert(want.end(), mine.begin(), mine.end());
  }
  CHECK(x.hap_order == want, "hap_order is not [table | other clean | odd], each longest first and stable");
  const bool shared = (int)uni.size() <= kPdTabClasses;
  for (int h = 0; h < nh; h++) {
    if (!x.hap_ncls[(size_t)h]) continue;
    const int n = x.hap_ncls[(size_t)h];
    CHECK(n <= kPdTabClasses, "haplotype %d: %d classes", h, n);
    const std::set<uint32_t> got(x.class_codes.begin() + 8 * h, x.class_codes.begin() + 8 * h + n);
    CHECK((int)got.size() == n, "haplotype %d lists a class twice", h);
    for (const uint32_t code : cls[(size_t)h]) CHECK(got.count(code) == 1, "haplotype %d: a column's code %08x is not in its list", h, code);
    CHECK(got == (shared ? uni : cls[(size_t)h]), "haplotype %d: %d classes listed, its own %zu, the union %zu", h, n, cls[(size_t)h].size(), uni.size());
    g.table_haps++;
  }
  if (n_tab > 1) (shared ? g.union_shared : g.union_kept)++;
  g.odd_haps += (long long)(nh - (int)n_clean);
  return true;
}

bool same_plan(const PdCrossPlan& a, const PdCrossPlan& b) {
  auto lanes_eq = [](const std::vector<PlanLane>& x, const std::vector<PlanLane>& y) {
    return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(PlanLane)) == 0);
  };
  return a.job_pair == b.job_pair && a.job_steps == b.job_steps && a.job_striped == b.job_striped && lanes_eq(a.cross_lanes, b.cross_lanes) &&
         a.hap_order == b.hap_order && a.chunk_steps == b.chunk_steps && a.chunk_rep == b.chunk_rep && a.n_tail == b.n_tail &&
         lanes_eq(a.tail_lanes, b.tail_lanes) && a.tail_pair == b.tail_pair && a.tail_steps == b.tail_steps && a.tail_striped == b.tail_striped &&
         a.hap_ncls == b.hap_ncls && a.class_codes == b.class_codes && a.n_clean_haps == b.n_clean_haps && a.n_tab_haps == b.n_tab_haps;
}

// One region planned and checked; *out: its plan.
bool plan_cross(const PdPlanSettings& set, PdPlanScratch* scratch, const PdProblem& q, PdCrossPlan* out) {
  pd_plan_cross_jobs(set, q, out);
  pd_plan_cross_routing(set, scratch, q, out);
  g.regions++;
  return check_cross_jobs(q, *out) && check_routing(set, q, *out) && check_tails(set, q, *out);
}

// pd_table_copies executed into a block of exactly L.total bytes, in the order pd_stage_tables makes the copies.
bool check_table_copies(const PdCallPlan& p) {
  const PdJobLayout L(p.job_counts());
  const PdTableCopies list = pd_table_copies(p, L);
  const size_t at[] = {L.jp, L.jn, L.js, L.cl, L.ho, L.cs, L.cr, L.tl, L.tp, L.tn, L.ts, L.nc, L.cc, L.pc, L.pl, L.cu, L.tg, L.fj};
  static_assert(sizeof at / sizeof at[0] == std::tuple_size<PdTableCopies>::value, "one offset per copy");
  std::vector<size_t> starts(std::begin(at), std::end(at));
  for (const size_t o : {L.jl, L.jf, L.total}) starts.push_back(o);
  std::unique_ptr<unsigned char[]> block(new unsigned char[L.total]);
  int i = 0;
  for (const PdTableCopy& t : list) {
    CHECK(t.offset == at[i], "copy %d goes to %zu, %zu expected", i, t.offset, at[i]);
    size_t next = L.total;   // the block that follows this one
    for (const size_t o : starts) if (o > t.offset) next = std::min(next, o);
    CHECK(t.offset % 256 == 0 && t.offset + t.bytes <= next, "copy %d: %zu bytes at %zu run into the block at %zu", i, t.bytes, t.offset, next);
    if (t.bytes) memcpy(block.get() + t.offset, t.src, t.bytes);
    i++;
  }
  CHECK(list.back().offset == L.fj && list.back().bytes == p.full_first.size() * 4, "the full launch's list comes last");
  const PdCrossPlan& x = p.x;
  auto same = [&](size_t off, const void* src, size_t bytes) { return bytes == 0 || memcmp(block.get() + off, src, bytes) == 0; };
  CHECK(same(L.jp, x.job_pair.data(), x.job_pair.size() * 4) && same(L.cl, x.cross_lanes.data(), x.cross_lanes.size() * sizeof(PlanLane)) &&
            same(L.ho, x.hap_order.data(), x.hap_order.size() * 4) && same(L.tl, x.tail_lanes.data(), x.tail_lanes.size() * sizeof(PlanLane)) &&
            same(L.cc, x.class_codes.data(), x.class_codes.size() * 4) && same(L.pc, p.place_chunk.data(), p.place_chunk.size() * 4) &&
            same(L.cu, p.chunk_used.data(), p.chunk_used.size()) && same(L.tg, p.tab_group_start.data(), p.tab_group_start.size() * 4) &&
            same(L.fj, p.full_first.data(), p.full_first.size() * 4), "a staged table differs from the plan's vector");
  CHECK((size_t)p.n_general == x.job_pair.size() && x.job_steps.size() == x.job_pair.size() && x.job_striped.size() == x.job_pair.size(), "listed jobs");
  return true;
}

bool check_groups(const std::vector<size_t>& tab_haps, const std::vector<int32_t>& start, const int32_t* groups) {
  size_t total = 0;
  for (const size_t n : tab_haps) total += n;
  CHECK(!start.empty() && start.front() == 0 && start.back() == (int32_t)total, "groups cover 0..%zu", total);
  size_t at = 0, gi = 0, n_groups = start.size() - 1;
  long long sum = 0;
  for (size_t k = 0; k < tab_haps.size(); k++) {
    const size_t end = at + tab_haps[k];
    int made = 0;
    while (gi < n_groups && (size_t)start[gi] < end) {
      const int size = start[gi + 1] - start[gi];
      CHECK(size >= 1 && size <= 6, "group %zu holds %d haplotypes", gi, size);
      CHECK((size_t)start[gi] >= at && (size_t)start[gi + 1] <= end, "group %zu [%d, %d) leaves region %zu [%zu, %zu)", gi, start[gi], start[gi + 1], k, at, end);
      g.grouped += size > 1;
      gi++; made++;
    }
    if (groups) { CHECK(groups[k] == made, "region %zu: %d groups counted, %d made", k, groups[k], made); sum += groups[k]; }
    at = end;
  }
  CHECK(gi == n_groups, "%zu groups, %zu inside the regions", n_groups, gi);
  if (groups) CHECK(sum == (long long)n_groups, "the regions' counts sum to %lld of %zu groups", sum, n_groups);
  return true;
}

bool check_cross_regions(const PdPlanSettings& set) {
  PdPlanScratch scratch;
  const int edge_len[] = {1, kPdRpl - 1, kPdRpl, kLongRead - 1, kLongRead};
  // the edge lengths side by side; striped reads only; 2049 short reads; then random regions
  for (int kind = 0; kind < 40; kind++) {
    const int nr = kind == 0 ? 10 : kind == 1 ? 3 : kind == 2 ? 2049 : pick(1, 60), nh = kind == 2 ? 3 : pick(1, 12);
    auto read_len = [&](int r) {
      return kind == 0 ? edge_len[r % 5] : kind == 1 ? kLongRead + r : kind == 2 ? pick(1, 150) : pick(0, 15) == 0 ? pick(kLongRead - 2, kLongRead + 40) : pick(1, 250);
    };
    const Inputs in = make_inputs(nr, nh, pick(1, 120), read_len);
    const int64_t n = (int64_t)nr * nh, width = set.fma_mode ? 8 : 4;
    for (const int64_t ref : {(int64_t)0, (int64_t)1, width - 1, width, width + 1, n, n + 1}) {
      if (kind == 2 && ref != 0 && ref != width + 1) continue;   // (the big region: two batch sizes are enough)
      const PdProblem q = in.cross(ref);
      PdCrossPlan x;
      if (!plan_cross(set, &scratch, q, &x)) return false;
      PdCallPlan p;
      p.x = x;
      CHECK(pd_plan_counts(set, q, &p), "too many jobs");
      CHECK(p.n_cross_jobs == (int)(x.chunk_steps.size() * (size_t)nh) && p.n_general == (int)x.job_pair.size() && p.n_jobs == p.n_cross_jobs + p.n_general, "job counts");
      if (!p.tab_group_start.empty()) {
        std::vector<int32_t> again;
        const size_t n_tab = x.n_tab_haps;
        pd_size_tab_groups(&n_tab, 1, p.n_cross_tab, &again, nullptr);
        CHECK(again == p.tab_group_start && check_groups({n_tab}, again, nullptr), "K = 1 groups");
        CHECK(p.n_tab_units == (int)((again.size() - 1) * x.chunk_steps.size()), "table units");
      }
      if (!check_table_copies(p)) return false;
    }
  }
  // the union rule both ways, with and without the table kernel; the same plan twice from one scratch across the wrap of the stamp
  for (int round = 0; round < 60; round++) {
    const int hap_kind = round % 3 == 0 ? 1 : round % 3 == 1 ? 2 : -1;
    const Inputs in = make_inputs(pick(1, 20), pick(2, 10), pick(20, 200), [&](int) { return pick(1, 100); }, hap_kind);
    PdPlanSettings s = set;
    s.use_table = round % 5 != 4;
    const PdProblem q = in.cross(0);
    PdPlanScratch wrap, fresh;   // `wrap`: one planning leaves the stamps 1, 2, .. behind, the next one meets them again behind the wrap
    PdCrossPlan a, b, c;
    if (!plan_cross(s, &wrap, q, &a) || !plan_cross(s, &fresh, q, &b)) return false;
    wrap.class_stamp_id = round % 2 ? 0xfffffffeu : 0xffffffffu;   // (the second: the first haplotype would meet its own old stamps)
    if (!plan_cross(s, &wrap, q, &c)) return false;
    CHECK(same_plan(a, b) && same_plan(a, c), "round %d: the same problem planned twice gives two plans", round);
    CHECK(!s.use_table || a.n_clean_haps < 2 || wrap.class_stamp_id < 0x1000u, "round %d: the stamp did not wrap (%08x)", round, wrap.class_stamp_id);
  }
  // two table haplotypes whose classes do not fit one table together: each keeps its own list
  {
    Inputs in = make_inputs(4, 2, 12, [&](int) { return 10; }, 0, true);
    for (int h = 0; h < 2; h++)
      for (int j = 0; j < 12; j++) {
        in.hb[(size_t)h * 12 + j] = "ACGT"[j % 4];
        in.pd[(size_t)h * 12 + j] = (int8_t)(j >= 10 ? kPdSnp | ((1 + 2 * h + (j - 10)) << 3) : 0);   // G and T with alleles 1, 2 in one, 3, 4 in the other
      }
    const PdProblem q = in.cross(0);
    PdCrossPlan x;
    const long long kept = g.union_kept;
    if (!plan_cross(set, &scratch, q, &x)) return false;
    CHECK(!set.use_table || (g.union_kept == kept + 1 && x.hap_ncls[0] == 6 && x.hap_ncls[1] == 6), "the lists of 6 + 6 classes were merged");
  }
  return true;
}

bool check_paired_plan(const PdPlanSettings& set, int n, int n_slices) {
  PdPlanScratch scratch;
  const Inputs in = make_inputs(n, n, pick(1, 150), [&](int) { return pick(0, 40) == 0 ? pick(kLongRead - 1, kLongRead + 30) : pick(1, 260); });
  const PdProblem q = in.paired();
  PdCallPlan p;
  const PdInputLayout layout((size_t)n, (size_t)n, (size_t)in.mh, (size_t)in.mr);
  pd_plan_slices(set, q, layout, &p);
  CHECK(p.n_slices == 1 && p.slice_lo[0] == 0 && p.slice_lo[1] == (size_t)n && p.staged == (layout.total <= kPdStageBytes), "a small call is one staged slice");
  if (n_slices > 1) {   // hand-set slices: 64-aligned cuts as pd_plan_slices makes them
    p.n_slices = n_slices;
    for (int k = 1; k < n_slices; k++) p.slice_lo[k] = (size_t)n * (size_t)k / (size_t)n_slices / 64 * 64;
    p.slice_lo[n_slices] = (size_t)n;
    g.sliced_plans++;
  }
  pd_plan_paired_jobs(set, &scratch, q, &p);
  CHECK(pd_plan_counts(set, q, &p), "too many jobs");
  if (!check_tails(set, q, p.x)) return false;
  const PdCrossPlan& x = p.x;
  const size_t n_vec = (size_t)n - x.n_tail, n_chunks = p.chunk_used.size();
  CHECK(p.place_chunk.size() == (size_t)n && p.place_lane.size() == (size_t)n, "placement of %d pairs", n);
  std::vector<std::vector<int>> taken(n_chunks, std::vector<int>(kPairLanes, -1));
  std::vector<int> steps(n_chunks, 0), slice_of(n_chunks, -1);
  size_t n_striped = 0;
  for (size_t i = 0; i < (size_t)n; i++) {
    const int nb = blocks_for((int)q.read_lengths[i], kPdRpl), c = p.place_chunk[i];
    if (i >= n_vec) { CHECK(c == -1, "tail pair %zu is placed", i); continue; }
    if (nb > kPairLanes) {
      CHECK(c == -1, "striped pair %zu is placed", i);
      CHECK(n_striped < x.job_pair.size() && x.job_pair[n_striped] == (int32_t)i && x.job_striped[n_striped] == 1, "striped pair %zu is not listed job %zu", i, n_striped);
      n_striped++;
      continue;
    }
    CHECK(c >= 0 && (size_t)c < n_chunks, "pair %zu: chunk %d of %zu", i, c, n_chunks);
    for (int b = 0; b < nb; b++) {
      const int l = p.place_lane[i] + b;
      CHECK(l < kPairLanes && taken[(size_t)c][(size_t)l] < 0, "pair %zu: lane %d of chunk %d is taken or beyond the wavefront", i, l, c);
      taken[(size_t)c][(size_t)l] = (int)i;
    }
    steps[(size_t)c] = std::max(steps[(size_t)c], (int)q.hap_lengths[i] + nb - 1);
    int k = 0;
    while (i >= std::min(p.slice_lo[k + 1], n_vec)) k++;
    CHECK(slice_of[(size_t)c] < 0 || slice_of[(size_t)c] == k, "chunk %d holds pairs of slices %d and %d", c, slice_of[(size_t)c], k);
    slice_of[(size_t)c] = k;
  }
  CHECK(p.n_striped == n_striped && (size_t)p.n_general == n_striped + n_chunks && p.n_packed == n_chunks, "%zu striped, %zu chunks, %d listed jobs", n_striped, n_chunks, p.n_general);
  for (size_t c = 0; c < n_chunks; c++) {
    int used = 0;
    while (used < kPairLanes && taken[c][(size_t)used] >= 0) used++;
    for (int l = used; l < kPairLanes; l++) CHECK(taken[c][(size_t)l] < 0, "chunk %zu: a gap in front of lane %d", c, l);
    CHECK(used > 0 && p.chunk_used[c] == used, "chunk %zu: %d lanes used, %d taken", c, p.chunk_used[c], used);
    const size_t j = n_striped + c;
    CHECK(x.job_steps[j] == steps[c] && x.job_striped[j] == 0, "chunk %zu: %d steps, %d expected", c, x.job_steps[j], steps[c]);
    CHECK(x.job_pair[j] >= 0 && p.place_chunk[(size_t)x.job_pair[j]] == (int32_t)c, "chunk %zu: its first pair %d is not in it", c, x.job_pair[j]);
    CHECK((int)c >= p.slice_chunk0[slice_of[c]] && (int)c < p.slice_chunk0[slice_of[c] + 1], "chunk %zu of slice %d lies outside [%d, %d)", c, slice_of[c],
          p.slice_chunk0[slice_of[c]], p.slice_chunk0[slice_of[c] + 1]);
  }
  for (int k = 0; k < p.n_slices; k++) CHECK(p.slice_chunk0[k] <= p.slice_chunk0[k + 1], "slice_chunk0 decreases at %d", k);
  CHECK(p.slice_chunk0[0] == 0 && p.slice_chunk0[p.n_slices] == (int32_t)n_chunks, "the slices' chunks are not all chunks");
  CHECK(p.n_striped_listed == (int32_t)n_striped && p.full_first.size() == n_striped, "the full launch's first list");
  g.paired_plans++;
  return check_table_copies(p);
}

// pd_plan_slices through its inputs alone: counts and sizes, no array is read.
bool check_slices(const PdPlanSettings& set) {
  auto slices = [&](int64_t n, int cross, bool in_hbm, int pipeline, size_t row) {
    PdProblem q{};
    q.n_pairs = n; q.cross_haps = cross; q.in_hbm = in_hbm;
    PdPlanSettings s = set;
    s.pipeline = pipeline;
    PdCallPlan p;
    pd_plan_slices(s, q, PdInputLayout((size_t)n, (size_t)n, row, row), &p);
    return p;
  };
  const size_t row = 200;   // 65 536 pairs: 6 x 13.1 MB, over kPdSliceMinBytes
  CHECK(slices(65536, 0, true, 1, row).n_slices == 1 && slices(65536, 64, false, 1, row).n_slices == 1 && slices(65536, 0, false, 0, row).n_slices == 1 &&
            slices(65535, 0, false, 1, 2 * row).n_slices == 1 && slices(65536, 0, false, 1, 100).n_slices == 1, "a call under a threshold was cut");
  CHECK(!slices(65536, 0, true, 1, 1).staged && slices(1000, 0, false, 1, row).staged, "staging");
  for (const int64_t n : {(int64_t)65536, (int64_t)100001, (int64_t)423936}) {
    const PdCallPlan p = slices(n, 0, false, 1, row);
    CHECK(p.n_slices == 7 && p.n_slices <= kPdMaxSlices && p.slice_lo[0] == 0 && p.slice_lo[7] == (size_t)n && !p.staged, "%lld pairs: %d slices", (long long)n, p.n_slices);
    for (int k = 0; k < 7; k++) CHECK(p.slice_lo[k] < p.slice_lo[k + 1] && p.slice_lo[k] % 64 == 0, "%lld pairs: slice %d starts at %zu", (long long)n, k, p.slice_lo[k]);
    g.sliced_plans++;
  }
  return true;
}

bool check_tab_groups() {
  for (int round = 0; round < 300; round++) {
    const int K = round == 0 ? 1 : pick(1, kPdMaxRegions);
    std::vector<size_t> tab_haps((size_t)K);
    for (size_t& n : tab_haps) n = (size_t)(pick(0, 3) == 0 ? 0 : pick(1, 30));
    std::vector<int32_t> start, groups((size_t)K, -1);
    pd_size_tab_groups(tab_haps.data(), K, pick(0, 1) ? pick(0, 30000) : pick(0, 400000), &start, groups.data());
    if (!check_groups(tab_haps, start, groups.data())) return false;
  }
  return true;
}

// The work of one launch set, pair by pair: how often the main launches and the tail launch reach each output pair.
struct Reach { std::vector<int> main, tail; };

bool check_multi(const PdPlanSettings& set, int round) {
  const int K = round == 0 ? 1 : round == 1 ? kPdMaxRegions : round == 2 ? 1 : pick(1, kPdMaxRegions);
  std::vector<Inputs> in;
  std::vector<PdProblem> Q;
  for (int k = 0; k < K; k++) {
    const bool tiny = pick(0, 5) == 0;
    const bool all_striped = pick(0, 11) == 0;
    in.push_back(make_inputs(tiny ? 1 : pick(1, 40), tiny ? 1 : pick(1, 9), pick(1, 90),
                             [&](int) { return all_striped || pick(0, 30) == 0 ? pick(kLongRead, kLongRead + 20) : pick(1, 200); }));
    Q.push_back(in.back().cross(pick(0, 2) == 0 ? pick(1, 50) : 0));
  }
  const PdMultiShape sh(Q);
  PdMultiFit fit;
  for (const PdProblem& q : Q) {
    const bool with = fit.fits_with(q);
    fit.take(q);
    CHECK(with == fit.fits(), "fits_with and take disagree at region %d", fit.count - 1);
  }
  CHECK(fit.count == K && fit.pairs == sh.NP && fit.nh == sh.NH && fit.nr == sh.NR && fit.mh == sh.mh && fit.mr == sh.mr &&
            fit.fits() == (sh.NP <= kPdMultiMaxPairs && sh.layout().total <= kPdStageBytes), "the fit rule's totals");
  PdPlanScratch scratch;
  PdMultiPlan plan;
  pd_multi_plan(set, &scratch, Q, sh, &plan);
  const PdMultiJobLayout L((size_t)K, sh.NH, plan);
  // the blocks: 256-aligned, disjoint, the staged ones inside staged_total, the lane rows behind them inside total
  const size_t ng = plan.n_general, nt = plan.n_tail;
  const std::vector<std::pair<size_t, size_t>> blocks = {
      {L.rg, ((size_t)K + 1) * sizeof(PdRegion)}, {L.cl, plan.n_chunks * kPdLaneRowBytes}, {L.cs, plan.n_chunks * 4}, {L.cr, plan.n_chunks * 4},
      {L.ho, sh.NH * 4}, {L.tg, plan.tab_group_start.size() * 4}, {L.nc, sh.NH}, {L.cc, sh.NH * 32}, {L.jp, ng * 4}, {L.jn, ng * 4}, {L.js, ng},
      {L.jf, ng}, {L.fj, ng * 4}, {L.fc, 4}, {L.tl, nt * kPdLaneRowBytes}, {L.tp, nt * 4}, {L.tn, nt * 4}, {L.ts, nt}, {L.jl, ng * kPdLaneRowBytes}};
  for (size_t i = 0; i < blocks.size(); i++) {
    const size_t lo = blocks[i].first, hi = lo + blocks[i].second, limit = lo == L.jl ? L.total : L.staged_total;
    CHECK(lo % 256 == 0 && hi <= limit && (lo != L.jl || lo >= L.staged_total), "block %zu [%zu, %zu) of %zu / %zu", i, lo, hi, L.staged_total, L.total);
    for (size_t j = 0; j < i; j++) CHECK(hi <= blocks[j].first || blocks[j].first + blocks[j].second <= lo, "blocks %zu and %zu overlap", j, i);
  }
  std::unique_ptr<unsigned char[]> block(new unsigned char[L.staged_total]);
  memset(block.get(), 0xAB, L.staged_total);
  pd_multi_fill_tables(plan, L, block.get());
  const unsigned char* hj = block.get();
  const PdRegion* rg = reinterpret_cast<const PdRegion*>(hj + L.rg);
  const PlanLane* cl = reinterpret_cast<const PlanLane*>(hj + L.cl);
  const int32_t *ho = reinterpret_cast<const int32_t*>(hj + L.ho), *tg = reinterpret_cast<const int32_t*>(hj + L.tg);
  const int32_t* lists[3] = {ho, ho + plan.n_tab_haps, ho + plan.n_tab_haps + plan.n_hot_haps};
  CHECK(memcmp(rg, plan.regions.data(), ((size_t)K + 1) * sizeof(PdRegion)) == 0 && rg[K].pair_base == (int32_t)sh.NP, "the region table");
  // what the launches reach, with the kernel's index functions
  Reach multi{std::vector<int>(sh.NP, 0), std::vector<int>(sh.NP, 0)};
  const int units[3] = {plan.n_tab_units, plan.n_hot_units, plan.n_full_units};
  for (int launch = 0; launch < 3; launch++)
    for (int u = 0; u < units[launch]; u++) {
      const int k = pd_region_of_unit(rg, K, launch, u);
      const PdRegion& r = rg[k];
      int item, chunk;
      pd_unit_split(r, launch, u, &item, &chunk);
      CHECK(chunk >= r.chunk_base && chunk < r.chunk_base + r.n_chunks && (size_t)chunk < plan.n_chunks, "launch %d unit %d: chunk %d of region %d", launch, u, chunk, k);
      const int h0 = launch == kPdLaunchTab ? tg[item] : item, h1 = launch == kPdLaunchTab ? tg[item + 1] : item + 1;
      for (int at = h0; at < h1; at++) {
        const int hi = lists[launch][at];
        CHECK(hi >= r.hap_base && hi < r.hap_base + r.n_haps, "launch %d unit %d: haplotype %d of region %d", launch, u, hi, k);
        for (int l = 0; l < kPairLanes; l++) {
          const PlanLane& s = cl[(size_t)chunk * kPairLanes + (size_t)l];
          if (s.read < 0 || s.block != 0) continue;
          CHECK(s.read >= r.read_base && s.read < rg[k + 1].read_base, "chunk %d: read %d of region %d", chunk, s.read, k);
          multi.main[(size_t)pd_pair_index(r, s.read, hi)]++;
        }
      }
    }
  const int32_t *jp = reinterpret_cast<const int32_t*>(hj + L.jp), *fj = reinterpret_cast<const int32_t*>(hj + L.fj), *jn = reinterpret_cast<const int32_t*>(hj + L.jn);
  CHECK(*reinterpret_cast<const int32_t*>(hj + L.fc) == (int32_t)ng, "the full launch's count");
  for (size_t j = 0; j < ng; j++) {
    CHECK(fj[j] == (int32_t)j && hj[L.js + j] == 1 && hj[L.jf + j] == 0 && jn[j] == 0 && jp[j] >= 0 && (size_t)jp[j] < sh.NP, "listed job %zu", j);
    multi.main[(size_t)jp[j]]++;
  }
  const int32_t* tp = reinterpret_cast<const int32_t*>(hj + L.tp);
  for (size_t t = 0; t < nt; t++) { CHECK(tp[t] >= 0 && (size_t)tp[t] < sh.NP, "tail job %zu", t); multi.tail[(size_t)tp[t]]++; }
  // the same from the K single-region plans, each in its own indices
  Reach single{std::vector<int>(sh.NP, 0), std::vector<int>(sh.NP, 0)};
  size_t pair_base = 0, tail_at = 0, n_table = 0;
  for (int k = 0; k < K; k++) {
    PdPlanScratch own;
    PdCrossPlan x;
    if (!plan_cross(set, &own, Q[(size_t)k], &x)) return false;
    CHECK(same_plan(x, plan.plans[(size_t)k]), "region %d: the set's plan is not the single call's", k);
    const size_t nh = (size_t)Q[(size_t)k].n_hap_items, n_chunks = x.chunk_steps.size();
    for (size_t j = 0; j < n_chunks * nh; j++) {   // cross job j = (hap_order[j / n_chunks], chunk j % n_chunks)
      const int32_t h = x.hap_order[j / n_chunks];
      for (int l = 0; l < kPairLanes; l++) {
        const PlanLane& s = x.cross_lanes[(j % n_chunks) * kPairLanes + (size_t)l];
        if (s.read >= 0 && s.block == 0) single.main[pair_base + (size_t)s.read * nh + (size_t)h]++;
      }
    }
    for (const int32_t p : x.job_pair) single.main[pair_base + (size_t)p]++;
    // the region's chunk tables and class lists, shifted to the concatenated numbering
    const PdRegion& r = rg[k];
    CHECK((size_t)r.n_chunks == n_chunks && (size_t)r.n_haps == nh && (size_t)r.pair_base == pair_base, "region %d of the table", k);
    for (size_t c = 0; c < n_chunks; c++)
      CHECK(reinterpret_cast<const int32_t*>(hj + L.cs)[(size_t)r.chunk_base + c] == x.chunk_steps[c] &&
                reinterpret_cast<const int32_t*>(hj + L.cr)[(size_t)r.chunk_base + c] == x.chunk_rep[c] + r.read_base, "region %d chunk %zu: steps / representative", k, c);
    for (size_t i = 0; i < n_chunks * kPairLanes; i++) {
      const PlanLane &s = x.cross_lanes[i], &m = cl[(size_t)r.chunk_base * kPairLanes + i];
      CHECK(m.block == s.block && m.read == (s.read < 0 ? -1 : s.read + r.read_base), "region %d lane %zu: {%d, %d}", k, i, m.read, m.block);
    }
    CHECK(memcmp(hj + L.nc + r.hap_base, x.hap_ncls.data(), nh) == 0 && memcmp(hj + L.cc + (size_t)r.hap_base * 32, x.class_codes.data(), nh * 32) == 0,
          "region %d: class counts / codes", k);
    for (size_t t = 0; t < x.n_tail; t++, tail_at++) {
      single.tail[pair_base + (size_t)x.tail_pair[t]]++;
      const PlanLane* row = reinterpret_cast<const PlanLane*>(hj + L.tl) + tail_at * kPairLanes;
      for (int l = 0; l < kPairLanes; l++)
        CHECK(row[l].block == x.tail_lanes[t * kPairLanes + (size_t)l].block &&
                  row[l].read == (x.tail_lanes[t * kPairLanes + (size_t)l].read < 0 ? -1 : tp[tail_at]), "tail job %zu lane %d", tail_at, l);
      CHECK(reinterpret_cast<const int32_t*>(hj + L.tn)[tail_at] == x.tail_steps[t] && hj[L.ts + tail_at] == x.tail_striped[t], "tail job %zu", tail_at);
    }
    pair_base += (size_t)Q[(size_t)k].n_pairs;
    n_table += x.n_tab_haps;
  }
  CHECK(multi.main == single.main && multi.tail == single.tail && n_table == plan.n_tab_haps, "the set reaches other pairs than its regions' single plans");
  for (size_t p = 0; p < sh.NP; p++) CHECK(multi.main[p] == 1 && multi.tail[p] <= 1, "pair %zu: reached %d times, %d times by the tail launch", p, multi.main[p], multi.tail[p]);
  std::vector<size_t> tab_haps;
  std::vector<int32_t> groups;
  for (int k = 0; k < K; k++) { tab_haps.push_back(plan.plans[(size_t)k].n_tab_haps); groups.push_back(rg[k + 1].list_start[kPdLaunchTab] - rg[k].list_start[kPdLaunchTab]); }
  if (!check_groups(tab_haps, plan.tab_group_start, groups.data())) return false;
  if (K == 1) {   // the filled tables are the single plan's vectors
    const PdCrossPlan& x = plan.plans[0];
    PdCallPlan p;
    p.x = x;
    CHECK(pd_plan_counts(set, Q[0], &p), "too many jobs");
    auto same = [&](size_t off, const void* src, size_t bytes) { return bytes == 0 || memcmp(hj + off, src, bytes) == 0; };
    CHECK(same(L.cl, x.cross_lanes.data(), x.cross_lanes.size() * sizeof(PlanLane)) && same(L.cs, x.chunk_steps.data(), x.chunk_steps.size() * 4) &&
              same(L.cr, x.chunk_rep.data(), x.chunk_rep.size() * 4) && same(L.ho, x.hap_order.data(), x.hap_order.size() * 4) &&
              same(L.nc, x.hap_ncls.data(), x.hap_ncls.size()) && same(L.cc, x.class_codes.data(), x.class_codes.size() * 4) &&
              same(L.jp, x.job_pair.data(), x.job_pair.size() * 4) && same(L.jn, x.job_steps.data(), x.job_steps.size() * 4) &&
              same(L.js, x.job_striped.data(), x.job_striped.size()) && same(L.fj, p.full_first.data(), p.full_first.size() * 4) &&
              same(L.tl, x.tail_lanes.data(), x.tail_lanes.size() * sizeof(PlanLane)) && same(L.tp, x.tail_pair.data(), x.n_tail * 4) &&
              same(L.tn, x.tail_steps.data(), x.n_tail * 4) && same(L.ts, x.tail_striped.data(), x.n_tail), "K = 1: a table differs from the single plan's");
    // (a region without a chunk: the single call sizes no groups, the set's have no units)
    CHECK(p.tab_group_start.empty() || plan.tab_group_start == p.tab_group_start, "K = 1: the table groups");
    CHECK(plan.n_tab_units == p.n_tab_units && plan.n_hot_units == p.n_cross_hot && plan.n_full_units == p.n_cross_jobs - p.n_cross_hot - p.n_cross_tab &&
              plan.entry_stride == p.entry_stride && (int)plan.n_general == p.n_general, "K = 1: the launch sizes");
  }
  g.multi_sets++;
  return true;
}
}  // namespace

int main() {
  if (!check_odd_bases() || !check_tab_groups()) return 1;
  {  // the fit rule at its limits, from the counts alone
    PdProblem big{};
    big.n_pairs = (int64_t)kPdMultiMaxPairs; big.n_hap_items = 64; big.n_read_items = 2048; big.max_hap_len = 100; big.max_read_len = 100;
    PdProblem one = big;
    one.n_pairs = 1; one.n_hap_items = one.n_read_items = 1;
    PdMultiFit fit;
    if (!fit.fits_with(big)) { std::fprintf(stderr, "kPdMultiMaxPairs pairs do not fit\n"); return 1; }
    fit.take(big);
    if (!fit.fits() || fit.fits_with(one)) { std::fprintf(stderr, "one pair beyond kPdMultiMaxPairs fits\n"); return 1; }
    PdProblem wide = one;
    wide.n_read_items = 1000; wide.n_pairs = 1000; wide.max_read_len = 1000;   // 5 MB of read arrays
    if (PdMultiFit().fits_with(wide) || PdInputLayout(1, 1000, 100, 1000).total <= kPdStageBytes) { std::fprintf(stderr, "inputs beyond kPdStageBytes fit\n"); return 1; }
  }
  for (int fma_mode = 0; fma_mode < 2; fma_mode++)
    for (int tail_mode = 0; tail_mode < 2; tail_mode++) {
      const PdPlanSettings set{fma_mode, tail_mode, 1, 1, fma_mode == 1};
      if (!check_cross_regions(set) || !check_slices(set)) return 1;
      const int width = fma_mode ? 8 : 4;
      for (const int n : {1, 2, 3, width - 1, width, width + 1, 63, 64, 65, 191, 192, 193, 200, 257, 300, pick(1, 400), pick(1, 400)})
        if (!check_paired_plan(set, n, 1)) return 1;
      for (const int n : {193, 400}) if (!check_paired_plan(set, n, 3)) return 1;   // sliced by hand
      {  // the cross layout's batch sizes through a striped tail: one read of kLongRead bases against width + 1 haplotypes
        PdPlanScratch scratch;
        const Inputs in = make_inputs(1, width + 1, 30, [&](int) { return kLongRead; });
        PdCrossPlan x;
        if (!plan_cross(set, &scratch, in.cross(0), &x)) return 1;
      }
      for (int round = 0; round < 75; round++) if (!check_multi(set, round)) return 1;   // 300 sets over the four settings
    }
  std::printf("ok: %lld regions, %lld multi sets, %lld striped reads, %lld table haplotypes, %lld odd haplotypes, %lld tail jobs, %lld striped tails, "
              "%lld sliced plans, %lld paired plans, %lld shared unions, %lld kept lists, %lld groups of several\n",
              g.regions, g.multi_sets, g.striped_reads, g.table_haps, g.odd_haps, g.tail_jobs, g.striped_tails, g.sliced_plans, g.paired_plans, g.union_shared,
              g.union_kept, g.grouped);
  return 0;
}
