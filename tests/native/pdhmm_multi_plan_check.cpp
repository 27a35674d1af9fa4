// Stand-alone check of gkl_amd/csrc/pdhmm_multi_plan.h (tests/test_pdhmm_multi_plan_cpu.py builds it with
// -fsanitize=address,undefined and expects exit 0): for a few hundred random sets of 1-64 regions of 1-300 reads x 1-50
// haplotypes, with random chunk counts, random routing of the haplotypes to the three launches and random table groups,
//   * every unit of every launch maps to exactly one (region, item, chunk) and every (region, item, chunk) is some unit's;
//   * every output pair index is produced by exactly one (region, read, haplotype);
//   * the inverse mapping (pair -> region, read, haplotype) agrees.
// And of gkl_amd/csrc/pdhmm_job_layout.h (check_layouts): the blocks of a single call's job tables and of the paired table
// route's scratch are 256-byte aligned, disjoint, in the documented order and end at the total.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gkl_amd/csrc/pdhmm_job_layout.h"
#include "../../gkl_amd/csrc/pdhmm_multi_plan.h"

using namespace gklhip;

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "set %d: %s failed: ", set, #cond);               \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      return 1;                                                              \
    }                                                                        \
  } while (0)

// The blocks of a layout in their documented order: every offset a multiple of 256, block i + 1 at or behind block i's
// end (bytes[i] behind its start: disjoint, in order), the total = the end of the last block rounded up to 256.
static int check_blocks(int set, const char* what, const std::vector<size_t>& at, const std::vector<size_t>& bytes, size_t total) {
  for (size_t i = 0; i < at.size(); i++) {
    CHECK(at[i] % 256 == 0, "%s: block %zu at %zu", what, i, at[i]);
    const size_t end = at[i] + pd_up(bytes[i]), next = i + 1 < at.size() ? at[i + 1] : total;
    CHECK(at[i] + bytes[i] <= next, "%s: block %zu [%zu, +%zu) runs into the next at %zu", what, i, at[i], bytes[i], next);
    CHECK(next == end, "%s: block %zu ends at %zu, the next starts at %zu", what, i, end, next);
  }
  CHECK(at.empty() || at[0] == 0, "%s: the first block at %zu", what, at[0]);
  CHECK(total % 256 == 0, "%s: total %zu", what, total);
  return 0;
}
static std::vector<size_t> job_blocks(const PdJobLayout& L) {
  return {L.jl, L.jp, L.jn, L.js, L.cl, L.ho, L.cs, L.cr, L.tl, L.tp, L.tn, L.ts, L.nc, L.cc, L.jf, L.pc, L.pl, L.cu, L.fj, L.tg};
}
static int check_job_layout(int set, const PdJobCounts& n) {
  const PdJobLayout L(n);
  const std::vector<size_t> bytes = {n.n_general * 512, n.n_general * 4, n.n_general * 4, n.n_general, n.n_chunks_cross * 512, n.n_haps_cross * 4,
                                     n.n_chunks_cross * 4, n.n_chunks_cross * 4, n.n_tail * 512, n.n_tail * 4, n.n_tail * 4, n.n_tail,
                                     n.n_haps_cross, n.n_haps_cross * 32, n.n_general, n.n_placed * 4, n.n_placed, n.n_chunks_paired,
                                     n.n_general * 4, n.n_tab_starts * 4};
  return check_blocks(set, "jobs", job_blocks(L), bytes, L.total);
}
static int check_tabx_layout(int set, size_t nh, size_t n_general, size_t entry_stride, bool with_ns) {
  const PdTabxLayout X(nh, n_general, entry_stride, with_ns);
  return check_blocks(set, "tabx", {X.nc, X.cc, X.sb, X.nt, X.hj, X.ns}, {nh, nh * 32, nh * (entry_stride / 64) * 8, n_general, n_general * 4,
                      with_ns ? n_general * entry_stride * 4 : 0}, X.total);
}

// gkl_amd/csrc/pdhmm_job_layout.h: a single call's job tables and the paired table route's scratch, for random counts
// (zeros included) and for four hand-written count sets against offsets worked out from the formulae that the layouts
// replaced (the chains of o_* / x_* sums in pd_run_locked before it was split into steps).
static int check_layouts(std::mt19937& rng) {
  auto pick = [&](int lo, int hi) { return (size_t)std::uniform_int_distribution<int>(lo, hi)(rng); };
  auto count = [&](int hi) { return pick(0, 3) == 0 ? (size_t)0 : pick(0, hi); };
  for (int set = 0; set < 400; set++) {
    const PdJobCounts n{count(3000), count(40), count(300), count(70), count(100000), count(3000), count(60)};
    if (const int rc = check_job_layout(set, n)) return rc;
    if (const int rc = check_tabx_layout(set, count(100000), n.n_general, 64 * pick(3, 190), pick(0, 1) != 0)) return rc;
  }
  struct Fixed {
    PdJobCounts n;
    size_t nh, entry_stride;
    bool with_ns;
    size_t jobs[21], tabx[7];   // the blocks in order, then the total
  };
  static const Fixed fixed[4] = {
      // paired, 37 pairs in 3 chunks, a tail of 5, the whole-job program's step tables
      {{3, 0, 0, 5, 37, 3, 0}, 37, 448, true,
       {0, 1536, 1792, 2048, 2304, 2304, 2304, 2304, 2304, 4864, 5120, 5376, 5632, 5632, 5632, 5888, 6144, 6400, 6656, 6912, 6912},
       {0, 256, 1536, 3840, 4096, 4352, 9728}},
      // paired, two striped pairs and nothing packed
      {{2, 0, 0, 0, 2, 0, 0}, 2, 640, false,
       {0, 1024, 1280, 1536, 1792, 1792, 1792, 1792, 1792, 1792, 1792, 1792, 1792, 1792, 1792, 2048, 2304, 2560, 2560, 2816, 2816},
       {0, 256, 512, 768, 1024, 1280, 1280}},
      // cross, 5 haplotypes x (2 chunks + 1 striped read), a tail of 4, two table groups
      {{5, 2, 5, 4, 0, 0, 3}, 5, 512, false,
       {0, 2560, 2816, 3072, 3328, 4352, 4608, 4864, 5120, 7168, 7424, 7680, 7936, 8192, 8448, 8704, 8704, 8704, 8704, 8960, 9216},
       {0, 256, 512, 1024, 1280, 1536, 1536}},
      // cross, 6 haplotypes x 1 chunk, nothing listed, no tail, no table haplotype
      {{0, 1, 6, 0, 0, 0, 0}, 6, 384, false,
       {0, 0, 0, 0, 0, 512, 768, 1024, 1280, 1280, 1280, 1280, 1280, 1536, 1792, 1792, 1792, 1792, 1792, 1792, 1792},
       {0, 256, 512, 1024, 1024, 1024, 1024}},
  };
  for (int set = 0; set < 4; set++) {
    const Fixed& f = fixed[set];
    const PdJobLayout L(f.n);
    std::vector<size_t> got = job_blocks(L);
    got.push_back(L.total);
    for (size_t i = 0; i < got.size(); i++) CHECK(got[i] == f.jobs[i], "jobs: value %zu is %zu, expected %zu", i, got[i], f.jobs[i]);
    const PdTabxLayout X(f.nh, f.n.n_general, f.entry_stride, f.with_ns);
    const size_t gx[7] = {X.nc, X.cc, X.sb, X.nt, X.hj, X.ns, X.total};
    for (size_t i = 0; i < 7; i++) CHECK(gx[i] == f.tabx[i], "tabx: value %zu is %zu, expected %zu", i, gx[i], f.tabx[i]);
    if (const int rc = check_job_layout(set, f.n)) return rc;
    if (const int rc = check_tabx_layout(set, f.nh, f.n.n_general, f.entry_stride, f.with_ns)) return rc;
  }
  return 0;
}

int main(int argc, char** argv) {
  const int n_sets = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937 rng(20240611u);
  auto pick = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  long long units_seen = 0, pairs_seen = 0;
  for (int set = 0; set < n_sets; set++) {
    const int K = set < 4 ? (set == 0 ? 1 : set == 1 ? 64 : set + 1) : pick(1, kPdMaxRegions);
    std::vector<PdRegionShape> shapes((size_t)K);
    for (PdRegionShape& s : shapes) {
      s.n_reads = pick(1, 300);
      s.n_haps = pick(1, 50);
      // chunks: none when every read is striped, else at most one per read (a read takes at least one lane of 64)
      s.n_chunks = pick(0, 9) == 0 ? 0 : pick(1, std::min(s.n_reads, 12));
      const int n_tab = pick(0, 3) == 0 ? 0 : pick(0, s.n_haps), n_hot = pick(0, s.n_haps - n_tab);
      s.n_items[kPdLaunchTab] = n_tab == 0 ? 0 : pick((n_tab + 5) / 6, n_tab);   // groups of one to six table haplotypes
      s.n_items[kPdLaunchHot] = n_hot;
      s.n_items[kPdLaunchFull] = s.n_haps - n_tab - n_hot;
    }
    std::vector<PdRegion> t((size_t)K + 1);
    pd_build_regions(shapes.data(), K, t.data());

    // units
    for (int launch = 0; launch < 3; launch++) {
      const int n_units = t[(size_t)K].unit_start[launch];
      long long expect = 0;
      for (const PdRegionShape& s : shapes) expect += (long long)s.n_items[launch] * s.n_chunks;
      CHECK(n_units == expect, "launch %d: %d units, expected %lld", launch, n_units, expect);
      // (item, chunk) cells of the launch: items and chunks are numbered across the regions
      const int n_items = t[(size_t)K].list_start[launch], n_chunks = t[(size_t)K].chunk_base;
      std::vector<uint8_t> cell((size_t)n_items * (size_t)std::max(n_chunks, 1), 0);
      for (int u = 0; u < n_units; u++) {
        const int k = pd_region_of_unit(t.data(), K, launch, u);
        CHECK(k >= 0 && k < K, "unit %d: region %d", u, k);
        CHECK(u >= t[(size_t)k].unit_start[launch] && u < t[(size_t)k + 1].unit_start[launch], "unit %d outside region %d", u, k);
        int item, chunk;
        pd_unit_split(t[(size_t)k], launch, u, &item, &chunk);
        CHECK(item >= t[(size_t)k].list_start[launch] && item < t[(size_t)k + 1].list_start[launch], "unit %d: item %d outside region %d", u, item, k);
        CHECK(chunk >= t[(size_t)k].chunk_base && chunk < t[(size_t)k + 1].chunk_base, "unit %d: chunk %d outside region %d", u, chunk, k);
        uint8_t& c = cell[(size_t)item * (size_t)n_chunks + (size_t)chunk];
        CHECK(c == 0, "launch %d: (item %d, chunk %d) produced twice", launch, item, chunk);
        c = 1;
        units_seen++;
      }
      // every cell of every region was hit: n_units distinct cells inside the regions' own blocks, and the blocks hold n_units
    }

    // pairs
    const int n_pairs = t[(size_t)K].pair_base;
    std::vector<uint8_t> hit((size_t)n_pairs, 0);
    for (int k = 0; k < K; k++) {
      const PdRegion& r = t[(size_t)k];
      CHECK(r.n_haps == shapes[(size_t)k].n_haps, "region %d: n_haps", k);
      for (int ri = r.read_base; ri < t[(size_t)k + 1].read_base; ri++)
        for (int hi = r.hap_base; hi < t[(size_t)k + 1].hap_base; hi++) {
          const int p = pd_pair_index(r, ri, hi);
          CHECK(p >= 0 && p < n_pairs, "pair %d of (%d, %d, %d)", p, k, ri, hi);
          CHECK(hit[(size_t)p] == 0, "pair %d produced twice", p);
          hit[(size_t)p] = 1;
          // read-major inside the region, like a single call's output
          CHECK(p - r.pair_base == (ri - r.read_base) * r.n_haps + (hi - r.hap_base), "pair %d is not read-major", p);
          const int k2 = pd_region_of_pair(t.data(), K, p);
          int ri2, hi2;
          pd_pair_split(t[(size_t)k2], p, &ri2, &hi2);
          CHECK(k2 == k && ri2 == ri && hi2 == hi, "pair %d: (%d, %d, %d) came back as (%d, %d, %d)", p, k, ri, hi, k2, ri2, hi2);
          pairs_seen++;
        }
    }
    for (int p = 0; p < n_pairs; p++) CHECK(hit[(size_t)p] == 1, "pair %d never produced", p);
  }
  if (const int rc = check_layouts(rng)) return rc;
  std::printf("ok: %d region sets, %lld units, %lld pairs\n", n_sets, units_seen, pairs_seen);
  return 0;
}
