// Stand-alone check of gkl_amd/csrc/pdhmm_multi_plan.h (tests/test_pdhmm_multi_plan_cpu.py builds it with
// -fsanitize=address,undefined and expects exit 0): for a few hundred random sets of 1-64 regions of 1-300 reads x 1-50
// haplotypes, with random chunk counts, random routing of the haplotypes to the three launches and random table groups,
//   * every unit of every launch maps to exactly one (region, item, chunk) and every (region, item, chunk) is some unit's;
//   * every output pair index is produced by exactly one (region, read, haplotype);
//   * the inverse mapping (pair -> region, read, haplotype) agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

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
  std::printf("ok: %d region sets, %lld units, %lld pairs\n", n_sets, units_seen, pairs_seen);
  return 0;
}
