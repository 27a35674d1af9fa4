// Stand-alone check of gkl_amd/csrc/pairhmm_multi_sets.h (tests/test_pairhmm_multi_sets_cpu.py builds it with
// -fsanitize=address,undefined and expects exit 0): for a few hundred random region lists of 0-200 regions with random
// qualify / kind flags and random block counts (0 and 1 included),
//   * the sets hold at most kMultiMax regions, are of one kind, take every qualifying region exactly once and in input
//     order, and a run of one kind is cut into as few sets as hold it, of sizes that differ by at most one;
//   * in a launch of every set, every block maps to exactly one (region, local block) inside that region's range, and
//     every (region, local block) maps back to its block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gkl_amd/csrc/pairhmm_multi_sets.h"

using namespace gklhip;

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "list %d: %s failed: ", list, #cond);             \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const int n_lists = argc > 1 ? std::atoi(argv[1]) : 300;
  static_assert(kCombineMax <= kMultiMax, "a combiner's set fits the kernels' table");
  std::mt19937 rng(20241018u);
  auto pick = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  long long sets_seen = 0, blocks_seen = 0;
  for (int list = 0; list < n_lists; list++) {
    // (the first lists: empty, one region, exactly one full set, one over it, all of one kind)
    const int K = list == 0 ? 0 : list == 1 ? 1 : list == 2 ? kMultiMax : list == 3 ? kMultiMax + 1 : pick(0, 200);
    const int p_qualify = list < 5 ? 100 : pick(0, 100), p_kind = list < 5 ? 0 : pick(0, 100);
    std::vector<uint8_t> qualifies((size_t)K), kind((size_t)K);
    std::vector<int32_t> blocks((size_t)K);
    for (int k = 0; k < K; k++) {
      qualifies[(size_t)k] = pick(1, 100) <= p_qualify;
      kind[(size_t)k] = pick(1, 100) <= p_kind;
      const int shape = pick(0, 9);
      blocks[(size_t)k] = shape == 0 ? 0 : shape <= 2 ? 1 : shape <= 7 ? pick(2, 40) : pick(41, 2048);
    }
    // the sets
    std::vector<int32_t> set_of((size_t)K + 1, -7);
    const int n_sets = multi_cut_sets(qualifies.data(), kind.data(), K, set_of.data());
    CHECK(set_of[(size_t)K] == -7, "wrote behind set_of");
    std::vector<std::vector<int>> sets((size_t)n_sets);
    int last_set = -1;
    for (int k = 0; k < K; k++) {
      const int s = set_of[(size_t)k];
      if (!qualifies[(size_t)k]) { CHECK(s == -1, "region %d does not qualify but is in set %d", k, s); continue; }
      CHECK(s >= 0 && s < n_sets, "region %d: set %d of %d", k, s, n_sets);
      CHECK(s == last_set || s == last_set + 1, "region %d: set %d after set %d (input order)", k, s, last_set);
      last_set = s;
      sets[(size_t)s].push_back(k);
    }
    CHECK(last_set == n_sets - 1, "%d sets, the last region is in set %d", n_sets, last_set);
    for (size_t s = 0; s < sets.size(); s++) {
      const std::vector<int>& m = sets[s];
      CHECK(!m.empty() && (int)m.size() <= kMultiMax, "set %zu holds %zu regions", s, m.size());
      for (int k : m) CHECK(kind[(size_t)k] == kind[(size_t)m[0]], "set %zu mixes kinds", s);
    }
    // a run of one kind is cut into as few sets as hold it, of sizes that differ by at most one
    for (size_t s = 0; s < sets.size();) {
      size_t e = s;
      int total = 0, lo = kMultiMax, hi = 0;
      while (e < sets.size() && kind[(size_t)sets[e][0]] == kind[(size_t)sets[s][0]]) {
        const int sz = (int)sets[e].size();
        total += sz; lo = sz < lo ? sz : lo; hi = sz > hi ? sz : hi;
        e++;
      }
      CHECK((int)(e - s) == (total + kMultiMax - 1) / kMultiMax, "a run of %d regions in %zu sets", total, e - s);
      CHECK(hi - lo <= 1, "a run's sets hold %d .. %d regions", lo, hi);
      s = e;
    }
    if (list == 3) CHECK(n_sets == 2 && sets[0].size() == 33 && sets[1].size() == 32, "65 regions of one kind: %d sets", n_sets);
    // one launch per set
    for (const std::vector<int>& m : sets) {
      const int n = (int)m.size();
      std::vector<int32_t> b((size_t)n), begin((size_t)n + 1, -1);
      for (int i = 0; i < n; i++) b[(size_t)i] = blocks[(size_t)m[(size_t)i]];
      multi_begin(b.data(), n, begin.data());
      long long grid = 0;
      for (int i = 0; i < n; i++) {
        CHECK(begin[(size_t)i] == grid, "begin[%d] = %d, expected %lld", i, begin[(size_t)i], grid);
        grid += b[(size_t)i];
      }
      CHECK(begin[(size_t)n] == grid, "grid %d, expected %lld", begin[(size_t)n], grid);
      std::vector<std::vector<uint8_t>> hit((size_t)n);
      for (int i = 0; i < n; i++) hit[(size_t)i].assign((size_t)b[(size_t)i], 0);
      for (int block = 0; block < (int)grid; block++) {
        const int r = multi_find(begin.data(), n, block);
        CHECK(r >= 0 && r < n, "block %d: call %d of %d", block, r, n);
        CHECK(block >= begin[(size_t)r] && block < begin[(size_t)r + 1], "block %d outside call %d", block, r);
        const int local = multi_local(begin.data(), r, block);
        CHECK(local >= 0 && local < b[(size_t)r], "block %d: local %d of %d", block, local, b[(size_t)r]);
        CHECK(hit[(size_t)r][(size_t)local] == 0, "(call %d, local %d) produced twice", r, local);
        hit[(size_t)r][(size_t)local] = 1;
        CHECK(multi_block(begin.data(), r, local) == block, "(call %d, local %d) does not map back to block %d", r, local, block);
        blocks_seen++;
      }
      for (int i = 0; i < n; i++)
        for (int l = 0; l < b[(size_t)i]; l++) CHECK(hit[(size_t)i][(size_t)l] == 1, "(call %d, local %d) never produced", i, l);
      sets_seen++;
    }
  }
  std::printf("ok: %d region lists, %lld sets, %lld blocks\n", n_lists, sets_seen, blocks_seen);
  return 0;
}
