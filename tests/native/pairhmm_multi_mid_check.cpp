// Stand-alone check of the mid-size part of gkl_amd/csrc/pairhmm_multi_sets.h (tests/test_pairhmm_multi_mid_cpu.py builds
// it with -fsanitize=address,undefined and expects exit 0).  A multi call cuts its regions twice, as dev_compute_host_multi
// does: the small ones with multi_cut_sets, where a mid-size region counts as "does not qualify", and the mid-size ones
// among themselves with multi_cut_mid_sets.  For a few hundred random lists of 0-200 regions of the four classes
// {small fused, small unfused, mid-size, not qualifying}:
//   * the small regions get exactly the sets they get when the mid-size regions are not in the list at all (a mid-size
//     region never interrupts a run of small ones), which is also what multi_cut_sets gives with them marked "does not
//     qualify";
//   * the mid-size sets hold 2 to kMultiMax regions, consecutive in mid-size input order, as few sets as hold them, of
//     sizes that differ by at most one; a lone mid-size region has no set; nothing else is in a mid-size set;
//   * per region of random size, the grids of its two policy launches: the flag blocks cover every pair once (the last
//     block may hold a single pair), and a strided walk b, b + g, b + 2 g, ... of g = multi_recompute_blocks(n_pairs)
//     blocks over a list of any count 0 .. n_pairs visits every entry exactly once.  (The grid functions are the ones the
//     host launches with; the walk is written out here as pair_recompute_block writes it -- this checks the arithmetic
//     of that grid, not the kernel's own loop.)
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

enum : uint8_t { kFused = 0, kUnfused = 1, kMid = 2, kNot = 3 };

int main(int argc, char** argv) {
  const int n_lists = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937 rng(20241019u);
  auto pick = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  long long mid_sets_seen = 0, lone_seen = 0, entries_seen = 0;
  for (int list = 0; list < n_lists; list++) {
    // (the first lists: empty, one mid-size region, two, exactly one full set, one over it, one between small ones)
    const int K = list == 0 ? 0 : list == 1 ? 1 : list == 2 ? 2 : list == 3 ? kMultiMax : list == 4 ? kMultiMax + 1 : list == 5 ? 3 : pick(0, 200);
    const int p_mid = pick(0, 100), p_not = pick(0, 40), p_fused = pick(0, 100);
    std::vector<uint8_t> cls((size_t)K);
    for (int k = 0; k < K; k++) {
      if (list < 5) cls[(size_t)k] = kMid;
      else if (list == 5) cls[(size_t)k] = k == 1 ? kMid : kFused;
      else cls[(size_t)k] = pick(1, 100) <= p_mid ? kMid : pick(1, 100) <= p_not ? kNot : pick(1, 100) <= p_fused ? kFused : kUnfused;
    }
    // the two cuts, as the host makes them
    std::vector<uint8_t> qualifies((size_t)K), kind((size_t)K), mid((size_t)K);
    for (int k = 0; k < K; k++) {
      qualifies[(size_t)k] = cls[(size_t)k] == kFused || cls[(size_t)k] == kUnfused;
      kind[(size_t)k] = cls[(size_t)k] == kFused;
      mid[(size_t)k] = cls[(size_t)k] == kMid;
    }
    std::vector<int32_t> set_of((size_t)K + 1, -7), mid_set_of((size_t)K + 1, -7);
    const int n_small_sets = multi_cut_sets(qualifies.data(), kind.data(), K, set_of.data());
    const int n_mid_sets = multi_cut_mid_sets(mid.data(), K, mid_set_of.data());
    CHECK(set_of[(size_t)K] == -7 && mid_set_of[(size_t)K] == -7, "wrote behind a set_of array");

    // ---- the small regions: the sets of the list without its mid-size regions ----
    {
      std::vector<int> at;   // the regions that are not mid-size, in input order
      std::vector<uint8_t> q2, k2;
      for (int k = 0; k < K; k++)
        if (!mid[(size_t)k]) { at.push_back(k); q2.push_back(qualifies[(size_t)k]); k2.push_back(kind[(size_t)k]); }
      std::vector<int32_t> s2(at.size() + 1, -7);
      const int n2 = multi_cut_sets(q2.data(), k2.data(), (int)at.size(), s2.data());
      CHECK(n2 == n_small_sets, "%d sets of small regions, %d without the mid-size regions", n_small_sets, n2);
      for (size_t i = 0; i < at.size(); i++)
        CHECK(set_of[(size_t)at[i]] == s2[i], "region %d: set %d, %d without the mid-size regions", at[i], set_of[(size_t)at[i]], s2[i]);
      for (int k = 0; k < K; k++)
        if (mid[(size_t)k]) CHECK(set_of[(size_t)k] == -1, "mid-size region %d is in small set %d", k, set_of[(size_t)k]);
    }

    // ---- the mid-size regions ----
    int n_mid = 0;
    for (int k = 0; k < K; k++) n_mid += mid[(size_t)k];
    std::vector<std::vector<int>> sets((size_t)n_mid_sets);
    int last_set = -1;
    for (int k = 0; k < K; k++) {
      const int s = mid_set_of[(size_t)k];
      if (!mid[(size_t)k]) { CHECK(s == -1, "region %d is not mid-size but is in mid-size set %d", k, s); continue; }
      if (n_mid < 2) { CHECK(s == -1 && n_mid_sets == 0, "a lone mid-size region (%d) has set %d of %d", k, s, n_mid_sets); lone_seen++; continue; }
      CHECK(s >= 0 && s < n_mid_sets, "region %d: set %d of %d", k, s, n_mid_sets);
      CHECK(s == last_set || s == last_set + 1, "region %d: set %d after set %d (input order)", k, s, last_set);
      last_set = s;
      sets[(size_t)s].push_back(k);
    }
    if (n_mid >= 2) {
      CHECK(last_set == n_mid_sets - 1, "%d sets, the last region is in set %d", n_mid_sets, last_set);
      CHECK(n_mid_sets == (n_mid + kMultiMax - 1) / kMultiMax, "%d mid-size regions in %d sets", n_mid, n_mid_sets);
      int lo = kMultiMax, hi = 0;
      for (const std::vector<int>& m : sets) {
        const int sz = (int)m.size();
        CHECK(sz >= 2 && sz <= kMultiMax, "a mid-size set of %d regions", sz);
        lo = sz < lo ? sz : lo; hi = sz > hi ? sz : hi;
        mid_sets_seen++;
      }
      CHECK(hi - lo <= 1, "mid-size sets of %d .. %d regions", lo, hi);
    }
    if (list == 1) CHECK(n_mid_sets == 0 && mid_set_of[0] == -1, "one mid-size region: %d sets", n_mid_sets);
    if (list == 2) CHECK(n_mid_sets == 1 && sets[0].size() == 2, "two mid-size regions: %d sets", n_mid_sets);
    if (list == 3) CHECK(n_mid_sets == 1 && sets[0].size() == (size_t)kMultiMax, "64 mid-size regions: %d sets", n_mid_sets);
    if (list == 4) CHECK(n_mid_sets == 2 && sets[0].size() == 33 && sets[1].size() == 32, "65 mid-size regions: %d sets", n_mid_sets);
    if (list == 5) CHECK(n_mid_sets == 0 && n_small_sets == 1 && set_of[0] == 0 && set_of[2] == 0, "small, mid-size, small: %d + %d sets", n_small_sets, n_mid_sets);

    // ---- the grids of a mid-size region's two policy launches ----
    for (int rep = 0; rep < 4; rep++) {
      const int shape = pick(0, 5);
      const int n_pairs = shape == 0 ? 2049 : shape == 1 ? 65536 : shape == 2 ? 256 * pick(9, 256) : shape == 3 ? 2100 : pick(2049, 65536);
      const int fb = multi_flag_blocks(n_pairs);
      CHECK((long long)fb * kFlagBlock >= n_pairs && (long long)(fb - 1) * kFlagBlock < n_pairs, "%d flag blocks for %d pairs", fb, n_pairs);
      if (n_pairs == 2049) CHECK(fb == 9, "2049 pairs: %d flag blocks", fb);
      const int g = multi_recompute_blocks(n_pairs);
      CHECK(g >= 256 && g >= n_pairs / 2 && (g == 256 || g == n_pairs / 2), "%d recomputation blocks for %d pairs", g, n_pairs);
      // counts: none, one, the grid and its neighbours, twice the grid, everything, anything
      const int counts[] = {0, 1, g - 1, g, g + 1, 2 * g, n_pairs, pick(0, n_pairs)};
      for (int n : counts) {
        if (n < 0 || n > n_pairs) continue;
        std::vector<uint8_t> hit((size_t)n, 0);
        int most = 0;
        for (int b = 0; b < g; b++) {
          int turns = 0;
          for (int i = b; i < n; i += g) {   // (the same stride as pair_recompute_block's loop, written out)
            CHECK(hit[(size_t)i] == 0, "entry %d of %d taken twice (grid %d)", i, n, g);
            hit[(size_t)i] = 1;
            turns++;
          }
          most = turns > most ? turns : most;
        }
        for (int i = 0; i < n; i++) CHECK(hit[(size_t)i] == 1, "entry %d of %d never taken (grid %d)", i, n, g);
        CHECK(most == (n + g - 1) / g, "a block took %d entries of %d (grid %d)", most, n, g);
        entries_seen += n;
      }
      if (n_pairs == 2100) CHECK(g == 1050, "2100 pairs: %d recomputation blocks (every block takes two pairs of a full list)", g);
    }
  }
  std::printf("ok: %d region lists, %lld mid-size sets, %lld lone mid-size regions, %lld list entries\n", n_lists, mid_sets_seen, lone_seen, entries_seen);
  return 0;
}
