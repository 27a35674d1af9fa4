// Stand-alone check of the rule by which a leader of concurrent callers picks its set (gkl_amd/csrc/pairhmm_multi_sets.h:
// CombinePick / combine_pick / combine_admits), on the host and under the sanitizers
// (tests/test_pairhmm_mid_combine_cpu.py builds it with -fsanitize=address,undefined).
//  - small kinds: exactly what the combiner's loop took before the rule had a name (written out below);
//  - mid-size kinds: the leader first, arrival order, the leader's kind and fma only, at most kCombineMax calls, the
//    set's pairs within kCombineMidPairs, FIRST FIT: a waiting call that does not fit is passed over and later ones
//    that fit still ride along -- so every call left behind is of another kind or mode, came after the set was full,
//    or did not fit at the moment it was looked at;
//  - the admission predicate: a free flight slot, and for a mid-size call fewer than kMidFlights mid-size sets in the air
//    (fewer than min(kMidFlights, slots - 1) where the combiner has two or three slots).
// combine_pick is the function SmallCombiner::run calls over its queue.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gkl_amd/csrc/pairhmm_multi_sets.h"

using namespace gklhip;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      fprintf(stderr, "FAILED %s (line %d, queue %d)\n", #cond, __LINE__, g_queue);  \
      exit(1);                                                                       \
    }                                                                                \
  } while (0)
static int g_queue = -1;

// the kinds as the library numbers them (pairhmm_aux_kernels.h); the rule only compares them
enum { kOneLaunch = 0, kFused = 1, kTwoStep = 2, kDouble = 3, kDoubleStream = 4 };
static bool is_mid(int kind) { return kind == kTwoStep || kind == kDoubleStream; }

// The loop of SmallCombiner::run as it was: the leader, then every waiting call of its fma mode and kind while the set
// holds fewer than kCombineMax.
static int old_loop(const std::vector<CombineCall>& q, int leader, int32_t* picked) {
  int n = 0;
  picked[n++] = leader;
  for (int i = 0; i < (int)q.size(); i++) {
    if (i == leader) continue;
    if (n < kCombineMax && q[(size_t)i].fma == q[(size_t)leader].fma && q[(size_t)i].kind == q[(size_t)leader].kind) picked[n++] = i;
  }
  return n;
}

int main() {
  static_assert(kCombineMidPairs == 131072 && kMidFlights == 2 && kCombineMax == 16, "the caps the documents state");
  std::mt19937 rng(75);
  auto uniform = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
  int n_small = 0, n_mid = 0, n_passed_over = 0, n_full = 0;
  for (g_queue = 0; g_queue < 400; g_queue++) {
    // a queue of 1 .. 40 waiting calls: a few kinds so that runs of one kind exceed kCombineMax now and then, mid-size
    // pair counts over the whole range with the ends over-represented
    // (every tenth queue is a crowd of one mid-size kind and mode with few pairs each: sets that fill up by count)
    const bool crowd = g_queue % 10 == 0;
    const int n = crowd ? uniform(20, 40) : uniform(1, 40);
    const int n_kinds = uniform(1, 5);
    std::vector<CombineCall> q((size_t)n);
    for (auto& c : q) {
      c.kind = crowd ? (g_queue % 20 == 0 ? kTwoStep : kDoubleStream) : uniform(0, n_kinds - 1) * (g_queue % 3 == 0 ? 2 : 1) % 5;
      c.fma = crowd || g_queue % 4 == 0 ? 1 : uniform(0, 1);
      if (is_mid(c.kind)) {
        const int how = uniform(0, 5);
        c.pairs = crowd ? uniform(2049, 6000) : how == 0 ? 2049 : how == 1 ? 65536 : how == 2 ? uniform(60000, 65536) : uniform(2049, 65536);
      } else {
        c.pairs = uniform(1, 2048);
      }
    }
    for (int leader = 0; leader < n; leader++) {
      const CombineCall& L = q[(size_t)leader];
      const bool mid = is_mid(L.kind);
      int32_t picked[kCombineMax + 1], old[kCombineMax + 1];
      picked[kCombineMax] = -77;   // (a canary behind what the function may write)
      const int m = combine_pick(q.data(), n, leader, mid, picked);
      CHECK(picked[kCombineMax] == -77);
      CHECK(m >= 1 && m <= kCombineMax && picked[0] == leader);
      if (!mid) {
        n_small++;
        const int mo = old_loop(q, leader, old);
        CHECK(m == mo);
        for (int i = 0; i < m; i++) CHECK(picked[i] == old[i]);
        continue;
      }
      n_mid++;
      int64_t total = L.pairs;
      for (int i = 1; i < m; i++) {
        const CombineCall& c = q[(size_t)picked[i]];
        CHECK(picked[i] != leader && picked[i] >= 0 && picked[i] < n);
        if (i > 1) CHECK(picked[i] > picked[i - 1]);   // arrival order
        CHECK(c.kind == L.kind && c.fma == L.fma);
        total += c.pairs;
      }
      CHECK(m == 1 || total <= kCombineMidPairs);   // (a leader goes whatever its size; at most 65 536 pairs here anyway)
      // first fit, replayed: every call not taken has its reason at the moment it was looked at
      int64_t running = L.pairs;
      int taken = 1;
      for (int i = 0; i < n; i++) {
        if (i == leader) continue;
        const CombineCall& c = q[(size_t)i];
        const bool like = c.kind == L.kind && c.fma == L.fma;
        const bool in_set = taken < m && picked[taken] == i;
        if (in_set) {
          CHECK(like && running + c.pairs <= kCombineMidPairs);
          running += c.pairs;
          taken++;
          continue;
        }
        if (!like) continue;
        if (taken >= kCombineMax) { n_full++; continue; }
        CHECK(running + c.pairs > kCombineMidPairs);   // passed over because it did not fit THEN
        n_passed_over++;
      }
      CHECK(taken == m && running == total);
    }
  }
  // a call that does not fit does not stop later, smaller ones
  {
    g_queue = -2;
    const CombineCall q[4] = {{kTwoStep, 1, 65536}, {kTwoStep, 1, 65000}, {kTwoStep, 1, 65536}, {kTwoStep, 1, 536}};
    int32_t picked[kCombineMax];
    CHECK(combine_pick(q, 4, 0, true, picked) == 3 && picked[0] == 0 && picked[1] == 1 && picked[2] == 3);
    CHECK(combine_pick(q, 4, 2, true, picked) == 2 && picked[0] == 2 && picked[1] == 0);   // (the first one fills the cap exactly)
    // the same triples as SMALL kinds are not capped
    const CombineCall s[4] = {{kOneLaunch, 1, 65536}, {kOneLaunch, 1, 65000}, {kOneLaunch, 1, 65536}, {kOneLaunch, 1, 536}};
    CHECK(combine_pick(s, 4, 0, false, picked) == 4);
    // exactly the cap fits, one pair more does not
    const CombineCall e[3] = {{kDoubleStream, 0, 65536}, {kDoubleStream, 0, 65536}, {kDoubleStream, 0, 2049}};
    CHECK(combine_pick(e, 3, 0, true, picked) == 2 && picked[1] == 1);
    const CombineCall f[3] = {{kDoubleStream, 0, 65536}, {kDoubleStream, 0, 65535}, {kDoubleStream, 0, 2049}};
    CHECK(combine_pick(f, 3, 0, true, picked) == 2 && picked[1] == 1);
    const CombineCall g[3] = {{kDoubleStream, 0, 65536}, {kDoubleStream, 0, 63487}, {kDoubleStream, 0, 2049}};
    CHECK(combine_pick(g, 3, 0, true, picked) == 3);
    // kinds and modes never mix, whatever the size
    const CombineCall h[4] = {{kTwoStep, 1, 2049}, {kDoubleStream, 1, 2049}, {kTwoStep, 0, 2049}, {kOneLaunch, 1, 100}};
    for (int leader = 0; leader < 4; leader++) CHECK(combine_pick(h, 4, leader, is_mid(h[leader].kind), picked) == 1);
  }
  // admission
  g_queue = -3;
  // (with fewer than four slots mid-size sets leave one to the small calls; one slot is whoever's comes first)
  static_assert(combine_mid_flights(4) == 2 && combine_mid_flights(3) == 2 && combine_mid_flights(2) == 1 && combine_mid_flights(1) == 1, "");
  for (int max_flights = 1; max_flights <= 4; max_flights++)
    for (int flights = 0; flights <= 5; flights++)
      for (int mid_flights = 0; mid_flights <= flights; mid_flights++) {
        const int mid_cap = max_flights == 1 ? 1 : max_flights - 1 < kMidFlights ? max_flights - 1 : kMidFlights;
        CHECK(combine_admits(false, flights, mid_flights, max_flights) == (flights < max_flights));
        CHECK(combine_admits(true, flights, mid_flights, max_flights) == (flights < max_flights && mid_flights < mid_cap));
        // with more than one slot, a small call finds one free whenever only admitted mid-size sets are in the air
        if (max_flights > 1 && flights == mid_flights && mid_flights <= mid_cap) CHECK(combine_admits(false, flights, mid_flights, max_flights));
      }
  CHECK(combine_admits(true, 2, 1, 4) && !combine_admits(true, 2, 2, 4) && combine_admits(false, 2, 2, 4) && combine_admits(false, 3, 2, 4));
  CHECK(combine_admits(true, 0, 0, 2) && !combine_admits(true, 1, 1, 2) && combine_admits(false, 1, 1, 2));
  printf("ok: 400 queues, %d small leaders like the old loop, %d mid-size leaders (%d calls passed over for the pair cap, %d left by full sets)\n",
         n_small, n_mid, n_passed_over, n_full);
  CHECK(n_small > 1000 && n_mid > 1000 && n_passed_over > 100 && n_full > 0);
  return 0;
}
