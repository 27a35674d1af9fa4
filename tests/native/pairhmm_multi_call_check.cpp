// Stand-alone check of gkl_amd/csrc/pairhmm_multi_call.h, the decisions of one multi-region PairHMM call
// (tests/test_pairhmm_multi_call_cpu.py builds it with -fsanitize=address,undefined and expects exit 0).  The driver runs
// over fake operations that record every call and fail where they are told to, for the fixed lists of 0, 1, 2, 64, 65, 66
// and 129 regions, a lone mid-size region between small ones, and a few hundred random lists of 0 - 200 regions of the
// classes {none, small fused, small one-launch, small double, mid-size, mid-size double} -- of an fp32 context, of a
// double-precision context, or mixed.  Checked per list:
//   * partition: every region ends as member of exactly one set that ran, or alone, or failed; nothing is staged after
//     its set ran, nothing runs that is not staged on the lane the driver says;
//   * sets: 1 .. kMultiMax members of one kind (mid-size: at least 2), all small sets before the mid-size ones, and the
//     membership is what multi_cut_sets / multi_cut_mid_sets give for the classes of the regions that were staged (up to
//     kMultiMax regions) or planned (more), less the members that fell away afterwards;
//   * the held rule of a double-precision context's first mid-size region; that an fp32 one is never held;
//   * longer lists: planned once on lane 0, once more on the lane they are staged on, lanes 0 .. m - 1 per set, a region
//     that changes its mind on the second plan goes alone and a mid-size set left with one member runs nobody;
//   * injected failures: a plan-side failure and a staging failure are the region's own, a set's failure is its members'
//     with the set's code, a mid-size set whose company failed to stage sends the survivor alone;
//   * lane ownership after the call: R[i].lane == l exactly when owner[l] == i, and only members of sets that ran have one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gkl_amd/csrc/pairhmm_multi_call.h"

using namespace gklhip;

static int g_list = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "list %d: %s failed: ", g_list, #cond);           \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

enum Cls : uint8_t { kNot = 0, kFused, kOneLaunch, kDouble, kMid, kMidDouble, kClasses };
static MultiClass class_of(Cls c) { return c == kNot ? kMultiNone : c >= kMid ? kMultiMid : kMultiSmall; }
static bool is_double(Cls c) { return c == kDouble || c == kMidDouble; }
enum { kPlanFailed = 55, kStageFailed = 66, kSetFailed = 77 };

struct Region {
  bool alone = false;
  int lane = -1;
};

struct Fake {
  enum Op { kPlan, kHold, kStage, kRun };
  struct Event { Op op; int i, lane; };
  int n;
  std::vector<Cls> first, second;                      // what the first and every later plan of a region say
  std::vector<char> fail_plan, fail_stage, fail_set;   // fail_set: a set with this member fails
  std::vector<Event> log;
  std::vector<std::vector<int>> plan_lanes, stage_lanes;   // per region, in order
  std::vector<int> stage_at;                           // per region: the log position of its last stage, -1: none
  std::vector<std::vector<int>> sets;                  // the sets that were run, failed ones too
  std::vector<int> set_rc, in_set, taken, failed;      // per set; per region: its set (-1), results taken, fail() code
  std::vector<int> content;                            // per lane: the region staged there
  int last_plan = -1, last_lane = -1, held = -1;
  std::vector<int> planned_since_hold;                 // lanes planned on since hold()

  Fake(const std::vector<Cls>& a, const std::vector<Cls>& b)
      : n((int)a.size()), first(a), second(b), fail_plan(a.size(), 0), fail_stage(a.size(), 0), fail_set(a.size(), 0), plan_lanes(a.size()), stage_lanes(a.size()),
        stage_at(a.size(), -1), in_set(a.size(), -1), taken(a.size(), 0), failed(a.size(), 0), content(kMultiMax, -1) {}

  MultiPlanned plan(int i, int lane) {
    CHECK(i >= 0 && i < n && lane >= 0 && lane < kMultiMax, "plan(%d, %d)", i, lane);
    CHECK(in_set[(size_t)i] < 0 && !failed[(size_t)i], "region %d is planned after it ran or failed", i);
    log.push_back({kPlan, i, lane});
    const bool again = !plan_lanes[(size_t)i].empty();
    plan_lanes[(size_t)i].push_back(lane);
    planned_since_hold.push_back(lane);
    last_plan = i; last_lane = lane;
    if (fail_plan[(size_t)i] && !again) { last_plan = -1; return {kPlanFailed, kMultiNone, 0, false}; }
    const Cls c = again ? second[(size_t)i] : first[(size_t)i];
    return {0, class_of(c), (uint8_t)(c + 10), is_double(c)};
  }
  void hold() {
    CHECK(last_plan >= 0 && first[(size_t)last_plan] == kMidDouble, "hold() after the plan of region %d", last_plan);
    CHECK(held < 0, "two plans held");
    log.push_back({kHold, last_plan, last_lane});
    held = last_plan;
    planned_since_hold.clear();
  }
  int stage(int i, int lane, bool from_held) {
    CHECK(i >= 0 && i < n && lane >= 0 && lane < kMultiMax, "stage(%d, %d)", i, lane);
    CHECK(in_set[(size_t)i] < 0 && !failed[(size_t)i], "region %d is staged after its set ran or it failed", i);
    CHECK(stage_lanes[(size_t)i].empty(), "region %d is staged twice", i);
    if (from_held) {
      CHECK(held == i && plan_lanes[(size_t)i].back() == lane, "stage(%d, %d, held) but %d is held", i, lane, held);
      for (int l : planned_since_hold) CHECK(l != lane, "lane %d was planned on again while it kept the held plan", lane);
      held = -1;
    } else {
      CHECK(last_plan == i && last_lane == lane, "stage(%d, %d) but the plan just made is (%d, %d)", i, lane, last_plan, last_lane);
    }
    stage_at[(size_t)i] = (int)log.size();
    log.push_back({kStage, i, lane});
    stage_lanes[(size_t)i].push_back(lane);
    content[(size_t)lane] = -1;   // (whatever was there is gone, whether this works or not)
    if (fail_stage[(size_t)i]) return kStageFailed;
    content[(size_t)lane] = i;
    return 0;
  }
  const Region* R = nullptr;
  int run(const int* members, int m) {
    CHECK(m >= 1 && m <= kMultiMax, "a set of %d", m);
    log.push_back({kRun, members[0], m});
    bool fails = false;
    for (int j = 0; j < m; j++) {
      const int i = members[j];
      CHECK(i >= 0 && i < n && in_set[(size_t)i] < 0, "region %d runs twice", i);
      CHECK(j == 0 || members[j - 1] < i, "members out of input order");
      CHECK(R[i].lane >= 0 && content[(size_t)R[i].lane] == i, "region %d runs but lane %d holds region %d", i, R[i].lane, R[i].lane < 0 ? -1 : content[(size_t)R[i].lane]);
      in_set[(size_t)i] = (int)sets.size();
      fails = fails || fail_set[(size_t)i];
    }
    sets.emplace_back(members, members + m);
    set_rc.push_back(fails ? kSetFailed : 0);
    return set_rc.back();
  }
  void take(int i, int j) {
    CHECK(!sets.empty() && set_rc.back() == 0 && j >= 0 && j < (int)sets.back().size() && sets.back()[(size_t)j] == i, "take(%d, %d)", i, j);
    taken[(size_t)i]++;
  }
  void fail(int i, int rc) {
    CHECK(rc != 0 && !failed[(size_t)i], "fail(%d, %d)", i, rc);
    failed[(size_t)i] = rc;
  }
};

struct Totals { long long lists = 0, regions = 0, sets = 0, held = 0, alone = 0, failed = 0, changed = 0; };

static void check_list(const std::vector<Cls>& first, const std::vector<Cls>& second, const std::vector<char>& fail_plan, const std::vector<char>& fail_stage,
                       const std::vector<char>& fail_set, Totals* T) {
  const int n = (int)first.size();
  const bool stage_first = n <= kMultiMax;
  Fake f(first, second);
  f.fail_plan = fail_plan; f.fail_stage = fail_stage; f.fail_set = fail_set;
  std::vector<Region> R((size_t)n);
  f.R = R.data();
  int32_t owner[kMultiMax + 1];
  for (int l = 0; l <= kMultiMax; l++) owner[l] = -1;
  owner[kMultiMax] = -7;
  multi_call_drive(R.data(), n, owner, f);
  CHECK(owner[kMultiMax] == -7, "wrote behind owner[]");
  CHECK(f.held < 0 || f.stage_lanes[(size_t)f.held].empty(), "a held plan");

  // ---- what the cuts say for the classes the driver had when it cut ----
  // up to kMultiMax regions: a region counts as its class when it was staged (or held to the end); more: as first planned
  std::vector<uint8_t> small((size_t)n), mid((size_t)n), kind((size_t)n);
  for (int i = 0; i < n; i++) {
    const Cls c = first[(size_t)i];
    const bool staged_ok = !f.stage_lanes[(size_t)i].empty() && !fail_stage[(size_t)i];
    const bool held_to_the_end = f.stage_lanes[(size_t)i].empty() && c == kMidDouble;
    const bool counts = !fail_plan[(size_t)i] && c != kNot && (!stage_first || staged_ok || held_to_the_end);
    small[(size_t)i] = counts && class_of(c) == kMultiSmall;
    mid[(size_t)i] = counts && class_of(c) == kMultiMid;
    kind[(size_t)i] = (uint8_t)(c + 10);
  }
  std::vector<int32_t> set_of((size_t)n + 1), mid_set_of((size_t)n + 1);
  const int n_small_sets = multi_cut_sets(small.data(), kind.data(), n, set_of.data());
  const int n_mid_sets = multi_cut_mid_sets(mid.data(), n, mid_set_of.data());
  // ... less the members that fell away after the cut (longer lists only: changed their mind, failed to stage)
  std::vector<std::vector<int>> want;
  std::vector<int> want_mid;   // per wanted set: is it mid-size
  for (int pass = 0; pass < 2; pass++)
    for (int s = 0; s < (pass ? n_mid_sets : n_small_sets); s++) {
      std::vector<int> m;
      for (int i = 0; i < n; i++) {
        if ((pass ? mid_set_of : set_of)[(size_t)i] != s || !(pass ? mid : small)[(size_t)i]) continue;
        if (!stage_first && (second[(size_t)i] != first[(size_t)i] || fail_stage[(size_t)i])) continue;
        m.push_back(i);
      }
      if (m.empty() || (pass == 1 && m.size() == 1)) continue;
      want.push_back(m);
      want_mid.push_back(pass);
    }
  CHECK(f.sets.size() == want.size(), "%zu sets ran, the cuts give %zu", f.sets.size(), want.size());
  bool seen_mid = false;
  for (size_t s = 0; s < want.size(); s++) {
    CHECK(f.sets[s] == want[s], "set %zu: not the members the cut gives (first %d, %zu members; wanted first %d, %zu)", s, f.sets[s][0], f.sets[s].size(), want[s][0], want[s].size());
    const std::vector<int>& m = f.sets[s];
    CHECK((int)m.size() <= kMultiMax && (!want_mid[s] || m.size() >= 2), "a set of %zu", m.size());
    for (int i : m) CHECK(first[(size_t)i] == first[(size_t)m[0]] || (want_mid[s] && class_of(first[(size_t)i]) == kMultiMid), "set %zu mixes kinds", s);
    for (int i : m) CHECK(want_mid[s] == (class_of(first[(size_t)i]) == kMultiMid), "set %zu mixes classes", s);
    CHECK(want_mid[s] || !seen_mid, "a small set after a mid-size one");
    seen_mid = seen_mid || want_mid[s];
    if (!stage_first)
      for (size_t j = 0; j < m.size(); j++) CHECK(f.stage_lanes[(size_t)m[j]].back() == (int)j, "set %zu: member %zu was staged on lane %d", s, j, f.stage_lanes[(size_t)m[j]].back());
    T->sets++;
  }

  // ---- partition, failures, lanes ----
  int n_mid_first = 0, first_mid = -1, second_mid = -1;
  for (int i = 0; i < n; i++)
    if (class_of(first[(size_t)i]) == kMultiMid && !fail_plan[(size_t)i]) { if (n_mid_first == 0) first_mid = i; if (n_mid_first == 1) second_mid = i; n_mid_first++; }
  for (int i = 0; i < n; i++) {
    const Region& r = R[(size_t)i];
    const int s = f.in_set[(size_t)i];
    const bool ran = s >= 0 && f.set_rc[(size_t)s] == 0;
    const int rc = f.failed[(size_t)i];
    CHECK((int)ran + (int)r.alone + (int)(rc != 0) == 1, "region %d: ran %d, alone %d, failed %d", i, (int)ran, (int)r.alone, rc);
    CHECK(f.taken[(size_t)i] == (ran ? 1 : 0), "region %d: results taken %d times", i, f.taken[(size_t)i]);
    CHECK(s < 0 || ran || rc == kSetFailed, "region %d was in a failed set and has code %d", i, rc);
    CHECK((rc == kSetFailed) == (s >= 0 && !ran), "region %d has the set's code without a failed set", i);
    CHECK((rc == kPlanFailed) == (bool)fail_plan[(size_t)i], "region %d: plan failure %d, code %d", i, (int)fail_plan[(size_t)i], rc);
    CHECK((rc == kStageFailed) == (fail_stage[(size_t)i] && !f.stage_lanes[(size_t)i].empty()), "region %d: staging failure, code %d", i, rc);
    CHECK(first[(size_t)i] != kNot || fail_plan[(size_t)i] || (r.alone && f.plan_lanes[(size_t)i].size() == 1 && f.stage_lanes[(size_t)i].empty()), "region %d does not qualify", i);
    CHECK((r.lane >= 0) <= ran, "region %d keeps lane %d but did not run", i, r.lane);
    if (r.lane >= 0) CHECK(r.lane < kMultiMax && owner[r.lane] == i, "region %d: lane %d is owned by %d", i, r.lane, owner[r.lane]);
    // plans: one per region, and in a longer list one more for each member of a cut set, on the lane it is staged on
    const bool in_cut = small[(size_t)i] ? set_of[(size_t)i] >= 0 : mid[(size_t)i] && mid_set_of[(size_t)i] >= 0;
    CHECK(f.plan_lanes[(size_t)i].size() == (size_t)(!stage_first && in_cut ? 2 : 1), "region %d was planned %zu times", i, f.plan_lanes[(size_t)i].size());
    CHECK(f.plan_lanes[(size_t)i][0] == (stage_first ? i : 0), "region %d was first planned on lane %d", i, f.plan_lanes[(size_t)i][0]);
    if (!f.stage_lanes[(size_t)i].empty()) CHECK(f.stage_lanes[(size_t)i][0] == f.plan_lanes[(size_t)i].back(), "region %d: planned on lane %d, staged on %d", i, f.plan_lanes[(size_t)i].back(), f.stage_lanes[(size_t)i][0]);
    if (!stage_first && in_cut && second[(size_t)i] != first[(size_t)i]) {
      CHECK(r.alone && f.stage_lanes[(size_t)i].empty(), "region %d changed its mind on the second plan", i);
      T->changed++;
    }
    T->alone += r.alone; T->failed += rc != 0;
  }
  for (int l = 0; l < kMultiMax; l++)
    if (owner[l] >= 0) CHECK(owner[l] < n && R[(size_t)owner[l]].lane == l, "lane %d is owned by region %d, whose lane is %d", l, owner[l], R[(size_t)owner[l]].lane);

  // ---- the held rule (up to kMultiMax regions) ----
  int holds = 0;
  for (const Fake::Event& e : f.log) holds += e.op == Fake::kHold;
  if (stage_first && first_mid >= 0 && first[(size_t)first_mid] == kMidDouble) {
    CHECK(holds == 1 && f.plan_lanes[(size_t)first_mid].size() == 1, "the first mid-size region of a double-precision context: %d holds", holds);
    if (n_mid_first == 1) {
      CHECK(f.stage_lanes[(size_t)first_mid].empty() && R[(size_t)first_mid].alone, "a lone held region was staged");
    } else {
      // staged immediately before the second one, and with it in one set (where neither fails)
      CHECK(f.stage_at[(size_t)first_mid] >= 0 && f.stage_at[(size_t)second_mid] == f.stage_at[(size_t)first_mid] + 1, "held region %d staged at %d, the second (%d) at %d", first_mid,
            f.stage_at[(size_t)first_mid], second_mid, f.stage_at[(size_t)second_mid]);
      if (!fail_stage[(size_t)first_mid] && !fail_stage[(size_t)second_mid])
        CHECK(f.in_set[(size_t)first_mid] >= 0 && f.in_set[(size_t)first_mid] == f.in_set[(size_t)second_mid], "the held region and the second are not in one set");
    }
    T->held++;
  } else {
    // an fp32 first mid-size region is never held -- unless it failed to stage and a double one follows as "the first"
    bool fp32_first_failed = first_mid >= 0 && fail_stage[(size_t)first_mid];
    CHECK(holds == 0 || (stage_first && fp32_first_failed), "%d holds without a double-precision first mid-size region", holds);
  }
  CHECK(stage_first || holds == 0, "a longer list holds a plan");
  T->lists++; T->regions += n;
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 400;
  std::mt19937 rng(20261020u);
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  Totals T;
  const int fixed[] = {0, 1, 2, 64, 65, 66, 129};
  const Cls fp32_classes[] = {kNot, kFused, kOneLaunch, kMid}, double_classes[] = {kNot, kDouble, kMidDouble};
  // the fixed lists: all of one class, for each class; and alternating classes of one context
  for (int n : fixed)
    for (int variant = 0; variant < kClasses + 2; variant++) {
      std::vector<Cls> c((size_t)n);
      for (int i = 0; i < n; i++)
        c[(size_t)i] = variant < kClasses ? (Cls)variant : variant == kClasses ? fp32_classes[i % 4] : double_classes[i % 3];
      const std::vector<char> none((size_t)n, 0);
      check_list(c, c, none, none, none, &T);
      g_list++;
    }
  // a lone mid-size region between small ones, of either context; and the held rule's cases written out
  const std::vector<std::vector<Cls>> written = {
      {kFused, kMid, kFused}, {kDouble, kMidDouble, kDouble}, {kMidDouble}, {kMidDouble, kMidDouble}, {kMidDouble, kDouble, kNot, kMidDouble, kMidDouble},
      {kMid}, {kMid, kMid}, {kMid, kFused, kMid}, {kMid, kMidDouble}, {kMidDouble, kMid}};
  for (const std::vector<Cls>& c : written) {
    const std::vector<char> none(c.size(), 0);
    check_list(c, c, none, none, none, &T);
    // ... and with each single region failing to plan, to stage, and its set failing
    for (size_t k = 0; k < c.size(); k++)
      for (int what = 0; what < 3; what++) {
        std::vector<char> fp(c.size(), 0), fs(c.size(), 0), fx(c.size(), 0);
        (what == 0 ? fp : what == 1 ? fs : fx)[k] = 1;
        check_list(c, c, fp, fs, fx, &T);
      }
    g_list++;
  }
  // random lists: without failures, then with failures and (longer lists) regions that change their mind
  for (int list = 0; list < n_random; list++, g_list++) {
    const int n = list % 7 == 0 ? pick(kMultiMax - 2, kMultiMax + 3) : pick(0, 200);
    const int context = pick(0, 2);   // fp32, double precision, mixed
    const int p_mid = pick(0, 100) < 30 ? pick(0, 3) : pick(0, 60), p_not = pick(0, 40);
    std::vector<Cls> c((size_t)n), c2;
    for (int i = 0; i < n; i++) {
      const bool dbl = context == 1 || (context == 2 && pick(0, 1));
      const int x = pick(1, 100);
      c[(size_t)i] = x <= p_not ? kNot : x <= p_not + p_mid ? (dbl ? kMidDouble : kMid) : dbl ? kDouble : pick(0, 1) ? kFused : kOneLaunch;
    }
    const std::vector<char> none((size_t)n, 0);
    check_list(c, c, none, none, none, &T);
    const int p_fail = pick(0, 12), p_change = pick(0, 10);
    std::vector<char> fp((size_t)n), fs((size_t)n), fx((size_t)n);
    c2 = c;
    for (int i = 0; i < n; i++) {
      fp[(size_t)i] = pick(1, 100) <= p_fail;
      fs[(size_t)i] = pick(1, 100) <= p_fail;
      fx[(size_t)i] = pick(1, 400) <= p_fail;
      if (pick(1, 100) <= p_change) c2[(size_t)i] = (Cls)pick(0, kClasses - 1);
    }
    check_list(c, c2, fp, fs, fx, &T);
    // a mid-size set of two whose first member fails to stage: the survivor goes alone
    if (list % 5 == 0) {
      std::vector<Cls> two = c;
      two.push_back(kMid); two.push_back(kMid);
      std::vector<char> fs2((size_t)n + 2, 0);
      int n_mid = 0;
      for (Cls x : two) n_mid += class_of(x) == kMultiMid;
      if (n_mid == 2) {
        fs2[(size_t)n] = 1;
        const std::vector<char> none2((size_t)n + 2, 0);
        check_list(two, two, none2, fs2, none2, &T);
      }
    }
  }
  std::printf("ok: %lld region lists, %lld regions, %lld sets, %lld held plans, %lld regions alone, %lld failed, %lld changed their mind\n", T.lists, T.regions, T.sets,
              T.held, T.alone, T.failed, T.changed);
  return 0;
}
