// What one multi-region PairHMM call (gklhip_compute_multi, gklhip_compute_multi_device) DECIDES: which regions are staged
// on which lane and when, which sets run in which order, what becomes of a region that fails or finds no set.  Everything
// that touches the device is behind four operations (MultiCallOps in pairhmm_host_call.h; fakes that record and fail on
// demand in tests/native/pairhmm_multi_call_check.cpp, which compiles this header for the host alone under the
// sanitizers).  Plain C++: no HIP, and nothing here knows where a region's arrays live.
//
// Ops:  MultiPlanned plan(int i, int lane)   plans region i on a lane: its class and kind, or an error code
//       void hold()                          keeps the plan just made (one at a time) for a later stage(.., true)
//       int stage(int i, int lane, bool held)  stages region i there from the plan just made on that lane, or the held one
//       int run(const int* members, int m)   runs the staged regions members[0 .. m) as one set, to completion
//       void take(int i, int j)              region i was member j of the set that just ran: its results
//       void fail(int i, int rc)             region i has failed with rc (the message is the last error's)
// Region: bool alone (the caller runs it through the single-call path), int lane (the lane that holds its raw sums after
// the call, or -1); false and -1 on entry.  owner[kMultiMax], all -1 on entry: the region of each lane.
// On return every region is in exactly one state: member of one set that ran, alone, or failed (Ops::fail was told); and
// R[i].lane == l exactly when owner[l] == i, which only a region of a set that ran can have.
#pragma once
#include <vector>

#include "pairhmm_multi_sets.h"

namespace gklhip {

enum MultiClass { kMultiNone = 0, kMultiSmall, kMultiMid };   // no set for the region / a small one / a mid-size one
struct MultiPlanned {
  int rc;            // not 0: the region could not be planned (cls is kMultiNone)
  MultiClass cls;    // kMultiNone with rc 0: it does not qualify and runs alone
  uint8_t kind;      // of a region that qualifies: multi_cut_sets cuts by it
  bool use_double;   // a double-precision context's region
};

template <class Region, class Ops>
void multi_call_drive(Region* R, int n, int32_t* owner, Ops& ops) {
  auto release = [&](int i) { if (R[i].lane >= 0) owner[R[i].lane] = -1; R[i].lane = -1; };
  auto plan = [&](int i, int lane) {
    const MultiPlanned p = ops.plan(i, lane);
    if (p.rc) ops.fail(i, p.rc);
    else if (p.cls == kMultiNone) R[i].alone = true;
    return p;
  };
  // A staging failure is the region's own.  The lane's earlier region (of a set that has run) loses its raw sums now.
  auto stage = [&](int i, int lane, bool held) {
    if (owner[lane] >= 0) release(owner[lane]);
    if (const int rc = ops.stage(i, lane, held)) { ops.fail(i, rc); return false; }
    owner[lane] = i; R[i].lane = lane;
    return true;
  };
  auto run_alone = [&](int i) { release(i); R[i].alone = true; };   // staged or not, it finds no set
  // Up to kMultiMax regions have a lane each (region i: lane i) and are staged as they are planned; a longer list is
  // planned on lane 0 only to be classified -- the cuts need the classes of the whole list -- and each set's members are
  // planned again and staged on lanes 0 .. m - 1 when the set's turn comes.
  const bool stage_first = n <= kMultiMax;
  std::vector<uint8_t> small((size_t)n), mid((size_t)n), kind((size_t)n);
  // A double-precision context's first mid-size region is held back, planned, until a second one shows up: one alone is no
  // set, and a call with ONE such region costs what it did before these regions shared (its plan here, then the single-call
  // path) -- staged and dropped it measured 0.01 - 0.03 ms more (400 x 40: 0.39 -> 0.41 ms).
  int held = -1;
  bool any_mid = false;
  for (int i = 0; i < n; i++) {
    const MultiPlanned p = plan(i, stage_first ? i : 0);
    MultiClass cls = p.cls;
    kind[(size_t)i] = p.kind;
    if (stage_first && cls != kMultiNone) {
      if (cls == kMultiMid && p.use_double && !any_mid) {
        held = i; ops.hold();
      } else {
        if (cls == kMultiMid && held >= 0) {
          if (!stage(held, held, true)) mid[(size_t)held] = 0;
          held = -1;
        }
        if (!stage(i, i, false)) cls = kMultiNone;
      }
      any_mid = any_mid || cls == kMultiMid;
    }
    small[(size_t)i] = cls == kMultiSmall;
    mid[(size_t)i] = cls == kMultiMid;
  }
  std::vector<int32_t> set_of((size_t)n), mid_set_of((size_t)n);
  const int n_small_sets = multi_cut_sets(small.data(), kind.data(), n, set_of.data());
  const int n_mid_sets = multi_cut_mid_sets(mid.data(), n, mid_set_of.data());
  for (int i = 0; i < n; i++)
    if (mid[(size_t)i] && mid_set_of[(size_t)i] < 0) run_alone(i);   // (a held region among them: never staged)
  // the small regions' sets, then the mid-size regions' (a set is of one kind)
  for (int pass = 0; pass < 2; pass++) {
    const std::vector<int32_t>& of = pass == 0 ? set_of : mid_set_of;
    const int n_sets = pass == 0 ? n_small_sets : n_mid_sets;
    const MultiClass want = pass == 0 ? kMultiSmall : kMultiMid;
    for (int s = 0, i = 0; s < n_sets; s++) {
      int members[kMultiMax], m = 0;
      for (; i < n && of[(size_t)i] <= s; i++) {
        if (of[(size_t)i] != s) continue;
        if (!stage_first) {
          const MultiPlanned p = plan(i, m);   // planned under another load it may have changed its mind:
          if (p.cls == kMultiNone) continue;   // ... it no longer qualifies (or failed): alone after all
          if (p.cls != want || p.kind != kind[(size_t)i]) { run_alone(i); continue; }   // ... or as another class or kind, too late for that cut
          if (!stage(i, m, false)) continue;
        }
        members[m++] = i;
      }
      if (m == 0) continue;
      if (pass == 1 && m == 1) { run_alone(members[0]); continue; }   // (its company fell away: one mid-size region is no set)
      const int rc = ops.run(members, m);
      for (int j = 0; j < m; j++) {
        if (rc == 0) { ops.take(members[j], j); continue; }
        ops.fail(members[j], rc);   // a failed set fails every member, and nothing of theirs is kept
        release(members[j]);
      }
    }
  }
}

}  // namespace gklhip
