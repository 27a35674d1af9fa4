// Stand-alone check of gkl_amd/csrc/pairhmm_pair_forms.h (tests/test_pairhmm_pair_forms_cpu.py builds it with
// -fsanitize=address,undefined and expects exit 0): the row tiers of the one-pair-per-wavefront kernels, the kernel form a
// call or a set launches, the occupancy rules and the dispatcher.
//   * the table of forms, written out below: 4 families x single / set x 4 tiers;
//   * every read length 1 .. 511: its tier holds the read in 64 lanes, the next narrower one does not, and the tier edges
//     are 127 | 128, 255 | 256, 383 | 384 and 511;
//   * every family and every multiset of member tiers (what a set of calls can hold): the set's form is the form of its
//     widest member and no narrower than any member's tier -- a form chosen too narrow would run off a prior table;
//   * every form returned is in the family's own list of instantiations (the lists of pairhmm_device_pass.h's launchers,
//     repeated here), so the dispatcher's fall-through is not reached; the dispatcher calls its function exactly once
//     with the constants asked for, and not at all for a form that is not in the list;
//   * a call of 8 rows never speculates; the two occupancy rules.
#include <cstdio>
#include <type_traits>

#include "../../gkl_amd/csrc/pairhmm_pair_forms.h"

using namespace gklhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "%s failed: ", #cond);         \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      g_failed++;                                         \
    }                                                     \
  } while (0)

constexpr int kTiers[4] = {2, 4, 6, 8};
constexpr PairFamily kFamilies[4] = {PairFamily::kPolicy, PairFamily::kRecompute, PairFamily::kFused, PairFamily::kF64};
const char* const kFamilyName[4] = {"policy", "recompute", "fused", "all-fp64"};
// [family][single, set][tier]: the MAXR template argument launched
constexpr int kTable[4][2][4] = {
    {{2, 4, 6, 8}, {6, 6, 6, 8}},   // policy
    {{2, 4, 6, 8}, {2, 4, 6, 8}},   // recompute
    {{4, 4, 6, 8}, {4, 4, 6, 8}},   // fused
    {{4, 4, 6, 8}, {4, 4, 6, 8}},   // all-fp64
};
// the families' lists of instantiations: [family][single, set], 0-terminated
constexpr int kForms[4][2][5] = {
    {{2, 4, 6, 8, 0}, {6, 8, 0}},
    {{2, 4, 6, 8, 0}, {2, 4, 6, 8, 0}},
    {{4, 6, 8, 0}, {4, 6, 8, 0}},
    {{4, 6, 8, 0}, {4, 6, 8, 0}},
};

// what the dispatcher handed to its function
struct Seen {
  int calls = 0, maxr = -1, fma = -1;
};
template <int... Forms>
Seen dispatched(int form, bool fma, bool* found) {
  Seen s;
  *found = dispatch_pair_form<Forms...>(form, fma, [&](auto maxr, auto fused_mul) {
    static_assert(std::is_same<decltype(maxr), std::integral_constant<int, decltype(maxr)::value>>::value, "an integral_constant");
    static_assert(std::is_same<decltype(fused_mul), std::bool_constant<decltype(fused_mul)::value>>::value, "a bool_constant");
    s.calls++;
    s.maxr = decltype(maxr)::value;
    s.fma = decltype(fused_mul)::value ? 1 : 0;
  });
  return s;
}
template <int... Forms>
int check_dispatch(const char* what) {
  int checked = 0;
  for (int form = -1; form <= 12; form++) {
    const bool in_list = ((form == Forms) || ...);
    for (int fma = 0; fma < 2; fma++) {
      bool found = false;
      const Seen s = dispatched<Forms...>(form, fma != 0, &found);
      CHECK(found == in_list, "%s: form %d found %d", what, form, (int)found);
      if (in_list) CHECK(s.calls == 1 && s.maxr == form && s.fma == fma, "%s: form %d fma %d -> %d calls with <%d, %d>", what, form, fma, s.calls, s.maxr, s.fma);
      else CHECK(s.calls == 0, "%s: form %d is not in the list and was called %d times", what, form, s.calls);
      checked++;
    }
  }
  return checked;
}

int main() {
  // ---- the table ----
  static_assert(pair_form(PairFamily::kPolicy, true, 2) == 6 && pair_form(PairFamily::kFused, false, 2) == 4, "usable in constant expressions");
  for (int f = 0; f < 4; f++)
    for (int set = 0; set < 2; set++)
      for (int t = 0; t < 4; t++) {
        const int form = pair_form(kFamilies[f], set != 0, kTiers[t]);
        CHECK(form == kTable[f][set][t], "%s %s rows %d: form %d, the table says %d", kFamilyName[f], set ? "set" : "single", kTiers[t], form, kTable[f][set][t]);
        bool listed = false;
        for (int i = 0; kForms[f][set][i]; i++) listed = listed || kForms[f][set][i] == form;
        CHECK(listed, "%s %s rows %d: form %d is not an instantiation of the family", kFamilyName[f], set ? "set" : "single", kTiers[t], form);
        CHECK(form >= kTiers[t], "%s %s rows %d: form %d is too narrow", kFamilyName[f], set ? "set" : "single", kTiers[t], form);
      }

  // ---- tiers ----
  CHECK(sizeof kPairTiers / sizeof kPairTiers[0] == 4, "four tiers");
  for (int t = 0; t < 4; t++) CHECK(kPairTiers[t] == kTiers[t], "tier %d is %d rows", t, kPairTiers[t]);
  CHECK(kRplPair8 == 8 && kPairLanes == 64, "the fourth tier, the wavefront");
  for (int R = 1; R <= 511; R++) {
    const int rows = pair_rows_for(R);
    CHECK(rows == 2 || rows == 4 || rows == 6 || rows == 8, "read of %d bases: %d rows", R, rows);
    if (rows <= 0) continue;
    CHECK((R + rows) / rows <= 64, "read of %d bases does not fit %d rows per lane", R, rows);
    if (rows > 2) CHECK((R + rows - 2) / (rows - 2) > 64, "read of %d bases fits %d rows per lane but got %d", R, rows - 2, rows);
    CHECK(R <= pair_tier_len_max(rows), "read of %d bases, tier of at most %d", R, pair_tier_len_max(rows));
  }
  CHECK(pair_rows_for(127) == 2 && pair_rows_for(128) == 4, "edge 127 | 128");
  CHECK(pair_rows_for(255) == 4 && pair_rows_for(256) == 6, "edge 255 | 256");
  CHECK(pair_rows_for(383) == 6 && pair_rows_for(384) == 8, "edge 383 | 384");
  CHECK(pair_rows_for(511) == 8 && pair_rows_for(1) == 2, "ends 1 and 511");
  CHECK(pair_tier_len_max(2) == 127 && pair_tier_len_max(4) == 255 && pair_tier_len_max(6) == 383 && pair_tier_len_max(8) == 511, "longest reads of the tiers");

  // ---- sets: every multiset with each tier none, once or twice among the members (80 of them; a third copy of a tier
  // changes nothing that two do not) ----
  int sets = 0;
  for (int f = 0; f < 4; f++)
    for (int code = 1; code < 81; code++) {
      const int count[4] = {code % 3, code / 3 % 3, code / 9 % 3, code / 27};
      int widest = kPairTiers[0];   // over the members, as SmallCombiner::launch_multi computes it
      for (int t = 0; t < 4; t++)
        for (int c = 0; c < count[t]; c++) widest = kTiers[t] > widest ? kTiers[t] : widest;
      const int form = pair_form(kFamilies[f], true, widest);
      int widest_member_form = 0;
      for (int t = 0; t < 4; t++)
        if (count[t]) {
          CHECK(form >= kTiers[t], "%s set %d: form %d under member tier %d", kFamilyName[f], code, form, kTiers[t]);
          widest_member_form = pair_form(kFamilies[f], true, kTiers[t]);   // (ascending: the last one is the widest member's)
        }
      CHECK(form == widest_member_form, "%s set %d: form %d, its widest member's %d", kFamilyName[f], code, form, widest_member_form);
      sets++;
    }

  // ---- the dispatcher, over the families' lists ----
  int dispatches = 0;
  dispatches += check_dispatch<2, 4, 6, 8>("policy, recompute");
  dispatches += check_dispatch<4, 6, 8>("fused, all-fp64");
  dispatches += check_dispatch<6, 8>("policy set");
  dispatches += check_dispatch<6>("speculation");

  // ---- speculation ----
  CHECK(pair_spec_form(8) == 0, "rows 8 speculates with form %d", pair_spec_form(8));
  for (int t = 0; t < 3; t++) CHECK(pair_spec_form(kTiers[t]) == 6, "rows %d speculates with form %d", kTiers[t], pair_spec_form(kTiers[t]));

  // ---- occupancy ----
  constexpr int kWavesFused[4] = {4, 4, 3, 2}, kWavesPolicy[4] = {3, 3, 3, 2};
  for (int t = 0; t < 4; t++) {
    CHECK(pair_waves_per_eu(kTiers[t]) == kWavesFused[t], "pair_waves_per_eu(%d) = %d", kTiers[t], pair_waves_per_eu(kTiers[t]));
    CHECK(pair_policy_waves_per_eu(kTiers[t]) == kWavesPolicy[t], "pair_policy_waves_per_eu(%d) = %d", kTiers[t], pair_policy_waves_per_eu(kTiers[t]));
  }

  if (g_failed) {
    std::fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok: 32 table entries, 511 read lengths, %d sets, %d dispatches\n", sets, dispatches);
  return 0;
}
