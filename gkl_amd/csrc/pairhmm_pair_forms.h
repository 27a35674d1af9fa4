// The one-pair-per-wavefront kernels (pairhmm_fwd_kernel.h: "One pair per wavefront"; their *_multi_kernel forms in
// pairhmm_aux_kernels.h): how many rows per lane a read needs, and which kernel instantiation a call -- or a set of calls
// with that widest read -- launches.  A new tier or family is an entry HERE (kPairTiers / pair_form), in the Forms list of
// the family's launcher (pairhmm_device_pass.h) and, for a tier, an arm of pair_recompute_by_rows.
// Plain C++ (tests/native/pairhmm_pair_forms_check.cpp compiles it for the host alone, under the sanitizers).
#pragma once
#include <type_traits>

namespace gklhip {

// ---- tiers: a read of R bases has R + 1 rows; alone in a wavefront of 64 lanes it takes ceil((R + 1) / rows) of them ----
constexpr int kPairLanes = 64;
constexpr int kPairTiers[] = {2, 4, 6, 8};   // rows per lane, narrowest first
// kRplPair8: the fourth tier, reads of 384 to 511 bases (small_read_limit 511) -- what one wavefront holds at 8 rows per
// lane in both precisions (fp32: pair_fp32_alone<8>, fp64: the f64r8 programs of the wide long-read kernel).
constexpr int kRplPair8 = 8;
constexpr int pair_tier_len_max(int rows) { return kPairLanes * rows - 1; }   // the longest read of a tier: 127, 255, 383, 511
// The tier of a read (of a call: its longest read).  A longer read never reaches these kernels (small_read_len_max); it is
// given the widest tier, which nothing then uses.
constexpr int pair_rows_for(int read_len) {
  for (int rows : kPairTiers)
    if (read_len <= pair_tier_len_max(rows)) return rows;
  return kRplPair8;
}

// ---- families and their launch forms ----
// kPolicy: the policy on the fp32 sums + fp64 recomputation in one launch; kRecompute: the second launch of the two-step
// policy; kFused: fp32 recurrence + policy + recomputation; kF64: every pair in fp64 (double-precision contexts).
enum class PairFamily { kPolicy, kRecompute, kFused, kF64 };
// The MAXR template argument to launch for a call of `widest_rows`, or (is_set) a set whose widest call has them.  Inside
// the kernel a pair takes the variant its own read needs, so a wider form is never wrong, only slower.
constexpr int pair_form(PairFamily family, bool is_set, int widest_rows) {
  // the fused and all-fp64 kernels have no 2-row form (their 4-row one already runs four wavefronts per SIMD)
  if ((family == PairFamily::kFused || family == PairFamily::kF64) && widest_rows < 4) return 4;
  // the policy kernel of a set has the 6- and the 8-row form only
  if (family == PairFamily::kPolicy && is_set && widest_rows < 6) return 6;
  return widest_rows;
}
// The speculating form of the fused family (pairhmm_pair_spec_kernel): 6 rows (kRplF64), and none for a call of the fourth
// tier -- 0: the call does not speculate.
constexpr int pair_spec_form(int rows) { return rows < kRplPair8 ? 6 : 0; }

// ---- occupancy (amdgpu_waves_per_eu) of a form.  Fused, all-fp64, speculating: four wavefronts per SIMD up to 4 rows per
// lane, three at 6, two at 8; policy, recompute: three, two at 8 ----
constexpr int pair_waves_per_eu(int maxr) { return maxr <= 4 ? 4 : maxr <= 6 ? 3 : 2; }
constexpr int pair_policy_waves_per_eu(int maxr) { return maxr <= 6 ? 3 : 2; }

// The run-time (form, fma) as compile-time constants: f(std::integral_constant<int, MAXR>{}, std::bool_constant<FMA>{}),
// once, for the member of Forms... that `form` names.  Forms... is the family's own list, so only its kernels are
// instantiated.  false: `form` is not in the list and f was not called.
template <int... Forms, typename F>
bool dispatch_pair_form(int form, bool fma, F&& f) {
  auto call = [&](auto maxr) { fma ? f(maxr, std::true_type{}) : f(maxr, std::false_type{}); return true; };
  return ((form == Forms && call(std::integral_constant<int, Forms>{})) || ...);
}

}  // namespace gklhip
