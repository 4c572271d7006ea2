// Launch arguments of the resampling kernels (resample.hip; ramp_resample_params in ramp_hip.h) and the host check of a group table.
#pragma once
#include "core.h"
#include <cmath>

namespace ramp {

// what a group table must satisfy: n_groups >= 1, [0] = 0, strictly increasing, [n_groups] = B.  Host only; 0 = well formed, otherwise
// the number of the rule it breaks (1 null / no group, 2 first entry, 3 not strictly increasing, 4 last entry)
inline int resample_group_table_fault(const int32_t* group_first, int n_groups, int B) {
  if (!group_first || n_groups < 1) return 1;
  if (group_first[0] != 0) return 2;
  for (int g = 0; g < n_groups; ++g)
    if (group_first[g + 1] <= group_first[g]) return 3;
  if (group_first[n_groups] != B) return 4;
  return 0;
}
inline bool resample_ess_frac_ok(double f) { return std::isfinite(f) && f >= 0.0 && f <= 2.0; }

// logw[b] += -lambda (c_b - c_prev[b]), c_prev[b] = c_b with c_b = w_obs terms[b][0] + w_smooth terms[b][1] + w_acc terms[b][2], all fp64,
// every product and sum rounded as written; a non-finite logw becomes -inf.  cost_out (B) receives c_b (may be null)
struct ResampleWeightArgs {
  const double* terms = nullptr;      // (B, 3) = launch_guide_cost's output
  double* logw = nullptr; double* c_prev = nullptr; double* cost_out = nullptr;
  int B = 0;
  double w_obs = 0, w_smooth = 0, w_acc = 0, lambda = 0;
};
int launch_resample_weights(const ResampleWeightArgs& a, hipStream_t s);

// one block per group: normalised weights, ESS, the gate, the inclusive prefix sums (into cum), the ancestors; where a group resamples,
// c_prev is permuted (through tmp) and its logw reset.  A group that does not resample gets identity ancestors and keeps logw / c_prev
struct ResampleGroupsArgs {
  double* logw = nullptr;             // (B)
  double* c_prev = nullptr;           // (B) or null
  const int* group_first = nullptr;   // device (n_groups + 1)
  const float* u = nullptr;           // device (n_groups), in (0, 1)
  double ess_frac = 0;
  double* cum = nullptr;              // scratch (B)
  double* tmp = nullptr;              // scratch (B); read only where c_prev != null
  int* ancestor = nullptr;            // (B): indices within the batch
  double* ess_out = nullptr;          // (n_groups) or null
  int B = 0, n_groups = 0;
};
int launch_resample_groups(const ResampleGroupsArgs& a, hipStream_t s);

// tmp[i] = x[ancestor[i]] for the whole row of HS floats (HS % 4 == 0, 16-byte vectors); an ancestor outside [0, B) reads row i itself
int launch_resample_gather(const float* x, const int* ancestor, float* tmp, int B, int HS, hipStream_t s);

}  // namespace ramp
