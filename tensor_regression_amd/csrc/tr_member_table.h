// tr_member_table.h — what the host side of the many-model fit routes shares: the Adam step's scalars
// (also the plain update step's, tr_api.hip), the per-iteration rows and scalar fields of a member's table
// entry and the common argument checks.  No HIP dependency: tests/cpp compiles it with the host compiler alone.
#pragma once

#include <stdint.h>

#include <cmath>
#include <map>
#include <tuple>

#include "../../include/tensor_regression_hip.h"

namespace tr {

// torch/optim/adam.py (non-capturable): the step's scalars in python-float (double) arithmetic.  The
// fp32 entry points round each to float; the fp64 one passes them to the fp64 ops unrounded.
struct AdamScalars {
  double bc1, bc2_sqrt, one_minus_b1, one_minus_b2;
};
inline AdamScalars adam_scalars(double beta1, double beta2, int64_t step) {
  const double st = (double)step;
  const double bc2 = 1.0 - std::pow(beta2, st);
  return {1.0 - std::pow(beta1, st), std::pow(bc2, 0.5), 1.0 - beta1, 1.0 - beta2};
}

// adam_scalars remembered per (beta1, beta2, step): the members of one table mostly share their betas
// and all share the step range, so a table costs 2 x 64 pow calls per distinct beta pair, not per member.
struct AdamMemo {
  std::map<std::tuple<double, double, int64_t>, AdamScalars> seen;
  int64_t computed = 0;  // adam_scalars calls made (the stand-alone checks count them)
  const AdamScalars& at(double beta1, double beta2, int64_t step) {
    const auto key = std::make_tuple(beta1, beta2, step);
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, adam_scalars(beta1, beta2, step)).first;
      ++computed;
    }
    return it->second;
  }
};

// One row per iteration of a launch (Adam step counts step, step + 1, ...): bc2_sqrt[k] = sqrt(1 - b2^t)
// and per learning rate step_size[f][k] = lr[f] / (1 - b1^t), divided in double, rounded once.  `memo` may be NULL.
template <int MAX_ITERS>
inline void fill_adam_rows(AdamMemo* memo, double beta1, double beta2, int64_t step, int n_iters, const double* lr,
                           int n_lr, float (*step_size)[MAX_ITERS], float* bc2_sqrt) {
  for (int k = 0; k < n_iters; ++k) {
    const AdamScalars as = memo != nullptr ? memo->at(beta1, beta2, step + k) : adam_scalars(beta1, beta2, step + k);
    for (int f = 0; f < n_lr; ++f) step_size[f][k] = (float)(lr[f] / as.bc1);
    bc2_sqrt[k] = (float)as.bc2_sqrt;
  }
}

// The scalar Adam fields of a table entry (ResArgs and LmMember name them alike).
template <class Entry>
inline void fill_adam_scalars(Entry* t, double beta1, double beta2, double eps, double weight_decay, int amsgrad) {
  t->one_minus_b1 = (float)(1.0 - beta1);
  t->beta2 = (float)beta2;
  t->one_minus_b2 = (float)(1.0 - beta2);
  t->eps = (float)eps;
  t->weight_decay = (float)weight_decay;
  t->amsgrad = amsgrad ? 1 : 0;
}

// The checks on the fields that tr_resident_member and tr_linear_member name alike; 0 or TR_E_ARG and `why`.
template <class Member>
inline int check_adam_member(const Member& m, int max_iters, const char** why) {
  if (m.exp_avg == nullptr || m.exp_avg_sq == nullptr || m.loss_hist == nullptr || m.stop_flag == nullptr) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (m.amsgrad && m.max_exp_avg_sq == nullptr) {
    *why = "amsgrad needs max_exp_avg_sq";
    return TR_E_ARG;
  }
  if (m.n_iters < 0 || m.n_iters > max_iters) {
    *why = "n_iters outside the call's range";
    return TR_E_ARG;
  }
  if (m.step < 1) {
    *why = "step must be >= 1";
    return TR_E_ARG;
  }
  if (m.iter < 0 || m.hist_base < 0) {
    *why = "iter and hist_base must be >= 0";
    return TR_E_ARG;
  }
  return 0;
}

}  // namespace tr
