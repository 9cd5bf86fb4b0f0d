// tr_adam.h — what every fp32 update kernel shares (k_update, k_update_conv, k_mnl_resident): the
// _single_tensor_adam sequence of torch/optim/adam.py (torch 2.10, non-capturable branch), the
// factor norms of the L2 term and the stop-flag prologue.  One place, because every numerical
// guarantee of the project is a bitwise statement about this step.
//
// The Adam helpers hold arithmetic only and are compiled without contraction (the pragma travels
// with the inlined instructions).  The caller keeps vm = fmaxf(vm, vv), every store and the order of
// the stores, its loops, and the wave butterfly (wv_allreduce) between norm_add and
// norm_finish: k_update sits at the SGPR ceiling (106, spilling to lanes), and with these pieces at
// the call site its gfx950 code is instruction for instruction what it was when the step was
// written out in the kernel.  (k64_update, tr_fp64.hip, is compiled with contraction on and keeps
// its own copy.)
#pragma once

#include "tr_common.h"

namespace tr {

// grad.add(param, alpha=wd); exp_avg.lerp_(grad, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
__device__ __forceinline__ void adam_moments(float p, float& g, float& mm, float& vv, float weight_decay,
                                             float one_minus_b1, float beta2, float one_minus_b2) {
#pragma clang fp contract(off)
  g = weight_decay != 0.0f ? fmaf(p, weight_decay, g) : g;
  mm = fmaf(one_minus_b1, g - mm, mm);
  vv = vv * beta2;
  vv = vv + one_minus_b2 * g * g;
}

// denom = sqrt(second) / bc2_sqrt + eps; param.addcdiv_(m, denom, -step_size).  `second` is
// exp_avg_sq, or max_exp_avg_sq under amsgrad.
__device__ __forceinline__ float adam_param(float p, float mm, float second, float bc2_sqrt, float eps,
                                            float step_size) {
#pragma clang fp contract(off)
  const float denom = sqrtf(second) / bc2_sqrt + eps;
  return p + (-step_size) * (mm / denom);
}

// ||A_f||_F^2 of every factor (raw parameters), one element of this thread's share: a thread sums the
// elements k = t (mod 1024) in increasing k, the factor's accumulator selected without a branch.
__device__ __forceinline__ void norm_add(const FactorSet& fs, int nf, int64_t k, float a, float (&accn)[TR_MAXF]) {
  const int f = factor_of(fs, nf, k);
#pragma unroll
  for (int g = 0; g < TR_MAXF; ++g) accn[g] = g == f ? fmaf(a, a, accn[g]) : accn[g];
}

// After the wave butterfly of every accumulator (wv_allreduce, lane 0 to wsum[f * 16 + wave]) and
// a barrier, thread f < nf: the wave-order sum of the NWV wave sums, ||A_f|| and the L2 coefficient,
// d/dA lambda ||A|| = (lambda / (2 ||A||)) * (2 A); a barrier follows.
template <int NWV>
__device__ __forceinline__ void norm_finish(const float* wsum, int f, float lambda, float* norms, float* coef) {
  float tot = 0.f;
  for (int w = 0; w < NWV; ++w) tot += wsum[f * 16 + w];
  norms[f] = sqrtf(tot);
  coef[f] = lambda / (2.0f * norms[f]);
}

// The stop flag and the gradient arena's status slot (grad[np + 1], summed over shards by the
// all-reduce) are loaded first and branched on after the norms.
struct StopState {
  int32_t stop0;
  float status;
  bool checked;
};
__device__ __forceinline__ StopState stop_load(const int32_t* stop, bool fit, const float* grad, int64_t np) {
  StopState s;
  s.checked = fit && stop != nullptr;
  s.stop0 = stop != nullptr ? *stop : 0;
  s.status = s.checked ? grad[np + 1] : 0.f;
  return s;
}
// True when the kernel returns before the step: the fit has stopped, or the pass failed (then the
// parameters and the Adam state stay those of the last good iteration).
__device__ __forceinline__ bool stop_taken(const StopState& s, int32_t* stop, int64_t iter, int t) {
  if (s.stop0 != 0) return true;
  if (s.checked && s.status != 0.0f) {
    if (t == 0) *stop = TR_STOP_DEVICE_ERROR - (int32_t)iter;
    return true;
  }
  return false;
}

}  // namespace tr
