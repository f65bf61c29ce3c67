// The Adam update of one element, ONCE, for the two kernels that must agree bit for bit: adam_kernel (adam.hip) and
// step_apply_kernel (train_step.hip).  Semantics of _single_tensor_adam (adam.hip's header states them); every
// multiply-add is an explicit fmaf and the remaining multiplies and divides feed one, so nothing here can contract.
#pragma once
#include "common.h"

namespace hgs {

// p, m, v: register copies of param, exp_avg and exp_avg_sq, updated in place
__device__ __forceinline__ void adam_update(const hgs_adam_tensor& T, float g, float& p, float& m, float& v) {
  if (T.weight_decay != 0.0f) g = fmaf(T.weight_decay, p, g);
  m = fmaf(T.one_minus_beta1, g, m * T.beta1);
  v = fmaf(T.one_minus_beta2 * g, g, v * T.beta2);
  const float denom = sqrtf(v) / T.bias_correction2_sqrt + T.eps;
  p = fmaf(-T.step_size, m / denom, p);
}

}  // namespace hgs
