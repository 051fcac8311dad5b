// LayerNorm statistics shared by nn_elem.hip and nn_fused.hip (device code only: uses HIP intrinsics).
#pragma once
#include "common.h"

// flax LayerNorm fast variance, max(E[x^2] - E[x]^2, 0), with the reference's non-finite behaviour.  The difference is one fma (what
// the compiler's contraction has always made of it: finite rows keep their bits), but an fma's exact product never overflows: where
// E[x]^2 overflows on its own (|E[x]| > 1.8e19) the reference's inf - inf = NaN is formed from the rounded square.  A NaN stays NaN.
__device__ inline float ln_fast_var(float mean, float mean2) {
  const float sq = __fmul_rn(mean, mean);
  return relu_nan(sq == INFINITY ? mean2 - sq : fmaf(-mean, mean, mean2));
}
