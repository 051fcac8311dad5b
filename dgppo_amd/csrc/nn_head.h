// tanh-Normal head (policy.py:62-74, distribution.py:10-46): the per-dimension arithmetic shared by policy_head_kernel
// (nn_elem.hip) and the act-step form of the wave-per-env kernel (env_wave.hip), so that both sample from ONE text.
//
// The two translation units are built with different contraction settings (env_wave.hip: -ffp-contract=off).  Every
// function here therefore states its own: products may contract into the sum that reads them, as in nn_elem.hip's
// build, whichever unit includes the header.  log and exp are the builtins for the same reason: the compiler expands them in
// place with the flags of the call, and a call through the math header's logf() / expf() wrappers would carry the
// including unit's flags, not this header's (log1pf, erfcf, tanhf and atanhf are library code with flags of their own).
#pragma once
#include "common.h"

#define STD_INIT_INV (-0.43275212956718856f)  // log(exp(0.5) - 1)
#define STD_MIN 1e-5f
#define THRESH 0.999f
#define INV_THRESH 3.8002011672502f           // atanh(0.999)
#define LOG_EPS (-6.907755278982137f)         // log(1 - 0.999)
#define HALF_LOG_2PI 0.9189385332046727f
#define LOG2_F 0.6931471805599453f

__device__ inline float softplusf_(float x) {
#pragma clang fp contract(fast)      // (also for the calls: expf / logf are expanded in place and inherit the caller's flags)
  return (x > 20.0f) ? x : log1pf(__builtin_expf(x));
}
// log Phi(z): erfc for the bulk, asymptotic series for the far left tail (tfp special_math.log_ndtr).  The series
// Phi(z) ~ phi(z) / (-z) * (1 - 1/z^2 + 3/z^4 - 15/z^6) is cut after its fourth term, so its relative error is the fifth,
// 105 / z^8: 1.05e-6 at z = -10 but 2.7e-4 at z = -5.  It therefore starts at z <= -10; down to there the erfc form is
// still made of normal fp32 numbers (erfcf(10 / sqrt 2) = 1.5e-23, expf(-50) = 1.9e-22).
#define NDTR_SERIES_BELOW (-10.0f)
__device__ inline float ndtr_tail_series(float z2) {
#pragma clang fp contract(fast)
  return 1.0f - 1.0f / z2 + 3.0f / (z2 * z2) - 15.0f / (z2 * z2 * z2);
}
__device__ inline float log_ndtrf_(float z) {
#pragma clang fp contract(fast)
  if (z > NDTR_SERIES_BELOW) return __builtin_logf(0.5f * erfcf(-z * 0.70710678118654752f));
  const float z2 = z * z;
  return -0.5f * z2 - __builtin_logf(-z) - HALF_LOG_2PI + __builtin_logf(ndtr_tail_series(z2));
}
// d/dz log Phi(z) = phi(z) / Phi(z); in the tail -z / series, with the terms of the value
__device__ inline float dlog_ndtrf_(float z) {
#pragma clang fp contract(fast)
  if (z > NDTR_SERIES_BELOW) return 0.3989422804014327f * __builtin_expf(-0.5f * z * z) / (0.5f * erfcf(-z * 0.70710678118654752f));
  return -z / ndtr_tail_series(z * z);
}
__device__ inline float tanh_fldj(float x) {
#pragma clang fp contract(fast)
  return 2.0f * (LOG2_F - x - softplusf_(-2.0f * x));
}

__device__ inline float tn_log_prob_dim(float act, float mu, float sd) {
#pragma clang fp contract(fast)
  const float ac = fminf(fmaxf(act, -THRESH), THRESH);
  if (ac <= -THRESH) return log_ndtrf_((-INV_THRESH - mu) / sd) - LOG_EPS;
  if (ac >= THRESH) return log_ndtrf_(-(INV_THRESH - mu) / sd) - LOG_EPS;
  const float x = atanhf(ac);
  const float z = (x - mu) / sd;
  return -0.5f * z * z - __builtin_logf(sd) - HALF_LOG_2PI - tanh_fldj(x);
}

// one action dimension of a row ms = [mean0, mean1, std_trans0, std_trans1]
__device__ inline float tn_std(float std_trans) {
#pragma clang fp contract(fast)
  return softplusf_(std_trans + STD_INIT_INV) + STD_MIN;
}
// PPOPolicy.get_action: tanh(mean)
__device__ inline float tn_mode_dim(float mu) {
#pragma clang fp contract(fast)
  return tanhf(mu);
}
// sample_action: tanh(mean + std * eps); log_prob recomputes atanh(clip(a)) like the reference (tn_log_prob_dim)
__device__ inline float tn_sample_dim(float mu, float sd, float eps) {
#pragma clang fp contract(fast)
  return tanhf(mu + sd * eps);
}
