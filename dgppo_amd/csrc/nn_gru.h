// Gate gradients of one GRU element (flax GRUCell: h' = (1 - z) n + z h, n = tanh(gi_n + r hn)), shared by the BPTT scan
// (nn_elem.hip, phase A) and the one-step form inside the weight-gradient pass (nn_dense.hip), so that the two write the
// same bits.  d = gradient arriving at h' (carried dh + upstream dhs); at T = 1 the carried dh is the scan's zero, and the
// caller passes gru_zero_carry(dhs), which is what the scan adds: -0.0 becomes +0.0 there too, and a NaN stays a NaN.
// The rounding of every operation is written out (contraction off, the one fused multiply-add explicit: it is the one the
// scan has always had), so the bits do not depend on what a translation unit's optimiser would choose to contract.
#pragma once
#include <hip/hip_runtime.h>

struct GruGateGrad {
  float dar, daz, dan, dhn;   // d pre-activation of r, z, n (= dgi's three blocks) and d hn (= dgh's third block)
};

__device__ __forceinline__ GruGateGrad gru_gate_grad(float d, float hp, float rg, float zg, float ng, float hn) {
#pragma clang fp contract(off)
  GruGateGrad o;
  const float dz = d * (hp - ng);
  const float dn = d * (1.0f - zg);
  o.dan = dn * __fmaf_rn(-ng, ng, 1.0f);        // 1 - n^2 in one rounding
  o.dhn = o.dan * rg;
  o.dar = o.dan * hn * rg * (1.0f - rg);
  o.daz = dz * zg * (1.0f - zg);
  return o;
}

// 0.0f + du, as an add that is really executed (IEEE: -0.0 -> +0.0)
__device__ __forceinline__ float gru_zero_carry(float du) { return __fadd_rn(0.0f, du); }
