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

// Division of a non-negative int by a divisor fixed per launch, as a multiply-high and two shifts (Granlund & Montgomery,
// "Division by invariant integers using multiplication", the round-up form): with l = ceil(log2 d) and
// mul = floor(2^32 (2^l - d) / d) + 1,  n / d = (t + ((n - t) >> 1)) >> (l - 1),  t = mulhi(mul, n),  exact for every 32-bit n.
// The map below divides twice per row address; the hardware has no integer divide, and the compiler's expansion of `/` by a
// run-time divisor is some forty instructions.
struct GruFastDiv {
  unsigned mul;
  int sh, d;
};

static inline GruFastDiv gru_fast_div(int d) {                // host side, d >= 1
  GruFastDiv f{0u, 0, d};
  if (d > 1) {
    int l = 0;
    while ((1ull << l) < (unsigned long long)d) ++l;
    f.mul = (unsigned)(((1ull << 32) * ((1ull << l) - (unsigned long long)d)) / (unsigned long long)d + 1ull);
    f.sh = l - 1;
  }
  return f;
}

__host__ __device__ __forceinline__ unsigned gru_div(unsigned n, const GruFastDiv& f) {
  if (f.d == 1) return n;
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned t = __umulhi(f.mul, n);
#else
  const unsigned t = (unsigned)(((unsigned long long)f.mul * n) >> 32);
#endif
  return (t + ((n - t) >> 1)) >> f.sh;
}

// Carry map of a one-step (T = 1) pass that reads its h0 rows where a record left them.  Sequence s is cell c = s / n_inner,
// agent a = s - c * n_inner; the cell is (e, t) = (c / n_time, c % n_time); its 64 floats start at
//   base + env * env_stride + t * time_stride + a * 64,   env = ids ? ids[e] : e     (strides in floats, multiples of 4).
// n_inner.d == 0: no map (the caller's dense / blocked addressing applies).
struct GruH0Map {
  const int* ids;
  long env_stride, time_stride;
  GruFastDiv n_inner, n_time;
};

static inline GruH0Map gru_h0_map(const int* ids, long env_stride, long time_stride, int n_inner, int n_time) {
  return GruH0Map{ids, env_stride, time_stride, gru_fast_div(n_inner), gru_fast_div(n_time)};
}

__device__ __forceinline__ const float* gru_h0_map_row(const float* base, const GruH0Map& m, int s) {
  const unsigned c = gru_div((unsigned)s, m.n_inner), ag = (unsigned)s - c * (unsigned)m.n_inner.d;
  const unsigned e = gru_div(c, m.n_time), t = c - e * (unsigned)m.n_time.d;
  const long env = m.ids ? (long)m.ids[e] : (long)e;
  return base + env * m.env_stride + (long)t * m.time_stride + (long)ag * 64;
}
