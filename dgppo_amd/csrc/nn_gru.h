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

// GRU gate non-linearities on the hardware transcendental units: exp through v_exp_f32 (scaled by log2 e), the quotient
// through v_rcp_f32; absolute error ~1e-7 on outputs in [-1, 1], far inside the 1e-5 parity tolerance, at ~1/4 of the
// VALU instructions of expf / tanhf / IEEE division (the gate math was ~70 instructions per element).
__device__ inline float gate_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ inline float gate_tanh(float x) { return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)), -1.0f); }

// Forward of one GRU element from its gate inputs g = gi (x Wi + bi, already rounded to fp32) and the hidden products
// a = h Wh summed from zero: the arithmetic of gru_fwd_kernel (nn_elem.hip), which the one-step kernel of nn_fused.hip that
// forms gi itself repeats so that hs and gates keep their bits.  Contraction mode: off, with the two fused multiply-adds
// written out.  They are the ones the compiler chose for gru_fwd_kernel while it was left to contract freely: n's argument in
// one rounding, and h' = (1 - z) n + z h with ONE of the two products rounded first — (1 - z) n in the 32-sequence-tile
// instance, z h in the 16-sequence-tile instance.  Both stay as they were: big_tiles says which instance the launch rule
// (gru_fwd_big_tiles) picks for the row count, and the one-step kernel follows the same rule.  (Left free, the same
// expressions came out of the one-step kernel as two packed products and an add: a third set of bits.)
struct GruGateFwd {
  float r, z, n, hn, h;     // the saved gates r | z | n | hn_lin and h'
};

__device__ __forceinline__ GruGateFwd gru_gate_fwd(float g_r, float g_z, float g_n, float a_r, float a_z, float a_n, float bn,
                                                   float hp, bool big_tiles) {
#pragma clang fp contract(off)
  GruGateFwd o;
  o.r = gate_sigmoid(g_r + a_r);
  o.z = gate_sigmoid(g_z + a_z);
  o.hn = a_n + bn;
  o.n = gate_tanh(__fmaf_rn(o.hn, o.r, g_n));
  const float zc = 1.0f - o.z;
  o.h = big_tiles ? __fmaf_rn(hp, o.z, zc * o.n) : __fmaf_rn(zc, o.n, o.z * hp);
  return o;
}

// 32-sequence tiles when there are enough of them to fill the device, otherwise 16 (half the MFMA chain per step)
// This rule is part of the numerical contract, not only a launch heuristic: it decides the rounding of h' (above) in
// gru_fwd_kernel and in gi_gru1_head_fwd_kernel alike.  Moving the threshold moves the bits of every pass whose row count
// changes sides; tests/test_gi_gru1_head_gpu.py holds the two kernels to each other on both sides of it (16 352 / 16 353).
static inline bool gru_fwd_big_tiles(int n_seq) { return (n_seq + 31) / 32 >= 512; }

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

// The same address in two steps, for a kernel that requests ids[e] a tile before it needs the row: the env slot e of
// sequence s and the offset of its cell inside the env's record, then the row from the env the id named.
struct GruH0Cell {
  unsigned e;
  long off;
};

__device__ __forceinline__ GruH0Cell gru_h0_map_cell(const GruH0Map& m, int s) {
  const unsigned c = gru_div((unsigned)s, m.n_inner), ag = (unsigned)s - c * (unsigned)m.n_inner.d;
  const unsigned e = gru_div(c, m.n_time), t = c - e * (unsigned)m.n_time.d;
  return GruH0Cell{e, (long)t * m.time_stride + (long)ag * 64};
}

__device__ __forceinline__ const float* gru_h0_map_cell_row(const float* base, const GruH0Map& m, const GruH0Cell& cell, long env) {
  return base + env * m.env_stride + cell.off;
}

__device__ __forceinline__ const float* gru_h0_map_row(const float* base, const GruH0Map& m, int s) {
  const unsigned c = gru_div((unsigned)s, m.n_inner), ag = (unsigned)s - c * (unsigned)m.n_inner.d;
  const unsigned e = gru_div(c, m.n_time), t = c - e * (unsigned)m.n_time.d;
  const long env = m.ids ? (long)m.ids[e] : (long)e;
  return base + env * m.env_stride + (long)t * m.time_stride + (long)ag * 64;
}
