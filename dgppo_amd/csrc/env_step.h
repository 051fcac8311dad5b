// Shared between env_step.hip (generic + workgroup-per-env LiDAR kernels) and env_wave.hip (wave-per-env LiDAR kernel).
// Both translation units are built with -ffp-contract=off (see Makefile): every fp32 operation is one IEEE operation.
#pragma once
#include "common.h"

enum { MODE_STEP = 0, MODE_SENSE = 1, MODE_GRAPH = 2 };

struct StepArgs {
  dgppo_env_cfg cfg;
  const float* agent;
  const float* action;
  const float* goal;
  const float* obst;
  const float* hits;
  const float* ray_cos;
  const float* ray_sin;
  float* next_agent;
  float* next_hits;
  float* reward;
  float* cost;
  dgppo_graph_out g;
  int has_graph;
  int mode;
  uint32_t rcp_n, rcp_k, rcp_no, rcp_no4;   // ceil(2^32 / d) for the index divisions of lidar_step_kernel (fdiv below)
  int B;
  float thr2_comm, thr2_lidar;              // sqrt_threshold(comm_radius), sqrt_threshold(lidar_mask_radius) (wave kernel)
};

// What the act-step form of the wave kernel (env_wave.hip, dgppo_env_act_step_feats) takes beside StepArgs: the policy's
// head output it samples the action from, and where the features and layer-0 queries of state t+1 go
struct ActFeatArgs {
  const float* ms;       // [B * n, 4]: mean0, mean1, std_trans0, std_trans1
  const float* eps;      // [B * n, 2] noise (sample != 0)
  float* action;         // [B, n, 2] out: what policy_head_kernel writes in modes 0 / 1
  float* log_pi;         // [B, n] out (sample != 0)
  int sample;            // 1: tanh(mean + std eps) and log pi; 0: tanh(mean)
  float *Xa, *Xo, *efeat, *emask;   // GraphFeats layout at Fp = 8 of state t+1; Xa == NULL: not emitted
  const float *Mcat, *cvec;         // [8, 24], [24]
  float* qt0;                       // [B * n, 24] = Xa Mcat + cvec of state t+1; NULL: not emitted
  int max_blocks;                   // > 0: cap of the persistent grid (tests: several rounds at a small batch)
};
struct NoActFeat {};

// state2feat: lidar_bicycle_target.py:113-118 (identity for the double integrator)
template <int SD>
__device__ inline void state2feat(const float* s, float* f) {
  if constexpr (SD == 5) {
    f[0] = s[0];
    f[1] = s[1];
    f[2] = s[4] * s[2];
    f[3] = s[4] * s[3];
  } else {
    f[0] = s[0]; f[1] = s[1]; f[2] = s[2]; f[3] = s[3];
  }
}

// Every clip of the step kernels goes through clampf_nan (common.h: jnp.clip semantics, a NaN stays a NaN).  NaN reaches the
// costs through a NaN hit point of the pre-step graph (ray parallel to an edge), and the actions and states
// through a NaN policy output, which the reference carries through clip_action (env/base.py:84-86) and clip_state into a
// visibly NaN rollout.
// clip_action (env/base.py:84-86), shared by the three step kernels and the action sweep
__device__ inline float clip_action(float u) { return clampf_nan(u, -1.0f, 1.0f); }

// The reference formulas every step kernel shares.  Each keeps the oracle's fp32 operation order.

// agent_step_euler: lidar_bicycle_target.py:95-107, lidar_env/base.py:146-149.  u0, u1: the clipped action; y_limit bounds
// the double integrator's y (area_size except MPECorridor / MPEConnectSpread: 2 A)
template <int SD>
__device__ inline void step_state(const float* x, float u0, float u1, const dgppo_env_cfg& c, float y_limit, float* nx) {
  const float dt = c.dt, A = c.area_size;
  if constexpr (SD == 5) {
    const float theta = atan2f(x[3], x[2]);
    const float theta_next = theta + x[4] * u0 * dt * 10.0f;
    nx[0] = clampf_nan(x[0] + x[4] * cosf(theta) * dt, 0.0f, A);
    nx[1] = clampf_nan(x[1] + x[4] * sinf(theta) * dt, 0.0f, A);
    nx[2] = clampf_nan(cosf(theta_next), -1.0f, 1.0f);
    nx[3] = clampf_nan(sinf(theta_next), -1.0f, 1.0f);
    nx[SD - 1] = clampf_nan(x[SD - 1] + u1 * dt * 10.0f, -0.5f, 0.5f);
  } else {
    const float vl = c.vel_limit;
    nx[0] = clampf_nan(x[2] * dt + x[0], 0.0f, A);
    nx[1] = clampf_nan(x[3] * dt + x[1], 0.0f, y_limit);
    nx[2] = clampf_nan((u0 * 10.0f) * dt + x[2], -vl, vl);
    nx[3] = clampf_nan((u1 * 10.0f) * dt + x[3], -vl, vl);
  }
}

// get_cost (lidar_env/base.py:180-207, mpe/base.py:164-191): a margin m becomes m -/+ 0.5 before the clip, which each
// caller applies (MPE clips only from below, through clip_lo_nan: like jnp.clip(cost, a_min=-1.0), mpe/base.py:189, that
// clip keeps a NaN, where fmaxf alone would report the safest cost there is)
__device__ inline float cost_value(float m) { return (m <= 0.0f) ? m - 0.5f : m + 0.5f; }
// one-sided clampf_nan: a NaN stays a NaN, every other input gets the bits of fmaxf(v, lo)
__device__ inline float clip_lo_nan(float v, float lo) { return (v != v) ? v : fmaxf(v, lo); }

// get_reward (lidar_spread.py:35-52 and its siblings) from the three sums in index order: distances to the ng reward
// goals, goals not reached, squared action norms of the n agents
__device__ inline float reward_from_sums(float s1, float s2, float s3, int ng, int n) {
  float r = 0.0f;
  r = r - (s1 / (float)ng) * 0.01f;
  r = r - (s2 / (float)ng) * 0.001f;
  r = r - (s3 / (float)n) * 0.0001f;
  return r;
}

// one segment test of obstacle.py:97-105 taken literally: det = sign(det0) * clip(|det0|, 1e-7, 1e7), then
// v * (na / det) + (1 - v) * 1e6 with v = (both quotients in [0, 1]).  The kernels' fast paths decide validity without the
// divisions and fall back to this for det0 == 0 (x / 0 -> 0 * inf = NaN) and NaN
__device__ inline float segment_alpha_literal(float det0, float na, float nb) {
  const float sgn = (det0 > 0.0f) ? 1.0f : ((det0 < 0.0f) ? -1.0f : det0);
  const float det = sgn * fminf(fmaxf(fabsf(det0), 1e-7f), 1e7f);
  const float aq = na / det, bq = nb / det;
  const float v = ((aq <= 1.0f) && (aq >= 0.0f) && (bq <= 1.0f) && (bq >= 0.0f)) ? 1.0f : 0.0f;
  return v * aq + (1.0f - v) * 1e6f;
}

// Rectangle.inside with radius r (obstacle.py:62-72); rec = 16-float record
__device__ inline bool rect_inside(const float* rec, float px, float py, float r) {
  float rel_x = px - rec[0];
  float rel_y = py - rec[1];
  float c = rec[5], s = rec[6];
  float rel_xx = fabsf(rel_x * c + rel_y * s) - rec[2] / 2.0f;
  float rel_yy = fabsf(rel_x * s - rel_y * c) - rec[3] / 2.0f;
  bool is_in_down = (rel_xx < r) && (rel_yy < 0.0f);
  bool is_in_up = (rel_xx < 0.0f) && (rel_yy < r);
  bool is_out_corner = (rel_xx > 0.0f) && (rel_yy > 0.0f);
  bool is_in_circle = sqrtf(rel_xx * rel_xx + rel_yy * rel_yy) < r;
  return is_in_down || is_in_up || (is_out_corner && is_in_circle);
}


// ---- LiDAR ray cast of the generic kernels (env_step.hip's workgroup-per-env kernel, env_sweep.hip) -------------------------
// per-segment constants of rectangle record `rec`, corner m: P[m] and the edge vector P[m-1] - P[m]
__device__ inline void segment_consts(const float* rec, int m, float* out4) {
  const int mm = (m + 3) & 3;
  const float* P = rec + 8;
  out4[0] = P[2 * m];
  out4[1] = P[2 * m + 1];
  out4[2] = P[2 * mm] - P[2 * m];          // x4 - x3
  out4[3] = P[2 * mm + 1] - P[2 * m + 1];  // y4 - y3
}

// smallest alpha of the ray from (x1, y1) in direction (rc, rs), length sr, over the 4 * no segments of s_seg
// (float4-aligned, segment_consts layout), before the start-inside factor.
// Exactly the reference's arithmetic (obstacle.py:97-105), evaluated without the two IEEE divisions per test:
//   valid = (0 <= num_a/det <= 1) && (0 <= num_b/det <= 1)  is decided from signs and magnitudes
//     fl(q) >= 0  <=>  q >= 0   (no quotient of these operands can underflow to -0: |num| is 0 or >= ~1e-22, |det| <= 1e7)
//     fl(q) <= 1  <=>  q <= 1   (num > det > 0 implies q >= 1 + 2^-24 + eps, which rounds above 1)
//   and only a valid segment needs alpha = num_a/det (one correctly rounded division).  det == 0 (sign(det) = 0 ->
//   x/0 -> 0*inf = NaN in the reference) takes the literal slow path so the NaN semantics are preserved bit for bit.
__device__ inline float ray_min_alpha(float x1, float y1, float rc, float rs, float sr, const float* s_seg, int no) {
  const float x2 = x1 + rc * sr;
  const float y2 = y1 + rs * sr;
  const float dx12 = x1 - x2, dy12 = y1 - y2;
  float amin = 0.0f;
  for (int o = 0; o < no; ++o) {
    float ao = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 sg = reinterpret_cast<const float4*>(s_seg)[o * 4 + m];
      const float x3 = sg.x, y3 = sg.y, ex = sg.z, ey = sg.w;
      const float det0 = dx12 * ey - dy12 * ex;
      const float ax = x1 - x3, ay = y1 - y3;
      const float na = ey * ax - ex * ay;
      const float nb = (-dy12) * ax + dx12 * ay;
      float al;
      if (det0 != 0.0f && det0 == det0) {
        const float det = copysignf(fminf(fmaxf(fabsf(det0), 1e-7f), 1e7f), det0);
        const bool pos = det > 0.0f;
        const bool va = (na == 0.0f || (na > 0.0f) == pos) && (pos ? (na <= det) : (na >= det));
        const bool vb = (nb == 0.0f || (nb > 0.0f) == pos) && (pos ? (nb <= det) : (nb >= det));
        al = 1e6f;
        if (va && vb) al = na / det + 0.0f;   // v*alpha + (1-v)*1e6 with v = 1: alpha + 0 (turns -0 into +0)
      } else {  // literal path: det = sign(det0) * clip(|det0|) = 0 (or NaN)
        al = segment_alpha_literal(det0, na, nb);
      }
      ao = (m == 0) ? al : nanmin(ao, al);
    }
    amin = (o == 0) ? ao : nanmin(amin, ao);
  }
  return amin;
}

// stable ascending rank of ray r among the R alphas `al` (env/utils.py:132-136): NaNs sort last, ties in index order
__device__ inline int ray_rank(const float* al, int R, int r) {
  const float ar = al[r];
  const bool nr = (ar != ar);
  int rank = 0;
  for (int j = 0; j < R; ++j) {
    const float aj = al[j];
    const bool nj = (aj != aj);
    bool less;
    if (nj || nr) less = (nj == nr) ? (j < r) : nr;
    else less = (aj < ar) || (aj == ar && j < r);
    rank += less ? 1 : 0;
  }
  return rank;
}

// hit point of a ray at alpha ar (env/utils.py:126-130)
__device__ inline void ray_hit(float x1, float y1, float rc, float rs, float sr, float ar, float* out2) {
  const float x2 = x1 + rc * sr;
  const float y2 = y1 + rs * sr;
  out2[0] = x1 + (x2 - x1) * ar;
  out2[1] = y1 + (y2 - y1) * ar;
}


#define MISS_BITS 0x49742400u  // bits of 1e6f

// wave-per-env LiDAR kernel (env_wave.hip): whether its instantiation list holds this (state_dim, spread, n_agents,
// n_obs), and the launch of that instance (step_family in env_step.hip decides when it runs)
bool lidar_wave_has_instance(const dgppo_env_cfg& c);
void launch_lidar_wave(const StepArgs& a, hipStream_t s);
bool lidar_wave_has_act_instance(const dgppo_env_cfg& c);                             // ... and its act-step form
void launch_lidar_wave_act(const StepArgs& a, const ActFeatArgs& f, hipStream_t s);   // MODE_STEP, compact record
