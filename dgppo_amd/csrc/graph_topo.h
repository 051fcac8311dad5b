// Slot topology of the per-agent fixed-fan-in graph, shared between graph_feats.hip (features), the attention kernels (nn_attn.h) and env_sweep.hip
// (features of a swept agent): both address the same (agent, slot) layout through these definitions.
#pragma once
#include "common.h"

struct Topo {
  int n, ng, gs, os, per, lidar, spread;  // per = k (LiDAR) or n_obs (MPE)
  int S, Ns;                              // slots per agent, nodes without pad
};

static inline Topo make_topo(const dgppo_env_cfg& c) {
  Topo t;
  t.n = c.n_agents; t.ng = c.n_goals; t.gs = cfg_goal_slots(c); t.os = cfg_obs_slots(c);
  t.lidar = cfg_is_lidar(c) ? 1 : 0; t.spread = cfg_is_spread(c) ? 1 : 0;
  t.per = t.os;
  t.S = t.n + t.gs + t.os;
  t.Ns = t.n + t.ng + cfg_obs_nodes(c);
  return t;
}

__device__ inline int sender_node(const Topo& t, int i, int s) {
  if (s < t.n) return s;
  if (s < t.n + t.gs) return t.spread ? t.n + (s - t.n) : t.n + i;
  const int m = s - t.n - t.gs;
  return t.lidar ? t.n + t.ng + i * t.per + m : t.n + t.ng + m;
}

// sqrt(dx^2 + dy^2) in single IEEE operations whatever the translation unit's contraction setting
__device__ inline float dist_rn(float dx, float dy) { return __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))); }
