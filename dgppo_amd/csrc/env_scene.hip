// Episode start from user-given scenes (one thread per environment; executed once per rollout, where the reset runs): the
// dense env state of dgppo_env_reset from S template scenes instead of from the Philox-sampled one.  The reference ships no
// way to start an episode anywhere but at reset: its env_states is a Python pytree a user fills by hand; here the state is a
// device record, and this is the door to it.
//   goals      copied word for word
//   obstacles  LiDAR: the 16-float record from (cx, cy, w, h, theta) with the expressions of env_reset.hip's obstacle block
//              (Rectangle.create, dgppo/env/obstacle.py:39-56); MPE: [ox, oy, 0, 0]
//   agents     the template rows, or (jitter J > 0) x, y moved by (2 u - 1) J: attempt a = 0..15 draws d = a n + i for agent i
//              from the stream of env_reset.hip (Philox(counter=(d,0,0,0), key=(lo32 seed, hi32 seed)), words 0, 1), always
//              measured from the template; the first attempt whose scene is valid is kept
//   flags      0 = valid; DGPPO_SCENE_* bits otherwise
// Built with -ffp-contract=off like env_reset.hip.
#include "env_step.h"

#define SCENE_MAX_AGENTS 64
#define SCENE_ATTEMPTS 16

struct SceneArgs {
  dgppo_env_cfg cfg;
  const float* agent_t;
  const float* goal_t;
  const float* obst_t;
  int S;
  const int32_t* scene_ids;
  const uint64_t* seeds;
  float jitter;
  float* agent;
  float* goal;
  float* obst;
  int32_t* flags;
  int* n_failed;
  int B;
};

__device__ inline bool scene_finite(const float* p, int n_words) {
  bool ok = true;
  for (int i = 0; i < n_words; ++i) ok = ok && isfinite(p[i]);
  return ok;
}

// the geometric bits of the agents as they stand in `agent` (bits 2, 4, 8); a NaN position is in none of them (bit 1 has it)
__device__ inline int scene_geometry(const dgppo_env_cfg& c, const float* agent, const float* obst, bool lidar) {
  const int n = c.n_agents, no = c.n_obs, SD = c.state_dim;
  int bits = 0;
  for (int i = 0; i < n; ++i) {
    const float x = agent[i * SD], y = agent[i * SD + 1];
    if (x < 0.0f || x > c.area_size || y < 0.0f || y > c.y_limit) bits |= DGPPO_SCENE_OUT_OF_AREA;
    for (int j = i + 1; j < n; ++j) {
      const float dx = x - agent[j * SD], dy = y - agent[j * SD + 1];
      if (sqrtf(dx * dx + dy * dy) < c.two_car_radius) bits |= DGPPO_SCENE_AGENTS_OVERLAP;
    }
    for (int o = 0; o < no; ++o) {
      if (lidar) {
        if (rect_inside(obst + o * DGPPO_RECT_STRIDE, x, y, c.car_radius)) bits |= DGPPO_SCENE_AGENT_IN_OBSTACLE;
      } else {
        const float dx = x - obst[o * SD], dy = y - obst[o * SD + 1];
        if (sqrtf(dx * dx + dy * dy) < c.car_plus_obs) bits |= DGPPO_SCENE_AGENT_IN_OBSTACLE;
      }
    }
  }
  return bits;
}

__global__ void env_scene_load_kernel(SceneArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const dgppo_env_cfg& c = a.cfg;
  const int n = c.n_agents, ng = c.n_goals, no = c.n_obs, SD = c.state_dim;
  const bool lidar = cfg_is_lidar(c);
  const int OT = lidar ? 5 : 2;                          // floats per obstacle template row
  const int s = a.scene_ids ? a.scene_ids[b] : b % a.S;
  const float* agent_t = a.agent_t + (size_t)s * n * SD;
  const float* goal_t = a.goal_t + (size_t)s * ng * SD;
  const float* obst_t = a.obst_t ? a.obst_t + (size_t)s * no * OT : nullptr;
  float* agent = a.agent + (size_t)b * n * SD;
  float* goal = a.goal + (size_t)b * ng * SD;
  float* obst = a.obst ? a.obst + (size_t)b * no * cfg_obst_stride(c) : nullptr;

  const bool finite = scene_finite(agent_t, n * SD) && scene_finite(goal_t, ng * SD) && (no == 0 || scene_finite(obst_t, no * OT));
  const int nonfinite = finite ? 0 : DGPPO_SCENE_NONFINITE;

  // words, not floats: a NaN keeps its payload
  for (int i = 0; i < ng * SD; ++i) ((uint32_t*)goal)[i] = ((const uint32_t*)goal_t)[i];
  for (int i = 0; i < n * SD; ++i) ((uint32_t*)agent)[i] = ((const uint32_t*)agent_t)[i];

  for (int o = 0; o < no; ++o) {
    if (lidar) {                                         // the record of env_reset_kernel, statement for statement
      const float* t = obst_t + o * 5;
      const float cx = t[0], cy = t[1], w = t[2], h = t[3], th = t[4];
      float cs = cosf(th), sn = sinf(th);
      float* rec = obst + o * DGPPO_RECT_STRIDE;
      rec[0] = cx; rec[1] = cy; rec[2] = w; rec[3] = h; rec[4] = th; rec[5] = cs; rec[6] = sn; rec[7] = 0.0f;
      float hw = w / 2.0f, hh = h / 2.0f;
      float bx[4] = {hw, -hw, -hw, hw};
      float by[4] = {hh, hh, -hh, -hh};
      for (int m = 0; m < 4; ++m) {  // obstacle.py:40-54
        rec[8 + 2 * m] = (cs * bx[m] + (-sn) * by[m]) + cx;
        rec[9 + 2 * m] = (sn * bx[m] + cs * by[m]) + cy;
      }
    } else {                                             // mpe/base.py:121
      for (int d = 0; d < SD; ++d) obst[o * SD + d] = 0.0f;
      obst[o * SD] = obst_t[o * 2];
      obst[o * SD + 1] = obst_t[o * 2 + 1];
    }
  }

  int bits = nonfinite | scene_geometry(c, agent, obst, lidar);
  if (a.jitter > 0.0f) {
    const uint64_t seed = a.seeds[b];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float J = a.jitter;
    for (int attempt = 0; attempt < SCENE_ATTEMPTS; ++attempt) {
      for (int i = 0; i < n; ++i) {
        Philox4 p = philox4x32_10((uint32_t)(attempt * n + i), 0u, 0u, 0u, k0, k1);
        const float u0 = u01_from_u32(p.v[0]), u1 = u01_from_u32(p.v[1]);
        agent[i * SD] = agent_t[i * SD] + (2.0f * u0 - 1.0f) * J;
        agent[i * SD + 1] = agent_t[i * SD + 1] + (2.0f * u1 - 1.0f) * J;
      }
      bits = nonfinite | scene_geometry(c, agent, obst, lidar);
      if (bits == 0) break;
    }
    if (bits != 0 && a.n_failed) atomicAdd(a.n_failed, 1);
  }
  if (a.flags) a.flags[b] = bits;
}

extern "C" int32_t dgppo_env_scene_load(const dgppo_env_cfg* cfg, const float* agent_t, const float* goal_t, const float* obst_t,
                                        int32_t S, const int32_t* scene_ids, const uint64_t* seeds, float jitter, float* agent,
                                        float* goal, float* obst, int32_t* flags, int32_t* n_failed, int32_t B, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_env_scene_load", "dgppo_vmas_reset_checked (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(S >= 1, "scene_load: S must be >= 1 (got %d)", S);
  DGPPO_REQUIRE(B >= 0, "scene_load: B must be >= 0 (got %d)", B);
  DGPPO_REQUIRE(jitter >= 0.0f, "scene_load: jitter must be >= 0 and not NaN (got %g)", (double)jitter);
  DGPPO_REQUIRE(agent_t && goal_t && agent && goal, "scene_load: agent_t/goal_t/agent/goal must not be NULL");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst_t == nullptr), "scene_load: obst_t must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst == nullptr), "scene_load: obst must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE(jitter == 0.0f || seeds, "scene_load: seeds must not be NULL when jitter > 0");
  DGPPO_REQUIRE(cfg->n_agents <= SCENE_MAX_AGENTS, "scene_load supports at most %d agents", SCENE_MAX_AGENTS);
  if (B == 0) return 0;
  SceneArgs a;
  a.cfg = *cfg; a.agent_t = agent_t; a.goal_t = goal_t; a.obst_t = obst_t; a.S = S; a.scene_ids = scene_ids; a.seeds = seeds;
  a.jitter = jitter; a.agent = agent; a.goal = goal; a.obst = obst; a.flags = flags; a.n_failed = n_failed; a.B = B;
  hipLaunchKernelGGL(env_scene_load_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
