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
// The second half of the file, dgppo_env_scene_mix, puts SOME envs of a batch that holds a reset into such scenes (training on a
// mix of sampled and given starts): one wave per environment, and nothing of an env is written unless its scene is valid.
// The last part goes the other way: dgppo_env_scene_mine reads, from a rollout record, the state a few steps before every env's first
// unsafe step as template rows, with the validity bits the two kernels above would give them, and dgppo_env_scene_pool_push keeps
// the valid ones in a ring of pool slots that a later dgppo_env_scene_mix starts envs in.
// Built with -ffp-contract=off like env_reset.hip.
#include <stdio.h>
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

// one rectangle template row (cx, cy, w, h, theta) -> its 16-float record: the record of env_reset_kernel, statement for
// statement.  Shared by the two kernels below, so that their records cannot differ
__device__ inline void scene_rect_record(const float* t, float* rec) {
  const float cx = t[0], cy = t[1], w = t[2], h = t[3], th = t[4];
  float cs = cosf(th), sn = sinf(th);
  rec[0] = cx; rec[1] = cy; rec[2] = w; rec[3] = h; rec[4] = th; rec[5] = cs; rec[6] = sn; rec[7] = 0.0f;
  float hw = w / 2.0f, hh = h / 2.0f;
  float bx[4] = {hw, -hw, -hw, hw};
  float by[4] = {hh, hh, -hh, -hh};
  for (int m = 0; m < 4; ++m) {  // obstacle.py:40-54
    rec[8 + 2 * m] = (cs * bx[m] + (-sn) * by[m]) + cx;
    rec[9 + 2 * m] = (sn * bx[m] + cs * by[m]) + cy;
  }
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
    if (lidar) {
      scene_rect_record(obst_t + o * 5, obst + o * DGPPO_RECT_STRIDE);
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

// ---- dgppo_env_scene_mix: the scene start of SOME envs of a batch that already holds a valid reset ---------------------------
// One wave64 per env, lane i = agent i (SCENE_MAX_AGENTS is the wave width) and, for the obstacle records, lane o = obstacle o
// (n_obs <= 64, dgppo_validate_cfg).  The candidate position and the obstacle record live in registers; a lane reads the other
// agents' positions and the obstacles' words through __shfl, and the validity bits are folded with __any, so the attempt loop
// and the commit are wave-uniform: no LDS, no barrier.  Draws, expressions, attempts and bits are env_scene_load_kernel's.
// Nothing of the record is written before the verdict: an env whose scene stays invalid keeps its reset.
#define SCENE_MIX_WAVES 4                                 // waves (envs) per 256-thread block

struct SceneMixArgs {
  dgppo_env_cfg cfg;
  const float* agent_t;
  const float* goal_t;
  const float* obst_t;
  int S;
  const int32_t* scene_of;
  const uint64_t* seeds;
  float jitter;
  float* agent;
  float* goal;
  float* obst;
  int32_t* flags;
  int* n_fallback;
  int B;
};

// any lane's word of p[0 .. n_words) not finite?  (lanes stride over the words)
__device__ inline bool scene_wave_nonfinite(const float* p, int n_words, int lane) {
  bool bad = false;
  for (int i = lane; i < n_words; i += 64) bad = bad || !isfinite(p[i]);
  return __any(bad);
}

// the geometric bits of scene_geometry for the wave's candidate: lane i < n holds agent i at (x, y); lane o < n_obs holds
// obstacle o's record in rec (LiDAR) or its centre in rec[0], rec[1] (MPE).  The pair (i, j > i) is tested by lane i
__device__ inline int scene_wave_geometry(const dgppo_env_cfg& c, int lane, float x, float y, const float* rec, bool lidar) {
  const int n = c.n_agents, no = c.n_obs;
  const bool mine = lane < n;
  const bool out = mine && (x < 0.0f || x > c.area_size || y < 0.0f || y > c.y_limit);
  bool overlap = false, inside = false;
  for (int j = 1; j < n; ++j) {
    const float dx = x - __shfl(x, j), dy = y - __shfl(y, j);
    if (mine && j > lane && sqrtf(dx * dx + dy * dy) < c.two_car_radius) overlap = true;
  }
  for (int o = 0; o < no; ++o) {
    if (lidar) {
      float r[7];                                        // the words rect_inside reads, from lane o's registers
      r[0] = __shfl(rec[0], o); r[1] = __shfl(rec[1], o); r[2] = __shfl(rec[2], o); r[3] = __shfl(rec[3], o);
      r[4] = 0.0f; r[5] = __shfl(rec[5], o); r[6] = __shfl(rec[6], o);
      if (mine && rect_inside(r, x, y, c.car_radius)) inside = true;
    } else {
      const float dx = x - __shfl(rec[0], o), dy = y - __shfl(rec[1], o);
      if (mine && sqrtf(dx * dx + dy * dy) < c.car_plus_obs) inside = true;
    }
  }
  return (__any(out) ? DGPPO_SCENE_OUT_OF_AREA : 0) | (__any(overlap) ? DGPPO_SCENE_AGENTS_OVERLAP : 0) |
         (__any(inside) ? DGPPO_SCENE_AGENT_IN_OBSTACLE : 0);
}

__global__ __launch_bounds__(64 * SCENE_MIX_WAVES) void env_scene_mix_kernel(SceneMixArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SCENE_MIX_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= a.B) return;
  const int s = a.scene_of[b];
  if (s < 0) return;                                     // a kept env: its reset stands, its flag is not ours
  const dgppo_env_cfg& c = a.cfg;
  const int n = c.n_agents, ng = c.n_goals, no = c.n_obs, SD = c.state_dim;
  const bool lidar = cfg_is_lidar(c);
  const int OT = lidar ? 5 : 2;
  const float* agent_t = a.agent_t + (size_t)s * n * SD;
  const float* goal_t = a.goal_t + (size_t)s * ng * SD;
  const float* obst_t = a.obst_t ? a.obst_t + (size_t)s * no * OT : nullptr;

  bool bad = scene_wave_nonfinite(agent_t, n * SD, lane);
  bad = scene_wave_nonfinite(goal_t, ng * SD, lane) || bad;
  if (no > 0) bad = scene_wave_nonfinite(obst_t, no * OT, lane) || bad;
  const int nonfinite = bad ? DGPPO_SCENE_NONFINITE : 0;

  float rec[DGPPO_RECT_STRIDE];
  for (int k = 0; k < DGPPO_RECT_STRIDE; ++k) rec[k] = 0.0f;
  if (lane < no) {
    if (lidar) {
      scene_rect_record(obst_t + lane * 5, rec);
    } else {
      rec[0] = obst_t[lane * 2];
      rec[1] = obst_t[lane * 2 + 1];
    }
  }
  const bool mine = lane < n;
  const float xt = mine ? agent_t[lane * SD] : 0.0f, yt = mine ? agent_t[lane * SD + 1] : 0.0f;
  float x = xt, y = yt;
  int bits;
  if (a.jitter > 0.0f) {
    const uint64_t seed = a.seeds[b];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float J = a.jitter;
    for (int attempt = 0; attempt < SCENE_ATTEMPTS; ++attempt) {
      Philox4 p = philox4x32_10((uint32_t)(attempt * n + lane), 0u, 0u, 0u, k0, k1);
      const float u0 = u01_from_u32(p.v[0]), u1 = u01_from_u32(p.v[1]);
      x = xt + (2.0f * u0 - 1.0f) * J;
      y = yt + (2.0f * u1 - 1.0f) * J;
      bits = nonfinite | scene_wave_geometry(c, lane, x, y, rec, lidar);
      if (bits == 0) break;
    }
  } else {
    bits = nonfinite | scene_wave_geometry(c, lane, x, y, rec, lidar);
  }

  if (bits == 0) {                                       // the commit: words, as env_scene_load_kernel copies them
    uint32_t* goal = (uint32_t*)(a.goal + (size_t)b * ng * SD);
    for (int i = lane; i < ng * SD; i += 64) goal[i] = ((const uint32_t*)goal_t)[i];
    if (mine) {
      float* agent = a.agent + (size_t)b * n * SD + lane * SD;
      for (int d = 0; d < SD; ++d) ((uint32_t*)agent)[d] = ((const uint32_t*)agent_t)[lane * SD + d];
      if (a.jitter > 0.0f) {
        agent[0] = x;
        agent[1] = y;
      }
    }
    for (int o = lane; o < no; o += 64) {                // n_obs <= 64: one trip, lane o's own record
      if (lidar) {
        float* out = a.obst + ((size_t)b * no + o) * DGPPO_RECT_STRIDE;
        for (int k = 0; k < DGPPO_RECT_STRIDE; ++k) out[k] = rec[k];
      } else {                                           // mpe/base.py:121
        float* out = a.obst + ((size_t)b * no + o) * SD;
        for (int d = 0; d < SD; ++d) out[d] = 0.0f;
        out[0] = rec[0];
        out[1] = rec[1];
      }
    }
  }
  if (lane == 0) {
    if (a.flags) a.flags[b] = bits;
    if (bits != 0 && a.n_fallback) atomicAdd(a.n_fallback, 1);
  }
}

extern "C" int32_t dgppo_env_scene_mix(const dgppo_env_cfg* cfg, const float* agent_t, const float* goal_t, const float* obst_t,
                                       int32_t S, const int32_t* scene_of, const uint64_t* seeds, float jitter, float* agent,
                                       float* goal, float* obst, int32_t* flags, int32_t* n_fallback, int32_t B, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {                                              // every refusal names the entry point: dgppo_validate_cfg's does not
    char why[256];
    snprintf(why, sizeof(why), "%s", dgppo_last_error());
    dgppo_set_error("dgppo_env_scene_mix: %s", why);
    return rc;
  }
  DGPPO_REFUSE_VMAS(cfg, "dgppo_env_scene_mix", "dgppo_vmas_reset_checked (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(S >= 1, "dgppo_env_scene_mix: S must be >= 1 (got %d)", S);
  DGPPO_REQUIRE(B >= 0, "dgppo_env_scene_mix: B must be >= 0 (got %d)", B);
  DGPPO_REQUIRE(jitter >= 0.0f, "dgppo_env_scene_mix: jitter must be >= 0 and not NaN (got %g)", (double)jitter);
  DGPPO_REQUIRE(agent_t && goal_t && agent && goal, "dgppo_env_scene_mix: agent_t/goal_t/agent/goal must not be NULL");
  DGPPO_REQUIRE(scene_of && seeds, "dgppo_env_scene_mix: scene_of/seeds must not be NULL");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst_t == nullptr), "dgppo_env_scene_mix: obst_t must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst == nullptr), "dgppo_env_scene_mix: obst must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE(cfg->n_agents <= SCENE_MAX_AGENTS, "dgppo_env_scene_mix supports at most %d agents", SCENE_MAX_AGENTS);
  if (B == 0) return 0;
  SceneMixArgs a;
  a.cfg = *cfg; a.agent_t = agent_t; a.goal_t = goal_t; a.obst_t = obst_t; a.S = S; a.scene_of = scene_of; a.seeds = seeds;
  a.jitter = jitter; a.agent = agent; a.goal = goal; a.obst = obst; a.flags = flags; a.n_fallback = n_fallback; a.B = B;
  hipLaunchKernelGGL(env_scene_mix_kernel, dim3(cdiv(B, SCENE_MIX_WAVES)), dim3(64 * SCENE_MIX_WAVES), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- dgppo_env_scene_mine: the state `back` steps before every env's first unsafe step, as scene template rows ---------------
// One wave64 per env, SCENE_MIX_WAVES envs per block.  The scan reads the env's cost row of a step, W = n * n_cost words, with
// consecutive lanes on consecutive words, max(1, 64 / W) steps per pass; the passes run in time order and the wave leaves at
// the first one in which any lane saw a word >= thresh (a NaN compares false), so a failing env reads only up to its failure.
// The smallest key t * W + w over the lanes is the first unsafe step and its lowest unsafe word.  The rows of step
// t0 = max(first - back, 0) are then copied word for word and judged with the functions of env_scene_mix_kernel: lane i = agent
// i, lane o = obstacle o with its record rebuilt from the five words the template keeps.  No LDS, no barrier.
struct SceneMineArgs {
  dgppo_env_cfg cfg;
  const float* agent_tm;
  const float* cost_tm;
  int Bs;
  const float* goal;
  const float* obst;
  int T;
  int back;
  float thresh;
  int32_t* first;
  int32_t* who;
  int32_t* t0;
  int32_t* flags;
  float* agent_t;
  float* goal_t;
  float* obst_t;
  int B;
};

#define SCENE_NO_KEY 0x7fffffff

__global__ __launch_bounds__(64 * SCENE_MIX_WAVES) void env_scene_mine_kernel(SceneMineArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SCENE_MIX_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= a.B) return;
  const dgppo_env_cfg& c = a.cfg;
  const int n = c.n_agents, ng = c.n_goals, no = c.n_obs, SD = c.state_dim;
  const bool lidar = cfg_is_lidar(c);
  const int OT = lidar ? 5 : 2, OS = cfg_obst_stride(c);
  const int W = n * c.n_cost;
  const int P = W < 64 ? 64 / W : 1;                     // steps per pass
  const size_t step_words = (size_t)a.Bs * W;
  const float* cost = a.cost_tm + (size_t)b * W;

  int key = SCENE_NO_KEY;
  for (int tb = 0; tb < a.T; tb += P) {
    for (int idx = lane; idx < P * W; idx += 64) {
      const int dt = idx / W, w = idx - dt * W, t = tb + dt;
      if (t < a.T && cost[(size_t)t * step_words + w] >= a.thresh) key = min(key, t * W + w);
    }
    if (__any(key != SCENE_NO_KEY)) break;
  }
  for (int m = 32; m >= 1; m >>= 1) key = min(key, __shfl_xor(key, m));

  if (key == SCENE_NO_KEY) {                             // never unsafe: the rows are not ours to touch
    if (lane == 0) {
      a.first[b] = -1; a.who[b] = -1; a.t0[b] = -1; a.flags[b] = 0;
    }
    return;
  }
  const int first = key / W, who = key - first * W;
  const int t0 = max(first - a.back, 0);
  const float* agent = a.agent_tm + ((size_t)t0 * a.Bs + b) * n * SD;
  const float* goal = a.goal + (size_t)b * ng * SD;
  const float* obst = a.obst ? a.obst + (size_t)b * no * OS : nullptr;

  bool bad = scene_wave_nonfinite(agent, n * SD, lane);
  bad = scene_wave_nonfinite(goal, ng * SD, lane) || bad;
  bool obad = false;
  for (int i = lane; i < no * OT; i += 64) {             // the template's words of the obstacle records
    const int o = i / OT;
    obad = obad || !isfinite(obst[o * OS + (i - o * OT)]);
  }
  bad = __any(obad) || bad;
  const int nonfinite = bad ? DGPPO_SCENE_NONFINITE : 0;

  float rec[DGPPO_RECT_STRIDE];
  for (int k = 0; k < DGPPO_RECT_STRIDE; ++k) rec[k] = 0.0f;
  if (lane < no) {
    if (lidar) {
      float t[5];
      for (int k = 0; k < 5; ++k) t[k] = obst[lane * OS + k];
      scene_rect_record(t, rec);
    } else {
      rec[0] = obst[lane * OS];
      rec[1] = obst[lane * OS + 1];
    }
  }
  const bool mine = lane < n;
  const float x = mine ? agent[lane * SD] : 0.0f, y = mine ? agent[lane * SD + 1] : 0.0f;
  const int bits = nonfinite | scene_wave_geometry(c, lane, x, y, rec, lidar);

  uint32_t* agent_t = (uint32_t*)(a.agent_t + (size_t)b * n * SD);
  for (int i = lane; i < n * SD; i += 64) agent_t[i] = ((const uint32_t*)agent)[i];
  uint32_t* goal_t = (uint32_t*)(a.goal_t + (size_t)b * ng * SD);
  for (int i = lane; i < ng * SD; i += 64) goal_t[i] = ((const uint32_t*)goal)[i];
  if (no > 0) {
    uint32_t* obst_t = (uint32_t*)(a.obst_t + (size_t)b * no * OT);
    for (int i = lane; i < no * OT; i += 64) {
      const int o = i / OT;
      obst_t[i] = ((const uint32_t*)obst)[o * OS + (i - o * OT)];
    }
  }
  if (lane == 0) {
    a.first[b] = first; a.who[b] = who; a.t0[b] = t0; a.flags[b] = bits;
  }
}

// every refusal of the two entry points below names them: dgppo_validate_cfg's own message does not
static int32_t scene_validate_cfg(const dgppo_env_cfg* cfg, const char* fn) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {
    char why[256];
    snprintf(why, sizeof(why), "%s", dgppo_last_error());
    dgppo_set_error("%s: %s", fn, why);
  }
  return rc;
}

extern "C" int32_t dgppo_env_scene_mine(const dgppo_env_cfg* cfg, const float* agent_tm, const float* cost_tm, int32_t Bs,
                                        const float* goal, const float* obst, int32_t T, int32_t back, float thresh,
                                        int32_t* first, int32_t* who, int32_t* t0, int32_t* flags, float* agent_t, float* goal_t,
                                        float* obst_t, int32_t B, void* stream) {
  int32_t rc = scene_validate_cfg(cfg, "dgppo_env_scene_mine");
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_env_scene_mine", "nothing (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(B >= 0, "dgppo_env_scene_mine: B must be >= 0 (got %d)", B);
  DGPPO_REQUIRE(Bs >= B, "dgppo_env_scene_mine: Bs, the envs per time slot of the record, must be >= B (got %d, B %d)", Bs, B);
  DGPPO_REQUIRE(T >= 1, "dgppo_env_scene_mine: T must be >= 1 (got %d)", T);
  DGPPO_REQUIRE(back >= 0, "dgppo_env_scene_mine: back must be >= 0 (got %d)", back);
  DGPPO_REQUIRE(isfinite(thresh), "dgppo_env_scene_mine: thresh must be finite (got %g)", (double)thresh);
  DGPPO_REQUIRE(agent_tm && cost_tm && goal, "dgppo_env_scene_mine: agent_tm/cost_tm/goal must not be NULL");
  DGPPO_REQUIRE(first && who && t0 && flags && agent_t && goal_t,
                "dgppo_env_scene_mine: first/who/t0/flags/agent_t/goal_t must not be NULL");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst == nullptr), "dgppo_env_scene_mine: obst must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst_t == nullptr), "dgppo_env_scene_mine: obst_t must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE(cfg->n_agents <= SCENE_MAX_AGENTS, "dgppo_env_scene_mine supports at most %d agents", SCENE_MAX_AGENTS);
  DGPPO_REQUIRE((int64_t)T * cfg->n_agents * cfg->n_cost < (int64_t)SCENE_NO_KEY,
                "dgppo_env_scene_mine: T * n_agents * n_cost must be below 2^31 - 1 (T %d)", T);
  if (B == 0) return 0;
  SceneMineArgs a;
  a.cfg = *cfg; a.agent_tm = agent_tm; a.cost_tm = cost_tm; a.Bs = Bs; a.goal = goal; a.obst = obst; a.T = T; a.back = back;
  a.thresh = thresh; a.first = first; a.who = who; a.t0 = t0; a.flags = flags; a.agent_t = agent_t; a.goal_t = goal_t;
  a.obst_t = obst_t; a.B = B;
  hipLaunchKernelGGL(env_scene_mine_kernel, dim3(cdiv(B, SCENE_MIX_WAVES)), dim3(64 * SCENE_MIX_WAVES), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- dgppo_env_scene_pool_push: the mined rows of the taken envs into a ring of pool slots ---------------------------------------
// One workgroup: a deterministic stream compaction.  Env b is taken iff first[b] >= 1 && flags[b] == 0; the taken envs are ranked
// in ascending b (a ballot per wave, a prefix over the waves in LDS, chunks of the block size over B) and rank r < R goes to slot
// fixed + (head + r) % R: the ranks are distinct, so are the slots, and no atomic decides anything.  A wave copies the rows of
// its own taken envs, its lanes striding over a row's words.
#define SCENE_PUSH_WAVES 4

struct ScenePushArgs {
  const int32_t* first;
  const int32_t* flags;
  const uint32_t* agent_t;
  const uint32_t* goal_t;
  const uint32_t* obst_t;
  uint32_t* pool_agent;
  uint32_t* pool_goal;
  uint32_t* pool_obst;
  int words_agent, words_goal, words_obst;               // per row
  int M, fixed;
  int32_t* state;
  int32_t* slot_of;
  int B;
};

__global__ __launch_bounds__(64 * SCENE_PUSH_WAVES) void env_scene_pool_push_kernel(ScenePushArgs a) {
  __shared__ int wave_count[SCENE_PUSH_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = a.M - a.fixed;
  const int head = a.state[0], filled = a.state[1], pushed = a.state[2];    // read before the first barrier, written after the last
  int base = 0;                                          // taken envs of the chunks before this one
  for (int chunk = 0; chunk < a.B; chunk += 64 * SCENE_PUSH_WAVES) {
    const int b = chunk + tid;
    const bool taken = b < a.B && a.first[b] >= 1 && a.flags[b] == 0;
    const unsigned long long ballot = __ballot(taken);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SCENE_PUSH_WAVES; ++w) {
      const int cnt = wave_count[w];
      if (w < wave) before += cnt;
      total += cnt;
    }
    const int r = base + before + __popcll(ballot & ((1ull << lane) - 1ull));
    const int slot = (taken && r < R) ? a.fixed + (head + r) % R : -1;
    if (b < a.B && a.slot_of) a.slot_of[b] = slot;
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {                                       // wave-uniform: one taken env of this wave per trip
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const size_t src = (size_t)(chunk + wave * 64 + k), dst = (size_t)__shfl(slot, k);
      for (int i = lane; i < a.words_agent; i += 64) a.pool_agent[dst * a.words_agent + i] = a.agent_t[src * a.words_agent + i];
      for (int i = lane; i < a.words_goal; i += 64) a.pool_goal[dst * a.words_goal + i] = a.goal_t[src * a.words_goal + i];
      for (int i = lane; i < a.words_obst; i += 64) a.pool_obst[dst * a.words_obst + i] = a.obst_t[src * a.words_obst + i];
    }
    base += total;
    __syncthreads();                                     // wave_count is rewritten by the next chunk
  }
  if (tid == 0) {
    const int m = min(base, R);
    a.state[0] = (head + m) % R;
    a.state[1] = min(R, filled + m);
    a.state[2] = (int32_t)((uint32_t)pushed + (uint32_t)m);
    a.state[3] = base;
  }
}

extern "C" int32_t dgppo_env_scene_pool_push(const dgppo_env_cfg* cfg, const int32_t* first, const int32_t* flags,
                                             const float* agent_t, const float* goal_t, const float* obst_t, float* pool_agent,
                                             float* pool_goal, float* pool_obst, int32_t M, int32_t fixed, int32_t* state,
                                             int32_t* slot_of, int32_t B, void* stream) {
  int32_t rc = scene_validate_cfg(cfg, "dgppo_env_scene_pool_push");
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_env_scene_pool_push", "nothing (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(B >= 0, "dgppo_env_scene_pool_push: B must be >= 0 (got %d)", B);
  DGPPO_REQUIRE(M >= 1 && M <= (1 << 30), "dgppo_env_scene_pool_push: M must be in [1, 2^30] (got %d)", M);
  DGPPO_REQUIRE(fixed >= 0 && fixed < M, "dgppo_env_scene_pool_push: fixed must be in [0, M) (got %d, M %d)", fixed, M);
  DGPPO_REQUIRE(first && flags && agent_t && goal_t && pool_agent && pool_goal && state,
                "dgppo_env_scene_pool_push: first/flags/agent_t/goal_t/pool_agent/pool_goal/state must not be NULL");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (obst_t == nullptr), "dgppo_env_scene_pool_push: obst_t must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE((cfg->n_obs == 0) == (pool_obst == nullptr),
                "dgppo_env_scene_pool_push: pool_obst must be NULL exactly when n_obs == 0");
  DGPPO_REQUIRE(cfg->n_agents <= SCENE_MAX_AGENTS, "dgppo_env_scene_pool_push supports at most %d agents", SCENE_MAX_AGENTS);
  ScenePushArgs a;
  a.first = first; a.flags = flags; a.agent_t = (const uint32_t*)agent_t; a.goal_t = (const uint32_t*)goal_t;
  a.obst_t = (const uint32_t*)obst_t; a.pool_agent = (uint32_t*)pool_agent; a.pool_goal = (uint32_t*)pool_goal;
  a.pool_obst = (uint32_t*)pool_obst;
  a.words_agent = cfg->n_agents * cfg->state_dim; a.words_goal = cfg->n_goals * cfg->state_dim;
  a.words_obst = cfg->n_obs * (cfg_is_lidar(*cfg) ? 5 : 2);
  a.M = M; a.fixed = fixed; a.state = state; a.slot_of = slot_of; a.B = B;
  hipLaunchKernelGGL(env_scene_pool_push_kernel, dim3(1), dim3(64 * SCENE_PUSH_WAVES), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
