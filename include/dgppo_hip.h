/*
 * dgppo_hip.h — C ABI of libdgppo_hip.so, the MI355X (gfx950) implementation of
 * DGPPO's data-parallel hot path.
 *
 * The reference (syzhang092218-source/dgppo) is pure Python/JAX and has NO FFI
 * of its own; the boundary it exposes is the Python API (dgppo.env / dgppo.algo /
 * dgppo.trainer).  This header is therefore the C ABI *underneath* that Python
 * API: every entry point names the reference function(s) (file:line relative to
 * /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (a torch.Tensor kept
 *     alive by Python); the library never allocates persistent memory, keeps no
 *     global mutable state apart from the thread-local error string, and never
 *     synchronises: all work is enqueued on the caller-supplied hipStream_t
 *     (passed as void*; NULL = the null stream);
 *   - all floating point is IEEE fp32, all indices int32, row-major, contiguous;
 *   - return value: 0 ok, <0 bad argument (see dgppo_last_error()), >0 hipError_t;
 *   - shapes are passed explicitly and validated on the host before any launch.
 */
#ifndef DGPPO_HIP_H
#define DGPPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGPPO_ABI_VERSION 3

/* environment kinds — dgppo/env/__init__.py:9-23 (registered ids on the hot path) */
enum {
  DGPPO_ENV_LIDAR_SPREAD = 0,         /* dgppo/env/lidar_env/lidar_spread.py */
  DGPPO_ENV_LIDAR_TARGET = 1,         /* dgppo/env/lidar_env/lidar_target.py */
  DGPPO_ENV_LIDAR_BICYCLE_TARGET = 2, /* dgppo/env/lidar_env/lidar_bicycle_target.py */
  DGPPO_ENV_MPE_SPREAD = 3,           /* dgppo/env/mpe/mpe_spread.py */
  DGPPO_ENV_MPE_TARGET = 4,           /* dgppo/env/mpe/mpe_target.py */
  /* task variants: same step / graph kernels, different reset, reward goals, goal-node count */
  DGPPO_ENV_LIDAR_LINE = 5,           /* dgppo/env/lidar_env/lidar_line.py : 2 landmark nodes, goals on the segment */
  DGPPO_ENV_MPE_LINE = 6,             /* dgppo/env/mpe/mpe_line.py */
  DGPPO_ENV_MPE_FORMATION = 7,        /* dgppo/env/mpe/mpe_formation.py : 1 landmark node, goals on a circle */
  DGPPO_ENV_MPE_CORRIDOR = 8,         /* dgppo/env/mpe/mpe_corridor.py : two fixed discs, y limit 2 * area */
  DGPPO_ENV_MPE_CONNECT_SPREAD = 9,   /* dgppo/env/mpe/mpe_connect_spread.py : third (connectivity) cost */
  /* contact physics (dgppo/env/vmas/): its own record and entry points (dgppo_vmas_*), see below */
  DGPPO_ENV_VMAS_REVERSE_TRANSPORT = 10 /* dgppo/env/vmas/vmas_reverse_transport.py */
};
/* dgppo_env_cfg.reward_goals: how the n positions the reward measures against follow from the goal nodes */
enum {
  DGPPO_GOALS_NODES = 0,         /* the goal nodes themselves                                   lidar_spread.py:35-52   */
  DGPPO_GOALS_LINE = 1,          /* l0 + i (l1 - l0) / (n - 1), i = 0..n-1                      lidar_line.py:131-136   */
  DGPPO_GOALS_LINE_INTERIOR = 2, /* l0 + (i + 1) (l1 - l0) / (n + 1)  (MPELine, n <= 3)         mpe_line.py:124-133     */
  DGPPO_GOALS_CIRCLE = 3         /* landmark + comm_radius [cos, sin](2 pi i / n)               mpe_formation.py:94-98  */
};

/* Obstacle record of the LiDAR envs: 16 floats per rectangle
 * (dgppo/env/obstacle.py:30-56  Rectangle(type, center, width, height, theta, points)):
 *   [0..1] center  [2] width  [3] height  [4] theta  [5] cos(theta)  [6] sin(theta)  [7] 0
 *   [8..15] points[4][2]
 * MPE obstacles are plain state rows [ox, oy, 0, 0] (dgppo/env/mpe/base.py:121).        */
#define DGPPO_RECT_STRIDE 16

/* Static description of one environment family + PARAMS
 * (dgppo/env/lidar_env/lidar_spread.py:13-22, dgppo/env/mpe/mpe_spread.py:12-19,
 *  dgppo/env/__init__.py:29-53).  Thresholds that the reference forms from Python
 * doubles and then rounds to fp32 are passed pre-rounded so host and device agree. */
typedef struct dgppo_env_cfg {
  int32_t kind;        /* DGPPO_ENV_* */
  int32_t n_agents;    /* n */
  int32_t n_goals;     /* goal NODES of the graph: n, 2 (Line: landmarks) or 1 (Formation) */
  int32_t n_obs;       /* rectangles (LiDAR) or discs (MPE); may be 0 */
  int32_t n_rays;      /* R (LiDAR only) */
  int32_t top_k;       /* k = top_k_rays (LiDAR only) */
  int32_t state_dim;   /* 4, or 5 for the bicycle */
  int32_t node_dim;    /* state_dim + 3 */
  float area_size;
  float dt;
  float car_radius;
  float comm_radius;
  float obs_radius;        /* MPE only */
  float dist2goal;
  float two_car_radius;    /* fp32(2 * car_radius)                       lidar_env/base.py:188 */
  float lidar_mask_radius; /* fp32(comm_radius - 1e-1)                   lidar_spread.py:88   */
  float eye_offset;        /* fp32(comm_radius + 1)                      lidar_spread.py:64   */
  float car_plus_obs;      /* fp32(car_radius + obs_radius)              mpe/base.py:181      */
  float vel_limit;         /* 0.5 (LiDAR) or 1.0 (MPE)                   state_lim()          */
  float reset_min_dist;    /* fp32(2.2*car_radius) LiDAR, fp32(2*car_radius) MPE, fp32(2.3*car_radius) ConnectSpread */
  /* ---- task variants (ABI 3); defaults reproduce the five base kinds ---- */
  int32_t reward_goals;    /* DGPPO_GOALS_*                                                                          */
  int32_t n_cost;          /* 2, or 3 with the connectivity cost                   mpe_connect_spread.py:46-52,115-117 */
  float obs_mask_radius;   /* MPE agent-obstacle edge mask: comm_radius, or fp32(100*comm_radius)  mpe_corridor.py:93   */
  float y_limit;           /* upper state limit in y: area_size or fp32(2*area_size)               mpe_corridor.py:62-65 */
  float connect_radius;    /* mpe_connect_spread.py:24                                                                */
  float reset_side_y;      /* height of the box agents / goals are sampled in at reset             mpe_corridor.py:50   */
  float goal_shift_y;      /* added to the sampled goals' y                                        mpe_corridor.py:52   */
  float line_min_dist;     /* minimum landmark separation                                          mpe_line.py:49-52    */
} dgppo_env_cfg;

/* Optional materialised GraphsTuple (dgppo/utils/graph.py:47-86, GetGraph.to_padded
 * :212-247).  Any pointer group may be NULL as a whole (all-or-nothing).            */
typedef struct dgppo_graph_out {
  float*   nodes;      /* [B, N, node_dim]   */
  float*   edges;      /* [B, E, 4]          */
  float*   states;     /* [B, N, state_dim]  */
  int32_t* receivers;  /* [B, E]             */
  int32_t* senders;    /* [B, E]             */
  int32_t* node_type;  /* [B, N]             */
  int32_t* n_node;     /* [B]                */
  int32_t* n_edge;     /* [B]                */
} dgppo_graph_out;

int32_t     dgppo_abi_version(void);
const char* dgppo_last_error(void);

/* number of nodes N (incl. pad) / edges E of the padded graph — graph.py:212-247 */
int32_t dgppo_env_num_nodes(const dgppo_env_cfg* cfg);
int32_t dgppo_env_num_edges(const dgppo_env_cfg* cfg);

/* ---- environment ---------------------------------------------------------------- */

/* One batched env.step: replaces LidarEnv.step (dgppo/env/lidar_env/base.py:151-174),
 * MPE.step (dgppo/env/mpe/base.py:137-162) and everything they call:
 *   clip_action/clip_state (env/base.py:80-86), agent_step_euler (lidar_env/base.py:142-149,
 *   lidar_bicycle_target.py:92-111, mpe/base.py:129-135), get_lidar/raytracing/top-k
 *   (env/utils.py:49-55,115-136; obstacle.py:62-105), get_reward (lidar_spread.py:35-52,
 *   lidar_target.py:35-52, mpe_spread.py:32-49, mpe_target.py:32-49), get_cost
 *   (lidar_env/base.py:180-207, mpe/base.py:164-191), edge_blocks + get_graph + to_padded.
 *
 *   agent      [B, n, sd]   state at t
 *   action     [B, n, 2]    raw action (clipped inside).  NULL => "sense only": no dynamics,
 *                           no reward/cost; next_agent := agent (used by reset to build graph_0)
 *   goal       [B, ng, sd]
 *   obst       LiDAR: [B, n_obs, 16] rectangle records; MPE: [B, n_obs, sd]; may be NULL iff n_obs==0
 *   hits       LiDAR: [B, n, k, 2] hit points of the graph at t (obstacle cost reads them,
 *                           lidar_env/base.py:194-197); NULL for MPE / n_obs==0 / sense-only
 *   ray_cos/ray_sin [R]     cos/sin(linspace(-pi, pi-2pi/R, R)) (env/utils.py:51), fp32
 *   next_agent [B, n, sd]   out
 *   next_hits  [B, n, k, 2] out (LiDAR)
 *   reward     [B]          out (reward of step t, on the pre-step graph)
 *   cost       [B, n, 2]    out
 *   gout       optional materialised graph at t+1                                        */
int32_t dgppo_env_step(const dgppo_env_cfg* cfg,
                       const float* agent, const float* action, const float* goal,
                       const float* obst, const float* hits,
                       const float* ray_cos, const float* ray_sin,
                       float* next_agent, float* next_hits, float* reward, float* cost,
                       const dgppo_graph_out* gout, int32_t B, void* stream);

/* One rollout step after the policy's forward, in one launch: draw the action from the head output (what
 * dgppo_policy_head does in modes 0 / 1), step the env (what dgppo_env_step writes to the compact record), and emit the
 * graph features of state t+1 (what dgppo_graph_feats gives for it at Fp = 8) and their layer-0 queries
 * qt0 = Xa Mcat + cvec (what dgppo_dense_fwd gives) -- each bit for bit.
 * dgppo_env_act_step_feats_supported: 1 if the configuration has such a kernel: a base LiDAR kind with 32 rays, top-k 8,
 * n_obs >= 1, eye_offset >= comm_radius, n_agents <= 8 and (state_dim, n_agents, n_obs) among the wave-per-env instances, at Fp = 8 and
 * H = 3; the entry point refuses everything else.
 *   agent, goal, obst, hits, ray_cos, ray_sin       as dgppo_env_step (16-byte aligned)
 *   ms         [B*n, 4]     head output: mean0, mean1, std_trans0, std_trans1
 *   eps        [B*n, 2]     noise (sample != 0; else may be NULL)
 *   sample     1: tanh(mean + std eps) and log pi; 0: tanh(mean)
 *   action     [B, n, 2]    out
 *   log_pi     [B, n]       out (sample != 0; else may be NULL)
 *   next_agent, next_hits, reward, cost             out, as dgppo_env_step
 *   Xa [B*n, 8], Xo [B*(n + n*k), 8], efeat [B*n, S, 4], emask [B*n, S]   out, of state t+1; Xa == NULL: not emitted
 *   Mcat [8, 24], cvec [24], qt0 [B*n, 24]          qt0 out, of state t+1; qt0 == NULL: not emitted
 *   max_blocks 0, or a cap of the persistent grid (tests)                                             */
int32_t dgppo_env_act_step_feats_supported(const dgppo_env_cfg* cfg, int32_t Fp, int32_t H);
int32_t dgppo_env_act_step_feats(const dgppo_env_cfg* cfg, const float* agent, const float* goal, const float* obst,
                                 const float* hits, const float* ray_cos, const float* ray_sin, const float* ms,
                                 const float* eps, int32_t sample, float* action, float* log_pi, float* next_agent,
                                 float* next_hits, float* reward, float* cost, float* Xa, float* Xo, float* efeat,
                                 float* emask, int32_t Fp, const float* Mcat, const float* cvec, float* qt0, int32_t H,
                                 int32_t max_blocks, int32_t B, void* stream);

/* Materialise the GraphsTuple of a stored compact record (lazy rollout.graph view):
 * same arithmetic as get_graph (lidar_env/base.py:227-271, mpe/base.py:211-241).     */
int32_t dgppo_graph_materialize(const dgppo_env_cfg* cfg,
                                const float* agent, const float* goal,
                                const float* obst, const float* hits,
                                const dgppo_graph_out* gout, int32_t B, void* stream);

/* Batched reset: replaces LidarEnv.reset (lidar_env/base.py:89-124), LidarBicycleTarget.reset
 * (lidar_bicycle_target.py:60-90), MPE.reset (mpe/base.py:81-127), get_node_goal_rng
 * (env/utils.py:139-244), Rectangle.create (obstacle.py:39-56).  Philox-4x32-10 counter RNG
 * keyed by seeds[b] (the JAX threefry stream cannot be reproduced).
 *   seeds [B] uint64;  out: agent [B,n,sd], goal [B,ng,sd], obst (layout as above).      */
int32_t dgppo_env_reset(const dgppo_env_cfg* cfg, const uint64_t* seeds,
                        float* agent, float* goal, float* obst, int32_t B, void* stream);
/* The same with a failure counter.  The reference's rejection loops (env/utils.py:139-244 `while_loop`s, mpe_connect_spread.py
 * :50-107) are unbounded; the kernels bound every loop so that all threads finish, and an env whose bound ran out holds an
 * INVALID scene.  *n_failed (DEVICE int32, caller-zeroed, may be NULL) is incremented once per such env; the caller reads it
 * at its next host sync and must not train on the batch when it is non-zero.  Both entry points also reject, on the host
 * and before launching, densities at which the placement cannot succeed (negative return).                              */
int32_t dgppo_env_reset_checked(const dgppo_env_cfg* cfg, const uint64_t* seeds, float* agent, float* goal, float* obst,
                                int32_t* n_failed, int32_t B, void* stream);

/* Episode start from user-given scenes: the dense env state that dgppo_env_reset writes, from S template scenes instead of
 * the sampled one.  Not in the reference, whose env_states is a Python pytree a user can fill (lidar_env/base.py:21-27); it
 * ships no way to start an episode anywhere but at reset.  Env b takes scene s = scene_ids ? scene_ids[b] : b % S.
 *   agent_t   [S, n, sd]   template rows, the record's own layout
 *   goal_t    [S, ng, sd]
 *   obst_t    LiDAR: [S, n_obs, 5] = cx, cy, w, h, theta; MPE: [S, n_obs, 2] = ox, oy; NULL iff n_obs == 0
 *   scene_ids [B] DEVICE int32 in [0, S) (the caller checks the range; the kernel trusts it), or NULL
 *   seeds     [B] uint64; NULL allowed iff jitter == 0
 *   agent, goal, obst      out, as dgppo_env_reset writes them (obst NULL iff n_obs == 0)
 *   flags     [B] out, or NULL: 0 = the scene is valid, else DGPPO_SCENE_* bits
 *   n_failed  as dgppo_env_reset_checked (caller-zeroed device int32, may be NULL)
 * Goal rows are copied word for word (a NaN keeps its payload).  A rectangle becomes the 16-float record above with
 * [5] = cosf(theta), [6] = sinf(theta) and the corner points of Rectangle.create (obstacle.py:39-56), formed exactly as the
 * reset forms them; a disc becomes [ox, oy, 0, 0].  Goals and obstacles are never jittered.
 * jitter == 0: the agent rows are copied and nothing is drawn; an invalid scene is still written, only its flags say so, and
 * *n_failed is not touched (the caller decides).
 * jitter = J > 0: the Philox stream keyed by seeds[b] as in dgppo_env_reset; attempt a = 0 .. 15 draws d = a * n + i for
 * agent i (two uniforms u0, u1: words 0, 1 of counter (d, 0, 0, 0)) and sets x = x_t + (2 u0 - 1) J, y = y_t + (2 u1 - 1) J,
 * always measured from the template; the other state columns are untouched.  The first attempt whose scene is valid is
 * kept; if none is, the last one stays, flags[b] holds its bits and *n_failed gains 1.
 * Refused on the host, before any launch: an invalid cfg, VMASReverseTransport, S < 1, B < 0, a negative or NaN jitter, NULL
 * operands (obst_t / obst must be NULL exactly when n_obs == 0; seeds may be NULL only with jitter == 0), n_agents > 64.   */
#define DGPPO_SCENE_NONFINITE 1         /* a non-finite word anywhere in the scene's template rows (goals: this test only) */
#define DGPPO_SCENE_OUT_OF_AREA 2       /* an agent with x outside [0, area_size] or y outside [0, y_limit]               */
#define DGPPO_SCENE_AGENTS_OVERLAP 4    /* a pair with sqrtf(dx*dx + dy*dy) < two_car_radius                              */
#define DGPPO_SCENE_AGENT_IN_OBSTACLE 8 /* LiDAR: Rectangle.inside at car_radius (obstacle.py:62-72); MPE: < car_plus_obs */
int32_t dgppo_env_scene_load(const dgppo_env_cfg* cfg, const float* agent_t, const float* goal_t, const float* obst_t,
                             int32_t S, const int32_t* scene_ids, const uint64_t* seeds, float jitter, float* agent,
                             float* goal, float* obst, int32_t* flags, int32_t* n_failed, int32_t B, void* stream);
/* The scene start of SOME envs of a batch whose record already holds a valid reset (training on a mix of sampled and given
 * starts).  Operands as dgppo_env_scene_load, but for
 *   scene_of   [B] DEVICE int32: < 0 = keep env b as it is, else its scene id in [0, S) (the caller checks the range)
 *   seeds      [B] uint64, never NULL
 *   agent, goal, obst      in / out: the dense record of dgppo_env_reset
 *   n_fallback DEVICE int32 [1], may be NULL
 * scene_of[b] < 0: nothing of env b is read or written, flags[b] included.
 * scene_of[b] = s: what dgppo_env_scene_load computes for (scene s, seeds[b], jitter): the same draws, expressions, 16 attempts
 * and validity bits.  Bits 0: env b's agent, goal and obstacle rows are written, word for word what dgppo_env_scene_load writes,
 * and flags[b] = 0.  Bits not 0 (a non-finite template, an invalid scene at jitter 0, no valid attempt at jitter > 0): none of
 * env b's rows is written, so the reset stands; flags[b] = the bits and *n_fallback gains 1, at jitter 0 too.
 * One wave64 per env: lane i holds agent i's candidate position in registers, the pair and obstacle tests read the other lanes
 * through __shfl, the bits are folded with __any; no LDS, no barrier.
 * Refused on the host, before any launch, with an error that names dgppo_env_scene_mix: an invalid cfg, VMASReverseTransport,
 * S < 1, B < 0, a negative or NaN jitter, NULL agent_t / goal_t / agent / goal / scene_of / seeds, obst_t / obst not NULL
 * exactly when n_obs == 0, n_agents > 64.  B == 0 returns 0.                                                               */
int32_t dgppo_env_scene_mix(const dgppo_env_cfg* cfg, const float* agent_t, const float* goal_t, const float* obst_t,
                            int32_t S, const int32_t* scene_of, const uint64_t* seeds, float jitter, float* agent,
                            float* goal, float* obst, int32_t* flags, int32_t* n_fallback, int32_t B, void* stream);
/* Failure scenes from a rollout record: for every env the first step at which its cost is unsafe, and the state `back` steps
 * before it as the template rows dgppo_env_scene_load reads.  Not in the reference.
 *   agent_tm [T+1, Bs, n, sd], cost_tm [T, Bs, n, n_cost]   the time-major record; Bs >= B is the number of envs per time
 *                                   slot of the allocation, the first B of them are mined
 *   goal [B, ng, sd], obst [B, n_obs, stride] (NULL iff n_obs == 0)   the per-env fields, dense
 *   T >= 1, back >= 0, thresh finite
 *   first [B]   the smallest t with any word of cost_tm[t, b] >= thresh (a NaN compares false), -1 if there is none
 *   who   [B]   the lowest word index i * n_cost + c that is unsafe at step first[b], or -1
 *   t0    [B]   max(first[b] - back, 0), or -1
 *   agent_t [B, n, sd] = agent_tm[t0, b], goal_t [B, ng, sd] = goal[b], word for word; obst_t [B, n_obs, 5] = words 0..4 of
 *               each rectangle record (LiDAR) or [B, n_obs, 2] = words 0, 1 of each obstacle row (MPE), NULL iff n_obs == 0
 *   flags [B]   the DGPPO_SCENE_* bits of those rows, formed with the functions of dgppo_env_scene_mix (the rectangle record
 *               rebuilt from the five words), so they are what dgppo_env_scene_load gives the mined row at jitter 0
 * Where first[b] < 0: flags[b] = 0 and none of env b's rows is written.
 * One wave64 per env; the cost scan runs in time order, several steps per pass where n * n_cost < 64, and stops at the first
 * pass with an unsafe word, so a failing env reads only up to its failure.
 * Refused on the host, before any launch, with an error that names dgppo_env_scene_mine: an invalid cfg, VMASReverseTransport,
 * B < 0, Bs < B, T < 1, back < 0, a non-finite thresh, NULL operands (obst / obst_t NULL exactly when n_obs == 0),
 * n_agents > 64, T * n * n_cost >= 2^31 - 1.  B == 0 returns 0.                                                          */
int32_t dgppo_env_scene_mine(const dgppo_env_cfg* cfg, const float* agent_tm, const float* cost_tm, int32_t Bs,
                             const float* goal, const float* obst, int32_t T, int32_t back, float thresh, int32_t* first,
                             int32_t* who, int32_t* t0, int32_t* flags, float* agent_t, float* goal_t, float* obst_t, int32_t B,
                             void* stream);
/* The mined rows of the taken envs into a ring of pool slots: a deterministic stream compaction in one workgroup.
 *   first, flags [B], agent_t, goal_t, obst_t [B, ...]   as dgppo_env_scene_mine wrote them
 *   pool_agent, pool_goal, pool_obst [M, ...]            the pool rows in the template shapes (pool_obst NULL iff n_obs == 0)
 *   M >= 1, 0 <= fixed < M     slots 0 .. fixed-1 are never written; the ring is the R = M - fixed slots after them
 *   state [4] DEVICE int32     head, filled, pushed_total, taken_last; head in [0, R) is the caller's to keep
 *   slot_of [B] out, or NULL   the slot env b went to, or -1
 * Env b is taken iff first[b] >= 1 && flags[b] == 0 (a failure at step 0 is a bad start, not a mined scene).  The taken envs
 * get ranks r = 0, 1, ... in ascending b; rank r < R is written to slot fixed + (head + r) % R word for word, later ranks are
 * dropped.  Then, with count the number of taken envs and m = min(count, R): head = (head + m) % R, filled = min(R, filled +
 * m), pushed_total += m, taken_last = count.  No atomic decides a slot: two runs give the same pool word for word.
 * Refused on the host with an error that names dgppo_env_scene_pool_push: an invalid cfg, VMASReverseTransport, B < 0, M
 * outside [1, 2^30], fixed outside [0, M), NULL operands (obst_t / pool_obst NULL exactly when n_obs == 0), n_agents > 64.
 * B == 0 is a push of nothing: taken_last = 0.                                                                            */
int32_t dgppo_env_scene_pool_push(const dgppo_env_cfg* cfg, const int32_t* first, const int32_t* flags, const float* agent_t,
                                  const float* goal_t, const float* obst_t, float* pool_agent, float* pool_goal,
                                  float* pool_obst, int32_t M, int32_t fixed, int32_t* state, int32_t* slot_of, int32_t B,
                                  void* stream);
/* ---- the pool by priority (csrc/env_scene_pool.hip): per-slot statistics, all DEVICE arrays of length M <= 65536
 *   score  float [M]   the EMA of the failed fraction of the slot's replays; 0.5 for a newly written and for a pinned slot
 *   visits int32 [M]   replays since the slot was written
 *   last   int32 [M]   the training step of the slot's last replay or write (pinned slots start at 0)
 *   state  int32 [8]   head, filled, pushed_total, taken_last (as above), evicted_last, dropped_last (the last push),
 *                      replays_last, replay_fails_last (the last score call)
 * One priority serves the draw and the push; in fp32, every operation a single IEEE operation in this order:
 *   w(s) = (4.0f * s) * (1.0f - s); a NaN or a value below 0 gives 0, a value above 1 gives 1
 *   q(s) = (uint32)(w(s) * 65535.0f) + 1, truncated: in [1, 65536]
 *
 * What the replays of a rollout did, folded into the statistics.
 *   scene_of, mix_flags [B]   the slot every env was assigned (dgppo_env_scene_pool_draw) and its bits from dgppo_env_scene_mix;
 *                             mix_flags[b] is not read where scene_of[b] < 0
 *   first [B]                 from dgppo_env_scene_mine of the same rollout
 *   tally int32 [2 M]         scratch, zero on entry and zero again on return
 *   beta in (0, 1], step
 * For slot m, r counts the envs b with scene_of[b] == m && mix_flags[b] == 0 (an env that fell back ran a sampled episode and is
 * no replay) and f those of them with first[b] >= 0.  Where r > 0: y = (float)f / (float)r, score[m] = score[m] + beta * (y -
 * score[m]), visits[m] += r, last[m] = step; where r == 0 slot m is untouched.  state[6] and state[7] receive the sums of r and f.
 * The counts are integers, summed by integer atomics (order-free); the float fold is one lane per slot.  Two launches.
 * Refused on the host with an error that names dgppo_env_scene_pool_score: an invalid cfg, VMASReverseTransport, B < 0, M outside
 * [1, 65536], beta outside (0, 1], NULL operands (the three [B] operands may be NULL at B == 0, which counts no replay).    */
int32_t dgppo_env_scene_pool_score(const dgppo_env_cfg* cfg, const int32_t* scene_of, const int32_t* mix_flags, const int32_t* first,
                                   float* score, int32_t* visits, int32_t* last, int32_t* tally, int32_t M, float beta, int32_t step,
                                   int32_t* state, int32_t B, void* stream);
/* The slot of every env of the window lo .. lo + B - 1 of a global batch of n_total envs of which n_scene are scene envs, drawn in
 * proportion to priority times staleness.
 *   scene_of [B] out   global env g = lo + b is a scene env iff (g + 1) n_scene / n_total > g n_scene / n_total (64-bit integer
 *                      division), and then has the ordinal k = g n_scene / n_total; every other env gets -1
 *   cum uint64 [M]     scratch: the inclusive prefix sums of Q
 * Slot m is live iff m < fixed or m < fixed + state[1].  Q[m] = live ? (uint64)q(score[m]) * min(1 + max(step - last[m], 0),
 * age_cap) : 0, total = sum of Q.  With total == 0 every scene env gets -1.  Otherwise scene env k takes Philox4x32-10 of counter
 * (k, step, 0, 0) and key (lo32, hi32 of draw_seed), forms u = (word0 << 32) | word1 and t = the high 64 bits of u * total, and
 * gets the smallest m whose inclusive prefix sum of Q exceeds t: a slot with Q == 0, an empty one included, is never drawn.
 * Integer arithmetic throughout.  One workgroup: the prefix sum in chunks of the block size with a carry, one binary search per env.
 * Refused on the host with an error that names dgppo_env_scene_pool_draw: an invalid cfg, VMASReverseTransport, B < 0, M outside
 * [1, 65536], fixed outside [0, M), age_cap outside [1, 1024], n_total outside [1, 2^31), n_scene outside [0, n_total], a window
 * outside the batch, NULL operands.  B == 0 returns 0.                                                                      */
int32_t dgppo_env_scene_pool_draw(const dgppo_env_cfg* cfg, const float* score, const int32_t* last, const int32_t* state, int32_t M,
                                  int32_t fixed, int32_t age_cap, int32_t step, uint64_t draw_seed, int64_t n_total, int64_t n_scene,
                                  int64_t lo, uint64_t* cum, int32_t* scene_of, int32_t B, void* stream);
/* dgppo_env_scene_pool_push with eviction by priority in place of the ring's "oldest first": the operands of that entry point, the
 * statistics, min_visits >= 0, evict_w in [0, 1], step, the [8] state and order int32 [M], scratch.
 * The taken envs and their ranks are as there.  The ranks go first to the empty ring positions filled, filled + 1, ..., then to the
 * evictable filled ring positions in ring order from head — position p < filled (slot m = fixed + p) is evictable iff visits[m] >=
 * min_visits && w(score[m]) <= evict_w, judged before anything is written — and the ranks beyond that are dropped.  A written slot
 * gets the rows word for word, score = 0.5, visits = 0, last = step.  head moves to one past the last evicted position and stays
 * when only empties were written; filled grows by the empties written; pushed_total grows by the slots written; taken_last,
 * evicted_last and dropped_last are set as named; state[6], state[7] are not touched.  One workgroup, two ballot-and-prefix
 * compactions (ring positions, envs); no atomic decides a slot: two runs give the same pool and statistics word for word.
 * Refused on the host with an error that names dgppo_env_scene_pool_push_evict: what dgppo_env_scene_pool_push refuses, M > 65536,
 * min_visits < 0, evict_w outside [0, 1], NULL statistics or order.  B == 0 is a push of nothing, and its [B] operands may be
 * NULL.                                                                                                                     */
int32_t dgppo_env_scene_pool_push_evict(const dgppo_env_cfg* cfg, const int32_t* first, const int32_t* flags, const float* agent_t,
                                        const float* goal_t, const float* obst_t, float* pool_agent, float* pool_goal,
                                        float* pool_obst, float* score, int32_t* visits, int32_t* last, int32_t* order, int32_t M,
                                        int32_t fixed, int32_t min_visits, float evict_w, int32_t step, int32_t* state,
                                        int32_t* slot_of, int32_t B, void* stream);

/* ---- VMASReverseTransport (dgppo/env/vmas/vmas_reverse_transport.py) ------------------------------------------
 * n agents (discs of radius 0.03) push a hollow 0.6 x 0.6 box of mass 10 towards a goal past 3 disc obstacles.  The record
 * differs from the other kinds, so the kind has its own entry points; dgppo_env_step / dgppo_env_reset* /
 * dgppo_graph_materialize / dgppo_graph_feats refuse it.  cfg: make_env_cfg of kind 10 (n_goals = n_obs = 0: the graph has
 * only the n agent nodes and the pad, N = n + 1, E = n * n), 1 <= n <= 16, state_dim 4, node_dim 20.
 *   agent [B, n, 4]  (x, y, vx, vy)                       a_pos | a_vel             vmas_reverse_transport.py:23-29
 *   body  [B, 4]     (x, y, vx, vy) of the box            box_pos | box_vel
 *   scene [B, 8]     goal | o0 | o1 | o2 (fixed per episode)  goal_pos | o_pos
 * Graph nodes (:251-311): [a_pos, a_vel, box_pos, box_vel, goal - box, in_contact, 3 unit vectors box->obstacle, 3
 * distances], the obstacles stably sorted by distance; graph states have zero columns (nothing is written to gout->states,
 * which may point to a 0-element buffer).                                                                              */

/* Reset (:90-128, get_node_goal_rng env/utils.py:139-244 without goals).  Philox-4x32-10 keyed by seeds[b] as
 * dgppo_env_reset; draw d gives two uniforms u0, u1 (words 0, 1 of counter (d, 0, 0, 0)):
 *   d = 0          box angle (u0, [0, 2 pi)), goal angle noise (u1, [-30, 30) degrees)
 *   d = 1, 2       obstacle angles: o0 = d1.u0, o1 = d1.u1, o2 = d2.u0 (d2.u1 unused)
 *   d = 3 .. 2+n   agent velocities: agent i = d(3+i).(u0, u1) in [-0.01, 0.01)
 *   d = 3+n ...    agent positions: one draw per candidate, rejection sampled in the 0.24 square (<= 1024 tries per
 *                  agent, <= 64 restarts), then shifted by box - 0.2.
 * Deviation: the goals that get_node_goal_rng samples next to the agents, and then discards, are not drawn.  n_failed as in
 * dgppo_env_reset_checked (caller-zeroed device int32, may be NULL).  Densities the placement cannot meet (n > 15) are
 * refused on the host.                                                                                                 */
int32_t dgppo_vmas_reset_checked(const dgppo_env_cfg* cfg, const uint64_t* seeds, float* agent, float* body, float* scene,
                                 int32_t* n_failed, int32_t B, void* stream);
/* Step (:130-249, physax/world.py:78-163, 361-474, 492-505, physax/geometry.py:8-102): clip the action to [-1, 1], agent
 * force 0.5 action, 4 world steps x 5 substeps of 0.02 with box-sphere contact forces (agents touch only the box, the box
 * does not rotate), drag 0.25 at the first substep of each world step, positions clipped to +-1.2.  reward [B] and cost
 * [B, n, 2] of the PRE-step state (:208-249); gout (optional) = the graph of the post-step state.                        */
int32_t dgppo_vmas_step(const dgppo_env_cfg* cfg, const float* agent, const float* body, const float* scene,
                        const float* action, float* next_agent, float* next_body, float* reward, float* cost,
                        const dgppo_graph_out* gout, int32_t B, void* stream);
/* GraphsTuple of a stored state (:251-311 get_graph + edge_blocks + to_padded).                                         */
int32_t dgppo_vmas_graph_materialize(const dgppo_env_cfg* cfg, const float* agent, const float* body, const float* scene,
                                     const dgppo_graph_out* gout, int32_t B, void* stream);
/* The networks' view of the same graphs (dgppo_graph_feats for this kind): Xa [G*n, Fp] node rows (20 columns, zero padded
 * to Fp >= 20), per-(agent, slot) edge features efeat [G*n, n, 4] (x_i - x_s) and masks emask [G*n, n] (0 on the self
 * slot).  Graph g = e * n_time + t reads agent + env*agent_se + t*agent_st, body + env*body_se + t*body_st and
 * scene + env*8 (env = env_ids ? env_ids[e] : e).                                                                        */
int32_t dgppo_vmas_graph_feats(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_se, int64_t agent_st,
                               const float* body, int64_t body_se, int64_t body_st, const float* scene,
                               const int32_t* env_ids, int32_t n_env, int32_t n_time, float* Xa, float* efeat, float* emask,
                               int32_t Fp, void* stream);

/* Standard-normal noise: Philox-4x32-10 + Box-Muller, out[i] for i<n_elem; replaces the
 * jax.random draw inside dist.sample(seed=key) (algo/module/policy.py:196-203).         */
int32_t dgppo_randn(uint64_t seed, uint64_t offset, float* out, int64_t n_elem, void* stream);
/* A column window of the same stream laid out as rows: out[r, c] (dense [rows, row_len]) = element r * global_row_len +
 * col_offset + c of dgppo_randn(seed, 0, ...).  Data-parallel rollouts: the sampling noise of step t is a row of
 * global_row_len = world * B_local * n * 2 normals and a rank fills the window of its envs, so that the union of the ranks'
 * rollouts is the single-device rollout of the global batch (jax.random.split(key, B) of dgppo/algo/informarl.py:254-256 is
 * likewise a function of the global env index).                                                                          */
int32_t dgppo_randn_rows(uint64_t seed, float* out, int64_t rows, int64_t row_len, int64_t global_row_len,
                         int64_t col_offset, void* stream);

/* ---- networks: building blocks ------------------------------------------------------------ */
/* All matrices row-major fp32; `ld*` = leading dimension in floats.                              */

/* Y[M,N] = act(X[M,K] W[K,N] + bias) on the fp32 matrix cores; act 0 none / 1 relu; accumulate: Y += ...;
 * trans_w: use W^T (W stored [N,K]) — the input-gradient of a Dense.  relu_mask (optional, [M,N], leading dimension ldm):
 * Y = (relu_mask > 0) ? result : 0 applied last — the backward of the ReLU whose OUTPUT relu_mask is, fused into the
 * kernel that finishes that gradient (jax.grad of nn.relu in dgppo/nn/gnn.py:39, mlp.py:29).  Replaces flax nn.Dense as
 * used by dgppo/nn/mlp.py:19-22, dgppo/nn/gnn.py:86-110, dgppo/nn/rnn.py:19-21, algo/module/policy.py:67-70, value.py:41,76. */
int32_t dgppo_dense_fwd(const float* X, int32_t ldx, const float* W, int32_t ldw, const float* bias, float* Y,
                        int32_t ldy, int32_t M, int32_t K, int32_t N, int32_t act, int32_t accumulate,
                        int32_t trans_w, const float* relu_mask, int32_t ldm, void* stream);
/* dW[K,N] += X^T dY ; db[N] += colsum(dY) (db may be NULL): the weight-gradient of a Dense
 * (jax.grad at dgppo/algo/informarl.py:377,440 ; dgppo/algo/dgppo.py:316).                          */
int32_t dgppo_dense_bwd_w(const float* X, int32_t ldx, const float* dY, int32_t ldy, float* dW, int32_t ldw,
                          float* db, int32_t M, int32_t K, int32_t N, float* workspace, int64_t workspace_bytes,
                          void* stream);
/* The MLP trunk and the GRU input projection as PPOPolicy / ValueNet compose them (dgppo/algo/module/policy.py:191-212,
 * value.py:58-80) in one launch: y1 = relu(LN(X W1 + b1)), y2 = relu(LN(y1 W2 + b2)) (MLP of dgppo/nn/mlp.py:17-29, hidden
 * 64, LayerNorm scale g / bias be, eps 1e-6), gi = y2 Wi + bi [M,192] (the input half of flax GRUCell, dgppo/nn/rnn.py:14-30,
 * gates r|z|n).  X [M, >= 64] with leading dimension ldx.  p1/y1/st1/p2/y2/st2 (pre-LN [M,64], post-ReLU [M,64], LN
 * statistics [M,2] per layer) are what the backward needs: all six or none (inference).  gi == NULL: the gate projection is
 * skipped and y2 is the result (dgppo_gi_gru1_head_fwd forms gi from it); y2 may then be given without the other five, and is
 * bit for bit the y2 of the call with gi.  That form needs 16-byte aligned X, W1, W2, Wi, y2 and ldx a multiple of 4 (refused
 * otherwise).                                                                                                      */
int32_t dgppo_mlp_gi_fwd(const float* X, int32_t ldx, const float* W1, const float* b1, const float* g1, const float* be1,
                         const float* W2, const float* b2, const float* g2, const float* be2, const float* Wi,
                         const float* bi, float* p1, float* y1, float* st1, float* p2, float* y2, float* st2, float* gi,
                         int32_t M, void* stream);
/* Backward of that chain with respect to its activations, in one launch (jax.grad through dgppo/nn/mlp.py:17-29 and the
 * GRUCell input Dense of dgppo/nn/rnn.py:14-30, as taken by dgppo/algo/informarl.py:377,440 / dgppo/algo/dgppo.py:316):
 * dpre2 = LNReLU'(p2, y2, st2, g2; dgi Wi^T), dpre1 = LNReLU'(p1, y1, st1, g1; dpre2 W2^T), dx = dpre1 W1^T, where
 * LNReLU'(p, y, st, g; dy) = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = dy (y > 0) g.  relu_mask [M, ldm] (may be
 * NULL): dx = (mask > 0) ? dx : 0.  dpre2 / dpre1 [M,64] are outputs (the weight gradients dW2 = y1^T dpre2, dW1 = X^T dpre1
 * read them); dg2/db2/dg1/db1 [64] += the LayerNorm scale / bias gradients.  M > 0 and a 16-byte aligned dgi [M,192] run
 * the rows-per-wave kernel (one 8-wave workgroup per CU); any other dgi the 16-row-tile kernel.  The choice depends on
 * nothing else and is the one dgppo_mlp_gi_bwd_w makes, on the same grid.                                           */
int32_t dgppo_mlp_gi_bwd(const float* dgi, const float* Wi, const float* W2, const float* W1, const float* g2,
                         const float* g1, const float* p2, const float* y2, const float* st2, const float* p1,
                         const float* y1, const float* st1, const float* relu_mask, int32_t ldm, float* dpre2, float* dpre1,
                         float* dx, int32_t lddx, float* dg2, float* db2, float* dg1, float* db1, int32_t M, void* stream);
/* The same weight gradient with its second stage DEFERRED: only the partial-slab kernel is launched; *pending describes the
 * reduction that is still owed (pending->pending = 0 when the call needed none).  The caller owns the descriptors and the
 * workspace REGION of every deferred call until it has flushed them with dgppo_dense_bwd_w_reduce_batch (one launch per
 * DGPPO_REDUCE_BATCH reductions, on the same stream).  A backward pass has ~12 weight gradients.                    */
#define DGPPO_REDUCE_BATCH 16
typedef struct dgppo_reduce_desc {
  const float* part;     /* partial slabs [slabs][part_stride] inside the caller's workspace region */
  float* dW;             /* [K, N] with leading dimension ldw: dW += sum of the slabs               */
  float* db;             /* [N] or NULL                                                              */
  int32_t part_stride, slabs, ldw, K, N;
  int32_t pending;       /* 1: this reduction is owed                                                */
} dgppo_reduce_desc;
int32_t dgppo_dense_bwd_w_deferred(const float* X, int32_t ldx, const float* dY, int32_t ldy, float* dW, int32_t ldw,
                                   float* db, int32_t M, int32_t K, int32_t N, float* workspace, int64_t workspace_bytes,
                                   dgppo_reduce_desc* pending, void* stream);
int32_t dgppo_dense_bwd_w_reduce_batch(const dgppo_reduce_desc* descs, int32_t n, void* stream);
/* Both gradients of one Dense Y = X W from one call: dW [K, lddw] += X^T dY, db [N] += colsum(dY) (db may be NULL) as
 * dgppo_dense_bwd_w, and the input gradient dX [M, lddx] = dY W^T (W [K, ldw]: the parameters), or with accumulate_mask != 0
 * dX = (X > 0) ? dX + dY W^T : 0 - dgppo_dense_fwd's accumulate + relu_mask epilogue with X itself as the mask (the Dense's input
 * is a ReLU output).  For the GNN glue shapes (K, N) in {(144, 64), (48, 32), (48, 64)} with X, dY, W, dX 16-byte
 * aligned and ldx, ldy, ldw, lddx multiples of 4 this is ONE launch that brings X in once and dY twice (once for the tile of
 * the weight gradient and once more in the operand layout of the input gradient: a cache hit by the measured fetch
 * counters, profiles/README.md round 7); every other call runs
 * dgppo_dense_bwd_w followed by dgppo_dense_fwd(trans_w) and gives their results.  The choice depends on nothing else.  The one
 * pass sums dX over n in a different order than dgppo_dense_fwd (agreement to fp32 rounding of a reordered sum of N terms).
 * dX must not overlap X, dY or W.  workspace as dgppo_dense_bwd_w; pending NULL reduces the slabs now, otherwise *pending
 * receives the owed reduction under the rules of dgppo_dense_bwd_w_deferred.                                                 */
int32_t dgppo_dense_bwd_xw(const float* X, int32_t ldx, const float* dY, int32_t ldy, const float* W, int32_t ldw, float* dX,
                           int32_t lddx, int32_t accumulate_mask, float* dW, int32_t lddw, float* db, int32_t M, int32_t K,
                           int32_t N, float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream);
/* dgppo_mlp_gi_bwd together with the weight gradients of the chain's two Dense layers, from the same pass over the rows:
 * dW2 [64, ldw2] += y1^T dpre2, dbias2 [64] += colsum(dpre2), dW1 [64, ldw1] += x^T dpre1, dbias1 [64] += colsum(dpre1), where
 * x [M, ldx] is the chain's input (it may be the relu_mask tensor itself).  dpre2 / dpre1 may be NULL: then they never leave
 * the CU.  dx (and dpre* where given) are bit for bit those of dgppo_mlp_gi_bwd; dg* / db* are the same sums, but both
 * entry points add per-workgroup partial sums with atomicAdd in arrival order (and, with a dgi that is not 16-byte aligned,
 * this one may split the rows over fewer workgroups), so from three workgroups on they agree only to the rounding of a
 * reordered fp32 sum.  Rows >= M of a ragged tile contribute exactly zero.  workspace:
 * dgppo_mlp_gi_bwd_w_workspace_bytes() bytes for one partial slab [dW2 | dbias2 | dW1 | dbias1] per workgroup (one per
 * CU); without room for a slab per workgroup (or NULL) the call adds atomically: correct, but slow at many rows.  Up to 4
 * workgroups (M <= 512) always add atomically.
 * pending == NULL: the slabs are reduced at once.  Otherwise pending[0..1] receive the two owed reductions (pending = 0 where
 * none is owed) for dgppo_dense_bwd_w_reduce_batch, under the rules of dgppo_dense_bwd_w_deferred.  M == 0 touches nothing. */
int64_t dgppo_mlp_gi_bwd_w_workspace_bytes(void);
int32_t dgppo_mlp_gi_bwd_w(const float* dgi, const float* Wi, const float* W2, const float* W1, const float* g2,
                           const float* g1, const float* p2, const float* y2, const float* st2, const float* p1,
                           const float* y1, const float* st1, const float* x, int32_t ldx, const float* relu_mask,
                           int32_t ldm, float* dpre2, float* dpre1, float* dx, int32_t lddx, float* dg2, float* db2,
                           float* dg1, float* db1, float* dW2, int32_t ldw2, float* dbias2, float* dW1, int32_t ldw1,
                           float* dbias1, int32_t M, float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending,
                           void* stream);
/* Backward of the output head in one pass over the rows (jax.grad through PolicyNet.head Dense -> TanhNormal Dense,
 * dgppo/algo/module/policy.py:62-74, or the value Dense, dgppo/algo/module/value.py:41,76).  Two layers (W2 != NULL; the shapes
 * of dgppo_gru1_head_fwd: W1 [64,64], W2 [64,n_out]): dW2 [64, ldw2] += u^T dout, db2 [n_out] += colsum(dout), du = dout W2^T
 * (kept on the CU), dW1 [64, ldw1] += feat^T du, db1 [64] += colsum(du), dhs [M,64] = du W1^T.  One layer (W2 = u = dW2 = db2 =
 * NULL, W1 [64,n_out]): dW1 [64, ldw1] += feat^T dout, db1 [n_out] += colsum(dout), dhs = dout W1^T.  feat [M, ldf >= 64],
 * u [M,64], dout [M,n_out], n_out <= 16; feat, u, dout, dhs 16-byte aligned and ldf a multiple of 4, else the call is refused.
 * workspace / pending: as dgppo_mlp_gi_bwd_w (dgppo_head_bwd_workspace_bytes(); pending[0..1], the second only for two layers). */
int64_t dgppo_head_bwd_workspace_bytes(void);
int32_t dgppo_head_bwd(const float* feat, int32_t ldf, const float* u, const float* dout, const float* W1, const float* W2,
                       float* dhs, float* dW1, int32_t ldw1, float* db1, float* dW2, int32_t ldw2, float* db2, int32_t M,
                       int32_t n_out, float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream);
/* One GRU step (T = 1) fused with the output Dense layer(s) on the same rows — the tail of a rollout step:
 * h' = GRUCell(gi, h0) (dgppo/nn/rnn.py:14-30, gi = x W_i + b_i from dgppo_mlp_gi_fwd), then either the policy head
 * u = h' W1 + b1 [64], out = u W2 + b2 (PolicyNet.head Dense -> TanhNormal Dense, dgppo/algo/module/policy.py:62-74; pass
 * W2/b2) or a value head out = h' W1 + b1 (dgppo/algo/module/value.py:41,76; W2 = b2 = NULL).  n_out <= 16.  hprev [M,64],
 * gates [M,256] (r|z|n|hn_lin) and u [M,64] are the activations the backward needs (each may be NULL).       */
int32_t dgppo_gru1_head_fwd(const float* gi, const float* Wh, const float* bhn, const float* h0, const float* W1,
                            const float* b1, const float* W2, const float* b2, float* hs, float* hprev, float* gates,
                            float* u, float* out, int32_t M, int32_t n_out, void* stream);
/* The tail of a value net's one-step (T = 1) pass from the trunk's output, in one launch: gi = y2 Wi + bi (the input half of
 * flax GRUCell, dgppo/nn/rnn.py:14-30; it stays on the CU), h' = GRUCell(gi, h0), out [M, ldo >= n_out] = h' W1 + b1 (the value
 * Dense, dgppo/algo/module/value.py:41,76; n_out <= 16).  y2 [M,64] is what dgppo_mlp_gi_fwd writes with gi == NULL.  hs [M,64]
 * (h') and gates [M,256] (r|z|n|hn_lin) are written where given: they are bit for bit those of dgppo_mlp_gi_fwd (with gi) +
 * dgppo_gru_fwd at T = 1 with hprev = h0; out sums over k in another order than dgppo_dense_fwd (fp32 rounding of a reordered
 * 64-term sum).  h0 by h0_form:
 *   DGPPO_H0_DENSE   h0 [M,64], or NULL for zeros;
 *   DGPPO_H0_BLOCKS  row m at h0 + (m / h0_rows_per_block) * h0_block_stride + (m % h0_rows_per_block) * 64 (dgppo_gru_fwd_h0_blocks);
 *   DGPPO_H0_MAP     row m through the map of dgppo_gru_fwd_h0_map (ids, n_env, n_time, n_inner, env_stride, time_stride).
 * The arguments of the other forms are ignored.  y2, Wi, Wh, h0 and hs must be 16-byte aligned and the strides multiples of 4
 * floats, otherwise the call is refused (the three separate launches serve such operands).  Rows >= M are neither read into a
 * result nor written.                                                                                                        */
#define DGPPO_H0_DENSE 0
#define DGPPO_H0_BLOCKS 1
#define DGPPO_H0_MAP 2
int32_t dgppo_gi_gru1_head_fwd(const float* y2, const float* Wi, const float* bi, const float* Wh, const float* bhn,
                               const float* W1, const float* b1, const float* h0, int32_t h0_form, int32_t h0_rows_per_block,
                               int64_t h0_block_stride, const int32_t* ids, int32_t n_env, int32_t n_time, int32_t n_inner,
                               int64_t env_stride, int64_t time_stride, float* out, int32_t ldo, float* hs, float* gates,
                               int32_t M, int32_t n_out, void* stream);
/* Scratch for dgppo_dense_bwd_w's two-stage reduction (per-workgroup partial sums, then one reduce kernel): the caller
 * owns it, like every other buffer (16-byte aligned device memory, reusable by consecutive calls on one stream).  The
 * returned size lets every workgroup keep its own slab (the MFMA kernels write one per CU, the narrow-K kernel up to
 * 1024); a smaller buffer shrinks the grid, NULL / 0 falls back to atomicAdd into dW (correct, slower).  No reference counterpart (XLA owns its scratch allocations).      */
int64_t dgppo_dense_bwd_w_workspace_bytes(int32_t K, int32_t N);

/* Row gather shared by up to DGPPO_GATHER_MAX tensors: dst_k[e] = src_k[ids[e]] for e < n_ids, every k in ONE launch (the
 * minibatch prelude: torch.index_select along dim 0 of each tensor).  Row ids[e] of tensor k starts at
 * src + ids[e] * src_stride (bytes; a view along dim 1 has src_stride > row_bytes); dst rows are dense.  row_bytes and
 * src_stride are multiples of 4 (refused otherwise); 16-byte accesses when both, and both pointers, are multiples of 16,
 * dwords otherwise.  descs is a HOST array.  ids are not range-checked.                                            */
#define DGPPO_GATHER_MAX 8
typedef struct dgppo_gather_desc {
  const void* src;
  void* dst;
  int64_t row_bytes, src_stride;
} dgppo_gather_desc;
int32_t dgppo_gather_rows(const dgppo_gather_desc* descs, int32_t n_desc, const int32_t* ids, int32_t n_ids, void* stream);

/* Compact record -> per-graph dense features for the GNN: agent node rows Xa [G*n,Fp], other node rows
 * Xo [G*(Ns-n),Fp], per-(agent,slot) edge features [G*n,S,4] and masks [G*n,S] (1/0).  Graph g = e*n_time + t reads
 * agent + env*agent_se + t*agent_st (env = env_ids ? env_ids[e] : e), likewise hits.  Same arithmetic as
 * get_graph/edge_blocks (lidar_env/base.py:227-271, lidar_spread.py:57-96, lidar_target.py:57-96, mpe twins).         */
int32_t dgppo_graph_feats(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_se, int64_t agent_st,
                          const float* goal, const float* obst, const float* hits, int64_t hits_se, int64_t hits_st,
                          const int32_t* env_ids, int32_t n_env, int32_t n_time, float* Xa, float* Xo, float* efeat,
                          float* emask, int32_t Fp, void* stream);

/* The same features for a Vh landscape: frame f (fid = frame_ids ? frame_ids[f] : f, read at agent + fid*agent_st and
 * hits + fid*hits_st) of ONE environment, with agent `agent_id` moved to every point of the grid xs [nx] x ys [ny].  Graph
 * g = (f*ny + iy)*nx + ix holds that agent at (xs[ix], ys[iy]) with its velocity (bicycle: heading and speed) kept; in the
 * LiDAR kinds its k hit points are cast again from there against this env's rectangles (get_lidar, env/utils.py:115-136,
 * lidar_env/base.py:126-140: start-inside factor, det == 0 NaN rays, stable top-k) while the other agents keep the recorded
 * ones; every output has dgppo_graph_feats' layout and arithmetic (get_graph, lidar_env/base.py:227-271) for the
 * G = n_frames*ny*nx graphs.  hits_out [G, k, 2] (may be NULL) receives the moved agent's hits.  goal / obst are this
 * env's rows (obst: LiDAR [n_obs,16] rectangles, MPE [n_obs, sd]).  This is the producer of the arrays the reference's
 * renderer draws as viz_opts["cbf"] (dgppo/env/plot.py:348-372,437-447); the reference ships none.                      */
int32_t dgppo_graph_feats_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                const float* obst, const float* hits, int64_t hits_st, const float* ray_cos,
                                const float* ray_sin, const int32_t* frame_ids, int32_t n_frames, int32_t agent_id,
                                const float* xs, int32_t nx, const float* ys, int32_t ny, float* Xa, float* Xo,
                                float* efeat, float* emask, float* hits_out, int32_t Fp, void* stream);

/* The environment's own cost over the same sweep: cost [G, n, n_cost] = get_cost (lidar_env/base.py:180-207,
 * mpe/base.py:164-191, mpe_connect_spread.py:115-134) of ALL n agents in graph g = (f*ny + iy)*nx + ix, i.e. frame fid of ONE
 * environment with agent `agent_id` at (xs[ix], ys[iy]).  Operands as in dgppo_graph_feats_sweep (no goals are needed): in the
 * LiDAR kinds the moved agent's k hits are cast again from the new position, every other agent's are the recorded ones; the
 * MPE kinds use the disc obstacles.  Margins 2r - min_j d_ij (1e6 on the diagonal), r - min hit distance / r + obs_r - min disc
 * distance (exactly 0 when n_obs == 0) and, for n_cost == 3, the NaN-propagating largest nearest-neighbour distance minus
 * connect_radius; then -/+ 0.5 and the clip (both sides for the LiDAR kinds and MPEConnectSpread, from below otherwise).  A NaN
 * stays a NaN.  hits_out [G, k, 2] (may be NULL) receives the moved agent's hits.  This is the ground truth the learned Vh of
 * the landscape is supposed to bound (Vh >= h); the reference ships no producer for either.                               */
int32_t dgppo_cost_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* obst, const float* hits,
                         int64_t hits_st, const float* ray_cos, const float* ray_sin, const int32_t* frame_ids,
                         int32_t n_frames, int32_t agent_id, const float* xs, int32_t nx, const float* ys, int32_t ny,
                         float* cost, float* hits_out, void* stream);

/* The features behind the discrete control barrier condition (dgppo/algo/dgppo.py:246-250: cbf_deriv = (Vh(graph[t+1]) -
 * Vh(graph[t])) / dt + alpha * Vh(graph[t])) with ONE agent's action swept: graph g = (f*nv + iv)*nu + iu is the graph of frame
 * fid + 1 (fid = frame_ids ? frame_ids[f] : f) of ONE environment in which row `agent_id` is agent_step_euler(row agent_id of
 * frame fid, clip_action((us[iu], vs[iv]))) (env/base.py:84-86, lidar_env/base.py:146-149, lidar_bicycle_target.py:95-107; the
 * step kernels' own arithmetic, y_limit included) and every other agent keeps its recorded next state.  The next position does
 * not depend on the action, so nothing is cast: hits (LiDAR kinds with obstacles; NULL otherwise) are the recorded ones of
 * frame fid + 1, read at hits + (fid+1)*hits_st; agent is read at agent + fid*agent_st (the row) and + (fid+1)*agent_st (the
 * frame), so fid + 1 must lie inside the record.  goal / obst are this env's rows; obst is read by the MPE kinds only
 * ([n_obs, sd] discs; may be NULL for a LiDAR kind).  Outputs: dgppo_graph_feats' layout and arithmetic (get_graph,
 * lidar_env/base.py:227-271) for the G = n_frames*nv*nu graphs.  The reference ships no producer for this.                   */
int32_t dgppo_graph_feats_action_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                       const float* obst, const float* hits, int64_t hits_st, const int32_t* frame_ids,
                                       int32_t n_frames, int32_t agent_id, const float* us, int32_t nu, const float* vs,
                                       int32_t nv, float* Xa, float* Xo, float* efeat, float* emask, int32_t Fp, void* stream);

/* The same what-if graphs for a barrier shield, for EVERY agent of n_env environments in one launch: graph
 * g = (e*n + i)*P + p, P = 1 + nv*nu, is the graph of next_agent[e] (the state after a provisional step) in which row i is
 * agent_step_euler(row i of agent[e], clip_action(candidate p)) (env/base.py:84-86, lidar_env/base.py:146-149,
 * lidar_bicycle_target.py:95-107) and every other agent keeps its provisional next state; candidate 0 is a_pol[e, i], candidate
 * 1 + iv*nu + iu is (us[iu], vs[iv]).  All operands are dense: agent / next_agent [n_env, n, sd], goal [n_env, n_goals, sd],
 * obst [n_env, n_obs, sd] (MPE discs; may be NULL for a LiDAR kind), next_hits [n_env, n, k, 2] (LiDAR kinds with obstacles; NULL
 * otherwise: nothing is cast, the next position does not depend on the action), a_pol [n_env, n, 2].  Outputs:
 * dgppo_graph_feats' layout and arithmetic (get_graph, lidar_env/base.py:227-271) for the G = n_env*n*P graphs — what the
 * constraint-value net reads to evaluate cbf_deriv (dgppo/algo/dgppo.py:246-250) per agent and candidate.  nu, nv >= 1.    */
int32_t dgppo_graph_feats_team_action_sweep(const dgppo_env_cfg* cfg, const float* agent, const float* next_agent,
                                            const float* goal, const float* obst, const float* next_hits, const float* a_pol,
                                            int32_t n_env, const float* us, int32_t nu, const float* vs, int32_t nv, float* Xa,
                                            float* Xo, float* efeat, float* emask, int32_t Fp, void* stream);

/* The shield's choice among those candidates, per (env e, agent i) on the agent's own row: h[e, i, p] = max_c ((Vh_next[e, i, p,
 * i, c] - Vh_t[e, i, c]) / dt + alpha * Vh_t[e, i, c]), the left-hand side of the barrier condition dgppo/algo/dgppo.py:246-250
 * (NaN-propagating max).  Vh_next [n_env, n, P, n, n_cost], Vh_t [n_env, n, n_cost], a_pol [n_env, n, 2].  A candidate is
 * admissible iff h <= -margin (never a NaN).  Candidate 0 is kept if admissible (flag 0); else the admissible candidate nearest
 * to it — du*du + dv*dv in fp32 on clipped actions, lowest index on ties (flag 1); else the smallest h, lowest index on ties,
 * NaN skipped, candidate 0 when every h is NaN (flag 2).  action [n_env, n, 2] is the chosen candidate clipped to [-1, 1],
 * index / flag [n_env, n] int32, h [n_env, n, P] (may be NULL).  The reference ships no runtime filter.                     */
int32_t dgppo_shield_select(const float* Vh_next, const float* Vh_t, const float* a_pol, int32_t n_env, int32_t n_agents,
                            int32_t n_cost, const float* us, int32_t nu, const float* vs, int32_t nv, float dt, float alpha,
                            float margin, float* action, int32_t* index, int32_t* flag, float* h, void* stream);

/* The what-if environments of the sweep above as a dense env state the step kernels run on, for a policy rollout FROM every
 * swept position: Vh is fitted to the discounted-to-max constraint return of the policy's own future (compute_dec_ocp_gae,
 * dgppo/algo/utils.py:38-45), which the instantaneous cost of dgppo_cost_sweep does not give.  Env g = (f*ny + iy)*nx + ix, G =
 * n_frames*ny*nx, is frame fid (fid = frame_ids ? frame_ids[f] : f; operands as in dgppo_graph_feats_sweep) of ONE environment:
 *   agent_out [G, n, sd]            frame fid's rows; columns 0, 1 of row agent_id become (xs[ix], ys[iy]), every other column
 *                                   (velocity; the bicycle's heading and speed, lidar_bicycle_target.py:95-107) is kept;
 *   goal_out  [G, n_goals, sd], obst_out [G, n_obs, 16 | sd]   copies: the step kernels index per-env fields by env;
 *   hits_out  [G, n, k, 2]          (LiDAR kinds with obstacles; otherwise not written, may be NULL) the recorded hits, row
 *                                   agent_id cast again from the new position (get_lidar, env/utils.py:115-136,
 *                                   lidar_env/base.py:126-140: start-inside factor, det == 0 NaN rays, stable top-k);
 *   carry_out [G*n, HC]             frame fid's rows of carry, read at carry + fid*carry_st ([n, HC] rows, the actor's packed
 *                                   carry), the same for every grid point of the frame; carry may be NULL: nothing is written.
 * The reference ships no way to start an episode anywhere but at reset (env/base.py reset).                                   */
int32_t dgppo_env_sweep_fork(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                             const float* obst, const float* hits, int64_t hits_st, const float* ray_cos, const float* ray_sin,
                             const int32_t* frame_ids, int32_t n_frames, int32_t agent_id, const float* xs, int32_t nx,
                             const float* ys, int32_t ny, const float* carry, int64_t carry_st, int32_t HC, float* agent_out,
                             float* goal_out, float* obst_out, float* hits_out, float* carry_out, void* stream);

/* The costs of a K-step rollout, cost [K, G, n, nh] time-major with step stride cost_st (floats), folded into what Vh is
 * trained on: compute_dec_ocp_gae's Vhs_row recursion (dgppo/algo/utils.py:38-45, discount_to_max=True) at gae_lambda = 1.  Per
 * (g, agent): V = h[K-1]; for k = K-2 .. 0: m = max_c h[k][c], V[c] = max(h[k][c], one_minus_gamma*m + gamma*V[c]) (one multiply,
 * one multiply and one add, in that order).  value [G, n, nh] = V, worst [G, n, nh] = max_k h[k][c].  Every max propagates NaN
 * (jnp.maximum / jnp.max).  Unlike the reference, which bootstraps with Vh of the state after the last step, the row starts
 * from the last cost itself: the net under test stays out of its own ground truth.  K >= 1, 1 <= nh <= 3.                    */
int32_t dgppo_constraint_return(const float* cost, int64_t cost_st, int32_t K, int32_t G, int32_t n_agents, int32_t nh,
                                float gamma, float one_minus_gamma, float* value, float* worst, void* stream);

/* The what-if environments of ONE step of a lookahead shield, as a dense env state the step kernels run on: env
 * g = (e*n + i)*P + p, P = 1 + nv*nu, G = n_env*n*P, is a copy of env e in which agent i is about to play candidate p and
 * everyone else the policy's action; candidate 0 is a_pol[e, i], candidate 1 + iv*nu + iu is (us[iu], vs[iv]) — the numbering
 * of dgppo_shield_select.  All operands are dense: agent [n_env, n, sd], goal [n_env, n_goals, sd], obst [n_env, n_obs, 16 | sd]
 * (NULL without obstacles), hits [n_env, n, k, 2] (LiDAR kinds with obstacles; NULL for every other kind, as is hits_out),
 * a_pol [n_env, n, 2], carry [n_env*n, HC] (the actor's packed carry after the step; NULL: carry_out is not written).  Outputs:
 * the same fields for the G envs, every one a copy of env e's rows, and action_out [G, n, 2]: row i of env g is candidate p,
 * every other row a_pol[e]'s.  Nothing is computed: words are copied as they are (a NaN keeps its payload) and the action is
 * NOT clipped — the step that applies it clips (clip_action, env/base.py; the step itself: env/base.py step,
 * lidar_env/base.py:146-149).  nu, nv >= 1, nu*nv < 2^24, G*n < 2^31.  The reference ships no runtime filter and no way to
 * start an episode anywhere but at reset.                                                                                     */
int32_t dgppo_env_team_action_fork(const dgppo_env_cfg* cfg, const float* agent, const float* goal, const float* obst,
                                   const float* hits, const float* a_pol, const float* carry, int32_t HC, int32_t n_env,
                                   const float* us, int32_t nu, const float* vs, int32_t nv, float* agent_out, float* goal_out,
                                   float* obst_out, float* hits_out, float* action_out, float* carry_out, void* stream);

/* The lookahead shield's choice among those candidates, per (env e, agent i) on the agent's own row of its own what-if env:
 * s[e, i, p] = max over k in [0, K) and c in [0, n_cost) of cost[k*cost_st + ((g*n + i)*n_cost + c)], g = (e*n + i)*P + p — the
 * worst cost (get_cost, lidar_env/base.py:203-205) the agent meets in the K states after the candidate's step, the others
 * playing the policy (NaN-propagating max).  cost points at step 1 of the rolled record, cost_st >= G*n*n_cost is its step
 * stride in floats.  A candidate is admissible iff s <= -margin (never a NaN).  Candidate 0 is kept if admissible (flag 0); else
 * the admissible candidate nearest to it — du*du + dv*dv in fp32 on clipped actions (clip_action, env/base.py), lowest index on
 * ties (flag 1); else the smallest s, lowest index on ties, NaN skipped, candidate 0 when every s is NaN (flag 2).  action
 * [n_env, n, 2] is the chosen candidate clipped to [-1, 1], index / flag [n_env, n] int32, s [n_env, n, P] (may be NULL).
 * K >= 1, 1 <= n_cost <= 3, margin no NaN.  The reference ships no runtime filter.                                            */
int32_t dgppo_lookahead_select(const float* cost, int64_t cost_st, int32_t K, int32_t n_env, int32_t n_agents, int32_t n_cost,
                               const float* a_pol, const float* us, int32_t nu, const float* vs, int32_t nv, float margin,
                               float* action, int32_t* index, int32_t* flag, float* s, void* stream);

/* dgppo_env_team_action_fork for a later round of the lookahead shield (Engine.lookahead_select_rounds): only the envs
 * env_ids[0 .. n_ids) are forked, and the joint action the candidates are set into is the one HELD after the rounds so far.
 * Output env g = (m*n + i)*P + p, G = n_ids*n*P, is a copy of env e = env_ids[m]; its joint action is a_base[e] with row i
 * replaced by candidate p for p > 0 — candidate 0 is a_base[e, i] itself — and its carry rows are env e's.  The sources stay
 * dense over all n_env envs (operands as above, a_base [n_env, n, 2] in the place of a_pol); env_ids == NULL is the identity
 * and needs n_ids == n_env, which makes the call dgppo_env_team_action_fork's, word for word.  The caller guarantees
 * 0 <= env_ids[m] < n_env (the binding checks it).  Words are copied as they are, nothing is clipped: the step clips
 * (clip_action, env/base.py).  Same device code, same refusals.  The reference ships no runtime filter.                      */
int32_t dgppo_env_team_action_fork_ids(const dgppo_env_cfg* cfg, const float* agent, const float* goal, const float* obst,
                                       const float* hits, const float* a_base, const float* carry, int32_t HC, int32_t n_env,
                                       const int32_t* env_ids, int32_t n_ids, const float* us, int32_t nu, const float* vs,
                                       int32_t nv, float* agent_out, float* goal_out, float* obst_out, float* hits_out,
                                       float* action_out, float* carry_out, void* stream);

/* The selection of one round of the lookahead shield's rounds, on the what-if envs of dgppo_env_team_action_fork_ids.  Per listed
 * env e = env_ids[m] (NULL: e = m) and agent i, s[p] is dgppo_lookahead_select's fold (the worst own-row cost, get_cost,
 * lidar_env/base.py:203-205, NaN-propagating) on what-if env (m*n + i)*P + p.  Candidate 0 is clip(action[e, i]), the action the
 * agent holds (clip_action, env/base.py).  Pick: 0 if s[0] <= -margin; else the admissible candidate nearest to clip(a_ref[e, i]),
 * the policy's action (du*du + dv*dv in fp32, a NaN distance counts as +inf, lowest index on ties); else the smallest s (lowest
 * index on ties, NaN skipped, 0 if every s is NaN).  Commit: mode 0 — every agent commits its pick; mode 1 — only the
 * lowest-numbered agent whose pick is not 0 commits, everyone else keeps candidate 0.  A committing agent with pick > 0 writes the
 * clipped candidate to action [n_env, n, 2] and the pick to index [n_env, n]; an agent that keeps candidate 0 writes
 * clip(action[e, i]) back and leaves index as it was, so index is the grid number of what is held (0: the policy's action).
 * flag [n_env, n] describes the action now held: 2 if its s is not admissible, else 0 if index == 0, else 1.  changed[e] = 1 iff
 * some agent committed a pick > 0, else 0.  joint[e] = 0 when changed (the held joint action was not rolled), 1 when unchanged and
 * some s[.., 0] is not admissible (rolled, not safe, nothing better), 2 when unchanged and all are (rolled and admissible for
 * every agent).  s [n_env, n, P] may be NULL.  Rows of envs that are not listed are not touched; env_ids must not repeat an env.
 * One workgroup per env settles the team after one barrier: the result does not depend on scheduling.  K >= 1,
 * 1 <= n_cost <= 3, n_agents <= 4096, margin no NaN, mode in {0, 1}.  The reference ships no runtime filter.                  */
int32_t dgppo_lookahead_reselect(const float* cost, int64_t cost_st, int32_t K, int32_t n_ids, int32_t n_agents, int32_t n_cost,
                                 const int32_t* env_ids, const float* a_ref, const float* us, int32_t nu, const float* vs,
                                 int32_t nv, float margin, int32_t mode, float* action, int32_t* index, int32_t* flag, float* s,
                                 int32_t* joint, int32_t* changed, void* stream);

/* The what-if environments of an action rollout landscape: ONE agent's action swept in recorded frames, as a dense env state the
 * step kernels run on.  Env g = (f*nv + iv)*nu + iu, G = n_frames*nv*nu (the numbering of dgppo_graph_feats_action_sweep), is a
 * copy of frame fid (fid = frame_ids ? frame_ids[f] : f; operands and frame strides as in dgppo_env_sweep_fork) of ONE
 * environment in which agent `agent_id` is about to play (us[iu], vs[iv]) and everyone else their recorded action of that step:
 *   agent_out  [G, n, sd]            frame fid's rows, unchanged;
 *   goal_out   [G, n_goals, sd], obst_out [G, n_obs, 16 | sd]   this env's rows (obst NULL without obstacles);
 *   hits_out   [G, n, k, 2]          the recorded hits of frame fid, read at hits + fid*hits_st: no position changes before the
 *                                    step, so nothing is cast (LiDAR kinds with obstacles; hits and hits_out are NULL otherwise);
 *   action_out [G, n, 2]             row agent_id is (us[iu], vs[iv]); every other row is a copy of action + fid*action_st, laid
 *                                    out [n, 2];
 *   carry_out  [G*n, HC]             the rows at carry + fid*carry_st ([n, HC], the actor's packed carry): the caller passes the
 *                                    carries AFTER each frame's policy forward, which do not depend on the action taken.  carry
 *                                    may be NULL: nothing is written.
 * Nothing is computed: words are copied as they are (a NaN keeps its payload) and the action is NOT clipped — the step that
 * applies it clips (clip_action, env/base.py; the step itself: env/base.py step, lidar_env/base.py:146-149).  nu, nv >= 1, nu*nv
 * < 2^24, n_frames >= 1, G*n < 2^31; every frame stride is at least its row block.  The reference ships no way to start an
 * episode anywhere but at reset.                                                                                               */
int32_t dgppo_env_action_sweep_fork(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                    const float* obst, const float* hits, int64_t hits_st, const float* action, int64_t action_st,
                                    const float* carry, int64_t carry_st, int32_t HC, const int32_t* frame_ids, int32_t n_frames,
                                    int32_t agent_id, const float* us, int32_t nu, const float* vs, int32_t nv, float* agent_out,
                                    float* goal_out, float* obst_out, float* hits_out, float* action_out, float* carry_out,
                                    void* stream);

/* GraphTransformer attention in fixed-fan-in form (dgppo/nn/gnn.py:85-117; jraph.segment_softmax/segment_sum):
 * qt [G*n,H*F] = x_i Mcat + cvec (a Dense), logits = qt . x_sender, masked softmax over the S slots of each agent,
 * zcat [G*n,Kp] = [x_i | per head: sum a x_s (F), sum a e (4) | 1 | 0...], attn [G*n,S,H] saved for backward (NULL in
 * inference: the weights are not written).  Any team size dgppo_validate_cfg admits (n <= 64): graphs whose whole image
 * does not fit 64 KB of LDS are walked in receiver tiles (F % 4 == 0, 8 <= F <= 64 there).  Bit-reproducible run to run.
 * An agent without any unmasked slot receives nothing (aggr = 0, gnn.py:109-111): its attention weights are 0, its aggregates
 * are 0 and its constant column is 0 instead of 1, so that the value bias does not reach it either.  In topologies with goal
 * slots the caller must leave at least the goal slots of every agent unmasked (the environments never mask them): the
 * constant column is then written as 1 without looking at the masks.                                                      */
int32_t dgppo_attn_fwd(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt, const float* Xa,
                       const float* Xo, const float* efeat, const float* emask, float* zcat, float* attn, int32_t G,
                       void* stream);
/* backward of the above: dqt [G*n,H*F]; dXa [G*n,F] / dXo [G*(Ns-n),F] written (not accumulated) when non-NULL.
 * relu_xo != 0: dXo *= (Xo > 0) — Xo is then the ReLU output of the previous layer's node update, and its gradient
 * needs no separate pass (dXa still receives the dqt Mcat^T term from dgppo_dense_fwd, which applies the mask).        */
int32_t dgppo_attn_bwd(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                       const float* attn, const float* qt, const float* Xa, const float* Xo, const float* efeat,
                       float* dqt, float* dXa, float* dXo, int32_t relu_xo, int32_t G, void* stream);
/* The first layer (F = 8) without the operands its kernels can form themselves.  On the kinds with a 4-float state the node
 * rows carry the state in columns 0..3 and dgppo_graph_feats / dgppo_env_act_step_feats write efeat[i, s] as the single rounded
 * difference of those columns of the receiver's and the sender's row (columns 2, 3 are 0 on a LiDAR hit slot), so:
 * dgppo_attn_fwd_rows = dgppo_attn_fwd without efeat, bit for bit the same zcat / attn when efeat holds those differences;
 * dgppo_attn_bwd_rows = dgppo_attn_bwd of the first layer (dqt only) without efeat, and with attn == NULL also without the saved
 * weights, which it forms again from qt and emask with the forward's arithmetic (same bits; qt and emask may be NULL otherwise).
 * Only the features of those two producers satisfy the identity: a caller with its own efeat uses dgppo_attn_fwd / _bwd.
 * dgppo_attn_rows_supported: 1 for the slot-sparse kernels (F = 8, H = 3, n <= 32, S <= 64, whole graph within 64 KB) on a kind
 * with a 4-float state — not the bicycle kinds, not VMASReverseTransport — else 0; the two entry points then return an error
 * and launch nothing (so does a Kp that is no multiple of 4).                                                              */
int32_t dgppo_attn_rows_supported(const dgppo_env_cfg* cfg, int32_t F, int32_t H);
int32_t dgppo_attn_fwd_rows(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt, const float* Xa,
                            const float* Xo, const float* emask, float* zcat, float* attn, int32_t G, void* stream);
int32_t dgppo_attn_bwd_rows(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat, const float* attn,
                            const float* qt, const float* emask, const float* Xa, const float* Xo, float* dqt, int32_t G,
                            void* stream);
/* The same layer (F = 32) with the sender rows of the nodes WITHOUT incoming edges (goals, LiDAR hits, obstacles) recomputed
 * inside the kernel instead of read: Xo = relu(Xo_raw Wo + bo), Xo_raw [G*(Ns-n),8] their padded raw features, Wo [8,ldwo] the
 * first 8 rows of the previous layer's update weight (Wout of dgppo_gnn_prep), bo [32] its bias — what the reference's
 * GraphTransformer layer produces for a node with aggr = 0 (dgppo/nn/gnn.py:109-111) before the next layer reads it as a
 * sender (gnn.py:85-117).  Saves the 9 KB per graph of materialised rows in the forward and again in the backward.
 * dgppo_attn_xo_supported: 1 if the topology has such a kernel (8 LiDAR hits per agent or no private nodes, <= 32 shared
 * nodes, H <= 4), else 0 -> materialise Xo with dgppo_dense_fwd and call dgppo_attn_fwd / dgppo_attn_bwd.
 * dXo of the backward is the gradient w.r.t. the RECOMPUTED rows (relu_xo != 0: already multiplied by relu'), i.e. exactly
 * what dgppo_dense_bwd_w needs for dWo / dbo.                                                                            */
int32_t dgppo_attn_xo_supported(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp);
int32_t dgppo_attn_fwd_xo(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt, const float* Xa,
                          const float* Xo_raw, const float* Wo, int32_t ldwo, const float* bo, const float* efeat,
                          const float* emask, float* zcat, float* attn, int32_t G, void* stream);
int32_t dgppo_attn_bwd_xo(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                          const float* attn, const float* qt, const float* Xa, const float* Xo_raw, const float* Wo,
                          int32_t ldwo, const float* bo, const float* efeat, float* dqt, float* dXa, float* dXo,
                          int32_t relu_xo, int32_t G, void* stream);
/* dgppo_attn_bwd_xo that CONSUMES the gradient of the recomputed rows instead of writing it (9 KB per graph that
 * dgppo_dense_bwd_w would read again): dWo [8,lddwo] += Xo_raw^T dpre, dbo [32] += colsum(dpre), dpre = relu'(Xo) * dXo — the
 * weight gradient jax.grad gives the previous layer's update Dense for the nodes without incoming edges (gnn.py:109-111).
 * workspace: dgppo_attn_xo_workspace_bytes(G) bytes, caller-owned, 16-byte aligned (per-graph partial sums, reduced by a
 * second launch on the same stream).                                                                                      */
int64_t dgppo_attn_xo_workspace_bytes(int32_t G);
int32_t dgppo_attn_bwd_xo_dw(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                             const float* attn, const float* qt, const float* Xa, const float* Xo_raw, const float* Wo,
                             int32_t ldwo, const float* bo, const float* efeat, float* dqt, float* dXa, float* dWo,
                             int32_t lddwo, float* dbo, float* workspace, int64_t workspace_bytes, int32_t G, void* stream);

/* GraphTransformer parameters (flax Dense_0..4 = q,k,v,e,u; gnn.py:86-110) -> Mcat [Fp,H*Fp], cvec [H*Fp],
 * Wout [Kp,D] used by dgppo_attn_* and the surrounding Denses; and the adjoint map (accumulates into d*).           */
int32_t dgppo_gnn_prep(const float* Wq, const float* bq, const float* Wk, const float* Wv, const float* bv,
                       const float* We, const float* Wu, float* Mcat, float* cvec, float* Wout, int32_t F, int32_t Fp,
                       int32_t D, int32_t H, int32_t Kp, void* stream);
int32_t dgppo_gnn_unprep(const float* dMcat, const float* dcvec, const float* dWout, const float* Wq, const float* bq,
                         const float* Wk, float* dWq, float* dbq, float* dWk, float* dWv, float* dbv, float* dWe,
                         float* dWu, int32_t F, int32_t Fp, int32_t D, int32_t H, int32_t Kp, void* stream);

/* y = relu(LayerNorm_64(x)) (dgppo/nn/mlp.py:27-29; flax LayerNorm eps 1e-6); stats [M,2] = mean, rstd.          */
int32_t dgppo_ln_relu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, int32_t M,
                          void* stream);
int32_t dgppo_ln_relu_bwd(const float* x, const float* y, const float* stats, const float* gamma, const float* dy,
                          float* dx, float* dgamma, float* dbeta, int32_t M, void* stream);

/* GRU scan (dgppo/nn/rnn.py:14-30, flax GRUCell, 64 features).  gi [rows,192] = x Wi + bi precomputed; Wh [64,192]
 * (r|z|n); sequence s at step tau lives in row ((s/n_inner)*T + tau)*n_inner + s%n_inner.  h0 [n_seq,64] or NULL.
 * hs [rows,64]; hprev [rows,64] and gates [rows,256] are saved for the backward when non-NULL.                      */
int32_t dgppo_gru_fwd(const float* gi, const float* Wh, const float* bhn, const float* h0, float* hs, float* hprev,
                      float* gates, int32_t n_seq, int32_t T, int32_t n_inner, void* stream);
/* The same scan with h0 read in place from a blocked buffer: the carry of sequence s lives at
 * h0 + (s / rows_per_block) * block_stride + (s % rows_per_block) * 64 (floats; block_stride a multiple of 4, h0 16-byte
 * aligned and not NULL).  With block_stride == rows_per_block * 64 this is dgppo_gru_fwd.  The Vh pre-pass reads the
 * env-major carry record [B, T+2, n, 64] this way: rows_per_block = (T+1)*n, block_stride = (T+2)*n*64.                */
int32_t dgppo_gru_fwd_h0_blocks(const float* gi, const float* Wh, const float* bhn, const float* h0,
                                int32_t rows_per_block, int64_t block_stride, float* hs, float* hprev, float* gates,
                                int32_t n_seq, int32_t T, int32_t n_inner, void* stream);
/* The one-step pass (T = 1) with h0 read in place through a two-level map with an optional id list: sequence s is cell
 * c = s / n_inner, agent a = s % n_inner, the cell is (e, t) = (c / n_time, c % n_time), and its carry lies at
 * h0 + env * env_stride + t * time_stride + a * 64, env = ids ? ids[e] : e (floats).  ids: n_env int32 env numbers on the
 * device (the caller vouches that each addresses the record) or NULL; n_seq <= n_env * n_time * n_inner.  h0 16-byte
 * aligned and both strides multiples of 4, anything else is refused.  time_stride = n_inner * 64 without ids is
 * dgppo_gru_fwd_h0_blocks with rows_per_block = n_time * n_inner.  The Vh minibatch pass reads the carry record of the
 * deterministic rollout this way, through the minibatch's env ids, instead of a gathered copy.                          */
int32_t dgppo_gru_fwd_h0_map(const float* gi, const float* Wh, const float* bhn, const float* h0, const int32_t* ids,
                             int32_t n_env, int32_t n_time, int64_t env_stride, int64_t time_stride, float* hs,
                             float* hprev, float* gates, int32_t n_seq, int32_t n_inner, void* stream);
/* BPTT over the T steps of every sequence: dgi [rows,192], dgh [rows,192] (then dWh = hprev^T dgh).               */
int32_t dgppo_gru_bwd(const float* dhs, const float* Wh, const float* hprev, const float* gates, float* dgi,
                      float* dgh, int32_t n_seq, int32_t T, int32_t n_inner, void* stream);
/* The same BPTT without the duplicate: dgh's r / z columns ARE dgi's, so only its third block leaves the kernel, as
 * dhn [rows,64] (= dgh[:,128:], bit for bit; dgi is bit for bit dgppo_gru_bwd's).  Feeds dgppo_gru_bwd_w.            */
int32_t dgppo_gru_bwd_dhn(const float* dhs, const float* Wh, const float* hprev, const float* gates, float* dgi,
                          float* dhn, int32_t n_seq, int32_t T, int32_t n_inner, void* stream);
/* All weight gradients of one GRU layer from one pass over its rows (jax.grad of flax GRUCell, dgppo/nn/rnn.py:14-30):
 * dWi [64,ldwi >= 192] += x^T dgi, dbi [192] += colsum(dgi), dWh [64,ldwh >= 192] += hprev^T [dgi[:,:128] | dhn],
 * dbhn [64] += colsum(dhn) (the hr / hz Denses have no bias).  x [M,ldx], hprev [M,ldh]; dgi [M,192] and dhn [M,64] dense;
 * all four 16-byte aligned, ldx / ldh multiples of 4.  workspace: dgppo_gru_bwd_w_workspace_bytes() bytes for one partial
 * slab per CU (smaller: fewer, longer workgroups; NULL / 0 or M <= 256: atomicAdd into the outputs).  pending: NULL reduces
 * the slabs now; otherwise [3] descriptors receive the owed reductions (pending = 0 where none is) for
 * dgppo_dense_bwd_w_reduce_batch, under the contract of dgppo_dense_bwd_w_deferred.                                      */
int64_t dgppo_gru_bwd_w_workspace_bytes(void);
int32_t dgppo_gru_bwd_w(const float* x, int32_t ldx, const float* hprev, int32_t ldh, const float* dgi, const float* dhn,
                        float* dWi, int32_t ldwi, float* dbi, float* dWh, int32_t ldwh, float* dbhn, int32_t M,
                        float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream);
/* The same pass for a one-step GRU (T = 1, the state before the step is h0 [M,ldh]) with the BPTT inside it: the gate gradients
 * are formed on chip from dhs [M,64], gates [M,256] (as dgppo_gru_fwd saved them) and h0, so neither dgppo_gru_bwd_dhn runs nor
 * dhn exists in memory.  Writes dgi [M,192] (bit-equal to dgppo_gru_bwd_dhn at T = 1, -0.0 and NaN inputs included) for the
 * layer below, and accumulates dWi, dbi, dWh, dbhn as dgppo_gru_bwd_w does from that dgi and the dhn of the same call
 * (summation order differs from it in dbi / dbhn only; h0 is loaded twice per tile, as operand of dWh and for the gates).  x, h0, dhs, gates, dgi 16-byte aligned, ldx / ldh multiples of 4;
 * workspace and pending as dgppo_gru_bwd_w.                                                                                     */
int32_t dgppo_gru_bwd_w_t1(const float* x, int32_t ldx, const float* h0, int32_t ldh, const float* dhs, const float* gates,
                           float* dgi, float* dWi, int32_t ldwi, float* dbi, float* dWh, int32_t ldwh, float* dbhn, int32_t M,
                           float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream);
/* dgppo_gru_bwd_w_t1 with row m of h0 read through the map of dgppo_gru_fwd_h0_map (both of its reads: the operand of dWh and
 * the gate gradients); M <= n_env * n_time * n_inner.  Every value and every sum is that of dgppo_gru_bwd_w_t1 on the gathered
 * dense copy of the same rows.                                                                                                  */
int32_t dgppo_gru_bwd_w_t1_map(const float* x, int32_t ldx, const float* h0, const int32_t* ids, int32_t n_env, int32_t n_time,
                               int32_t n_inner, int64_t env_stride, int64_t time_stride, const float* dhs, const float* gates,
                               float* dgi, float* dWi, int32_t ldwi, float* dbi, float* dWh, int32_t ldwh, float* dbhn,
                               int32_t M, float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream);

/* LSTM scan (train.py --use-lstm; dgppo/nn/rnn.py:22-24 with flax nn.LSTMCell(64): i,f,o sigmoid, g tanh, c' = f c + i g,
 * h' = o tanh(c'), carry (c, h)).  zi [rows,256] = x [W_ii|W_if|W_ig|W_io] precomputed (flax's input Denses have no bias);
 * Wh [64,256], bh [256] (the hidden Denses' biases); row addressing as dgppo_gru_fwd.  c0 / h0 [n_seq,64] or NULL.
 * cs / hs [rows,64]; cprev, hprev [rows,64] and gates [rows,256] (post-activation) are saved for the backward when non-NULL. */
int32_t dgppo_lstm_fwd(const float* zi, const float* Wh, const float* bh, const float* c0, const float* h0, float* cs,
                       float* hs, float* cprev, float* hprev, float* gates, int32_t n_seq, int32_t T, int32_t n_inner,
                       void* stream);
/* BPTT of the above from the gradient of every step's output: dz [rows,256] = gradient of the gate pre-activations
 * (then dW_i = x^T dz, dW_h = hprev^T dz, db_h = colsum dz, dx = dz W_i^T outside).                                     */
int32_t dgppo_lstm_bwd(const float* dhs, const float* Wh, const float* cprev, const float* gates, float* dz,
                       int32_t n_seq, int32_t T, int32_t n_inner, void* stream);

/* tanh-Normal head (algo/module/policy.py:62-74,191-212 ; distribution.py:10-46).  ms [rows,4] = mean(2)|std_trans(2).
 * mode 0 sample (eps [rows,2]) -> action, log_pi; 1 mode -> action = tanh(mean); 2 eval (action_in, eps = the constant
 * entropy noise [n_agents,2]) -> log_pi, entropy and, when dms != NULL, the PPO clipped-surrogate loss gradient
 * (informarl.py:428-438) w.r.t. ms plus stats[0..3] += sum loss, sum entropy, sum(l2>l1), sum|rho-1|.               */
int32_t dgppo_policy_head(const float* ms, const float* eps, const float* action_in, float* action, float* log_pi,
                          float* entropy, int32_t rows, int32_t n_agents, int32_t mode, const float* log_pi_old,
                          const float* adv, float* dms, float* stats, float clip_eps, float coef_ent, void* stream);

/* optax.l2_loss(v, target).mean() (informarl.py:374, dgppo.py:310): dv = (v-target)/count, stats[0] += sum 1/2 d^2 */
int32_t dgppo_value_loss(const float* v, const float* target, float* dv, float* stats, int32_t count, void* stream);
/* mean over the n agents of each graph (value.py:33): x [G,n,D] -> y [G,D]; backward = 1: x = dy [G,D] -> y = dx [G,n,D]
 * (= x / n); backward = 2: y[g,i,:] += x[g,:] (broadcast-add of a per-graph row, the tiled global feature of
 * DecRStateFn(use_global_info=True), value.py:66-68); both optionally through the ReLU that produced the pooled rows
 * (relu_mask [G,n,D] = that ReLU's output, or NULL)                                                                      */
int32_t dgppo_mean_agents(const float* x, float* y, int32_t G, int32_t n, int32_t D, int32_t backward,
                          const float* relu_mask, void* stream);
/* dy *= (y > 0), in place                                                                                             */
int32_t dgppo_relu_bwd(float* dy, const float* y, int64_t count, void* stream);

/* ---- GAE, advantage, optimiser ---------------------------------------------------------------- */

/* compute_dec_ocp_gae (dgppo/algo/utils.py:11-79) for B envs (env-major): costs [B,T,n,nh], rewards [B,T] (l = -reward),
 * Vh [B,T+1,n,nh], Vl [B,T+1], lam_pow [T+1] = lambda^i  ->  Qh [B,T,n,nh], Ql [B,T].                                  */
int32_t dgppo_gae(const float* costs, const float* rewards, const float* Vh, const float* Vl, const float* lam_pow,
                  float gamma, float one_minus_gamma, float one_minus_lam, float* Qh, float* Ql, int32_t B, int32_t T,
                  int32_t n, int32_t nh, void* stream);
/* advantage block (dgppo/algo/dgppo.py:239-259): per-env normalised Ql-Vl, CBF derivative, safe gate, schedule weight
 * -> adv [B,T,n] (already negated); stats[0] += number of safe (t, agent) pairs (eval/safe_data numerator).
 * Vh == NULL: InforMARL's advantage (dgppo/algo/informarl.py:334-336): -(Ql-Vl normalised per env), no CBF terms.    */
int32_t dgppo_advantage(const float* Ql, const float* Vl, const float* Vh, float dt, float alpha, float cbf_eps,
                        float cbf_weight, float* adv, float* stats, int32_t B, int32_t T, int32_t n, int32_t nh,
                        void* stream);
/* InforMARL-Lagrangian advantage (dgppo/algo/informarl_lagr.py:219-235): Al = (Ql - Vl) standardised per env over T, Ah =
 * (Qh - Vh[:, :T]) standardised per (env, agent, component) over T (population std, + 1e-8), adv = -Al - mean_h(Ah *
 * lagr[a,h]).  Ql [B,T], Vl [B,T+1], Qh [B,T,n,nh], Vh [B,T+1,n,nh], lagr [n,nh] -> adv [B,T,n], Ah [B,T,n,nh].
 * n * nh <= 192 (64 agents x 3 costs, every admitted team); more columns are refused before anything is launched.        */
int32_t dgppo_advantage_lagr(const float* Ql, const float* Vl, const float* Qh, const float* Vh, const float* lagr,
                             float* adv, float* Ah, int32_t B, int32_t T, int32_t n, int32_t nh, void* stream);
/* update_lagr (informarl_lagr.py:286-309) on one minibatch of n_env envs: delta[a,h] = -mean_{env,t}(Vh (1 - gamma) +
 * exp(lp_new - lp_old) Ah), lagr = relu(lagr - delta * lr).  lp_* [n_env,T,n], Ah [n_env,T,n,nh] (gathered), Vh: base of
 * the gathered value rows with vh_env_stride floats between envs (first T steps used), sums [n*nh]: zeroed scratch.    */
int32_t dgppo_lagr_update(const float* lp_new, const float* lp_old, const float* Vh, int64_t vh_env_stride,
                          const float* Ah, float* lagr, float* sums, int32_t n_env, int32_t T, int32_t n, int32_t nh,
                          float one_minus_gamma, float lr, void* stream);
/* The same step in two halves for the data-parallel update (the `.mean()` of informarl_lagr.py:300-304 runs over the GLOBAL
 * minibatch): dgppo_lagr_sums accumulates this rank's share into sums[n*nh] (+=), the caller all-reduces sums, and
 * dgppo_lagr_apply does lagr = relu(lagr + lr * sums / rows_total) with rows_total = global n_env * T, then zeroes sums. */
int32_t dgppo_lagr_sums(const float* lp_new, const float* lp_old, const float* Vh, int64_t vh_env_stride, const float* Ah,
                        float* sums, int32_t n_env, int32_t T, int32_t n, int32_t nh, float one_minus_gamma, void* stream);
int32_t dgppo_lagr_apply(float* lagr, float* sums, int32_t count, int64_t rows_total, float lr, void* stream);
/* out = max(x, 0): jnp.clip(rollout.costs, a_min=0) of informarl_lagr.py:213                                             */
int32_t dgppo_relu_fwd(const float* x, float* out, int64_t count, void* stream);
/* InforMARL's stage cost l = -reward + w * sum_{agents, components} max(cost, 0) (dgppo/algo/informarl.py:329), as the
 * equivalent reward out = reward - w * sum(...) for dgppo_gae.  reward/out [rows], cost [rows, n, nh].              */
int32_t dgppo_shaped_reward(const float* reward, const float* cost, float cost_weight, float* out, int64_t rows,
                            int32_t n, int32_t nh, void* stream);
/* compute_norm_and_clip + has_any_nan_or_inf (dgppo/trainer/utils.py:89-118) and optax.apply_if_finite(adam)
 * (dgppo/algo/informarl.py:131-137) on one flat buffer.  state [DGPPO_OPT_STATE_FLOATS] lives on the device (zero it once):
 * [2] adam count, [3] total steps, [4] last grad norm, [5] last non-finite flag, [8..] per-workgroup partial sums of the
 * norm / non-finite statistics — reduced in a FIXED order with no atomics, so that data-parallel replicas that start
 * from identical gradients stay bit-identical.
 * grad_scale multiplies every gradient entry as it is read (norm, non-finite test and update all see g * grad_scale):
 * 1 for a single device, 1/world after dgppo_comm_allreduce_sum_f32 (the mean of equal-sized shards' gradients is the
 * gradient of the global mean loss), so the data-parallel path needs no separate scaling pass.                       */
#define DGPPO_OPT_PARTIALS 256
#define DGPPO_OPT_STATE_FLOATS (8 + 2 * DGPPO_OPT_PARTIALS)
int32_t dgppo_clip_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float* state, float lr,
                             float b1, float b2, float eps, float max_norm, float grad_scale, void* stream);

/* ---- C1: gradient exchange over RCCL / xGMI (no reference counterpart: the reference is single-device, SURVEY F2;
 * this is jax.lax.pmean of the gradient trees of a pmap'ed update_inner, dgppo/algo/dgppo.py:188-294) -------------- */
#define DGPPO_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (ncclGetUniqueId); the caller ships the 128 bytes to the other ranks out of band.   */
int32_t dgppo_comm_unique_id(uint8_t* id_out);
/* version code of the RCCL library the process resolved (ncclGetVersion), for the diagnostics a multi-GPU launch prints
 * before its first collective; no device work.                                                                       */
int32_t dgppo_comm_version(int32_t* version_out);
/* every rank, after selecting its HIP device: join the communicator (ncclCommInitRank).  *comm_out is an opaque
 * handle owned by the library until dgppo_comm_destroy.  Collective: blocks until all `world` ranks have called it. */
int32_t dgppo_comm_init(const uint8_t* id, int32_t rank, int32_t world, void** comm_out);
/* in-place all-reduce(sum) of buf[count] fp32 (DEVICE pointer) enqueued on `stream`; never synchronises the host.
 * One call per minibatch on the flat [g_policy | g_Vl | g_Vh | scalars] buffer.                        */
int32_t dgppo_comm_allreduce_sum_f32(void* comm, float* buf, int64_t count, void* stream);
int32_t dgppo_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* DGPPO_HIP_H */
