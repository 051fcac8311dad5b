// VMASReverseTransport: batched reset, contact-physics step and graph features.
//
// Reference arithmetic replaced (file:line relative to the reference repository):
//   VMASReverseTransport.reset / step / get_reward / get_cost / get_graph / edge_blocks
//                                dgppo/env/vmas/vmas_reverse_transport.py:90-128, 130-206, 208-221, 223-249, 251-311
//   World.step / _integrate_state_pos / _box_sphere_collision / _get_constraint_forces
//                                dgppo/env/vmas/physax/world.py:78-163, 361-474, 476-505
//   get_closest_point_line / get_closest_point_box / get_all_lines_box
//                                dgppo/env/vmas/physax/geometry.py:8-102
//   get_node_goal_rng            dgppo/env/utils.py:139-244 (agents only)
//   GetGraph.to_padded / EdgeBlock.make_edges   dgppo/utils/graph.py:35-44, 212-247
//
// Step layout: one lane per (env, agent), P = next power of two >= n lanes per env, 64 / P envs per wave.  A substep needs
// the box position (the same on every lane of the env) and the sum of the agents' contact forces on the box, which every
// lane of the env forms itself from __shfl reads in agent order, so that the box is integrated redundantly and identically
// on each lane: no LDS and no barrier across the 20 substeps.  Built with -ffp-contract=off (Makefile EXACT_SRCS): each
// fp32 operation below is one IEEE operation in the order of tests/vmas_np.py, so a step without contact matches that
// restatement bit for bit; with contact the forces go through expf / log1pf (a few ulps).
//
// Non-finite inputs: the reference clips with jnp.clip and reduces with jnp.min, which keep a NaN, and jnp.argsort sorts NaN
// last.  Every clip below goes through clampf_nan and both cost minima through nanmin (common.h), and the obstacle rank of
// node_row puts NaN last, so a NaN action or state gives the reference's visibly NaN rollout and not a finite one; for every
// non-NaN input these give the bits of fminf / fmaxf and of the plain comparison.
#include "common.h"

namespace {

// constants the reference forms in Python doubles and JAX rounds to fp32 (weakly typed scalars)
constexpr float kHalfSide = (float)(0.6 / 2);                   // box_length / 2 = box_width / 2, geometry.py:77-78
constexpr float kDistMin = (float)(0.03 + 4.0 / 6e2);           // radius + Default.LINE_MIN_DIST, world.py:460-463
constexpr float kMargin = (float)6e-3;                          // contact_margin, vmas_reverse_transport.py:143
constexpr float kMinDist = (float)1e-6;                         // world.py:485
constexpr float kCollisionForce = 500.0f;
constexpr float kSubDt = (float)(0.1 / 5);                      // World dt 0.1, 5 substeps
constexpr float kDragKeep = (float)(1 - 0.25);                  // Default.DRAG
constexpr float kSemidim = (float)1.2;
constexpr float kBoxMass = 10.0f;
constexpr float kUMult = 0.5f;
constexpr float kContactThr = (float)(0.6 - 1e-2);              // get_a_incontact: package_width - eps, :266-268
constexpr float kTwoAgentR = (float)(0.03 * 2);
constexpr float kObsR = (float)0.15;
constexpr float kDist2Goal = (float)0.01;
constexpr int kSubsteps = 5, kFrameSkip = 4;
constexpr int kMaxAgents = 16;

struct Vec2f {
  float x, y;
};

__device__ inline float norm2f(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }

// jnp.sign: 0 at 0
__device__ inline float signf0(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : x); }

// closest point of one side (geometry.py:8-33): line centre (lx, ly), direction (rx, ry), half length kHalfSide
__device__ inline Vec2f closest_on_line(float lx, float ly, float rx, float ry, float px, float py) {
  const float dx = lx - px, dy = ly - py;
  const float dot = dx * rx + dy * ry;
  const float s = signf0(dot);
  const float dfc = fminf(fabsf(dot), kHalfSide);
  const float sd = s * dfc;
  return Vec2f{lx - sd * rx, ly - sd * ry};
}

// contact force on the agent at (px, py) from the hollow box at (bx, by) (world.py:361-474, 476-505).  The box's second
// side direction is (cos, sin)(fp32(pi / 2)) = (-4.371139e-08, 1) (geometry.py:71-72).
__device__ inline Vec2f contact_force(float px, float py, float bx, float by) {
  const float c90 = -4.37113883e-08f;              // cosf(1.57079637f)
  const float r2x = c90, r2y = 1.0f;
  // side centres p1..p4 (geometry.py:80-84): box_pos +- rotated_vector * half
  const float h1x = 1.0f * kHalfSide, h1y = 0.0f * kHalfSide;
  const float h2x = r2x * kHalfSide, h2y = r2y * kHalfSide;
  const float lx[4] = {bx + h1x, bx - h1x, bx + h2x, bx - h2x};
  const float ly[4] = {by + h1y, by - h1y, by + h2y, by - h2y};
  // sides 1, 2 run along rot + pi / 2, sides 3, 4 along rot (geometry.py:86-90)
  float cx = INFINITY, cy = INFINITY, best = INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Vec2f q = (k <= 1) ? closest_on_line(lx[k], ly[k], r2x, r2y, px, py) : closest_on_line(lx[k], ly[k], 1.0f, 0.0f, px, py);
    const float d = norm2f(px - q.x, py - q.y);
    if (d < best) { best = d; cx = q.x; cy = q.y; }          // strict <: the first of equal sides wins (geometry.py:44-48)
  }
  const float dx = px - cx, dy = py - cy;
  const float dist = norm2f(dx, dy);
  const float v = ((kDistMin - dist) * 1.0f) / kMargin;
  const float pen = (fmaxf(0.0f, v) + log1pf(expf(-fabsf(v)))) * kMargin;   // jnp.logaddexp(0, v) * k
  const float den = (dist > 0.0f) ? dist : 1e-8f;
  float fx = ((kCollisionForce * dx) / den) * pen;
  float fy = ((kCollisionForce * dy) / den) * pen;
  if (dist < kMinDist || dist > kDistMin) { fx = 0.0f; fy = 0.0f; }
  return Vec2f{fx, fy};
}

// one node row of get_graph (:251-289): 20 columns
__device__ inline void node_row(const float* a, const float* body, const float* scene, float* out) {
  const float bx = body[0], by = body[1];
  out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
  out[4] = bx; out[5] = by; out[6] = body[2]; out[7] = body[3];
  out[8] = scene[0] - bx; out[9] = scene[1] - by;
  out[10] = (fabsf(a[0] - bx) > kContactThr || fabsf(a[1] - by) > kContactThr) ? 1.0f : 0.0f;
  float vx[3], vy[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float rx = scene[2 + 2 * k] - bx, ry = scene[3 + 2 * k] - by;
    d[k] = sqrtf((rx * rx + ry * ry) + 1e-6f);
    vx[k] = rx / d[k]; vy[k] = ry / d[k];
  }
  // stable argsort of 3 distances, NaN last (jnp.argsort; ray_rank of env_step.h): rank = #smaller + #equal before.  The ranks
  // are a permutation of 0, 1, 2, so each slot below finds its obstacle and every column is written.
  int rank[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool nk = (d[k] != d[k]);
    int r = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const bool nj = (d[j] != d[j]);
      bool less;
      if (nj || nk) less = (nj == nk) ? (j < k) : nk;
      else less = (d[j] < d[k]) || (d[j] == d[k] && j < k);
      r += less ? 1 : 0;
    }
    rank[k] = r;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = (rank[0] == r) ? 0 : ((rank[1] == r) ? 1 : 2);
    out[11 + 2 * r] = (k == 0) ? vx[0] : ((k == 1) ? vx[1] : vx[2]);
    out[12 + 2 * r] = (k == 0) ? vy[0] : ((k == 1) ? vy[1] : vy[2]);
    out[17 + r] = (k == 0) ? d[0] : ((k == 1) ? d[1] : d[2]);
  }
}

// padded GraphsTuple of one env (graph.py:212-247): lane i of the env writes agent row i and edge row i (n edges); the
// lane with i == 0 also writes the pad node and the counts.  states has zero columns: nothing to write.
__device__ inline void write_graph(const dgppo_graph_out& g, int b, int i, int n, const float* a_i, const float* body,
                                   const float* scene, const float* sx, const float* sy, const float* svx, const float* svy) {
  const int Nn = n + 1, E = n * n;
  float row[20];
  node_row(a_i, body, scene, row);
  float* nd = g.nodes + ((size_t)b * Nn + i) * 20;
#pragma unroll
  for (int c = 0; c < 20; ++c) nd[c] = row[c];
  g.node_type[(size_t)b * Nn + i] = 0;
  for (int j = 0; j < n; ++j) {
    const size_t e = (size_t)b * E + (size_t)i * n + j;
    reinterpret_cast<float4*>(g.edges)[e] = make_float4(a_i[0] - sx[j], a_i[1] - sy[j], a_i[2] - svx[j], a_i[3] - svy[j]);
    g.receivers[e] = (i != j) ? i : n;
    g.senders[e] = (i != j) ? j : n;
  }
  if (i == 0) {
    float* pad = g.nodes + ((size_t)b * Nn + n) * 20;
    for (int c = 0; c < 20; ++c) pad[c] = 0.0f;
    g.node_type[(size_t)b * Nn + n] = -1;
    g.n_node[b] = Nn;
    g.n_edge[b] = E;
  }
}

struct VmasStepArgs {
  const float* agent;
  const float* body;
  const float* scene;
  const float* action;      // NULL: graph only
  float* next_agent;
  float* next_body;
  float* reward;
  float* cost;
  dgppo_graph_out g;
  int has_graph;
  int n, B;
};

template <int P>
__global__ __launch_bounds__(256) void vmas_step_kernel(VmasStepArgs a) {
  const int gl = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gl / P, i = gl % P;
  const int n = a.n;
  const bool env_ok = b < a.B;
  const bool live = env_ok && i < n;
  float px = 0.0f, py = 0.0f, vx = 0.0f, vy = 0.0f, ux = 0.0f, uy = 0.0f;
  float bx = 0.0f, by = 0.0f, bvx = 0.0f, bvy = 0.0f;
  float sc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (live) {
    const float* s = a.agent + ((size_t)b * n + i) * 4;
    px = s[0]; py = s[1]; vx = s[2]; vy = s[3];
    if (a.action) {
      const float* u = a.action + ((size_t)b * n + i) * 2;
      ux = clampf_nan(u[0], -1.0f, 1.0f) * kUMult;          // clip_action, then u_multiplier (entity.py, world.py:296-309)
      uy = clampf_nan(u[1], -1.0f, 1.0f) * kUMult;
    }
  }
  if (env_ok) {
    const float* bd = a.body + (size_t)b * 4;
    bx = bd[0]; by = bd[1]; bvx = bd[2]; bvy = bd[3];
#pragma unroll
    for (int k = 0; k < 8; ++k) sc[k] = a.scene[(size_t)b * 8 + k];
  }
  if (a.action) {
    // ---- reward and cost of the pre-step state (:208-249) ----
    float mind = 3.4e38f;
    for (int j = 0; j < n; ++j) {
      const float qx = __shfl(px, j, P), qy = __shfl(py, j, P);
      const float d = norm2f(px - qx, py - qy) + ((j == i) ? 1e6f : 0.0f);
      mind = nanmin(mind, d);                               // jnp.min: a NaN distance makes the margin NaN
    }
    float mino = 3.4e38f;
#pragma unroll
    for (int k = 0; k < 3; ++k) mino = nanmin(mino, norm2f(bx - sc[2 + 2 * k], by - sc[3 + 2 * k]));
    if (live) {
      float c0 = 4.0f * (kTwoAgentR - mind), c1 = 2.0f * (kObsR - mino);
      c0 = (c0 <= 0.0f) ? c0 - 0.5f : c0 + 0.5f;
      c1 = (c1 <= 0.0f) ? c1 - 0.5f : c1 + 0.5f;
      a.cost[((size_t)b * n + i) * 2] = clampf_nan(c0, -1.0f, 1.0f);
      a.cost[((size_t)b * n + i) * 2 + 1] = clampf_nan(c1, -1.0f, 1.0f);
      if (i == 0) {
        const float dg = norm2f(sc[0] - bx, sc[1] - by);
        float r = -dg * 0.01f;
        r = r - ((dg > kDist2Goal) ? 1.0f : 0.0f) * 0.001f;
        a.reward[b] = r;
      }
    }
    // ---- 4 world steps x 5 substeps (world.py:78-105) ----
    for (int w = 0; w < kFrameSkip; ++w) {
#pragma unroll 1
      for (int s = 0; s < kSubsteps; ++s) {
        const Vec2f f = live ? contact_force(px, py, bx, by) : Vec2f{0.0f, 0.0f};
        // the box collects -f of each agent in agent order (update_forcetorque, world.py:492-505)
        float Fbx = 0.0f, Fby = 0.0f;
        for (int j = 0; j < n; ++j) {
          const float gx = __shfl(-f.x, j, P), gy = __shfl(-f.y, j, P);
          if (j == 0) { Fbx = gx; Fby = gy; } else { Fbx = Fbx + gx; Fby = Fby + gy; }
        }
        Fbx = 0.0f + Fbx; Fby = 0.0f + Fby;
        const float Fax = ux + f.x, Fay = uy + f.y;
        if (s == 0) {
          vx = vx * kDragKeep; vy = vy * kDragKeep;
          bvx = bvx * kDragKeep; bvy = bvy * kDragKeep;
        }
        vx = vx + (Fax / 1.0f) * kSubDt; vy = vy + (Fay / 1.0f) * kSubDt;
        px = clampf_nan(px + vx * kSubDt, -kSemidim, kSemidim);
        py = clampf_nan(py + vy * kSubDt, -kSemidim, kSemidim);
        bvx = bvx + (Fbx / kBoxMass) * kSubDt; bvy = bvy + (Fby / kBoxMass) * kSubDt;
        bx = clampf_nan(bx + bvx * kSubDt, -kSemidim, kSemidim);
        by = clampf_nan(by + bvy * kSubDt, -kSemidim, kSemidim);
      }
    }
    if (live) {
      float* o = a.next_agent + ((size_t)b * n + i) * 4;
      o[0] = px; o[1] = py; o[2] = vx; o[3] = vy;
      if (i == 0) {
        float* ob = a.next_body + (size_t)b * 4;
        ob[0] = bx; ob[1] = by; ob[2] = bvx; ob[3] = bvy;
      }
    }
  }
  if (a.has_graph) {
    float sx[kMaxAgents], sy[kMaxAgents], svx[kMaxAgents], svy[kMaxAgents];
#pragma unroll
    for (int j = 0; j < kMaxAgents; ++j) {
      if (j < n) { sx[j] = __shfl(px, j, P); sy[j] = __shfl(py, j, P); svx[j] = __shfl(vx, j, P); svy[j] = __shfl(vy, j, P); }
    }
    if (live) {
      const float ai[4] = {px, py, vx, vy};
      const float body[4] = {bx, by, bvx, bvy};
      write_graph(a.g, b, i, n, ai, body, sc, sx, sy, svx, svy);
    }
  }
}

// ---- reset -------------------------------------------------------------------------------------------------------------
struct VmasResetArgs {
  const uint64_t* seeds;
  float* agent;
  float* body;
  float* scene;
  int32_t* n_failed;
  int n, B;
};

struct VStream {
  uint32_t k0, k1, d;
  __device__ inline void uniform2(float& u0, float& u1) {
    Philox4 p = philox4x32_10(d, 0u, 0u, 0u, k0, k1);
    d += 1;
    u0 = u01_from_u32(p.v[0]);
    u1 = u01_from_u32(p.v[1]);
  }
};

// jax.random.uniform(minval, maxval): max(minval, u * (maxval - minval) + minval)
__device__ inline float juniform(float u, float lo, float hi) { return fmaxf(lo, u * (hi - lo) + lo); }

__global__ void vmas_reset_kernel(VmasResetArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n;
  const uint64_t seed = a.seeds[b];
  VStream st;
  st.k0 = (uint32_t)seed; st.k1 = (uint32_t)(seed >> 32); st.d = 0;
  constexpr float kTwoPi = (float)(2 * 3.14159265358979323846);
  constexpr float kPi = (float)3.14159265358979323846;
  constexpr float kNoise = (float)(30.0 * (3.14159265358979323846 / 180.0));  // np.deg2rad(30)
  constexpr float kX0R = (float)(0.98 * (0.8 - 0.5 * 0.6));
  constexpr float kObsRing = (float)(0.98 * (0.8 - 0.5 * 0.6) - 1.5 * 0.15);
  constexpr float kSide = (float)(0.4 * 0.6);
  constexpr float kShift = 0.2f;
  float u0, u1;
  st.uniform2(u0, u1);                                      // d = 0
  const float th = juniform(u0, 0.0f, kTwoPi);
  const float gth = (th + kPi) + juniform(u1, -kNoise, kNoise);
  const float bx = kX0R * cosf(th), by = kX0R * sinf(th);
  float* sc = a.scene + (size_t)b * 8;
  sc[0] = kX0R * cosf(gth); sc[1] = kX0R * sinf(gth);
  float oth[3];
  st.uniform2(u0, u1);                                      // d = 1
  oth[0] = juniform(u0, 0.0f, kTwoPi); oth[1] = juniform(u1, 0.0f, kTwoPi);
  st.uniform2(u0, u1);                                      // d = 2
  oth[2] = juniform(u0, 0.0f, kTwoPi);
  for (int k = 0; k < 3; ++k) { sc[2 + 2 * k] = kObsRing * cosf(oth[k]); sc[3 + 2 * k] = kObsRing * sinf(oth[k]); }
  float* ag = a.agent + (size_t)b * n * 4;
  for (int i = 0; i < n; ++i) {                             // d = 3 .. 2 + n
    st.uniform2(u0, u1);
    ag[i * 4 + 2] = juniform(u0, -0.01f, 0.01f);
    ag[i * 4 + 3] = juniform(u1, -0.01f, 0.01f);
  }
  // get_node_goal_rng(key, 0.24, 2, n, 0.06): the work array's unfilled rows are zeros (env/utils.py:150-151)
  float pos[2 * kMaxAgents];
  bool placed = false;
  for (int attempt = 0; attempt < 64 && !placed; ++attempt) {
    for (int k = 0; k < 2 * n; ++k) pos[k] = 0.0f;
    bool failed = false;
    for (int i = 0; i < n && !failed; ++i) {
      int it = 0;
      float cx = 0.0f, cy = 0.0f;
      while (true) {
        st.uniform2(u0, u1);
        cx = juniform(u0, 0.0f, kSide); cy = juniform(u1, 0.0f, kSide);
        float dmin = 3.4e38f;
        for (int j = 0; j < n; ++j) dmin = fminf(dmin, norm2f(pos[2 * j] - cx, pos[2 * j + 1] - cy));
        if (!(dmin <= kTwoAgentR) || it >= 1024) break;
        it += 1;
      }
      pos[2 * i] = cx; pos[2 * i + 1] = cy;
      failed = it >= 1024;
    }
    placed = !failed;
  }
  for (int i = 0; i < n; ++i) {
    ag[i * 4] = (pos[2 * i] - kShift) + bx;
    ag[i * 4 + 1] = (pos[2 * i + 1] - kShift) + by;
  }
  float* bd = a.body + (size_t)b * 4;
  bd[0] = bx; bd[1] = by; bd[2] = 0.0f; bd[3] = 0.0f;
  if (!placed && a.n_failed) atomicAdd(a.n_failed, 1);
}

// ---- features for the networks -------------------------------------------------------------------------------------
struct VmasFeatArgs {
  const float* agent; long agent_se, agent_st;
  const float* body; long body_se, body_st;
  const float* scene;
  const int32_t* env_ids;
  int n_env, n_time, n, Fp;
  float* Xa;      // [G*n, Fp]
  float* efeat;   // [G*n, n, 4]
  float* emask;   // [G*n, n]
};

// one thread per (graph, agent) row
__global__ void vmas_feats_kernel(VmasFeatArgs a) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = a.n;
  const long G = (long)a.n_env * a.n_time;
  if (r >= G * n) return;
  const long g = r / n;
  const int i = (int)(r - g * n);
  const int e = (int)(g / a.n_time), tt = (int)(g - (long)e * a.n_time);
  const int env = a.env_ids ? a.env_ids[e] : e;
  const float* ag = a.agent + (size_t)env * a.agent_se + (size_t)tt * a.agent_st;
  const float* bd = a.body + (size_t)env * a.body_se + (size_t)tt * a.body_st;
  const float* sc = a.scene + (size_t)env * 8;
  float ai[4] = {ag[i * 4], ag[i * 4 + 1], ag[i * 4 + 2], ag[i * 4 + 3]};
  float body[4] = {bd[0], bd[1], bd[2], bd[3]};
  float scene[8];
  for (int k = 0; k < 8; ++k) scene[k] = sc[k];
  float row[20];
  node_row(ai, body, scene, row);
  float* x = a.Xa + (size_t)r * a.Fp;
  for (int c = 0; c < a.Fp; ++c) x[c] = (c < 20) ? row[c] : 0.0f;
  for (int s = 0; s < n; ++s) {
    reinterpret_cast<float4*>(a.efeat)[(size_t)r * n + s] =
        make_float4(ai[0] - ag[s * 4], ai[1] - ag[s * 4 + 1], ai[2] - ag[s * 4 + 2], ai[3] - ag[s * 4 + 3]);
    a.emask[(size_t)r * n + s] = (s != i) ? 1.0f : 0.0f;
  }
}

int32_t check_vmas_cfg(const dgppo_env_cfg* cfg, const char* what) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REQUIRE(cfg_is_vmas(*cfg), "%s: env kind %d is not VMASReverseTransport (10)", what, cfg->kind);
  return 0;
}

int32_t launch_vmas_step(const dgppo_env_cfg* cfg, const float* agent, const float* body, const float* scene,
                         const float* action, float* next_agent, float* next_body, float* reward, float* cost,
                         const dgppo_graph_out* gout, int32_t B, void* stream, const char* what) {
  int32_t rc = check_vmas_cfg(cfg, what);
  if (rc) return rc;
  DGPPO_REQUIRE(B >= 0, "%s: B must be >= 0 (got %d)", what, B);
  if (B == 0) return 0;
  DGPPO_REQUIRE(agent && body && scene, "%s: agent/body/scene must not be NULL", what);
  if (action) DGPPO_REQUIRE(next_agent && next_body && reward && cost, "%s: step needs next_agent, next_body, reward and cost", what);
  VmasStepArgs a;
  a.agent = agent; a.body = body; a.scene = scene; a.action = action; a.next_agent = next_agent; a.next_body = next_body;
  a.reward = reward; a.cost = cost; a.n = cfg->n_agents; a.B = B;
  a.g = dgppo_graph_out{};
  a.has_graph = 0;
  if (gout) {
    DGPPO_REQUIRE(gout->nodes && gout->edges && gout->receivers && gout->senders && gout->node_type && gout->n_node && gout->n_edge,
                  "%s: the graph output needs nodes, edges, receivers, senders, node_type, n_node and n_edge", what);
    DGPPO_REQUIRE(((uintptr_t)gout->edges & 15) == 0, "%s: graph edges must be 16-byte aligned", what);
    a.g = *gout;
    a.has_graph = 1;
  }
  DGPPO_REQUIRE(action || gout, "%s: nothing to do (no action and no graph output)", what);
  const int n = cfg->n_agents;
  const int P = n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16;
  const dim3 grid(cdiv((long)B * P, 256)), block(256);
  const hipStream_t s = (hipStream_t)stream;
  switch (P) {
    case 1: hipLaunchKernelGGL(vmas_step_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(vmas_step_kernel<2>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(vmas_step_kernel<4>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(vmas_step_kernel<8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(vmas_step_kernel<16>, grid, block, 0, s, a); break;
  }
  DGPPO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int32_t dgppo_vmas_step(const dgppo_env_cfg* cfg, const float* agent, const float* body, const float* scene,
                                   const float* action, float* next_agent, float* next_body, float* reward, float* cost,
                                   const dgppo_graph_out* gout, int32_t B, void* stream) {
  if (!action) { dgppo_set_error("dgppo_vmas_step: action is NULL (dgppo_vmas_graph_materialize builds a graph alone)"); return -1; }
  return launch_vmas_step(cfg, agent, body, scene, action, next_agent, next_body, reward, cost, gout, B, stream,
                          "dgppo_vmas_step");
}

extern "C" int32_t dgppo_vmas_graph_materialize(const dgppo_env_cfg* cfg, const float* agent, const float* body,
                                                const float* scene, const dgppo_graph_out* gout, int32_t B, void* stream) {
  if (!gout) { dgppo_set_error("dgppo_vmas_graph_materialize: gout is NULL"); return -1; }
  return launch_vmas_step(cfg, agent, body, scene, nullptr, nullptr, nullptr, nullptr, nullptr, gout, B, stream,
                          "dgppo_vmas_graph_materialize");
}

extern "C" int32_t dgppo_vmas_reset_checked(const dgppo_env_cfg* cfg, const uint64_t* seeds, float* agent, float* body,
                                            float* scene, int32_t* n_failed, int32_t B, void* stream) {
  int32_t rc = check_vmas_cfg(cfg, "dgppo_vmas_reset_checked");
  if (rc) return rc;
  {
    // the density rule of dgppo_env_reset_checked: n discs of diameter 0.06 with centres in the 0.24 square
    const double d = 2 * 0.03, side = 0.4 * 0.6;
    const double cover = cfg->n_agents * 3.14159265358979 * (d / 2) * (d / 2), room = (side + d) * (side + d);
    DGPPO_REQUIRE(cover <= 0.5 * room,
                  "dgppo_vmas_reset_checked: %d agents with minimum separation %.3f cannot be placed in the %.2f square by "
                  "rejection sampling (disc coverage %.2f of the area; the limit used here is 0.50)",
                  cfg->n_agents, d, side, cover / room);
  }
  DGPPO_REQUIRE(B >= 0, "B must be >= 0");
  if (B == 0) return 0;
  DGPPO_REQUIRE(seeds && agent && body && scene, "dgppo_vmas_reset_checked: seeds/agent/body/scene must not be NULL");
  VmasResetArgs a;
  a.seeds = seeds; a.agent = agent; a.body = body; a.scene = scene; a.n_failed = n_failed; a.n = cfg->n_agents; a.B = B;
  hipLaunchKernelGGL(vmas_reset_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t dgppo_vmas_graph_feats(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_se, int64_t agent_st,
                                          const float* body, int64_t body_se, int64_t body_st, const float* scene,
                                          const int32_t* env_ids, int32_t n_env, int32_t n_time, float* Xa, float* efeat,
                                          float* emask, int32_t Fp, void* stream) {
  int32_t rc = check_vmas_cfg(cfg, "dgppo_vmas_graph_feats");
  if (rc) return rc;
  DGPPO_REQUIRE(n_env >= 0 && n_time >= 0, "dgppo_vmas_graph_feats: negative counts");
  if (n_env == 0 || n_time == 0) return 0;
  DGPPO_REQUIRE(agent && body && scene && Xa && efeat && emask, "dgppo_vmas_graph_feats: NULL operand");
  DGPPO_REQUIRE(Fp >= 20 && Fp <= 32, "dgppo_vmas_graph_feats: Fp must be in [20, 32] (got %d)", Fp);
  DGPPO_REQUIRE(((uintptr_t)efeat & 15) == 0, "dgppo_vmas_graph_feats: efeat must be 16-byte aligned");
  VmasFeatArgs a;
  a.agent = agent; a.agent_se = agent_se; a.agent_st = agent_st; a.body = body; a.body_se = body_se; a.body_st = body_st;
  a.scene = scene; a.env_ids = env_ids; a.n_env = n_env; a.n_time = n_time; a.n = cfg->n_agents; a.Fp = Fp;
  a.Xa = Xa; a.efeat = efeat; a.emask = emask;
  const long rows = (long)n_env * n_time * cfg->n_agents;
  DGPPO_REQUIRE(rows < (1L << 31), "dgppo_vmas_graph_feats: too many rows");
  hipLaunchKernelGGL(vmas_feats_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
