// Graph features of the per-agent fixed-fan-in graph: only agents receive messages and every sender slot of an agent has a static
// node id (dgppo/utils/graph.py:35-44, dgppo/env/lidar_env/lidar_spread.py:57-96), see nn_attn.h.
#include "graph_topo.h"

// ---------------------------------------------------------------------------------------------------------------------
// graph features: compact record -> agent/other node feature matrices, per-slot edge features and masks.
// Same arithmetic (explicit _rn ops = no fma contraction) as env_step.hip phase 5, i.e. as
// lidar_env/base.py:227-271 + lidar_spread.py:57-96 (+ MPE twins), so masks agree bit for bit with the GraphsTuple.
// ---------------------------------------------------------------------------------------------------------------------
struct FeatArgs {
  dgppo_env_cfg cfg;
  Topo t;
  const float* agent; long agent_se, agent_st;   // agent + env*se + time*st  -> [n, sd]
  const float* goal;                             // goal + env*ng*sd
  const float* obst;                             // MPE: obst + env*n_obs*sd
  const float* hits; long hits_se, hits_st;      // LiDAR: hits + env*se + time*st -> [n, k, 2]
  const int32_t* env_ids;                        // [n_env] or NULL (identity)
  int n_env, n_time;                             // graphs g = e * n_time + t
  float* Xa;      // [G*n, Fp]
  float* Xo;      // [G*(Ns-n), Fp]
  float* efeat;   // [G*n, S, 4]
  float* emask;   // [G*n, S]
  int Fp;
  uint32_t rcp_fp, rcp_S;   // ceil(2^32 / d): index divisions by Fp and S as one v_mul_hi_u32 (exact for idx < 2^16)
};

template <int SD>
__global__ void graph_feats_kernel(FeatArgs a) {
  extern __shared__ float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const Topo& t = a.t;
  const int g = blockIdx.x;
  const int e = g / a.n_time, tt = g - e * a.n_time;
  const int env = a.env_ids ? a.env_ids[e] : e;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = t.n, ng = t.ng, S = t.S, Fp = a.Fp;
  const int n_on = t.Ns - n - ng;
  float* s_ag = sm;                 // n*SD
  float* s_go = s_ag + n * SD;      // ng*SD
  float* s_ob = s_go + ng * SD;     // n_on * 2 (positions of hit / obstacle nodes) then MPE extra state
  float* s_fa = s_ob + n_on * SD;   // n*4
  float* s_fg = s_fa + n * 4;       // ng*4
  const float* ag = a.agent + (size_t)env * a.agent_se + (size_t)tt * a.agent_st;
  for (int i = tid; i < n * SD; i += nt) s_ag[i] = ag[i];
  for (int i = tid; i < ng * SD; i += nt) s_go[i] = a.goal[(size_t)env * ng * SD + i];
  if (n_on > 0) {
    if (t.lidar) {
      const float* hp = a.hits + (size_t)env * a.hits_se + (size_t)tt * a.hits_st;
      for (int i = tid; i < n_on * 2; i += nt) {
        const int q = i >> 1, d = i & 1;
        s_ob[q * SD + d] = hp[i];
      }
      for (int i = tid; i < n_on * (SD - 2); i += nt) {
        const int q = i / (SD - 2), d = i - q * (SD - 2);
        s_ob[q * SD + 2 + d] = 0.0f;
      }
    } else {
      for (int i = tid; i < n_on * SD; i += nt) s_ob[i] = a.obst[(size_t)env * n_on * SD + i];
    }
  }
  __syncthreads();
  for (int i = tid; i < n + ng; i += nt) {
    const float* s = (i < n) ? s_ag + i * SD : s_go + (i - n) * SD;
    float* f = (i < n) ? s_fa + i * 4 : s_fg + (i - n) * 4;
    if constexpr (SD == 5) {
      f[0] = s[0]; f[1] = s[1]; f[2] = __fmul_rn(s[4], s[2]); f[3] = __fmul_rn(s[4], s[3]);
    } else {
      f[0] = s[0]; f[1] = s[1]; f[2] = s[2]; f[3] = s[3];
    }
  }
  __syncthreads();
  // node feature rows: [state | obs, goal, agent indicator], zero padded to Fp
  constexpr int ND = SD + 3;
  for (int idx = tid; idx < t.Ns * Fp; idx += nt) {
    const int nd = (int)__umulhi((uint32_t)idx, a.rcp_fp), col = idx - nd * Fp;
    float v = 0.0f;
    if (nd < n) v = (col < SD) ? s_ag[nd * SD + col] : ((col == SD + 2) ? 1.0f : 0.0f);
    else if (nd < n + ng) v = (col < SD) ? s_go[(nd - n) * SD + col] : ((col == SD + 1) ? 1.0f : 0.0f);
    else v = (col < SD) ? s_ob[(nd - n - ng) * SD + col] : ((col == SD) ? 1.0f : 0.0f);
    if (col >= ND) v = 0.0f;
    if (nd < n) a.Xa[((size_t)g * n + nd) * Fp + col] = v;
    else a.Xo[((size_t)g * (t.Ns - n) + (nd - n)) * Fp + col] = v;
  }
  // per-slot edge feature + mask
  for (int idx = tid; idx < n * S; idx += nt) {
    const int i = (int)__umulhi((uint32_t)idx, a.rcp_S), s = idx - i * S;
    float4 f;
    bool mask;
    const float* fi = s_fa + i * 4;
    const float px = s_ag[i * SD], py = s_ag[i * SD + 1];
    if (s < n) {
      const float* fj = s_fa + s * 4;
      f = make_float4(__fsub_rn(fi[0], fj[0]), __fsub_rn(fi[1], fj[1]), __fsub_rn(fi[2], fj[2]), __fsub_rn(fi[3], fj[3]));
      float d = __fadd_rn(dist_rn(__fsub_rn(px, s_ag[s * SD]), __fsub_rn(py, s_ag[s * SD + 1])), (i == s) ? c.eye_offset : 0.0f);
      mask = d < c.comm_radius;
    } else if (s < n + t.gs) {
      const int gi = t.spread ? (s - n) : i;
      const float* fg = s_fg + gi * 4;
      f = make_float4(__fsub_rn(fi[0], fg[0]), __fsub_rn(fi[1], fg[1]), __fsub_rn(fi[2], fg[2]), __fsub_rn(fi[3], fg[3]));
      mask = true;
    } else {
      const int m = s - n - t.gs;
      if (t.lidar) {
        const float* hp = s_ob + (i * t.per + m) * SD;
        const float lx = __fsub_rn(px, hp[0]), ly = __fsub_rn(py, hp[1]);
        f = make_float4(lx, ly, 0.0f, 0.0f);
        mask = dist_rn(lx, ly) < c.lidar_mask_radius;
      } else {
        const float* xo = s_ob + m * SD;
        const float* xi = s_ag + i * SD;
        f = make_float4(__fsub_rn(xi[0], xo[0]), __fsub_rn(xi[1], xo[1]), __fsub_rn(xi[2], xo[2]), __fsub_rn(xi[3], xo[3]));
        mask = dist_rn(__fsub_rn(xi[0], xo[0]), __fsub_rn(xi[1], xo[1])) < c.obs_mask_radius;   // mpe_corridor.py:93: 100 x comm_radius
      }
    }
    reinterpret_cast<float4*>(a.efeat)[(size_t)g * n * S + idx] = f;
    a.emask[(size_t)g * n * S + idx] = mask ? 1.0f : 0.0f;
  }
}

extern "C" int32_t dgppo_graph_feats(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_se, int64_t agent_st,
                                     const float* goal, const float* obst, const float* hits, int64_t hits_se,
                                     int64_t hits_st, const int32_t* env_ids, int32_t n_env, int32_t n_time, float* Xa,
                                     float* Xo, float* efeat, float* emask, int32_t Fp, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_graph_feats", "dgppo_vmas_graph_feats");
  DGPPO_REQUIRE(n_env >= 0 && n_time >= 0, "graph_feats: negative counts");
  if (n_env == 0 || n_time == 0) return 0;
  DGPPO_REQUIRE(agent && goal && Xa && efeat && emask, "graph_feats: NULL operand");
  DGPPO_REQUIRE(Fp >= cfg->node_dim && Fp <= 32, "graph_feats: Fp must be in [node_dim, 32]");
  FeatArgs a;
  a.cfg = *cfg; a.t = make_topo(*cfg);
  const int n_on = a.t.Ns - a.t.n - a.t.ng;
  DGPPO_REQUIRE(n_on == 0 || Xo, "graph_feats: Xo is NULL");
  DGPPO_REQUIRE(a.t.Ns == a.t.n || Xo, "graph_feats: Xo is NULL");
  if (n_on > 0) {
    if (a.t.lidar) DGPPO_REQUIRE(hits, "graph_feats: hits is NULL");
    else DGPPO_REQUIRE(obst, "graph_feats: obst is NULL");
  }
  DGPPO_REQUIRE(((uintptr_t)efeat & 15) == 0, "graph_feats: efeat must be 16-byte aligned");
  a.agent = agent; a.agent_se = agent_se; a.agent_st = agent_st; a.goal = goal; a.obst = obst;
  a.hits = hits; a.hits_se = hits_se; a.hits_st = hits_st; a.env_ids = env_ids; a.n_env = n_env; a.n_time = n_time;
  a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.Fp = Fp;
  a.rcp_fp = (uint32_t)((0x100000000ull + (uint64_t)Fp - 1) / (uint64_t)Fp);
  a.rcp_S = (uint32_t)((0x100000000ull + (uint64_t)a.t.S - 1) / (uint64_t)a.t.S);
  DGPPO_REQUIRE(Fp >= 2 && a.t.S >= 2 && (long)a.t.Ns * Fp < 65536 && (long)a.t.n * a.t.S < 65536, "graph_feats: sizes out of range");
  const int SD = cfg->state_dim;
  const size_t smem = sizeof(float) * ((size_t)a.t.n * SD + a.t.ng * SD + (size_t)n_on * SD + a.t.n * 4 + a.t.ng * 4);
  const long G = (long)n_env * n_time;
  if (SD == 5) hipLaunchKernelGGL(graph_feats_kernel<5>, dim3(G), dim3(128), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(graph_feats_kernel<4>, dim3(G), dim3(128), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
