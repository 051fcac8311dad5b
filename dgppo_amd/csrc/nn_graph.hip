// Graph side of the GraphTransformer layer (dgppo/nn/gnn.py:78-117) in per-agent fixed-fan-in form.
//
// Only agents receive messages and every sender slot of an agent has a static node id (SURVEY F5/F7;
// dgppo/utils/graph.py:35-44, dgppo/env/lidar_env/lidar_spread.py:57-96), so jraph.segment_softmax / segment_sum over
// the flat edge list reduce to a masked softmax over S = n + goal_slots + obs_slots slots per agent.  Masked edges are
// re-routed pad->pad in the reference and therefore never reach an agent: here they are simply excluded.
//
// Algebraic form (same function, different summation order; see DESIGN.md "GNN layer"):
//   logit[i,s,h] = <q_h(x_i), k_h(x_s)>/sqrt(D) = qt[i,h,:] . x_s + const(i,h)   with qt = x_i Mcat + c   (dense, outside)
//   sum_s a[i,s,h] (v_h(x_s) + e_h(edge_is)) = (sum_s a[i,s,h] [x_s ; edge_is]) [Wv_h ; We_h] + bv_h   (dense, outside)
// so this file only does: graph features, logits against RAW sender features, masked softmax, aggregation of raw
// features, and the matching backward.  const(i,h) (the key bias) cancels in the softmax.
#include "graph_topo.h"

// slot through which node nd sends to agent i (or -1)
__device__ inline int slot_of(const Topo& t, int nd, int i) {
  if (nd < t.n) return nd;
  if (nd < t.n + t.ng) {
    const int g = nd - t.n;
    return t.spread ? t.n + g : (g == i ? t.n : -1);
  }
  const int q = nd - t.n - t.ng;
  if (t.lidar) return (q / t.per == i) ? t.n + t.gs + (q - i * t.per) : -1;
  return t.n + t.gs + q;
}

// The constant-one column of zcat carries sum_s a[i,s,h] b_v = b_v.  An agent without any unmasked sender slot has no
// incoming edge (aggr = 0, gnn.py:109-111), so its column is 0.  Goal slots are never masked: only topologies without them
// (VMASReverseTransport, agent slots only) have to look at the masks.
__device__ inline float ones_col(const Topo& t, const float* mrow) {
  if (t.gs > 0) return 1.0f;
  for (int s = 0; s < t.S; ++s)
    if (mrow[s] != 0.0f) return 1.0f;
  return 0.0f;
}

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

// ---------------------------------------------------------------------------------------------------------------------
// attention forward: one workgroup per graph
// ---------------------------------------------------------------------------------------------------------------------
struct AttnArgs {
  Topo t;
  int F, H, Kp;          // feature width of this layer's inputs, heads, padded width of zcat
  const float* qt;       // [G*n, H*F]
  const float* Xa;       // [G*n, F]
  const float* Xo;       // [G*(Ns-n), F]
  const float* efeat;    // [G*n, S, 4]
  const float* emask;    // [G*n, S]
  float* zcat;           // [G*n, Kp]   = [x_i | per head: sum a x_s (F), sum a e (4) | 1 | 0-pad]
  float* attn;           // [G*n, S, H]
  // backward
  const float* dzcat;    // [G*n, Kp]
  float* dqt;            // [G*n, H*F]
  float* dXa;            // [G*n, F]   (written, not accumulated) or NULL
  float* dXo;            // [G*(Ns-n), F] or NULL
  int relu_xo;           // dXo *= (Xo > 0): Xo is the ReLU output of the previous layer's update (gnn.py:109-111, aggr = 0)
  int G;
  // block-diagonal kernels only (dgppo_attn_fwd_xo / _bwd_xo): the other nodes' rows are not read but recomputed,
  // Xo = relu(Xo_raw Wo + bo) with Xo_raw [G*(Ns-n), 8] the padded raw node features (gnn.py:109-111 with aggr = 0)
  const float* Xo_raw; const float* Wo; const float* bo; int ldwo;
  // backward with recomputed rows: instead of writing dXo, every graph writes raw^T dXo [8 x 32] and colsum dXo [32] (the gradient
  // of Wo / bo through the ReLU) to dwo_slab + g * ABD_DW_STRIDE; a reduce kernel adds the slabs up
  float* dwo_slab;
  int TI;                // tiled kernels only: receivers per tile (chosen on the host from the LDS budget)
};

__global__ void __launch_bounds__(256) attn_fwd_valu_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = t.n, S = t.S, Ns = t.Ns, F = a.F, H = a.H, Fl = F + 1;
  float* s_x = sm;                      // Ns * Fl
  float* s_q = s_x + Ns * Fl;           // n * H * Fl
  float* s_e = s_q + n * H * Fl;        // n * S * 4
  float* s_m = s_e + n * S * 4;         // n * S
  float* s_a = s_m + n * S;             // n * S * H
  for (int idx = tid; idx < Ns * F; idx += nt) {
    const int nd = idx / F, f = idx - nd * F;
    s_x[nd * Fl + f] = (nd < n) ? a.Xa[((size_t)g * n + nd) * F + f] : a.Xo[((size_t)g * (Ns - n) + (nd - n)) * F + f];
  }
  for (int idx = tid; idx < n * H * F; idx += nt) {
    const int ih = idx / F, f = idx - ih * F;
    s_q[ih * Fl + f] = a.qt[(size_t)g * n * H * F + idx];
  }
  for (int idx = tid; idx < n * S * 4; idx += nt) s_e[idx] = a.efeat[(size_t)g * n * S * 4 + idx];
  for (int idx = tid; idx < n * S; idx += nt) s_m[idx] = a.emask[(size_t)g * n * S + idx];
  __syncthreads();
  // logits
  for (int idx = tid; idx < n * S * H; idx += nt) {
    const int h = idx % H, is = idx / H;
    const int i = is / S, s = is - i * S;
    const float* x = s_x + sender_node(t, i, s) * Fl;
    const float* q = s_q + (i * H + h) * Fl;
    float acc = 0.0f;
    for (int f = 0; f < F; ++f) acc = fmaf(q[f], x[f], acc);
    s_a[idx] = acc;
  }
  __syncthreads();
  // masked softmax over the slots of (i, h)   [jraph.segment_softmax: subtract max, exp, normalise]
  for (int ih = tid; ih < n * H; ih += nt) {
    const int i = ih / H, h = ih - i * H;
    float mx = -INFINITY;
    for (int s = 0; s < S; ++s)
      if (s_m[i * S + s] != 0.0f) mx = fmaxf(mx, s_a[(i * S + s) * H + h]);
    float den = 0.0f;
    for (int s = 0; s < S; ++s) {
      float ev = 0.0f;
      if (s_m[i * S + s] != 0.0f) ev = expf(s_a[(i * S + s) * H + h] - mx);
      s_a[(i * S + s) * H + h] = ev;
      den += ev;
    }
    const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
    for (int s = 0; s < S; ++s) s_a[(i * S + s) * H + h] *= inv;
  }
  __syncthreads();
  if (a.attn != nullptr)
    for (int idx = tid; idx < n * S * H; idx += nt) a.attn[(size_t)g * n * S * H + idx] = s_a[idx];
  // aggregation of raw sender / edge features
  const int W = F + 4;
  for (int idx = tid; idx < n * H * W; idx += nt) {
    const int w = idx % W, ih = idx / W;
    const int i = ih / H, h = ih - i * H;
    float acc = 0.0f;
    if (w < F) {
      for (int s = 0; s < S; ++s) {
        const float av = s_a[(i * S + s) * H + h];
        if (av != 0.0f) acc = fmaf(av, s_x[sender_node(t, i, s) * Fl + w], acc);
      }
    } else {
      // masked slots carry a == 0; their (unclamped, up to 5e5) edge features must not produce 0*inf/NaN: skip them
      for (int s = 0; s < S; ++s) {
        const float av = s_a[(i * S + s) * H + h];
        if (av != 0.0f) acc = fmaf(av, s_e[(i * S + s) * 4 + (w - F)], acc);
      }
    }
    a.zcat[((size_t)g * n + i) * a.Kp + F + h * W + w] = acc;
  }
  for (int idx = tid; idx < n * F; idx += nt) {
    const int i = idx / F, f = idx - i * F;
    a.zcat[((size_t)g * n + i) * a.Kp + f] = s_x[i * Fl + f];
  }
  const int kc = F + H * W;  // index of the constant-one column (carries mean_h b_v)
  for (int idx = tid; idx < n * (a.Kp - kc); idx += nt) {
    const int i = idx / (a.Kp - kc), c = kc + idx - i * (a.Kp - kc);
    a.zcat[((size_t)g * n + i) * a.Kp + c] = (c == kc) ? ones_col(a.t, a.emask + ((size_t)g * n + i) * a.t.S) : 0.0f;
  }
}

__global__ void __launch_bounds__(256) attn_bwd_valu_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = t.n, S = t.S, Ns = t.Ns, F = a.F, H = a.H, Fl = F + 1, W = F + 4;
  float* s_x = sm;                      // Ns * Fl
  float* s_q = s_x + Ns * Fl;           // n * H * Fl
  float* s_e = s_q + n * H * Fl;        // n * S * 4
  float* s_a = s_e + n * S * 4;         // n * S * H   attention weights
  float* s_d = s_a + n * S * H;         // n * S * H   dA then dlogit
  float* s_z = s_d + n * S * H;         // n * H * (W+1)  dz (aggregated part)
  const int Wl = W + 1;
  for (int idx = tid; idx < Ns * F; idx += nt) {
    const int nd = idx / F, f = idx - nd * F;
    s_x[nd * Fl + f] = (nd < n) ? a.Xa[((size_t)g * n + nd) * F + f] : a.Xo[((size_t)g * (Ns - n) + (nd - n)) * F + f];
  }
  for (int idx = tid; idx < n * H * F; idx += nt) {
    const int ih = idx / F, f = idx - ih * F;
    s_q[ih * Fl + f] = a.qt[(size_t)g * n * H * F + idx];
  }
  for (int idx = tid; idx < n * S * 4; idx += nt) s_e[idx] = a.efeat[(size_t)g * n * S * 4 + idx];
  for (int idx = tid; idx < n * S * H; idx += nt) s_a[idx] = a.attn[(size_t)g * n * S * H + idx];
  for (int idx = tid; idx < n * H * W; idx += nt) {
    const int w = idx % W, ih = idx / W;
    const int i = ih / H, h = ih - i * H;
    s_z[ih * Wl + w] = a.dzcat[((size_t)g * n + i) * a.Kp + F + h * W + w];
  }
  __syncthreads();
  // dA[i,s,h] = dzx[i,h,:] . x_s + dze[i,h,:] . e_is
  for (int idx = tid; idx < n * S * H; idx += nt) {
    const int h = idx % H, is = idx / H;
    const int i = is / S, s = is - i * S;
    float acc = 0.0f;
    if (s_a[idx] != 0.0f) {
      const float* x = s_x + sender_node(t, i, s) * Fl;
      const float* dz = s_z + (i * H + h) * Wl;
      for (int f = 0; f < F; ++f) acc = fmaf(dz[f], x[f], acc);
      for (int c = 0; c < 4; ++c) acc = fmaf(dz[F + c], s_e[is * 4 + c], acc);
    }
    s_d[idx] = acc;
  }
  __syncthreads();
  // softmax backward: dlogit = a * (dA - sum_s a dA)
  for (int ih = tid; ih < n * H; ih += nt) {
    const int i = ih / H, h = ih - i * H;
    float dot = 0.0f;
    for (int s = 0; s < S; ++s) dot = fmaf(s_a[(i * S + s) * H + h], s_d[(i * S + s) * H + h], dot);
    for (int s = 0; s < S; ++s) {
      const int k = (i * S + s) * H + h;
      s_d[k] = s_a[k] * (s_d[k] - dot);
    }
  }
  __syncthreads();
  // dqt[i,h,f] = sum_s dlogit[i,s,h] x_s[f]
  for (int idx = tid; idx < n * H * F; idx += nt) {
    const int f = idx % F, ih = idx / F;
    const int i = ih / H, h = ih - i * H;
    float acc = 0.0f;
    for (int s = 0; s < S; ++s) {
      const float dv = s_d[(i * S + s) * H + h];
      if (dv != 0.0f) acc = fmaf(dv, s_x[sender_node(t, i, s) * Fl + f], acc);
    }
    a.dqt[(size_t)g * n * H * F + idx] = acc;
  }
  // d x_nd[f] = sum over receivers i of sum_h (a * dzx + dlogit * qt)  (+ the direct x_i part for agents)
  if (a.dXa != nullptr) {
    for (int idx = tid; idx < Ns * F; idx += nt) {
      const int nd = idx / F, f = idx - nd * F;
      if (nd >= n && a.dXo == nullptr) continue;
      float acc = 0.0f;
      for (int i = 0; i < n; ++i) {
        const int s = slot_of(t, nd, i);
        if (s < 0) continue;
        for (int h = 0; h < H; ++h) {
          const int k = (i * S + s) * H + h;
          acc = fmaf(s_a[k], s_z[(i * H + h) * Wl + f], acc);
          acc = fmaf(s_d[k], s_q[(i * H + h) * Fl + f], acc);
        }
      }
      if (nd < n) a.dXa[((size_t)g * n + nd) * F + f] = acc + a.dzcat[((size_t)g * n + nd) * a.Kp + f];
      else a.dXo[((size_t)g * (Ns - n) + (nd - n)) * F + f] = acc;
    }
  }
}


// =====================================================================================================================
// Matrix-core attention.  Per graph (one workgroup, 4 waves) everything is a small dense product through LDS:
//   L [nH x Ns]  = Qt [nH x F] * Xs^T            logits of every (agent, head) against every node      (MFMA)
//   a            = masked softmax of L gathered at the agent's S slots                                   (half-wave shuffles)
//   P [nH x Ns]  = a scattered back to node columns (0 elsewhere)
//   Zx [nH x F]  = P * Xs                          aggregated sender features                            (MFMA)
//   ze [nH x 4]  = sum_s a * edge feature                                                                 (VALU, tiny)
// backward:  dA = dZx * Xs^T (MFMA) (+ dze . e), softmax backward, dQt = dL * Xs (MFMA),
//            dXs = P^T * dZx + dL^T * Qt (MFMA), agents also get the direct x_i part of dzcat.
// v_mfma_f32_16x16x4_f32: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15], D[row = (lane>>4)*4 + r][col = lane&15].
// Padding rows/columns of every operand are zero-filled so that they cannot leak into valid outputs.
// =====================================================================================================================
using f32x4g = __attribute__((ext_vector_type(4))) float;
#ifdef DGPPO_STAMPS
__device__ unsigned long long g_astamps[32];
#define ASTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_astamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int32_t dgppo_debug_stamps_attn(unsigned long long* out) {
  return (int32_t)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_astamps), sizeof(unsigned long long) * 32);
}
#else
#define ASTAMP(i)
#endif

struct AttnDims {
  int n, H, F, S, Ns, nH, RT, CT, Fl, Ll, W;   // RT = ceil(nH/16), CT = ceil(Ns/16), W = lanes per (agent, head) pair
};
__host__ __device__ inline AttnDims attn_dims(const Topo& t, int F, int H) {
  AttnDims d;
  d.n = t.n; d.H = H; d.F = F; d.S = t.S; d.Ns = t.Ns; d.nH = t.n * H;
  d.RT = (d.nH + 15) / 16; d.CT = (d.Ns + 15) / 16;
  d.Fl = F + 1; d.Ll = d.CT * 16 + 1; d.W = (t.S > 32) ? 64 : 32;
  return d;
}
static size_t attn_mfma_smem(const AttnDims& d, bool bwd) {
  size_t fl = (size_t)d.CT * 16 * d.Fl        // s_x   node features (rows >= Ns zero)
              + (size_t)d.RT * 16 * d.Fl      // s_q   qt (rows >= nH zero)
              + (size_t)d.RT * 16 * d.Ll      // s_L   logits -> P
              + 8 + (size_t)d.n * d.S * 5     // s_e (4, float4-aligned) + s_m (1)
              + 2 * (size_t)d.nH * ((d.S + 3) & ~3);   // compact per-pair rows (s_a, and s_c in the backward)
  if (bwd) fl += (size_t)d.RT * 16 * d.Ll     // s_D   dA -> dL (dense)
                 + (size_t)d.RT * 16 * (d.F + 5);  // s_z   dz (aggregated part), rows >= nH zero
  return fl * sizeof(float);
}

__device__ inline float red_max(float v, int W) {
  for (int o = W >> 1; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, W));
  return v;
}
__device__ inline float red_sum(float v, int W) {
  for (int o = W >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}

// C[rows x cols] (tile list dealt round-robin to the 4 waves) = A[rows x K] * B[K x cols]; element accessors are lambdas
template <typename FA, typename FB, typename FC>
__device__ inline void mfma_tiles(int RTn, int CTn, int K4, int wave, int lane, FA fa, FB fb, FC fc) {
  const int li = lane & 15, lq = lane >> 4;
  for (int tile = wave; tile < RTn * CTn; tile += 4) {
    const int rt = tile / CTn, ct = tile - rt * CTn;
    f32x4g acc = {0.f, 0.f, 0.f, 0.f};
    // fragments of 4 k-steps are fetched together (one LDS round trip), then 4 MFMAs issue back to back
    int k4 = 0;
    for (; k4 + 4 <= K4; k4 += 4) {
      float av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = fa(rt * 16 + li, (k4 + u) * 4 + lq); bv[u] = fb((k4 + u) * 4 + lq, ct * 16 + li); }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; k4 < K4; ++k4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa(rt * 16 + li, k4 * 4 + lq), fb(k4 * 4 + lq, ct * 16 + li), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) fc(rt * 16 + lq * 4 + r, ct * 16 + li, acc[r]);
  }
}


// Issue up to MAXIT float4 loads per lane back to back (all in flight together), then hand them to `put`.
template <int MAXIT, typename FL, typename FP>
__device__ inline void stage4(int count4, int tid, FL load, FP put) {
  float4 v[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int idx = tid + it * 256;
    v[it] = (idx < count4) ? load(idx) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int idx = tid + it * 256;
    if (idx < count4) put(idx, v[it]);
  }
  for (int idx = tid + MAXIT * 256; idx < count4; idx += 256) put(idx, load(idx));
}
__device__ inline void put4(float* d, float4 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }

#define ATT_SMAX 64   // max slots per agent handled by the per-pair register row

__global__ void __launch_bounds__(256) attn_fwd_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const AttnDims d = attn_dims(t, a.F, a.H);
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = d.n, S = d.S, Ns = d.Ns, F = d.F, H = d.H, Fl = d.Fl, Ll = d.Ll, nH = d.nH;
  const int Sp = (S + 3) & ~3;
  float* s_x = sm;
  float* s_q = s_x + d.CT * 16 * Fl;
  float* s_L = s_q + d.RT * 16 * Fl;
  float* s_e = sm + (((d.CT * 16 * Fl + d.RT * 16 * Fl + d.RT * 16 * Ll) + 3) & ~3);   // float4-aligned
  float* s_m = s_e + n * S * 4;
  float* s_a = s_m + n * S;               // compact [nH][Sp]: logits at the slots -> attention weights
  ASTAMP(0);
  // ---- stage operands (zero padding): every global load of the lane is issued before the first LDS store ----
  {
    const int F4 = F >> 2;
    const float4* xa = reinterpret_cast<const float4*>(a.Xa + (size_t)g * n * F);
    const float4* xo = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (Ns - n) * F);
    const float4* q4 = reinterpret_cast<const float4*>(a.qt + (size_t)g * nH * F);
    const float4* e4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
    const float* mk = a.emask + (size_t)g * n * S;
    const int nA = n * F4, nX = Ns * F4, nXp = d.CT * 16 * F4, nQ = nH * F4, nQp = d.RT * 16 * F4, nE = n * S;
    float4 vx[4], vq[2], ve[2];
    float vm[2];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int it = 0; it < 4; ++it) { const int idx = tid + it * 256; vx[it] = (idx < nA) ? xa[idx] : ((idx < nX) ? xo[idx - nA] : z4); }
#pragma unroll
    for (int it = 0; it < 2; ++it) { const int idx = tid + it * 256; vq[it] = (idx < nQ) ? q4[idx] : z4; ve[it] = (idx < nE) ? e4[idx] : z4; vm[it] = (idx < nE) ? mk[idx] : 0.0f; }
#pragma unroll
    for (int it = 0; it < 4; ++it) { const int idx = tid + it * 256; if (idx < nXp) { const int nd = idx / F4, q = idx - nd * F4; put4(s_x + nd * Fl + 4 * q, vx[it]); } }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + it * 256;
      if (idx < nQp) { const int row = idx / F4, q = idx - row * F4; put4(s_q + row * Fl + 4 * q, vq[it]); }
      if (idx < nE) { const float4 ev = ve[it]; reinterpret_cast<float4*>(s_e)[idx] = make_float4(ev.x, ev.y, ev.z, ev.w); s_m[idx] = vm[it]; }
    }
    // sizes beyond the register budget (large n): plain loops
    for (int idx = tid + 1024; idx < nXp; idx += 256) { const int nd = idx / F4, q = idx - nd * F4; put4(s_x + nd * Fl + 4 * q, (idx < nA) ? xa[idx] : ((idx < nX) ? xo[idx - nA] : z4)); }
    for (int idx = tid + 512; idx < nQp; idx += 256) { const int row = idx / F4, q = idx - row * F4; put4(s_q + row * Fl + 4 * q, (idx < nQ) ? q4[idx] : z4); }
    for (int idx = tid + 512; idx < nE; idx += 256) { reinterpret_cast<float4*>(s_e)[idx] = e4[idx]; s_m[idx] = mk[idx]; }
  }
  __syncthreads();
  ASTAMP(1);
  // ---- L = Qt * Xs^T ----
  mfma_tiles(d.RT, d.CT, F / 4, wave, lane,
             [&](int row, int k) { return s_q[row * Fl + k]; },
             [&](int k, int col) { return s_x[col * Fl + k]; },
             [&](int row, int col, float v) { s_L[row * Ll + col] = v; });
  __syncthreads();
  ASTAMP(2);
  // ---- gather the logits at the agent's slots into the compact rows (masked slots -> -inf) ----
  for (int idx = tid; idx < nH * Sp; idx += 256) {
    const int pair = idx / Sp, s = idx - pair * Sp, i = pair / H;
    float l = -INFINITY;
    if (s < S && s_m[i * S + s] != 0.0f) l = s_L[pair * Ll + sender_node(t, i, s)];
    s_a[idx] = l;
  }
  // A private LiDAR-hit row whose one slot is masked reaches nobody.  Zx = P * Xs below would still meet it as 0 * x on the
  // matrix cores, and a NaN hit point (NaN row) would poison every agent of the graph: zero the row (s_x is not read in this phase).
  if (t.lidar && t.os > 0)
    for (int q = tid >> 6; q < n * t.os; q += 4) {          // one wave per row, its lanes over the F columns
      const int i = q / t.os;
      if (s_m[i * S + n + t.gs + (q - i * t.os)] == 0.0f)
        for (int f = tid & 63; f < F; f += 64) s_x[(n + t.ng + q) * Fl + f] = 0.0f;
    }
  __syncthreads();
  ASTAMP(3);
  // ---- 8 lanes per (agent, head): softmax over the compact row (<= 8 slots per lane in registers, 3-step xor
  //      reductions) + the edge-feature aggregation; afterwards every lane helps clearing s_L for the scatter of P ----
  const int Wd = F + 4;
  float* zc = a.zcat + (size_t)g * n * a.Kp;
  for (int p0 = 0; p0 < nH; p0 += 32) {
    const int pair = p0 + (tid >> 3), sub = tid & 7;
    const bool live = pair < nH;
    const int i = live ? pair / H : 0, h = live ? pair - (pair / H) * H : 0;
    float l[ATT_SMAX / 8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < ATT_SMAX / 8; ++j) {
      const int sl = sub + 8 * j;
      l[j] = (live && sl < S) ? s_a[pair * Sp + sl] : -INFINITY;
      mx = fmaxf(mx, l[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 8)); mx = fmaxf(mx, __shfl_xor(mx, 2, 8)); mx = fmaxf(mx, __shfl_xor(mx, 4, 8));
    float den = 0.0f;
#pragma unroll
    for (int j = 0; j < ATT_SMAX / 8; ++j) {
      if (sub + 8 * j < S) { const float ev = (l[j] == -INFINITY) ? 0.0f : expf(l[j] - mx); l[j] = ev; den += ev; }
    }
    den += __shfl_xor(den, 1, 8); den += __shfl_xor(den, 2, 8); den += __shfl_xor(den, 4, 8);
    const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
#pragma unroll
    for (int j = 0; j < ATT_SMAX / 8; ++j) {
      const int sl = sub + 8 * j;
      if (live && sl < S) {
        const float av = l[j] * inv;
        s_a[pair * Sp + sl] = av;
        if (av != 0.0f) {   // masked slots may carry 5e5 / NaN edge features: skip, never multiply
          const float4 e = reinterpret_cast<const float4*>(s_e)[i * S + sl];
          z0 = fmaf(av, e.x, z0); z1 = fmaf(av, e.y, z1); z2 = fmaf(av, e.z, z2); z3 = fmaf(av, e.w, z3);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { z0 += __shfl_xor(z0, o, 8); z1 += __shfl_xor(z1, o, 8); z2 += __shfl_xor(z2, o, 8); z3 += __shfl_xor(z3, o, 8); }
    if (live && sub == 0) *reinterpret_cast<float4*>(zc + i * a.Kp + F + h * Wd + F) = make_float4(z0, z1, z2, z3);
  }
  for (int idx = tid; idx < d.RT * 16 * Ll; idx += 256) s_L[idx] = 0.0f;
  __syncthreads();
  ASTAMP(4);
  // ---- scatter P, write the attention weights ----
  for (int idx = tid; idx < n * S * H; idx += 256) {
    const int h = idx % H, is = idx / H, i = is / S, s = is - i * S;
    const float av = s_a[(i * H + h) * Sp + s];
    if (a.attn != nullptr) a.attn[(size_t)g * n * S * H + idx] = av;
    if (av != 0.0f) s_L[(i * H + h) * Ll + sender_node(t, i, s)] = av;
  }
  __syncthreads();
  ASTAMP(5);
  // ---- Zx = P * Xs, written straight into zcat; the direct x_i part and the constant column ----
  mfma_tiles(d.RT, (F + 15) / 16, d.CT * 4, wave, lane,
             [&](int row, int k) { return s_L[row * Ll + k]; },
             [&](int k, int col) { return (col < F) ? s_x[k * Fl + col] : 0.0f; },
             [&](int row, int col, float v) {
               if (row < nH && col < F) { const int i = row / H, h = row - i * H; zc[i * a.Kp + F + h * Wd + col] = v; }
             });
  for (int idx = tid; idx < n * F; idx += 256) {
    const int i = idx / F, f = idx - i * F;
    zc[i * a.Kp + f] = s_x[i * Fl + f];
  }
  const int kc = F + H * Wd;
  for (int idx = tid; idx < n * (a.Kp - kc); idx += 256) {
    const int i = idx / (a.Kp - kc), c = kc + idx - i * (a.Kp - kc);
    zc[i * a.Kp + c] = (c == kc) ? ones_col(t, a.emask + ((size_t)g * n + i) * S) : 0.0f;
  }
  ASTAMP(6);
}

// reductions over the 8 lanes that own an (agent, head) pair: DPP moves inside the VALU (quad swaps, then the mirror of
// the 8-lane half row); every lane of the group ends with the result.  __shfl_xor(width 8) would be 3 LDS-crossbar round
// trips per reduction.
template <int CTRL> __device__ inline float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ inline float grp8_sum(float v) {
  v += dpp_f<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);    // row_half_mirror
  return v;
}
__device__ inline float grp8_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  return v;
}

// ---- narrow layers (F = 8: the first GNN layer, node features padded 7 -> 8): slot-sparse VALU kernels ---------------
// With 8 features a dense [n*H x nodes] logit tile on the matrix cores computes 3.3x more products than the S slots of
// an agent need (24 of 80 nodes for LidarSpread n = 8) and needs three dependent memory round trips per graph (operands
// -> logits through LDS -> P -> aggregation).  Here one wave owns a graph and a group of 8 lanes owns an AGENT: every
// lane loads the sender rows / edge features / masks of its SJ slots STRAIGHT from global memory, once for all heads
// (sender ids are static, so every address is known at entry: ONE memory round trip per graph), forms its H * SJ logits
// with 8 FMAs each, and the per-(agent, head) reductions are DPP row operations.  No LDS, no matrix cores, ~1/3 of the
// instructions and of the L1 requests; sums run over slots in a different order than the dense form (tests: 1e-5).
// NPA = ceil(n / 8) passes over groups of 8 agents.
template <int H, int NPA, int SJ>
__global__ void __launch_bounds__(256) attn_fwd_slot8_kernel(AttnArgs a) {
  constexpr int F = 8, Wd = F + 4;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
  const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (g >= a.G) return;
  const int n = t.n, S = t.S, Ns = t.Ns, Kp = a.Kp, kc = F + H * Wd;
  const float* Xa = a.Xa + (size_t)g * n * F;
  const float* Xo = a.Xo + (size_t)g * (Ns - n) * F - (size_t)n * F;   // indexed by node id (>= n)
  const float* qt = a.qt + (size_t)g * n * H * F;
  const float* ef = a.efeat + (size_t)g * n * S * 4;
  const float* mk = a.emask + (size_t)g * n * S;
  float* zc = a.zcat + (size_t)g * n * Kp;
  float* at = a.attn + (size_t)g * n * S * H;
  // the parts of zcat that are plain copies: x_i, the constant column, zero padding
  for (int idx = lane; idx < n * 2; idx += 64)
    *reinterpret_cast<float4*>(zc + (idx >> 1) * Kp + 4 * (idx & 1)) = reinterpret_cast<const float4*>(Xa)[idx];
  for (int i = lane; i < n; i += 64)
    for (int c = kc; c < Kp; ++c) zc[i * Kp + c] = (c == kc) ? ones_col(a.t, mk + i * S) : 0.0f;
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int ia = grp + 8 * p;
    const bool live = ia < n;
    const int i = live ? ia : n - 1;
    float4 q[H][2], x[SJ][2], e[SJ];
    float m[SJ];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float4* qp = reinterpret_cast<const float4*>(qt + (i * H + h) * F);
      q[h][0] = qp[0]; q[h][1] = qp[1];
    }
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
      int sl = sub + 8 * j;
      sl = sl < S ? sl : S - 1;
      const int nd = sender_node(t, i, sl);
      const float4* xp = reinterpret_cast<const float4*>((nd < n ? Xa : Xo) + (size_t)nd * F);
      x[j][0] = xp[0]; x[j][1] = xp[1];
      e[j] = reinterpret_cast<const float4*>(ef)[i * S + sl];
      m[j] = mk[i * S + sl];
    }
    float av[SJ][H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        const bool ok = live && (sub + 8 * j) < S && m[j] != 0.0f;
        float acc = q[h][0].x * x[j][0].x;
        acc = fmaf(q[h][0].y, x[j][0].y, acc); acc = fmaf(q[h][0].z, x[j][0].z, acc); acc = fmaf(q[h][0].w, x[j][0].w, acc);
        acc = fmaf(q[h][1].x, x[j][1].x, acc); acc = fmaf(q[h][1].y, x[j][1].y, acc);
        acc = fmaf(q[h][1].z, x[j][1].z, acc); acc = fmaf(q[h][1].w, x[j][1].w, acc);
        av[j][h] = ok ? acc : -INFINITY;
        mx = fmaxf(mx, av[j][h]);
      }
      mx = grp8_max(mx);
      float den = 0.0f;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        const float ev = (av[j][h] == -INFINITY) ? 0.0f : __expf(av[j][h] - mx);   /* v_exp_f32: rel. error ~1e-7 on weights <= 1 */
        av[j][h] = ev;
        den += ev;
      }
      den = grp8_sum(den);
      const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
#pragma unroll
      for (int j = 0; j < SJ; ++j) av[j][h] *= inv;
    }
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
      const int sl = sub + 8 * j;
      if (live && sl < S) {
#pragma unroll
        for (int h = 0; h < H; ++h) if (a.attn != nullptr) at[(i * S + sl) * H + h] = av[j][h];
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float z[Wd];
#pragma unroll
      for (int c = 0; c < Wd; ++c) z[c] = 0.0f;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        const float w = av[j][h];
        if (w != 0.0f) {   // masked slots (and dead lanes) have w == 0; they may carry 5e5 / NaN features: skip, never multiply
          z[0] = fmaf(w, x[j][0].x, z[0]); z[1] = fmaf(w, x[j][0].y, z[1]); z[2] = fmaf(w, x[j][0].z, z[2]); z[3] = fmaf(w, x[j][0].w, z[3]);
          z[4] = fmaf(w, x[j][1].x, z[4]); z[5] = fmaf(w, x[j][1].y, z[5]); z[6] = fmaf(w, x[j][1].z, z[6]); z[7] = fmaf(w, x[j][1].w, z[7]);
          z[8] = fmaf(w, e[j].x, z[8]); z[9] = fmaf(w, e[j].y, z[9]); z[10] = fmaf(w, e[j].z, z[10]); z[11] = fmaf(w, e[j].w, z[11]);
        }
      }
#pragma unroll
      for (int c = 0; c < Wd; ++c) z[c] = grp8_sum(z[c]);
      if (live && sub == h) {             // lane h of the group stores head h: the stores of the H heads go out together
        float4* o = reinterpret_cast<float4*>(zc + i * Kp + F + h * Wd);   // (F + h*Wd) % 4 == 0 and Kp % 4 == 0
        o[0] = make_float4(z[0], z[1], z[2], z[3]);
        o[1] = make_float4(z[4], z[5], z[6], z[7]);
        o[2] = make_float4(z[8], z[9], z[10], z[11]);
      }
    }
  }
}

// backward of the above for the first layer, whose inputs are raw features (no dXa / dXo): dqt only.
//   dA = dzx . x_s + dze . e  at the slots with a != 0;  dl = a (dA - sum_s a dA);  dqt[i,h,:] = sum_s dl x_s
template <int H, int NPA, int SJ>
__global__ void __launch_bounds__(256) attn_bwd_slot8_kernel(AttnArgs a) {
  constexpr int F = 8, Wd = F + 4;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
  const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (g >= a.G) return;
  const int n = t.n, S = t.S, Ns = t.Ns, Kp = a.Kp;
  const float* Xa = a.Xa + (size_t)g * n * F;
  const float* Xo = a.Xo + (size_t)g * (Ns - n) * F - (size_t)n * F;
  const float* ef = a.efeat + (size_t)g * n * S * 4;
  const float* at = a.attn + (size_t)g * n * S * H;
  const float* dzc = a.dzcat + (size_t)g * n * Kp;
  float* dq = a.dqt + (size_t)g * n * H * F;
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int ia = grp + 8 * p;
    const bool live = ia < n;
    const int i = live ? ia : n - 1;
    float4 dz[H][3], x[SJ][2], e[SJ];
    float av[SJ][H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float4* zp = reinterpret_cast<const float4*>(dzc + i * Kp + F + h * Wd);
      dz[h][0] = zp[0]; dz[h][1] = zp[1]; dz[h][2] = zp[2];
    }
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
      int sl = sub + 8 * j;
      const bool in = live && sl < S;
      sl = sl < S ? sl : S - 1;
      const int nd = sender_node(t, i, sl);
      const float4* xp = reinterpret_cast<const float4*>((nd < n ? Xa : Xo) + (size_t)nd * F);
      x[j][0] = xp[0]; x[j][1] = xp[1];
      e[j] = reinterpret_cast<const float4*>(ef)[i * S + sl];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float w = at[(i * S + sl) * H + h];
        av[j][h] = in ? w : 0.0f;
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float dA[SJ];
      float dot = 0.0f;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        float acc = 0.0f;
        if (av[j][h] != 0.0f) {               // masked slots may carry 5e5 / NaN features: skip, never multiply
          acc = dz[h][0].x * x[j][0].x;
          acc = fmaf(dz[h][0].y, x[j][0].y, acc); acc = fmaf(dz[h][0].z, x[j][0].z, acc); acc = fmaf(dz[h][0].w, x[j][0].w, acc);
          acc = fmaf(dz[h][1].x, x[j][1].x, acc); acc = fmaf(dz[h][1].y, x[j][1].y, acc);
          acc = fmaf(dz[h][1].z, x[j][1].z, acc); acc = fmaf(dz[h][1].w, x[j][1].w, acc);
          acc = fmaf(dz[h][2].x, e[j].x, acc); acc = fmaf(dz[h][2].y, e[j].y, acc);
          acc = fmaf(dz[h][2].z, e[j].z, acc); acc = fmaf(dz[h][2].w, e[j].w, acc);
          dot = fmaf(av[j][h], acc, dot);
        }
        dA[j] = acc;
      }
      dot = grp8_sum(dot);
      float o[F];
#pragma unroll
      for (int c = 0; c < F; ++c) o[c] = 0.0f;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        if (av[j][h] != 0.0f) {
          const float dl = av[j][h] * (dA[j] - dot);
          o[0] = fmaf(dl, x[j][0].x, o[0]); o[1] = fmaf(dl, x[j][0].y, o[1]); o[2] = fmaf(dl, x[j][0].z, o[2]); o[3] = fmaf(dl, x[j][0].w, o[3]);
          o[4] = fmaf(dl, x[j][1].x, o[4]); o[5] = fmaf(dl, x[j][1].y, o[5]); o[6] = fmaf(dl, x[j][1].z, o[6]); o[7] = fmaf(dl, x[j][1].w, o[7]);
        }
      }
#pragma unroll
      for (int c = 0; c < F; ++c) o[c] = grp8_sum(o[c]);
      if (live && sub == h) {
        float4* op = reinterpret_cast<float4*>(dq + (i * H + h) * F);
        op[0] = make_float4(o[0], o[1], o[2], o[3]);
        op[1] = make_float4(o[4], o[5], o[6], o[7]);
      }
    }
  }
}

template <int H, int NPA>
static bool launch_attn_slot8_sj(const AttnArgs& a, int SJ, int grid, hipStream_t s, bool bwd) {
#define DGPPO_SJ(J)                                                                                              \
  case J:                                                                                                        \
    if (bwd) hipLaunchKernelGGL((attn_bwd_slot8_kernel<H, NPA, J>), dim3(grid), dim3(256), 0, s, a);             \
    else hipLaunchKernelGGL((attn_fwd_slot8_kernel<H, NPA, J>), dim3(grid), dim3(256), 0, s, a);                 \
    return true;
  switch (SJ) {
    DGPPO_SJ(1) DGPPO_SJ(2) DGPPO_SJ(3) DGPPO_SJ(4) DGPPO_SJ(5) DGPPO_SJ(6) DGPPO_SJ(7) DGPPO_SJ(8)
    default: return false;
  }
#undef DGPPO_SJ
}
// H = 3 heads (the reference's GraphTransformer default, dgppo/nn/gnn.py:81), n <= 32 agents, S <= 64 slots
static bool attn_slot8_shape(const Topo& t, int F, int H) { return F == 8 && H == 3 && t.n <= 32 && t.S <= 64; }
static bool launch_attn_slot8(const AttnArgs& a, hipStream_t s, bool bwd) {
  if (!attn_slot8_shape(a.t, a.F, a.H)) return false;
  const int grid = (a.G + 3) / 4, NPA = (a.t.n + 7) / 8, SJ = (a.t.S + 7) / 8;
  switch (NPA) {
    case 1: return launch_attn_slot8_sj<3, 1>(a, SJ, grid, s, bwd);
    case 2: return launch_attn_slot8_sj<3, 2>(a, SJ, grid, s, bwd);
    case 3: return launch_attn_slot8_sj<3, 3>(a, SJ, grid, s, bwd);
    case 4: return launch_attn_slot8_sj<3, 4>(a, SJ, grid, s, bwd);
    default: return false;
  }
}

// ---- F = 32, block-diagonal form (one wave per graph) -----------------------------------------------------------
// A dense [n*H x nodes] logit tile (the workgroup MFMA kernels) is mostly wasted work: an agent only attends to the nodes
// every agent sees (agents, goals: "shared") and to its OWN 8 LiDAR hit nodes, so 4/5 of the tile's columns (LidarSpread
// n = 8: 64 of 80) are used by one agent in eight.  Here the wave is laid out as 8 lanes per AGENT (il = lane / 8, sub = lane & 7):
//   * lane (il, sub) owns, for every head, the slots  {shared node p * 8 + sub, p < PS}  and  {hit sub}  of agent il, i.e.
//     all S slots of an agent live in its 8 lanes (PS + 1 registers per head) and the softmax is a register / DPP matter;
//   * all products run on the matrix cores as v_mfma_f32_4x4x1 (16 independent 4x4 blocks, one k per instruction): block
//     (il, g2 = bit 2 of the lane), A rows = the 4 heads of agent il, B columns = 4 nodes (logits, dA) or 4 feature quads
//     (aggregation, dQt).  A block only ever multiplies what its agent needs: 96 + 96 small MFMAs (1.5 k SIMD cycles) per
//     graph forward instead of the dense tile's 160 16x16x4 tiles (5.1 k), 2.7 k instead of 10.2 k backward;
//   * every global row is read ONCE, as coalesced 16-byte pieces, into a padded LDS image (shared rows, the 64 hit rows of
//     the agent batch, query / dZ rows) from which all operand layouts are read (a dense one-wave form that re-read the
//     node rows from global memory per layout moved 2.4x the algorithmic bytes, profiles/r03_nn_counters.json).
// More than 8 agents: batches of 8 agents run one after the other over the same staged shared rows.
// Requirements (attn_bd_shape): F = 32, H <= 4, LiDAR hits 8 per agent (or no private nodes at all), at most
// 32 shared nodes.  Same arithmetic as gnn.py:85-117 up to the summation order.
#define ABD_XL 36                      // LDS row stride of a staged 32-float row (16-byte aligned, conflict-free b128 row reads)
#define ABD_DZL 40                     // the staged dZ rows carry the 4 edge-feature gradients behind the 32 features
typedef float4 abd_f4;
__device__ inline f32x4g mfma4(float a_, float b_, f32x4g c_) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a_, b_, c_, 0, 0, 0); }
__device__ inline const float* f4e(const float4& v) { return reinterpret_cast<const float*>(&v); }
__device__ inline float4 ld4_if(bool ok, const float4* p) {      // predicated 16-byte load, zeros otherwise
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) v = *p;
  return v;
}

// An opaque zero that DEPENDS on loaded values (v_and_b32 with 0 behind an asm the optimiser cannot see through): added to the
// LDS addresses of the staging writes it ties the loads of the small operands (masks, edge features, attention weights ...)
// to the first trip to memory.  Left alone the scheduler sinks them into the first MFMA phase and the wave pays a second trip;
// a side-effecting fence (sched_barrier, asm volatile) at that place makes the compiler keep the staging arrays in scratch.
__device__ inline int opaque_zero(int bits) {
  asm("v_and_b32 %0, 0, %0" : "+v"(bits));
  return bits;
}
__device__ inline int f4bits(const float4& v) { return __float_as_int(v.x) | __float_as_int(v.y) | __float_as_int(v.z) | __float_as_int(v.w); }

template <int PS, bool HITS> struct AbdLds {
  static constexpr int NSP = PS * 8, PC = NSP + (HITS ? 8 : 0), PL = PC + 4;
  static constexpr int XS = NSP * ABD_XL, XH = HITS ? 64 * ABD_XL + 64 : 0;
  static constexpr int QP = (32 * ABD_XL > 32 * PL) ? 32 * ABD_XL : 32 * PL;      // query rows, later the P tile [32][PL]
  static constexpr int FWD = XS + XH + QP;
  static constexpr int DZ = 32 * ABD_DZL, PTL = NSP + 1, PT = 32 * PTL, DL = 32 * PL;
  static constexpr int BWD = XS + XH + DZ + PT + DL;
};

// ---- other nodes recomputed in the kernel (XOF variants) ----
// Goals, LiDAR hits and obstacles receive no messages, so their layer-1 features are relu(x W_u[:8] + b_u) of the 8 raw
// features (gnn.py:109-111 with aggr = 0).  Materialised, those rows are 9 KB of the 19 KB a graph's forward moves (and are
// written once and read again by the backward); here the wave reads the 32-byte raw rows and forms the 16-row x 32 tiles on
// the matrix cores (2 k-steps x 2 column tiles of 16x16x4 per 16 rows) straight into the LDS images.
#define ABD_KR 8
#define ABD_DW_STRIDE 320              // 8 x 32 (dWo) + 32 (dbo), rounded to 64 floats
template <int GT> struct AbdXoRegs { float ag[GT][2], ah[4][2], wo[2][2], bo[2]; };
// request the A fragments: row li of each 16-row tile, raw feature lq + 4 s
template <int GT, bool HITS>
__device__ inline void abd_xo_load(AbdXoRegs<GT>& x, const AttnArgs& a, const float* raw, int n_shared_other, int ng, int hit0,
                                   int n_hits, int li, int lq, bool first) {
  if (first) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) x.wo[s_][ct] = a.Wo[(lq + 4 * s_) * a.ldwo + ct * 16 + li];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) x.bo[ct] = a.bo[ct * 16 + li];
#pragma unroll
    for (int t = 0; t < GT; ++t) {
      int o = t * 16 + li;
      o = o < n_shared_other ? o : n_shared_other - 1;
      o = o < 0 ? 0 : o;
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) x.ag[t][s_] = raw[o * ABD_KR + lq + 4 * s_];
    }
  }
  if constexpr (HITS) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int hb = hit0 + t * 16 + li;
      hb = hb < n_hits ? hb : n_hits - 1;
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) x.ah[t][s_] = raw[(ng + hb) * ABD_KR + lq + 4 * s_];
    }
  }
}
// tiles -> LDS images (C/D layout: row lq * 4 + r, column ct * 16 + li)
template <int GT, bool HITS>
__device__ inline void abd_xo_emit(const AbdXoRegs<GT>& x, float* XS, float* XH, int n, int n_shared_other, int li, int lq, bool first) {
  auto tile = [&](const float (&ar)[2], f32x4g (&v)[2]) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      v[ct] = f32x4g{0.f, 0.f, 0.f, 0.f};
      v[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[0], x.wo[0][ct], v[ct], 0, 0, 0);
      v[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[1], x.wo[1][ct], v[ct], 0, 0, 0);
    }
  };
  if (first) {
#pragma unroll
    for (int t = 0; t < GT; ++t) {
      f32x4g v[2];
      tile(x.ag[t], v);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = t * 16 + lq * 4 + r;
          if (o < n_shared_other) XS[(n + o) * ABD_XL + ct * 16 + li] = relu_nan(v[ct][r] + x.bo[ct]);
        }
    }
  }
  if constexpr (HITS) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4g v[2];
      tile(x.ah[t], v);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int hr = t * 16 + lq * 4 + r;
          XH[hr * ABD_XL + (hr >> 3) * 8 + ct * 16 + li] = relu_nan(v[ct][r] + x.bo[ct]);
        }
    }
  }
}
template <int GT> __device__ inline int abd_xo_bits(const AbdXoRegs<GT>& x, bool hits) {
  int b = 0;
#pragma unroll
  for (int t = 0; t < GT; ++t) b |= __float_as_int(x.ag[t][0]) | __float_as_int(x.ag[t][1]);
  if (hits) {
#pragma unroll
    for (int t = 0; t < 4; ++t) b |= __float_as_int(x.ah[t][0]) | __float_as_int(x.ah[t][1]);
  }
  b |= __float_as_int(x.wo[0][0]) | __float_as_int(x.wo[0][1]) | __float_as_int(x.wo[1][0]) | __float_as_int(x.wo[1][1]);
  b |= __float_as_int(x.bo[0]) | __float_as_int(x.bo[1]);
  return b;
}

template <int PS, bool HITS, int AB, bool XOF>
__global__ void __launch_bounds__(128) attn_fwd_bd_kernel(AttnArgs a) {
  extern __shared__ float4 abd_sm[];
  using L = AbdLds<PS, HITS>;
  constexpr int F = 32, NSP = L::NSP, PC = L::PC, PL = L::PL, NPR = PS + (HITS ? 1 : 0), Wd = F + 4;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * 2 + wave);
  if (g >= a.G) return;                                        // no barriers below
  const int n = t.n, S = t.S, Ns = t.Ns, H = a.H, Kp = a.Kp;
  const int NSH = HITS ? t.n + t.ng : Ns;
  const int kc = F + H * Wd;
  float* XS = reinterpret_cast<float*>(abd_sm) + wave * L::FWD;
  float* XH = XS + L::XS;
  float* QP = XH + L::XH;
  const float4* Xa4 = reinterpret_cast<const float4*>(a.Xa + (size_t)g * n * F);
  const float4* Xo4 = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (Ns - n) * F);
  const float4* qt4 = reinterpret_cast<const float4*>(a.qt + (size_t)g * n * H * F);
  float* zc = a.zcat + (size_t)g * n * Kp;
  const int il = lane >> 3, sub = lane & 7, g2 = (lane >> 2) & 1, c = lane & 3, hA = lane & 3;
  ASTAMP(0);
  // ---- every global read is requested before anything waits: rows are fetched unconditionally from clamped addresses (a
  //      pad row duplicates a real one; it only ever meets zeros of P), so there is no branch around a load and the wave
  //      makes ONE trip to memory per agent batch ----
  float4 vs[PS];
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    const int row = p * 8 + il;
    const int ra = row < n ? row : n - 1, ro = (row < NSH ? row : NSH - 1) - n;
    const float4* src = (XOF || row < n || NSH == n) ? Xa4 + ra * 8 + sub : Xo4 + ro * 8 + sub;
    vs[p] = *src;
  }
  constexpr int GT = (NSP + 15) / 16;
  AbdXoRegs<GT> xo;
  const float* raw = XOF ? a.Xo_raw + (size_t)g * (Ns - n) * ABD_KR : nullptr;
  const int li_ = lane & 15, lq_ = lane >> 4;
  const float* mk = a.emask + (size_t)g * n * S;
  const float4* ef4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
  float* at = a.attn + (size_t)g * n * S * H;
#pragma unroll
  for (int ab = 0; ab < AB; ++ab) {       // AB = ceil(n / 8), a compile-time count: straight-line code, every array in registers
    const int i = ab * 8 + il;
    const bool live = i < n;
    const int ic = live ? i : n - 1;
    float4 vh[HITS ? 8 : 1], vq[4];
    if constexpr (XOF) abd_xo_load<GT, HITS>(xo, a, raw, NSH - n, t.ng, ab * 64, n * 8, li_, lq_, ab == 0);
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int hb = ab * 64 + k * 8 + il;
        hb = hb < n * 8 ? hb : n * 8 - 1;
        vh[k] = Xo4[(t.ng + hb) * 8 + sub];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = k * 8 + il;
      int ri = ab * 8 + (row >> 2), rh = row & 3;
      ri = ri < n ? ri : n - 1; rh = rh < H ? rh : H - 1;
      vq[k] = qt4[(ri * H + rh) * 8 + sub];
    }
    // the lane's slots: mask and edge features
    int slot[NPR];
    float mkv[NPR];
    float4 efv[NPR];
#pragma unroll
    for (int p = 0; p < NPR; ++p) {
      int sl;
      if (HITS && p == PS) sl = n + t.gs + sub;
      else { const int j = p * 8 + sub; sl = (j < NSH) ? slot_of(t, j, ic) : -1; }
      slot[p] = live ? sl : -1;
      const int sc = sl < 0 ? 0 : sl;
      mkv[p] = mk[ic * S + sc];
      efv[p] = ef4[ic * S + sc];
    }
    ASTAMP(1);
    int pin = 0;
#pragma unroll
    for (int p = 0; p < NPR; ++p) pin |= __float_as_int(mkv[p]) | f4bits(efv[p]);
    if constexpr (XOF) pin |= abd_xo_bits<GT>(xo, HITS);
    const int pin0 = opaque_zero(pin);
    if (ab == 0) {
#pragma unroll
      for (int p = 0; p < PS; ++p) {
        float4 v = vs[p];
        if (XOF && p * 8 + il >= n) v = make_float4(0.f, 0.f, 0.f, 0.f);       // pad rows stay zero, the others are recomputed below
        *reinterpret_cast<float4*>(XS + pin0 + (p * 8 + il) * ABD_XL + sub * 4) = v;
      }
    }
    if constexpr (XOF) abd_xo_emit<GT, HITS>(xo, XS + pin0, XH + pin0, n, NSH - n, li_, lq_, ab == 0);
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + pin0 + (k * 8 + il) * ABD_XL + k * 8 + sub * 4) = vh[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(QP + pin0 + (k * 8 + il) * ABD_XL + sub * 4) = vq[k];
#pragma unroll
    for (int p = 0; p < NPR; ++p) mkv[p] = (slot[p] >= 0) ? mkv[p] : 0.0f;
    if constexpr (HITS) {
      // The lane's own hit row reaches nobody when its slot is masked, but Zx = P Xs would still meet it as 0 * x on the matrix
      // cores (a NaN hit point: NaN row): the owner zeroes it.  DS operations of a wave execute in order: after the staging above.
      if (mkv[PS] == 0.0f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + lane * ABD_XL + il * 8 + k * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    ASTAMP(2);
    // ---- logits: A = the query row of (agent il, head hA), B = the lane's own node rows ----
    f32x4g acc[NPR];
#pragma unroll
    for (int p = 0; p < NPR; ++p) acc[p] = f32x4g{0.f, 0.f, 0.f, 0.f};
    {
      const float* qrow = QP + (il * 4 + hA) * ABD_XL;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float4 q = *reinterpret_cast<const float4*>(qrow + k * 4);
        float4 x[NPR];
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          if (HITS && p == PS) x[p] = *reinterpret_cast<const float4*>(XH + lane * ABD_XL + il * 8 + k * 4);
          else x[p] = *reinterpret_cast<const float4*>(XS + (p * 8 + sub) * ABD_XL + k * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < NPR; ++p) acc[p] = mfma4(f4e(q)[u], f4e(x[p])[u], acc[p]);
      }
    }
    ASTAMP(3);
    // ---- masked softmax per head over the 8 lanes x NPR registers of the agent; edge aggregation; P -> LDS ----
    float* PT = QP;                                            // DS operations of a wave execute in order: the query rows are read
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (h < H) {
        float l[NPR];
        float mx = -INFINITY;
#pragma unroll
        for (int p = 0; p < NPR; ++p) { l[p] = (mkv[p] != 0.0f) ? acc[p][h] : -INFINITY; mx = fmaxf(mx, l[p]); }
        mx = grp8_max(mx);
        float den = 0.0f;
#pragma unroll
        for (int p = 0; p < NPR; ++p) { l[p] = (l[p] == -INFINITY) ? 0.0f : __expf(l[p] - mx); den += l[p]; }
        den = grp8_sum(den);
        const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
        float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          const float av = l[p] * inv;
          acc[p][h] = av;
          if (slot[p] >= 0) {
            if (a.attn != nullptr) at[(i * S + slot[p]) * H + h] = av;
            if (av != 0.0f) {   // masked slots may carry 5e5 / NaN edge features: skip, never multiply
              const float4 e = efv[p];
              z0 = fmaf(av, e.x, z0); z1 = fmaf(av, e.y, z1); z2 = fmaf(av, e.z, z2); z3 = fmaf(av, e.w, z3);
            }
          }
        }
        z0 = grp8_sum(z0); z1 = grp8_sum(z1); z2 = grp8_sum(z2); z3 = grp8_sum(z3);
        if (live && sub == 0) *reinterpret_cast<float4*>(zc + i * Kp + F + h * Wd + F) = make_float4(z0, z1, z2, z3);
      } else {
#pragma unroll
        for (int p = 0; p < NPR; ++p) acc[p][h] = 0.0f;
      }
#pragma unroll
      for (int p = 0; p < NPR; ++p) PT[(il * 4 + h) * PL + p * 8 + sub] = acc[p][h];
    }
    ASTAMP(4);
    // ---- Zx = P Xs: A = row (il, hA) of P, B = feature quad (g2 * 4 + c) of the node of the k-step ----
    {
      float pa[PC];
#pragma unroll
      for (int k = 0; k < PC / 4; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(PT + (il * 4 + hA) * PL + k * 4);
        pa[k * 4] = v.x; pa[k * 4 + 1] = v.y; pa[k * 4 + 2] = v.z; pa[k * 4 + 3] = v.w;
      }
      f32x4g az[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) az[q] = f32x4g{0.f, 0.f, 0.f, 0.f};
      const int fq = (g2 * 4 + c) * 4;
#pragma unroll
      for (int kk = 0; kk < NSP; ++kk) {
        const float4 b = *reinterpret_cast<const float4*>(XS + kk * ABD_XL + fq);
#pragma unroll
        for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[kk], f4e(b)[q], az[q]);
      }
      if constexpr (HITS) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float4 b = *reinterpret_cast<const float4*>(XH + (il * 8 + m) * ABD_XL + il * 8 + fq);
#pragma unroll
          for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[NSP + m], f4e(b)[q], az[q]);
        }
      }
      if (live) {
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (h < H) *reinterpret_cast<float4*>(zc + i * Kp + F + h * Wd + fq) = make_float4(az[0][h], az[1][h], az[2][h], az[3][h]);
      }
    }
  }
  ASTAMP(5);
  // the parts of zcat that are plain copies: x_i (from its staged image), the constant column, zero padding
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    const int row = p * 8 + il;
    if (row < n) *reinterpret_cast<float4*>(zc + row * Kp + sub * 4) = *reinterpret_cast<const float4*>(XS + row * ABD_XL + sub * 4);
  }
  {
    const int wpad = Kp - kc;                                  // >= 1: the constant column, then zeros
    for (int i = lane; i < n; i += 64)
      for (int cc = 0; cc < wpad; ++cc) zc[i * Kp + kc + cc] = (cc == 0) ? ones_col(a.t, mk + i * S) : 0.0f;
  }
  ASTAMP(6);
}

// ---- the same forward with PERSISTENT waves and the next graph's loads in flight (n <= 8: one agent batch) ----------------
// A third of a wave's time per graph is the wait for its one trip to memory (in-kernel stamps: 6.7 k of 21 k cycles) and LDS
// limits a CU to 10 of these waves, so that wait is not hidden.  Here a wave walks graphs g, g + W, g + 2 W, ...; the loads of
// the next graph are requested right after the current one's rows are staged and land during its MFMA / softmax phases (+55
// registers: 8 instead of 10 waves per CU).  Launches of up to twice the resident waves keep the kernel above (rollouts).
template <int PS, bool HITS, bool XOF>
struct AbdFwdRegs {
  float4 vs[PS], vq[4], vh[(HITS && !XOF) ? 8 : 1];
  AbdXoRegs<(PS * 8 + 15) / 16> xo;
  float mkv[PS + (HITS ? 1 : 0)];
  float4 efv[PS + (HITS ? 1 : 0)];
};
template <int PS, bool HITS, bool XOF>
__global__ void __launch_bounds__(128) attn_fwd_bdp_kernel(AttnArgs a) {
  extern __shared__ float4 abd_sm[];
  using L = AbdLds<PS, HITS>;
  constexpr int F = 32, NSP = L::NSP, PC = L::PC, PL = L::PL, NPR = PS + (HITS ? 1 : 0), Wd = F + 4, GT = (NSP + 15) / 16;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int g = __builtin_amdgcn_readfirstlane(blockIdx.x * 2 + wave);
  const int stride = gridDim.x * 2;
  if (g >= a.G) return;                                        // no barriers below
  const int n = t.n, S = t.S, Ns = t.Ns, H = a.H, Kp = a.Kp;
  const int NSH = HITS ? t.n + t.ng : Ns;
  const int kc = F + H * Wd;
  float* XS = reinterpret_cast<float*>(abd_sm) + wave * L::FWD;
  float* XH = XS + L::XS;
  float* QP = XH + L::XH;
  const int il = lane >> 3, sub = lane & 7, g2 = (lane >> 2) & 1, c = lane & 3, hA = lane & 3;
  const int li_ = lane & 15, lq_ = lane >> 4;
  const int i = il;
  const bool live = i < n;
  const int ic = live ? i : n - 1;
  // the lane's slots do not depend on the graph
  int slot[NPR], sc[NPR];
#pragma unroll
  for (int p = 0; p < NPR; ++p) {
    int sl;
    if (HITS && p == PS) sl = n + t.gs + sub;
    else { const int j = p * 8 + sub; sl = (j < NSH) ? slot_of(t, j, ic) : -1; }
    slot[p] = live ? sl : -1;
    sc[p] = sl < 0 ? 0 : sl;
  }
  using Regs = AbdFwdRegs<PS, HITS, XOF>;
  auto load = [&](int gg, Regs& R) {
    const float4* Xa4 = reinterpret_cast<const float4*>(a.Xa + (size_t)gg * n * F);
    const float4* Xo4 = reinterpret_cast<const float4*>(a.Xo + (size_t)gg * (Ns - n) * F);
    const float4* qt4 = reinterpret_cast<const float4*>(a.qt + (size_t)gg * n * H * F);
#pragma unroll
    for (int p = 0; p < PS; ++p) {
      const int row = p * 8 + il;
      const int ra = row < n ? row : n - 1, ro = (row < NSH ? row : NSH - 1) - n;
      const float4* src = (XOF || row < n || NSH == n) ? Xa4 + ra * 8 + sub : Xo4 + ro * 8 + sub;
      R.vs[p] = *src;
    }
    if constexpr (XOF) abd_xo_load<GT, HITS>(R.xo, a, a.Xo_raw + (size_t)gg * (Ns - n) * ABD_KR, NSH - n, t.ng, 0, n * 8, li_, lq_, true);
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int hb = k * 8 + il;
        hb = hb < n * 8 ? hb : n * 8 - 1;
        R.vh[k] = Xo4[(t.ng + hb) * 8 + sub];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = k * 8 + il;
      int ri = row >> 2, rh = row & 3;
      ri = ri < n ? ri : n - 1; rh = rh < H ? rh : H - 1;
      R.vq[k] = qt4[(ri * H + rh) * 8 + sub];
    }
    const float* mk = a.emask + (size_t)gg * n * S;
    const float4* ef4 = reinterpret_cast<const float4*>(a.efeat + (size_t)gg * n * S * 4);
#pragma unroll
    for (int p = 0; p < NPR; ++p) {
      R.mkv[p] = mk[ic * S + sc[p]];
      R.efv[p] = ef4[ic * S + sc[p]];
    }
  };
  auto stage = [&](Regs& R) {
    int pin = 0;
#pragma unroll
    for (int p = 0; p < NPR; ++p) pin |= __float_as_int(R.mkv[p]) | f4bits(R.efv[p]);
    if constexpr (XOF) pin |= abd_xo_bits<GT>(R.xo, HITS);
    const int pin0 = opaque_zero(pin);
#pragma unroll
    for (int p = 0; p < PS; ++p) {
      float4 v = R.vs[p];
      if (XOF && p * 8 + il >= n) v = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(XS + pin0 + (p * 8 + il) * ABD_XL + sub * 4) = v;
    }
    if constexpr (XOF) abd_xo_emit<GT, HITS>(R.xo, XS + pin0, XH + pin0, n, NSH - n, li_, lq_, true);
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + pin0 + (k * 8 + il) * ABD_XL + k * 8 + sub * 4) = R.vh[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(QP + pin0 + (k * 8 + il) * ABD_XL + sub * 4) = R.vq[k];
#pragma unroll
    for (int p = 0; p < NPR; ++p) R.mkv[p] = (slot[p] >= 0) ? R.mkv[p] : 0.0f;
    if constexpr (HITS) {
      // The lane's own hit row reaches nobody when its slot is masked, but Zx = P Xs would still meet it as 0 * x on the matrix
      // cores (a NaN hit point: NaN row): the owner zeroes it.  DS operations of a wave execute in order: after the staging above.
      if (R.mkv[PS] == 0.0f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + lane * ABD_XL + il * 8 + k * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto compute = [&](int gg, const Regs& R) {
    float* zc = a.zcat + (size_t)gg * n * Kp;
    float* at = a.attn + (size_t)gg * n * S * H;
    f32x4g acc[NPR];
#pragma unroll
    for (int p = 0; p < NPR; ++p) acc[p] = f32x4g{0.f, 0.f, 0.f, 0.f};
    {
      const float* qrow = QP + (il * 4 + hA) * ABD_XL;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float4 q = *reinterpret_cast<const float4*>(qrow + k * 4);
        float4 x[NPR];
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          if (HITS && p == PS) x[p] = *reinterpret_cast<const float4*>(XH + lane * ABD_XL + il * 8 + k * 4);
          else x[p] = *reinterpret_cast<const float4*>(XS + (p * 8 + sub) * ABD_XL + k * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < NPR; ++p) acc[p] = mfma4(f4e(q)[u], f4e(x[p])[u], acc[p]);
      }
    }
    float* PT = QP;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (h < H) {
        float l[NPR];
        float mx = -INFINITY;
#pragma unroll
        for (int p = 0; p < NPR; ++p) { l[p] = (R.mkv[p] != 0.0f) ? acc[p][h] : -INFINITY; mx = fmaxf(mx, l[p]); }
        mx = grp8_max(mx);
        float den = 0.0f;
#pragma unroll
        for (int p = 0; p < NPR; ++p) { l[p] = (l[p] == -INFINITY) ? 0.0f : __expf(l[p] - mx); den += l[p]; }
        den = grp8_sum(den);
        const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
        float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          const float av = l[p] * inv;
          acc[p][h] = av;
          if (slot[p] >= 0) {
            if (a.attn != nullptr) at[(i * S + slot[p]) * H + h] = av;
            if (av != 0.0f) {   // masked slots may carry 5e5 / NaN edge features: skip, never multiply
              const float4 e = R.efv[p];
              z0 = fmaf(av, e.x, z0); z1 = fmaf(av, e.y, z1); z2 = fmaf(av, e.z, z2); z3 = fmaf(av, e.w, z3);
            }
          }
        }
        z0 = grp8_sum(z0); z1 = grp8_sum(z1); z2 = grp8_sum(z2); z3 = grp8_sum(z3);
        if (live && sub == 0) *reinterpret_cast<float4*>(zc + i * Kp + F + h * Wd + F) = make_float4(z0, z1, z2, z3);
      } else {
#pragma unroll
        for (int p = 0; p < NPR; ++p) acc[p][h] = 0.0f;
      }
#pragma unroll
      for (int p = 0; p < NPR; ++p) PT[(il * 4 + h) * PL + p * 8 + sub] = acc[p][h];
    }
    {
      float pa[PC];
#pragma unroll
      for (int k = 0; k < PC / 4; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(PT + (il * 4 + hA) * PL + k * 4);
        pa[k * 4] = v.x; pa[k * 4 + 1] = v.y; pa[k * 4 + 2] = v.z; pa[k * 4 + 3] = v.w;
      }
      f32x4g az[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) az[q] = f32x4g{0.f, 0.f, 0.f, 0.f};
      const int fq = (g2 * 4 + c) * 4;
#pragma unroll
      for (int kk = 0; kk < NSP; ++kk) {
        const float4 b = *reinterpret_cast<const float4*>(XS + kk * ABD_XL + fq);
#pragma unroll
        for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[kk], f4e(b)[q], az[q]);
      }
      if constexpr (HITS) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float4 b = *reinterpret_cast<const float4*>(XH + (il * 8 + m) * ABD_XL + il * 8 + fq);
#pragma unroll
          for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[NSP + m], f4e(b)[q], az[q]);
        }
      }
      if (live) {
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (h < H) *reinterpret_cast<float4*>(zc + i * Kp + F + h * Wd + fq) = make_float4(az[0][h], az[1][h], az[2][h], az[3][h]);
      }
    }
#pragma unroll
    for (int p = 0; p < PS; ++p) {
      const int row = p * 8 + il;
      if (row < n) *reinterpret_cast<float4*>(zc + row * Kp + sub * 4) = *reinterpret_cast<const float4*>(XS + row * ABD_XL + sub * 4);
    }
    {
      const int wpad = Kp - kc;                                  // >= 1: the constant column, then zeros
      for (int ii = lane; ii < n; ii += 64)
        for (int cc = 0; cc < wpad; ++cc) zc[ii * Kp + kc + cc] = (cc == 0) ? ones_col(a.t, a.emask + ((size_t)gg * n + ii) * a.t.S) : 0.0f;
    }
  };
  Regs cur;
  load(g, cur);
  for (;;) {
    stage(cur);
    const int gn = g + stride;
    const bool more = gn < a.G;                                // wave-uniform
    Regs nxt;
    if (more) load(gn, nxt);
    compute(g, cur);
    if (!more) break;
    cur = nxt;
    g = gn;
  }
}

// backward of the block-diagonal form: dA (as the logits), softmax backward in registers, dQt = dL Xs (as the aggregation),
// dXs of the shared nodes on 16x16x4 tiles (contraction over the batch's (agent, head) rows, accumulated over the agent
// batches), dXs of the hit nodes as 4x4 blocks whose A operand (P and dL of the lane's own hit) never leaves the registers.
template <int PS, bool HITS, int AB, bool XOF>
__global__ void __launch_bounds__(64) attn_bwd_bd_kernel(AttnArgs a) {
  extern __shared__ float4 abd_sm[];
  using L = AbdLds<PS, HITS>;
  constexpr int F = 32, NSP = L::NSP, PC = L::PC, PL = L::PL, PTL = L::PTL, NPR = PS + (HITS ? 1 : 0), Wd = F + 4;
  constexpr int RTS = (NSP + 15) / 16;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x;
  if (g >= a.G) return;
  const int n = t.n, S = t.S, Ns = t.Ns, H = a.H, Kp = a.Kp;
  const int NSH = HITS ? t.n + t.ng : Ns;
  float* XS = reinterpret_cast<float*>(abd_sm);
  float* XH = XS + L::XS;
  float* DZ = XH + L::XH;
  float* PT = DZ + L::DZ;
  float* DL = PT + L::PT;
  const float4* Xa4 = reinterpret_cast<const float4*>(a.Xa + (size_t)g * n * F);
  const float4* Xo4 = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (Ns - n) * F);
  const float* qt = a.qt + (size_t)g * n * H * F;
  const float* dzc = a.dzcat + (size_t)g * n * Kp;
  const bool want_dx = a.dXa != nullptr;
  const int il = lane >> 3, sub = lane & 7, g2 = (lane >> 2) & 1, c = lane & 3, hA = lane & 3;
  const int li = lane & 15, lq = lane >> 4;
  // ---- every global read is requested before anything waits (clamped addresses, no branches: see the forward) ----
  float4 vs[PS];
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    const int row = p * 8 + il;
    const int ra = row < n ? row : n - 1, ro = (row < NSH ? row : NSH - 1) - n;
    const float4* src = (XOF || row < n || NSH == n) ? Xa4 + ra * 8 + sub : Xo4 + ro * 8 + sub;
    vs[p] = *src;
  }
  constexpr int GT = (NSP + 15) / 16;
  AbdXoRegs<GT> xo;
  const float* raw = XOF ? a.Xo_raw + (size_t)g * (Ns - n) * ABD_KR : nullptr;
  const int li_ = lane & 15, lq_ = lane >> 4;
  // the direct x_i part of dzcat for the agent rows of dXa, in the C/D layout of the shared-node tiles
  float dir[RTS][2][4];
#pragma unroll
  for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int node = rt * 16 + lq * 4 + r;
        dir[rt][ft][r] = dzc[(node < n ? node : n - 1) * Kp + ft * 16 + li];
      }
  f32x4g dxs[RTS][2];
#pragma unroll
  for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) dxs[rt][ft] = f32x4g{0.f, 0.f, 0.f, 0.f};
  f32x4g dwacc[2] = {f32x4g{0.f, 0.f, 0.f, 0.f}, f32x4g{0.f, 0.f, 0.f, 0.f}};      // XOF + dwo_slab: (dWo | dbo)^T, rows f, columns k
  float rbg[NSP / 4];
  const float4* ef4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
  const float* at = a.attn + (size_t)g * n * S * H;
#pragma unroll
  for (int ab = 0; ab < AB; ++ab) {       // AB = ceil(n / 8), a compile-time count: straight-line code, every array in registers
    const int i = ab * 8 + il;
    const bool live = i < n;
    const int ic = live ? i : n - 1;
    float4 vh[HITS ? 8 : 1], vz[5];
    if constexpr (XOF) abd_xo_load<GT, HITS>(xo, a, raw, NSH - n, t.ng, ab * 64, n * 8, li_, lq_, ab == 0);
    // B operands of the weight-gradient contraction (dgppo_attn_bwd_xo_dw): raw feature li & 7 of other-row 4 s + lq, requested
    // with everything else (read in the loop that uses them they were 16 dependent trips to L2)
    float rbh[HITS ? 16 : 1];
    if constexpr (XOF && HITS) {
#pragma unroll
      for (int s_ = 0; s_ < 16; ++s_) {
        int hb = ab * 64 + s_ * 4 + lq;
        hb = hb < n * 8 ? hb : n * 8 - 1;
        rbh[s_] = raw[(t.ng + hb) * ABD_KR + (li & 7)];
      }
    }
    if constexpr (XOF) {
      if (ab == 0) {
#pragma unroll
        for (int s_ = 0; s_ < NSP / 4; ++s_) {
          int o = s_ * 4 + lq;
          o = o < NSH - n ? o : NSH - n - 1;
          o = o < 0 ? 0 : o;
          rbg[s_] = raw[o * ABD_KR + (li & 7)];
        }
      }
    }
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int hb = ab * 64 + k * 8 + il;
        hb = hb < n * 8 ? hb : n * 8 - 1;
        vh[k] = Xo4[(t.ng + hb) * 8 + sub];
      }
    }
    // dZ rows of the batch: 32 rows (agent, head) x 9 float4 (32 features + 4 edge terms); rows past n / H duplicate a real
    // row: they only meet zeros of P and dL
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      int tt = k * 64 + lane;
      tt = tt < 288 ? tt : 287;
      const int row = tt / 9, ch = tt - row * 9;
      int ri = ab * 8 + (row >> 2), rh = row & 3;
      ri = ri < n ? ri : n - 1; rh = rh < H ? rh : H - 1;
      vz[k] = *reinterpret_cast<const float4*>(dzc + ri * Kp + F + rh * Wd + ch * 4);
    }
    int slot[NPR];
    float4 efv[NPR];
    float av[NPR][4];
#pragma unroll
    for (int p = 0; p < NPR; ++p) {
      int sl;
      if (HITS && p == PS) sl = n + t.gs + sub;
      else { const int j = p * 8 + sub; sl = (j < NSH) ? slot_of(t, j, ic) : -1; }
      slot[p] = live ? sl : -1;
      const int sc = sl < 0 ? 0 : sl;
      efv[p] = ef4[ic * S + sc];
#pragma unroll
      for (int h = 0; h < 4; ++h) av[p][h] = at[(ic * S + sc) * H + (h < H ? h : H - 1)];
    }
    // operands that come straight from global memory: the query rows as B operands of the hit-node blocks (feature octet c
    // of every head of the lane's agent) and of the shared-node tiles (row = agent ks of the batch, head lq)
    float4 q8[4][2];
    if constexpr (HITS) {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const float4* qr = reinterpret_cast<const float4*>(qt + (size_t)(ic * H + (h < H ? h : H - 1)) * F + c * 8);
        q8[h][0] = qr[0]; q8[h][1] = qr[1];
      }
    }
    float bQ[8][2];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int ri = ab * 8 + ks;
      const float* qr = qt + (size_t)((ri < n ? ri : n - 1) * H + (lq < H ? lq : H - 1)) * F;   // rows past n / H: dL is 0 there
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) bQ[ks][ft] = qr[ft * 16 + li];
    }
    int pin = 0;
#pragma unroll
    for (int p = 0; p < NPR; ++p) {
      pin |= f4bits(efv[p]);
#pragma unroll
      for (int h = 0; h < 4; ++h) pin |= __float_as_int(av[p][h]);
    }
    if constexpr (HITS) {
#pragma unroll
      for (int h = 0; h < 4; ++h) pin |= f4bits(q8[h][0]) | f4bits(q8[h][1]);
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) pin |= __float_as_int(bQ[ks][0]) | __float_as_int(bQ[ks][1]);
    if (ab == 0) {
#pragma unroll
      for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
          for (int r = 0; r < 4; ++r) pin |= __float_as_int(dir[rt][ft][r]);
    }
    if constexpr (XOF) pin |= abd_xo_bits<GT>(xo, HITS);
    if constexpr (XOF && HITS) {
#pragma unroll
      for (int s_ = 0; s_ < 16; ++s_) pin |= __float_as_int(rbh[s_]);
    }
    if constexpr (XOF) {
      if (ab == 0) {
#pragma unroll
        for (int s_ = 0; s_ < NSP / 4; ++s_) pin |= __float_as_int(rbg[s_]);
      }
    }
    const int pin0 = opaque_zero(pin);
    if (ab == 0) {
#pragma unroll
      for (int p = 0; p < PS; ++p) {
        float4 v = vs[p];
        if (XOF && p * 8 + il >= n) v = make_float4(0.f, 0.f, 0.f, 0.f);       // pad rows stay zero, the others are recomputed below
        *reinterpret_cast<float4*>(XS + pin0 + (p * 8 + il) * ABD_XL + sub * 4) = v;
      }
    }
    if constexpr (XOF) abd_xo_emit<GT, HITS>(xo, XS + pin0, XH + pin0, n, NSH - n, li_, lq_, ab == 0);
    if constexpr (HITS && !XOF) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + pin0 + (k * 8 + il) * ABD_XL + k * 8 + sub * 4) = vh[k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int tt = k * 64 + lane, row = tt / 9, ch = tt - row * 9;
      if (tt < 288) *reinterpret_cast<float4*>(DZ + pin0 + row * ABD_DZL + ch * 4) = vz[k];
    }
#pragma unroll
    for (int p = 0; p < NPR; ++p)
#pragma unroll
      for (int h = 0; h < 4; ++h) av[p][h] = (slot[p] >= 0 && h < H) ? av[p][h] : 0.0f;
    if constexpr (HITS) {
      // the lane's own hit row, if its slot carries no weight (a == 0 in every head: the saved weights are consulted, not the mask,
      // so also an unmasked slot whose softmax weight underflowed), is zeroed before dQt = dL Xs meets it as 0 * x (see the forward)
      if (av[PS][0] == 0.0f && av[PS][1] == 0.0f && av[PS][2] == 0.0f && av[PS][3] == 0.0f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(XH + lane * ABD_XL + il * 8 + k * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // ---- dA = dZx Xs^T at the lane's slots ----
    f32x4g acc[NPR];
#pragma unroll
    for (int p = 0; p < NPR; ++p) acc[p] = f32x4g{0.f, 0.f, 0.f, 0.f};
    {
      const float* zrow = DZ + (il * 4 + hA) * ABD_DZL;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float4 q = *reinterpret_cast<const float4*>(zrow + k * 4);
        float4 x[NPR];
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          if (HITS && p == PS) x[p] = *reinterpret_cast<const float4*>(XH + lane * ABD_XL + il * 8 + k * 4);
          else x[p] = *reinterpret_cast<const float4*>(XS + (p * 8 + sub) * ABD_XL + k * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < NPR; ++p) acc[p] = mfma4(f4e(q)[u], f4e(x[p])[u], acc[p]);
      }
    }
    // ---- softmax backward per head: dl = a (dA + dze.e - sum a (dA + dze.e)); tiles: P (shared columns) and dL ----
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float4 dze = *reinterpret_cast<const float4*>(DZ + (il * 4 + h) * ABD_DZL + F);
      float dot = 0.0f;
#pragma unroll
      for (int p = 0; p < NPR; ++p) {
        const float w = av[p][h];
        const float4 e = efv[p];
        // masked slots (a == 0) may carry 5e5 / NaN edge features: never multiply them
        const float dA = (w != 0.0f) ? acc[p][h] + fmaf(dze.x, e.x, fmaf(dze.y, e.y, fmaf(dze.z, e.z, dze.w * e.w))) : 0.0f;
        acc[p][h] = dA;
        dot = fmaf(w, dA, dot);
      }
      dot = grp8_sum(dot);
#pragma unroll
      for (int p = 0; p < NPR; ++p) {
        acc[p][h] = av[p][h] * (acc[p][h] - dot);
        DL[(il * 4 + h) * PL + p * 8 + sub] = acc[p][h];
        if (p < PS) PT[(il * 4 + h) * PTL + p * 8 + sub] = av[p][h];
      }
    }
    // ---- dQt = dL Xs ----
    {
      float pa[PC];
#pragma unroll
      for (int k = 0; k < PC / 4; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(DL + (il * 4 + hA) * PL + k * 4);
        pa[k * 4] = v.x; pa[k * 4 + 1] = v.y; pa[k * 4 + 2] = v.z; pa[k * 4 + 3] = v.w;
      }
      f32x4g az[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) az[q] = f32x4g{0.f, 0.f, 0.f, 0.f};
      const int fq = (g2 * 4 + c) * 4;
#pragma unroll
      for (int kk = 0; kk < NSP; ++kk) {
        const float4 b = *reinterpret_cast<const float4*>(XS + kk * ABD_XL + fq);
#pragma unroll
        for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[kk], f4e(b)[q], az[q]);
      }
      if constexpr (HITS) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float4 b = *reinterpret_cast<const float4*>(XH + (il * 8 + m) * ABD_XL + il * 8 + fq);
#pragma unroll
          for (int q = 0; q < 4; ++q) az[q] = mfma4(pa[NSP + m], f4e(b)[q], az[q]);
        }
      }
      if (live) {
        float* dq = a.dqt + ((size_t)g * n + i) * H * F;
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (h < H) *reinterpret_cast<float4*>(dq + h * F + fq) = make_float4(az[0][h], az[1][h], az[2][h], az[3][h]);
      }
    }
    if (want_dx) {
      // ---- shared nodes: dXs += P^T dZx + dL^T Qt over the 32 (agent, head) rows of the batch ----
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int prow = ks * 4 + lq;                          // = agent ks of the batch, head lq
        float bD[2];
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) bD[ft] = DZ[prow * ABD_DZL + ft * 16 + li];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
          const int col = (rt * 16 + li < NSP) ? rt * 16 + li : NSP - 1;      // tile rows past NSP are never stored
          const float aP = PT[prow * PTL + col], aL = DL[prow * PL + col];
#pragma unroll
          for (int ft = 0; ft < 2; ++ft) {
            dxs[rt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(aP, bD[ft], dxs[rt][ft], 0, 0, 0);
            dxs[rt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(aL, bQ[ks][ft], dxs[rt][ft], 0, 0, 0);
          }
        }
      }
      // ---- hit nodes: block (il, g2) = 4 hits x 4 feature octets, k = (head, P | dL) ----
      if constexpr (HITS) {
        if (a.dXo != nullptr || (XOF && a.dwo_slab != nullptr)) {
          f32x4g af[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) af[q] = f32x4g{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const float4 d0 = *reinterpret_cast<const float4*>(DZ + (il * 4 + h) * ABD_DZL + c * 8);
            const float4 d1 = *reinterpret_cast<const float4*>(DZ + (il * 4 + h) * ABD_DZL + c * 8 + 4);
            const float pw = av[PS][h], dw = acc[PS][h];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              af[q] = mfma4(pw, f4e(d0)[q], af[q]);
              af[q + 4] = mfma4(pw, f4e(d1)[q], af[q + 4]);
              af[q] = mfma4(dw, f4e(q8[h][0])[q], af[q]);
              af[q + 4] = mfma4(dw, f4e(q8[h][1])[q], af[q + 4]);
            }
          }
          float4 x0[4], x1[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float* xr = XH + (il * 8 + g2 * 4 + m) * ABD_XL + il * 8 + c * 8;
            x0[m] = *reinterpret_cast<const float4*>(xr);
            x1[m] = *reinterpret_cast<const float4*>(xr + 4);
          }
          const bool to_slab = XOF && a.dwo_slab != nullptr;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int hb = ab * 64 + il * 8 + g2 * 4 + m;
            float4 v0 = make_float4(af[0][m], af[1][m], af[2][m], af[3][m]);
            float4 v1 = make_float4(af[4][m], af[5][m], af[6][m], af[7][m]);
            if (a.relu_xo || to_slab) {
              v0.x = x0[m].x > 0.f ? v0.x : 0.f; v0.y = x0[m].y > 0.f ? v0.y : 0.f; v0.z = x0[m].z > 0.f ? v0.z : 0.f; v0.w = x0[m].w > 0.f ? v0.w : 0.f;
              v1.x = x1[m].x > 0.f ? v1.x : 0.f; v1.y = x1[m].y > 0.f ? v1.y : 0.f; v1.z = x1[m].z > 0.f ? v1.z : 0.f; v1.w = x1[m].w > 0.f ? v1.w : 0.f;
            }
            if (to_slab) {            // the hit image becomes the image of its gradient (rows of agents past n: zeros, P and dL are 0 there)
              float* xr = XH + (il * 8 + g2 * 4 + m) * ABD_XL + il * 8 + c * 8;
              *reinterpret_cast<float4*>(xr) = v0;
              *reinterpret_cast<float4*>(xr + 4) = v1;
            } else if (hb < n * 8) {
              float* o = a.dXo + ((size_t)g * (Ns - n) + t.ng + hb) * F + c * 8;
              *reinterpret_cast<float4*>(o) = v0;
              *reinterpret_cast<float4*>(o + 4) = v1;
            }
          }
          if constexpr (XOF) {
            if (to_slab) {
              // dWo^T [f][k] += sum over the batch's 64 hit rows dX[row][f] raw[row][k]  (column 8 of B = 1: the bias gradient)
#pragma unroll
              for (int s_ = 0; s_ < 16; ++s_) {
                const int hr = s_ * 4 + lq;
                const float bv = li < 8 ? rbh[s_] : (li == 8 ? 1.0f : 0.0f);
#pragma unroll
                for (int ft = 0; ft < 2; ++ft) {
                  const float av_ = XH[hr * ABD_XL + (hr >> 3) * 8 + ft * 16 + li];
                  dwacc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_, bv, dwacc[ft], 0, 0, 0);
                }
              }
            }
          }
        }
      }
    }
  }
  if (want_dx) {
    float xm[RTS][2][4];
#pragma unroll
    for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int node = rt * 16 + lq * 4 + r;
          xm[rt][ft][r] = (node < NSP) ? XS[node * ABD_XL + ft * 16 + li] : 0.0f;
        }
#pragma unroll
    for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int node = rt * 16 + lq * 4 + r, f = ft * 16 + li;
          float v = dxs[rt][ft][r];
          if (node < n) a.dXa[((size_t)g * n + node) * F + f] = v + dir[rt][ft][r];
          else if (XOF && a.dwo_slab != nullptr) {
            if (node < NSP) XS[node * ABD_XL + f] = (node < NSH && xm[rt][ft][r] > 0.0f) ? v : 0.0f;   // gradient image of the shared other rows
          } else if (node < NSH && a.dXo != nullptr) {
            if (a.relu_xo) v = (xm[rt][ft][r] > 0.0f) ? v : 0.0f;
            a.dXo[((size_t)g * (Ns - n) + (node - n)) * F + f] = v;
          }
        }
    if constexpr (XOF) {
      if (a.dwo_slab != nullptr) {
        const int nsho = NSH - n;
#pragma unroll
        for (int s_ = 0; s_ < NSP / 4; ++s_) {
          const int o = s_ * 4 + lq;
          const float bv = li < 8 ? rbg[s_] : (li == 8 ? 1.0f : 0.0f);
#pragma unroll
          for (int ft = 0; ft < 2; ++ft) {
            const int node = n + o;
            const float av_ = (o < nsho && node < NSP) ? XS[(node < NSP ? node : NSP - 1) * ABD_XL + ft * 16 + li] : 0.0f;
            dwacc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_, bv, dwacc[ft], 0, 0, 0);
          }
        }
        if (li <= 8) {
          float* o = a.dwo_slab + (size_t)g * ABD_DW_STRIDE + li * 32 + lq * 4;
#pragma unroll
          for (int ft = 0; ft < 2; ++ft)
            *reinterpret_cast<float4*>(o + ft * 16) = make_float4(dwacc[ft][0], dwacc[ft][1], dwacc[ft][2], dwacc[ft][3]);
        }
      }
    }
  }
}

// the block-diagonal kernels apply when the private nodes are exactly 8 LiDAR hits per agent (or there are none), there are at
// most 32 shared nodes (PS <= 4 groups of 8) and at most 16 agents (AB = ceil(n / 8) <= 2 agent batches; the shared nodes
// include the agents, so AB <= PS)
static bool attn_bd_shape(const Topo& t, int F, int H, int& PS, bool& hits) {
  if (F != 32 || H < 1 || H > 4 || t.n > 16) return false;
  const int n_priv = t.Ns - t.n - t.ng;
  hits = t.lidar && n_priv > 0;
  if (hits && (t.per != 8 || n_priv != t.n * 8)) return false;
  const int nsh = hits ? t.n + t.ng : t.Ns;
  PS = (nsh + 7) / 8;
  return PS >= 1 && PS <= 4;
}
template <int PS, bool HITS, int AB, bool XOF>
static void launch_attn_bd_x(const AttnArgs& a, hipStream_t s, bool bwd) {
  using L = AbdLds<PS, HITS>;
  if (bwd) { hipLaunchKernelGGL((attn_bwd_bd_kernel<PS, HITS, AB, XOF>), dim3(a.G), dim3(64), sizeof(float) * L::BWD, s, a); return; }
  if constexpr (AB == 1) {
    // persistent waves with the next graph's loads in flight: as many 2-wave workgroups as fit the chip (LDS-limited), unless
    // the launch is small enough that every graph gets its own wave anyway
    static thread_local int cap = 0;
    if (cap == 0) {
      int per_cu = 0, dev = 0, cus = 256;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&attn_fwd_bdp_kernel<PS, HITS, XOF>), 128,
                                                       sizeof(float) * 2 * L::FWD) != hipSuccess || per_cu < 1) per_cu = 1;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
          cus < 1) cus = 256;
      cap = per_cu * cus;
    }
    if ((a.G + 1) / 2 > 2 * cap) {   // (smaller launches: one graph per wave in the leaner kernel below — more waves per CU)
      hipLaunchKernelGGL((attn_fwd_bdp_kernel<PS, HITS, XOF>), dim3(cap), dim3(128), sizeof(float) * 2 * L::FWD, s, a);
      return;
    }
  }
  hipLaunchKernelGGL((attn_fwd_bd_kernel<PS, HITS, AB, XOF>), dim3((a.G + 1) / 2), dim3(128), sizeof(float) * 2 * L::FWD, s, a);
}
template <int PS, bool HITS, int AB>
static void launch_attn_bd_one(const AttnArgs& a, hipStream_t s, bool bwd) {
  if (a.Xo_raw != nullptr) launch_attn_bd_x<PS, HITS, AB, true>(a, s, bwd);
  else launch_attn_bd_x<PS, HITS, AB, false>(a, s, bwd);
}
static bool launch_attn_bd(const AttnArgs& a, hipStream_t s, bool bwd) {
  int PS = 0;
  bool hits = false;
  if (!attn_bd_shape(a.t, a.F, a.H, PS, hits)) return false;
  const int AB = (a.t.n + 7) / 8;
  switch ((PS * 2 + (hits ? 1 : 0)) * 4 + AB) {
#define DGPPO_BD(P, HT, B) case ((P) * 2 + (HT)) * 4 + (B): launch_attn_bd_one<P, (HT) != 0, B>(a, s, bwd); return true;
    DGPPO_BD(1, 0, 1) DGPPO_BD(1, 1, 1) DGPPO_BD(2, 0, 1) DGPPO_BD(2, 1, 1) DGPPO_BD(2, 0, 2) DGPPO_BD(2, 1, 2)
    DGPPO_BD(3, 0, 1) DGPPO_BD(3, 1, 1) DGPPO_BD(3, 0, 2) DGPPO_BD(3, 1, 2)
    DGPPO_BD(4, 0, 1) DGPPO_BD(4, 1, 1) DGPPO_BD(4, 0, 2) DGPPO_BD(4, 1, 2)
#undef DGPPO_BD
    default: return false;
  }
}

__global__ void __launch_bounds__(256) attn_bwd_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const AttnDims d = attn_dims(t, a.F, a.H);
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = d.n, S = d.S, Ns = d.Ns, F = d.F, H = d.H, Fl = d.Fl, Ll = d.Ll, nH = d.nH;
  const int Wd = F + 4, Zl = F + 5, Sp = (S + 3) & ~3;
  float* s_x = sm;
  float* s_q = s_x + d.CT * 16 * Fl;
  float* s_P = s_q + d.RT * 16 * Fl;
  float* s_e = sm + (((d.CT * 16 * Fl + d.RT * 16 * Fl + d.RT * 16 * Ll) + 3) & ~3);   // float4-aligned
  float* s_c = s_e + n * S * 4;           // compact [nH][Sp]: dA at the slots -> dl     (the forward's s_m + s_a space)
  float* s_a = s_c + nH * Sp;             // compact [nH][Sp]: attention weights
  float* s_D = s_a + nH * Sp;
  float* s_z = s_D + d.RT * 16 * Ll;
  const float* dzc = a.dzcat + (size_t)g * n * a.Kp;
  {
    const int F4 = F >> 2, W4 = Wd >> 2;       // Wd = F + 4, Kp and F are multiples of 4 -> 16-byte aligned pieces
    const float4* xa = reinterpret_cast<const float4*>(a.Xa + (size_t)g * n * F);
    const float4* xo = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (Ns - n) * F);
    const float4* q4 = reinterpret_cast<const float4*>(a.qt + (size_t)g * nH * F);
    const float4* e4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
    const float* at = a.attn + (size_t)g * n * S * H;
    const int nA = n * F4, nX = Ns * F4, nXp = d.CT * 16 * F4, nQ = nH * F4, nQp = d.RT * 16 * F4, nE = n * S;
    const int nZp = d.RT * 16 * W4, nAt = n * S * H;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto ldz = [&](int idx) {
      const int row = idx / W4, q = idx - row * W4;
      if (row >= nH) return z4;
      const int i = row / H, h = row - i * H;
      return *reinterpret_cast<const float4*>(dzc + i * a.Kp + F + h * Wd + 4 * q);
    };
    float4 vx[4], vq[2], ve[2], vz[2];
    float va[3];
#pragma unroll
    for (int it = 0; it < 4; ++it) { const int idx = tid + it * 256; vx[it] = (idx < nA) ? xa[idx] : ((idx < nX) ? xo[idx - nA] : z4); }
#pragma unroll
    for (int it = 0; it < 2; ++it) { const int idx = tid + it * 256; vq[it] = (idx < nQ) ? q4[idx] : z4; ve[it] = (idx < nE) ? e4[idx] : z4; vz[it] = (idx < nZp) ? ldz(idx) : z4; }
#pragma unroll
    for (int it = 0; it < 3; ++it) { const int idx = tid + it * 256; va[it] = (idx < nAt) ? at[idx] : 0.0f; }
#pragma unroll
    for (int it = 0; it < 4; ++it) { const int idx = tid + it * 256; if (idx < nXp) { const int nd = idx / F4, q = idx - nd * F4; put4(s_x + nd * Fl + 4 * q, vx[it]); } }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + it * 256;
      if (idx < nQp) { const int row = idx / F4, q = idx - row * F4; put4(s_q + row * Fl + 4 * q, vq[it]); }
      if (idx < nE) reinterpret_cast<float4*>(s_e)[idx] = ve[it];
      if (idx < nZp) { const int row = idx / W4, q = idx - row * W4; put4(s_z + row * Zl + 4 * q, vz[it]); }
    }
    auto puta = [&](int idx, float v) { const int h = idx % H, is = idx / H, i = is / S, s = is - i * S; s_a[(i * H + h) * Sp + s] = v; };
#pragma unroll
    for (int it = 0; it < 3; ++it) { const int idx = tid + it * 256; if (idx < nAt) puta(idx, va[it]); }
    for (int idx = tid + 1024; idx < nXp; idx += 256) { const int nd = idx / F4, q = idx - nd * F4; put4(s_x + nd * Fl + 4 * q, (idx < nA) ? xa[idx] : ((idx < nX) ? xo[idx - nA] : z4)); }
    for (int idx = tid + 512; idx < nQp; idx += 256) { const int row = idx / F4, q = idx - row * F4; put4(s_q + row * Fl + 4 * q, (idx < nQ) ? q4[idx] : z4); }
    for (int idx = tid + 512; idx < nE; idx += 256) reinterpret_cast<float4*>(s_e)[idx] = e4[idx];
    for (int idx = tid + 512; idx < nZp; idx += 256) { const int row = idx / W4, q = idx - row * W4; put4(s_z + row * Zl + 4 * q, ldz(idx)); }
    for (int idx = tid + 768; idx < nAt; idx += 256) puta(idx, at[idx]);
    for (int idx = tid; idx < d.RT * 16 * Ll; idx += 256) s_P[idx] = 0.0f;
    if (Sp != S) for (int idx = tid; idx < nH; idx += 256) for (int s = S; s < Sp; ++s) s_a[idx * Sp + s] = 0.0f;
  }
  __syncthreads();
  // P scatter (for dXs) and dA = dZx * Xs^T
  for (int idx = tid; idx < nH * S; idx += 256) {
    const int pair = idx / S, s = idx - pair * S, i = pair / H;
    const float av = s_a[pair * Sp + s];
    if (av != 0.0f) s_P[pair * Ll + sender_node(t, i, s)] = av;
  }
  mfma_tiles(d.RT, d.CT, F / 4, wave, lane,
             [&](int row, int k) { return s_z[row * Zl + k]; },
             [&](int k, int col) { return s_x[col * Fl + k]; },
             [&](int row, int col, float v) { s_D[row * Ll + col] = v; });
  __syncthreads();
  // gather dA at the slots (+ the edge-feature term) into the compact rows
  for (int idx = tid; idx < nH * Sp; idx += 256) {
    const int pair = idx / Sp, s = idx - pair * Sp, i = pair / H;
    float dA = 0.0f;
    if (s < S && s_a[idx] != 0.0f) {
      dA = s_D[pair * Ll + sender_node(t, i, s)];
      const float* dz = s_z + pair * Zl + F;
      const float4 e = reinterpret_cast<const float4*>(s_e)[i * S + s];
      dA = fmaf(dz[0], e.x, fmaf(dz[1], e.y, fmaf(dz[2], e.z, fmaf(dz[3], e.w, dA))));
    }
    s_c[idx] = dA;
  }
  // a private LiDAR-hit row whose slot carries no weight (a == 0 in every head: the saved weights are consulted, not the mask, so
  // also an unmasked slot whose softmax weight underflowed) is zeroed before dQt = dL * Xs meets it as 0 * x (see the forward)
  if (t.lidar && t.os > 0)
    for (int q = tid >> 6; q < n * t.os; q += 4) {          // one wave per row, its lanes over the F columns
      const int i = q / t.os, s = n + t.gs + (q - i * t.os);
      bool dead = true;
      for (int h = 0; h < H; ++h) dead = dead && s_a[(i * H + h) * Sp + s] == 0.0f;
      if (dead)
        for (int f = tid & 63; f < F; f += 64) s_x[(n + t.ng + q) * Fl + f] = 0.0f;
    }
  __syncthreads();
  // 8 lanes per (agent, head): softmax backward dl = a * (dA - sum_s a dA); then every lane helps clearing s_D
  for (int p0 = 0; p0 < nH; p0 += 32) {
    const int pair = p0 + (tid >> 3), sub = tid & 7;
    const bool live = pair < nH;
    float av[ATT_SMAX / 8], dA[ATT_SMAX / 8];
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < ATT_SMAX / 8; ++j) {
      const int sl = sub + 8 * j;
      av[j] = (live && sl < S) ? s_a[pair * Sp + sl] : 0.0f;
      dA[j] = (live && sl < S) ? s_c[pair * Sp + sl] : 0.0f;
      dot = fmaf(av[j], dA[j], dot);
    }
    dot = grp8_sum(dot);
#pragma unroll
    for (int j = 0; j < ATT_SMAX / 8; ++j) {
      const int sl = sub + 8 * j;
      if (live && sl < S) s_c[pair * Sp + sl] = av[j] * (dA[j] - dot);
    }
  }
  for (int idx = tid; idx < d.RT * 16 * Ll; idx += 256) s_D[idx] = 0.0f;
  __syncthreads();
  for (int idx = tid; idx < nH * S; idx += 256) {
    const int pair = idx / S, s = idx - pair * S, i = pair / H;
    const float dl = s_c[pair * Sp + s];
    if (dl != 0.0f) s_D[pair * Ll + sender_node(t, i, s)] = dl;
  }
  __syncthreads();
  // dQt = dL * Xs
  float* dq = a.dqt + (size_t)g * nH * F;
  mfma_tiles(d.RT, (F + 15) / 16, d.CT * 4, wave, lane,
             [&](int row, int k) { return s_D[row * Ll + k]; },
             [&](int k, int col) { return (col < F) ? s_x[k * Fl + col] : 0.0f; },
             [&](int row, int col, float v) { if (row < nH && col < F) dq[row * F + col] = v; });
  // dXs = P^T * dZx + dL^T * Qt  (+ direct x_i part for agents)
  if (a.dXa != nullptr) {
    const int li = lane & 15, lq = lane >> 4;
    const int FT = (F + 15) / 16;
    for (int tile = wave; tile < d.CT * FT; tile += 4) {
      const int rt = tile / FT, ct = tile - rt * FT;
      f32x4g acc = {0.f, 0.f, 0.f, 0.f};
      const int nd_a = rt * 16 + li, col_b = ct * 16 + li;
#pragma unroll 4
      for (int k4 = 0; k4 < d.RT * 4; ++k4) {
        const int kk = k4 * 4 + lq;   // (agent, head) row
        const float bz = (col_b < F) ? s_z[kk * Zl + col_b] : 0.0f;
        const float bq = (col_b < F) ? s_q[kk * Fl + col_b] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_P[kk * Ll + nd_a], bz, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_D[kk * Ll + nd_a], bq, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nd = rt * 16 + lq * 4 + r, f = ct * 16 + li;
        if (nd >= Ns || f >= F) continue;
        if (nd < n) a.dXa[((size_t)g * n + nd) * F + f] = acc[r] + dzc[nd * a.Kp + f];
        else if (a.dXo != nullptr) a.dXo[((size_t)g * (Ns - n) + (nd - n)) * F + f] = acc[r];
      }
    }
  }
}

// =====================================================================================================================
// Tiled attention: graphs whose whole-graph LDS image does not fit (teams of more than ~20 agents; S up to 136 slots).
// One workgroup (4 waves) per graph walks the receiving agents in tiles of TI.  The sender rows come in two groups, as in
// the block-diagonal family:
//   shared   nodes every agent reads: the n agents, all goals (Spread kinds), all obstacles (MPE kinds); NSH <= 192 rows,
//            staged once per graph and resident in LDS for all tiles (rows >= NSH of the 16-row padding are zero)
//   private  an agent's own goal (Target kinds, row 0) and its own k LiDAR hits: NP rows per agent, staged per tile
// Per tile (rows = TI*H (agent, head) pairs) one buffer B [rows x (NSHp | NP)] carries, column by column, the logits, then
// the attention weights P:  B[:, :NSHp] = Q Xs^T and Zx = P Xs run on the matrix cores (mfma_tiles), the private columns
// are slot-wise dot products on the VALU, the masked softmax runs over the S slots of a pair with 8 lanes per pair and
// the buffer as its row (no register rows: S reaches 136).  Edge features, masks and attention weights are used once per
// head and read from global memory where they are needed.
// Backward: B = dA (MFMA + VALU), softmax backward in place (B = dL), dQt = dL Xs (+ private part); the private nodes'
// gradient rows are written per tile; the shared nodes' gradient  sum over tiles of dL^T Q + P^T dZ  lives in the
// accumulator registers of the MFMA output tiles a wave owns for the whole graph (at most ATL_MAXT tiles of 16 x 16 per
// wave: no second LDS block, no atomics, no zero-fill) and is stored once after the last tile, with the direct
// dzcat[:, :F] part added for agents.  B is reloaded with P (shared columns) for the second product.
// Everything sums in a fixed order: both passes are bit-reproducible run to run.
// =====================================================================================================================
#define ATL_MAXT 12                    // output tiles of the shared nodes' gradient per wave: ceil(NSH/16) * ceil(F/16) <= 48
struct TiledDims {
  int NSH, NP, CT, NSHp, FT, TI, RT, Rp, Fl, Bl, Zl, NPl;
};
__host__ __device__ inline TiledDims tiled_dims(const Topo& t, int F, int H, int TI) {
  TiledDims d;
  d.NSH = t.n + (t.spread ? t.ng : 0) + (t.lidar ? 0 : t.os);
  d.NP = (t.spread ? 0 : 1) + (t.lidar ? t.os : 0);
  d.CT = (d.NSH + 15) / 16; d.NSHp = d.CT * 16; d.FT = (F + 15) / 16;
  d.TI = TI; d.RT = (TI * H + 15) / 16; d.Rp = d.RT * 16;
  d.Fl = F + 1; d.Bl = d.NSHp + d.NP + 1; d.Zl = F + 5; d.NPl = d.NP > 0 ? d.NP : 1;
  return d;
}
static size_t attn_tiled_smem(const TiledDims& d, bool bwd) {
  size_t fl = (size_t)d.NSHp * d.Fl + (size_t)d.TI * d.NP * d.Fl + (size_t)d.Rp * d.Fl + (size_t)d.Rp * d.Bl;
  if (bwd) fl += (size_t)d.Rp * d.Zl + (size_t)d.Rp * d.NPl;
  return fl * sizeof(float);
}
// column of B that holds slot s of an agent: the shared node's index, or NSHp + private index
__device__ inline int tiled_col(const Topo& t, int NSHp, int s) {
  if (s < t.n) return s;
  if (s < t.n + t.gs) return t.spread ? s : NSHp;
  const int m = s - t.n - t.gs;
  if (t.lidar) return NSHp + (t.spread ? 0 : 1) + m;
  return t.n + (t.spread ? t.ng : 0) + m;
}
__device__ inline int tiled_shared_node(const Topo& t, int j) { return (j < t.n || t.spread) ? j : j + t.ng; }
__device__ inline int tiled_shared_slot(const Topo& t, int j) { return (j < t.n || t.spread) ? j : j + t.gs; }
__device__ inline int tiled_private_node(const Topo& t, int i, int p) {
  if (!t.spread && p == 0) return t.n + i;
  return t.n + t.ng + i * t.per + (p - (t.spread ? 0 : 1));
}
// shared rows -> LDS (zero padding)
__device__ inline void tiled_stage_shared(const AttnArgs& a, const TiledDims& d, int g, int tid, float* s_xs) {
  const Topo& t = a.t;
  const int F4 = a.F >> 2;
  const float4* xa = reinterpret_cast<const float4*>(a.Xa + (size_t)g * t.n * a.F);
  const float4* xo = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (t.Ns - t.n) * a.F);
  for (int idx = tid; idx < d.NSHp * F4; idx += 256) {
    const int j = idx / F4, q = idx - j * F4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < d.NSH) {
      const int nd = tiled_shared_node(t, j);
      v = (nd < t.n) ? xa[nd * F4 + q] : xo[(nd - t.n) * F4 + q];
    }
    put4(s_xs + j * d.Fl + 4 * q, v);
  }
}
// the tile's query rows (zero padding) and private sender rows -> LDS
__device__ inline void tiled_stage_tile(const AttnArgs& a, const TiledDims& d, int g, int tid, int i0, int ti, float* s_q, float* s_xp) {
  const Topo& t = a.t;
  const int F4 = a.F >> 2, rows = ti * a.H;
  const float4* q4 = reinterpret_cast<const float4*>(a.qt + ((size_t)g * t.n + i0) * a.H * a.F);
  for (int idx = tid; idx < d.Rp * F4; idx += 256) {
    const int row = idx / F4, q = idx - row * F4;
    put4(s_q + row * d.Fl + 4 * q, (row < rows) ? q4[idx] : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  if (d.NP > 0) {
    const float4* xo = reinterpret_cast<const float4*>(a.Xo + (size_t)g * (t.Ns - t.n) * a.F);
    for (int idx = tid; idx < ti * d.NP * F4; idx += 256) {
      const int r = idx / F4, q = idx - r * F4, il = r / d.NP, p = r - il * d.NP;
      put4(s_xp + r * d.Fl + 4 * q, xo[(tiled_private_node(t, i0 + il, p) - t.n) * F4 + q]);
    }
  }
}

__global__ void __launch_bounds__(256) attn_fwd_tiled_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const TiledDims d = tiled_dims(t, a.F, a.H, a.TI);
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = t.n, S = t.S, F = a.F, H = a.H, Fl = d.Fl, Bl = d.Bl, NP = d.NP, NSHp = d.NSHp, Kp = a.Kp, Wd = F + 4;
  float* s_xs = sm;                         // NSHp * Fl   shared sender rows (resident)
  float* s_xp = s_xs + NSHp * Fl;           // TI * NP * Fl  private sender rows of the tile
  float* s_q = s_xp + d.TI * NP * Fl;       // Rp * Fl     query rows of the tile
  float* s_B = s_q + d.Rp * Fl;             // Rp * Bl     logits -> attention weights
  float* zc = a.zcat + (size_t)g * n * Kp;
  const float* mk = a.emask + (size_t)g * n * S;
  const float4* ef4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
  float* at = (a.attn != nullptr) ? a.attn + (size_t)g * n * S * H : nullptr;
  tiled_stage_shared(a, d, g, tid, s_xs);
  for (int i0 = 0; i0 < n; i0 += d.TI) {
    const int ti = min(d.TI, n - i0), rows = ti * H;
    tiled_stage_tile(a, d, g, tid, i0, ti, s_q, s_xp);
    __syncthreads();
    // ---- logits: shared columns on the matrix cores, private columns slot-wise ----
    mfma_tiles(d.RT, d.CT, F / 4, wave, lane,
               [&](int row, int k) { return s_q[row * Fl + k]; },
               [&](int k, int col) { return s_xs[col * Fl + k]; },
               [&](int row, int col, float v) { s_B[row * Bl + col] = v; });
    for (int idx = tid; idx < rows * NP; idx += 256) {
      const int row = idx / NP, p = idx - row * NP;
      const float* q = s_q + row * Fl;
      const float* x = s_xp + ((row / H) * NP + p) * Fl;
      float acc = 0.0f;
      for (int f = 0; f < F; ++f) acc = fmaf(q[f], x[f], acc);
      s_B[row * Bl + NSHp + p] = acc;
    }
    __syncthreads();
    // ---- masked softmax over the S slots of a pair, 8 lanes per pair; the edge-feature aggregation ----
    for (int p0 = 0; p0 < rows; p0 += 32) {
      const int pair = p0 + (tid >> 3), sub = tid & 7;
      const bool live = pair < rows;
      const int il = live ? pair / H : 0, h = live ? pair - il * H : 0, i = i0 + il;
      float* brow = s_B + (live ? pair : 0) * Bl;
      float mx = -INFINITY;
      if (live)
        for (int s = sub; s < S; s += 8) {
          const int c = tiled_col(t, NSHp, s);
          const float l = (mk[i * S + s] != 0.0f) ? brow[c] : -INFINITY;
          brow[c] = l;
          mx = fmaxf(mx, l);
        }
      mx = grp8_max(mx);
      float den = 0.0f;
      if (live)
        for (int s = sub; s < S; s += 8) {
          const int c = tiled_col(t, NSHp, s);
          const float l = brow[c];
          const float ev = (l == -INFINITY) ? 0.0f : expf(l - mx);
          brow[c] = ev;
          den += ev;
        }
      den = grp8_sum(den);
      const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
      float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
      if (live)
        for (int s = sub; s < S; s += 8) {
          const int c = tiled_col(t, NSHp, s);
          const float av = brow[c] * inv;
          brow[c] = av;
          if (at != nullptr) at[(i * S + s) * H + h] = av;
          if (av != 0.0f) {   // masked slots may carry 5e5 / NaN edge features: skip, never multiply
            const float4 e = ef4[i * S + s];
            z0 = fmaf(av, e.x, z0); z1 = fmaf(av, e.y, z1); z2 = fmaf(av, e.z, z2); z3 = fmaf(av, e.w, z3);
          }
        }
      z0 = grp8_sum(z0); z1 = grp8_sum(z1); z2 = grp8_sum(z2); z3 = grp8_sum(z3);
      if (live && sub == 0) {
        float* o = zc + i * Kp + F + h * Wd + F;
        o[0] = z0; o[1] = z1; o[2] = z2; o[3] = z3;
      }
    }
    __syncthreads();
    // ---- Zx = P Xs (+ the private slots), written straight into zcat ----
    mfma_tiles(d.RT, d.FT, d.CT * 4, wave, lane,
               [&](int row, int k) { return s_B[row * Bl + k]; },
               [&](int k, int col) { return (col < F) ? s_xs[k * Fl + col] : 0.0f; },
               [&](int row, int col, float v) {
                 if (row < rows && col < F) {
                   const int il = row / H, h = row - il * H;
                   for (int p = 0; p < NP; ++p) {
                     const float av = s_B[row * Bl + NSHp + p];
                     if (av != 0.0f) v = fmaf(av, s_xp[(il * NP + p) * Fl + col], v);
                   }
                   zc[(i0 + il) * Kp + F + h * Wd + col] = v;
                 }
               });
    __syncthreads();
  }
  // the parts of zcat that are plain copies: x_i (agents are the first shared rows), the constant column, zero padding
  for (int idx = tid; idx < n * F; idx += 256) {
    const int i = idx / F, f = idx - i * F;
    zc[i * Kp + f] = s_xs[i * Fl + f];
  }
  const int kc = F + H * Wd;
  for (int idx = tid; idx < n * (Kp - kc); idx += 256) {
    const int i = idx / (Kp - kc), c = kc + idx - i * (Kp - kc);
    zc[i * Kp + c] = (c == kc) ? ones_col(t, mk + i * S) : 0.0f;
  }
}

__global__ void __launch_bounds__(256) attn_bwd_tiled_kernel(AttnArgs a) {
  extern __shared__ float sm[];
  const Topo& t = a.t;
  const TiledDims d = tiled_dims(t, a.F, a.H, a.TI);
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int n = t.n, S = t.S, Ns = t.Ns, F = a.F, H = a.H, Fl = d.Fl, Bl = d.Bl, Zl = d.Zl, NP = d.NP, NPl = d.NPl, NSHp = d.NSHp;
  const int Kp = a.Kp, Wd = F + 4;
  float* s_xs = sm;                         // NSHp * Fl   shared sender rows (resident)
  float* s_xp = s_xs + NSHp * Fl;           // TI * NP * Fl  private sender rows of the tile
  float* s_q = s_xp + d.TI * NP * Fl;       // Rp * Fl     query rows of the tile
  float* s_B = s_q + d.Rp * Fl;             // Rp * Bl     dA -> dL, then P (shared columns)
  float* s_z = s_B + d.Rp * Bl;             // Rp * Zl     dz rows (aggregated part: F features + 4 edge features)
  float* s_ap = s_z + d.Rp * Zl;            // Rp * NPl    attention weights of the private slots
  const float* dzc = a.dzcat + (size_t)g * n * Kp;
  const float4* ef4 = reinterpret_cast<const float4*>(a.efeat + (size_t)g * n * S * 4);
  const float* at = a.attn + (size_t)g * n * S * H;
  float* dq = a.dqt + (size_t)g * n * H * F;
  const bool want_dx = a.dXa != nullptr;
  const int ntile = d.CT * d.FT;
  f32x4g gacc[ATL_MAXT];
#pragma unroll
  for (int k = 0; k < ATL_MAXT; ++k) gacc[k] = f32x4g{0.f, 0.f, 0.f, 0.f};
  tiled_stage_shared(a, d, g, tid, s_xs);
  for (int i0 = 0; i0 < n; i0 += d.TI) {
    const int ti = min(d.TI, n - i0), rows = ti * H;
    tiled_stage_tile(a, d, g, tid, i0, ti, s_q, s_xp);
    for (int idx = tid; idx < d.Rp * Wd; idx += 256) {
      const int row = idx / Wd, w = idx - row * Wd;
      float v = 0.0f;
      if (row < rows) { const int il = row / H, h = row - il * H; v = dzc[(i0 + il) * Kp + F + h * Wd + w]; }
      s_z[row * Zl + w] = v;
    }
    __syncthreads();
    // ---- dA = dZx Xs^T: shared columns on the matrix cores, private columns slot-wise ----
    mfma_tiles(d.RT, d.CT, F / 4, wave, lane,
               [&](int row, int k) { return s_z[row * Zl + k]; },
               [&](int k, int col) { return s_xs[col * Fl + k]; },
               [&](int row, int col, float v) { s_B[row * Bl + col] = v; });
    for (int idx = tid; idx < rows * NP; idx += 256) {
      const int row = idx / NP, p = idx - row * NP;
      const float* z = s_z + row * Zl;
      const float* x = s_xp + ((row / H) * NP + p) * Fl;
      float acc = 0.0f;
      for (int f = 0; f < F; ++f) acc = fmaf(z[f], x[f], acc);
      s_B[row * Bl + NSHp + p] = acc;
    }
    __syncthreads();
    // ---- softmax backward dl = a (dA - sum_s a dA), 8 lanes per pair; dA gains the edge-feature term first ----
    for (int p0 = 0; p0 < rows; p0 += 32) {
      const int pair = p0 + (tid >> 3), sub = tid & 7;
      const bool live = pair < rows;
      const int il = live ? pair / H : 0, h = live ? pair - il * H : 0, i = i0 + il;
      float* brow = s_B + (live ? pair : 0) * Bl;
      const float* dze = s_z + (live ? pair : 0) * Zl + F;
      float dot = 0.0f;
      if (live)
        for (int s = sub; s < S; s += 8) {
          const int c = tiled_col(t, NSHp, s);
          const float av = at[(i * S + s) * H + h];
          float dA = 0.0f;
          if (av != 0.0f) {   // masked slots may carry 5e5 / NaN edge features: skip, never multiply
            const float4 e = ef4[i * S + s];
            dA = fmaf(dze[0], e.x, fmaf(dze[1], e.y, fmaf(dze[2], e.z, fmaf(dze[3], e.w, brow[c]))));
            dot = fmaf(av, dA, dot);
          }
          brow[c] = dA;
        }
      dot = grp8_sum(dot);
      if (live)
        for (int s = sub; s < S; s += 8) {
          const int c = tiled_col(t, NSHp, s);
          const float av = at[(i * S + s) * H + h];
          brow[c] = (av != 0.0f) ? av * (brow[c] - dot) : 0.0f;
          if (c >= NSHp) s_ap[pair * NPl + (c - NSHp)] = av;
        }
    }
    __syncthreads();
    // ---- dQt = dL Xs (+ the private slots) ----
    mfma_tiles(d.RT, d.FT, d.CT * 4, wave, lane,
               [&](int row, int k) { return s_B[row * Bl + k]; },
               [&](int k, int col) { return (col < F) ? s_xs[k * Fl + col] : 0.0f; },
               [&](int row, int col, float v) {
                 if (row < rows && col < F) {
                   const int il = row / H;
                   for (int p = 0; p < NP; ++p) {
                     const float dl = s_B[row * Bl + NSHp + p];
                     if (dl != 0.0f) v = fmaf(dl, s_xp[(il * NP + p) * Fl + col], v);
                   }
                   dq[(i0 * H + row) * F + col] = v;
                 }
               });
    if (want_dx) {
      // ---- shared nodes: gacc += dL^T Q (rows >= `rows` of B and Q are zero) ----
#pragma unroll
      for (int k = 0; k < ATL_MAXT; ++k) {
        const int tile = wave + 4 * k;
        if (tile < ntile) {
          const int rt = tile / d.FT, ct = tile - rt * d.FT;
          const int nd_a = rt * 16 + li, col_b = ct * 16 + li;
          for (int k4 = 0; k4 < d.RT * 4; ++k4) {
            const int kk = k4 * 4 + lq;
            const float bq = (col_b < F) ? s_q[kk * Fl + col_b] : 0.0f;
            gacc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_B[kk * Bl + nd_a], bq, gacc[k], 0, 0, 0);
          }
        }
      }
      // ---- private nodes: every row has one receiver, written directly ----
      if (a.dXo != nullptr) {
        for (int idx = tid; idx < ti * NP * F; idx += 256) {
          const int r = idx / F, f = idx - r * F, il = r / NP, p = r - il * NP;
          float acc = 0.0f;
          for (int h = 0; h < H; ++h) {
            const int row = il * H + h;
            acc = fmaf(s_ap[row * NPl + p], s_z[row * Zl + f], acc);
            acc = fmaf(s_B[row * Bl + NSHp + p], s_q[row * Fl + f], acc);
          }
          a.dXo[((size_t)g * (Ns - n) + (tiled_private_node(t, i0 + il, p) - n)) * F + f] = acc;
        }
      }
      __syncthreads();
      // ---- B <- P at the shared columns (zero padding), then gacc += P^T dZx ----
      for (int idx = tid; idx < d.Rp * NSHp; idx += 256) {
        const int row = idx / NSHp, j = idx - row * NSHp;
        float v = 0.0f;
        if (row < rows && j < d.NSH) { const int il = row / H, h = row - il * H; v = at[((i0 + il) * S + tiled_shared_slot(t, j)) * H + h]; }
        s_B[row * Bl + j] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < ATL_MAXT; ++k) {
        const int tile = wave + 4 * k;
        if (tile < ntile) {
          const int rt = tile / d.FT, ct = tile - rt * d.FT;
          const int nd_a = rt * 16 + li, col_b = ct * 16 + li;
          for (int k4 = 0; k4 < d.RT * 4; ++k4) {
            const int kk = k4 * 4 + lq;
            const float bz = (col_b < F) ? s_z[kk * Zl + col_b] : 0.0f;
            gacc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_B[kk * Bl + nd_a], bz, gacc[k], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- the shared nodes' gradient, once: agents also get the direct x_i part of dzcat ----
  if (want_dx) {
#pragma unroll
    for (int k = 0; k < ATL_MAXT; ++k) {
      const int tile = wave + 4 * k;
      if (tile < ntile) {
        const int rt = tile / d.FT, ct = tile - rt * d.FT;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = rt * 16 + lq * 4 + r, f = ct * 16 + li;
          if (j >= d.NSH || f >= F) continue;
          const int nd = tiled_shared_node(t, j);
          if (nd < n) a.dXa[((size_t)g * n + nd) * F + f] = gacc[k][r] + dzc[nd * Kp + f];
          else if (a.dXo != nullptr) a.dXo[((size_t)g * (Ns - n) + (nd - n)) * F + f] = gacc[k][r];
        }
      }
    }
  }
}

// receivers per tile: the largest of 16, 8, 4, 2, 1 whose image fits the default 64 KB of dynamic LDS (3 or 2 workgroups = 12 or 8
// waves per CU); only shapes that do not fit even with one receiver per tile (F = 64 with ~190 shared nodes) opt in to more
static int32_t attn_tiled_plan(AttnArgs& a, bool bwd, size_t& smem) {
  const TiledDims d0 = tiled_dims(a.t, a.F, a.H, 1);
  DGPPO_REQUIRE((a.F & 3) == 0 && a.F >= 8 && a.F <= 64 && d0.CT * d0.FT <= 4 * ATL_MAXT,
                "attn_%s: graph too large for LDS and no tiled kernel for F=%d (needs F %% 4 == 0, 8 <= F <= 64, shared nodes <= 192)",
                bwd ? "bwd" : "fwd", a.F);
  for (size_t cap : {(size_t)64 * 1024, (size_t)160 * 1024})
    for (int ti = 16; ti >= 1; ti >>= 1) {
      smem = attn_tiled_smem(tiled_dims(a.t, a.F, a.H, ti), bwd);
      if (smem <= cap) { a.TI = ti; return 0; }
    }
  DGPPO_REQUIRE(false, "attn_%s: one receiver tile needs %zu B of LDS, a CU has 160 KB", bwd ? "bwd" : "fwd", smem);
  return -1;
}
static int32_t launch_attn_tiled(AttnArgs& a, hipStream_t s, bool bwd) {
  size_t smem = 0;
  const int32_t rc = attn_tiled_plan(a, bwd, smem);
  if (rc) return rc;
  const void* fn = bwd ? reinterpret_cast<const void*>(&attn_bwd_tiled_kernel) : reinterpret_cast<const void*>(&attn_fwd_tiled_kernel);
  if (smem > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    DGPPO_REQUIRE(e == hipSuccess, "attn tiled: cannot reserve %zu bytes of LDS per workgroup: %s", smem, hipGetErrorString(e));
  }
  if (bwd) hipLaunchKernelGGL(attn_bwd_tiled_kernel, dim3(a.G), dim3(256), smem, s, a);
  else hipLaunchKernelGGL(attn_fwd_tiled_kernel, dim3(a.G), dim3(256), smem, s, a);
  return 0;
}

static int32_t attn_check(const dgppo_env_cfg* cfg, int F, int H, int Kp, int G, AttnArgs& a) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  a.t = make_topo(*cfg);
  DGPPO_REQUIRE(F >= 1 && F <= 64 && H >= 1 && H <= 8, "attn: bad F=%d H=%d", F, H);
  DGPPO_REQUIRE(Kp >= F + H * (F + 4) + 1, "attn: Kp=%d too small", Kp);
  DGPPO_REQUIRE(G >= 0, "attn: G < 0");
  a.F = F; a.H = H; a.Kp = Kp; a.G = G;
  return 0;
}

// The attention kernel families, chosen by shape alone; the first one whose conditions hold runs:
//   SLOT8  F = 8, H = 3, n <= 32, S <= 64 (attn_slot8_shape); the backward writes no input gradient (first layer only)
//   BD     F = 32 block-diagonal topologies (attn_bd_shape)
//   MFMA   one workgroup per graph on the matrix cores: F % 4 == 0, S <= 64, LDS image <= 64 KB; backward for F >= 16 only
//   VALU   one workgroup per graph, every other shape (and the narrow backward, where it beats MFMA: measured)
// Before any of them:
//   TILED  one workgroup per graph, receivers in tiles: every shape whose whole-graph image (attn_image_bytes, the VALU family's)
//          exceeds 64 KB, i.e. teams above ~17-35 agents depending on the kind (such calls were refused before this family
//          existed, so every other shape keeps its family); forward and backward cross that line at different n, the attn /
//          zcat layouts are the contract between the families
// The one-wave families (SLOT8, BD) store zcat rows in 16-byte pieces, hence Kp % 4 == 0.
enum class AttnFamily { SLOT8, BD, MFMA, VALU, TILED };
static size_t attn_image_bytes(const Topo& t, int F, int H, bool bwd) {
  if (bwd)
    return sizeof(float) * ((size_t)t.Ns * (F + 1) + (size_t)t.n * H * (F + 1) + (size_t)t.n * t.S * 4 + 2 * (size_t)t.n * t.S * H +
                            (size_t)t.n * H * (F + 5));
  return sizeof(float) * ((size_t)t.Ns * (F + 1) + (size_t)t.n * H * (F + 1) + (size_t)t.n * t.S * 5 + (size_t)t.n * t.S * H);
}
static AttnFamily attn_family(const Topo& t, int F, int H, int Kp, bool bwd, bool dXa) {
  int PS = 0;
  bool hits = false;
  if (attn_image_bytes(t, F, H, bwd) > 64 * 1024) return AttnFamily::TILED;
  if ((Kp & 3) == 0 && attn_slot8_shape(t, F, H) && !(bwd && dXa)) return AttnFamily::SLOT8;
  if ((Kp & 3) == 0 && attn_bd_shape(t, F, H, PS, hits)) return AttnFamily::BD;
  if ((F & 3) == 0 && t.S <= 64 && attn_mfma_smem(attn_dims(t, F, H), bwd) <= 64 * 1024 && (!bwd || F >= 16)) return AttnFamily::MFMA;
  return AttnFamily::VALU;
}

extern "C" int32_t dgppo_attn_fwd(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt,
                                  const float* Xa, const float* Xo, const float* efeat, const float* emask, float* zcat,
                                  float* attn, int32_t G, void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  if (G == 0) return 0;
  DGPPO_REQUIRE(qt && Xa && efeat && emask && zcat, "attn_fwd: NULL operand");      // attn == NULL: inference, weights not kept
  DGPPO_REQUIRE(a.t.Ns == a.t.n || Xo, "attn_fwd: Xo is NULL");
  a.qt = qt; a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.zcat = zcat; a.attn = attn;
  const Topo& t = a.t;
  const hipStream_t s = (hipStream_t)stream;
  const size_t smem = attn_image_bytes(t, F, H, false);
  bool launched = true;
  switch (attn_family(t, F, H, Kp, false, false)) {
    case AttnFamily::SLOT8: launched = launch_attn_slot8(a, s, false); break;
    case AttnFamily::BD: launched = launch_attn_bd(a, s, false); break;
    case AttnFamily::MFMA:
      hipLaunchKernelGGL(attn_fwd_kernel, dim3(G), dim3(256), attn_mfma_smem(attn_dims(t, F, H), false), s, a);
      break;
    case AttnFamily::VALU: hipLaunchKernelGGL(attn_fwd_valu_kernel, dim3(G), dim3(256), smem, s, a); break;
    case AttnFamily::TILED:
      rc = launch_attn_tiled(a, s, false);
      if (rc) return rc;
      break;
  }
  DGPPO_REQUIRE(launched, "attn_fwd: dispatch failed");
  DGPPO_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t dgppo_attn_bwd(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                                  const float* attn, const float* qt, const float* Xa, const float* Xo,
                                  const float* efeat, float* dqt, float* dXa, float* dXo, int32_t relu_xo, int32_t G,
                                  void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  if (G == 0) return 0;
  DGPPO_REQUIRE(dzcat && attn && qt && Xa && efeat && dqt, "attn_bwd: NULL operand");
  DGPPO_REQUIRE(a.t.Ns == a.t.n || Xo, "attn_bwd: Xo is NULL");
  DGPPO_REQUIRE(!(dXo && !dXa), "attn_bwd: dXo needs dXa");
  a.dzcat = dzcat; a.attn = (float*)attn; a.qt = qt; a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.dqt = dqt; a.dXa = dXa; a.dXo = dXo;
  const Topo& t = a.t;
  const hipStream_t s = (hipStream_t)stream;
  const size_t smem = attn_image_bytes(t, F, H, true);
  const AttnFamily fam = attn_family(t, F, H, Kp, true, dXa != nullptr);
  a.relu_xo = (relu_xo && dXo && fam == AttnFamily::BD) ? 1 : 0;     // fused into the block-diagonal kernel's dXo store
  bool launched = true;
  switch (fam) {
    case AttnFamily::SLOT8: launched = launch_attn_slot8(a, s, true); break;
    case AttnFamily::BD: launched = launch_attn_bd(a, s, true); break;
    case AttnFamily::MFMA:
      hipLaunchKernelGGL(attn_bwd_kernel, dim3(G), dim3(256), attn_mfma_smem(attn_dims(t, F, H), true), s, a);
      break;
    case AttnFamily::VALU: hipLaunchKernelGGL(attn_bwd_valu_kernel, dim3(G), dim3(256), smem, s, a); break;
    case AttnFamily::TILED:
      rc = launch_attn_tiled(a, s, true);
      if (rc) return rc;
      break;
  }
  DGPPO_REQUIRE(launched, "attn_bwd: dispatch failed");
  DGPPO_LAUNCH_CHECK();
  if (relu_xo && dXo && !a.relu_xo)    // the workgroup kernels do not fuse the ReLU mask of the other nodes' gradient: separate pass
    return dgppo_relu_bwd(dXo, Xo, (int64_t)G * (t.Ns - t.n) * F, stream);
  return 0;
}

// ---- the same layer with the other nodes' rows recomputed inside the kernel (block-diagonal kernels only) ------------------
// Xo = relu(Xo_raw Wo + bo), Xo_raw [G*(Ns-n), 8] = the padded raw features of goals / hits / obstacles, Wo [8, ldwo >= 32] =
// the first 8 rows of the previous layer's update weight, bo [32] its bias: what the reference computes for nodes without
// incoming edges (gnn.py:109-111 with aggr = 0) and then feeds to the next GraphTransformer layer as sender rows
// (gnn.py:85-117).  dgppo_attn_xo_supported tells the caller whether the topology has such a kernel; if not, materialise Xo
// (dgppo_dense_fwd) and call dgppo_attn_fwd / dgppo_attn_bwd.
static bool attn_xo_ok(const Topo& t, int F, int H, int Kp) {
  return t.Ns > t.n && attn_family(t, F, H, Kp, true, true) == AttnFamily::BD;
}
extern "C" int32_t dgppo_attn_xo_supported(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp) {
  AttnArgs a{};
  if (attn_check(cfg, F, H, Kp, 0, a)) return 0;
  return attn_xo_ok(a.t, F, H, Kp) ? 1 : 0;
}
extern "C" int32_t dgppo_attn_fwd_xo(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt, const float* Xa,
                                     const float* Xo_raw, const float* Wo, int32_t ldwo, const float* bo, const float* efeat,
                                     const float* emask, float* zcat, float* attn, int32_t G, void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  if (G == 0) return 0;
  DGPPO_REQUIRE(qt && Xa && Xo_raw && Wo && bo && efeat && emask && zcat, "attn_fwd_xo: NULL operand");
  DGPPO_REQUIRE(ldwo >= 32, "attn_fwd_xo: ldwo=%d < 32", ldwo);
  DGPPO_REQUIRE(attn_xo_ok(a.t, F, H, Kp), "attn_fwd_xo: no fused kernel for this topology (ask dgppo_attn_xo_supported)");
  a.qt = qt; a.Xa = Xa; a.Xo = nullptr; a.efeat = efeat; a.emask = emask; a.zcat = zcat; a.attn = attn;
  a.Xo_raw = Xo_raw; a.Wo = Wo; a.ldwo = ldwo; a.bo = bo;
  const bool launched = launch_attn_bd(a, (hipStream_t)stream, false);
  DGPPO_REQUIRE(launched, "attn_fwd_xo: dispatch failed");
  DGPPO_LAUNCH_CHECK();
  return 0;
}
extern "C" int32_t dgppo_attn_bwd_xo(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                                     const float* attn, const float* qt, const float* Xa, const float* Xo_raw, const float* Wo,
                                     int32_t ldwo, const float* bo, const float* efeat, float* dqt, float* dXa, float* dXo,
                                     int32_t relu_xo, int32_t G, void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  if (G == 0) return 0;
  DGPPO_REQUIRE(dzcat && attn && qt && Xa && Xo_raw && Wo && bo && efeat && dqt, "attn_bwd_xo: NULL operand");
  DGPPO_REQUIRE(ldwo >= 32, "attn_bwd_xo: ldwo=%d < 32", ldwo);
  DGPPO_REQUIRE(!(dXo && !dXa), "attn_bwd_xo: dXo needs dXa");
  DGPPO_REQUIRE(attn_xo_ok(a.t, F, H, Kp), "attn_bwd_xo: no fused kernel for this topology (ask dgppo_attn_xo_supported)");
  a.dzcat = dzcat; a.attn = (float*)attn; a.qt = qt; a.Xa = Xa; a.Xo = nullptr; a.efeat = efeat; a.dqt = dqt; a.dXa = dXa; a.dXo = dXo;
  a.relu_xo = (relu_xo && dXo) ? 1 : 0;
  a.Xo_raw = Xo_raw; a.Wo = Wo; a.ldwo = ldwo; a.bo = bo;
  const bool launched = launch_attn_bd(a, (hipStream_t)stream, true);
  DGPPO_REQUIRE(launched, "attn_bwd_xo: dispatch failed");
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// sum of the per-graph slabs of attn_bwd_bd_kernel<.., XOF>: dWo [8, lddwo] += , dbo [32] +=
__global__ void __launch_bounds__(320) attn_xo_dw_reduce_kernel(const float* slab, int G, float* dWo, int lddwo, float* dbo) {
  const int e = threadIdx.x;                      // 0..287: k * 32 + f, then the 32 bias entries
  if (e >= 288) return;
  const int per = (G + gridDim.x - 1) / gridDim.x;
  const int g0 = blockIdx.x * per, g1 = min(G, g0 + per);
  float sacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int g = g0;
  for (; g + 7 < g1; g += 8) {                     // eight loads in flight per thread
#pragma unroll
    for (int u = 0; u < 8; ++u) sacc[u] += slab[(size_t)(g + u) * ABD_DW_STRIDE + e];
  }
  for (; g < g1; ++g) sacc[0] += slab[(size_t)g * ABD_DW_STRIDE + e];
  const float sum = ((sacc[0] + sacc[1]) + (sacc[2] + sacc[3])) + ((sacc[4] + sacc[5]) + (sacc[6] + sacc[7]));
  if (g0 >= g1) return;
  if (e < 256) atomicAdd(dWo + (size_t)(e >> 5) * lddwo + (e & 31), sum);
  else atomicAdd(dbo + (e - 256), sum);
}
extern "C" int64_t dgppo_attn_xo_workspace_bytes(int32_t G) { return G < 0 ? 0 : (int64_t)G * ABD_DW_STRIDE * (int64_t)sizeof(float); }
// dgppo_attn_bwd_xo that CONSUMES the gradient of the recomputed rows instead of writing it: dWo [8, lddwo] += Xo_raw^T dpre,
// dbo [32] += colsum dpre with dpre = relu'(Xo) * dXo — the weight gradient jax.grad assigns to the previous layer's update Dense
// for the nodes without incoming edges (gnn.py:109-111).  workspace: dgppo_attn_xo_workspace_bytes(G) bytes, caller-owned.
extern "C" int32_t dgppo_attn_bwd_xo_dw(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                                        const float* attn, const float* qt, const float* Xa, const float* Xo_raw, const float* Wo,
                                        int32_t ldwo, const float* bo, const float* efeat, float* dqt, float* dXa, float* dWo,
                                        int32_t lddwo, float* dbo, float* workspace, int64_t workspace_bytes, int32_t G,
                                        void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  if (G == 0) return 0;
  DGPPO_REQUIRE(dzcat && attn && qt && Xa && Xo_raw && Wo && bo && efeat && dqt && dXa && dWo && dbo && workspace,
                "attn_bwd_xo_dw: NULL operand");
  DGPPO_REQUIRE(ldwo >= 32 && lddwo >= 32, "attn_bwd_xo_dw: ldwo=%d lddwo=%d < 32", ldwo, lddwo);
  DGPPO_REQUIRE(workspace_bytes >= dgppo_attn_xo_workspace_bytes(G) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                "attn_bwd_xo_dw: workspace too small or not 16-byte aligned");
  DGPPO_REQUIRE(attn_xo_ok(a.t, F, H, Kp), "attn_bwd_xo_dw: no fused kernel for this topology (ask dgppo_attn_xo_supported)");
  a.dzcat = dzcat; a.attn = (float*)attn; a.qt = qt; a.Xa = Xa; a.Xo = nullptr; a.efeat = efeat; a.dqt = dqt; a.dXa = dXa; a.dXo = nullptr;
  a.relu_xo = 1;
  a.Xo_raw = Xo_raw; a.Wo = Wo; a.ldwo = ldwo; a.bo = bo; a.dwo_slab = workspace;
  const bool launched = launch_attn_bd(a, (hipStream_t)stream, true);
  DGPPO_REQUIRE(launched, "attn_bwd_xo_dw: dispatch failed");
  int blocks = (G + 31) / 32;                      // 32 graphs per workgroup: <= 512 atomics per address at 16 384 graphs
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  hipLaunchKernelGGL(attn_xo_dw_reduce_kernel, dim3(blocks), dim3(320), 0, (hipStream_t)stream, workspace, G, dWo, lddwo, dbo);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
