// Graph features of the per-agent fixed-fan-in graph: only agents receive messages and every sender slot of an agent has a static
// node id (dgppo/utils/graph.py:35-44, dgppo/env/lidar_env/lidar_spread.py:57-96), see nn_attn.h.
#include "graph_topo.h"

// ---------------------------------------------------------------------------------------------------------------------
// graph features: compact record -> agent/other node feature matrices, per-slot edge features and masks.
// Same arithmetic (single rounded operations, no product contracted into a difference: see feat4) as env_step.hip phase 5, i.e. as
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
  int vecX, vecM;                    // 16-byte stores of the node rows (Fp % 4 == 0, aligned) / of the masks (n*S % 4 == 0, aligned)
  uint32_t rcp_fp, rcp_fq, rcp_S;    // ceil(2^32 / d): index divisions by Fp, Fp/4 and S as one v_mul_hi_u32 (exact for idx < 2^16)
};

// One wave owns one graph and walks graphs g, g + stride, ...: no workgroup barrier anywhere.  The record of a graph
// ([agent | goal | hits or obst], R floats) sits in a wave-private LDS slice.  Its first GF_PF * 64 floats are requested into
// registers ONE GRAPH AHEAD, before the stores of the current graph are issued (as gru_fwd_kernel stages its next h0 tile),
// so a wave's load latency hides behind its own stores; what a larger record (teams above ~20 agents) has beyond that is
// loaded at the top of its graph.
#define GF_PF 8
// LDS of a wave is written and read by that wave alone and LDS operations of one wave complete in order: ordering the
// compiler is all it takes (no instruction is emitted)
#define GF_WAVE_SYNC()                                  \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                    \
  } while (0)

struct FeatRec { const float *ag, *go, *ob; };

// the 4 edge-feature inputs of an agent / goal state: [x, y, vx, vy], with the bicycle's v * (cos, sin) products
template <int SD>
__device__ inline float4 feat4(const float* s) {
  if constexpr (SD == 5) {
    // the products are ROUNDED before the edge subtraction reads them (state2feat, then the difference): the empty asm keeps
    // the compiler from contracting product and difference into one fma (no instruction is emitted)
    float vx = __fmul_rn(s[4], s[2]), vy = __fmul_rn(s[4], s[3]);
    asm volatile("" : "+v"(vx), "+v"(vy));
    return make_float4(s[0], s[1], vx, vy);
  } else {
    return make_float4(s[0], s[1], s[2], s[3]);
  }
}

template <int SD>
__global__ void __launch_bounds__(256) graph_feats_kernel(FeatArgs a) {
  extern __shared__ float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const Topo& t = a.t;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wpb = blockDim.x >> 6;
  const int n = t.n, ng = t.ng, S = t.S, Fp = a.Fp;
  const int n_on = t.Ns - n - ng;
  const int nA = n * SD, nG = ng * SD, nO = n_on * (t.lidar ? 2 : SD), R = nA + nG + nO;   // LiDAR hit nodes: (x, y) only
  float* s_ag = sm + (size_t)wv * R;   // n*SD
  float* s_go = s_ag + nA;             // ng*SD
  float* s_ob = s_go + nG;             // hits [n_on, 2] or obstacle states [n_on, SD]
  const long G = (long)a.n_env * a.n_time, stride = (long)gridDim.x * wpb;
  long g = (long)blockIdx.x * wpb + wv;
  if (g >= G) return;
  // the env of a graph is read TWO graphs ahead, so that the record's addresses never wait for an env_ids load
  auto env_of = [&](long gg) { const int e = (int)gg / a.n_time; return a.env_ids ? (int)a.env_ids[e] : e; };
  auto locate = [&](long gg, int env) {
    const int tt = (int)gg % a.n_time;
    FeatRec p;
    p.ag = a.agent + (size_t)env * a.agent_se + (size_t)tt * a.agent_st;
    p.go = a.goal + (size_t)env * nG;
    p.ob = nullptr;
    if (nO > 0) p.ob = t.lidar ? a.hits + (size_t)env * a.hits_se + (size_t)tt * a.hits_st : a.obst + (size_t)env * nO;
    return p;
  };
  auto fetch = [&](const FeatRec& p, int i) { return i < nA ? p.ag[i] : (i < nA + nG ? p.go[i - nA] : p.ob[i - nA - nG]); };
  float r0, r1, r2, r3, r4, r5, r6, r7;   // (plain floats: an array captured by a lambda may end up in scratch)
  static_assert(GF_PF == 8, "one register per prefetched dword");
#define GF_EACH(OP) OP(r0, 0) OP(r1, 1) OP(r2, 2) OP(r3, 3) OP(r4, 4) OP(r5, 5) OP(r6, 6) OP(r7, 7)
#define GF_REQUEST(r, j) { const int i = lane + 64 * j; r = 0.0f; if (i < R) r = fetch(p, i); }
#define GF_COMMIT(r, j)  { const int i = lane + 64 * j; if (i < R) s_ag[i] = r; }
  FeatRec p = locate(g, env_of(g));
  GF_EACH(GF_REQUEST)
  long gn = g + stride;
  int env_n = gn < G ? env_of(gn) : 0;
  for (;;) {
    GF_EACH(GF_COMMIT)
    for (int i = GF_PF * 64 + lane; i < R; i += 64) s_ag[i] = fetch(p, i);
    GF_WAVE_SYNC();
    const bool more = gn < G;
    if (more) {
      p = locate(gn, env_n);
      GF_EACH(GF_REQUEST)
      if (gn + stride < G) env_n = env_of(gn + stride);
    }
    // node feature rows: [state | obs, goal, agent indicator], zero padded to Fp
    auto node_src = [&](int nd, const float*& src, int& ns, int& one) {
      if (nd < n) { src = s_ag + nd * SD; ns = SD; one = SD + 2; }
      else if (nd < n + ng) { src = s_go + (nd - n) * SD; ns = SD; one = SD + 1; }
      else if (t.lidar) { src = s_ob + (nd - n - ng) * 2; ns = 2; one = SD; }    // hit node: (x, y, 0, ...)
      else { src = s_ob + (nd - n - ng) * SD; ns = SD; one = SD; }
    };
    if (a.vecX) {
      const int Fq = Fp >> 2;
      for (int q = lane; q < t.Ns * Fq; q += 64) {
        const int nd = (int)__umulhi((uint32_t)q, a.rcp_fq), col0 = (q - nd * Fq) * 4;
        const float* src; int ns, one;
        node_src(nd, src, ns, one);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int col = col0 + k;
          v[k] = (col < ns) ? src[col] : ((col == one) ? 1.0f : 0.0f);
        }
        float* dst = (nd < n) ? a.Xa + ((size_t)g * n + nd) * Fp + col0 : a.Xo + ((size_t)g * (t.Ns - n) + (nd - n)) * Fp + col0;
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else {
      for (int idx = lane; idx < t.Ns * Fp; idx += 64) {
        const int nd = (int)__umulhi((uint32_t)idx, a.rcp_fp), col = idx - nd * Fp;
        const float* src; int ns, one;
        node_src(nd, src, ns, one);
        const float v = (col < ns) ? src[col] : ((col == one) ? 1.0f : 0.0f);
        if (nd < n) a.Xa[((size_t)g * n + nd) * Fp + col] = v;
        else a.Xo[((size_t)g * (t.Ns - n) + (nd - n)) * Fp + col] = v;
      }
    }
    // per-slot edge feature + mask
    const int nE = n * S;
    for (int base = 0; base < nE; base += 64) {
      const int idx = base + lane;
      bool mask = false;
      if (idx < nE) {
        const int i = (int)__umulhi((uint32_t)idx, a.rcp_S), s = idx - i * S;
        float4 f;
        const float4 fi = feat4<SD>(s_ag + i * SD);
        const float px = s_ag[i * SD], py = s_ag[i * SD + 1];
        if (s < n) {
          const float4 fj = feat4<SD>(s_ag + s * SD);
          f = make_float4(__fsub_rn(fi.x, fj.x), __fsub_rn(fi.y, fj.y), __fsub_rn(fi.z, fj.z), __fsub_rn(fi.w, fj.w));
          float d = __fadd_rn(dist_rn(__fsub_rn(px, s_ag[s * SD]), __fsub_rn(py, s_ag[s * SD + 1])), (i == s) ? c.eye_offset : 0.0f);
          mask = d < c.comm_radius;
        } else if (s < n + t.gs) {
          const int gi = t.spread ? (s - n) : i;
          const float4 fg = feat4<SD>(s_go + gi * SD);
          f = make_float4(__fsub_rn(fi.x, fg.x), __fsub_rn(fi.y, fg.y), __fsub_rn(fi.z, fg.z), __fsub_rn(fi.w, fg.w));
          mask = true;
        } else {
          const int m = s - n - t.gs;
          if (t.lidar) {
            const float* hp = s_ob + (i * t.per + m) * 2;
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
        reinterpret_cast<float4*>(a.efeat)[(size_t)g * nE + idx] = f;
        if (!a.vecM) a.emask[(size_t)g * nE + idx] = mask ? 1.0f : 0.0f;
      }
      if (a.vecM) {   // the 64 masks of this pass as a bit set: lanes 0..15 write four each
        const unsigned long long bits = __ballot(mask);
        const int i4 = base + 4 * lane;
        if (lane < 16 && i4 < nE) {
          const unsigned b = (unsigned)(bits >> (4 * lane));
          *reinterpret_cast<float4*>(a.emask + (size_t)g * nE + i4) =
              make_float4((b & 1u) ? 1.0f : 0.0f, (b & 2u) ? 1.0f : 0.0f, (b & 4u) ? 1.0f : 0.0f, (b & 8u) ? 1.0f : 0.0f);
        }
      }
    }
    GF_WAVE_SYNC();
    if (!more) break;
    g = gn;
    gn += stride;
  }
#undef GF_EACH
#undef GF_REQUEST
#undef GF_COMMIT
}

// resident workgroups of the kernel on the current device (occupancy x CUs), remembered for the last launch shape
static int feats_grid_cap(const void* fn, int wpb, size_t smem) {
  static thread_local const void* k_fn = nullptr;
  static thread_local int k_wpb = 0, k_cap = 0;
  static thread_local size_t k_smem = 0;
  if (fn == k_fn && wpb == k_wpb && smem == k_smem) return k_cap;
  int per_cu = 0, dev = 0, cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * wpb, smem) != hipSuccess || per_cu < 1) per_cu = 1;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  k_fn = fn; k_wpb = wpb; k_smem = smem; k_cap = per_cu * cus;
  return k_cap;
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
  a.vecX = (Fp % 4 == 0 && ((uintptr_t)Xa & 15) == 0 && ((uintptr_t)Xo & 15) == 0) ? 1 : 0;     // (Fp >= node_dim >= 7: Fp / 4 >= 2)
  a.vecM = ((a.t.n * a.t.S) % 4 == 0 && ((uintptr_t)emask & 15) == 0) ? 1 : 0;
  a.rcp_fq = a.vecX ? (uint32_t)((0x100000000ull + (uint64_t)(Fp / 4) - 1) / (uint64_t)(Fp / 4)) : 0u;
  const int SD = cfg->state_dim;
  // the record of one graph in a wave's LDS slice; four waves per workgroup unless a large team's records do not fit
  const size_t rec = sizeof(float) * ((size_t)a.t.n * SD + (size_t)a.t.ng * SD + (size_t)n_on * (a.t.lidar ? 2 : SD));
  int wpb = 4;
  while (wpb > 1 && rec * wpb > 65536) wpb >>= 1;
  const long G = (long)n_env * n_time;
  const void* fn = SD == 5 ? reinterpret_cast<const void*>(&graph_feats_kernel<5>) : reinterpret_cast<const void*>(&graph_feats_kernel<4>);
  const int cap = feats_grid_cap(fn, wpb, rec * wpb);
  const long wgs = (G + wpb - 1) / wpb;
  const dim3 grid((unsigned)(wgs < cap ? wgs : cap)), block(64 * wpb);
  if (SD == 5) hipLaunchKernelGGL(graph_feats_kernel<5>, grid, block, rec * wpb, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(graph_feats_kernel<4>, grid, block, rec * wpb, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
