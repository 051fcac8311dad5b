// Vh landscape: the graph features of one frozen frame with ONE agent moved over a grid of positions — what the
// reference's renderer consumes as viz_opts["cbf"] (dgppo/env/plot.py:348-372,437-447) and ships no producer for.
//
// Graph g = (f * ny + iy) * nx + ix is the graph of frame fid = frame_ids[f] in which agent `agent_id` stands at
// (xs[ix], ys[iy]): its velocity (bicycle: heading and speed) is kept, its k LiDAR hit points are cast again from the new
// position (get_lidar, env/utils.py:115-136: start-inside factor, det == 0 NaN rays, stable top-k), every other agent's hit
// points are the recorded ones.  The outputs have the layout and arithmetic of dgppo_graph_feats (graph_feats.hip) for G graphs.
//
// Organisation: a workgroup stages the frame (states, goals, rectangle segments, recorded hits) in LDS once — per tile of
// 64 grid points, a few hundred floats that stay in L2 across the tiles of a frame — and walks the tile, one wave per point: the wave casts the R rays of the moved agent, ranks them, and streams the graph's four
// dense outputs with unit-stride stores (edge features as float4).  Consecutive points are consecutive graphs, so the four
// waves of a pass write one contiguous range of each output.
//
// Built with -ffp-contract=off; the ray arithmetic is env_step.h's (shared with env_step.hip), the slot topology
// graph_topo.h's (shared with graph_feats.hip).
#include <string>

#include "env_step.h"
#include "graph_topo.h"

#define SWEEP_NT 256
#define SWEEP_WAVES (SWEEP_NT / DGPPO_WAVE)
#define SWEEP_TILE 64   // grid points per workgroup

struct SweepArgs {
  dgppo_env_cfg cfg;
  Topo t;
  const float* agent; long agent_st;
  const float* goal;
  const float* obst;
  const float* hits; long hits_st;
  const float* ray_cos;
  const float* ray_sin;
  const int32_t* frame_ids;
  int agent_id, nx, nxy, tiles;
  const float* xs;
  const float* ys;
  float* Xa;
  float* Xo;
  float* efeat;
  float* emask;
  float* hits_out;
  int Fp;
  uint32_t rcp_fp, rcp_S;   // ceil(2^32 / d): index divisions by Fp and S as one v_mul_hi_u32 (exact for idx < 2^16)
};

// orders the LDS accesses of ONE wave around it: its earlier writes are visible to its later reads
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline int sweep_div(int x, uint32_t rcp) { return (int)__umulhi((uint32_t)x, rcp); }

template <int SD>
__global__ void __launch_bounds__(SWEEP_NT) graph_feats_sweep_kernel(SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const Topo& t = a.t;
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int fid = a.frame_ids ? a.frame_ids[f] : f;
  const int n = t.n, ng = t.ng, S = t.S, Fp = a.Fp, aid = a.agent_id;
  const int n_on = t.Ns - n - ng;
  const int no = c.n_obs, R = c.n_rays, k = c.top_k;
  const bool cast = t.lidar && n_on > 0;
  // LDS carve: every offset is a multiple of 4 floats
  const int al4 = 3;
  float* s_seg = sm;                                             // no*16 segment constants (LiDAR)
  float* s_rec = s_seg + (cast ? no * 16 : 0);                   // no*16 rectangle records (LiDAR) | n_obs*SD (MPE)
  float* s_ag = s_rec + (((t.lidar ? (cast ? no * 16 : 0) : n_on * SD) + al4) & ~al4);   // n*SD
  float* s_go = s_ag + ((n * SD + al4) & ~al4);                  // ng*SD
  float* s_fa = s_go + ((ng * SD + al4) & ~al4);                 // n*4   state2feat(agent), the moved agent's at its base position
  float* s_fg = s_fa + n * 4;                                    // ng*4
  float* s_hp = s_fg + ng * 4;                                   // n*k*2 recorded hits (LiDAR)
  float* s_rc = s_hp + (cast ? ((n * k * 2 + al4) & ~al4) : 0);  // R
  float* s_rs = s_rc + (cast ? ((R + al4) & ~al4) : 0);          // R
  float* s_al = s_rs + (cast ? ((R + al4) & ~al4) : 0);          // waves * R   alphas of the wave's point
  float* s_hit = s_al + (cast ? SWEEP_WAVES * ((R + al4) & ~al4) : 0);   // waves * k*2 hits of the moved agent
  const int Rp = (R + al4) & ~al4, K2 = (k * 2 + al4) & ~al4;

  // ---- the frame, once per workgroup ----
  const float* ag = a.agent + (size_t)fid * a.agent_st;
  for (int i = tid; i < n * SD; i += SWEEP_NT) s_ag[i] = ag[i];
  for (int i = tid; i < ng * SD; i += SWEEP_NT) s_go[i] = a.goal[i];
  if (cast) {
    for (int i = tid; i < no * 16; i += SWEEP_NT) s_rec[i] = a.obst[i];
    const float* hp = a.hits + (size_t)fid * a.hits_st;
    for (int i = tid; i < n * k * 2; i += SWEEP_NT) s_hp[i] = hp[i];
    for (int i = tid; i < R; i += SWEEP_NT) { s_rc[i] = a.ray_cos[i]; s_rs[i] = a.ray_sin[i]; }
  } else if (!t.lidar) {
    for (int i = tid; i < n_on * SD; i += SWEEP_NT) s_rec[i] = a.obst[i];
  }
  __syncthreads();
  if (cast)
    for (int q = tid; q < no * 4; q += SWEEP_NT) segment_consts(s_rec + (q >> 2) * DGPPO_RECT_STRIDE, q & 3, s_seg + q * 4);
  for (int i = tid; i < n + ng; i += SWEEP_NT)
    state2feat<SD>((i < n) ? s_ag + i * SD : s_go + (i - n) * SD, (i < n) ? s_fa + i * 4 : s_fg + (i - n) * 4);
  __syncthreads();

  const int q0 = tile * SWEEP_TILE, q1 = min(q0 + SWEEP_TILE, a.nxy);
  float* w_al = s_al + wave * Rp;
  float* w_hit = s_hit + wave * K2;
  const float sr = c.comm_radius;
  constexpr int ND = SD + 3;
  // from here on the waves are independent: w_al / w_hit belong to one wave, whose LDS operations complete in issue order,
  // so between its phases a wave-level fence (no reordering by the compiler, no workgroup barrier) is enough
  for (int q = q0 + wave; q < q1; q += SWEEP_WAVES) {
    const int iy = q / a.nx, ix = q - iy * a.nx;
    const float px = a.xs[ix], py = a.ys[iy];
    if (cast) {
      {
        // start inside a rectangle (env/utils.py:117, r = 0): all alphas become 0
        bool in = false;
        for (int o = lane; o < no; o += DGPPO_WAVE) in = in || rect_inside(s_rec + o * DGPPO_RECT_STRIDE, px, py, 0.0f);
        const float is_in = (__ballot(in) != 0ull) ? 1.0f : 0.0f;
        for (int r = lane; r < R; r += DGPPO_WAVE)
          w_al[r] = ray_min_alpha(px, py, s_rc[r], s_rs[r], sr, s_seg, no) * (1.0f - is_in);
      }
      wave_sync();
      for (int r = lane; r < R; r += DGPPO_WAVE) {
        const int rank = ray_rank(w_al, R, r);
        if (rank < k) ray_hit(px, py, s_rc[r], s_rs[r], sr, w_al[r], w_hit + rank * 2);
      }
      wave_sync();
    }
    const size_t g = (size_t)f * a.nxy + q;
    // position and feature row of agent i in this graph
    auto posx = [&](int i) { return (i == aid) ? px : s_ag[i * SD]; };
    auto posy = [&](int i) { return (i == aid) ? py : s_ag[i * SD + 1]; };
    auto feat = [&](int i, int d) { return (i == aid && d < 2) ? (d == 0 ? px : py) : s_fa[i * 4 + d]; };
    // hit point m of agent i
    auto hit = [&](int i, int m) { return (i == aid) ? w_hit + m * 2 : s_hp + (i * k + m) * 2; };

    // node feature rows: [state | obs, goal, agent indicator], zero padded to Fp
    float* xa = a.Xa + g * n * Fp;
    for (int idx = lane; idx < n * Fp; idx += DGPPO_WAVE) {
      const int nd = sweep_div(idx, a.rcp_fp), col = idx - nd * Fp;
      float v = (col < SD) ? s_ag[nd * SD + col] : ((col == SD + 2) ? 1.0f : 0.0f);
      if (nd == aid && col < 2) v = (col == 0) ? px : py;
      if (col >= ND) v = 0.0f;
      xa[idx] = v;
    }
    float* xo = a.Xo + g * (t.Ns - n) * Fp;
    for (int idx = lane; idx < (t.Ns - n) * Fp; idx += DGPPO_WAVE) {
      const int r = sweep_div(idx, a.rcp_fp), col = idx - r * Fp;
      float v;
      if (r < ng) v = (col < SD) ? s_go[r * SD + col] : ((col == SD + 1) ? 1.0f : 0.0f);
      else {
        const int qn = r - ng;
        if (t.lidar) {
          const int m = qn - aid * k;
          const float* hp = (m >= 0 && m < k) ? w_hit + m * 2 : s_hp + qn * 2;
          v = (col < 2) ? hp[col] : ((col == SD) ? 1.0f : 0.0f);
        } else {
          v = (col < SD) ? s_rec[qn * SD + col] : ((col == SD) ? 1.0f : 0.0f);
        }
      }
      if (col >= ND) v = 0.0f;
      xo[idx] = v;
    }
    // per-slot edge feature + mask (lidar_env/base.py:227-271, lidar_spread.py:57-96 and the MPE twins)
    float4* ef = reinterpret_cast<float4*>(a.efeat) + g * n * S;
    float* em = a.emask + g * n * S;
    for (int idx = lane; idx < n * S; idx += DGPPO_WAVE) {
      const int i = sweep_div(idx, a.rcp_S), s = idx - i * S;
      float4 fe;
      bool mask;
      const float xi = posx(i), yi = posy(i);
      if (s < n) {
        fe = make_float4(feat(i, 0) - feat(s, 0), feat(i, 1) - feat(s, 1), feat(i, 2) - feat(s, 2), feat(i, 3) - feat(s, 3));
        const float d = dist_rn(xi - posx(s), yi - posy(s)) + ((i == s) ? c.eye_offset : 0.0f);
        mask = d < c.comm_radius;
      } else if (s < n + t.gs) {
        const float* fg = s_fg + (t.spread ? (s - n) : i) * 4;
        fe = make_float4(feat(i, 0) - fg[0], feat(i, 1) - fg[1], feat(i, 2) - fg[2], feat(i, 3) - fg[3]);
        mask = true;
      } else {
        const int m = s - n - t.gs;
        if (t.lidar) {
          const float* hp = hit(i, m);
          const float lx = xi - hp[0], ly = yi - hp[1];
          fe = make_float4(lx, ly, 0.0f, 0.0f);
          mask = dist_rn(lx, ly) < c.lidar_mask_radius;
        } else {
          const float* xob = s_rec + m * SD;
          const float dx = xi - xob[0], dy = yi - xob[1];
          fe = make_float4(dx, dy, s_ag[i * SD + 2] - xob[2], s_ag[i * SD + 3] - xob[3]);
          mask = dist_rn(dx, dy) < c.obs_mask_radius;
        }
      }
      ef[idx] = fe;
      em[idx] = mask ? 1.0f : 0.0f;
    }
    if (cast && a.hits_out != nullptr)
      for (int i = lane; i < k * 2; i += DGPPO_WAVE) a.hits_out[g * k * 2 + i] = w_hit[i];
    wave_sync();   // the next point's cast overwrites w_al / w_hit
  }
}

extern "C" int32_t dgppo_graph_feats_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                           const float* obst, const float* hits, int64_t hits_st, const float* ray_cos,
                                           const float* ray_sin, const int32_t* frame_ids, int32_t n_frames, int32_t agent_id,
                                           const float* xs, int32_t nx, const float* ys, int32_t ny, float* Xa, float* Xo,
                                           float* efeat, float* emask, float* hits_out, int32_t Fp, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_graph_feats_sweep", "dgppo_vmas_graph_feats on a tiled record (there is no VMAS sweep)");
  DGPPO_REQUIRE(agent_id >= 0 && agent_id < cfg->n_agents, "dgppo_graph_feats_sweep: agent_id %d outside [0, %d)", agent_id,
                cfg->n_agents);
  DGPPO_REQUIRE(nx >= 0 && ny >= 0 && n_frames >= 0, "dgppo_graph_feats_sweep: negative counts");
  if (nx == 0 || ny == 0 || n_frames == 0) return 0;
  DGPPO_REQUIRE(agent && goal && xs && ys && Xa && efeat && emask, "dgppo_graph_feats_sweep: NULL operand");
  DGPPO_REQUIRE(Fp >= cfg->node_dim && Fp <= 32, "dgppo_graph_feats_sweep: Fp must be in [node_dim, 32]");
  SweepArgs a;
  a.cfg = *cfg; a.t = make_topo(*cfg);
  const Topo& t = a.t;
  const int n_on = t.Ns - t.n - t.ng;
  DGPPO_REQUIRE(t.Ns == t.n || Xo, "dgppo_graph_feats_sweep: Xo is NULL");
  if (n_on > 0) {
    DGPPO_REQUIRE(obst, "dgppo_graph_feats_sweep: obst is NULL");
    if (t.lidar) DGPPO_REQUIRE(hits && ray_cos && ray_sin, "dgppo_graph_feats_sweep: hits / ray_cos / ray_sin is NULL");
  }
  DGPPO_REQUIRE(((uintptr_t)efeat & 15) == 0, "dgppo_graph_feats_sweep: efeat must be 16-byte aligned");
  DGPPO_REQUIRE(Fp >= 2 && t.S >= 2 && (long)t.Ns * Fp < 65536 && (long)t.n * t.S < 65536,
                "dgppo_graph_feats_sweep: sizes out of range");
  const long nxy = (long)nx * ny;
  DGPPO_REQUIRE(nxy <= (1L << 24), "dgppo_graph_feats_sweep: grid too large (nx * ny <= 2^24)");
  const long tiles = (nxy + SWEEP_TILE - 1) / SWEEP_TILE;
  DGPPO_REQUIRE(tiles * n_frames < (1L << 31), "dgppo_graph_feats_sweep: too many graphs");
  a.agent = agent; a.agent_st = agent_st; a.goal = goal; a.obst = obst; a.hits = hits; a.hits_st = hits_st;
  a.ray_cos = ray_cos; a.ray_sin = ray_sin; a.frame_ids = frame_ids; a.agent_id = agent_id; a.nx = nx; a.nxy = (int)nxy;
  a.tiles = (int)tiles; a.xs = xs; a.ys = ys; a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.hits_out = hits_out;
  a.Fp = Fp;
  auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
  a.rcp_fp = rcp(Fp); a.rcp_S = rcp(t.S);
  const int SD = cfg->state_dim, no = cfg->n_obs, R = cfg->n_rays, k = cfg->top_k;
  const bool cast = t.lidar && n_on > 0;
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  long fl = up4(t.lidar ? (cast ? no * 16 : 0) : (long)n_on * SD) + up4((long)t.n * SD) + up4((long)t.ng * SD) + t.n * 4 + t.ng * 4;
  if (cast) fl += no * 16 + up4((long)t.n * k * 2) + 2 * up4(R) + SWEEP_WAVES * (up4(R) + up4(k * 2));
  DGPPO_REQUIRE(fl * 4 <= 64 * 1024, "dgppo_graph_feats_sweep: the frame does not fit the LDS (%ld bytes)", fl * 4);
  const size_t smem = sizeof(float) * (size_t)fl;
  const dim3 grid((unsigned)(tiles * n_frames));
  if (SD == 5) hipLaunchKernelGGL(graph_feats_sweep_kernel<5>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(graph_feats_sweep_kernel<4>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- cost landscape ------------------------------------------------------------------------------------------------------------
// The environment's own cost h = get_cost (lidar_env/base.py:180-207, mpe/base.py:164-191, mpe_connect_spread.py:115-134) of
// ALL n agents in the graphs of the sweep above: what the learned Vh is supposed to bound, at the same swept positions.
//
// Per frame almost everything is invariant: every unmoved agent's nearest unmoved neighbour (with the 1e6 diagonal term) and its
// obstacle margin distance (recorded hits / discs).  A workgroup stages those once (s_md, s_mo); min is order independent and
// returns one of its operands, so "min over the staged part, then the moved agent's distance" has the oracle's bits.
// Phase 1 computes what depends on the point — the moved agent's nearest neighbour and obstacle distance (and the connectivity
// term) — into LDS, phase 2 streams the tile's n * n_cost words per point, one lane per word, unit stride over the whole tile.
// Phase 1 has two shapes: with a cast (LiDAR kinds with obstacles) a group of 32 lanes casts the R <= 32 rays of one point (two
// points per wave; 64 lanes when R > 32); without one (MPE, or no obstacles) a lane per point.
#define COST_NT 256
#define COST_WAVES (COST_NT / DGPPO_WAVE)
#define COST_TILE_CAST 64    // grid points per workgroup: 8 groups of 32 lanes walk 8 points a pass
#define COST_TILE_LANE 256   // a lane per point
#define COST_GROUPS (COST_NT / 32)

struct CostSweepArgs {
  dgppo_env_cfg cfg;
  const float* agent; long agent_st;
  const float* obst;
  const float* hits; long hits_st;
  const float* ray_cos;
  const float* ray_sin;
  const int32_t* frame_ids;
  int agent_id, nx, nxy, tiles;
  const float* xs;
  const float* ys;
  float* cost;
  float* hits_out;
  uint32_t rcp_W, rcp_nc;   // ceil(2^32 / d) for d = n * n_cost and n_cost (exact for idx < 2^16)
};

// sqrt(dx^2 + dy^2) as get_cost forms it, every operation correctly rounded: this file is built with -ffp-contract=off and
// sqrtf is the IEEE square root, as in env_step.hip.  (graph_topo.h's dist_rn goes through __fsqrt_rn, which the HIP headers
// map to the native, not correctly rounded, square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined: one ulp off the oracle
// in these outputs on the MI355X.  Elsewhere it only feeds mask comparisons.)
__device__ inline float dist_cost(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }
// NaN-propagating max (jnp.max semantics)
__device__ inline float nanmax(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }
// nanmin over the aligned group of `width` lanes (a power of two <= 64) this lane belongs to
__device__ inline float group_nanmin(float v, int width) {
  for (int off = width >> 1; off > 0; off >>= 1) v = nanmin(v, __shfl_xor(v, off));
  return v;
}

template <bool CAST>
__global__ void __launch_bounds__(COST_NT) cost_sweep_kernel(CostSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const dgppo_env_cfg& c = a.cfg;
  constexpr int TILE = CAST ? COST_TILE_CAST : COST_TILE_LANE;
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int fid = a.frame_ids ? a.frame_ids[f] : f;
  const int n = c.n_agents, SD = c.state_dim, aid = a.agent_id, nc = c.n_cost;
  const int no = c.n_obs, R = c.n_rays, k = c.top_k;
  const bool lidar = cfg_is_lidar(c);
  const float inf = __builtin_inff();
  // LDS carve: every offset is a multiple of 4 floats
  const int n4 = (n + 3) & ~3, Rp = (R + 3) & ~3, K2 = (k * 2 + 3) & ~3;
  float* s_x = sm;                 // n   positions of the frame
  float* s_y = s_x + n4;
  float* s_md = s_y + n4;          // n   nearest unmoved neighbour of every unmoved agent (1e6 diagonal included)
  float* s_mo = s_md + n4;         // n   nearest recorded hit / disc of every unmoved agent
  float* s_px = s_mo + n4;         // TILE  the tile's points and what phase 1 found for the moved agent there
  float* s_py = s_px + TILE;
  float* s_pmd = s_py + TILE;
  float* s_pmo = s_pmd + TILE;
  float* s_pw = s_pmo + TILE;      //       connectivity term (n_cost == 3)
  float* s_ob = s_pw + TILE;       // no*2 disc centres (MPE) | no*16 segment constants (cast)
  float* s_rec = s_ob + no * 16;   // cast only from here: no*16 rectangle records
  float* s_rc = s_rec + no * 16;   // R
  float* s_rs = s_rc + Rp;         // R
  float* s_al = s_rs + Rp;         // groups * R    alphas of the group's point
  float* s_hit = s_al + COST_GROUPS * Rp;   // groups * k*2  hits of the moved agent

  // ---- the frame, once per workgroup ----
  const float* ag = a.agent + (size_t)fid * a.agent_st;
  for (int i = tid; i < n; i += COST_NT) { s_x[i] = ag[i * SD]; s_y[i] = ag[i * SD + 1]; }
  if (CAST) {
    for (int i = tid; i < no * 16; i += COST_NT) s_rec[i] = a.obst[i];
    for (int i = tid; i < R; i += COST_NT) { s_rc[i] = a.ray_cos[i]; s_rs[i] = a.ray_sin[i]; }
  } else if (!lidar) {
    for (int i = tid; i < no; i += COST_NT) { s_ob[i * 2] = a.obst[i * SD]; s_ob[i * 2 + 1] = a.obst[i * SD + 1]; }
  }
  __syncthreads();
  if (CAST)
    for (int q = tid; q < no * 4; q += COST_NT) segment_consts(s_rec + (q >> 2) * DGPPO_RECT_STRIDE, q & 3, s_ob + q * 4);
  if (no > 0)
    for (int j = tid; j < n; j += COST_NT) {
      if (j == aid) continue;                        // the moved agent's own terms depend on the point: phase 1
      float mo;
      if (lidar) {
        const float* hp = a.hits + (size_t)fid * a.hits_st + (size_t)j * k * 2;
        mo = dist_cost(hp[0] - s_x[j], hp[1] - s_y[j]);
        for (int m = 1; m < k; ++m) mo = nanmin(mo, dist_cost(hp[m * 2] - s_x[j], hp[m * 2 + 1] - s_y[j]));
      } else {
        mo = dist_cost(s_x[j] - s_ob[0], s_y[j] - s_ob[1]);
        for (int m = 1; m < no; ++m) mo = nanmin(mo, dist_cost(s_x[j] - s_ob[m * 2], s_y[j] - s_ob[m * 2 + 1]));
      }
      s_mo[j] = mo;
    }
  for (int j = wave; j < n; j += COST_WAVES) {     // a wave per agent, a lane per neighbour
    if (j == aid) continue;
    float v = inf;
    for (int i = lane; i < n; i += DGPPO_WAVE)
      if (i != aid) {
        const float d = dist_cost(s_x[j] - s_x[i], s_y[j] - s_y[i]);
        v = nanmin(v, (i == j) ? d + 1e6f : d);
      }
    v = group_nanmin(v, DGPPO_WAVE);
    if (lane == 0) s_md[j] = v;
  }
  __syncthreads();

  const int q0 = tile * TILE, q1 = min(q0 + TILE, a.nxy);
  // ---- phase 1: the moved agent at every point of the tile ----
  if (CAST) {
    const float sr = c.comm_radius;
    const int LP = (R <= 32) ? 32 : DGPPO_WAVE, PW = DGPPO_WAVE / LP;      // lanes per point, points per wave
    const int sub = lane / LP, sl = lane - sub * LP;
    const uint64_t gmask = (LP == DGPPO_WAVE) ? ~0ull : (0xffffffffull << (32 * sub));
    float* w_al = s_al + (wave * PW + sub) * Rp;
    float* w_hit = s_hit + (wave * PW + sub) * K2;
    // w_al / w_hit belong to one group of one wave, whose LDS operations complete in issue order: wave-level fences suffice.
    // A group past the end of the tile repeats the last point (the wave stays convergent) and stores nothing
    for (int base = q0 + wave * PW; base < q1; base += COST_WAVES * PW) {
      const bool act = base + sub < q1;
      const int q = act ? base + sub : q1 - 1;
      const int iy = q / a.nx, ix = q - iy * a.nx;
      const float px = a.xs[ix], py = a.ys[iy];
      {
        // start inside a rectangle (env/utils.py:117, r = 0): all alphas become 0
        bool in = false;
        for (int o = sl; o < no; o += LP) in = in || rect_inside(s_rec + o * DGPPO_RECT_STRIDE, px, py, 0.0f);
        const float is_in = ((__ballot(in) & gmask) != 0ull) ? 1.0f : 0.0f;
        for (int r = sl; r < R; r += LP) w_al[r] = ray_min_alpha(px, py, s_rc[r], s_rs[r], sr, s_ob, no) * (1.0f - is_in);
      }
      wave_sync();
      for (int r = sl; r < R; r += LP) {
        const int rank = ray_rank(w_al, R, r);
        if (rank < k) ray_hit(px, py, s_rc[r], s_rs[r], sr, w_al[r], w_hit + rank * 2);
      }
      wave_sync();
      float mo = inf, md = inf;
      for (int m = sl; m < k; m += LP) mo = nanmin(mo, dist_cost(w_hit[m * 2] - px, w_hit[m * 2 + 1] - py));
      for (int j = sl; j < n; j += LP) {
        const float d = dist_cost(px - ((j == aid) ? px : s_x[j]), py - ((j == aid) ? py : s_y[j]));
        md = nanmin(md, (j == aid) ? d + 1e6f : d);
      }
      mo = group_nanmin(mo, LP);
      md = group_nanmin(md, LP);
      if (act) {
        if (sl == 0) { s_px[q - q0] = px; s_py[q - q0] = py; s_pmd[q - q0] = md; s_pmo[q - q0] = mo; }
        if (a.hits_out != nullptr) {
          float* ho = a.hits_out + ((size_t)f * a.nxy + q) * k * 2;
          for (int i = sl; i < k * 2; i += LP) ho[i] = w_hit[i];
        }
      }
      wave_sync();   // the next point's cast overwrites w_al / w_hit
    }
  } else {
    for (int q = q0 + tid; q < q1; q += COST_NT) {
      const int iy = q / a.nx, ix = q - iy * a.nx;
      const float px = a.xs[ix], py = a.ys[iy];
      float md = inf, w = -inf, mo = 0.0f;
      for (int j = 0; j < n; ++j) {
        const float d = dist_cost(px - ((j == aid) ? px : s_x[j]), py - ((j == aid) ? py : s_y[j]));
        md = nanmin(md, (j == aid) ? d + 1e6f : d);
        if (nc == 3 && j != aid) w = nanmax(w, nanmin(s_md[j], d) - c.connect_radius);
      }
      if (nc == 3) w = nanmax(w, md - c.connect_radius);
      if (!lidar && no > 0) {
        mo = dist_cost(px - s_ob[0], py - s_ob[1]);
        for (int m = 1; m < no; ++m) mo = nanmin(mo, dist_cost(px - s_ob[m * 2], py - s_ob[m * 2 + 1]));
      }
      s_px[q - q0] = px; s_py[q - q0] = py; s_pmd[q - q0] = md; s_pmo[q - q0] = mo; s_pw[q - q0] = w;
    }
  }
  __syncthreads();

  // ---- phase 2: the tile's words, a lane per word ----
  const int W = n * nc, words = (q1 - q0) * W;
  const bool clip_hi = lidar || c.kind == DGPPO_ENV_MPE_CONNECT_SPREAD;   // mpe/base.py:189 clips only from below
  const float r_obs = lidar ? c.car_radius : c.car_plus_obs;
  float* out = a.cost + ((size_t)f * a.nxy + q0) * W;
  for (int idx = tid; idx < words; idx += COST_NT) {
    const int p = sweep_div(idx, a.rcp_W), rem = idx - p * W;
    const int j = sweep_div(rem, a.rcp_nc), cc = rem - j * nc;
    float m;
    if (cc == 0) {
      const float md = (j == aid) ? s_pmd[p] : nanmin(s_md[j], dist_cost(s_px[p] - s_x[j], s_py[p] - s_y[j]));
      m = c.two_car_radius - md;
    } else if (cc == 1) {
      m = (no == 0) ? 0.0f : r_obs - ((j == aid) ? s_pmo[p] : s_mo[j]);
    } else {
      m = s_pw[p];
    }
    const float v = cost_value(m);
    out[idx] = clip_hi ? clampf_nan(v, -1.0f, 1.0f) : clip_lo_nan(v, -1.0f);
  }
}

extern "C" int32_t dgppo_cost_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* obst,
                                    const float* hits, int64_t hits_st, const float* ray_cos, const float* ray_sin,
                                    const int32_t* frame_ids, int32_t n_frames, int32_t agent_id, const float* xs, int32_t nx,
                                    const float* ys, int32_t ny, float* cost, float* hits_out, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_cost_sweep", "dgppo_vmas_step on a tiled record (there is no VMAS sweep)");
  DGPPO_REQUIRE(agent_id >= 0 && agent_id < cfg->n_agents, "dgppo_cost_sweep: agent_id %d outside [0, %d)", agent_id,
                cfg->n_agents);
  DGPPO_REQUIRE(nx >= 0 && ny >= 0 && n_frames >= 0, "dgppo_cost_sweep: negative counts");
  if (nx == 0 || ny == 0 || n_frames == 0) return 0;
  DGPPO_REQUIRE(agent && xs && ys && cost, "dgppo_cost_sweep: NULL operand");
  const int n = cfg->n_agents, no = cfg->n_obs, R = cfg->n_rays, k = cfg->top_k, nc = cfg->n_cost;
  const bool lidar = cfg_is_lidar(*cfg), cast = lidar && no > 0;
  if (no > 0) {
    DGPPO_REQUIRE(obst, "dgppo_cost_sweep: obst is NULL");
    if (lidar) DGPPO_REQUIRE(hits && ray_cos && ray_sin, "dgppo_cost_sweep: hits / ray_cos / ray_sin is NULL");
  }
  DGPPO_REQUIRE(nc >= 2 && !(cast && nc != 2), "dgppo_cost_sweep: n_cost must be 2 (3 for a kind without a cast)");
  const int tile = cast ? COST_TILE_CAST : COST_TILE_LANE;
  DGPPO_REQUIRE((long)tile * n * nc < 65536, "dgppo_cost_sweep: sizes out of range");
  const long nxy = (long)nx * ny;
  DGPPO_REQUIRE(nxy <= (1L << 24), "dgppo_cost_sweep: grid too large (nx * ny <= 2^24)");
  const long tiles = (nxy + tile - 1) / tile;
  // gridDim.x * blockDim.x has to stay below 2^32
  DGPPO_REQUIRE(tiles * n_frames * COST_NT < (1L << 32), "dgppo_cost_sweep: too many grid points (%ld workgroups of %d threads)",
                tiles * n_frames, COST_NT);
  CostSweepArgs a;
  a.cfg = *cfg;
  a.agent = agent; a.agent_st = agent_st; a.obst = obst; a.hits = hits; a.hits_st = hits_st; a.ray_cos = ray_cos;
  a.ray_sin = ray_sin; a.frame_ids = frame_ids; a.agent_id = agent_id; a.nx = nx; a.nxy = (int)nxy; a.tiles = (int)tiles;
  a.xs = xs; a.ys = ys; a.cost = cost; a.hits_out = cast ? hits_out : nullptr;
  auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
  a.rcp_W = rcp(n * nc); a.rcp_nc = rcp(nc);
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  long fl = 4 * up4(n) + 5 * tile + (long)no * 16;
  if (cast) fl += (long)no * 16 + 2 * up4(R) + COST_GROUPS * (up4(R) + up4(k * 2));
  DGPPO_REQUIRE(fl * 4 <= 64 * 1024, "dgppo_cost_sweep: the frame does not fit the LDS (%ld bytes)", fl * 4);
  const size_t smem = sizeof(float) * (size_t)fl;
  const dim3 grid((unsigned)(tiles * n_frames));
  if (cast) hipLaunchKernelGGL(cost_sweep_kernel<true>, grid, dim3(COST_NT), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(cost_sweep_kernel<false>, grid, dim3(COST_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- CBF action landscape -----------------------------------------------------------------------------------------------------
// The graph features behind the discrete barrier condition DGPPO's advantage is shaped by (dgppo/algo/dgppo.py:246-250):
// cbf_deriv[t] = (Vh(graph[t+1]) - Vh(graph[t])) / dt + alpha * Vh(graph[t]), with ONE agent's action at step t swept over a grid.
//
// Graph g = (f * nv + iv) * nu + iu is the graph of frame fid + 1 (fid = frame_ids[f]) in which row `agent_id` is
// agent_step_euler(row agent_id of frame fid, clip_action((us[iu], vs[iv]))) — step_state of env_step.h, the device code of the
// step kernels, y_limit included; every other agent keeps its recorded next state, i.e. its recorded action.
//
// What changes with the action: in both dynamics the next POSITION does not depend on it (double integrator x + v dt, bicycle
// x + v cos(theta) dt), so the LiDAR hits of frame fid + 1, every mask and every Xo row are the recorded ones and NO RAY IS CAST.
// The velocity columns change (bicycle: cos(theta'), sin(theta'), v') and, through state2feat, every edge feature that touches
// the agent.  The position is still taken from step_state's output: in a record the step kernels wrote, its bits are the record's.
//
// Organisation: the sweep above without its cast.  A workgroup stages frame fid + 1 (states, goals, discs, recorded hits) and
// row agent_id of frame fid in LDS once per tile of 64 grid points and walks the tile, one wave per point: lane 0 steps the row
// into the wave's LDS slot, then the wave streams the four dense outputs with unit-stride stores (edge features as float4).
// The outputs have the layout and arithmetic of dgppo_graph_feats (graph_feats.hip) for G = n_frames * nv * nu graphs.
#define ACT_TILE 64   // grid points per workgroup

struct ActionSweepArgs {
  dgppo_env_cfg cfg;
  Topo t;
  const float* agent; long agent_st;
  const float* goal;
  const float* obst;
  const float* hits; long hits_st;
  const int32_t* frame_ids;
  int agent_id, nu, nuv, tiles;
  const float* us;
  const float* vs;
  float* Xa;
  float* Xo;
  float* efeat;
  float* emask;
  int Fp;
  uint32_t rcp_fp, rcp_S;   // ceil(2^32 / d): index divisions by Fp and S as one v_mul_hi_u32 (exact for idx < 2^16)
};

template <int SD>
__global__ void __launch_bounds__(SWEEP_NT) graph_feats_action_sweep_kernel(ActionSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const Topo& t = a.t;
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int fid = a.frame_ids ? a.frame_ids[f] : f;
  const int n = t.n, ng = t.ng, S = t.S, Fp = a.Fp, aid = a.agent_id;
  const int n_on = t.Ns - n - ng;
  const int k = c.top_k;
  const bool rec_hits = t.lidar && n_on > 0;
  // LDS carve: every offset is a multiple of 4 floats
  const int al4 = 3;
  float* s_rec = sm;                                                   // n_obs*SD discs (MPE)
  float* s_ag = s_rec + ((t.lidar ? 0 : (n_on * SD + al4) & ~al4));    // n*SD   frame fid + 1
  float* s_go = s_ag + ((n * SD + al4) & ~al4);                        // ng*SD
  float* s_fa = s_go + ((ng * SD + al4) & ~al4);                       // n*4    state2feat(agent) of frame fid + 1
  float* s_fg = s_fa + n * 4;                                          // ng*4
  float* s_hp = s_fg + ng * 4;                                         // n*k*2  recorded hits of frame fid + 1 (LiDAR)
  float* s_x0 = s_hp + (rec_hits ? ((n * k * 2 + al4) & ~al4) : 0);    // 8      row agent_id of frame fid
  float* s_w = s_x0 + 8;                                               // waves * 12: the stepped row (8) and its features (4)

  // ---- frame fid + 1 and the row to step, once per workgroup ----
  const float* ag = a.agent + (size_t)(fid + 1) * a.agent_st;
  for (int i = tid; i < n * SD; i += SWEEP_NT) s_ag[i] = ag[i];
  for (int i = tid; i < ng * SD; i += SWEEP_NT) s_go[i] = a.goal[i];
  if (rec_hits) {
    const float* hp = a.hits + (size_t)(fid + 1) * a.hits_st;
    for (int i = tid; i < n * k * 2; i += SWEEP_NT) s_hp[i] = hp[i];
  } else if (!t.lidar) {
    for (int i = tid; i < n_on * SD; i += SWEEP_NT) s_rec[i] = a.obst[i];
  }
  if (tid < SD) s_x0[tid] = a.agent[(size_t)fid * a.agent_st + aid * SD + tid];
  __syncthreads();
  for (int i = tid; i < n + ng; i += SWEEP_NT)
    state2feat<SD>((i < n) ? s_ag + i * SD : s_go + (i - n) * SD, (i < n) ? s_fa + i * 4 : s_fg + (i - n) * 4);
  __syncthreads();

  const int q0 = tile * ACT_TILE, q1 = min(q0 + ACT_TILE, a.nuv);
  float* w_st = s_w + wave * 12;
  float* w_f = w_st + 8;
  constexpr int ND = SD + 3;
  // from here on the waves are independent: w_st / w_f belong to one wave, whose LDS operations complete in issue order,
  // so between its phases a wave-level fence (no reordering by the compiler, no workgroup barrier) is enough
  for (int q = q0 + wave; q < q1; q += SWEEP_WAVES) {
    const int iv = q / a.nu, iu = q - iv * a.nu;
    if (lane == 0) {
      const float u0 = clip_action(a.us[iu]), u1 = clip_action(a.vs[iv]);   // clip_action, env/base.py:84-86
      step_state<SD>(s_x0, u0, u1, c, c.y_limit, w_st);
      state2feat<SD>(w_st, w_f);
    }
    wave_sync();
    const size_t g = (size_t)f * a.nuv + q;
    // state and feature row of agent i in this graph
    auto st = [&](int i) { return (i == aid) ? w_st : s_ag + i * SD; };
    auto ft = [&](int i) { return (i == aid) ? w_f : s_fa + i * 4; };

    // node feature rows: [state | obs, goal, agent indicator], zero padded to Fp
    float* xa = a.Xa + g * n * Fp;
    for (int idx = lane; idx < n * Fp; idx += DGPPO_WAVE) {
      const int nd = sweep_div(idx, a.rcp_fp), col = idx - nd * Fp;
      float v = (col < SD) ? st(nd)[col] : ((col == SD + 2) ? 1.0f : 0.0f);
      if (col >= ND) v = 0.0f;
      xa[idx] = v;
    }
    float* xo = a.Xo + g * (t.Ns - n) * Fp;
    for (int idx = lane; idx < (t.Ns - n) * Fp; idx += DGPPO_WAVE) {
      const int r = sweep_div(idx, a.rcp_fp), col = idx - r * Fp;
      float v;
      if (r < ng) v = (col < SD) ? s_go[r * SD + col] : ((col == SD + 1) ? 1.0f : 0.0f);
      else {
        const int qn = r - ng;
        if (t.lidar) v = (col < 2) ? s_hp[qn * 2 + col] : ((col == SD) ? 1.0f : 0.0f);
        else v = (col < SD) ? s_rec[qn * SD + col] : ((col == SD) ? 1.0f : 0.0f);
      }
      if (col >= ND) v = 0.0f;
      xo[idx] = v;
    }
    // per-slot edge feature + mask (lidar_env/base.py:227-271, lidar_spread.py:57-96 and the MPE twins)
    float4* ef = reinterpret_cast<float4*>(a.efeat) + g * n * S;
    float* em = a.emask + g * n * S;
    for (int idx = lane; idx < n * S; idx += DGPPO_WAVE) {
      const int i = sweep_div(idx, a.rcp_S), s = idx - i * S;
      float4 fe;
      bool mask;
      const float* xi = st(i);
      const float* fi = ft(i);
      if (s < n) {
        const float* xs_ = st(s);
        const float* fs = ft(s);
        fe = make_float4(fi[0] - fs[0], fi[1] - fs[1], fi[2] - fs[2], fi[3] - fs[3]);
        const float d = dist_rn(xi[0] - xs_[0], xi[1] - xs_[1]) + ((i == s) ? c.eye_offset : 0.0f);
        mask = d < c.comm_radius;
      } else if (s < n + t.gs) {
        const float* fg = s_fg + (t.spread ? (s - n) : i) * 4;
        fe = make_float4(fi[0] - fg[0], fi[1] - fg[1], fi[2] - fg[2], fi[3] - fg[3]);
        mask = true;
      } else {
        const int m = s - n - t.gs;
        if (t.lidar) {
          const float* hp = s_hp + (i * k + m) * 2;
          const float lx = xi[0] - hp[0], ly = xi[1] - hp[1];
          fe = make_float4(lx, ly, 0.0f, 0.0f);
          mask = dist_rn(lx, ly) < c.lidar_mask_radius;
        } else {
          const float* xob = s_rec + m * SD;
          const float dx = xi[0] - xob[0], dy = xi[1] - xob[1];
          fe = make_float4(dx, dy, xi[2] - xob[2], xi[3] - xob[3]);
          mask = dist_rn(dx, dy) < c.obs_mask_radius;
        }
      }
      ef[idx] = fe;
      em[idx] = mask ? 1.0f : 0.0f;
    }
    wave_sync();   // the next point's step overwrites w_st / w_f
  }
}

extern "C" int32_t dgppo_graph_feats_action_sweep(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st,
                                                  const float* goal, const float* obst, const float* hits, int64_t hits_st,
                                                  const int32_t* frame_ids, int32_t n_frames, int32_t agent_id, const float* us,
                                                  int32_t nu, const float* vs, int32_t nv, float* Xa, float* Xo, float* efeat,
                                                  float* emask, int32_t Fp, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, "dgppo_graph_feats_action_sweep",
                    "dgppo_vmas_step and dgppo_vmas_graph_feats on a tiled record (there is no VMAS sweep)");
  DGPPO_REQUIRE(agent_id >= 0 && agent_id < cfg->n_agents, "dgppo_graph_feats_action_sweep: agent_id %d outside [0, %d)",
                agent_id, cfg->n_agents);
  DGPPO_REQUIRE(nu >= 0 && nv >= 0 && n_frames >= 0, "dgppo_graph_feats_action_sweep: negative counts");
  if (nu == 0 || nv == 0 || n_frames == 0) return 0;
  DGPPO_REQUIRE(agent && goal && us && vs && Xa && efeat && emask, "dgppo_graph_feats_action_sweep: NULL operand");
  DGPPO_REQUIRE(Fp >= cfg->node_dim && Fp <= 32, "dgppo_graph_feats_action_sweep: Fp must be in [node_dim, 32]");
  ActionSweepArgs a;
  a.cfg = *cfg; a.t = make_topo(*cfg);
  const Topo& t = a.t;
  const int n_on = t.Ns - t.n - t.ng;
  DGPPO_REQUIRE(t.Ns == t.n || Xo, "dgppo_graph_feats_action_sweep: Xo is NULL");
  if (n_on > 0) {
    if (t.lidar) DGPPO_REQUIRE(hits, "dgppo_graph_feats_action_sweep: hits is NULL");
    else DGPPO_REQUIRE(obst, "dgppo_graph_feats_action_sweep: obst is NULL");
  }
  DGPPO_REQUIRE(((uintptr_t)efeat & 15) == 0, "dgppo_graph_feats_action_sweep: efeat must be 16-byte aligned");
  DGPPO_REQUIRE(Fp >= 2 && t.S >= 2 && (long)t.Ns * Fp < 65536 && (long)t.n * t.S < 65536,
                "dgppo_graph_feats_action_sweep: sizes out of range");
  const long nuv = (long)nu * nv;
  DGPPO_REQUIRE(nuv <= (1L << 24), "dgppo_graph_feats_action_sweep: grid too large (nu * nv <= 2^24)");
  const long tiles = (nuv + ACT_TILE - 1) / ACT_TILE;
  DGPPO_REQUIRE(tiles * n_frames < (1L << 31), "dgppo_graph_feats_action_sweep: too many graphs");
  a.agent = agent; a.agent_st = agent_st; a.goal = goal; a.obst = obst; a.hits = hits; a.hits_st = hits_st;
  a.frame_ids = frame_ids; a.agent_id = agent_id; a.nu = nu; a.nuv = (int)nuv; a.tiles = (int)tiles; a.us = us; a.vs = vs;
  a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.Fp = Fp;
  auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
  a.rcp_fp = rcp(Fp); a.rcp_S = rcp(t.S);
  const int SD = cfg->state_dim, k = cfg->top_k;
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  long fl = (t.lidar ? 0 : up4((long)n_on * SD)) + up4((long)t.n * SD) + up4((long)t.ng * SD) + t.n * 4 + t.ng * 4 + 8 +
            SWEEP_WAVES * 12;
  if (t.lidar && n_on > 0) fl += up4((long)t.n * k * 2);
  DGPPO_REQUIRE(fl * 4 <= 64 * 1024, "dgppo_graph_feats_action_sweep: the frame does not fit the LDS (%ld bytes)", fl * 4);
  const size_t smem = sizeof(float) * (size_t)fl;
  const dim3 grid((unsigned)(tiles * n_frames));
  if (SD == 5) hipLaunchKernelGGL(graph_feats_action_sweep_kernel<5>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(graph_feats_action_sweep_kernel<4>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- barrier shield: every agent's action swept at once ------------------------------------------------------------------------
// The what-if graphs of one shielded step (Engine.rollout_shielded): for env e, agent i and candidate p, graph
// g = (e * n + i) * P + p, P = 1 + nv * nu, is the graph of next_agent[e] — the state after the provisional step with the
// policy's own actions — in which row i is agent_step_euler(row i of agent[e], clip_action(candidate p)) and every other agent
// keeps its provisional next state.  Candidate 0 is the agent's own policy action a_pol[e, i], candidate 1 + iv * nu + iu is
// (us[iu], vs[iv]).  This is dgppo_graph_feats_action_sweep's graph with the same arithmetic (step_state of env_step.h, nothing
// is cast: the next position does not depend on the action, so next_hits are final), for all agents and environments in ONE
// launch instead of B * n.
//
// Organisation: the action sweep's.  A workgroup serves one (e, i, tile of 64 candidates): it stages next_agent[e], the goals,
// discs and next_hits of env e and row i of agent[e] in LDS once and walks the tile, one wave per candidate: lane 0 steps the
// row into the wave's LDS slot, then the wave streams the four dense outputs with unit-stride stores (edge features as float4).
struct TeamSweepArgs {
  dgppo_env_cfg cfg;
  Topo t;
  const float* agent;        // [B, n, SD]   state t
  const float* next_agent;   // [B, n, SD]   provisional state t + 1
  const float* goal;         // [B, ng, SD]
  const float* obst;         // [B, n_obs, SD] discs (MPE)
  const float* next_hits;    // [B, n, k, 2] (LiDAR with obstacles)
  const float* a_pol;        // [B, n, 2]
  int nu, P, tiles;
  const float* us;
  const float* vs;
  float* Xa;
  float* Xo;
  float* efeat;
  float* emask;
  int Fp;
  uint32_t rcp_fp, rcp_S;   // ceil(2^32 / d): index divisions by Fp and S as one v_mul_hi_u32 (exact for idx < 2^16)
};

template <int SD>
__global__ void __launch_bounds__(SWEEP_NT) graph_feats_team_action_sweep_kernel(TeamSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const Topo& t = a.t;
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int ei = blockIdx.x / a.tiles, tile = blockIdx.x - ei * a.tiles;   // ei = e * n + i
  const int n = t.n, ng = t.ng, S = t.S, Fp = a.Fp;
  const int e = ei / n, aid = ei - e * n;
  const int n_on = t.Ns - n - ng;
  const int k = c.top_k;
  const bool rec_hits = t.lidar && n_on > 0;
  // LDS carve: every offset is a multiple of 4 floats
  const int al4 = 3;
  float* s_rec = sm;                                                   // n_obs*SD discs (MPE)
  float* s_ag = s_rec + ((t.lidar ? 0 : (n_on * SD + al4) & ~al4));    // n*SD   next_agent[e]
  float* s_go = s_ag + ((n * SD + al4) & ~al4);                        // ng*SD
  float* s_fa = s_go + ((ng * SD + al4) & ~al4);                       // n*4    state2feat(next_agent[e])
  float* s_fg = s_fa + n * 4;                                          // ng*4
  float* s_hp = s_fg + ng * 4;                                         // n*k*2  next_hits[e] (LiDAR)
  float* s_x0 = s_hp + (rec_hits ? ((n * k * 2 + al4) & ~al4) : 0);    // 8      row aid of agent[e]
  float* s_w = s_x0 + 8;                                               // waves * 12: the stepped row (8) and its features (4)

  // ---- the provisional next frame of env e and the row to step, once per workgroup ----
  const float* ag = a.next_agent + (size_t)e * n * SD;
  for (int i = tid; i < n * SD; i += SWEEP_NT) s_ag[i] = ag[i];
  const float* go = a.goal + (size_t)e * ng * SD;
  for (int i = tid; i < ng * SD; i += SWEEP_NT) s_go[i] = go[i];
  if (rec_hits) {
    const float* hp = a.next_hits + (size_t)e * n * k * 2;
    for (int i = tid; i < n * k * 2; i += SWEEP_NT) s_hp[i] = hp[i];
  } else if (!t.lidar) {
    const float* ob = a.obst + (size_t)e * n_on * SD;
    for (int i = tid; i < n_on * SD; i += SWEEP_NT) s_rec[i] = ob[i];
  }
  if (tid < SD) s_x0[tid] = a.agent[(size_t)ei * SD + tid];
  __syncthreads();
  for (int i = tid; i < n + ng; i += SWEEP_NT)
    state2feat<SD>((i < n) ? s_ag + i * SD : s_go + (i - n) * SD, (i < n) ? s_fa + i * 4 : s_fg + (i - n) * 4);
  __syncthreads();

  const int q0 = tile * ACT_TILE, q1 = min(q0 + ACT_TILE, a.P);
  float* w_st = s_w + wave * 12;
  float* w_f = w_st + 8;
  constexpr int ND = SD + 3;
  // from here on the waves are independent: w_st / w_f belong to one wave, whose LDS operations complete in issue order,
  // so between its phases a wave-level fence (no reordering by the compiler, no workgroup barrier) is enough
  for (int q = q0 + wave; q < q1; q += SWEEP_WAVES) {
    if (lane == 0) {
      float u0, u1;
      if (q == 0) {
        u0 = a.a_pol[(size_t)ei * 2]; u1 = a.a_pol[(size_t)ei * 2 + 1];
      } else {
        const int iv = (q - 1) / a.nu, iu = (q - 1) - iv * a.nu;
        u0 = a.us[iu]; u1 = a.vs[iv];
      }
      step_state<SD>(s_x0, clip_action(u0), clip_action(u1), c, c.y_limit, w_st);   // clip_action, env/base.py:84-86
      state2feat<SD>(w_st, w_f);
    }
    wave_sync();
    const size_t g = (size_t)ei * a.P + q;
    // state and feature row of agent i in this graph
    auto st = [&](int i) { return (i == aid) ? w_st : s_ag + i * SD; };
    auto ft = [&](int i) { return (i == aid) ? w_f : s_fa + i * 4; };

    // node feature rows: [state | obs, goal, agent indicator], zero padded to Fp
    float* xa = a.Xa + g * n * Fp;
    for (int idx = lane; idx < n * Fp; idx += DGPPO_WAVE) {
      const int nd = sweep_div(idx, a.rcp_fp), col = idx - nd * Fp;
      float v = (col < SD) ? st(nd)[col] : ((col == SD + 2) ? 1.0f : 0.0f);
      if (col >= ND) v = 0.0f;
      xa[idx] = v;
    }
    float* xo = a.Xo + g * (t.Ns - n) * Fp;
    for (int idx = lane; idx < (t.Ns - n) * Fp; idx += DGPPO_WAVE) {
      const int r = sweep_div(idx, a.rcp_fp), col = idx - r * Fp;
      float v;
      if (r < ng) v = (col < SD) ? s_go[r * SD + col] : ((col == SD + 1) ? 1.0f : 0.0f);
      else {
        const int qn = r - ng;
        if (t.lidar) v = (col < 2) ? s_hp[qn * 2 + col] : ((col == SD) ? 1.0f : 0.0f);
        else v = (col < SD) ? s_rec[qn * SD + col] : ((col == SD) ? 1.0f : 0.0f);
      }
      if (col >= ND) v = 0.0f;
      xo[idx] = v;
    }
    // per-slot edge feature + mask (lidar_env/base.py:227-271, lidar_spread.py:57-96 and the MPE twins)
    float4* ef = reinterpret_cast<float4*>(a.efeat) + g * n * S;
    float* em = a.emask + g * n * S;
    for (int idx = lane; idx < n * S; idx += DGPPO_WAVE) {
      const int i = sweep_div(idx, a.rcp_S), s = idx - i * S;
      float4 fe;
      bool mask;
      const float* xi = st(i);
      const float* fi = ft(i);
      if (s < n) {
        const float* xs_ = st(s);
        const float* fs = ft(s);
        fe = make_float4(fi[0] - fs[0], fi[1] - fs[1], fi[2] - fs[2], fi[3] - fs[3]);
        const float d = dist_rn(xi[0] - xs_[0], xi[1] - xs_[1]) + ((i == s) ? c.eye_offset : 0.0f);
        mask = d < c.comm_radius;
      } else if (s < n + t.gs) {
        const float* fg = s_fg + (t.spread ? (s - n) : i) * 4;
        fe = make_float4(fi[0] - fg[0], fi[1] - fg[1], fi[2] - fg[2], fi[3] - fg[3]);
        mask = true;
      } else {
        const int m = s - n - t.gs;
        if (t.lidar) {
          const float* hp = s_hp + (i * k + m) * 2;
          const float lx = xi[0] - hp[0], ly = xi[1] - hp[1];
          fe = make_float4(lx, ly, 0.0f, 0.0f);
          mask = dist_rn(lx, ly) < c.lidar_mask_radius;
        } else {
          const float* xob = s_rec + m * SD;
          const float dx = xi[0] - xob[0], dy = xi[1] - xob[1];
          fe = make_float4(dx, dy, xi[2] - xob[2], xi[3] - xob[3]);
          mask = dist_rn(dx, dy) < c.obs_mask_radius;
        }
      }
      ef[idx] = fe;
      em[idx] = mask ? 1.0f : 0.0f;
    }
    wave_sync();   // the next candidate's step overwrites w_st / w_f
  }
}

extern "C" int32_t dgppo_graph_feats_team_action_sweep(const dgppo_env_cfg* cfg, const float* agent, const float* next_agent,
                                                       const float* goal, const float* obst, const float* next_hits,
                                                       const float* a_pol, int32_t n_env, const float* us, int32_t nu,
                                                       const float* vs, int32_t nv, float* Xa, float* Xo, float* efeat,
                                                       float* emask, int32_t Fp, void* stream) {
  const char* fn = "dgppo_graph_feats_team_action_sweep";
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, fn, "dgppo_vmas_step and dgppo_vmas_graph_feats on a tiled record (there is no VMAS sweep)");
  DGPPO_REQUIRE(nu >= 1 && nv >= 1 && n_env >= 0, "%s: nu and nv must be >= 1 and n_env >= 0 (got %d, %d, %d)", fn, nu, nv, n_env);
  if (n_env == 0) return 0;
  DGPPO_REQUIRE(agent && next_agent && goal && a_pol && us && vs && Xa && efeat && emask, "%s: NULL operand", fn);
  DGPPO_REQUIRE(Fp >= cfg->node_dim && Fp <= 32, "%s: Fp must be in [node_dim, 32]", fn);
  TeamSweepArgs a;
  a.cfg = *cfg; a.t = make_topo(*cfg);
  const Topo& t = a.t;
  const int n_on = t.Ns - t.n - t.ng;
  DGPPO_REQUIRE(t.Ns == t.n || Xo, "%s: Xo is NULL", fn);
  if (n_on > 0) {
    if (t.lidar) DGPPO_REQUIRE(next_hits, "%s: next_hits is NULL", fn);
    else DGPPO_REQUIRE(obst, "%s: obst is NULL", fn);
  }
  DGPPO_REQUIRE(((uintptr_t)efeat & 15) == 0, "%s: efeat must be 16-byte aligned", fn);
  DGPPO_REQUIRE(Fp >= 2 && t.S >= 2 && (long)t.Ns * Fp < 65536 && (long)t.n * t.S < 65536, "%s: sizes out of range", fn);
  const long nuv = (long)nu * nv;
  DGPPO_REQUIRE(nuv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  const long P = 1 + nuv;
  const long tiles = (P + ACT_TILE - 1) / ACT_TILE;
  DGPPO_REQUIRE(tiles * n_env * t.n < (1L << 31), "%s: too many graphs", fn);
  a.agent = agent; a.next_agent = next_agent; a.goal = goal; a.obst = obst; a.next_hits = next_hits; a.a_pol = a_pol;
  a.nu = nu; a.P = (int)P; a.tiles = (int)tiles; a.us = us; a.vs = vs;
  a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.Fp = Fp;
  auto rcp = [](int d) { return (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d); };
  a.rcp_fp = rcp(Fp); a.rcp_S = rcp(t.S);
  const int SD = cfg->state_dim, k = cfg->top_k;
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  long fl = (t.lidar ? 0 : up4((long)n_on * SD)) + up4((long)t.n * SD) + up4((long)t.ng * SD) + t.n * 4 + t.ng * 4 + 8 +
            SWEEP_WAVES * 12;
  if (t.lidar && n_on > 0) fl += up4((long)t.n * k * 2);
  DGPPO_REQUIRE(fl * 4 <= 64 * 1024, "%s: the frame does not fit the LDS (%ld bytes)", fn, fl * 4);
  const size_t smem = sizeof(float) * (size_t)fl;
  const dim3 grid((unsigned)(tiles * n_env * t.n));
  if (SD == 5) hipLaunchKernelGGL(graph_feats_team_action_sweep_kernel<5>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(graph_feats_team_action_sweep_kernel<4>, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- barrier shield: selection -------------------------------------------------------------------------------------------------
// Per (env e, agent i), over the P = 1 + nv * nu candidates of the sweep above, on the agent's OWN row (the filter is
// decentralised):  h[p] = max_c ((Vh_next[e, i, p, i, c] - Vh_t[e, i, c]) / dt + alpha * Vh_t[e, i, c])  — the discrete barrier
// condition of dgppo/algo/dgppo.py:246-250, NaN-propagating max, fp32 without contraction.  A candidate is admissible iff
// h <= -margin (a NaN never is).  Candidate 0 (the policy's action) is kept if admissible (flag 0); otherwise the admissible
// candidate nearest to it, du * du + dv * dv on clipped actions, lowest index on ties (a NaN distance counts as +inf) (flag 1);
// with nothing admissible the candidate with the smallest h, lowest index on ties, NaN skipped, candidate 0 if every h is NaN
// (flag 2).  One wave per (e, i), lanes over the candidates, two (value, index) minima reduced with __shfl_xor.
#define SHIELD_NT 256
#define SHIELD_WAVES (SHIELD_NT / DGPPO_WAVE)

struct ShieldArgs {
  const float* Vh_next;   // [E, n, P, n, nh]
  const float* Vh_t;      // [E, n, nh]
  const float* a_pol;     // [E, n, 2]
  const float* us;
  const float* vs;
  int rows, n, nh, nu, P;
  float dt, alpha, margin;
  float* action;          // [E, n, 2]
  int32_t* index;         // [E, n]
  int32_t* flag;          // [E, n]
  float* h;               // [E, n, P] or NULL
};

// lexicographic (value, index) minimum over the wave
__device__ inline void wave_argmin(float& v, int& i) {
  for (int off = DGPPO_WAVE >> 1; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// The choice among an agent's P candidates, shared by the barrier shield and the lookahead shield: a lane feeds its candidates'
// values to pick_consider and the wave settles in pick_finish.  Candidate 0 is the policy's action (a0, a1), already clipped.
struct ShieldPick {
  float bd, bh, h0;       // nearest admissible distance, smallest value, candidate 0's value
  int bdi, bhi;
};

__device__ inline ShieldPick pick_init() {
  ShieldPick k;
  k.bd = __builtin_inff(); k.bh = __builtin_inff(); k.h0 = 0.0f; k.bdi = 0x7fffffff; k.bhi = 0x7fffffff;
  return k;
}

__device__ inline void pick_candidate(int p, float a0, float a1, const float* us, const float* vs, int nu, float& cu, float& cv) {
  cu = a0; cv = a1;
  if (p > 0) {
    const int iv = (p - 1) / nu, iu = (p - 1) - iv * nu;
    cu = clip_action(us[iu]); cv = clip_action(vs[iv]);
  }
}

// (r0, r1): the action the distance is measured from — candidate 0 itself for the one-shot shields, the policy's action where
// candidate 0 is an action held from an earlier round (dgppo_lookahead_reselect)
__device__ inline void pick_consider(ShieldPick& k, float h, int p, float a0, float a1, float r0, float r1, float thr,
                                     const float* us, const float* vs, int nu) {
  if (p == 0) k.h0 = h;
  float cu, cv;
  pick_candidate(p, a0, a1, us, vs, nu, cu, cv);
  if (h <= thr) {                               // admissible (false for a NaN)
    const float du = cu - r0, dv = cv - r1;
    float d = du * du + dv * dv;
    if (d != d) d = __builtin_inff();
    if (d < k.bd || (d == k.bd && p < k.bdi)) { k.bd = d; k.bdi = p; }
  }
  if (h == h && (h < k.bh || (h == k.bh && p < k.bhi))) { k.bh = h; k.bhi = p; }
}

__device__ inline void pick_consider(ShieldPick& k, float h, int p, float a0, float a1, float thr, const float* us,
                                     const float* vs, int nu) {
  pick_consider(k, h, p, a0, a1, a0, a1, thr, us, vs, nu);
}

// every lane of the wave calls it and every lane gets the row's choice: the candidate and its flag (0 kept, 1 admissible, 2 not)
__device__ inline void pick_settle(ShieldPick& k, float thr, int& idx, int& fl) {
  const float h0 = __shfl(k.h0, 0);
  wave_argmin(k.bd, k.bdi);
  wave_argmin(k.bh, k.bhi);
  if (h0 <= thr) { idx = 0; fl = 0; }
  else if (k.bdi != 0x7fffffff) { idx = k.bdi; fl = 1; }
  else { idx = (k.bhi != 0x7fffffff) ? k.bhi : 0; fl = 2; }
}

// every lane of the wave calls it; lane 0 writes the row's choice
__device__ inline void pick_finish(ShieldPick& k, int lane, long row, float a0, float a1, float thr, const float* us,
                                   const float* vs, int nu, float* action, int32_t* index, int32_t* flag) {
  int idx, fl;
  pick_settle(k, thr, idx, fl);
  if (lane != 0) return;
  float cu, cv;
  pick_candidate(idx, a0, a1, us, vs, nu, cu, cv);
  action[row * 2] = cu; action[row * 2 + 1] = cv;
  index[row] = idx; flag[row] = fl;
}

__global__ void __launch_bounds__(SHIELD_NT) shield_select_kernel(ShieldArgs a) {
  const int lane = threadIdx.x & (DGPPO_WAVE - 1);
  const long row = (long)blockIdx.x * SHIELD_WAVES + threadIdx.x / DGPPO_WAVE;   // row = e * n + i
  if (row >= a.rows) return;                      // whole waves leave: no lane of a live wave is missing from the shuffles
  const int i = (int)(row % a.n), nh = a.nh, P = a.P;
  const float* vt = a.Vh_t + row * nh;
  const float* vn = a.Vh_next + ((size_t)row * P * a.n + i) * nh;
  const size_t vn_st = (size_t)a.n * nh;
  const float a0 = clip_action(a.a_pol[row * 2]), a1 = clip_action(a.a_pol[row * 2 + 1]);
  const float thr = -a.margin;
  ShieldPick k = pick_init();
  for (int p = lane; p < P; p += DGPPO_WAVE) {
    float h = 0.0f;
    for (int cc = 0; cc < nh; ++cc) {
      const float v = vt[cc];
      const float hc = (vn[p * vn_st + cc] - v) / a.dt + a.alpha * v;
      h = (cc == 0) ? hc : nanmax(h, hc);
    }
    if (a.h != nullptr) a.h[(size_t)row * P + p] = h;
    pick_consider(k, h, p, a0, a1, thr, a.us, a.vs, a.nu);
  }
  pick_finish(k, lane, row, a0, a1, thr, a.us, a.vs, a.nu, a.action, a.index, a.flag);
}

extern "C" int32_t dgppo_shield_select(const float* Vh_next, const float* Vh_t, const float* a_pol, int32_t n_env,
                                       int32_t n_agents, int32_t n_cost, const float* us, int32_t nu, const float* vs, int32_t nv,
                                       float dt, float alpha, float margin, float* action, int32_t* index, int32_t* flag,
                                       float* h, void* stream) {
  const char* fn = "dgppo_shield_select";
  DGPPO_REQUIRE(n_env >= 0 && n_agents >= 1 && n_cost >= 1, "%s: n_env >= 0, n_agents >= 1 and n_cost >= 1 are required", fn);
  DGPPO_REQUIRE(nu >= 1 && nv >= 1, "%s: nu and nv must be >= 1 (got %d, %d)", fn, nu, nv);
  DGPPO_REQUIRE((long)nu * nv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  DGPPO_REQUIRE(dt > 0.0f && alpha == alpha && margin == margin, "%s: dt must be > 0, alpha and margin no NaN", fn);
  if (n_env == 0) return 0;
  DGPPO_REQUIRE(Vh_next && Vh_t && a_pol && us && vs && action && index && flag, "%s: NULL operand", fn);
  const long rows = (long)n_env * n_agents;
  DGPPO_REQUIRE(rows < (1L << 31) - SHIELD_WAVES, "%s: too many rows", fn);
  ShieldArgs a;
  a.Vh_next = Vh_next; a.Vh_t = Vh_t; a.a_pol = a_pol; a.us = us; a.vs = vs;
  a.rows = (int)rows; a.n = n_agents; a.nh = n_cost; a.nu = nu; a.P = 1 + nu * nv;
  a.dt = dt; a.alpha = alpha; a.margin = margin; a.action = action; a.index = index; a.flag = flag; a.h = h;
  const dim3 grid((unsigned)((rows + SHIELD_WAVES - 1) / SHIELD_WAVES));
  hipLaunchKernelGGL(shield_select_kernel, grid, dim3(SHIELD_NT), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- rollout landscape: the what-if environments of a sweep as a dense env state ---------------------------------------------
// Vh is fitted to Qh, the discounted-to-max constraint return of the policy's own future (compute_dec_ocp_gae,
// dgppo/algo/utils.py:38-45), so its ground truth at a swept position is a policy rollout FROM that position.  The fork below
// builds the start of those rollouts: env g = (f * ny + iy) * nx + ix is frame fid = frame_ids[f] with agent `agent_id` standing
// at (xs[ix], ys[iy]) — the graph of dgppo_graph_feats_sweep above, written as the state the step kernels run on (agent rows,
// goals, obstacle records, hit points, the actor's carry) instead of as its features.
//
// Organisation: the sweep's.  A workgroup stages the frame (states, goals, obstacle records, recorded hits) in LDS once per tile
// of 64 grid points and walks the tile, one wave per point: the wave casts the R rays of the moved agent and ranks them
// (env_step.h's ray arithmetic, as above), then streams the env's rows with unit-stride stores.  Consecutive points are
// consecutive envs, so the four waves of a pass write one contiguous range of each output.  The carry rows are a plain copy
// per point and go from global memory to global memory (n * HC floats that stay in L2 across a frame's tiles): the LDS
// budget does not depend on HC.
struct ForkArgs {
  dgppo_env_cfg cfg;
  const float* agent; long agent_st;
  const float* goal;
  const float* obst;
  const float* hits; long hits_st;
  const float* ray_cos;
  const float* ray_sin;
  const int32_t* frame_ids;
  int agent_id, nx, nxy, tiles;
  const float* xs;
  const float* ys;
  const float* carry; long carry_st;
  int HC;
  float* agent_out;
  float* goal_out;
  float* obst_out;
  float* hits_out;
  float* carry_out;
};

__global__ void __launch_bounds__(SWEEP_NT) env_sweep_fork_kernel(ForkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const dgppo_env_cfg& c = a.cfg;
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int fid = a.frame_ids ? a.frame_ids[f] : f;
  const int n = c.n_agents, ng = c.n_goals, SD = c.state_dim, aid = a.agent_id;
  const int no = c.n_obs, R = c.n_rays, k = c.top_k;
  const bool lidar = cfg_is_lidar(c), cast = lidar && no > 0;
  const int OS = lidar ? DGPPO_RECT_STRIDE : SD;                 // floats per obstacle record
  // LDS carve: every offset is a multiple of 4 floats
  const int al4 = 3;
  const int Rp = (R + al4) & ~al4, K2 = (k * 2 + al4) & ~al4;
  float* s_seg = sm;                                             // no*16 segment constants (cast)
  float* s_rec = s_seg + (cast ? no * 16 : 0);                   // no*OS obstacle records
  float* s_ag = s_rec + ((no * OS + al4) & ~al4);                // n*SD
  float* s_go = s_ag + ((n * SD + al4) & ~al4);                  // ng*SD
  float* s_hp = s_go + ((ng * SD + al4) & ~al4);                 // n*k*2 recorded hits (cast)
  float* s_rc = s_hp + (cast ? ((n * k * 2 + al4) & ~al4) : 0);  // R
  float* s_rs = s_rc + (cast ? Rp : 0);                          // R
  float* s_al = s_rs + (cast ? Rp : 0);                          // waves * R    alphas of the wave's point
  float* s_hit = s_al + (cast ? SWEEP_WAVES * Rp : 0);           // waves * k*2  hits of the moved agent

  // ---- the frame, once per workgroup ----
  const float* ag = a.agent + (size_t)fid * a.agent_st;
  for (int i = tid; i < n * SD; i += SWEEP_NT) s_ag[i] = ag[i];
  for (int i = tid; i < ng * SD; i += SWEEP_NT) s_go[i] = a.goal[i];
  for (int i = tid; i < no * OS; i += SWEEP_NT) s_rec[i] = a.obst[i];
  if (cast) {
    const float* hp = a.hits + (size_t)fid * a.hits_st;
    for (int i = tid; i < n * k * 2; i += SWEEP_NT) s_hp[i] = hp[i];
    for (int i = tid; i < R; i += SWEEP_NT) { s_rc[i] = a.ray_cos[i]; s_rs[i] = a.ray_sin[i]; }
  }
  __syncthreads();
  if (cast)
    for (int q = tid; q < no * 4; q += SWEEP_NT) segment_consts(s_rec + (q >> 2) * DGPPO_RECT_STRIDE, q & 3, s_seg + q * 4);
  __syncthreads();

  const int q0 = tile * SWEEP_TILE, q1 = min(q0 + SWEEP_TILE, a.nxy);
  float* w_al = s_al + wave * Rp;
  float* w_hit = s_hit + wave * K2;
  const float sr = c.comm_radius;
  const int hit0 = aid * k * 2, hit1 = hit0 + k * 2;            // the moved agent's words of a hits row
  const float* cr = a.carry ? a.carry + (size_t)fid * a.carry_st : nullptr;
  // from here on the waves are independent: w_al / w_hit belong to one wave, whose LDS operations complete in issue order,
  // so between its phases a wave-level fence (no reordering by the compiler, no workgroup barrier) is enough
  for (int q = q0 + wave; q < q1; q += SWEEP_WAVES) {
    const int iy = q / a.nx, ix = q - iy * a.nx;
    const float px = a.xs[ix], py = a.ys[iy];
    if (cast) {
      {
        // start inside a rectangle (env/utils.py:117, r = 0): all alphas become 0
        bool in = false;
        for (int o = lane; o < no; o += DGPPO_WAVE) in = in || rect_inside(s_rec + o * DGPPO_RECT_STRIDE, px, py, 0.0f);
        const float is_in = (__ballot(in) != 0ull) ? 1.0f : 0.0f;
        for (int r = lane; r < R; r += DGPPO_WAVE)
          w_al[r] = ray_min_alpha(px, py, s_rc[r], s_rs[r], sr, s_seg, no) * (1.0f - is_in);
      }
      wave_sync();
      for (int r = lane; r < R; r += DGPPO_WAVE) {
        const int rank = ray_rank(w_al, R, r);
        if (rank < k) ray_hit(px, py, s_rc[r], s_rs[r], sr, w_al[r], w_hit + rank * 2);
      }
      wave_sync();
    }
    const size_t g = (size_t)f * a.nxy + q;
    // agent rows: frame fid's, columns 0 and 1 of row agent_id replaced; every other column (velocity; the bicycle's heading
    // and speed) kept
    float* ao = a.agent_out + g * n * SD;
    for (int i = lane; i < n * SD; i += DGPPO_WAVE) {
      float v = s_ag[i];
      if (i == aid * SD) v = px;
      if (i == aid * SD + 1) v = py;
      ao[i] = v;
    }
    // the step kernels index goals and obstacle records by env: every what-if env gets its own copy
    float* go = a.goal_out + g * ng * SD;
    for (int i = lane; i < ng * SD; i += DGPPO_WAVE) go[i] = s_go[i];
    if (no > 0) {
      float* oo = a.obst_out + g * no * OS;
      for (int i = lane; i < no * OS; i += DGPPO_WAVE) oo[i] = s_rec[i];
    }
    if (cast) {
      float* ho = a.hits_out + g * n * k * 2;
      for (int i = lane; i < n * k * 2; i += DGPPO_WAVE) ho[i] = (i >= hit0 && i < hit1) ? w_hit[i - hit0] : s_hp[i];
    }
    if (cr != nullptr) {
      float* co = a.carry_out + g * n * a.HC;
      for (int i = lane; i < n * a.HC; i += DGPPO_WAVE) co[i] = cr[i];
    }
    wave_sync();   // the next point's cast overwrites w_al / w_hit
  }
}

extern "C" int32_t dgppo_env_sweep_fork(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                        const float* obst, const float* hits, int64_t hits_st, const float* ray_cos,
                                        const float* ray_sin, const int32_t* frame_ids, int32_t n_frames, int32_t agent_id,
                                        const float* xs, int32_t nx, const float* ys, int32_t ny, const float* carry,
                                        int64_t carry_st, int32_t HC, float* agent_out, float* goal_out, float* obst_out,
                                        float* hits_out, float* carry_out, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {   // the configuration's own refusal, under this entry point's name
    const std::string why = dgppo_last_error();
    dgppo_set_error("dgppo_env_sweep_fork: %s", why.c_str());
    return rc;
  }
  DGPPO_REFUSE_VMAS(cfg, "dgppo_env_sweep_fork", "dgppo_vmas_step on a tiled record (there is no VMAS sweep)");
  DGPPO_REQUIRE(agent_id >= 0 && agent_id < cfg->n_agents, "dgppo_env_sweep_fork: agent_id %d outside [0, %d)", agent_id,
                cfg->n_agents);
  DGPPO_REQUIRE(nx >= 0 && ny >= 0 && n_frames >= 0, "dgppo_env_sweep_fork: negative counts");
  if (nx == 0 || ny == 0 || n_frames == 0) return 0;
  DGPPO_REQUIRE(agent && goal && xs && ys && agent_out && goal_out, "dgppo_env_sweep_fork: NULL operand");
  const int n = cfg->n_agents, ng = cfg->n_goals, SD = cfg->state_dim, no = cfg->n_obs, R = cfg->n_rays, k = cfg->top_k;
  const bool lidar = cfg_is_lidar(*cfg), cast = lidar && no > 0;
  if (no > 0) {
    DGPPO_REQUIRE(obst, "dgppo_env_sweep_fork: obst is NULL");
    DGPPO_REQUIRE(obst_out, "dgppo_env_sweep_fork: obst_out is NULL");
    if (cast) {
      DGPPO_REQUIRE(hits && ray_cos && ray_sin, "dgppo_env_sweep_fork: hits / ray_cos / ray_sin is NULL");
      DGPPO_REQUIRE(hits_out, "dgppo_env_sweep_fork: hits_out is NULL");
    }
  }
  if (carry != nullptr) {
    DGPPO_REQUIRE(carry_out, "dgppo_env_sweep_fork: carry_out is NULL");
    DGPPO_REQUIRE(HC >= 1 && (long)n * HC < (1L << 31), "dgppo_env_sweep_fork: HC %d out of range", HC);
  }
  const int OS = lidar ? DGPPO_RECT_STRIDE : SD;
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  long fl = up4((long)no * OS) + up4((long)n * SD) + up4((long)ng * SD);
  if (cast) fl += (long)no * 16 + up4((long)n * k * 2) + 2 * up4(R) + SWEEP_WAVES * (up4(R) + up4(k * 2));
  DGPPO_REQUIRE(fl * 4 <= 64 * 1024, "dgppo_env_sweep_fork: the frame does not fit the LDS (%ld bytes)", fl * 4);
  const long nxy = (long)nx * ny;
  DGPPO_REQUIRE(nxy <= (1L << 24), "dgppo_env_sweep_fork: grid too large (nx * ny <= 2^24)");
  const long tiles = (nxy + SWEEP_TILE - 1) / SWEEP_TILE;
  DGPPO_REQUIRE(tiles * n_frames < (1L << 31), "dgppo_env_sweep_fork: too many envs");
  ForkArgs a;
  a.cfg = *cfg;
  a.agent = agent; a.agent_st = agent_st; a.goal = goal; a.obst = obst; a.hits = hits; a.hits_st = hits_st;
  a.ray_cos = ray_cos; a.ray_sin = ray_sin; a.frame_ids = frame_ids; a.agent_id = agent_id; a.nx = nx; a.nxy = (int)nxy;
  a.tiles = (int)tiles; a.xs = xs; a.ys = ys; a.carry = carry; a.carry_st = carry_st; a.HC = HC;
  a.agent_out = agent_out; a.goal_out = goal_out; a.obst_out = obst_out; a.hits_out = hits_out; a.carry_out = carry_out;
  const size_t smem = sizeof(float) * (size_t)fl;
  const dim3 grid((unsigned)(tiles * n_frames));
  hipLaunchKernelGGL(env_sweep_fork_kernel, grid, dim3(SWEEP_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- rollout landscape: the costs of a K-step rollout folded into what Vh is trained on ------------------------------------------
// compute_dec_ocp_gae's Vhs_row recursion (dgppo/algo/utils.py:38-45, discount_to_max) at gae_lambda = 1, per (env, agent) row:
// V = h[K-1]; for k = K-2 .. 0: m = max_c h[k][c], V[c] = max(h[k][c], one_minus_gamma * m + gamma * V[c]) — one multiply, one
// multiply and one add, in that order (this file is built with -ffp-contract=off).  The reference bootstraps with Vh of the state
// after the last step; here the row starts from the last cost itself, so that the net under test stays out of its own ground
// truth.  worst[c] = max_k h[k][c].  Every max propagates NaN (jnp.maximum / jnp.max).
// A lane per row: the nh <= 3 words of a row are consecutive and rows are consecutive, so a wave reads one contiguous range per
// step; NH is a template parameter, the row's values live in named registers.
#define FOLD_NT 256

template <int NH>
__global__ void __launch_bounds__(FOLD_NT) constraint_return_kernel(const float* __restrict__ cost, long cost_st, int K, long rows,
                                                                     float gamma, float omg, float* __restrict__ value,
                                                                     float* __restrict__ worst) {
  const long r = (long)blockIdx.x * FOLD_NT + threadIdx.x;
  if (r >= rows) return;
  const float* h = cost + (size_t)(K - 1) * cost_st + (size_t)r * NH;
  float v0 = h[0], v1 = (NH > 1) ? h[1] : 0.0f, v2 = (NH > 2) ? h[2] : 0.0f;
  float w0 = v0, w1 = v1, w2 = v2;
  for (int k = K - 2; k >= 0; --k) {
    h -= cost_st;
    const float h0 = h[0], h1 = (NH > 1) ? h[1] : 0.0f, h2 = (NH > 2) ? h[2] : 0.0f;
    float m = h0;
    if (NH > 1) m = nanmax(m, h1);
    if (NH > 2) m = nanmax(m, h2);
    const float dm = omg * m;
    v0 = nanmax(h0, dm + gamma * v0); w0 = nanmax(w0, h0);
    if (NH > 1) { v1 = nanmax(h1, dm + gamma * v1); w1 = nanmax(w1, h1); }
    if (NH > 2) { v2 = nanmax(h2, dm + gamma * v2); w2 = nanmax(w2, h2); }
  }
  float* vo = value + (size_t)r * NH;
  float* wo = worst + (size_t)r * NH;
  vo[0] = v0; wo[0] = w0;
  if (NH > 1) { vo[1] = v1; wo[1] = w1; }
  if (NH > 2) { vo[2] = v2; wo[2] = w2; }
}

extern "C" int32_t dgppo_constraint_return(const float* cost, int64_t cost_st, int32_t K, int32_t G, int32_t n_agents, int32_t nh,
                                           float gamma, float one_minus_gamma, float* value, float* worst, void* stream) {
  const char* fn = "dgppo_constraint_return";
  DGPPO_REQUIRE(K >= 1, "%s: K must be >= 1 (got %d)", fn, K);
  DGPPO_REQUIRE(nh >= 1 && nh <= 3, "%s: nh %d outside [1, 3]", fn, nh);
  DGPPO_REQUIRE(G >= 0 && n_agents >= 0, "%s: negative counts", fn);
  if (G == 0 || n_agents == 0) return 0;
  DGPPO_REQUIRE(cost && value && worst, "%s: NULL operand", fn);
  const long rows = (long)G * n_agents;
  DGPPO_REQUIRE(K == 1 || cost_st >= rows * nh, "%s: the step stride %ld is shorter than a step (%ld floats)", fn, (long)cost_st,
                rows * nh);
  const long blocks = (rows + FOLD_NT - 1) / FOLD_NT;
  DGPPO_REQUIRE(blocks < (1L << 31), "%s: too many rows", fn);
  const dim3 grid((unsigned)blocks), block(FOLD_NT);
  hipStream_t s = (hipStream_t)stream;
  if (nh == 1) hipLaunchKernelGGL(constraint_return_kernel<1>, grid, block, 0, s, cost, (long)cost_st, K, rows, gamma, one_minus_gamma, value, worst);
  else if (nh == 2) hipLaunchKernelGGL(constraint_return_kernel<2>, grid, block, 0, s, cost, (long)cost_st, K, rows, gamma, one_minus_gamma, value, worst);
  else hipLaunchKernelGGL(constraint_return_kernel<3>, grid, block, 0, s, cost, (long)cost_st, K, rows, gamma, one_minus_gamma, value, worst);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- lookahead shield: the what-if environments of one step, per (env, agent, candidate action) -----------------------------------
// The barrier shield above trusts the learned Vh one step ahead.  The lookahead shield judges a candidate by what it leads to:
// env g = (e * n + i) * P + p, P = 1 + nv * nu, is a copy of env e in which agent i plays candidate p in the coming step and
// everyone else the policy's action; the plain step kernels then apply that joint action and the deterministic policy rolls the
// copy forward (Engine.lookahead_select).  The fork is pure data movement: every field of env e is repeated n * P times, and only
// row i of the joint action differs between the copies.  The action is NOT clipped here: the step clips (clip_action).
//
// Organisation: a workgroup owns FORKT_TILE consecutive output envs, i.e. ONE contiguous range of every output field, and walks
// each field with unit-stride vector stores; the source vector is found by one division per vector.  The vector width of a field
// (16, 8 or 4 bytes) is the widest its row length and the alignment of its two pointers allow, chosen on the host.  Words are
// moved as integers: a NaN's payload and values outside [-1, 1] arrive as they left.
#define FORKT_NT 256
#define FORKT_TILE 64   // output envs per workgroup

struct ForkField {
  const uint32_t* src;    // source block b starts at src + b * st
  uint32_t* dst;          // [G, len]
  long st;                // words between source blocks: len for a dense [n_env, len] source, the frame stride of a record, 0 for
                          // a field with ONE block (the per-env rows of the action fork below)
  int len;                // words per env; 0: the field is not held
  int vec;                // words per load / store: 4, 2 or 1
};

// the widest vector a field allows: its row length, the stride between its source blocks and both pointers have to be multiples
inline ForkField fork_field(const float* s, float* d, long len, long st) {
  ForkField f;
  f.src = reinterpret_cast<const uint32_t*>(s); f.dst = reinterpret_cast<uint32_t*>(d); f.len = (int)len; f.st = st;
  const uintptr_t al = (uintptr_t)s | (uintptr_t)d;
  f.vec = (len % 4 == 0 && st % 4 == 0 && al % 16 == 0) ? 4 : (len % 2 == 0 && st % 2 == 0 && al % 8 == 0) ? 2 : 1;
  return f;
}

struct TeamForkArgs {
  ForkField f[5];         // agent, goal, obst, hits, carry
  const uint32_t* a_pol;  // [n_env, n, 2]
  const int32_t* ids;     // source env of output block m (dgppo_env_team_action_fork_ids); NULL: m itself
  const uint32_t* us;
  const uint32_t* vs;
  uint32_t* action_out;   // [G, n, 2]
  long G;
  int n, nu, P, nP, avec; // avec: 2 where a_pol and action_out are 8-byte aligned
};

// The one copy loop of the forks: output env g takes source block (g / per), looked up in ids where given (the frame numbers of
// the action fork).  G < 2^31 (the host checks G * n): env numbers are divided as 32-bit words
template <typename V>
__device__ inline void fork_copy(const ForkField& fd, uint32_t g0, int envs, uint32_t per, const int32_t* ids, int tid) {
  constexpr int W = sizeof(V) / 4;
  const int lv = fd.len / W;                                    // vectors per env
  const size_t sv = (size_t)(fd.st / W);                        // vectors between source blocks
  const V* src = reinterpret_cast<const V*>(fd.src);
  V* dst = reinterpret_cast<V*>(fd.dst) + (size_t)g0 * lv;
  const int total = envs * lv;
  for (int o = tid; o < total; o += FORKT_NT) {
    const int gl = o / lv, j = o - gl * lv;
    uint32_t b = (g0 + (uint32_t)gl) / per;
    if (ids != nullptr) b = (uint32_t)ids[b];
    dst[o] = src[(size_t)b * sv + j];
  }
}

template <int NF>
__device__ inline void fork_fields(const ForkField (&f)[NF], uint32_t g0, int envs, uint32_t per, const int32_t* ids, int tid) {
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const ForkField& fd = f[k];
    if (fd.len == 0) continue;
    if (fd.vec == 4) fork_copy<uint4>(fd, g0, envs, per, ids, tid);
    else if (fd.vec == 2) fork_copy<uint2>(fd, g0, envs, per, ids, tid);
    else fork_copy<uint32_t>(fd, g0, envs, per, ids, tid);
  }
}

__global__ void __launch_bounds__(FORKT_NT) env_team_action_fork_kernel(TeamForkArgs a) {
  const int tid = threadIdx.x;
  const uint32_t g0 = blockIdx.x * FORKT_TILE;
  const int envs = (int)min((long)FORKT_TILE, a.G - (long)g0);
  fork_fields(a.f, g0, envs, (uint32_t)a.nP, a.ids, tid);
  // the joint action: a_pol[e]'s words, row i replaced by candidate p (p = 0 is a_pol[e, i] itself)
  const int n = a.n, rows = envs * n;
  for (int o = tid; o < rows; o += FORKT_NT) {
    const int gl = o / n, r = o - gl * n;
    const uint32_t g = g0 + (uint32_t)gl, m = g / (uint32_t)a.nP;
    const uint32_t e = a.ids ? (uint32_t)a.ids[m] : m;
    const int rem = (int)(g - m * (uint32_t)a.nP), i = rem / a.P, p = rem - i * a.P;
    uint2 w;
    if (r == i && p > 0) {
      const int iv = (p - 1) / a.nu, iu = (p - 1) - iv * a.nu;
      w.x = a.us[iu]; w.y = a.vs[iv];
    } else if (a.avec == 2) {
      w = reinterpret_cast<const uint2*>(a.a_pol)[(size_t)e * n + r];
    } else {
      const uint32_t* s = a.a_pol + ((size_t)e * n + r) * 2;
      w.x = s[0]; w.y = s[1];
    }
    const size_t q = (size_t)g0 * n + o;
    if (a.avec == 2) reinterpret_cast<uint2*>(a.action_out)[q] = w;
    else { a.action_out[q * 2] = w.x; a.action_out[q * 2 + 1] = w.y; }
  }
}

// both entry points: the G = n_ids * n * P copies of the envs env_ids[0 .. n_ids) (NULL: env m itself) of n_env dense envs
static int32_t team_action_fork(const char* fn, const dgppo_env_cfg* cfg, const float* agent, const float* goal, const float* obst,
                                const float* hits, const float* a_pol, const float* carry, int32_t HC, int32_t n_env,
                                const int32_t* env_ids, int32_t n_ids, const float* us, int32_t nu, const float* vs, int32_t nv,
                                float* agent_out, float* goal_out, float* obst_out, float* hits_out, float* action_out,
                                float* carry_out, void* stream) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {   // the configuration's own refusal, under this entry point's name
    const std::string why = dgppo_last_error();
    dgppo_set_error("%s: %s", fn, why.c_str());
    return rc;
  }
  DGPPO_REFUSE_VMAS(cfg, fn, "dgppo_vmas_step on a tiled record (there is no VMAS fork)");
  DGPPO_REQUIRE(nu >= 1 && nv >= 1, "%s: nu and nv must be >= 1 (got %d, %d)", fn, nu, nv);
  DGPPO_REQUIRE((long)nu * nv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  DGPPO_REQUIRE(n_env >= 0 && n_ids >= 0, "%s: negative counts", fn);
  DGPPO_REQUIRE(env_ids != nullptr || n_ids == n_env, "%s: without env_ids the list is every env (n_ids %d != n_env %d)", fn, n_ids,
                n_env);
  DGPPO_REQUIRE(n_ids == 0 || n_env >= 1, "%s: %d envs listed of none", fn, n_ids);
  const int n = cfg->n_agents, ng = cfg->n_goals, SD = cfg->state_dim, no = cfg->n_obs, k = cfg->top_k;
  const long P = 1 + (long)nu * nv, nP = (long)n * P;
  DGPPO_REQUIRE((double)n_ids * (double)nP * (double)n < 2147483648.0, "%s: too many envs (G * n < 2^31)", fn);
  const bool lidar = cfg_is_lidar(*cfg), cast = lidar && no > 0;
  if (carry != nullptr) {
    DGPPO_REQUIRE(HC >= 1 && (long)n * HC < (1L << 24), "%s: HC %d out of range", fn, HC);
  }
  if (n_ids == 0) return 0;
  DGPPO_REQUIRE(agent && goal && a_pol && us && vs && agent_out && goal_out && action_out, "%s: NULL operand", fn);
  if (no > 0) {
    DGPPO_REQUIRE(obst, "%s: obst is NULL", fn);
    DGPPO_REQUIRE(obst_out, "%s: obst_out is NULL", fn);
  }
  if (cast) {
    DGPPO_REQUIRE(hits, "%s: hits is NULL", fn);
    DGPPO_REQUIRE(hits_out, "%s: hits_out is NULL", fn);
  } else {
    DGPPO_REQUIRE(!hits && !hits_out, "%s: hits / hits_out are for the kinds that cast rays (LiDAR with obstacles)", fn);
  }
  if (carry != nullptr) DGPPO_REQUIRE(carry_out, "%s: carry_out is NULL", fn);
  const int OS = lidar ? DGPPO_RECT_STRIDE : SD;
  TeamForkArgs a;
  auto field = [](const float* s, float* d, long len) { return fork_field(s, d, len, len); };   // dense [n_env, len] sources
  a.f[0] = field(agent, agent_out, (long)n * SD);
  a.f[1] = field(goal, goal_out, (long)ng * SD);
  a.f[2] = field(obst, obst_out, no > 0 ? (long)no * OS : 0);
  a.f[3] = field(hits, hits_out, cast ? (long)n * k * 2 : 0);
  a.f[4] = field(carry, carry_out, carry != nullptr ? (long)n * HC : 0);
  a.a_pol = reinterpret_cast<const uint32_t*>(a_pol);
  a.ids = env_ids;
  a.us = reinterpret_cast<const uint32_t*>(us); a.vs = reinterpret_cast<const uint32_t*>(vs);
  a.action_out = reinterpret_cast<uint32_t*>(action_out);
  a.avec = (((uintptr_t)a_pol | (uintptr_t)action_out) % 8 == 0) ? 2 : 1;
  a.G = (long)n_ids * nP; a.n = n; a.nu = nu; a.P = (int)P; a.nP = (int)nP;
  const dim3 grid((unsigned)((a.G + FORKT_TILE - 1) / FORKT_TILE));
  hipLaunchKernelGGL(env_team_action_fork_kernel, grid, dim3(FORKT_NT), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t dgppo_env_team_action_fork(const dgppo_env_cfg* cfg, const float* agent, const float* goal, const float* obst,
                                              const float* hits, const float* a_pol, const float* carry, int32_t HC, int32_t n_env,
                                              const float* us, int32_t nu, const float* vs, int32_t nv, float* agent_out,
                                              float* goal_out, float* obst_out, float* hits_out, float* action_out,
                                              float* carry_out, void* stream) {
  return team_action_fork("dgppo_env_team_action_fork", cfg, agent, goal, obst, hits, a_pol, carry, HC, n_env, nullptr, n_env, us,
                          nu, vs, nv, agent_out, goal_out, obst_out, hits_out, action_out, carry_out, stream);
}

// The fork of a later shield round: only the envs env_ids[0 .. n_ids) are copied, output block m from env env_ids[m], and the
// joint action the candidates are set into is a_base[e] — the action held after the rounds so far — not the policy's.  The
// sources stay dense over all n_env envs; the caller guarantees 0 <= env_ids[m] < n_env.
extern "C" int32_t dgppo_env_team_action_fork_ids(const dgppo_env_cfg* cfg, const float* agent, const float* goal,
                                                  const float* obst, const float* hits, const float* a_base, const float* carry,
                                                  int32_t HC, int32_t n_env, const int32_t* env_ids, int32_t n_ids, const float* us,
                                                  int32_t nu, const float* vs, int32_t nv, float* agent_out, float* goal_out,
                                                  float* obst_out, float* hits_out, float* action_out, float* carry_out,
                                                  void* stream) {
  return team_action_fork("dgppo_env_team_action_fork_ids", cfg, agent, goal, obst, hits, a_base, carry, HC, n_env, env_ids,
                          n_ids, us, nu, vs, nv, agent_out, goal_out, obst_out, hits_out, action_out, carry_out, stream);
}


// ---- action rollout landscape: the what-if environments of a RECORDED frame with one agent's action swept ------------------------
// The measured twin of the CBF action landscape above: env g = (f * nv + iv) * nu + iu (dgppo_graph_feats_action_sweep's
// numbering) is a copy of frame fid = frame_ids[f] of ONE environment of a record in which agent `agent_id` is about to play
// (us[iu], vs[iv]) and everyone else their recorded action of that step; the plain step kernels then apply the joint action and the
// deterministic policy rolls the copy forward (Engine.action_rollout_landscape).  No position changes before the step, so nothing
// is cast: the hits are the recorded ones.  The carry rows are the ones the caller points at — the carries AFTER each frame's
// policy forward, which do not depend on the action taken.
//
// Organisation: the team fork's, with the same device code (fork_fields): a workgroup owns FORKT_TILE consecutive output envs and
// walks each field with unit-stride vector stores.  The source block of an output env is a frame of a strided record (agent, hits,
// carry: block frame_ids[g / (nv * nu)] at the field's frame stride, which the vector width has to divide as well) or the single
// block of a per-env field (goal, obst: stride 0).  Words move as integers; the action is NOT clipped: the step clips.
struct ActionForkArgs {
  ForkField f[5];         // agent, goal, obst, hits, carry
  const uint32_t* action; long action_st;   // [n, 2] rows of frame t at action + t * action_st
  const int32_t* frame_ids;
  const uint32_t* us;
  const uint32_t* vs;
  uint32_t* action_out;   // [G, n, 2]
  long G;
  int n, nu, nuv, agent_id, avec;   // avec: 2 where action, its frame stride and action_out are 8-byte aligned
};

__global__ void __launch_bounds__(FORKT_NT) env_action_sweep_fork_kernel(ActionForkArgs a) {
  const int tid = threadIdx.x;
  const uint32_t g0 = blockIdx.x * FORKT_TILE;
  const int envs = (int)min((long)FORKT_TILE, a.G - (long)g0);
  fork_fields(a.f, g0, envs, (uint32_t)a.nuv, a.frame_ids, tid);
  // the joint action: the recorded rows of frame fid, row agent_id replaced by the grid action
  const int n = a.n, rows = envs * n;
  for (int o = tid; o < rows; o += FORKT_NT) {
    const int gl = o / n, r = o - gl * n;
    const uint32_t g = g0 + (uint32_t)gl, f = g / (uint32_t)a.nuv;
    uint2 w;
    if (r == a.agent_id) {
      const int q = (int)(g - f * (uint32_t)a.nuv), iv = q / a.nu, iu = q - iv * a.nu;
      w.x = a.us[iu]; w.y = a.vs[iv];
    } else {
      const uint32_t fid = a.frame_ids ? (uint32_t)a.frame_ids[f] : f;
      const uint32_t* s = a.action + (size_t)fid * a.action_st + (size_t)r * 2;
      if (a.avec == 2) w = *reinterpret_cast<const uint2*>(s);
      else { w.x = s[0]; w.y = s[1]; }
    }
    const size_t q = (size_t)g0 * n + o;
    if (a.avec == 2) reinterpret_cast<uint2*>(a.action_out)[q] = w;
    else { a.action_out[q * 2] = w.x; a.action_out[q * 2 + 1] = w.y; }
  }
}

extern "C" int32_t dgppo_env_action_sweep_fork(const dgppo_env_cfg* cfg, const float* agent, int64_t agent_st, const float* goal,
                                               const float* obst, const float* hits, int64_t hits_st, const float* action,
                                               int64_t action_st, const float* carry, int64_t carry_st, int32_t HC,
                                               const int32_t* frame_ids, int32_t n_frames, int32_t agent_id, const float* us,
                                               int32_t nu, const float* vs, int32_t nv, float* agent_out, float* goal_out,
                                               float* obst_out, float* hits_out, float* action_out, float* carry_out,
                                               void* stream) {
  const char* fn = "dgppo_env_action_sweep_fork";
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {   // the configuration's own refusal, under this entry point's name
    const std::string why = dgppo_last_error();
    dgppo_set_error("%s: %s", fn, why.c_str());
    return rc;
  }
  DGPPO_REFUSE_VMAS(cfg, fn, "dgppo_vmas_step on a tiled record (there is no VMAS fork)");
  DGPPO_REQUIRE(nu >= 1 && nv >= 1, "%s: nu and nv must be >= 1 (got %d, %d)", fn, nu, nv);
  DGPPO_REQUIRE((long)nu * nv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  DGPPO_REQUIRE(n_frames >= 1, "%s: n_frames must be >= 1 (got %d)", fn, n_frames);
  const int n = cfg->n_agents, ng = cfg->n_goals, SD = cfg->state_dim, no = cfg->n_obs, k = cfg->top_k;
  DGPPO_REQUIRE(agent_id >= 0 && agent_id < n, "%s: agent_id %d outside [0, %d)", fn, agent_id, n);
  const long nuv = (long)nu * nv;
  DGPPO_REQUIRE((double)n_frames * (double)nuv * (double)n < 2147483648.0, "%s: too many envs (G * n < 2^31)", fn);
  const bool lidar = cfg_is_lidar(*cfg), cast = lidar && no > 0;
  if (carry != nullptr) {
    DGPPO_REQUIRE(HC >= 1 && (long)n * HC < (1L << 24), "%s: HC %d out of range", fn, HC);
    DGPPO_REQUIRE(carry_st >= (long)n * HC, "%s: the frame stride of carry (%ld) is shorter than its rows (%ld floats)", fn,
                  (long)carry_st, (long)n * HC);
  }
  DGPPO_REQUIRE(agent_st >= (long)n * SD, "%s: the frame stride of agent (%ld) is shorter than its rows (%ld floats)", fn,
                (long)agent_st, (long)n * SD);
  DGPPO_REQUIRE(action_st >= (long)n * 2, "%s: the frame stride of action (%ld) is shorter than its rows (%ld floats)", fn,
                (long)action_st, (long)n * 2);
  if (cast)
    DGPPO_REQUIRE(hits_st >= (long)n * k * 2, "%s: the frame stride of hits (%ld) is shorter than its rows (%ld floats)", fn,
                  (long)hits_st, (long)n * k * 2);
  DGPPO_REQUIRE(agent && goal && action && us && vs && agent_out && goal_out && action_out, "%s: NULL operand", fn);
  if (no > 0) {
    DGPPO_REQUIRE(obst, "%s: obst is NULL", fn);
    DGPPO_REQUIRE(obst_out, "%s: obst_out is NULL", fn);
  }
  if (cast) {
    DGPPO_REQUIRE(hits, "%s: hits is NULL", fn);
    DGPPO_REQUIRE(hits_out, "%s: hits_out is NULL", fn);
  } else {
    DGPPO_REQUIRE(!hits && !hits_out, "%s: hits / hits_out are for the kinds that cast rays (LiDAR with obstacles)", fn);
  }
  if (carry != nullptr) DGPPO_REQUIRE(carry_out, "%s: carry_out is NULL", fn);
  const int OS = lidar ? DGPPO_RECT_STRIDE : SD;
  ActionForkArgs a;
  a.f[0] = fork_field(agent, agent_out, (long)n * SD, agent_st);
  a.f[1] = fork_field(goal, goal_out, (long)ng * SD, 0);
  a.f[2] = fork_field(obst, obst_out, no > 0 ? (long)no * OS : 0, 0);
  a.f[3] = fork_field(hits, hits_out, cast ? (long)n * k * 2 : 0, hits_st);
  a.f[4] = fork_field(carry, carry_out, carry != nullptr ? (long)n * HC : 0, carry_st);
  a.action = reinterpret_cast<const uint32_t*>(action); a.action_st = action_st;
  a.frame_ids = frame_ids;
  a.us = reinterpret_cast<const uint32_t*>(us); a.vs = reinterpret_cast<const uint32_t*>(vs);
  a.action_out = reinterpret_cast<uint32_t*>(action_out);
  a.avec = (((uintptr_t)action | (uintptr_t)action_out) % 8 == 0 && action_st % 2 == 0) ? 2 : 1;
  a.G = (long)n_frames * nuv; a.n = n; a.nu = nu; a.nuv = (int)nuv; a.agent_id = agent_id;
  const dim3 grid((unsigned)((a.G + FORKT_TILE - 1) / FORKT_TILE));
  hipLaunchKernelGGL(env_action_sweep_fork_kernel, grid, dim3(FORKT_NT), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- lookahead shield: selection on the rolled costs ----------------------------------------------------------------------------
// Per (env e, agent i), over the P candidates of the fork above, on the agent's OWN row of its own what-if env g = (e * n + i) * P
// + p:  s[p] = max over the K steps and the nh components of cost[k][g, i, c] — the worst cost (get_cost,
// lidar_env/base.py:203-205) agent i meets within the horizon if it plays candidate p now; NaN-propagating max.  Admissible iff
// s <= -margin; the choice among the candidates is shield_select_kernel's: the same pick_consider / pick_finish.  One wave per (e, i), lanes over the
// candidates: a lane folds K * nh words of ONE row per candidate, 1 / n of what a fold over every row of the what-if envs
// (dgppo_constraint_return) would read, and nothing but the outputs is written.
struct LookaheadArgs {
  const float* cost;      // step 1 of the block record: [K][G, n, nh] with step stride cost_st
  long cost_st;
  const float* a_pol;     // [E, n, 2]
  const float* us;
  const float* vs;
  int rows, n, nh, nu, P, K;
  float margin;
  float* action;          // [E, n, 2]
  int32_t* index;         // [E, n]
  int32_t* flag;          // [E, n]
  float* s;               // [E, n, P] or NULL
};

__global__ void __launch_bounds__(SHIELD_NT) lookahead_select_kernel(LookaheadArgs a) {
  const int lane = threadIdx.x & (DGPPO_WAVE - 1);
  const long row = (long)blockIdx.x * SHIELD_WAVES + threadIdx.x / DGPPO_WAVE;   // row = e * n + i
  if (row >= a.rows) return;                      // whole waves leave: no lane of a live wave is missing from the shuffles
  const int i = (int)(row % a.n), nh = a.nh, P = a.P;
  const float a0 = clip_action(a.a_pol[row * 2]), a1 = clip_action(a.a_pol[row * 2 + 1]);
  const float thr = -a.margin;
  ShieldPick k = pick_init();
  for (int p = lane; p < P; p += DGPPO_WAVE) {
    const float* c = a.cost + (((size_t)row * P + p) * a.n + i) * nh;
    float h = c[0];
    for (int st = 0; st < a.K; ++st, c += a.cost_st)
      for (int cc = 0; cc < nh; ++cc) h = nanmax(h, c[cc]);
    if (a.s != nullptr) a.s[(size_t)row * P + p] = h;
    pick_consider(k, h, p, a0, a1, thr, a.us, a.vs, a.nu);
  }
  pick_finish(k, lane, row, a0, a1, thr, a.us, a.vs, a.nu, a.action, a.index, a.flag);
}

extern "C" int32_t dgppo_lookahead_select(const float* cost, int64_t cost_st, int32_t K, int32_t n_env, int32_t n_agents,
                                          int32_t n_cost, const float* a_pol, const float* us, int32_t nu, const float* vs,
                                          int32_t nv, float margin, float* action, int32_t* index, int32_t* flag, float* s,
                                          void* stream) {
  const char* fn = "dgppo_lookahead_select";
  DGPPO_REQUIRE(n_env >= 0 && n_agents >= 1, "%s: n_env >= 0 and n_agents >= 1 are required", fn);
  DGPPO_REQUIRE(n_cost >= 1 && n_cost <= 3, "%s: n_cost %d outside [1, 3]", fn, n_cost);
  DGPPO_REQUIRE(K >= 1, "%s: K must be >= 1 (got %d)", fn, K);
  DGPPO_REQUIRE(nu >= 1 && nv >= 1, "%s: nu and nv must be >= 1 (got %d, %d)", fn, nu, nv);
  DGPPO_REQUIRE((long)nu * nv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  DGPPO_REQUIRE(margin == margin, "%s: margin must not be NaN", fn);
  const long P = 1 + (long)nu * nv;
  DGPPO_REQUIRE((double)n_env * (double)n_agents * (double)P * (double)n_agents < 2147483648.0,
                "%s: too many envs (G * n < 2^31)", fn);
  const long rows = (long)n_env * n_agents, step = rows * P * n_agents * n_cost;
  DGPPO_REQUIRE(K == 1 || cost_st >= step, "%s: the step stride %ld is shorter than a step (%ld floats)", fn, (long)cost_st, step);
  if (n_env == 0) return 0;
  DGPPO_REQUIRE(cost && a_pol && us && vs && action && index && flag, "%s: NULL operand", fn);
  LookaheadArgs a;
  a.cost = cost; a.cost_st = (long)cost_st; a.a_pol = a_pol; a.us = us; a.vs = vs;
  a.rows = (int)rows; a.n = n_agents; a.nh = n_cost; a.nu = nu; a.P = (int)P; a.K = K;
  a.margin = margin; a.action = action; a.index = index; a.flag = flag; a.s = s;
  const dim3 grid((unsigned)((rows + SHIELD_WAVES - 1) / SHIELD_WAVES));
  hipLaunchKernelGGL(lookahead_select_kernel, grid, dim3(SHIELD_NT), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}


// ---- lookahead shield: the selection of a later round ---------------------------------------------------------------------------
// Round r of Engine.lookahead_select_rounds re-judges the envs env_ids[0 .. n_ids) with the joint action held so far as candidate 0
// (dgppo_env_team_action_fork_ids): the fold is lookahead_select_kernel's on what-if env (m * n + i) * P + p, the pick the same
// pick_consider / pick_settle with the distance measured from the policy's action a_ref, and what an agent commits depends on
// the whole team (mode 1: the lowest-numbered agent that wants to move moves alone).  One workgroup per listed env: its waves
// take the agents in turn and leave every agent's pick in LDS, one barrier, then a thread per agent commits — no atomics, no
// second launch, and nothing depends on the order the waves ran in.  Rows of envs that are not listed are not touched.
struct ReselectArgs {
  const float* cost;      // step 1 of the block record: [K][n_ids * n * P, n, nh] with step stride cost_st
  long cost_st;
  const int32_t* env_ids; // [n_ids] or NULL: env m itself
  const float* a_ref;     // [n_env, n, 2]
  const float* us;
  const float* vs;
  int n, nh, nu, P, K, mode;
  float margin;
  float* action;          // [n_env, n, 2] in and out
  int32_t* index;         // [n_env, n] in and out
  int32_t* flag;          // [n_env, n]
  float* s;               // [n_env, n, P] or NULL
  int32_t* joint;         // [n_env]
  int32_t* changed;       // [n_env]
};

__global__ void __launch_bounds__(SHIELD_NT) lookahead_reselect_kernel(ReselectArgs a) {
  extern __shared__ int32_t rs_pick[];            // [n] the pick, then [n] its flag
  const int tid = threadIdx.x, lane = tid & (DGPPO_WAVE - 1), wave = tid / DGPPO_WAVE;
  const int n = a.n, nh = a.nh, P = a.P;
  int32_t* rs_flag = rs_pick + n;
  const long m = blockIdx.x;
  const long e = a.env_ids ? (long)a.env_ids[m] : m;
  const float thr = -a.margin;
  for (int i = wave; i < n; i += SHIELD_WAVES) {  // the whole wave takes the agent: no lane is missing from the shuffles
    const long row = e * n + i, wrow = m * n + i;
    const float a0 = clip_action(a.action[row * 2]), a1 = clip_action(a.action[row * 2 + 1]);
    const float r0 = clip_action(a.a_ref[row * 2]), r1 = clip_action(a.a_ref[row * 2 + 1]);
    ShieldPick k = pick_init();
    for (int p = lane; p < P; p += DGPPO_WAVE) {
      const float* c = a.cost + (((size_t)wrow * P + p) * n + i) * nh;
      float h = c[0];
      for (int st = 0; st < a.K; ++st, c += a.cost_st)
        for (int cc = 0; cc < nh; ++cc) h = nanmax(h, c[cc]);
      if (a.s != nullptr) a.s[(size_t)row * P + p] = h;
      pick_consider(k, h, p, a0, a1, r0, r1, thr, a.us, a.vs, a.nu);
    }
    int idx, fl;
    pick_settle(k, thr, idx, fl);
    if (lane == 0) { rs_pick[i] = idx; rs_flag[i] = fl; }
  }
  __syncthreads();
  // the lowest-numbered agent that wants to move, and whether candidate 0 — the joint action that was rolled — holds for everyone
  int first = n, unsafe = 0;
  for (int i = 0; i < n; ++i) {
    if (rs_pick[i] != 0 && i < first) first = i;
    unsafe |= rs_flag[i] != 0;
  }
  for (int i = tid; i < n; i += SHIELD_NT) {
    const long row = e * n + i;
    const int idx = rs_pick[i], fl = rs_flag[i];
    const float a0 = clip_action(a.action[row * 2]), a1 = clip_action(a.action[row * 2 + 1]);
    float cu = a0, cv = a1;
    int out;
    if (idx != 0 && (a.mode == 0 || i == first)) {
      pick_candidate(idx, a0, a1, a.us, a.vs, a.nu, cu, cv);
      a.index[row] = idx;
      out = fl;                                   // 1: the pick is admissible; 2: the least bad of none
    } else {
      out = (fl != 0) ? 2 : (a.index[row] == 0 ? 0 : 1);
    }
    a.action[row * 2] = cu; a.action[row * 2 + 1] = cv;
    a.flag[row] = out;
  }
  if (tid == 0) {
    const int ch = first < n;
    a.changed[e] = ch;
    a.joint[e] = ch ? 0 : (unsafe ? 1 : 2);
  }
}

extern "C" int32_t dgppo_lookahead_reselect(const float* cost, int64_t cost_st, int32_t K, int32_t n_ids, int32_t n_agents,
                                            int32_t n_cost, const int32_t* env_ids, const float* a_ref, const float* us,
                                            int32_t nu, const float* vs, int32_t nv, float margin, int32_t mode, float* action,
                                            int32_t* index, int32_t* flag, float* s, int32_t* joint, int32_t* changed,
                                            void* stream) {
  const char* fn = "dgppo_lookahead_reselect";
  DGPPO_REQUIRE(n_ids >= 0 && n_agents >= 1, "%s: n_ids >= 0 and n_agents >= 1 are required", fn);
  DGPPO_REQUIRE(n_agents <= 4096, "%s: n_agents %d above 4096", fn, n_agents);
  DGPPO_REQUIRE(n_cost >= 1 && n_cost <= 3, "%s: n_cost %d outside [1, 3]", fn, n_cost);
  DGPPO_REQUIRE(K >= 1, "%s: K must be >= 1 (got %d)", fn, K);
  DGPPO_REQUIRE(nu >= 1 && nv >= 1, "%s: nu and nv must be >= 1 (got %d, %d)", fn, nu, nv);
  DGPPO_REQUIRE((long)nu * nv < (1L << 24), "%s: grid too large (nu * nv < 2^24)", fn);
  DGPPO_REQUIRE(margin == margin, "%s: margin must not be NaN", fn);
  DGPPO_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (every agent commits) or 1 (one mover) (got %d)", fn, mode);
  const long P = 1 + (long)nu * nv;
  DGPPO_REQUIRE((double)n_ids * (double)n_agents * (double)P * (double)n_agents < 2147483648.0,
                "%s: too many envs (G * n < 2^31)", fn);
  const long rows = (long)n_ids * n_agents, step = rows * P * n_agents * n_cost;
  DGPPO_REQUIRE(K == 1 || cost_st >= step, "%s: the step stride %ld is shorter than a step (%ld floats)", fn, (long)cost_st, step);
  if (n_ids == 0) return 0;
  DGPPO_REQUIRE(cost && a_ref && us && vs && action && index && flag && joint && changed, "%s: NULL operand", fn);
  ReselectArgs a;
  a.cost = cost; a.cost_st = (long)cost_st; a.env_ids = env_ids; a.a_ref = a_ref; a.us = us; a.vs = vs;
  a.n = n_agents; a.nh = n_cost; a.nu = nu; a.P = (int)P; a.K = K; a.mode = mode;
  a.margin = margin; a.action = action; a.index = index; a.flag = flag; a.s = s; a.joint = joint; a.changed = changed;
  const size_t smem = sizeof(int32_t) * 2 * (size_t)n_agents;
  hipLaunchKernelGGL(lookahead_reselect_kernel, dim3((unsigned)n_ids), dim3(SHIELD_NT), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
