// Attention, tiled kernels for large teams (family TILED of attn_family in attn.hip).
#include "nn_attn.h"

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
int32_t launch_attn_tiled(AttnArgs& a, hipStream_t s, bool bwd) {
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
