// Fused row pipelines (fp32 MFMA): chains of row-local layers that the reference runs back to back on the same rows,
// executed by one persistent kernel so that the activations between them never leave the CU.
//
// Reference arithmetic replaced (file:line relative to /root/reference):
//   MLP block (Dense -> LayerNorm -> ReLU) x 2     dgppo/nn/mlp.py:17-29   (hid_sizes (64, 64), act_final=True)
//   GRUCell input projection  x W_i + b_i          dgppo/nn/rnn.py:14-30   (flax GRUCell: dense_i of the r|z|n gates)
//   as composed by                                  dgppo/algo/module/policy.py:191-212, value.py:58-80
#include <type_traits>
#include "common.h"
#include "nn_ln.h"
#include "nn_gru.h"

using f32x4 = __attribute__((ext_vector_type(4))) float;
#define FZ_H 64            // hidden width of every layer in the chain
#define FZ_HL 66           // LDS row stride = 2 (mod 32): A-fragment reads touch banks (2 li + lq) mod 32, distinct in each half-wave (65 was 2-way: r03_nn_counters.json)
#define FZ_RB 32           // rows per tile (2 row tiles of 16 per wave)
#define FZ_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// sum over the 16 lanes of a DPP row (= the 16 columns a wave owns), result valid in every lane.  DPP moves stay inside
// the VALU; __shfl_xor would go through the LDS crossbar (ds_bpermute) with a round trip per step.
__device__ inline float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));   // row_mirror
  return v;
}

struct MlpGiArgs {
  const float* X; int ldx; int M;
  const float *W1, *b1, *g1, *be1, *W2, *b2, *g2, *be2, *Wi, *bi;
  float *p1, *y1, *st1, *p2, *y2, *st2;   // saved for the backward (all NULL in inference)
  float* gi;                              // [M, 192]
};

// One workgroup = 4 waves; wave w owns hidden columns 16w..16w+15 of the 64-wide layers and column tiles w, w+4, w+8 of
// the 192-wide gate projection.  All weight fragments of the wave (16 + 16 + 48 k-step registers) are loaded once and
// stay resident while the workgroup walks 32-row tiles; the next tile's rows are requested while the current one
// computes.  LayerNorm statistics: 16-lane shuffle reduction inside the wave, 4-way exchange through LDS.  Four LDS-only
// barriers per tile.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) mlp_gi_fwd_kernel(MlpGiArgs a) {
  extern __shared__ float sm[];
  float* s_x = sm;                              // [RB][HL]  input rows
  float* s_y1 = s_x + FZ_RB * FZ_HL;            // [RB][HL]  relu(LN(x W1 + b1))
  float* s_y2 = s_y1 + FZ_RB * FZ_HL;           // [RB][HL]  relu(LN(y1 W2 + b2))
  float* s_red = s_y2 + FZ_RB * FZ_HL;          // [RB][8]   per-row (sum, sum of squares) of each of the 4 waves
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int c = w * 16 + li;
  float w1[16], w2[16], wi[16][3];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int k = kk * 4 + lq;
    w1[kk] = a.W1[k * FZ_H + c];
    w2[kk] = a.W2[k * FZ_H + c];
#pragma unroll
    for (int t = 0; t < 3; ++t) wi[kk][t] = a.Wi[k * 192 + t * 64 + c];
  }
  const float b1 = a.b1[c], g1 = a.g1[c], e1 = a.be1[c], b2 = a.b2[c], g2 = a.g2[c], e2 = a.be2[c];
  const float bi0 = a.bi[c], bi1 = a.bi[64 + c], bi2 = a.bi[128 + c];
  const int n_tiles = (a.M + FZ_RB - 1) / FZ_RB;
  const bool vec = ((a.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15) == 0);
  float xpf[2][4];
  auto fetch = [&](int tile) {            // 32 rows x 16 float4 = 512 slots, 2 per lane; rows clamped
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, r = idx >> 4, q = idx & 15;
      int row = tile * FZ_RB + r;
      row = row < a.M ? row : a.M - 1;
      const float* p = a.X + (size_t)row * a.ldx + 4 * q;
      if (vec) { const float4 v = *reinterpret_cast<const float4*>(p); xpf[u][0] = v.x; xpf[u][1] = v.y; xpf[u][2] = v.z; xpf[u][3] = v.w; }
      else { xpf[u][0] = p[0]; xpf[u][1] = p[1]; xpf[u][2] = p[2]; xpf[u][3] = p[3]; }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, r = idx >> 4, q = idx & 15;
      float* d = s_x + r * FZ_HL + 4 * q;
      d[0] = xpf[u][0]; d[1] = xpf[u][1]; d[2] = xpf[u][2]; d[3] = xpf[u][3];
    }
  };
  // y = relu(LN(v)) for this lane's 8 elements (2 row tiles x 4 rows, column c); v is overwritten
  auto ln_relu = [&](float (&v)[2][4], float g, float e, float* s_out, float* y_out, float* st_out, int row0) {
    // partial sums over the wave's 16 columns
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = row16_sum(v[rt][r]), q = row16_sum(v[rt][r] * v[rt][r]);
        if (li == 0) { float* d = s_red + (rt * 16 + lq * 4 + r) * 8 + 2 * w; d[0] = s; d[1] = q; }
      }
    FZ_LDS_BARRIER();
    float4 pa[2][4], pb[2][4];            // all 16 reads in one LDS round trip
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = rt * 16 + lq * 4 + r;
        pa[rt][r] = *reinterpret_cast<const float4*>(s_red + rl * 8);
        pb[rt][r] = *reinterpret_cast<const float4*>(s_red + rl * 8 + 4);
      }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = rt * 16 + lq * 4 + r;
        const float4 p0 = pa[rt][r], p1 = pb[rt][r];
        const float mean = ((p0.x + p0.z) + (p1.x + p1.z)) * (1.0f / 64.0f);
        const float mean2 = ((p0.y + p0.w) + (p1.y + p1.w)) * (1.0f / 64.0f);
        const float var = ln_fast_var(mean, mean2);
        const float rstd = rsqrtf(var + 1e-6f);
        const float y = relu_nan((v[rt][r] - mean) * rstd * g + e);
        s_out[rl * FZ_HL + c] = y;
        const int row = row0 + rl;
        if (y_out != nullptr && row < a.M) {
          y_out[(size_t)row * FZ_H + c] = y;
          if (c == 0) { st_out[(size_t)row * 2] = mean; st_out[(size_t)row * 2 + 1] = rstd; }
        }
      }
    FZ_LDS_BARRIER();
  };
  int tile = blockIdx.x;
  if (tile < n_tiles) { fetch(tile); commit(); }
  __syncthreads();
  for (; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * FZ_RB;
    const int nxt = tile + gridDim.x;
    const bool more = nxt < n_tiles;
    if (more) fetch(nxt);
    __builtin_amdgcn_sched_barrier(0);
    float areg[2][16];
    f32x4 acc[2];
    float v[2][4];
    // ---- layer 1 ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_x[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
    __builtin_amdgcn_sched_barrier(0);    // keep the 32 reads together: one LDS round trip, then MFMAs back to back
    acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], w1[kk], acc[rt], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[rt][r] = acc[rt][r] + b1;
        const int row = row0 + rt * 16 + lq * 4 + r;
        if (a.p1 != nullptr && row < a.M) a.p1[(size_t)row * FZ_H + c] = v[rt][r];
      }
    // (the first barrier inside ln_relu also retires every read of s_x: the next tile's rows may be committed after it)
    ln_relu(v, g1, e1, s_y1, a.y1, a.st1, row0);
    if (more) commit();
    // ---- layer 2 ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_y1[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
    __builtin_amdgcn_sched_barrier(0);
    acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], w2[kk], acc[rt], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[rt][r] = acc[rt][r] + b2;
        const int row = row0 + rt * 16 + lq * 4 + r;
        if (a.p2 != nullptr && row < a.M) a.p2[(size_t)row * FZ_H + c] = v[rt][r];
      }
    ln_relu(v, g2, e2, s_y2, a.y2, a.st2, row0);
    // ---- gate projection ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_y2[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
    __builtin_amdgcn_sched_barrier(0);
    f32x4 ag[2][3];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 3; ++t) ag[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < 3; ++t) ag[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], wi[kk][t], ag[rt][t], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rt * 16 + lq * 4 + r;
        if (row < a.M) {
          float* o = a.gi + (size_t)row * 192 + c;
          o[0] = ag[rt][0][r] + bi0; o[64] = ag[rt][1][r] + bi1; o[128] = ag[rt][2][r] + bi2;
        }
      }
  }
}

// ---- the same chain, rows per WAVE (round 3) ----------------------------------------------------------------------------
// mlp_gi_fwd_kernel above splits the 64 columns of a 32-row tile over the 4 waves of a workgroup: every LayerNorm needs an
// exchange through LDS and two workgroup barriers, four barriers per tile at 2 workgroups per CU (232 VGPRs) — its matrix cores
// are busy 37 % of the time and a launch over 32 768 rows (a rollout step) takes 24 us for 8 us of MFMA work.  Here a WAVE owns
// 16 rows through the whole chain and all 64 / 192 output columns of every layer:
//   * the three weight matrices (80 KB) sit in LDS once per CU ([k][c] rows, stride = 1 (mod 64) x 16 so that the B fragment of
//     a k-step — lane (li, lq) reads W[lq * 16 + kk][ct * 16 + li] — touches 64 different banks); one workgroup of 16 waves
//     per CU shares them (gfx950: a workgroup may declare all 160 KB);
//   * LayerNorm statistics are sums over the lane's 4 column tiles + one 16-lane DPP reduction: no exchange, NO barrier after
//     the weights are staged;
//   * a layer's output (C/D layout) becomes the next layer's A operand through a wave-private 16 x 68 LDS tile (DS operations of
//     a wave execute in order); the contraction index is permuted so that a lane's 16 k-values are 16 consecutive columns
//     (four 16-byte reads; the input rows come straight from global memory the same way).
#define RW_WL 65
#define RW_WIL 193
#define RW_YL 68
#define RW_WAVES 16
__global__ void __launch_bounds__(64 * RW_WAVES) mlp_gi_fwd_rw_kernel(MlpGiArgs a) {
  extern __shared__ float sm[];
  float* sW1 = sm;                               // [64][65]
  float* sW2 = sW1 + 64 * RW_WL;                 // [64][65]
  float* sWi = sW2 + 64 * RW_WL;                 // [64][193]
  float* sP = sWi + 64 * RW_WIL;                 // b1 g1 be1 b2 g2 be2 (6 x 64), bi (192)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  float* sY = sP + 576 + w * (16 * RW_YL);       // wave-private transposition tile
  {   // the 80 KB of weights: five 16-byte loads per thread, ALL requested before the first LDS write (a load -> store loop
      // is one trip to L2 per iteration)
    static_assert(RW_WAVES == 16, "the staging below assumes 1024 threads");
    const float4 v1 = reinterpret_cast<const float4*>(a.W1)[tid], v2 = reinterpret_cast<const float4*>(a.W2)[tid];
    const bool want_gi = a.gi != nullptr;        // without gi (the caller forms it: dgppo_gi_gru1_head_fwd) Wi is not staged
    float4 vi[3] = {};
    if (want_gi) {
#pragma unroll
      for (int j = 0; j < 3; ++j) vi[j] = reinterpret_cast<const float4*>(a.Wi)[j * 1024 + tid];
    }
    {
      const int k = tid >> 4, c = (tid & 15) * 4;
      float* d1 = sW1 + k * RW_WL + c; float* d2 = sW2 + k * RW_WL + c;
      d1[0] = v1.x; d1[1] = v1.y; d1[2] = v1.z; d1[3] = v1.w;
      d2[0] = v2.x; d2[1] = v2.y; d2[2] = v2.z; d2[3] = v2.w;
    }
    if (want_gi) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int q = j * 1024 + tid, k = q / 48, c = (q - k * 48) * 4;
        float* d = sWi + k * RW_WIL + c;
        d[0] = vi[j].x; d[1] = vi[j].y; d[2] = vi[j].z; d[3] = vi[j].w;
      }
    }
  }
  if (tid < 64) {
    sP[tid] = a.b1[tid]; sP[64 + tid] = a.g1[tid]; sP[128 + tid] = a.be1[tid];
    sP[192 + tid] = a.b2[tid]; sP[256 + tid] = a.g2[tid]; sP[320 + tid] = a.be2[tid];
  }
  if (tid < 192 && a.gi != nullptr) sP[384 + tid] = a.bi[tid];
  __syncthreads();
  const int n_tiles = (a.M + 15) >> 4;
  const bool save = a.p1 != nullptr;
  float A[16];
  auto fetch = [&](int tile) {                   // A operand of layer 1: row li of the tile, columns lq * 16 .. + 15
    int row = tile * 16 + li;
    row = row < a.M ? row : a.M - 1;
    const float4* p = reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + lq * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float4 v = p[j]; A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w; }
  };
  // one 64-wide layer: acc = A W + b, LayerNorm + ReLU; result to the wave's LDS tile and back as the next A operand
  auto layer = [&](const float* sW, const float* par, float* p_out, float* y_out, float* st_out, int row0) {
    f32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B fragments come from LDS: the reads of the NEXT four k-steps are in flight while the matrix cores work on the current
    // four (left to itself the compiler emits read -> wait -> 2 MFMAs with one pair of registers: the wave idles on every wait)
    float bw[2][4][4];
    auto ldw = [&](int buf, int g) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float* wr = sW + (lq * 16 + g * 4 + kk) * RW_WL + li;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bw[buf][kk][ct] = wr[ct * 16];
      }
    };
    ldw(0, 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g + 1 < 4) ldw((g + 1) & 1, g + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[g * 4 + kk], bw[g & 1][kk][ct], acc[ct], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float b = par[ct * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[ct][r] += b;
        s[r] += acc[ct][r];
        q[r] = fmaf(acc[ct][r], acc[ct][r], q[r]);
        const int row = row0 + lq * 4 + r;
        if (save && row < a.M) p_out[(size_t)row * FZ_H + ct * 16 + li] = acc[ct][r];
      }
    }
    float mean[4], rstd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mean[r] = row16_sum(s[r]) * (1.0f / 64.0f);
      const float m2 = row16_sum(q[r]) * (1.0f / 64.0f);
      rstd[r] = rsqrtf(ln_fast_var(mean[r], m2) + 1e-6f);
      const int row = row0 + lq * 4 + r;
      if (save && li == 0 && row < a.M) { st_out[(size_t)row * 2] = mean[r]; st_out[(size_t)row * 2 + 1] = rstd[r]; }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float g = par[64 + ct * 16 + li], e = par[128 + ct * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = relu_nan((acc[ct][r] - mean[r]) * rstd[r] * g + e);
        sY[(lq * 4 + r) * RW_YL + ct * 16 + li] = y;
        const int row = row0 + lq * 4 + r;
        if (save && row < a.M) y_out[(size_t)row * FZ_H + ct * 16 + li] = y;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(sY + li * RW_YL + lq * 16 + 4 * j);
      A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w;
    }
  };
  for (int tile = w * gridDim.x + blockIdx.x; tile < n_tiles; tile += gridDim.x * RW_WAVES) {   // consecutive tiles on different CUs
    const int row0 = tile * 16;
    fetch(tile);
    layer(sW1, sP, a.p1, a.y1, a.st1, row0);
    layer(sW2, sP + 192, a.p2, a.y2, a.st2, row0);
    if (!save && a.y2 != nullptr) {   // y2 alone (no gi): from the A operand, 16 bytes per lane
      if (row0 + li < a.M) {
        float4* yp = reinterpret_cast<float4*>(a.y2 + (size_t)(row0 + li) * FZ_H + lq * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) yp[j] = make_float4(A[4 * j], A[4 * j + 1], A[4 * j + 2], A[4 * j + 3]);
      }
    }
    if (a.gi == nullptr) continue;
    // gate projection: 12 column tiles in two halves (24 accumulator registers at a time)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4 ag[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) ag[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      float bg[2][2][6];                           // two k-steps per group, double-buffered (see layer())
      auto ldg = [&](int buf, int g) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const float* wr = sWi + (lq * 16 + g * 2 + kk) * RW_WIL + half * 96 + li;
#pragma unroll
          for (int t = 0; t < 6; ++t) bg[buf][kk][t] = wr[t * 16];
        }
      };
      ldg(0, 0);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (g + 1 < 8) ldg((g + 1) & 1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int t = 0; t < 6; ++t) ag[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[g * 2 + kk], bg[g & 1][kk][t], ag[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const int col = half * 96 + t * 16 + li;
        const float b = sP[384 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + lq * 4 + r;
          if (row < a.M) a.gi[(size_t)row * 192 + col] = ag[t][r] + b;
        }
      }
    }
  }
}

// ---- backward of the chain above: the three input gradients and the two LayerNorm+ReLU backward passes in ONE launch -----
//   dy2 = dgi Wi^T,  dpre2 = LNReLU'(p2, y2, st2, g2; dy2),  dy1 = dpre2 W2^T,  dpre1 = LNReLU'(p1, y1, st1, g1; dy1),
//   dx = dpre1 W1^T  (optionally masked by relu'(mask): the chain's input is a ReLU output for the per-agent networks)
// (jax.grad through MLP + GRUCell input Dense, dgppo/nn/mlp.py:17-29, dgppo/nn/rnn.py:14-30, as taken by
// dgppo/algo/informarl.py:377,440 and dgppo/algo/dgppo.py:316.)  It replaces five launches (dense^T, ln_relu_bwd, dense^T,
// ln_relu_bwd, dense^T) and the two round trips of dy2 / dy1 through HBM; dgppo_mlp_gi_bwd writes dpre2 / dpre1 for the
// weight gradients dW2 = y1^T dpre2, dW1 = x^T dpre1 (dgppo_dense_bwd_w), dgppo_mlp_gi_bwd_w forms them itself (WG below).
// LayerNorm parameter gradients
// (dgamma = sum dl xhat, dbeta = sum dl) are accumulated per workgroup and added with one atomic per column.
// Same tiling as the forward: wave w owns columns 16w..16w+15 of every 64-wide result; W^T fragments (48 + 16 + 16
// registers) stay resident; 32-row tiles; the dgi tile (192 wide) is staged in LDS, the next one prefetched in registers.
struct MlpGiBwdArgs {
  const float* dgi; int M;
  const float *Wi, *W2, *W1, *g2, *g1;
  const float *p2, *y2, *st2, *p1, *y1, *st1;
  const float* mask; int ldm;
  float *dpre2, *dpre1, *dx; int lddx;
  float *dg2, *db2, *dg1, *db1;
  // weight gradients (mlp_gi_bwd_kernel<true> only): x [M, ldx] is the chain's input; part [grid][TW_SLAB] or NULL: atomicAdd
  const float* x; int ldx;
  float* part;
  float* dW2; int ldw2; float* dbias2;
  float* dW1; int ldw1; float* dbias1;
};
// one partial slab of a workgroup: [dW2 64x64 | dbias2 64 | dW1 64x64 | dbias1 64], each half in the [K*N | N] form of a
// dgppo_reduce_desc with a bias
#define TW_HALF (FZ_H * FZ_H + FZ_H)
#define TW_SLAB (2 * TW_HALF)
#define TW_MIN_TILES 4     // tiles a workgroup walks at least when it writes a slab (see dgppo_mlp_gi_bwd_w)
#define FZ_GL 194          // LDS row stride of the dgi tile: = 2 (mod 32)
#ifndef FZ_BWD_RT
#define FZ_BWD_RT 1         // row tiles (of 16 rows) per wave in the backward chain
#endif
#ifndef FZ_BWD_WPE
#define FZ_BWD_WPE 2
#endif

// WG: the weight gradients of the two Dense layers as well, dW2 += y1^T dpre2, dW1 += x^T dpre1 and their bias sums, so that
// dpre2 / dpre1 need not go through HBM (they are written only where given).  Wave w owns the 16 output columns it already
// holds dpre for: its dpre values in the C/D layout (row 4 lq + r, column c) ARE the B operand of k-step r if that step
// contracts over rows {4 lq + r : lq = 0..3}; the A operand reads the same rows of the full 64-wide y1 / x tile from LDS,
// where the four waves put the columns they loaded anyway.  16 MFMAs and 16 accumulator registers per matrix and tile, all
// independent of the dy chain; one slab per workgroup for the common second stage (dgppo_dense_bwd_w_reduce_batch).
// Register budget: <true> compiles to 254 of the 256 VGPRs that two waves per SIMD allow (no AGPRs, no scratch; <false> 210).
// There is no headroom: anything more that is live across the tile loop spills, so check -Rpass-analysis=kernel-resource-usage
// after every edit of the chain.
template <bool WG>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FZ_BWD_WPE, 8))) mlp_gi_bwd_kernel(MlpGiBwdArgs a) {
  // 16-row tiles (ONE row tile per wave, the forward has two): the W^T fragments take 80 registers, every per-row quantity of
  // the two LayerNorm backward passes is live next to them, and two row tiles spill
  constexpr int BRT = FZ_BWD_RT, BRB = 16 * BRT;
  extern __shared__ float sm[];
  float* s_g = sm;                              // [RB][GL]  dgi rows
  float* s_d2 = s_g + BRB * FZ_GL;            // [RB][HL]  dpre2
  float* s_d1 = s_d2 + BRB * FZ_HL;           // [RB][HL]  dpre1
  float* s_red = s_d1 + BRB * FZ_HL;          // [RB][8]   per-row (sum dxhat, sum dxhat xhat) of each of the 4 waves
  float* s_y1 = s_red + BRB * 8;              // [RB][HL]  y1 rows (WG only; rows >= M are zeros)
  float* s_x = s_y1 + BRB * FZ_HL;            // [RB][HL]  x rows  (WG only)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int c = w * 16 + li;
  // B operands of X W^T: B[k][n] = W[n][k]; lane (li, lq) holds k = 4 kk + lq of output column n = c
  float wi[48], w2[16], w1[16];
#pragma unroll
  for (int kk = 0; kk < 48; ++kk) wi[kk] = a.Wi[c * 192 + kk * 4 + lq];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) { w2[kk] = a.W2[c * FZ_H + kk * 4 + lq]; w1[kk] = a.W1[c * FZ_H + kk * 4 + lq]; }
  const float g2 = a.g2[c], g1 = a.g1[c];
  float dgs[2] = {0.f, 0.f}, dbs[2] = {0.f, 0.f};     // this lane's partial sums of dgamma / dbeta: [layer 2, layer 1], column c
  float dcs[2] = {0.f, 0.f};                          // ... and of the Dense bias gradients (column sums of dpre2, dpre1)
  f32x4 aw2[4], aw1[4];                               // dW2 / dW1 rows 16 kt + 4 lq + r, column c
  if constexpr (WG) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) aw2[kt] = aw1[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int n_tiles = (a.M + BRB - 1) / BRB;
  constexpr int GSL = BRB * 48 / 256;       // float4 slots of a dgi tile per lane
  float4 gpf[GSL];
  const bool gvec = (reinterpret_cast<uintptr_t>(a.dgi) & 15) == 0;   // (an aligned dgi takes mlp_gi_bwd_rw_kernel: see the selection)
  auto fetch = [&](int tile) {            // BRB rows x 48 float4; rows clamped
#pragma unroll
    for (int u = 0; u < GSL; ++u) {
      const int idx = u * 256 + tid, r = idx / 48, q = idx - r * 48;
      int row = tile * BRB + r;
      row = row < a.M ? row : a.M - 1;
      const float* p = a.dgi + (size_t)row * 192 + 4 * q;
      if (gvec) gpf[u] = *reinterpret_cast<const float4*>(p);
      else gpf[u] = make_float4(p[0], p[1], p[2], p[3]);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < GSL; ++u) {
      const int idx = u * 256 + tid, r = idx / 48, q = idx - r * 48;
      float2* d = reinterpret_cast<float2*>(s_g + r * FZ_GL + 4 * q);
      d[0] = make_float2(gpf[u].x, gpf[u].y); d[1] = make_float2(gpf[u].z, gpf[u].w);
    }
  };
  // LayerNorm + ReLU backward for this lane's 8 elements (2 row tiles x 4 rows, column c).  v: dy in, dpre out.
  // mid() runs between the two barriers: LDS writes made there are visible after the second one
  auto ln_relu_bwd = [&](float (&v)[BRT][4], const float (&pv)[BRT][4], const float (&yv)[BRT][4], const float2 (&st)[BRT][4], float g,
                         float& dg_acc, float& db_acc, float& dc_acc, float* s_out, float* d_out, int row0, auto&& mid) {
    float xh[BRT][4], dxh[BRT][4];
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = rt * 16 + lq * 4 + r;
        int row = row0 + rl;
        const bool ok = row < a.M;
        row = ok ? row : a.M - 1;
        const float2 ms = st[rt][r];
        xh[rt][r] = (pv[rt][r] - ms.x) * ms.y;
        const float dl = (ok && yv[rt][r] > 0.0f) ? v[rt][r] : 0.0f;
        dg_acc += dl * xh[rt][r];
        db_acc += dl;
        dxh[rt][r] = dl * g;
        const float s1 = row16_sum(dxh[rt][r]), s2 = row16_sum(dxh[rt][r] * xh[rt][r]);
        if (li == 0) { float* d = s_red + rl * 8 + 2 * w; d[0] = s1; d[1] = s2; }
        v[rt][r] = ms.y;                                  // keep rstd for the second half
      }
    FZ_LDS_BARRIER();
    mid();
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = rt * 16 + lq * 4 + r;
        const float4 p0 = *reinterpret_cast<const float4*>(s_red + rl * 8), p1 = *reinterpret_cast<const float4*>(s_red + rl * 8 + 4);
        const float m1 = ((p0.x + p0.z) + (p1.x + p1.z)) * (1.0f / 64.0f);
        const float m2 = ((p0.y + p0.w) + (p1.y + p1.w)) * (1.0f / 64.0f);
        const float dp = v[rt][r] * (dxh[rt][r] - m1 - xh[rt][r] * m2);
        v[rt][r] = dp;
        s_out[rl * FZ_HL + c] = dp;
        const int row = row0 + rl;
        if constexpr (WG) {
          const bool ok = row < a.M;
          if (ok) dc_acc += dp;                           // rows >= M contribute exactly zero, whatever the clamped row holds
          if (ok && d_out != nullptr) d_out[(size_t)row * FZ_H + c] = dp;
        } else {
          if (row < a.M) d_out[(size_t)row * FZ_H + c] = dp;
        }
      }
    FZ_LDS_BARRIER();
  };
  auto load_st = [&](const float* src, int row0, float2 (&o)[BRT][4]) {        // (mean, rstd) of this lane's rows
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + rt * 16 + lq * 4 + r;
        row = row < a.M ? row : a.M - 1;
        o[rt][r] = reinterpret_cast<const float2*>(src)[row];
      }
  };
  auto load8 = [&](const float* src, int ld, int row0, float (&o)[BRT][4]) {      // this lane's 8 elements of a [M, ld] matrix
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + rt * 16 + lq * 4 + r;
        row = row < a.M ? row : a.M - 1;
        o[rt][r] = src[(size_t)row * ld + c];
      }
  };
  // acc[kt] += A^T dpre over the tile's 16 rows: A = s_a (y1 or x rows, zeros past M), B = this lane's dpre values
  auto wgrad = [&](f32x4 (&acc)[4], const float* s_a, const float (&v)[BRT][4], int row0) {
    static_assert(BRT == 1, "the weight-gradient contraction is written for one row tile per wave");
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float bv = (row0 + lq * 4 + r < a.M) ? v[0][r] : 0.0f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_a[(lq * 4 + r) * FZ_HL + kt * 16 + li], bv, acc[kt], 0, 0, 0);
    }
  };
  // the next tile's dgi rows are requested while the current tile computes (3 float4 per lane with 16-row tiles) and committed
  // to LDS once every read of the current tile is retired (after the first barrier pair of the first LayerNorm backward)
  int tile = blockIdx.x;
  if (tile < n_tiles) { fetch(tile); commit(); }
  __syncthreads();
  for (; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * BRB;
    const int nxt = tile + gridDim.x;
    const bool more = nxt < n_tiles;
    if (more) fetch(nxt);
    // everything this tile reads from global memory is requested here, before the first GEMM: a load issued where it is
    // needed costs a full memory round trip per LayerNorm stage (measured: 155 -> 139 -> see profiles/README.md)
    float pv2[BRT][4], yv2[BRT][4], pv1[BRT][4], yv1[BRT][4], mk[BRT][4], xv[BRT][4];
    float2 sv2[BRT][4], sv1[BRT][4];
    load8(a.p2, FZ_H, row0, pv2); load8(a.y2, FZ_H, row0, yv2); load_st(a.st2, row0, sv2);
    load8(a.p1, FZ_H, row0, pv1); load8(a.y1, FZ_H, row0, yv1); load_st(a.st1, row0, sv1);
    if constexpr (WG) {
      load8(a.x, a.ldx, row0, xv);
      if (a.mask != nullptr) {                     // the per-agent networks mask by their own input: one load serves both
        if (a.mask == a.x && a.ldm == a.ldx) {
#pragma unroll
          for (int r = 0; r < 4; ++r) mk[0][r] = xv[0][r];
        } else {
          load8(a.mask, a.ldm, row0, mk);
        }
      }
    } else {
      if (a.mask != nullptr) load8(a.mask, a.ldm, row0, mk);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[BRT];
    float v[BRT][4];
    // ---- dy2 = dgi Wi^T (K = 192) ----
    for (int rt = 0; rt < BRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c0 = 0; c0 < 48; c0 += 8) {          // chunks of 8 k-steps: 16 A registers at a time (the kernel is register-bound)
      float areg[BRT][8];
#pragma unroll
      for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) areg[rt][kk] = s_g[(rt * 16 + li) * FZ_GL + (c0 + kk) * 4 + lq];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk)
#pragma unroll
        for (int rt = 0; rt < BRT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], wi[c0 + kk], acc[rt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[rt][r] = acc[rt][r];
    // (the barriers inside ln_relu_bwd retire every read of s_g: the next tile's rows may be committed after it)
    // (s_y1 / s_x of the previous tile are read until its end: they are rewritten behind the first barrier of this tile)
    ln_relu_bwd(v, pv2, yv2, sv2, g2, dgs[0], dbs[0], dcs[0], s_d2, a.dpre2, row0, [&]() {
      if constexpr (WG) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = lq * 4 + r;
          const bool ok = row0 + rl < a.M;
          s_y1[rl * FZ_HL + c] = ok ? yv1[0][r] : 0.0f;
          s_x[rl * FZ_HL + c] = ok ? xv[0][r] : 0.0f;
        }
      }
    });
    if (more) commit();
    // ---- dy1 = dpre2 W2^T ----
    {
      float areg[BRT][16];
#pragma unroll
      for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_d2[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
      __builtin_amdgcn_sched_barrier(0);
      for (int rt = 0; rt < BRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int rt = 0; rt < BRT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], w2[kk], acc[rt], 0, 0, 0);
      if constexpr (WG) wgrad(aw2, s_y1, v, row0);          // v still holds dpre2: independent MFMAs next to the dependent chain
    }
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[rt][r] = acc[rt][r];
    ln_relu_bwd(v, pv1, yv1, sv1, g1, dgs[1], dbs[1], dcs[1], s_d1, a.dpre1, row0, []() {});
    // ---- dx = dpre1 W1^T ----
    {
      float areg[BRT][16];
#pragma unroll
      for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_d1[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
      __builtin_amdgcn_sched_barrier(0);
      for (int rt = 0; rt < BRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int rt = 0; rt < BRT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], w1[kk], acc[rt], 0, 0, 0);
      if constexpr (WG) wgrad(aw1, s_x, v, row0);
    }
#pragma unroll
    for (int rt = 0; rt < BRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rt * 16 + lq * 4 + r;
        float o = acc[rt][r];
        if (a.mask != nullptr) o = (mk[rt][r] > 0.0f) ? o : 0.0f;
        if (row < a.M) a.dx[(size_t)row * a.lddx + c] = o;
      }
    // (s_d1 is next written after two more barriers of the following tile: no hazard with the reads above)
  }
  // ---- LayerNorm parameter gradients: sum the 4 row groups of each column in LDS, one atomic per column and workgroup ----
  __syncthreads();
  float* red = sm;                                // [4 (+ 2) values][4 lq][64 columns]
  red[(0 * 4 + lq) * 64 + c] = dgs[0]; red[(1 * 4 + lq) * 64 + c] = dbs[0];
  red[(2 * 4 + lq) * 64 + c] = dgs[1]; red[(3 * 4 + lq) * 64 + c] = dbs[1];
  if constexpr (WG) { red[(4 * 4 + lq) * 64 + c] = dcs[0]; red[(5 * 4 + lq) * 64 + c] = dcs[1]; }
  __syncthreads();
  auto colsum = [&](int which, int col) {
    return (red[(which * 4 + 0) * 64 + col] + red[(which * 4 + 1) * 64 + col]) +
           (red[(which * 4 + 2) * 64 + col] + red[(which * 4 + 3) * 64 + col]);
  };
  {
    const int which = tid >> 6, col = tid & 63;
    float* dst = which == 0 ? a.dg2 : (which == 1 ? a.db2 : (which == 2 ? a.dg1 : a.db1));
    atomicAdd(dst + col, colsum(which, col));
  }
  if constexpr (WG) {
    float* slab = a.part ? a.part + (size_t)blockIdx.x * TW_SLAB : nullptr;
    if (tid < 128) {                              // Dense bias gradients: layer 2, layer 1
      const int l = tid >> 6, col = tid & 63;
      const float tot = colsum(4 + l, col);
      if (slab) slab[l * TW_HALF + FZ_H * FZ_H + col] = tot;
      else atomicAdd((l == 0 ? a.dbias2 : a.dbias1) + col, tot);
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = kt * 16 + lq * 4 + r;
        if (slab) {
          slab[krow * FZ_H + c] = aw2[kt][r];
          slab[TW_HALF + krow * FZ_H + c] = aw1[kt][r];
        } else {
          atomicAdd(a.dW2 + (size_t)krow * a.ldw2 + c, aw2[kt][r]);
          atomicAdd(a.dW1 + (size_t)krow * a.ldw1 + c, aw1[kt][r]);
        }
      }
  }
}

// grid cap of the persistent backward chain kernel: every workgroup the device can hold at once
template <bool WG>
static int mlp_gi_bwd_cap(size_t smem) {
  static thread_local int cap = 0;
  if (cap == 0) {
    int per_cu = 0, dev = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&mlp_gi_bwd_kernel<WG>), 256, smem) !=
            hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    cap = per_cu * cus;
  }
  return cap;
}
template <bool WG>
constexpr size_t mlp_gi_bwd_smem() {
  constexpr int BRB = 16 * FZ_BWD_RT;
  // the final reduction of the LayerNorm (and bias) gradients reuses the tile buffers
  constexpr size_t smem_t = sizeof(float) * (BRB * FZ_GL + (WG ? 4 : 2) * BRB * FZ_HL + BRB * 8), smem_r = sizeof(float) * (WG ? 24 : 16) * 64;
  return smem_t > smem_r ? smem_t : smem_r;
}

// ---- the same backward chain, rows per WAVE (round 12) -----------------------------------------------------------------------
// mlp_gi_bwd_kernel above has the shape mlp_gi_fwd_kernel had: the 64 columns of a tile split over four waves, so each LayerNorm
// backward is a cross-wave exchange with two barriers, each product one dependent chain of MFMAs, and 80 registers of W^T next to
// everything else.  Here, as in mlp_gi_fwd_rw_kernel, a WAVE owns 16 rows through the whole chain and all 64 columns of each result:
//   * the three weight matrices sit in LDS once per workgroup in the forward's [k][c] layout; the B fragment of X W^T is the
//     transposed read — lane (li, lq) reads W[ct * 16 + li][lq * 16 + kk]: bank (li + 16 lq + kk) mod 64, all different;
//   * four independent accumulators per product, B fragments double-buffered two k-steps at a time;
//   * dgi rows come from global memory in the A layout, 32 bytes per lane and chunk of 8 k-steps, two chunks in flight;
//   * both row sums of a LayerNorm backward are sums over the lane's four column tiles + row16_sum: no exchange, no barrier;
//   * dpre2 / dpre1 become the next A operand through the wave's own 16 x 68 LDS tile (DS operations of a wave execute in order);
//     rows >= M are written there as zeros, so the tile is also the B operand of the weight gradients;
//   * WG: dW2 += y1^T dpre2 and dW1 += x^T dpre1 with BOTH operands in the C/D layout (y1 and x are loaded in it anyway, as the
//     ReLU mask of layer 1 and of dx): k-step r contracts rows {4 lq + r}; 64 MFMAs and 64 accumulator registers per matrix,
//     live across the tile loop.  dpre comes back from the LDS tile (16 reads) rather than staying live through the next product.
// Register plan at two waves per SIMD (256): 128 dW accumulators, 8 running bias sums (those of dgamma / dbeta sit in LDS), and a
// chain that requests each tile's p / y / st / x one stage ahead of their use and no earlier.  <true> compiles to exactly 256
// VGPRs without scratch (profiles/r12_resource_usage.txt; profiles/README.md, round 12, lists what that took): tile bases are
// scalar, lane offsets 32-bit and formed where they are used.  Check -Rpass-analysis=kernel-resource-usage after every edit.
// End: LayerNorm / bias sums of the 8 waves x 4 row groups are added in LDS in a fixed order; the dW accumulators meet in wave 0
// through lane-major LDS images in three halving rounds (head_bwd_kernel), one slab per workgroup.
#define BRW_WAVES 8
#define BRW_SUMS 16                                         // dgamma / dbeta running sums of a lane: [layer][kind][ct]
#define BRW_CHAIN_FLOATS (2 * 64 * RW_WL + 64 * RW_WIL + 128 + BRW_WAVES * 16 * RW_YL + BRW_WAVES * BRW_SUMS * 64)
#define BRW_IMAGE_FLOATS ((BRW_WAVES / 2) * 128 * 64)      // first halving round: 4 waves x 128 values x 64 lanes
template <bool WG>
__global__ void __launch_bounds__(64 * BRW_WAVES) mlp_gi_bwd_rw_kernel(MlpGiBwdArgs a) {
  extern __shared__ float sm[];
  float* sW1 = sm;                               // [64][65]   W1[k][c]
  float* sW2 = sW1 + 64 * RW_WL;                 // [64][65]
  float* sWi = sW2 + 64 * RW_WL;                 // [64][193]
  float* sP = sWi + 64 * RW_WIL;                 // g2, g1
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: tile bases below are scalar, lane offsets 32-bit
  float* sY = sP + 128 + w * (16 * RW_YL);       // wave-private transposition tile
  // the lane's running sums of dgamma / dbeta live in LDS (slot j at [j][lane]: conflict-free, touched by this lane alone):
  // next to the 128 dW accumulators there are no 16 registers for them while a tile's saved rows are in flight
  float* sS = sP + 128 + BRW_WAVES * (16 * RW_YL) + w * (BRW_SUMS * 64) + lane;
#pragma unroll
  for (int j = 0; j < BRW_SUMS; ++j) sS[j * 64] = 0.0f;
  {   // weights as single words (parameter slices: any alignment), ALL requested before the first LDS write
    static_assert(BRW_WAVES == 8, "the staging below assumes 512 threads");
    float v1[8], v2[8], vi[24];
#pragma unroll
    for (int j = 0; j < 8; ++j) { v1[j] = a.W1[j * 512 + tid]; v2[j] = a.W2[j * 512 + tid]; }
#pragma unroll
    for (int j = 0; j < 24; ++j) vi[j] = a.Wi[j * 512 + tid];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = j * 512 + tid, k = idx >> 6, c = idx & 63;
      sW1[k * RW_WL + c] = v1[j]; sW2[k * RW_WL + c] = v2[j];
    }
#pragma unroll
    for (int j = 0; j < 24; ++j) {
      const int idx = j * 512 + tid, k = idx / 192, c = idx - k * 192;
      sWi[k * RW_WIL + c] = vi[j];
    }
  }
  if (tid < 64) { sP[tid] = a.g2[tid]; sP[64 + tid] = a.g1[tid]; }
  __syncthreads();
  f32x4 aw2[4][4], aw1[4][4];                    // dW2 / dW1 rows 16 kt + 4 lq + r, columns 16 ct + li (WG)
  float dcs[2][4];                               // running sums of the Dense bias gradients: [layer 2, layer 1][ct]
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) aw2[kt][ct] = aw1[kt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < 2; ++l)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) dcs[l][ct] = 0.0f;
  const int n_tiles = (a.M + 15) >> 4, stride = gridDim.x * BRW_WAVES;
  // element i (a 32-bit lane offset) of a scalar tile base: scalar base + 32-bit byte offset is one address register, not two
  auto at = [](auto* base, unsigned i) -> decltype(*base)& {
    using T = std::remove_reference_t<decltype(*base)>;
    using B = std::conditional_t<std::is_const_v<T>, const char, char>;
    return *reinterpret_cast<T*>(reinterpret_cast<B*>(base) + i * (unsigned)sizeof(T));
  };
  const bool x_masks = WG && a.mask == a.x && a.ldm == a.ldx;      // the per-agent networks mask by their own input: one load
  // dgi in the A layout: row li, k-step s of the product reads column (s >> 4) * 64 + lq * 16 + (s & 15); chunk q = 8 k-steps
  float G[2][8];
  auto grow = [&](int t) {                       // t < n_tiles: the clamped row is never below the tile's first
    const int last = a.M - 1 - t * 16;           // scalar
    int l = lane;
    asm volatile("" : "+v"(l));                  // (li and 16 lq are formed here, twice a tile, rather than kept in registers)
    const int rl = (l & 15) < last ? (l & 15) : last;
    return &at(a.dgi + (size_t)t * (16 * 192), (unsigned)(rl * 192 + (l & 48)));
  };
  auto fetchG = [&](int buf, const float* gp, int q) {
    const float4* p = reinterpret_cast<const float4*>(gp + (q >> 1) * 64 + (q & 1) * 8);
    const float4 u0 = p[0], u1 = p[1];
    G[buf][0] = u0.x; G[buf][1] = u0.y; G[buf][2] = u0.z; G[buf][3] = u0.w;
    G[buf][4] = u1.x; G[buf][5] = u1.y; G[buf][6] = u1.z; G[buf][7] = u1.w;
  };
  // one 64-wide product from the wave's LDS tile: acc = A W^T, A = row li, columns lq * 16 .. + 15 of the tile
  auto gemm64 = [&](f32x4 (&acc)[4], const float* sW) {
    float A[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(sY + li * RW_YL + lq * 16 + 4 * j);
      A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w;
    }
    float bw[2][2][4];
    auto ldb = [&](int buf, int g) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const float* wr = sW + li * RW_WL + lq * 16 + g * 2 + kk;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bw[buf][kk][ct] = wr[ct * 16 * RW_WL];
      }
    };
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    ldb(0, 0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g + 1 < 8) ldb((g + 1) & 1, g + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[g * 2 + kk], bw[g & 1][kk][ct], acc[ct], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int tile = w * gridDim.x + blockIdx.x;         // consecutive tiles on different CUs
  if (tile < n_tiles) { const float* gp = grow(tile); fetchG(0, gp, 0); fetchG(1, gp, 1); }
  for (; tile < n_tiles; tile += stride) {          // (the tile's first two dgi chunks are on their way)
    const int row0 = tile * 16;
    const float* gp = grow(tile);
    int rl[4]; bool ok[4];                       // this lane's rows in the C/D layout, relative to row0, clamped
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int last = a.M - 1 - row0;           // scalar
      ok[r] = lq * 4 + r <= last;
      rl[r] = ok[r] ? lq * 4 + r : last;
      asm volatile("" : "+v"(rl[r]));            // offsets are formed from these four where they are used: as selects between a
    }                                            // hoisted (lq * 4 + r) * ld + li and the clamped row they cost 4 registers per ld
    auto load16 = [&](const float* src, int ld, float (&o)[4][4]) {
      const float* base = src + (size_t)row0 * ld;               // scalar
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[ct][r] = at(base + ct * 16, (unsigned)(rl[r] * ld + li));
    };
    auto load_st = [&](const float* src, float2 (&o)[4]) {
      const float2* base = reinterpret_cast<const float2*>(src) + row0;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = at(base, (unsigned)rl[r]);
    };
    // LayerNorm + ReLU backward on the C/D layout: v = dy in, dpre out (zeros in rows >= M), also to the wave's LDS tile
    auto ln_relu_bwd = [&](f32x4 (&v)[4], float (&pv)[4][4], const float (&yv)[4][4], const float2 (&st)[4], const float* gam,
                           float* s_acc, float (&dc_acc)[4], float* d_out) {
      float* d_base = d_out + (size_t)row0 * FZ_H;               // (only dereferenced where d_out is given)
      float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float g = gam[ct * 16 + li];
        float dg_t = 0.0f, db_t = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float2 ms = st[r];
          const float xh = (pv[ct][r] - ms.x) * ms.y;
          const float dl = (ok[r] && yv[ct][r] > 0.0f) ? v[ct][r] : 0.0f;
          dg_t += dl * xh;
          db_t += dl;
          const float dxh = dl * g;
          s1[r] += dxh;
          s2[r] += dxh * xh;
          pv[ct][r] = xh;
          v[ct][r] = dxh;
        }
        s_acc[ct * 64] += dg_t;
        s_acc[(4 + ct) * 64] += db_t;
      }
      float m1[4], m2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        m1[r] = row16_sum(s1[r]) * (1.0f / 64.0f);
        m2[r] = row16_sum(s2[r]) * (1.0f / 64.0f);
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dp = st[r].y * (v[ct][r] - m1[r] - pv[ct][r] * m2[r]);
          if (ok[r]) {                                          // rows >= M contribute exactly zero, whatever the clamped row holds
            dc_acc[ct] += dp;
            if (d_out != nullptr) at(d_base + ct * 16, (unsigned)(rl[r] * FZ_H + li)) = dp;
          }
          v[ct][r] = ok[r] ? dp : 0.0f;
          sY[(lq * 4 + r) * RW_YL + ct * 16 + li] = v[ct][r];
        }
      // the bias sums are complete HERE: left alone, the compiler sinks such additions to the end of the tile and keeps their
      // terms live until then
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) asm volatile("" : "+v"(dc_acc[ct]));
    };
    // acc[kt][ct] += A^T dpre over the tile's rows: A = av (y1 or x in the C/D layout, zeros past M), dpre from the wave's tile
    auto wgrad = [&](f32x4 (&acc)[4][4], const float (&av)[4][4]) {
      float bv[4][4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[ct][r] = sY[(lq * 4 + r) * RW_YL + ct * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const float x = ok[r] ? av[kt][r] : 0.0f;
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[kt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, bv[ct][r], acc[kt][ct], 0, 0, 0);
        }
    };
    float pv[4][4], yv[4][4];
    float2 sv[4];
    load16(a.p2, FZ_H, pv); load16(a.y2, FZ_H, yv); load_st(a.st2, sv);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[4];
    // ---- dy2 = dgi Wi^T (K = 192): 48 k-steps, the B fragment one step ahead (this is the stage where the tile's saved rows
    // are in flight next to the dgi chunks: two steps ahead, as in gemm64, is 8 registers too many); the dgi chunk two ahead is
    // requested when its buffer falls free ----
    {
      float bw[2][4];
      auto ldb = [&](int buf, int s) {
        const float* wr = sWi + li * RW_WIL + (s >> 4) * 64 + lq * 16 + (s & 15);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bw[buf][ct] = wr[ct * 16 * RW_WIL];
      };
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      ldb(0, 0);
#pragma unroll
      for (int s = 0; s < 48; ++s) {
        if (s + 1 < 48) ldb((s + 1) & 1, s + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(G[(s >> 3) & 1][s & 7], bw[s & 1][ct], acc[ct], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if ((s & 7) == 7 && (s >> 3) + 2 < 6) fetchG((s >> 3) & 1, gp, (s >> 3) + 2);
      }
    }
    ln_relu_bwd(acc, pv, yv, sv, sP, sS, dcs[0], a.dpre2);
    // layer 1's saved rows are requested here and land behind the next product
    float xv[4][4];
    load16(a.p1, FZ_H, pv); load16(a.y1, FZ_H, yv); load_st(a.st1, sv);
    __builtin_amdgcn_sched_barrier(0);
    // ---- dy1 = dpre2 W2^T, then dW2 += y1^T dpre2 ----
    gemm64(acc, sW2);
    if constexpr (WG) {
      wgrad(aw2, yv);
      load16(a.x, a.ldx, xv);
      __builtin_amdgcn_sched_barrier(0);
    }
    ln_relu_bwd(acc, pv, yv, sv, sP + 64, sS + 8 * 64, dcs[1], a.dpre1);
    // ---- dx = dpre1 W1^T, then dW1 += x^T dpre1 ----
    gemm64(acc, sW1);
    if (a.mask != nullptr) {
      if (x_masks) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[ct][r] = xv[ct][r] > 0.0f ? acc[ct][r] : 0.0f;
      } else {                                   // a separate mask is the rare form: requested where it is used, a row at a time
        const float* mb = a.mask + (size_t)row0 * a.ldm;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float mk[4];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) mk[ct] = at(mb + ct * 16, (unsigned)(rl[r] * a.ldm + li));
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[ct][r] = mk[ct] > 0.0f ? acc[ct][r] : 0.0f;
        }
      }
    }
    float* dxb = a.dx + (size_t)row0 * a.lddx;
    unsigned ob = (unsigned)(lq * 4 * a.lddx + li);              // (a stored row is never a clamped one)
    asm volatile("" : "+v"(ob));                 // formed here: hoisted out of the tile loop, the four row offsets cost 8 registers
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ok[r]) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) at(dxb + ct * 16, ob + (unsigned)(r * a.lddx)) = acc[ct][r];
      }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (WG) wgrad(aw1, xv);
    if (tile + stride < n_tiles) { const float* gn = grow(tile + stride); fetchG(0, gn, 0); fetchG(1, gn, 1); }
  }
  // ---- LayerNorm parameter (and Dense bias) gradients: 8 waves x 4 row groups per column, added in LDS in a fixed order ----
  float dgs[2][4], dbs[2][4];
#pragma unroll
  for (int l = 0; l < 2; ++l)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) { dgs[l][ct] = sS[(l * 8 + ct) * 64]; dbs[l][ct] = sS[(l * 8 + 4 + ct) * 64]; }
  __syncthreads();                               // the weights, every wave's tile and its sums are dead
  constexpr int NK = WG ? 3 : 2;                 // kinds per layer: dgamma, dbeta(, dbias)
  {
    const int slot = w * 4 + lq;
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int col = ct * 16 + li;
        sm[((l * NK + 0) * 32 + slot) * 64 + col] = dgs[l][ct];
        sm[((l * NK + 1) * 32 + slot) * 64 + col] = dbs[l][ct];
        if constexpr (WG) sm[((l * NK + 2) * 32 + slot) * 64 + col] = dcs[l][ct];
      }
  }
  __syncthreads();
  float* slab = (WG && a.part) ? a.part + (size_t)blockIdx.x * TW_SLAB : nullptr;
  if (tid < 2 * NK * 64) {
    const int which = tid >> 6, col = tid & 63, l = which / NK, kind = which - l * NK;
    float tot = 0.0f;
    for (int j = 0; j < 32; ++j) tot += sm[(which * 32 + j) * 64 + col];
    if (kind == 0) atomicAdd((l == 0 ? a.dg2 : a.dg1) + col, tot);
    else if (kind == 1) atomicAdd((l == 0 ? a.db2 : a.db1) + col, tot);
    else if (slab) slab[l * TW_HALF + FZ_H * FZ_H + col] = tot;
    else atomicAdd((l == 0 ? a.dbias2 : a.dbias1) + col, tot);
  }
  if constexpr (WG) {
    // the eight waves' dW accumulators meet in wave 0: three halving rounds through lane-major LDS images (slot j of lane l at
    // [j][l]: conflict-free, the same lane of every wave holds the same element), then wave 0 writes the slab from registers
    auto each = [&](auto&& f) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            aw2[kt][ct][r] = f((kt * 4 + ct) * 4 + r, aw2[kt][ct][r]);
            aw1[kt][ct][r] = f(64 + (kt * 4 + ct) * 4 + r, aw1[kt][ct][r]);
          }
    };
    __syncthreads();                             // the column sums above are read
#pragma unroll
    for (int half = BRW_WAVES / 2; half >= 1; half >>= 1) {
      if (w >= half && w < 2 * half) each([&](int j, float v) { sm[((w - half) * 128 + j) * 64 + lane] = v; return v; });
      __syncthreads();
      if (w < half) each([&](int j, float v) { return v + sm[(w * 128 + j) * 64 + lane]; });
      __syncthreads();
    }
    if (w != 0) return;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int krow = kt * 16 + lq * 4 + r, col = ct * 16 + li;
          if (slab) {
            slab[krow * FZ_H + col] = aw2[kt][ct][r];
            slab[TW_HALF + krow * FZ_H + col] = aw1[kt][ct][r];
          } else {
            atomicAdd(a.dW2 + (size_t)krow * a.ldw2 + col, aw2[kt][ct][r]);
            atomicAdd(a.dW1 + (size_t)krow * a.ldw1 + col, aw1[kt][ct][r]);
          }
        }
  }
}

static int head_bwd_cus();                      // (the device's CU count, defined with dgppo_head_bwd below)
// Which kernel a call runs, for BOTH entry points (by shape and alignment only): the rows-per-wave form needs 16-byte dgi rows
// (192 floats: the first one decides); every other operand moves as single words.  Its grid: one 8-wave workgroup per CU, fewer
// when the 16-row tiles do not give every wave one.
static bool mlp_gi_bwd_rw_selected(const float* dgi, int M) { return M > 0 && (reinterpret_cast<uintptr_t>(dgi) & 15) == 0; }
static int mlp_gi_bwd_rw_grid(int M) {
  const int tiles = (M + 15) / 16, want = (tiles + BRW_WAVES - 1) / BRW_WAVES, cus = head_bwd_cus();
  return want < cus ? want : cus;
}
template <bool WG>
constexpr size_t mlp_gi_bwd_rw_smem() {
  return sizeof(float) * ((WG && BRW_IMAGE_FLOATS > BRW_CHAIN_FLOATS) ? BRW_IMAGE_FLOATS : BRW_CHAIN_FLOATS);
}
template <bool WG>
static int32_t mlp_gi_bwd_rw_launch(const MlpGiBwdArgs& a, int grid, hipStream_t stream) {
  constexpr size_t smem = mlp_gi_bwd_rw_smem<WG>();
  static_assert(smem <= 160 * 1024 && sizeof(float) * 2 * 3 * 32 * 64 <= smem, "mlp_gi_bwd_rw: LDS image");
  static thread_local bool opted = false;
  if (!opted) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_gi_bwd_rw_kernel<WG>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    DGPPO_REQUIRE(e == hipSuccess, "mlp_gi_bwd: cannot reserve %zu bytes of LDS per workgroup: %s", smem, hipGetErrorString(e));
    opted = true;
  }
  hipLaunchKernelGGL(mlp_gi_bwd_rw_kernel<WG>, dim3(grid), dim3(64 * BRW_WAVES), smem, stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t dgppo_mlp_gi_bwd(const float* dgi, const float* Wi, const float* W2, const float* W1, const float* g2,
                                    const float* g1, const float* p2, const float* y2, const float* st2, const float* p1,
                                    const float* y1, const float* st1, const float* relu_mask, int32_t ldm, float* dpre2,
                                    float* dpre1, float* dx, int32_t lddx, float* dg2, float* db2, float* dg1, float* db1,
                                    int32_t M, void* stream) {
  DGPPO_REQUIRE(M >= 0 && lddx >= FZ_H && (relu_mask == nullptr || ldm >= FZ_H), "mlp_gi_bwd: bad shape M=%d lddx=%d ldm=%d", M, lddx, ldm);
  DGPPO_REQUIRE(dgi && Wi && W2 && W1 && g2 && g1 && p2 && y2 && st2 && p1 && y1 && st1 && dpre2 && dpre1 && dx && dg2 && db2 &&
                dg1 && db1, "mlp_gi_bwd: NULL operand");
  if (M == 0) return 0;
  MlpGiBwdArgs a{dgi, M, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, relu_mask, ldm, dpre2, dpre1, dx, lddx, dg2, db2, dg1, db1,
                 nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr};
  if (mlp_gi_bwd_rw_selected(dgi, M)) return mlp_gi_bwd_rw_launch<false>(a, mlp_gi_bwd_rw_grid(M), (hipStream_t)stream);
  constexpr size_t smem = mlp_gi_bwd_smem<false>();
  const int cap = mlp_gi_bwd_cap<false>(smem);
  const int tiles = (M + 16 * FZ_BWD_RT - 1) / (16 * FZ_BWD_RT);
  hipLaunchKernelGGL(mlp_gi_bwd_kernel<false>, dim3(tiles < cap ? tiles : cap), dim3(256), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- the same chain with the trunk's weight gradients (mlp_gi_bwd_kernel<true>) ----------------------------------------------
// One slab per workgroup.  The grid is the device's capacity (2 workgroups per CU) as long as every workgroup walks at least
// TW_MIN_TILES tiles: below that the slab a workgroup writes (33 KB) outweighs the rows it reads (7.4 KB per tile), so fewer
// workgroups walk more tiles (16 384 rows with the batched reduce: 44 us at 1 or 2 tiles, 39 at 4, 51 at 8); at <= 4 workgroups
// the sums go straight into the outputs with atomicAdd, as in dense_bwd_w.
// The rows-per-wave form (mlp_gi_bwd_rw_kernel<true>, an aligned dgi) writes one slab per workgroup of its own grid, which is the
// grid of dgppo_mlp_gi_bwd at the same M: at most one per CU, and the workspace is sized for that.  Up to 4 workgroups, or
// with no room for a slab each, it adds atomically from the SAME grid.  mlp_gi_bwd_kernel<true> with that workspace walks
// at most one workgroup per slab.
extern "C" int64_t dgppo_mlp_gi_bwd_w_workspace_bytes(void) { return (int64_t)TW_SLAB * sizeof(float) * head_bwd_cus(); }

extern "C" int32_t dgppo_mlp_gi_bwd_w(const float* dgi, const float* Wi, const float* W2, const float* W1, const float* g2,
                                      const float* g1, const float* p2, const float* y2, const float* st2, const float* p1,
                                      const float* y1, const float* st1, const float* x, int32_t ldx, const float* relu_mask,
                                      int32_t ldm, float* dpre2, float* dpre1, float* dx, int32_t lddx, float* dg2, float* db2,
                                      float* dg1, float* db1, float* dW2, int32_t ldw2, float* dbias2, float* dW1, int32_t ldw1,
                                      float* dbias1, int32_t M, float* workspace, int64_t workspace_bytes,
                                      dgppo_reduce_desc* pending, void* stream) {
  DGPPO_REQUIRE(M >= 0 && lddx >= FZ_H && ldx >= FZ_H && (relu_mask == nullptr || ldm >= FZ_H) && ldw2 >= FZ_H && ldw1 >= FZ_H,
                "mlp_gi_bwd_w: bad shape M=%d lddx=%d ldx=%d ldm=%d ldw2=%d ldw1=%d", M, lddx, ldx, ldm, ldw2, ldw1);
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "mlp_gi_bwd_w: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "mlp_gi_bwd_w: workspace must be 16-byte aligned");
  if (pending) pending[0].pending = pending[1].pending = 0;
  if (M == 0) return 0;                            // (the row operands of an empty call may be NULL)
  DGPPO_REQUIRE(dgi && Wi && W2 && W1 && g2 && g1 && p2 && y2 && st2 && p1 && y1 && st1 && x && dx && dg2 && db2 && dg1 && db1 &&
                dW2 && dbias2 && dW1 && dbias1, "mlp_gi_bwd_w: NULL operand");
  const long max_slabs = (long)(workspace_bytes / (sizeof(float) * TW_SLAB));
  int grid;
  float* ws;
  if (mlp_gi_bwd_rw_selected(dgi, M)) {
    grid = mlp_gi_bwd_rw_grid(M);
    ws = (grid > 4 && max_slabs >= grid) ? workspace : nullptr;
    MlpGiBwdArgs a{dgi, M, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, relu_mask, ldm, dpre2, dpre1, dx, lddx, dg2, db2, dg1, db1,
                   x, ldx, ws, dW2, ldw2, dbias2, dW1, ldw1, dbias1};
    const int32_t rc = mlp_gi_bwd_rw_launch<true>(a, grid, (hipStream_t)stream);
    if (rc != 0) return rc;
  } else {
    constexpr size_t smem = mlp_gi_bwd_smem<true>();
    const int tiles = (M + 16 * FZ_BWD_RT - 1) / (16 * FZ_BWD_RT);
    grid = mlp_gi_bwd_cap<true>(smem);
    if (grid > tiles / TW_MIN_TILES) grid = tiles / TW_MIN_TILES;
    ws = (grid > 4 && max_slabs >= 8) ? workspace : nullptr;
    if (ws && grid > max_slabs) grid = (int)max_slabs;
    if (!ws) grid = tiles < 4 ? tiles : 4;
    MlpGiBwdArgs a{dgi, M, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, relu_mask, ldm, dpre2, dpre1, dx, lddx, dg2, db2, dg1, db1,
                   x, ldx, ws, dW2, ldw2, dbias2, dW1, ldw1, dbias1};
    hipLaunchKernelGGL(mlp_gi_bwd_kernel<true>, dim3(grid), dim3(256), smem, (hipStream_t)stream, a);
    DGPPO_LAUNCH_CHECK();
  }
  if (!ws) return 0;
  dgppo_reduce_desc d[2];
  d[0] = dgppo_reduce_desc{ws, dW2, dbias2, TW_SLAB, grid, ldw2, FZ_H, FZ_H, 1};
  d[1] = dgppo_reduce_desc{ws + TW_HALF, dW1, dbias1, TW_SLAB, grid, ldw1, FZ_H, FZ_H, 1};
  if (pending) {
    pending[0] = d[0]; pending[1] = d[1];
    return 0;
  }
  return dgppo_dense_bwd_w_reduce_batch(d, 2, stream);
}

extern "C" int32_t dgppo_mlp_gi_fwd(const float* X, int32_t ldx, const float* W1, const float* b1, const float* g1,
                                    const float* be1, const float* W2, const float* b2, const float* g2, const float* be2,
                                    const float* Wi, const float* bi, float* p1, float* y1, float* st1, float* p2, float* y2,
                                    float* st2, float* gi, int32_t M, void* stream) {
  DGPPO_REQUIRE(M >= 0 && ldx >= FZ_H, "mlp_gi_fwd: bad shape M=%d ldx=%d", M, ldx);
  DGPPO_REQUIRE(X && W1 && b1 && g1 && be1 && W2 && b2 && g2 && be2 && Wi && bi, "mlp_gi_fwd: NULL operand");
  // gi == NULL: the trunk alone, y2 is the result (dgppo_gi_gru1_head_fwd forms the gate inputs from it); then y2 may be given
  // without the other saves
  const bool save = p1 || y1 || st1 || p2 || st2 || (gi && y2);
  DGPPO_REQUIRE(!save || (p1 && y1 && st1 && p2 && y2 && st2), "mlp_gi_fwd: the saved activations are all-or-none");
  DGPPO_REQUIRE(gi || y2, "mlp_gi_fwd: neither gi nor y2 to write");
  const bool rw = (ldx & 3) == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(W1) |
                                      reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(Wi)) & 15) == 0;
  DGPPO_REQUIRE(gi || (rw && (reinterpret_cast<uintptr_t>(y2) & 15) == 0),
                "mlp_gi_fwd: gi == NULL needs 16-byte aligned X, W1, W2, Wi, y2 and ldx a multiple of 4");
  if (M == 0) return 0;
  MlpGiArgs a{X, ldx, M, W1, b1, g1, be1, W2, b2, g2, be2, Wi, bi, p1, y1, st1, p2, y2, st2, gi};
  // rows per wave, weights in LDS (one 16-wave workgroup per CU): needs 16-byte addressable input rows
  if (rw) {
    static thread_local int cus = 0;
    if (cus == 0) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    }
    const size_t smem_rw = sizeof(float) * (2 * 64 * RW_WL + 64 * RW_WIL + 576 + RW_WAVES * 16 * RW_YL);
    static thread_local bool attr = false;
    if (!attr) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_gi_fwd_rw_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_rw);
      DGPPO_REQUIRE(e == hipSuccess, "mlp_gi_fwd: cannot reserve %zu bytes of LDS per workgroup: %s", smem_rw, hipGetErrorString(e));
      attr = true;
    }
    const int tiles16 = (M + 15) / 16;            // spread over every CU even when there are fewer tiles than wave slots
    hipLaunchKernelGGL(mlp_gi_fwd_rw_kernel, dim3(tiles16 < cus ? tiles16 : cus), dim3(64 * RW_WAVES), smem_rw, (hipStream_t)stream, a);
    DGPPO_LAUNCH_CHECK();
    return 0;
  }
  const size_t smem = sizeof(float) * (3 * FZ_RB * FZ_HL + FZ_RB * 8);
  static thread_local int cap = 0;
  if (cap == 0) {
    int per_cu = 0, dev = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&mlp_gi_fwd_kernel), 256, smem) !=
            hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    cap = per_cu * cus;
  }
  const int tiles = (M + FZ_RB - 1) / FZ_RB;
  hipLaunchKernelGGL(mlp_gi_fwd_kernel, dim3(tiles < cap ? tiles : cap), dim3(256), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// One GRU step (T = 1) + the output Dense layer(s) on the same rows: the tail of PPOPolicy.get_action / ValueNet.get_value
// in a rollout step (dgppo/nn/rnn.py:14-30 -> dgppo/algo/module/policy.py:62-74 [PolicyNet head Dense(64) -> TanhNormal
// Dense(4)], value.py:41,76 [Dense(n_out)]).
//   h' = GRU(gi, h0)      gi = x Wi + bi precomputed (mlp_gi_fwd_kernel),  r|z|n gate order, flax GRUCell
//   TWO = true :  u = h' W1 + b1  [64]   out = u W2 + b2   [n_out <= 16]       (policy)
//   TWO = false:  out = h' W1 + b1  [n_out <= 16]                               (value nets)
// Persistent 32-row tiles; Wh (48) + W1 (16) + W2 (16) k-step fragments stay in registers; h0 / h' / u tiles in LDS.
// ---------------------------------------------------------------------------------------------------------------------
struct GruHeadArgs {
  const float *gi, *Wh, *bhn, *h0;        // gi [M,192], Wh [64,192], bhn [64], h0 [M,64] or NULL (zeros)
  const float *W1, *b1, *W2, *b2;         // TWO: W1 [64,64], W2 [64,n_out];  else W1 [64,n_out], W2 unused
  float *hs, *hprev, *gates, *u, *out;    // hs [M,64]; hprev [M,64] / gates [M,256] / u [M,64] saved for training or NULL
  int M, n_out;
};
// (gate_sigmoid / gate_tanh: nn_gru.h)

template <bool TWO>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) gru1_head_fwd_kernel(GruHeadArgs a) {
  extern __shared__ float sm[];
  float* s_h = sm;                          // [RB][HL] h0 rows
  float* s_n = s_h + FZ_RB * FZ_HL;         // [RB][HL] h' rows
  float* s_u = s_n + FZ_RB * FZ_HL;         // [RB][HL] u rows (TWO)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int c = w * 16 + li;
  float wh[16][3], w1[16], w2[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int k = kk * 4 + lq;
#pragma unroll
    for (int t = 0; t < 3; ++t) wh[kk][t] = a.Wh[k * 192 + t * 64 + c];
    if (TWO) {
      w1[kk] = a.W1[k * FZ_H + c];
      w2[kk] = (li < a.n_out) ? a.W2[k * a.n_out + li] : 0.0f;      // single column tile: identical in every wave
    } else {
      w1[kk] = (li < a.n_out) ? a.W1[k * a.n_out + li] : 0.0f;
      w2[kk] = 0.0f;
    }
  }
  const float bn = a.bhn[c];
  const float b1 = TWO ? a.b1[c] : ((li < a.n_out) ? a.b1[li] : 0.0f);
  const float b2 = (TWO && li < a.n_out) ? a.b2[li] : 0.0f;
  const int n_tiles = (a.M + FZ_RB - 1) / FZ_RB;
  float hpf[2][4];
  auto fetch_h0 = [&](int tile) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, r = idx >> 4, q = idx & 15;
      int row = tile * FZ_RB + r;
      row = row < a.M ? row : a.M - 1;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.h0 != nullptr) v = reinterpret_cast<const float4*>(a.h0 + (size_t)row * FZ_H)[q];
      hpf[u][0] = v.x; hpf[u][1] = v.y; hpf[u][2] = v.z; hpf[u][3] = v.w;
    }
  };
  auto commit_h0 = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, r = idx >> 4, q = idx & 15;
      float* d = s_h + r * FZ_HL + 4 * q;
      d[0] = hpf[u][0]; d[1] = hpf[u][1]; d[2] = hpf[u][2]; d[3] = hpf[u][3];
    }
  };
  int tile = blockIdx.x;
  if (tile < n_tiles) { fetch_h0(tile); commit_h0(); }
  __syncthreads();
  for (; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * FZ_RB;
    const int nxt = tile + gridDim.x;
    const bool more = nxt < n_tiles;
    // gate inputs of this tile and the next tile's h0 rows: requested before the MFMAs
    float g[2][4][3];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + rt * 16 + lq * 4 + r;
        row = row < a.M ? row : a.M - 1;
        const float* gp = a.gi + (size_t)row * 192 + c;
        g[rt][r][0] = gp[0]; g[rt][r][1] = gp[64]; g[rt][r][2] = gp[128];
      }
    if (more) fetch_h0(nxt);
    __builtin_amdgcn_sched_barrier(0);
    float areg[2][16];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_h[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[2][3];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], wh[kk][t], acc[rt][t], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = rt * 16 + lq * 4 + r, row = row0 + rl;
        const float hp = s_h[rl * FZ_HL + c];
        const float rg = gate_sigmoid(g[rt][r][0] + acc[rt][0][r]);
        const float zg = gate_sigmoid(g[rt][r][1] + acc[rt][1][r]);
        const float hn = acc[rt][2][r] + bn;
        const float ng = gate_tanh(g[rt][r][2] + rg * hn);
        const float hnew = (1.0f - zg) * ng + zg * hp;
        s_n[rl * FZ_HL + c] = hnew;
        if (row < a.M) {
          a.hs[(size_t)row * FZ_H + c] = hnew;
          if (a.hprev != nullptr) a.hprev[(size_t)row * FZ_H + c] = hp;
          if (a.gates != nullptr) {
            float* gs = a.gates + (size_t)row * 256;
            gs[c] = rg; gs[64 + c] = zg; gs[128 + c] = ng; gs[192 + c] = hn;
          }
        }
      }
    FZ_LDS_BARRIER();                     // h' complete; every read of s_h is done
    if (more) commit_h0();
    // ---- first Dense on h' ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) areg[rt][kk] = s_n[(rt * 16 + li) * FZ_HL + kk * 4 + lq];
    __builtin_amdgcn_sched_barrier(0);
    if (TWO) {
      f32x4 au[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) au[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rt][kk], w1[kk], au[rt], 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = rt * 16 + lq * 4 + r, row = row0 + rl;
          const float uv = au[rt][r] + b1;
          s_u[rl * FZ_HL + c] = uv;
          if (a.u != nullptr && row < a.M) a.u[(size_t)row * FZ_H + c] = uv;
        }
      FZ_LDS_BARRIER();
      // ---- second Dense: one column tile, row tile w (waves 0 and 1) ----
      if (w < 2) {
        float ar[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) ar[kk] = s_u[(w * 16 + li) * FZ_HL + kk * 4 + lq];
        f32x4 ao = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) ao = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[kk], w2[kk], ao, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + w * 16 + lq * 4 + r;
          if (row < a.M && li < a.n_out) a.out[(size_t)row * a.n_out + li] = ao[r] + b2;
        }
      }
    } else if (w < 2) {
      f32x4 ao = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) ao = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[w][kk], w1[kk], ao, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + w * 16 + lq * 4 + r;
        if (row < a.M && li < a.n_out) a.out[(size_t)row * a.n_out + li] = ao[r] + b1;
      }
    }
    FZ_LDS_BARRIER();                     // next tile's h0 committed; s_n / s_u free again
  }
}

// ---- the same step with rows per WAVE and the weights in LDS (inference form: nothing saved for a backward) -----------------
// As mlp_gi_fwd_rw_kernel: a wave carries 16 rows through the GRU step and the head; Wh (48 KB), W1 and W2 sit in LDS once per CU,
// shared by the 16 waves of the one workgroup; h' and u change from the C/D layout to the A layout through a wave-private LDS
// tile; no barrier after the staging.  The rollout step (32 768 rows) took 19 us with the tiled kernel above (two workgroup
// barriers per 32-row tile, 212 VGPRs: two workgroups per CU) for 9 us of matrix-core work.
#define RWH_W1L 65
template <bool TWO>
__global__ void __launch_bounds__(64 * RW_WAVES) gru1_head_fwd_rw_kernel(GruHeadArgs a) {
  extern __shared__ float sm[];
  float* sWh = sm;                                // [64][193]
  float* sW1 = sWh + 64 * RW_WIL;                 // TWO: [64][65] (64 columns); else [64][17] in the same stride-65 rows (16 columns)
  float* sW2 = sW1 + 64 * RWH_W1L;                // TWO: [64][17]
  float* sB = sW2 + 64 * 17;                      // bhn (64), b1 (64), b2 (16)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  float* sY = sB + 144 + w * (16 * RW_YL);
  {
    static_assert(RW_WAVES == 16, "the staging below assumes 1024 threads");
    float4 vh[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) vh[j] = reinterpret_cast<const float4*>(a.Wh)[j * 1024 + tid];
    float w1v[4] = {0.f, 0.f, 0.f, 0.f};
    float w2v = 0.0f;
    if (TWO) {
      const float4 v = reinterpret_cast<const float4*>(a.W1)[tid];          // [64][64]
      w1v[0] = v.x; w1v[1] = v.y; w1v[2] = v.z; w1v[3] = v.w;
      { const int k = tid >> 4, c = tid & 15; w2v = (c < a.n_out) ? a.W2[k * a.n_out + c] : 0.0f; }
    } else {
      const int k = tid >> 4, c = tid & 15;
      w1v[0] = (c < a.n_out) ? a.W1[k * a.n_out + c] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int q = j * 1024 + tid, k = q / 48, c = (q - k * 48) * 4;
      float* d = sWh + k * RW_WIL + c;
      d[0] = vh[j].x; d[1] = vh[j].y; d[2] = vh[j].z; d[3] = vh[j].w;
    }
    if (TWO) {
      const int k = tid >> 4, c = (tid & 15) * 4;
      float* d = sW1 + k * RWH_W1L + c;
      d[0] = w1v[0]; d[1] = w1v[1]; d[2] = w1v[2]; d[3] = w1v[3];
      sW2[(tid >> 4) * 17 + (tid & 15)] = w2v;
    } else {
      sW1[(tid >> 4) * RWH_W1L + (tid & 15)] = w1v[0];
    }
    if (tid < 64) { sB[tid] = a.bhn[tid]; sB[64 + tid] = TWO ? a.b1[tid] : ((tid < a.n_out) ? a.b1[tid] : 0.0f); }
    if (tid < 16) sB[128 + tid] = (TWO && tid < a.n_out) ? a.b2[tid] : 0.0f;
  }
  __syncthreads();
  const int n_tiles = (a.M + 15) >> 4;
  for (int tile = w * gridDim.x + blockIdx.x; tile < n_tiles; tile += gridDim.x * RW_WAVES) {
    const int row0 = tile * 16;
    // A operand: h0 row li, columns lq * 16 .. + 15 (zeros without h0); the same rows again in the C/D layout for the update
    float A[16];
    {
      int row = row0 + li;
      row = row < a.M ? row : a.M - 1;
      if (a.h0 != nullptr) {
        const float4* p = reinterpret_cast<const float4*>(a.h0 + (size_t)row * FZ_H + lq * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float4 v = p[j]; A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w; }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) A[j] = 0.0f;
      }
    }
    float hp[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + lq * 4 + r;
        row = row < a.M ? row : a.M - 1;
        hp[ct][r] = (a.h0 != nullptr) ? a.h0[(size_t)row * FZ_H + ct * 16 + li] : 0.0f;
      }
    // hidden column group ct (16 columns): r, z, n gate tiles ct, ct + 4, ct + 8 of gh = h0 Wh, seeded with the input projection gi
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 ar, az, an = f32x4{0.f, 0.f, 0.f, 0.f};
      float gn[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + lq * 4 + r;
        row = row < a.M ? row : a.M - 1;
        const float* gp = a.gi + (size_t)row * 192 + ct * 16 + li;
        ar[r] = gp[0]; az[r] = gp[64]; gn[r] = gp[128];
      }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const float* wr = sWh + (lq * 16 + kk) * RW_WIL + ct * 16 + li;
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], wr[0], ar, 0, 0, 0);
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], wr[64], az, 0, 0, 0);
        an = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], wr[128], an, 0, 0, 0);
      }
      const float bn = sB[ct * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rg = gate_sigmoid(ar[r]);
        const float zg = gate_sigmoid(az[r]);
        const float ng = gate_tanh(gn[r] + rg * (an[r] + bn));
        const float hnew = (1.0f - zg) * ng + zg * hp[ct][r];
        sY[(lq * 4 + r) * RW_YL + ct * 16 + li] = hnew;
        const int row = row0 + lq * 4 + r;
        if (row < a.M) a.hs[(size_t)row * FZ_H + ct * 16 + li] = hnew;
      }
    }
    // h' as the next A operand
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(sY + li * RW_YL + lq * 16 + 4 * j);
      A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w;
    }
    if (TWO) {
      f32x4 au[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) au[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const float* wr = sW1 + (lq * 16 + kk) * RWH_W1L + li;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) au[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], wr[ct * 16], au[ct], 0, 0, 0);
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float b = sB[64 + ct * 16 + li];
#pragma unroll
        for (int r = 0; r < 4; ++r) sY[(lq * 4 + r) * RW_YL + ct * 16 + li] = au[ct][r] + b;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(sY + li * RW_YL + lq * 16 + 4 * j);
        A[4 * j] = v.x; A[4 * j + 1] = v.y; A[4 * j + 2] = v.z; A[4 * j + 3] = v.w;
      }
    }
    {
      f32x4 ao = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* sWo = TWO ? sW2 : sW1;
      const int ld = TWO ? 17 : RWH_W1L;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) ao = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], sWo[(lq * 16 + kk) * ld + li], ao, 0, 0, 0);
      const float b = TWO ? sB[128 + li] : sB[64 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + lq * 4 + r;
        if (row < a.M && li < a.n_out) a.out[(size_t)row * a.n_out + li] = ao[r] + b;
      }
    }
  }
}

extern "C" int32_t dgppo_gru1_head_fwd(const float* gi, const float* Wh, const float* bhn, const float* h0, const float* W1,
                                       const float* b1, const float* W2, const float* b2, float* hs, float* hprev,
                                       float* gates, float* u, float* out, int32_t M, int32_t n_out, void* stream) {
  DGPPO_REQUIRE(M >= 0 && n_out >= 1 && n_out <= 16, "gru1_head_fwd: bad shape M=%d n_out=%d", M, n_out);
  DGPPO_REQUIRE(gi && Wh && bhn && W1 && b1 && hs && out, "gru1_head_fwd: NULL operand");
  const bool two = W2 != nullptr;
  DGPPO_REQUIRE(!two || b2, "gru1_head_fwd: W2 without b2");
  DGPPO_REQUIRE(two || !u, "gru1_head_fwd: u is only produced by the two-layer head");
  if (M == 0) return 0;
  GruHeadArgs a{gi, Wh, bhn, h0, W1, b1, W2, b2, hs, hprev, gates, u, out, M, n_out};
  // inference (nothing saved): rows per wave, weights in LDS
  if (!hprev && !gates && !u && ((reinterpret_cast<uintptr_t>(Wh) | reinterpret_cast<uintptr_t>(W1) | reinterpret_cast<uintptr_t>(h0)) & 15) == 0) {
    static thread_local int cus = 0;
    if (cus == 0) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    }
    const size_t smem_rw = sizeof(float) * (64 * RW_WIL + 64 * RWH_W1L + 64 * 17 + 144 + RW_WAVES * 16 * RW_YL);
    static thread_local bool attr[2] = {false, false};
    if (!attr[two]) {
      const void* f = two ? reinterpret_cast<const void*>(&gru1_head_fwd_rw_kernel<true>)
                          : reinterpret_cast<const void*>(&gru1_head_fwd_rw_kernel<false>);
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_rw);
      DGPPO_REQUIRE(e == hipSuccess, "gru1_head_fwd: cannot reserve %zu bytes of LDS per workgroup: %s", smem_rw, hipGetErrorString(e));
      attr[two] = true;
    }
    const int tiles16 = (M + 15) / 16, grid_rw = tiles16 < cus ? tiles16 : cus;
    if (two) hipLaunchKernelGGL(gru1_head_fwd_rw_kernel<true>, dim3(grid_rw), dim3(64 * RW_WAVES), smem_rw, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gru1_head_fwd_rw_kernel<false>, dim3(grid_rw), dim3(64 * RW_WAVES), smem_rw, (hipStream_t)stream, a);
    DGPPO_LAUNCH_CHECK();
    return 0;
  }
  const size_t smem = sizeof(float) * 3 * FZ_RB * FZ_HL;
  const void* fn = two ? reinterpret_cast<const void*>(&gru1_head_fwd_kernel<true>)
                       : reinterpret_cast<const void*>(&gru1_head_fwd_kernel<false>);
  static thread_local int cap[2] = {0, 0};
  if (cap[two] == 0) {
    int per_cu = 0, dev = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, smem) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    cap[two] = per_cu * cus;
  }
  const int tiles = (M + FZ_RB - 1) / FZ_RB;
  const int grid = tiles < cap[two] ? tiles : cap[two];
  if (two) hipLaunchKernelGGL(gru1_head_fwd_kernel<true>, dim3(grid), dim3(256), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(gru1_head_fwd_kernel<false>, dim3(grid), dim3(256), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- gate projection + one GRU step + value head, rows per WAVE: the tail of the constraint-value net's T = 1 passes --------------
//   gi = y2 Wi + bi  (never leaves registers),  h' = GRU(gi, h0),  out = h' W1 + b1  [n_out <= 16]
// (flax GRUCell, dgppo/nn/rnn.py:14-30, and the value Dense, dgppo/algo/module/value.py:41,76, on the rows of one step.)
// It replaces the gate projection of mlp_gi_fwd_rw_kernel, gru_fwd_kernel at T = 1 and the head's dense_fwd_kernel, and with them
// the 768-byte gi row written once and read once, and (inference) the hs row nobody reads.  With T = 1 the step is row-local, so a
// WAVE owns 16 rows from y2 to out as in gru1_head_fwd_rw_kernel; no barrier after the weights are staged.
// LDS: Wi and Wh [64][193] (98 816 B), W1 [64][17] (4 352 B), biases (1 088 B), one 16 x 68 tile per wave (4 352 B): 12 waves
// = 156 480 B of the 160 KB (16 waves would need 173 888 B); one workgroup per CU, three waves per SIMD (<= 170 VGPRs).
// Arithmetic, so that hs and gates keep the bits of the launches replaced:
//   gi : summed from zero in the permuted k order of mlp_gi_fwd_rw_kernel (a lane's 16 k-values are 16 consecutive columns of its
//        y2 row; step j of lane group lq contracts k = lq * 16 + j), then + bi;
//   gh : summed from zero in the natural k order of gru_fwd_kernel (step kk contracts k = kk * 4 + lq).  The A fragments of that
//        order come from the wave's tile (h0 rows written row-major, read back one float per step); Wh is staged with its rows
//        permuted (row k at (k & 3) * 16 + (k >> 2)) so that both B fragments are read at [lq * 16 + step]: 64 different banks;
//   gates: gru_gate_fwd (nn_gru.h).
// The tile then holds h0 in the C/D layout for the update, which puts h' in its place (same lane, same element), and h' goes back
// out as the head's A operand and as 16-byte stores of hs.
// Every row operand of tile t + 1 is requested before tile t computes; with ids, the id of tile t + 2 as well.
#define GG_WAVES 12
#define GG_W1L 17
#define GG_BIAS 272                                 // bi (192) | bhn (64) | b1 (16)
#define GG_LDS_FLOATS (2 * 64 * RW_WIL + 64 * GG_W1L + GG_BIAS + GG_WAVES * 16 * RW_YL)
static_assert(GG_LDS_FLOATS * sizeof(float) <= 160 * 1024, "gi_gru1_head_fwd_kernel: LDS");
struct GiGruHeadArgs {
  const float *y2, *Wi, *bi, *Wh, *bhn, *W1, *b1;   // y2 [M,64], Wi / Wh [64,192], bi [192], bhn [64], W1 [64,n_out], b1 [n_out]
  const float* h0;                                  // NULL (zeros), dense [M,64], blocked (h0_rpb > 0) or mapped (h0_map.n_inner.d > 0)
  float *out, *hs, *gates;                          // out [M, ldo]; hs [M,64] / gates [M,256] or NULL
  int M, n_out, ldo;
  int h0_rpb;
  long h0_bstride;
  GruH0Map h0_map;
  bool big_tiles;                                   // gru_fwd_big_tiles(M): the rounding of h' gru_fwd_kernel has at this row count
};

__global__ void __launch_bounds__(64 * GG_WAVES) gi_gru1_head_fwd_kernel(GiGruHeadArgs a) {
  extern __shared__ float sm[];
  float* sWi = sm;                                  // [64][193]
  float* sWh = sWi + 64 * RW_WIL;                   // [64][193], rows permuted
  float* sW1 = sWh + 64 * RW_WIL;                   // [64][17], columns >= n_out zero
  float* sB = sW1 + 64 * GG_W1L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  float* sT = sB + GG_BIAS + w * (16 * RW_YL);      // wave-private tile
  {   // 96 KB of weights: eight 16-byte loads per thread, all requested before the first LDS write
    static_assert(GG_WAVES == 12, "the staging below assumes 768 threads");
    float4 vi[4], vh[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vi[j] = reinterpret_cast<const float4*>(a.Wi)[j * 768 + tid];
      vh[j] = reinterpret_cast<const float4*>(a.Wh)[j * 768 + tid];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = j * 768 + tid, k = q / 48, c = (q - k * 48) * 4;
      float* di = sWi + k * RW_WIL + c;
      float* dh = sWh + ((k & 3) * 16 + (k >> 2)) * RW_WIL + c;
      di[0] = vi[j].x; di[1] = vi[j].y; di[2] = vi[j].z; di[3] = vi[j].w;
      dh[0] = vh[j].x; dh[1] = vh[j].y; dh[2] = vh[j].z; dh[3] = vh[j].w;
    }
    for (int i = tid; i < 64 * 16; i += 64 * GG_WAVES) {
      const int k = i >> 4, c = i & 15;
      sW1[k * GG_W1L + c] = (c < a.n_out) ? a.W1[k * a.n_out + c] : 0.0f;
    }
    if (tid < 192) sB[tid] = a.bi[tid];
    if (tid < 64) sB[192 + tid] = a.bhn[tid];
    if (tid < 16) sB[256 + tid] = (tid < a.n_out) ? a.b1[tid] : 0.0f;
  }
  __syncthreads();
  const int n_tiles = (a.M + 15) >> 4, step = gridDim.x * GG_WAVES;
  const bool has_h0 = a.h0 != nullptr, mapped = has_h0 && a.h0_map.n_inner.d > 0, by_id = mapped && a.h0_map.ids != nullptr;
  auto seq_of = [&](int tile) {                     // this lane's row of the tile in the A layout, clamped for loads
    const int s = tile * 16 + li;
    return s < a.M ? s : a.M - 1;
  };
  auto request_id = [&](int tile) { return a.h0_map.ids[gru_h0_map_cell(a.h0_map, seq_of(tile)).e]; };
  float nY[16], nH[16];                             // the next tile's y2 and h0 rows: row li, columns lq * 16 .. + 15
  auto request = [&](int tile, int id) {
    const int s = seq_of(tile);
    const float4* py = reinterpret_cast<const float4*>(a.y2 + (size_t)s * FZ_H + lq * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float4 v = py[j]; nY[4 * j] = v.x; nY[4 * j + 1] = v.y; nY[4 * j + 2] = v.z; nY[4 * j + 3] = v.w; }
    if (has_h0) {
      const float* hp = a.h0 + (size_t)s * FZ_H;
      if (mapped) {
        const GruH0Cell cell = gru_h0_map_cell(a.h0_map, s);
        hp = gru_h0_map_cell_row(a.h0, a.h0_map, cell, by_id ? (long)id : (long)cell.e);
      } else if (a.h0_rpb > 0) {
        const int b = s / a.h0_rpb;
        hp = a.h0 + (size_t)b * a.h0_bstride + (size_t)(s - b * a.h0_rpb) * FZ_H;
      }
      const float4* ph = reinterpret_cast<const float4*>(hp + lq * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float4 v = ph[j]; nH[4 * j] = v.x; nH[4 * j + 1] = v.y; nH[4 * j + 2] = v.z; nH[4 * j + 3] = v.w; }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) nH[j] = 0.0f;
    }
  };
  int tile = w * gridDim.x + blockIdx.x;            // consecutive tiles on different CUs
  int id_n = 0;                                     // with ids: the env of the NEXT request's row
  if (tile < n_tiles) {
    if (by_id) id_n = request_id(tile);
    request(tile, id_n);
    if (by_id && tile + step < n_tiles) id_n = request_id(tile + step);
  }
  for (; tile < n_tiles; tile += step) {
    const int row0 = tile * 16, nxt = tile + step;
    float Y[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) Y[j] = nY[j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(sT + li * RW_YL + lq * 16 + 4 * j) = make_float4(nH[4 * j], nH[4 * j + 1], nH[4 * j + 2], nH[4 * j + 3]);
    if (nxt < n_tiles) {
      request(nxt, id_n);
      if (by_id && nxt + step < n_tiles) id_n = request_id(nxt + step);
    }
    __builtin_amdgcn_sched_barrier(0);
    float Hk[16];                                   // h0 in the A layout of the natural k order
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) Hk[kk] = sT[li * RW_YL + kk * 4 + lq];
    // hidden column group ct: gate tiles ct, ct + 4, ct + 8 of gi and of gh, 96 MFMAs
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 gi[3], gh[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) { gi[t] = f32x4{0.f, 0.f, 0.f, 0.f}; gh[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      float bq[2][2][6];                            // two k-steps per group, double-buffered (see mlp_gi_fwd_rw_kernel)
      auto ldb = [&](int buf, int g) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int o = (lq * 16 + g * 2 + kk) * RW_WIL + ct * 16 + li;
#pragma unroll
          for (int t = 0; t < 3; ++t) { bq[buf][kk][t] = sWi[o + t * 64]; bq[buf][kk][3 + t] = sWh[o + t * 64]; }
        }
      };
      ldb(0, 0);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (g + 1 < 8) ldb((g + 1) & 1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            gi[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Y[g * 2 + kk], bq[g & 1][kk][t], gi[t], 0, 0, 0);
            gh[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Hk[g * 2 + kk], bq[g & 1][kk][3 + t], gh[t], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      const int col = ct * 16 + li;
      const float bir = sB[col], biz = sB[64 + col], bin = sB[128 + col], bn = sB[192 + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* tp = sT + (lq * 4 + r) * RW_YL + col;
        const GruGateFwd gg = gru_gate_fwd(gi[0][r] + bir, gi[1][r] + biz, gi[2][r] + bin, gh[0][r], gh[1][r], gh[2][r], bn, *tp, a.big_tiles);
        *tp = gg.h;
        const int row = row0 + lq * 4 + r;
        if (a.gates != nullptr && row < a.M) {
          float* gs = a.gates + (size_t)row * 256 + col;
          gs[0] = gg.r; gs[64] = gg.z; gs[128] = gg.n; gs[192] = gg.hn;
        }
      }
    }
    // h' as the head's A operand (permuted contraction) and, 16 bytes per lane, as hs
    float Hn[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(sT + li * RW_YL + lq * 16 + 4 * j);
      Hn[4 * j] = v.x; Hn[4 * j + 1] = v.y; Hn[4 * j + 2] = v.z; Hn[4 * j + 3] = v.w;
      if (a.hs != nullptr && row0 + li < a.M) reinterpret_cast<float4*>(a.hs + (size_t)(row0 + li) * FZ_H + lq * 16)[j] = v;
    }
    f32x4 ao = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) ao = __builtin_amdgcn_mfma_f32_16x16x4f32(Hn[kk], sW1[(lq * 16 + kk) * GG_W1L + li], ao, 0, 0, 0);
    const float b = sB[256 + li];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + lq * 4 + r;
      if (row < a.M && li < a.n_out) a.out[(size_t)row * a.ldo + li] = ao[r] + b;
    }
  }
}

extern "C" int32_t dgppo_gi_gru1_head_fwd(const float* y2, const float* Wi, const float* bi, const float* Wh, const float* bhn,
                                          const float* W1, const float* b1, const float* h0, int32_t h0_form,
                                          int32_t h0_rows_per_block, int64_t h0_block_stride, const int32_t* ids, int32_t n_env,
                                          int32_t n_time, int32_t n_inner, int64_t env_stride, int64_t time_stride, float* out,
                                          int32_t ldo, float* hs, float* gates, int32_t M, int32_t n_out, void* stream) {
  DGPPO_REQUIRE(M >= 0 && n_out >= 1 && n_out <= 16 && ldo >= n_out, "gi_gru1_head_fwd: bad shape M=%d n_out=%d ldo=%d", M, n_out, ldo);
  DGPPO_REQUIRE(y2 && Wi && bi && Wh && bhn && W1 && b1 && out, "gi_gru1_head_fwd: NULL operand");
  DGPPO_REQUIRE(((reinterpret_cast<uintptr_t>(y2) | reinterpret_cast<uintptr_t>(Wi) | reinterpret_cast<uintptr_t>(Wh) |
                  reinterpret_cast<uintptr_t>(hs) | reinterpret_cast<uintptr_t>(h0)) & 15) == 0,
                "gi_gru1_head_fwd: y2, Wi, Wh, h0 and hs must be 16-byte aligned");
  GiGruHeadArgs a{};
  a.y2 = y2; a.Wi = Wi; a.bi = bi; a.Wh = Wh; a.bhn = bhn; a.W1 = W1; a.b1 = b1; a.h0 = h0;
  a.out = out; a.hs = hs; a.gates = gates; a.M = M; a.n_out = n_out; a.ldo = ldo;
  a.big_tiles = gru_fwd_big_tiles(M);
  if (h0_form == DGPPO_H0_BLOCKS) {
    DGPPO_REQUIRE(h0 != nullptr, "gi_gru1_head_fwd: blocked h0 is NULL");
    DGPPO_REQUIRE(h0_rows_per_block >= 1, "gi_gru1_head_fwd: rows_per_block must be >= 1 (got %d)", h0_rows_per_block);
    DGPPO_REQUIRE(h0_block_stride >= (int64_t)h0_rows_per_block * FZ_H && h0_block_stride % 4 == 0,
                  "gi_gru1_head_fwd: block_stride must be a multiple of 4 and >= rows_per_block * 64");
    a.h0_rpb = h0_rows_per_block; a.h0_bstride = (long)h0_block_stride;
  } else if (h0_form == DGPPO_H0_MAP) {
    DGPPO_REQUIRE(h0 != nullptr, "gi_gru1_head_fwd: mapped h0 is NULL");
    DGPPO_REQUIRE(n_env >= 1 && n_time >= 1 && n_inner >= 1, "gi_gru1_head_fwd: bad sizes n_env=%d n_time=%d n_inner=%d", n_env,
                  n_time, n_inner);
    DGPPO_REQUIRE(env_stride % 4 == 0 && time_stride % 4 == 0 && env_stride >= 0 && time_stride >= 0,
                  "gi_gru1_head_fwd: env_stride and time_stride must be non-negative multiples of 4 floats");
    DGPPO_REQUIRE((int64_t)M <= (int64_t)n_env * n_time * n_inner, "gi_gru1_head_fwd: the map holds fewer than M = %d carries", M);
    a.h0_map = gru_h0_map(ids, (long)env_stride, (long)time_stride, n_inner, n_time);
  } else {
    DGPPO_REQUIRE(h0_form == DGPPO_H0_DENSE, "gi_gru1_head_fwd: unknown h0 form %d", h0_form);
  }
  if (M == 0) return 0;
  static thread_local int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  }
  const size_t smem = sizeof(float) * GG_LDS_FLOATS;
  static thread_local bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gi_gru1_head_fwd_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    DGPPO_REQUIRE(e == hipSuccess, "gi_gru1_head_fwd: cannot reserve %zu bytes of LDS per workgroup: %s", smem, hipGetErrorString(e));
    attr = true;
  }
  const int tiles16 = (M + 15) / 16;
  hipLaunchKernelGGL(gi_gru1_head_fwd_kernel, dim3(tiles16 < cus ? tiles16 : cus), dim3(64 * GG_WAVES), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- backward of the output head in ONE pass over the rows ---------------------------------------------------------------------
//   two layers (policy: u = feat Ws + bs, out = u Wms + bms, dgppo/algo/module/policy.py:62-74):
//     dW2 += u^T dout, db2 += colsum dout, du = dout W2^T (never leaves the CU), dW1 += feat^T du, db1 += colsum du, dhs = du W1^T
//   one layer (values: out = feat Wo + bo, dgppo/algo/module/value.py:41,76):
//     dW1 += feat^T dout, db1 += colsum dout, dhs = dout W1^T
// It replaces dense_bwd_w, dense_smallk, dense_bwd_w, dense_fwd (two layers) or dense_bwd_w, dense_smallk (one) and the round trip
// of du.  One 8-wave workgroup per CU; every WAVE walks 16-row tiles of its own with a wave-private LDS image (feat | u | du rows),
// so there is no workgroup barrier in the loop; the next tile's rows are requested while the current one computes.  n_out <= 16:
// the narrow matrix is one zero-padded 16-wide column tile.  As in mlp_gi_bwd_kernel<true>, du in the C/D layout is the B operand
// of dW1 with the contraction rows permuted; dW2 contracts in natural row order (dout read from global memory in either layout:
// 16 x n_out floats per tile).  At the end the eight waves' accumulators meet in wave 0 through LDS (three halving rounds) and the
// workgroup writes ONE partial slab [narrow dW | its bias | pad | dW1 64x64 | db1] for the common second stage.
#define HB_HL 68                          // LDS row stride: 16-byte rows; A-fragment reads at most 2-way
#define HB_WAVES 8
#define HB_TILE (16 * HB_HL)
#define HB_BIG 1088                       // offset of [dW1 | db1] in a two-layer slab (>= 64 * 16 + 16, a multiple of 64)
#define HB_SLAB_ONE HB_BIG
#define HB_SLAB_TWO (HB_BIG + FZ_H * FZ_H + FZ_H)
struct HeadBwdArgs {
  const float* feat; int ldf;
  const float* u;                         // [M,64], two layers only
  const float* dout; int n_out;           // [M,n_out]
  const float *W1, *W2;                   // two layers: W1 [64,64], W2 [64,n_out]; one: W1 [64,n_out], W2 NULL
  float* dhs;                             // [M,64]
  float* dW1; int ldw1; float* db1;
  float* dW2; int ldw2; float* db2;
  float* part;                            // [grid][slab] or NULL: atomicAdd straight into the outputs
  int M;
};

template <bool TWO>
__global__ void __launch_bounds__(64 * HB_WAVES) head_bwd_kernel(HeadBwdArgs a) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  float* s_f = sm + w * 3 * HB_TILE;      // feat rows (zeros past M)
  float* s_u = s_f + HB_TILE;             // u rows
  float* s_du = s_u + HB_TILE;            // du rows
  const int n_out = a.n_out, ks = (n_out + 3) >> 2;
  const float* Wn = TWO ? a.W2 : a.W1;    // the narrow matrix [64, n_out]
  // B operand of dout Wn^T: B[k][n] = Wn[n][k]; lane (li, lq) holds k = 4 kk + lq of output column 16 t + li (zero-padded)
  float wn[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = kk * 4 + lq;
      wn[t][kk] = k < n_out ? Wn[(t * 16 + li) * n_out + k] : 0.0f;
    }
  // W1 (two layers) sits in LDS once per workgroup: B operand of du W1^T, B[k][n] = W1[n][k] read as s_w1[n][k]
  float* s_w1 = sm + HB_WAVES * 3 * HB_TILE;
  if constexpr (TWO) {
    for (int i = tid; i < FZ_H * FZ_H; i += 64 * HB_WAVES) s_w1[(i >> 6) * HB_HL + (i & 63)] = a.W1[i];   // (a parameter slice: any alignment)
    __syncthreads();
  }
  f32x4 an[4];                            // narrow dW rows 16 kt + 4 lq + r, column li
  f32x4 aw1[TWO ? 4 : 1][TWO ? 4 : 1];    // dW1 rows 16 kt + 4 lq + r, column 16 t + li
  float cs_n = 0.0f, cs_u[4] = {0.f, 0.f, 0.f, 0.f};   // column sums: dout column li (over this lane's rows), du column 16 t + li
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) an[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (TWO) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int t = 0; t < 4; ++t) aw1[kt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int n_tiles = (a.M + 15) >> 4, stride = gridDim.x * HB_WAVES;
  float4 pf[TWO ? 8 : 4];                 // the next tile's feat (and u) rows: 16 rows x 16 float4 each, 4 per lane
  auto fetch = [&](int tile) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int idx = s * 64 + lane, r = idx >> 4, q = idx & 15;
      int row = tile * 16 + r;
      row = row < a.M ? row : a.M - 1;
      pf[s] = *reinterpret_cast<const float4*>(a.feat + (size_t)row * a.ldf + 4 * q);
      if constexpr (TWO) pf[4 + s] = *reinterpret_cast<const float4*>(a.u + (size_t)row * FZ_H + 4 * q);
    }
  };
  auto commit = [&](int tile) {           // rows >= M become zeros
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int idx = s * 64 + lane, r = idx >> 4, q = idx & 15;
      const float m = tile * 16 + r < a.M ? 1.0f : 0.0f;
      auto pick = [&](const float4& v) { return make_float4(m != 0.f ? v.x : 0.f, m != 0.f ? v.y : 0.f, m != 0.f ? v.z : 0.f, m != 0.f ? v.w : 0.f); };
      *reinterpret_cast<float4*>(s_f + r * HB_HL + 4 * q) = pick(pf[s]);
      if constexpr (TWO) *reinterpret_cast<float4*>(s_u + r * HB_HL + 4 * q) = pick(pf[4 + s]);
    }
  };
  int tile = blockIdx.x * HB_WAVES + w;
  fetch(tile);                            // (rows are clamped: a fetch past the last tile reads row M - 1 and is never committed)
  for (; tile < n_tiles; tile += stride) {
    const int row0 = tile * 16;
    commit(tile);
    fetch(tile + stride);
    // dout in both operand layouts, zero outside [M, n_out]
    float a_d[4], b_d[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ra = row0 + li, ka = kk * 4 + lq;              // A[row li][k = 4 kk + lq]
      a_d[kk] = (ra < a.M && ka < n_out) ? a.dout[(size_t)ra * n_out + ka] : 0.0f;
      const int rb = row0 + kk * 4 + lq;                         // B[k = row 4 kk + lq][column li]
      b_d[kk] = (rb < a.M && li < n_out) ? a.dout[(size_t)rb * n_out + li] : 0.0f;
      cs_n += b_d[kk];
    }
    __builtin_amdgcn_sched_barrier(0);
    // g = dout Wn^T [16, 64]: du (two layers) or dhs (one)
    f32x4 g[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) g[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_d[0], wn[t][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    if (ks > 1) {                                                // wave-uniform: the k-steps beyond n_out are all zeros
#pragma unroll
      for (int kk = 1; kk < 4; ++kk)
#pragma unroll
        for (int t = 0; t < 4; ++t) g[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_d[kk], wn[t][kk], g[t], 0, 0, 0);
    }
    // narrow weight gradient: (u or feat)^T dout, contraction rows in natural order
    const float* s_a = TWO ? s_u : s_f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        an[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_a[(s * 4 + lq) * HB_HL + kt * 16 + li], b_d[s], an[kt], 0, 0, 0);
    if constexpr (TWO) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s_du[(lq * 4 + r) * HB_HL + t * 16 + li] = g[t][r];
          cs_u[t] += g[t][r];
        }
      // dW1 += feat^T du: step r contracts over rows {4 lq + r}, where this lane's du values are the B operand
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const float av = s_f[(lq * 4 + r) * HB_HL + kt * 16 + li];
#pragma unroll
          for (int t = 0; t < 4; ++t) aw1[kt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, g[t][r], aw1[kt][t], 0, 0, 0);
        }
      // dhs = du W1^T: du as the A operand from the wave's own LDS rows (written above by this wave: no barrier)
      float ad[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) ad[kk] = s_du[li * HB_HL + kk * 4 + lq];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        g[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          g[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[kk], s_w1[(t * 16 + li) * HB_HL + kk * 4 + lq], g[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + lq * 4 + r;
        if (row < a.M) a.dhs[(size_t)row * FZ_H + t * 16 + li] = g[t][r];
      }
    // (the next commit overwrites s_f / s_u / s_du of THIS wave only, after its own reads above)
  }
  // ---- the eight waves' accumulators meet in wave 0: three halving rounds through lane-major LDS images (slot j of lane l at
  // [j][l]: conflict-free, and the same lane of every wave holds the same element), then wave 0 writes the slab from registers
  constexpr int NV = TWO ? 85 : 17;       // values per lane: narrow dW 16, (dW1 64,) dout column sum 1, (du column sums 4)
  auto each = [&](auto&& f) {             // value = f(slot, value) over this lane's values, the same order in every wave
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) an[kt][r] = f(kt * 4 + r, an[kt][r]);
    cs_n = f(16, cs_n);
    if constexpr (TWO) {
#pragma unroll
      for (int t = 0; t < 4; ++t) cs_u[t] = f(17 + t, cs_u[t]);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) aw1[kt][t][r] = f(21 + (kt * 4 + t) * 4 + r, aw1[kt][t][r]);
    }
  };
  __syncthreads();                        // every wave is done with its tile images
#pragma unroll
  for (int half = HB_WAVES / 2; half >= 1; half >>= 1) {
    if (w >= half && w < 2 * half) each([&](int j, float v) { sm[((w - half) * NV + j) * 64 + lane] = v; return v; });
    __syncthreads();
    if (w < half) each([&](int j, float v) { return v + sm[(w * NV + j) * 64 + lane]; });
    __syncthreads();
  }
  if (w != 0) return;
  // column sums: add the four row groups (lanes li, li + 16, li + 32, li + 48)
  cs_n += __shfl_xor(cs_n, 16); cs_n += __shfl_xor(cs_n, 32);
  if constexpr (TWO) {
#pragma unroll
    for (int t = 0; t < 4; ++t) { cs_u[t] += __shfl_xor(cs_u[t], 16); cs_u[t] += __shfl_xor(cs_u[t], 32); }
  }
  constexpr int SLAB = TWO ? HB_SLAB_TWO : HB_SLAB_ONE;
  const int nb = FZ_H * n_out;            // the narrow dW is dense [64, n_out] in the slab, its bias follows
  float* slab = a.part ? a.part + (size_t)blockIdx.x * SLAB : nullptr;
  float* dWn = TWO ? a.dW2 : a.dW1;
  float* dbn = TWO ? a.db2 : a.db1;
  const int ldn = TWO ? a.ldw2 : a.ldw1;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int krow = kt * 16 + lq * 4 + r;
      if (li < n_out) {
        if (slab) slab[krow * n_out + li] = an[kt][r];
        else atomicAdd(dWn + (size_t)krow * ldn + li, an[kt][r]);
      }
      if constexpr (TWO) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (slab) slab[HB_BIG + krow * FZ_H + t * 16 + li] = aw1[kt][t][r];
          else atomicAdd(a.dW1 + (size_t)krow * a.ldw1 + t * 16 + li, aw1[kt][t][r]);
        }
      }
    }
  if (lq == 0) {
    if (li < n_out) {
      if (slab) slab[nb + li] = cs_n;
      else atomicAdd(dbn + li, cs_n);
    }
    if constexpr (TWO) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (slab) slab[HB_BIG + FZ_H * FZ_H + t * 16 + li] = cs_u[t];
        else atomicAdd(a.db1 + t * 16 + li, cs_u[t]);
      }
    }
  }
}

static int head_bwd_cus() {
  static thread_local int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  }
  return cus;
}

extern "C" int64_t dgppo_head_bwd_workspace_bytes(void) { return (int64_t)HB_SLAB_TWO * sizeof(float) * head_bwd_cus(); }

extern "C" int32_t dgppo_head_bwd(const float* feat, int32_t ldf, const float* u, const float* dout, const float* W1,
                                  const float* W2, float* dhs, float* dW1, int32_t ldw1, float* db1, float* dW2, int32_t ldw2,
                                  float* db2, int32_t M, int32_t n_out, float* workspace, int64_t workspace_bytes,
                                  dgppo_reduce_desc* pending, void* stream) {
  const bool two = W2 != nullptr;
  DGPPO_REQUIRE(M >= 0 && n_out >= 1 && n_out <= 16 && ldf >= FZ_H && ldw1 >= (two ? FZ_H : n_out) && (!two || ldw2 >= n_out),
                "head_bwd: bad shape M=%d n_out=%d ldf=%d ldw1=%d ldw2=%d", M, n_out, ldf, ldw1, ldw2);
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "head_bwd: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "head_bwd: workspace must be 16-byte aligned");
  if (pending) pending[0].pending = pending[1].pending = 0;
  if (M == 0) return 0;                            // (the row operands of an empty call may be NULL)
  DGPPO_REQUIRE(feat && dout && W1 && dhs && dW1 && db1 && (!two || (u && dW2 && db2)), "head_bwd: NULL operand");
  DGPPO_REQUIRE((ldf & 3) == 0 && ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(u) |
                 reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dhs)) & 15) == 0,
                "head_bwd: feat, u, dout, dhs must be 16-byte aligned, the leading dimension of feat a multiple of 4");
  const int slab = two ? HB_SLAB_TWO : HB_SLAB_ONE;
  constexpr size_t smem = sizeof(float) * (HB_WAVES * 3 * HB_TILE + FZ_H * HB_HL);
  static_assert(sizeof(float) * HB_WAVES * 3 * HB_TILE >= sizeof(float) * (HB_WAVES / 2) * 85 * 64 && smem <= 160 * 1024, "head_bwd: LDS image");
  static thread_local bool opted = false;
  if (!opted) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    opted = true;
  }
  // one workgroup per CU, a tile per wave and round; <= 4 workgroups (or no room for 8 slabs) add atomically, as dense_bwd_w
  const int tiles = (M + 15) / 16;
  int grid = (tiles + HB_WAVES - 1) / HB_WAVES;
  if (grid > head_bwd_cus()) grid = head_bwd_cus();
  const long max_slabs = (long)(workspace_bytes / (sizeof(float) * slab));
  float* ws = (grid > 4 && max_slabs >= 8) ? workspace : nullptr;
  if (ws && grid > max_slabs) grid = (int)max_slabs;
  HeadBwdArgs a{feat, ldf, u, dout, n_out, W1, W2, dhs, dW1, ldw1, db1, dW2, ldw2, db2, ws, M};
  if (two) hipLaunchKernelGGL(head_bwd_kernel<true>, dim3(grid), dim3(64 * HB_WAVES), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_bwd_kernel<false>, dim3(grid), dim3(64 * HB_WAVES), smem, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  if (!ws) return 0;
  dgppo_reduce_desc d[2];
  d[0] = dgppo_reduce_desc{ws, two ? dW2 : dW1, two ? db2 : db1, slab, grid, two ? ldw2 : ldw1, FZ_H, n_out, 1};
  d[1] = dgppo_reduce_desc{ws + HB_BIG, dW1, db1, slab, grid, ldw1, FZ_H, FZ_H, two ? 1 : 0};
  if (pending) {
    pending[0] = d[0];
    if (two) pending[1] = d[1];
    return 0;
  }
  return dgppo_dense_bwd_w_reduce_batch(d, two ? 2 : 1, stream);
}
