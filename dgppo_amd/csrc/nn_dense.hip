// Dense (fully connected) building blocks on the fp32 matrix cores of gfx950 (v_mfma_f32_16x16x4_f32):
//   dgppo_dense_fwd   Y[M,N]  = act(X[M,K] * W[K,N] + b)        (also  dX = dY * W^T via trans_w)
//   dgppo_dense_bwd_w dW[K,N] += X[M,K]^T * dY[M,N],  db[N] += colsum(dY)
// They replace flax nn.Dense as used by dgppo/nn/mlp.py:19-22, dgppo/nn/gnn.py:86-110, dgppo/nn/rnn.py:19-21 (GRUCell
// input/recurrent projections), dgppo/algo/module/policy.py:67-70 and dgppo/algo/module/value.py:41,76 — and the
// jax.grad of those (dgppo/algo/informarl.py:377,440; dgppo/algo/dgppo.py:316).
// fp32-input MFMA is bit-for-bit a k-ordered fmaf chain (exact fp32, no reduced precision).
#include "common.h"
#include "nn_gru.h"

using f32x4 = __attribute__((ext_vector_type(4))) float;
#ifdef DGPPO_STAMPS
__device__ unsigned long long g_dstamps[32];
#define DSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_dstamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int32_t dgppo_debug_stamps_dense(unsigned long long* out) {
  return (int32_t)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dstamps), sizeof(unsigned long long) * 32);
}
#else
#define DSTAMP(i)
#endif

#define DENSE_ROWS 64  // rows per workgroup (4 waves x 16)

struct DenseArgs {
  const float* X; int ldx;
  const float* W; int ldw;
  const float* bias;
  float* Y; int ldy;
  int M, K, N;
  int act;         // 0 none, 1 relu
  int accumulate;  // Y += result
  int trans_w;     // use W^T: result[m,n] = sum_k X[m,k] * W[n,k]
  const float* mask; int ldm;   // optional [M, N]: Y = (mask > 0) ? result : 0  — the ReLU backward of the layer whose output `mask` is
};


// Stage a [rows x 4*W4] tile of a row-major matrix into LDS (row stride Ls floats).  Loads are issued in batches of 8
// float4 per lane before any LDS store, so 8 global requests per lane are in flight instead of one.
template <bool ALIGNED_LDS>
__device__ inline void stage_tile_f4(const float* __restrict__ src, int ld, int row0, int row_end, int rows, int W4,
                                     float* __restrict__ dst, int Ls, int tid) {
  const int total = rows * W4;
  for (int base = 0; base < total; base += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * 256 + tid;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < total) {
        const int r = idx / W4, q = idx - r * W4;
        if (row0 + r < row_end) v[u] = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * ld + 4 * q);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * 256 + tid;
      if (idx < total) {
        const int r = idx / W4, q = idx - r * W4;
        float* d = dst + r * Ls + 4 * q;
        if (ALIGNED_LDS) *reinterpret_cast<float4*>(d) = v[u];
        else { d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w; }
      }
    }
  }
}

// Persistent workgroups: each keeps ITS W fragments for the whole K in registers (read once from L2), then walks row
// tiles with a stride of gridDim.x.  Per tile: the NEXT tile's X rows are fetched from HBM into registers while the
// current tile (already in LDS) runs on the matrix cores, then written to the other LDS buffer — one LDS-only barrier
// per tile.  Everything in the tile loop is branch-free: K is padded (with zeros, in LDS and in the W fragments) to
// KQ*16, out-of-range rows are clamped on load and masked on store.
//   CG  column groups (waves that split the N/16 column tiles), RG = 4/CG row groups, RTW row tiles (16 rows) per wave,
//   NTW column tiles per wave, KQ = padded K / 16.  Rows per tile RB = 16*RTW*RG.
template <int NTW, int RTW, int CG, int KQ, bool ACC>
__global__ void __launch_bounds__(256) dense_fwd_kernel(DenseArgs a) {
  extern __shared__ float xs_all[];
  constexpr int RG = 4 / CG, RB = 16 * RTW * RG;
  constexpr int KS = KQ * 4;                                   // k-steps of 4 (one MFMA each)
  // LDS row stride = 2 (mod 32) floats: an A-fragment read touches banks (2 li + lq) mod 32, all distinct inside each half of
  // the wave (lq in {0,1} / {2,3}); the odd stride used before put (li, lq = 1) and (li + 1, lq = 0) on the same bank whenever KQ
  // is even (K = 32, 64, 192): SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.5 (profiles/r03_nn_counters.json).  It also makes
  // every float4 slot 8-byte aligned: two ds_write_b64 per slot instead of four ds_write_b32.
  constexpr int Kl = KQ * 16 + 2;
  constexpr int SLOTS = RB * KS;                               // float4 slots per tile
  constexpr int PF = (SLOTS + 255) / 256;                      // prefetch registers (float4) per lane
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int cg = wave % CG, rg = wave / CG;
  const int K = a.K, N = a.N;
  const bool vec = ((K & 3) == 0) && ((a.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15) == 0);
  const int K4 = K >> 2;
  const int n_tiles = (a.M + RB - 1) / RB;
  DSTAMP(0);
  // ---- W fragments and bias of this wave ----
  float breg[KS][NTW], bias[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t) {
    const int col = (cg + CG * t) * 16 + li;
    bias[t] = (a.bias && col < N) ? a.bias[col] : 0.0f;
  }
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const int k = kk * 4 + lq;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int col = (cg + CG * t) * 16 + li;
      float bv = 0.0f;
      if (k < K && col < N) bv = a.trans_w ? a.W[(size_t)col * a.ldw + k] : a.W[(size_t)k * a.ldw + col];
      breg[kk][t] = bv;
    }
  }
  float4 pf[PF];
  auto fetch = [&](int tile) {          // global -> registers; every load is issued before anything waits
    const int row0 = tile * RB;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      int idx = u * 256 + tid;
      idx = idx < SLOTS ? idx : SLOTS - 1;                     // duplicates are benign
      const int r = idx / KS, q = idx - r * KS;
      int row = row0 + r;
      row = row < a.M ? row : a.M - 1;
      const int qc = q < K4 ? q : K4 - 1;
      pf[u] = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + 4 * qc);   // zero padding applied in commit
    }
  };
  auto commit = [&](int b) {            // registers -> LDS buffer b
    float* xs = xs_all + b * (RB * Kl);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      int idx = u * 256 + tid;
      idx = idx < SLOTS ? idx : SLOTS - 1;
      const int r = idx / KS, q = idx - r * KS;
      float2* d = reinterpret_cast<float2*>(xs + r * Kl + 4 * q);
      const bool pad = q >= K4;                                // touching pf only here keeps the loads in flight
      d[0] = pad ? make_float2(0.0f, 0.0f) : make_float2(pf[u].x, pf[u].y);
      d[1] = pad ? make_float2(0.0f, 0.0f) : make_float2(pf[u].z, pf[u].w);
    }
  };
  auto stage_scalar = [&](int tile, int b) {   // unaligned / K % 4 != 0 fallback (no prefetch)
    float* xs = xs_all + b * (RB * Kl);
    const int row0 = tile * RB;
    for (int idx = tid; idx < RB * (KQ * 16); idx += 256) {
      const int r = idx / (KQ * 16), k = idx - r * (KQ * 16);
      xs[r * Kl + k] = (row0 + r < a.M && k < K) ? a.X[(size_t)(row0 + r) * a.ldx + k] : 0.0f;
    }
  };
  f32x4 acc[RTW][NTW];
  f32x4 yold[ACC ? RTW : 1][ACC ? NTW : 1];
  auto load_yold = [&](int tile) {      // accumulate mode: the old Y tile, issued before the prefetch (in-order vmcnt)
    if constexpr (ACC) {
      const int row0 = tile * RB;
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        int col = (cg + CG * t) * 16 + li;
        col = col < N ? col : N - 1;
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int row = row0 + (rg * RTW + r) * 16 + lq * 4 + j;
            row = row < a.M ? row : a.M - 1;
            yold[r][t][j] = a.Y[(size_t)row * a.ldy + col];
          }
      }
    }
  };
  auto compute = [&](int b) {
    const float* xs = xs_all + b * (RB * Kl) + (rg * RTW * 16 + li) * Kl + lq;
#pragma unroll
    for (int r = 0; r < RTW; ++r)
#pragma unroll
      for (int t = 0; t < NTW; ++t) acc[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KS; c += 16) {
      float areg[RTW][16];
#pragma unroll
      for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          if (c + kk < KS) areg[r][kk] = xs[r * 16 * Kl + (c + kk) * 4];
      __builtin_amdgcn_sched_barrier(0);          // one LDS round trip for the chunk, then the MFMAs back to back
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
          for (int t = 0; t < NTW; ++t)
            if (c + kk < KS)
              acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[r][kk], breg[c + kk][t], acc[r][t], 0, 0, 0);
    }
  };
  auto epilogue = [&](int tile) {       // C/D layout: col = lane & 15, row = (lane >> 4) * 4 + reg
    const int row0 = tile * RB;
    // the ReLU-mask values of the whole tile are read BEFORE the first store: read per element in the store loop, every
    // load waits (vmcnt(0)) for the store in front of it as well — one serialised HBM round trip per element
    float mk[RTW][NTW][4];
    if (a.mask != nullptr) {
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        int col = (cg + CG * t) * 16 + li;
        col = col < N ? col : N - 1;
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int row = row0 + (rg * RTW + r) * 16 + lq * 4 + j;
            row = row < a.M ? row : a.M - 1;
            mk[r][t][j] = a.mask[(size_t)row * a.ldm + col];
          }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int col = (cg + CG * t) * 16 + li;
#pragma unroll
      for (int r = 0; r < RTW; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = row0 + (rg * RTW + r) * 16 + lq * 4 + j;
          float v = acc[r][t][j] + bias[t];
          if constexpr (ACC) v += yold[r][t][j];
          if (a.act == 1) v = relu_nan(v);
          if (a.mask != nullptr) v = (mk[r][t][j] > 0.0f) ? v : 0.0f;
          if (col < N && row < a.M) a.Y[(size_t)row * a.ldy + col] = v;
        }
      }
    }
  };
  // LDS-only barrier: __syncthreads() would also wait for the epilogue's global stores (vmcnt(0)) on every tile.
  // Y is never re-read across waves, so only the ds_writes have to land before the other waves read them.
#define DGPPO_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
  int tile = blockIdx.x;
  if (vec) {
    fetch(tile);
    commit(0);
    __syncthreads();
    DSTAMP(1);
    int cur = 0;
    for (; tile < n_tiles; tile += gridDim.x) {
      int nxt = tile + gridDim.x;
      nxt = nxt < n_tiles ? nxt : n_tiles - 1;                 // last round re-fetches a valid tile; never committed-to-use
      load_yold(tile);
      fetch(nxt);                                              // in flight during the MFMAs below
      __builtin_amdgcn_sched_barrier(0);                       // keep the scheduler from sinking the loads past them
      compute(cur);
      commit(cur ^ 1);                                         // before the stores: vmcnt retires in order
      __builtin_amdgcn_sched_barrier(0);
      epilogue(tile);
      DGPPO_LDS_BARRIER();
      cur ^= 1;
    }
  } else {
    for (; tile < n_tiles; tile += gridDim.x) {
      stage_scalar(tile, 0);
      load_yold(tile);
      __syncthreads();
      compute(0);
      epilogue(tile);
      DGPPO_LDS_BARRIER();
    }
  }
#undef DGPPO_LDS_BARRIER
  DSTAMP(2);
}

template <int NTW, int RTW, int CG, int KQ, bool ACC>
static void launch_dense_acc(const DenseArgs& a, hipStream_t s) {
  constexpr int RB = 16 * RTW * (4 / CG);
  constexpr size_t smem = 2 * (size_t)RB * (KQ * 16 + 2) * sizeof(float);
  static_assert(smem <= 160 * 1024, "dense tile exceeds the 160 KB LDS of a gfx950 CU");
  // persistent grid = what is actually resident (registers and LDS both limit it); queried once per instantiation
  static thread_local int cap = 0;
  if (cap == 0) {
    int per_cu = 0, dev = 0, cus = 256;
    if (smem > 64 * 1024)                          // above the default dynamic-LDS limit: opt in explicitly
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_fwd_kernel<NTW, RTW, CG, KQ, ACC>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(
            &dense_fwd_kernel<NTW, RTW, CG, KQ, ACC>), 256, smem) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    cap = per_cu * cus;
  }
  const int n_tiles = cdiv(a.M, RB);
  const int grid = n_tiles < cap ? n_tiles : cap;
  hipLaunchKernelGGL((dense_fwd_kernel<NTW, RTW, CG, KQ, ACC>), dim3(grid), dim3(256), smem, s, a);
}

template <int NTW, int RTW, int CG, int KQ>
static void launch_dense_kq(const DenseArgs& a, hipStream_t s) {
  if (a.accumulate) launch_dense_acc<NTW, RTW, CG, KQ, true>(a, s);
  else launch_dense_acc<NTW, RTW, CG, KQ, false>(a, s);
}

template <int NTW, int RTW, int CG>
static void launch_dense(const DenseArgs& a, hipStream_t s) {
  const int kq = cdiv(a.K, 16);                    // padded-K instantiations: 16,32,48,64,96,128,144,192,256
  if (kq <= 1) launch_dense_kq<NTW, RTW, CG, 1>(a, s);
  else if (kq == 2) launch_dense_kq<NTW, RTW, CG, 2>(a, s);
  else if (kq == 3) launch_dense_kq<NTW, RTW, CG, 3>(a, s);
  else if (kq == 4) launch_dense_kq<NTW, RTW, CG, 4>(a, s);
  else if (kq <= 6) launch_dense_kq<NTW, RTW, CG, 6>(a, s);
  else if (kq <= 8) launch_dense_kq<NTW, RTW, CG, 8>(a, s);
  else if (kq == 9) launch_dense_kq<NTW, RTW, CG, 9>(a, s);
  else if (kq <= 12) launch_dense_kq<NTW, RTW, CG, 12>(a, s);
  else launch_dense_kq<NTW, RTW, CG, 16>(a, s);
}

// ---- narrow inputs (K <= 16): the query projection of the first GNN layer (K = 8), the input gradients of the 4- /
// 1- / 2-wide heads.  These move 100+ bytes per row for a handful of FMAs: a tile pipeline with a barrier per 32 rows
// (above) runs at its latency floor (23 us for 17 MB).  Here a thread owns four consecutive output columns of a row, the
// whole W (<= 16 x 192) sits in LDS in [k][n] order (transposed on the way in if trans_w), X is read straight from global
// memory (the threads of a row read the same addresses: one L1 broadcast) and Y is written as coalesced 16-byte stores.
#define DSK_MAXK 16
template <bool VECY>
__global__ void __launch_bounds__(256) dense_smallk_kernel(DenseArgs a) {
  __shared__ float sW[DSK_MAXK * 192 + 192];
  const int K = a.K, N = a.N, nq = (N + 3) >> 2, Nl = nq * 4;
  for (int idx = threadIdx.x; idx < K * Nl; idx += 256) {
    const int k = idx / Nl, c = idx - k * Nl;
    float w = 0.0f;
    if (c < N) w = a.trans_w ? a.W[(size_t)c * a.ldw + k] : a.W[(size_t)k * a.ldw + c];
    sW[idx] = w;
  }
  for (int c = threadIdx.x; c < Nl; c += 256) sW[K * Nl + c] = (a.bias && c < N) ? a.bias[c] : 0.0f;
  __syncthreads();
  const long items = (long)a.M * nq;
  const uint32_t rcp = (uint32_t)((0x100000000ull + nq - 1) / nq);    // item / nq as a multiply-high (exact below 2^32 / nq items)
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const int row = (int)__umulhi((uint32_t)it, rcp);
    const int c0 = ((int)it - row * nq) * 4;
    const float* x = a.X + (size_t)row * a.ldx;
    float4 acc = *reinterpret_cast<const float4*>(sW + K * Nl + c0);
    for (int k = 0; k < K; ++k) {
      const float xv = x[k];
      const float4 w = *reinterpret_cast<const float4*>(sW + k * Nl + c0);
      acc.x = fmaf(xv, w.x, acc.x); acc.y = fmaf(xv, w.y, acc.y); acc.z = fmaf(xv, w.z, acc.z); acc.w = fmaf(xv, w.w, acc.w);
    }
    float* y = a.Y + (size_t)row * a.ldy + c0;
    float r[4] = {acc.x, acc.y, acc.z, acc.w};
    if (VECY) {
      if (a.accumulate) { const float4 o = *reinterpret_cast<const float4*>(y); r[0] += o.x; r[1] += o.y; r[2] += o.z; r[3] += o.w; }
      if (a.act == 1) { r[0] = relu_nan(r[0]); r[1] = relu_nan(r[1]); r[2] = relu_nan(r[2]); r[3] = relu_nan(r[3]); }
      if (a.mask) {
        const float4 mk = *reinterpret_cast<const float4*>(a.mask + (size_t)row * a.ldm + c0);
        r[0] = mk.x > 0.f ? r[0] : 0.f; r[1] = mk.y > 0.f ? r[1] : 0.f; r[2] = mk.z > 0.f ? r[2] : 0.f; r[3] = mk.w > 0.f ? r[3] : 0.f;
      }
      *reinterpret_cast<float4*>(y) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      for (int u = 0; u < 4; ++u) {
        if (c0 + u >= N) break;
        float v = r[u];
        if (a.accumulate) v += y[u];
        if (a.act == 1) v = relu_nan(v);
        if (a.mask) v = a.mask[(size_t)row * a.ldm + c0 + u] > 0.f ? v : 0.f;
        y[u] = v;
      }
    }
  }
}

static bool dense_smallk_ok(const DenseArgs& a) {
  const long nq = (a.N + 3) / 4;                    // the multiply-high row index is exact while items * nq < 2^32
  return a.K <= DSK_MAXK && a.N <= 192 && (long)a.M * nq * nq < (1l << 32);
}
static void launch_dense_smallk(const DenseArgs& a, hipStream_t s) {
  const long items = (long)a.M * ((a.N + 3) / 4);
  long blocks = (items + 256 * 4 - 1) / (256 * 4);            // >= 4 items per thread amortise the staging of W
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  const bool vec = (a.N & 3) == 0 && (a.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Y) & 15) == 0 &&
                   (!a.mask || ((a.ldm & 3) == 0 && (reinterpret_cast<uintptr_t>(a.mask) & 15) == 0));
  if (vec) hipLaunchKernelGGL(dense_smallk_kernel<true>, dim3((int)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dense_smallk_kernel<false>, dim3((int)blocks), dim3(256), 0, s, a);
}

int32_t dense_fwd_launch(const DenseArgs& a, hipStream_t s) {
  DGPPO_REQUIRE(a.M >= 0 && a.K >= 1 && a.N >= 1, "dense: bad shape M=%d K=%d N=%d", a.M, a.K, a.N);
  DGPPO_REQUIRE(a.N <= 192 && a.K <= 256, "dense: N <= 192 and K <= 256 supported (N=%d K=%d)", a.N, a.K);
  DGPPO_REQUIRE(a.X && a.W && a.Y, "dense: NULL operand");
  DGPPO_REQUIRE(a.ldx >= a.K && a.ldy >= a.N, "dense: leading dimensions too small");
  if (a.M == 0) return 0;
  const int nt = cdiv(a.N, 16);
  if (dense_smallk_ok(a)) launch_dense_smallk(a, s);
  else if (nt >= 9) launch_dense<3, 2, 4>(a, s);   // N in (128, 192]
  else if (nt >= 5) launch_dense<2, 2, 4>(a, s);   // N in (64, 128]
  else if (nt == 4) launch_dense<1, 2, 4>(a, s);   // N in (48, 64]
  else if (nt == 3) launch_dense<2, 1, 2>(a, s);   // N in (32, 48]
  else if (nt == 2) launch_dense<1, 1, 2>(a, s);   // N in (16, 32]
  else launch_dense<1, 1, 1>(a, s);                // N <= 16  (64-row tiles, one row tile per wave)
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- weight gradient: dW[K,N] += X^T dY, db[N] += colsum(dY) -------------------------------------------------------
struct DenseBwdWArgs {
  const float* X; int ldx;
  const float* dY; int ldy;
  float* dW; int ldw;
  float* db;  // may be NULL
  int M, K, N;
  int rows_per_block;
  float* part;        // scratch for per-workgroup partials [grid][part_stride], or NULL: atomicAdd straight into dW/db
  int part_stride;    // >= K*N + N
  size_t ws_bytes;    // size of the caller's scratch buffer behind `part`
  // dense_bwd_xw only (the DX kernels): the input gradient of the same Dense from the same pass
  const float* W; int ldwp;   // [K,N] parameters
  float* dX; int lddx;        // [M,K]: dX = dY W^T, or with acc_mask: dX = (X > 0) ? dX + dY W^T : 0
  int acc_mask;
};

// A workgroup owns a contiguous chunk of rows and walks it in tiles of 32.  X[32,K] and dY[32,N] tiles live in LDS
// (double-buffered); the NEXT tile's rows are fetched from HBM into registers while the current one runs on the matrix
// cores and are written to the other buffer afterwards — one LDS-only barrier per tile (no global stores in the loop, and
// a __syncthreads() would wait for the prefetch).  Wave w accumulates the output row-tiles kt = w, w+4, ... x all NT
// column tiles over the tile's 8 four-row slabs (A[i=k][kk=m] = X[m][k], B[kk=m][j] = dY[m][j]).  K and N are padded to
// KT*16 / NT*16 with zeros in LDS so the loop is branch-free; db's column sums are accumulated per lane from the
// prefetch registers and reduced once at the end.  Write-out: every workgroup stores its K*N (+N) partial sums to a
// slab of the caller's workspace and dense_bwd_w_reduce_kernel folds the slabs into dW/db — with hundreds of workgroups
// finishing together, atomicAdd on the same K*N addresses serialises (measured: 137 us vs 10 us for K=64, N=4).  Only
// launches of <= 4 workgroups (or a NULL / too small workspace) use atomicAdd directly.
// NG > 1: a workgroup is NG such 4-wave groups (256 * NG threads, one workgroup per CU), each with its own row chunk of
// rows_per_block rows and its own pair of LDS tile buffers; they walk their chunks in step (the barrier is the workgroup's),
// add their accumulators through the tile LDS once the chunks are done, and group 0 writes the workgroup's ONE slab: a
// CU that kept NG resident workgroups busy wrote NG slabs for the second stage to read back.
// DX: the same pass also forms dX[32,K] = dY W^T of every tile (dgppo_dense_bwd_xw; K = KT*16 and N = NT*16 exactly, 16-byte
// aligned operands: the launcher's condition).  The tile's 2 KT products (16 rows x 16 columns, reduction over n) are dealt
// over the group's four waves so that every wave issues the same number of MFMAs per tile (XwDeal below; a wave without a
// KTW-th row tile of dW skips it instead of redoing the last one).  A wave keeps W^T in registers only for the column tiles of
// its own units (at most kw() * NT float4 per lane); the dY operand is read from memory again in the fragment layout (lane
// (li, lq) = row li, the four columns 16s + 4lq ..: one float4 per 16 columns, the k-steps taking n in that order on both
// operands) - the rows were just fetched for the LDS tile, so these are cache hits, and a column walk of the row-major LDS
// tile would be an 8-way bank conflict.  The product is formed transposed (W dY^T), which leaves a lane with 16 contiguous bytes
// of one dX row; the `+=` form adds the old dX (requested in that shape with the dY operand, at the top of the round) and applies
// the ReLU mask, X itself: the LDS tile.  The units go to a dX tile in LDS, and the tile leaves one round later as 16-byte
// stores of whole rows by all threads of the group; a second LDS barrier per round separates that read-out from the next units.
#define BW_ROWS 32
// DX: how a group's four waves share the 2 KT products (16-row tile mt, 16-column tile kt) of a dX tile, unit u = 2 kt + mt.
// Wave w owns nkt(w) row tiles of dW, 8 NT MFMAs per tile each against 4 NT per unit: with units(w) = KT - 2 nkt(w) every
// wave issues KT * 4 NT MFMAs per tile (KT = 9: 3, 5, 5, 5 units; KT = 3: 1, 1, 1, 3; KT = 2: 0, 0, 2, 2), and the units of a
// wave are consecutive, so that it keeps W^T for at most kw() column tiles.
template <int KT>
struct XwDeal {
  static constexpr int nkt(int w) { return w < KT ? (KT - w + 3) / 4 : 0; }
  static constexpr int units(int w) { return KT - 2 * nkt(w); }
  static constexpr int start(int w) { int s = 0; for (int v = 0; v < w; ++v) s += units(v); return s; }
  static constexpr int kw() {
    int m = 1;
    for (int w = 0; w < 4; ++w) {
      const int k = units(w) > 0 ? ((start(w) + units(w) - 1) >> 1) - (start(w) >> 1) + 1 : 0;
      m = k > m ? k : m;
    }
    return m;
  }
};
#define XW_DL(KT) ((KT) * 16 + 4)   // row stride of the dX tile in LDS: = 4 (mod 8) floats, 16-byte fragment stores hit 8 x 4 banks

template <int NT, int KT, int NG, bool DX = false, bool ACCM = false>
__global__ void __launch_bounds__(256 * NG) dense_bwd_w_kernel(DenseBwdWArgs a) {
  extern __shared__ float sm_wg[];
  constexpr int KTW = (KT + 3) / 4;
  // row strides = 16 mod 32 floats: the four slab rows of a fragment read hit disjoint bank halves
  constexpr int Kl = (KT & 1) ? KT * 16 : KT * 16 + 16;
  constexpr int Nl = (NT & 1) ? NT * 16 : NT * 16 + 16;
  constexpr int BUF = BW_ROWS * (Kl + Nl);
  constexpr int XQ = KT * 4, YQ = NT * 4;                      // float4 slots per padded row
  constexpr int PFX = (BW_ROWS * XQ + 255) / 256, PFY = (BW_ROWS * YQ + 255) / 256;
  const int K = a.K, N = a.N;
  const int grp = NG > 1 ? (int)(threadIdx.x >> 8) : 0;
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  float* sm = sm_wg + grp * 2 * BUF;
  // group 0 holds the longest chunk of the workgroup: its tile count is everyone's trip count (rows past a group's own
  // m_end are zeros in LDS), so that every wave meets every barrier
  const int wg_begin = blockIdx.x * NG * a.rows_per_block;
  const int m_begin = wg_begin + grp * a.rows_per_block;
  const int m_end = min(a.M, m_begin + a.rows_per_block);
  const int n_tiles = (min(a.M - wg_begin, a.rows_per_block) + BW_ROWS - 1) / BW_ROWS;
  const bool vec = ((K & 3) == 0) && ((a.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15) == 0) &&
                   ((N & 3) == 0) && ((a.ldy & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.dY) & 15) == 0);
  const int K4 = K >> 2, N4 = N >> 2;
  f32x4 acc[KTW][NT];
#pragma unroll
  for (int i = 0; i < KTW; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 pfx[PFX], pfy[PFY], csum[PFY];
#pragma unroll
  for (int u = 0; u < PFY; ++u) csum[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  // DX: the product is formed TRANSPOSED, dX^T[16 k, 16 m] = W dY^T: A[i = li][kk = lq] of k-step (s, e) = W[kt*16 + li][16 s + 4 lq + e],
  // B[kk = lq][j = li] of the same step = dY[row li][16 s + 4 lq + e]; the C/D layout (row i = 4 lq + reg, col j = li) then leaves
  // a lane with dX[row li][kt*16 + 4 lq .. + 3]: 16 contiguous bytes of one row
  using D = XwDeal<KT>;
  constexpr int KW = DX ? D::kw() : 1;
  constexpr int Dl = XW_DL(KT);
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int u0 = wv == 0 ? D::start(0) : wv == 1 ? D::start(1) : wv == 2 ? D::start(2) : D::start(3);
  const int u1 = u0 + (wv == 0 ? D::units(0) : wv == 1 ? D::units(1) : wv == 2 ? D::units(2) : D::units(3));
  const int kb = u0 >> 1;               // the wave's first column tile of dX
  float* dxs = sm_wg + NG * 2 * BUF + grp * BW_ROWS * Dl;     // the group's dX tile [32][Dl], behind every group's X / dY buffers
  float4 wreg[KW][DX ? NT : 1], old[ACCM ? KW : 1][ACCM ? 2 : 1];
  if constexpr (DX) {
    static_assert(KT >= 2 && D::start(3) + D::units(3) == 2 * KT, "dense_bwd_xw: the waves' units cover the dX tile");
#pragma unroll
    for (int c = 0; c < KW; ++c) {
      const int kt = kb + c < KT ? kb + c : KT - 1;
#pragma unroll
      for (int s = 0; s < NT; ++s)
        wreg[c][s] = *reinterpret_cast<const float4*>(a.W + (size_t)(kt * 16 + li) * a.ldwp + 16 * s + 4 * lq);
    }
  }
  auto fetch_old = [&](int m0) {        // ACCM: the old dX of the wave's units in the fragment shape (rows clamped; stores are masked)
    if constexpr (ACCM) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        int row = m0 + mt * 16 + li;
        row = row < a.M ? row : a.M - 1;
#pragma unroll
        for (int c = 0; c < KW; ++c) {
          const int u = 2 * (kb + c) + mt;
          if (u >= u0 && u < u1) old[c][mt] = *reinterpret_cast<const float4*>(a.dX + (size_t)row * a.lddx + (kb + c) * 16 + 4 * lq);
        }
      }
    }
  };
  auto dx_tile = [&](int b) {           // DX: the wave's units of the dX tile -> dxs; b = the X tile's buffer (the mask of ACCM)
    if constexpr (DX) {
      [[maybe_unused]] const float* xs = sm + b * BUF;
      if (u1 == u0) return;
      // the dY operand from the row-major LDS tile: 16 bytes per lane, a 2-way bank conflict (rows li and li + 4 of a 16-lane
      // group share banks at a stride of 16 mod 32 floats) on NT reads per 16 rows
      const float* ys = sm + b * BUF + BW_ROWS * Kl + li * Nl + 4 * lq;
      f32x4 ya[2][NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int s = 0; s < NT; ++s) ya[mt][s] = *reinterpret_cast<const f32x4*>(ys + mt * 16 * Nl + 16 * s);
#pragma unroll
      for (int c = 0; c < KW; ++c)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const int u = 2 * (kb + c) + mt;
          if (u < u0 || u >= u1) continue;
          f32x4 dx = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < NT; ++s) {
            dx = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[c][s].x, ya[mt][s][0], dx, 0, 0, 0);
            dx = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[c][s].y, ya[mt][s][1], dx, 0, 0, 0);
            dx = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[c][s].z, ya[mt][s][2], dx, 0, 0, 0);
            dx = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[c][s].w, ya[mt][s][3], dx, 0, 0, 0);
          }
          const int rl = mt * 16 + li, col = (kb + c) * 16 + 4 * lq;
          if constexpr (ACCM) {
            const float4 x = *reinterpret_cast<const float4*>(xs + rl * Kl + col);
            const float4 o = old[c][mt];
            dx[0] = (x.x > 0.0f) ? o.x + dx[0] : 0.0f; dx[1] = (x.y > 0.0f) ? o.y + dx[1] : 0.0f;
            dx[2] = (x.z > 0.0f) ? o.z + dx[2] : 0.0f; dx[3] = (x.w > 0.0f) ? o.w + dx[3] : 0.0f;
          }
          *reinterpret_cast<f32x4*>(dxs + rl * Dl + col) = dx;
        }
    }
  };
#define DGPPO_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
  // DX: the finished dX tile leaves as whole rows, 16 bytes per thread, by all threads of the group: dxs -> registers before a
  // barrier (the waves' next units overwrite dxs behind it), registers -> memory after it.  m0 = m_begin - 32 in round 0: no row
  // passes the mask
  auto rows_out = [&](int m0, bool in_loop) {
    if constexpr (DX) {
      // RPP whole rows per pass, thread (r0, q) = (tid / XQ, tid % XQ) of each: one LDS address and one row pointer per thread,
      // the passes differ by compile-time offsets (rows past the tile's 32 are clamped for the read and masked for the store)
      constexpr int RPP = 256 / XQ, NP = (BW_ROWS + RPP - 1) / RPP;
      const int r0 = tid / XQ, q = tid - r0 * XQ;
      const bool lane_ok = r0 < RPP;
      const float* src = dxs + (lane_ok ? r0 : 0) * Dl + 4 * q;
      f32x4 q4[NP];                     // (a vector type: float4 copies out of LDS would keep the array in scratch)
#pragma unroll
      for (int u = 0; u < NP; ++u)
        q4[u] = *reinterpret_cast<const f32x4*>(src + (u * RPP + RPP <= BW_ROWS ? u * RPP : BW_ROWS - RPP) * Dl);
      if (in_loop) DGPPO_LDS_BARRIER();
      float* dst = a.dX + (size_t)(m0 + r0) * a.lddx + 4 * q;
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        // the last pass re-reads rows of the pass before (its window is shifted up to end at row 31): it stores only the new ones
        constexpr int kShift = NP * RPP - BW_ROWS;
        const int r = (u == NP - 1 ? u * RPP - kShift : u * RPP) + r0;
        const bool fresh = u < NP - 1 || r0 >= kShift;
        if (lane_ok && fresh && m0 + r >= m_begin && m0 + r < m_end)
          *reinterpret_cast<f32x4*>(dst + (ptrdiff_t)(u == NP - 1 ? u * RPP - kShift : u * RPP) * a.lddx) = q4[u];
      }
    }
  };

  int tl = tid;                         // tid as fetch / commit see it (DX: made opaque once per round, see the loop)
  auto fetch = [&](int m0) {            // global -> registers (rows clamped; masking happens in commit)
#pragma unroll
    for (int u = 0; u < PFX; ++u) {
      int idx = u * 256 + tl;
      idx = idx < BW_ROWS * XQ ? idx : BW_ROWS * XQ - 1;
      const int r = idx / XQ, q = idx - r * XQ;
      int row = m0 + r;
      row = row < a.M ? row : a.M - 1;
      pfx[u] = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + 4 * (q < K4 ? q : K4 - 1));
    }
#pragma unroll
    for (int u = 0; u < PFY; ++u) {
      int idx = u * 256 + tl;
      idx = idx < BW_ROWS * YQ ? idx : BW_ROWS * YQ - 1;
      const int r = idx / YQ, q = idx - r * YQ;
      int row = m0 + r;
      row = row < a.M ? row : a.M - 1;
      pfy[u] = *reinterpret_cast<const float4*>(a.dY + (size_t)row * a.ldy + 4 * (q < N4 ? q : N4 - 1));
    }
  };
  auto commit = [&](int m0, int b) {    // registers -> LDS buffer b; rows >= m_end and padded columns become zeros
    float* xs = sm + b * BUF;
    float* ys = xs + BW_ROWS * Kl;
#pragma unroll
    for (int u = 0; u < PFX; ++u) {
      const int idx = u * 256 + tl;
      const int r = idx / XQ, q = idx - r * XQ;
      const bool ok = (m0 + r < m_end) && (q < K4);
      const float4 v = ok ? pfx[u] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < BW_ROWS * XQ) *reinterpret_cast<float4*>(xs + r * Kl + 4 * q) = v;
    }
#pragma unroll
    for (int u = 0; u < PFY; ++u) {
      const int idx = u * 256 + tl;
      const int r = idx / YQ, q = idx - r * YQ;
      const bool ok = (m0 + r < m_end) && (q < N4) && (idx < BW_ROWS * YQ);
      const float4 v = ok ? pfy[u] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < BW_ROWS * YQ) *reinterpret_cast<float4*>(ys + r * Nl + 4 * q) = v;
      csum[u].x += v.x; csum[u].y += v.y; csum[u].z += v.z; csum[u].w += v.w;
    }
  };
  auto stage_scalar = [&](int m0) {     // unaligned / odd-width fallback: synchronous, buffer 0
    float* xs = sm;
    float* ys = xs + BW_ROWS * Kl;
    for (int idx = tid; idx < BW_ROWS * KT * 16; idx += 256) {
      const int r = idx / (KT * 16), k = idx - r * (KT * 16);
      xs[r * Kl + k] = (m0 + r < m_end && k < K) ? a.X[(size_t)(m0 + r) * a.ldx + k] : 0.0f;
    }
    for (int idx = tid; idx < BW_ROWS * NT * 16; idx += 256) {
      const int r = idx / (NT * 16), c = idx - r * (NT * 16);
      ys[r * Nl + c] = (m0 + r < m_end && c < N) ? a.dY[(size_t)(m0 + r) * a.ldy + c] : 0.0f;
    }
  };
  // the first NA of the wave's KTW row tiles x all NT column tiles over the tile's 8 four-row slabs
#define DGPPO_BW_COMPUTE(NA)                                                                                                  \
  _Pragma("unroll") for (int s4 = 0; s4 < BW_ROWS / 4; ++s4) {                                                                \
    float bv[NT], av[(NA) > 0 ? (NA) : 1];                                                                                    \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) bv[t] = ys[s4 * 4 * Nl + t * 16];                                         \
    _Pragma("unroll") for (int i = 0; i < (NA); ++i) {                                                                        \
      int kt = wave + 4 * i;                                                                                                  \
      kt = kt < KT ? kt : KT - 1;                              /* surplus waves redo the last tile (never written back) */    \
      av[i] = xs[s4 * 4 * Kl + kt * 16];                                                                                      \
    }                                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < (NA); ++i)                                                                          \
      _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                                          \
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[t], acc[i][t], 0, 0, 0);                                   \
  }
  // DX: a wave without a KTW-th row tile skips it (its MFMAs are dealt to dX units instead: XwDeal)
  const bool surplus = DX && wv + 4 * (KTW - 1) >= KT;
  auto compute = [&](int b) {
    const float* xs = sm + b * BUF + lq * Kl + li;
    const float* ys = sm + b * BUF + BW_ROWS * Kl + lq * Nl + li;
    if (DX && surplus) { DGPPO_BW_COMPUTE(KTW - 1) }
    else { DGPPO_BW_COMPUTE(KTW) }
  };
#undef DGPPO_BW_COMPUTE
  float colsum = 0.0f;                 // scalar path only
  // DX has no scalar path (it would form no dX): the host launches it only where bwd_w_vec() holds, which is `vec`
  if (DX || vec) {
    fetch(m_begin);
    commit(m_begin, 0);
    __syncthreads();
    int cur = 0;
    for (int it = 0, m0 = m_begin; it < n_tiles; ++it, m0 += BW_ROWS) {
      // DX: what fetch / commit derive from the thread index is formed again every round instead of living in ~40 registers
      if constexpr (DX) asm volatile("" : "+v"(tl));
      rows_out(m0 - BW_ROWS, true);                            // DX: the tile of the round before, one round behind its products
      if constexpr (DX) __builtin_amdgcn_sched_barrier(0);     // (its registers are free again before the fetches take theirs)
      fetch_old(m0);
      fetch(m0 + BW_ROWS);                                     // past m_end on the last round: masked to zeros in commit
      __builtin_amdgcn_sched_barrier(0);
      compute(cur);
      commit(m0 + BW_ROWS, cur ^ 1);
      dx_tile(cur);                                            // reads X's tile (the mask) before the barrier frees it
      DGPPO_LDS_BARRIER();
      cur ^= 1;
    }
    rows_out(m_begin + (n_tiles - 1) * BW_ROWS, false);        // DX: the last tile
  } else {
    for (int it = 0, m0 = m_begin; it < n_tiles; ++it, m0 += BW_ROWS) {
      stage_scalar(m0);
      __syncthreads();
      if (a.db != nullptr && tid < N) {
        const float* ys = sm + BW_ROWS * Kl;
        float cs = 0.0f;
#pragma unroll 8
        for (int r = 0; r < BW_ROWS; ++r) cs += ys[r * Nl + tid];
        colsum += cs;
      }
      compute(0);
      __syncthreads();
    }
  }
#undef DGPPO_LDS_BARRIER
  if (NG > 1) {
    // groups 1.. park their accumulators and column sums in their own (now idle) tile buffers, lane-major; group 0 adds them
    constexpr int ACCF = KTW * NT * 4 * 256;
    static_assert(NG == 1 || ACCF + PFY * 4 * 256 <= 2 * BUF, "dense_bwd_w: the group exchange does not fit the tile buffers");
    __syncthreads();
    if (grp > 0) {
#pragma unroll
      for (int i = 0; i < KTW; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) sm[((i * NT + t) * 4 + r) * 256 + tid] = acc[i][t][r];
      if (!vec) csum[0].x = colsum;
#pragma unroll
      for (int u = 0; u < PFY; ++u) {
        sm[ACCF + (u * 4 + 0) * 256 + tid] = csum[u].x; sm[ACCF + (u * 4 + 1) * 256 + tid] = csum[u].y;
        sm[ACCF + (u * 4 + 2) * 256 + tid] = csum[u].z; sm[ACCF + (u * 4 + 3) * 256 + tid] = csum[u].w;
      }
    }
    __syncthreads();
    if (grp == 0) {
      for (int g = 1; g < NG; ++g) {
        const float* o = sm_wg + g * 2 * BUF;
#pragma unroll
        for (int i = 0; i < KTW; ++i)
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][t][r] += o[((i * NT + t) * 4 + r) * 256 + tid];
        if (!vec) colsum += o[ACCF + tid];
        else {
#pragma unroll
          for (int u = 0; u < PFY; ++u) {
            csum[u].x += o[ACCF + (u * 4 + 0) * 256 + tid]; csum[u].y += o[ACCF + (u * 4 + 1) * 256 + tid];
            csum[u].z += o[ACCF + (u * 4 + 2) * 256 + tid]; csum[u].w += o[ACCF + (u * 4 + 3) * 256 + tid];
          }
        }
      }
    }
  }
  float* slab = a.part ? a.part + (size_t)blockIdx.x * a.part_stride : nullptr;
#pragma unroll
  for (int i = 0; i < KTW; ++i) {
    const int kt = wave + 4 * i;
    if (kt >= KT || grp != 0) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = t * 16 + li;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = kt * 16 + lq * 4 + r;
        if (krow >= K) continue;
        if (slab) slab[krow * N + col] = acc[i][t][r];
        else atomicAdd(a.dW + (size_t)krow * a.ldw + col, acc[i][t][r]);
      }
    }
  }
  if (a.db != nullptr) {
    float cs = colsum;
    if (vec) {                          // reduce the per-lane column sums through LDS: red[row slot][column]
      __syncthreads();
      float* red = sm;
#pragma unroll
      for (int u = 0; u < PFY; ++u) {
        const int idx = u * 256 + tid;
        const int r = idx / YQ, q = idx - r * YQ;
        if (idx < BW_ROWS * YQ) *reinterpret_cast<float4*>(red + r * (YQ * 4) + 4 * q) = csum[u];
      }
      __syncthreads();
      cs = 0.0f;
      if (tid < N) {
#pragma unroll 8
        for (int r = 0; r < BW_ROWS; ++r) cs += red[r * (YQ * 4) + tid];
      }
    }
    if (tid < N && grp == 0) {
      if (slab) slab[K * N + tid] = cs;
      else atomicAdd(a.db + tid, cs);
    }
  }
}

// Slabs summed by one thread of the second stage before its atomicAdd.  With one slab per CU (G = 256) 16 gives 16 splits:
// 16 x E/256 workgroups (784 for a 64 x 192 gradient, 112 for 48 x 32) of four independent 4-deep load chains each, and
// 16 atomicAdds per element (200 k for the largest gradient, far below the atomic rate).  32 would halve the workgroups
// of the small gradients, which are latency- and not bandwidth-bound.
#define REDUCE_SLABS_PER_SPLIT 16

// Second stage: dW[k][n] += sum_g part[g][k*N + n], db[n] += sum_g part[g][K*N + n].  blockIdx.y splits the slabs so
// that small outputs still fill the device; the splits meet in at most gridDim.y atomicAdds per element.
__global__ void __launch_bounds__(256) dense_bwd_w_reduce_kernel(const float* __restrict__ part, int part_stride, int G,
                                                                 float* __restrict__ dW, int ldw, float* __restrict__ db,
                                                                 int K, int N) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int E = K * N + (db ? N : 0);
  if (e >= E) return;
  const int per = (G + gridDim.y - 1) / gridDim.y;
  const int g0 = blockIdx.y * per, g1 = min(G, g0 + per);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int g = g0;
  for (; g + 3 < g1; g += 4) {
    s0 += part[(size_t)g * part_stride + e];
    s1 += part[(size_t)(g + 1) * part_stride + e];
    s2 += part[(size_t)(g + 2) * part_stride + e];
    s3 += part[(size_t)(g + 3) * part_stride + e];
  }
  for (; g < g1; ++g) s0 += part[(size_t)g * part_stride + e];
  const float sum = (s0 + s1) + (s2 + s3);
  if (g0 >= g1) return;
  if (e < K * N) {
    const int k = e / N, n = e - k * N;
    atomicAdd(dW + (size_t)k * ldw + n, sum);
  } else {
    atomicAdd(db + (e - K * N), sum);
  }
}

// Deferred second stage: dgppo_dense_bwd_w_deferred launches only the partial-slab kernel and hands the description of the
// pending reduction back to the caller, who flushes up to DGPPO_REDUCE_BATCH of them with ONE launch
// (dgppo_dense_bwd_w_reduce_batch; blockIdx.z = reduction).  A backward pass has ~12 weight gradients: 12 reduce launches
// of ~6 us become one.
static thread_local dgppo_reduce_desc* g_defer = nullptr;

struct ReduceBatch {
  int n;
  dgppo_reduce_desc d[DGPPO_REDUCE_BATCH];
};

__global__ void __launch_bounds__(256) dense_bwd_w_reduce_batch_kernel(ReduceBatch b) {
  const dgppo_reduce_desc& d = b.d[blockIdx.z];
  const int K = d.K, N = d.N, G = d.slabs;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int E = K * N + (d.db ? N : 0);
  if (e >= E) return;
  // the same split of the slabs over blockIdx.y as the single reduce kernel: splits meet in <= gridDim.y atomicAdds
  const int splits = min((int)gridDim.y, max(1, (G + REDUCE_SLABS_PER_SPLIT - 1) / REDUCE_SLABS_PER_SPLIT));
  if ((int)blockIdx.y >= splits) return;
  const int per = (G + splits - 1) / splits;
  const int g0 = blockIdx.y * per, g1 = min(G, g0 + per);
  if (g0 >= g1) return;
  const float* part = d.part;
  const size_t st = (size_t)d.part_stride;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int g = g0;
  for (; g + 3 < g1; g += 4) {
    s0 += part[(size_t)g * st + e]; s1 += part[(size_t)(g + 1) * st + e];
    s2 += part[(size_t)(g + 2) * st + e]; s3 += part[(size_t)(g + 3) * st + e];
  }
  for (; g < g1; ++g) s0 += part[(size_t)g * st + e];
  const float sum = (s0 + s1) + (s2 + s3);
  if (e < K * N) {
    const int k = e / N, n = e - k * N;
    atomicAdd(d.dW + (size_t)k * d.ldw + n, sum);
  } else {
    atomicAdd(d.db + (e - K * N), sum);
  }
}

// second stage of one weight gradient: launched now, or recorded for a batched launch
static void reduce_or_defer(hipStream_t s, const float* part, int stride, int grid, float* dW, int ldw, float* db, int K, int N) {
  if (g_defer != nullptr) {
    dgppo_reduce_desc& d = *g_defer;
    d.part = part; d.part_stride = stride; d.slabs = grid; d.dW = dW; d.ldw = ldw; d.db = db; d.K = K; d.N = N; d.pending = 1;
    return;
  }
  const int E = K * N + (db ? N : 0);
  int splits = cdiv(grid, REDUCE_SLABS_PER_SPLIT);
  splits = splits < 1 ? 1 : (splits > 64 ? 64 : splits);
  hipLaunchKernelGGL(dense_bwd_w_reduce_kernel, dim3(cdiv(E, 256), splits), dim3(256), 0, s, part, stride, grid, dW, ldw, db, K, N);
}

static int device_cus() {
  static thread_local int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  }
  return cus;
}

// 4-wave groups per workgroup of the slab path: as many as fit a CU's 160 KB of LDS with their tile buffers (what the CU
// would hold as separate workgroups), at most 4 (1024 threads); 1 where the tile buffers cannot carry the group exchange
template <int NT, int KT>
constexpr int bwd_w_groups() {
  constexpr int KTW = (KT + 3) / 4;
  constexpr int Kl = (KT & 1) ? KT * 16 : KT * 16 + 16;
  constexpr int Nl = (NT & 1) ? NT * 16 : NT * 16 + 16;
  constexpr int BUF2 = 2 * BW_ROWS * (Kl + Nl);
  constexpr int PFY = (BW_ROWS * NT * 4 + 255) / 256;
  constexpr int fit = (160 * 1024) / (BUF2 * 4);
  constexpr bool xch = KTW * NT * 4 * 256 + PFY * 4 * 256 <= BUF2;
  return (!xch || fit < 2) ? 1 : (fit > 4 ? 4 : fit);
}

// NGX: group count given by the caller (the DX sites, kXwSites below); 0 = what the tile buffers allow
template <int NT, int KT, bool DX = false, int NGX = 0, bool ACCM = false>
static void launch_bwd_w_kt(DenseBwdWArgs a, hipStream_t s) {
  constexpr int Kl = (KT & 1) ? KT * 16 : KT * 16 + 16;
  constexpr int Nl = (NT & 1) ? NT * 16 : NT * 16 + 16;
  // per group: the two X / dY buffers, and with DX the dX tile
  constexpr size_t smem = sizeof(float) * BW_ROWS * (2 * (Kl + Nl) + (DX ? XW_DL(KT) : 0));
  constexpr int NG = NGX > 0 ? NGX : bwd_w_groups<NT, KT>();
  static_assert(NG <= bwd_w_groups<NT, KT>(), "dense_bwd_w: more groups than the tile buffers and their exchange allow");
  static_assert(smem * NG <= 160 * 1024, "dense_bwd_w tiles exceed the 160 KB LDS of a gfx950 CU");
  static thread_local bool opted = false;
  if (!opted) {
    if (smem > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bwd_w_kernel<NT, KT, 1, DX, ACCM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (NG > 1 && smem * NG > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bwd_w_kernel<NT, KT, NG, DX, ACCM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(smem * NG));
    opted = true;
  }
  const int cus = device_cus();
  // rows per 4-wave group: NG groups on every CU, a multiple of the 32-row tile, at least two tiles
  int rpb = cdiv(a.M, NG * cus);
  rpb = ((rpb + BW_ROWS - 1) / BW_ROWS) * BW_ROWS;
  if (rpb < 2 * BW_ROWS) rpb = 2 * BW_ROWS;
  // up to one group per CU the groups stay workgroups of their own (a slab per CU either way, and every CU gets rows)
  const int ng = cdiv(a.M, rpb) > cus ? NG : 1;
  // partial slabs: stride rounded to 64 floats; shrink the grid if the scratch buffer cannot hold one slab per workgroup
  const int stride = ((a.K * a.N + a.N + 63) / 64) * 64;
  const size_t ws_bytes = a.ws_bytes;
  float* ws = cdiv(a.M, rpb) > 4 ? a.part : nullptr;
  if (ws) {
    const long max_slabs = (long)(ws_bytes / (sizeof(float) * stride));
    if (max_slabs < 8) ws = nullptr;
    else if (cdiv(a.M, rpb * ng) > max_slabs) rpb = ((cdiv(a.M, (int)max_slabs * ng) + BW_ROWS - 1) / BW_ROWS) * BW_ROWS;
  }
  a.rows_per_block = rpb;
  a.part = ws;
  a.part_stride = stride;
  const int grid = cdiv(a.M, rpb * ng);
  if (NG > 1 && ng > 1) hipLaunchKernelGGL((dense_bwd_w_kernel<NT, KT, NG, DX, ACCM>), dim3(grid), dim3(256 * NG), smem * NG, s, a);
  else hipLaunchKernelGGL((dense_bwd_w_kernel<NT, KT, 1, DX, ACCM>), dim3(grid), dim3(256), smem, s, a);
  if (ws) reduce_or_defer(s, ws, stride, grid, a.dW, a.ldw, a.db, a.K, a.N);
}

template <int NT>
static void launch_bwd_w(const DenseBwdWArgs& a, hipStream_t s) {
  const int kt = cdiv(a.K, 16);                    // padded-K instantiations: 16,32,48,64,96,128,144,192,256
  if (kt <= 1) launch_bwd_w_kt<NT, 1>(a, s);
  else if (kt == 2) launch_bwd_w_kt<NT, 2>(a, s);
  else if (kt == 3) launch_bwd_w_kt<NT, 3>(a, s);
  else if (kt == 4) launch_bwd_w_kt<NT, 4>(a, s);
  else if (kt <= 6) launch_bwd_w_kt<NT, 6>(a, s);
  else if (kt <= 8) launch_bwd_w_kt<NT, 8>(a, s);
  else if (kt == 9) launch_bwd_w_kt<NT, 9>(a, s);
  else if (kt <= 12) launch_bwd_w_kt<NT, 12>(a, s);
  else launch_bwd_w_kt<NT, 16>(a, s);
}

// ---- narrow weight gradients (K <= 16, N <= 64: dMcat of the first GNN layer, K = 8, N = 24) ------------------------
// A thread owns four output columns and all K rows of dW (4K accumulators) and walks its share of the M input rows: dY is
// read as coalesced 16-byte loads, X[m][0..K) is the same address for the N/4 threads of a row.  The row-lanes of a
// workgroup meet in LDS (float atomics, once per workgroup), the workgroup writes one partial slab, and the common
// second stage (dense_bwd_w_reduce_kernel) folds the slabs into dW / db.
template <int KMAX, bool VECX>
__global__ void __launch_bounds__(256) dense_bwd_w_smallk_kernel(DenseBwdWArgs a) {
  extern __shared__ float sP[];                     // [256][K*4 + 4 + 1]: every thread's accumulators, then summed per column
  const int K = a.K, N = a.N, nq = N >> 2;
  const int per = K * 4 + 4, Pl = per + 1;
  const int lanes = 256 / nq;                       // row-lanes of the workgroup
  const int rl = threadIdx.x / nq, cq = threadIdx.x - rl * nq;
  float4 acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 accb = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rl < lanes) {
    const int r0 = blockIdx.x * a.rows_per_block;
    const int r1 = min(a.M, r0 + a.rows_per_block);
    // UR rows in flight per thread: the loop is a chain of dependent loads otherwise (one row = 1 + K/4 requests)
    constexpr int UR = 4;
    for (int rb = r0 + rl; rb < r1; rb += lanes * UR) {
      float4 d[UR];
      float xv[UR][KMAX];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int r = rb + u * lanes;
        const bool in = r < r1;
        const int rr = in ? r : r0;
        d[u] = *reinterpret_cast<const float4*>(a.dY + (size_t)rr * a.ldy + cq * 4);
        if (!in) d[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* x = a.X + (size_t)rr * a.ldx;
        if (VECX) {
#pragma unroll
          for (int k4 = 0; k4 < KMAX / 4; ++k4) {
            if (k4 * 4 < K) {
              const float4 t = *reinterpret_cast<const float4*>(x + k4 * 4);
              xv[u][k4 * 4] = t.x; xv[u][k4 * 4 + 1] = t.y; xv[u][k4 * 4 + 2] = t.z; xv[u][k4 * 4 + 3] = t.w;
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < KMAX; ++k) if (k < K) xv[u][k] = x[k];
        }
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        accb.x += d[u].x; accb.y += d[u].y; accb.z += d[u].z; accb.w += d[u].w;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          if (k < K) {
            acc[k].x = fmaf(xv[u][k], d[u].x, acc[k].x); acc[k].y = fmaf(xv[u][k], d[u].y, acc[k].y);
            acc[k].z = fmaf(xv[u][k], d[u].z, acc[k].z); acc[k].w = fmaf(xv[u][k], d[u].w, acc[k].w);
          }
        }
      }
    }
  }
  float* mine = sP + threadIdx.x * Pl;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) { mine[k * 4] = acc[k].x; mine[k * 4 + 1] = acc[k].y; mine[k * 4 + 2] = acc[k].z; mine[k * 4 + 3] = acc[k].w; }
  }
  mine[K * 4] = accb.x; mine[K * 4 + 1] = accb.y; mine[K * 4 + 2] = accb.z; mine[K * 4 + 3] = accb.w;
  __syncthreads();
  // output element e = k*N + c (k == K: the bias row) is the sum over the row-lanes of thread (rl, cq = c/4), slot k*4 + c%4
  float* out = a.part + (size_t)blockIdx.x * a.part_stride;
  const int E = K * N + N;
  for (int e = threadIdx.x; e < E; e += 256) {
    const int k = e / N, c = e - k * N;
    const float* src = sP + (c >> 2) * Pl + k * 4 + (c & 3);
    float s0 = 0.f, s1 = 0.f;
    int l = 0;
    for (; l + 1 < lanes; l += 2) { s0 += src[(size_t)l * nq * Pl]; s1 += src[(size_t)(l + 1) * nq * Pl]; }
    if (l < lanes) s0 += src[(size_t)l * nq * Pl];
    out[e] = s0 + s1;
  }
}

static bool launch_bwd_w_smallk(DenseBwdWArgs a, hipStream_t s) {
  if (a.K > 16 || a.N > 64 || (a.N & 3) || (a.ldy & 3) || (reinterpret_cast<uintptr_t>(a.dY) & 15) || a.M < 4096)
    return false;
  const int stride = ((a.K * a.N + a.N + 63) / 64) * 64;
  const long max_slabs = a.part ? (long)(a.ws_bytes / (sizeof(float) * stride)) : 0;
  if (max_slabs < 8) return false;
  int grid = a.M >= (1 << 19) ? 1024 : 512;          // 2-4 workgroups per CU
  if (grid > max_slabs) grid = (int)max_slabs;
  int rpb = cdiv(a.M, grid);
  grid = cdiv(a.M, rpb);
  a.rows_per_block = rpb;
  a.part_stride = stride;
  const size_t smem = sizeof(float) * 256 * (a.K * 4 + 5);            // <= 69 KB
  const bool vx = (a.K & 3) == 0 && (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0;
  if (a.K <= 8) {
    if (vx) hipLaunchKernelGGL((dense_bwd_w_smallk_kernel<8, true>), dim3(grid), dim3(256), smem, s, a);
    else hipLaunchKernelGGL((dense_bwd_w_smallk_kernel<8, false>), dim3(grid), dim3(256), smem, s, a);
  } else {
    static thread_local bool opted = false;
    if (!opted) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bwd_w_smallk_kernel<16, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 256 * 69 * 4);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bwd_w_smallk_kernel<16, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 256 * 69 * 4);
      opted = true;
    }
    if (vx) hipLaunchKernelGGL((dense_bwd_w_smallk_kernel<16, true>), dim3(grid), dim3(256), smem, s, a);
    else hipLaunchKernelGGL((dense_bwd_w_smallk_kernel<16, false>), dim3(grid), dim3(256), smem, s, a);
  }
  reduce_or_defer(s, a.part, stride, grid, a.dW, a.ldw, a.db, a.K, a.N);
  return true;
}

int32_t dense_bwd_w_launch(DenseBwdWArgs a, hipStream_t s) {
  DGPPO_REQUIRE(a.M >= 0 && a.K >= 1 && a.N >= 1, "dense_bwd_w: bad shape");
  DGPPO_REQUIRE(a.N <= 192 && a.K <= 256, "dense_bwd_w: N <= 192 and K <= 256 supported (N=%d K=%d)", a.N, a.K);
  DGPPO_REQUIRE(a.X && a.dY && a.dW, "dense_bwd_w: NULL operand");
  DGPPO_REQUIRE(a.ldx >= a.K && a.ldy >= a.N && a.ldw >= a.N, "dense_bwd_w: leading dimensions too small");
  if (a.M == 0) return 0;
  const int nt = cdiv(a.N, 16);
  if (launch_bwd_w_smallk(a, s)) {}
  else if (nt <= 1) launch_bwd_w<1>(a, s);
  else if (nt <= 2) launch_bwd_w<2>(a, s);
  else if (nt <= 4) launch_bwd_w<4>(a, s);
  else if (nt <= 6) launch_bwd_w<6>(a, s);
  else launch_bwd_w<12>(a, s);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- input and weight gradient of a Dense from one pass (dgppo_dense_bwd_xw) ---------------------------------------------
// THE place that chooses between the fused kernel and the pair (dense_bwd_w, then dense_fwd with W^T): shape and alignment
// only.  The shapes are GNN glue Denses of the networks, each moved here after a measured per-call gain at 131 072 rows
// (profiles/README.md, rounds 7 and 10); everything else runs the pair.  Round 10, fused against the round-9 path, us per call:
// 144 x 64 81.5 -> 66.1, 48 x 32 25.2 -> 23.6, 48 x 64 41.7 -> 32.6, and the `+=` site 32 x 96 54.6 (the pair) -> 33.9 now that
// its four waves all multiply: 1.5 - 1.75 times the time of their bytes at 4.5 TB/s.
// The sites, in ONE table: shape, its tiles, the groups per CU (what 160 KB of LDS hold of two X / dY buffers and a dX tile per
// group, with rows that divide over groups x CUs: 3 groups would leave 28 CUs idle at 131 072 rows), and whether the `+=` form
// is fused too: at 144 x 64 it is not (no caller has it; with the old dX fragments the kernel would not fit 256 registers).
struct XwSite { int K, N, NT, KT, NG; bool ACC; };
constexpr XwSite kXwSites[] = {{144, 64, 4, 9, 2, false}, {48, 32, 2, 3, 4, true}, {48, 64, 4, 3, 2, true}, {32, 96, 6, 2, 2, true}};
constexpr int kXwSiteCount = sizeof(kXwSites) / sizeof(kXwSites[0]);

// what dense_bwd_w_kernel calls `vec`: the fused form exists only on the 16-byte staging path (its scalar path forms no dX)
static bool bwd_w_vec(const DenseBwdWArgs& a) {
  return (a.K & 3) == 0 && (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0 && (a.N & 3) == 0 && (a.ldy & 3) == 0 &&
         (reinterpret_cast<uintptr_t>(a.dY) & 15) == 0;
}

static bool bwd_xw_fused(const DenseBwdWArgs& a) {
  bool site = false;
  for (int i = 0; i < kXwSiteCount; ++i) site = site || (a.K == kXwSites[i].K && a.N == kXwSites[i].N && (kXwSites[i].ACC || !a.acc_mask));
  const uintptr_t p = reinterpret_cast<uintptr_t>(a.W) | reinterpret_cast<uintptr_t>(a.dX);
  return site && a.N <= 192 && bwd_w_vec(a) && ((a.ldwp | a.lddx) & 3) == 0 && (p & 15) == 0;
}

template <int I>
static void launch_xw_site(const DenseBwdWArgs& a, hipStream_t s) {
  if constexpr (I < kXwSiteCount) {
    constexpr XwSite S = kXwSites[I];
    static_assert(S.K == S.KT * 16 && S.N == S.NT * 16, "dense_bwd_xw: a site is whole 16-wide tiles (W^T and dY fragments are unguarded)");
    if (a.K != S.K || a.N != S.N) launch_xw_site<I + 1>(a, s);
    else if (!a.acc_mask) launch_bwd_w_kt<S.NT, S.KT, true, S.NG, false>(a, s);
    else if constexpr (S.ACC) launch_bwd_w_kt<S.NT, S.KT, true, S.NG, true>(a, s);
  }
}

static int32_t dense_bwd_xw_launch(DenseBwdWArgs a, hipStream_t s) {
  DGPPO_REQUIRE(a.M >= 0 && a.K >= 1 && a.N >= 1, "dense_bwd_xw: bad shape");
  DGPPO_REQUIRE(a.X && a.dY && a.dW && a.W && a.dX, "dense_bwd_xw: NULL operand");
  DGPPO_REQUIRE(a.ldx >= a.K && a.ldy >= a.N && a.ldw >= a.N && a.ldwp >= a.N && a.lddx >= a.K,
                "dense_bwd_xw: leading dimensions too small");
  if (a.M == 0) return 0;
  if (!bwd_xw_fused(a)) {
    const int32_t rc = dense_bwd_w_launch(a, s);
    if (rc) return rc;
    DenseArgs f{a.dY, a.ldy, a.W, a.ldwp, nullptr, a.dX, a.lddx, a.M, a.N, a.K, 0, a.acc_mask, 1, a.acc_mask ? a.X : nullptr, a.ldx};
    return dense_fwd_launch(f, s);
  }
  launch_xw_site<0>(a, s);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- GRU weight gradients in one pass ------------------------------------------------------------------------------------
//   dWi[64,192] += x^T dgi               dbi[192] += colsum(dgi)
//   dWh[64,192] += hprev^T [dgi[:, :128] | dhn]      dbhn[64] += colsum(dhn)      (hr / hz carry no bias)
// The same tiling as dense_bwd_w_kernel: 32-row tiles [x | hprev] (128 wide) and [dgi | dhn] (256 wide) double-buffered in
// LDS, the next tile's rows prefetched into registers while the current one is on the matrix cores, one LDS-only barrier per
// tile.  One 8-wave workgroup per CU: waves 0-3 accumulate dWi (A = x), waves 4-7 dWh (A = hprev, B = the r / z columns of
// dgi and dhn) from the SAME tiles, wave w of either half owning output rows 16w..16w+15 x all 12 column tiles.  Every input
// row is read once (384 floats; the three dense_bwd_w calls this replaces read 576), and a CU writes one slab
// [dWi | dbi | dWh | dbhn] for the common second stage.
#define GW_AL 144          // [x | hprev] row: 128 + 16, stride = 16 (mod 32) as in dense_bwd_w_kernel
#define GW_YL 272          // [dgi | dhn] row: 256 + 16
#define GW_BUF (BW_ROWS * (GW_AL + GW_YL))
#define GW_SLAB_WI 0
#define GW_SLAB_BI (64 * 192)
#define GW_SLAB_WH (64 * 192 + 192)
#define GW_SLAB_BHN (2 * 64 * 192 + 192)
#define GW_SLAB (2 * 64 * 192 + 192 + 64)     // 24832 floats, a multiple of 64
struct GruBwdWArgs {
  const float* x; int ldx;
  const float* hprev; int ldh;
  const float* dgi;       // [M,192] dense
  const float* dhn;       // [M,64] dense
  float* dWi; int ldwi;
  float* dbi;
  float* dWh; int ldwh;
  float* dbhn;
  int M, rows_per_block;
  float* part;            // [grid][GW_SLAB] or NULL: atomicAdd straight into the outputs
  // T1 only (hprev is h0; dgi / dhn above are unused): the gate gradients are formed here
  const float* dhs;       // [M,64] dense
  const float* gates;     // [M,256] dense (r | z | n | hn)
  float* dgi_out;         // [M,192] dense
  GruH0Map hmap;          // n_inner.d > 0: row m of h0 is read through the carry map (nn_gru.h) instead of hprev + m * ldh
};

// T1: the one-step GRU backward inside the pass.  With T = 1 the scan (gru_bwd_kernel) is elementwise in (dhs, gates, h0), so
// the [dgi | dhn] tile is formed on chip instead of being written by the scan and read back: thread (row tid/16, column quad
// tid%16) loads d, h0, r, z, n, hn of its four columns once (six 16-byte loads), forms all four gradient quads with
// gru_gate_grad (the scan's expressions: the same bits), stages them and stores dgi's three for the trunk's backward.  dhn
// never reaches memory.  The MFMA loop, the slabs and the epilogue are the same code.
template <bool T1>
__global__ void __launch_bounds__(512) gru_bwd_w_kernel(GruBwdWArgs a) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, half = tid >> 8;
  const int li = lane & 15, lq = lane >> 4;
  const int m_begin = blockIdx.x * a.rows_per_block;
  const int m_end = min(a.M, m_begin + a.rows_per_block);
  f32x4 acc[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // float4 slots of a tile: [x | hprev] 32 rows x 32 quads (2 per thread), [dgi | dhn] 32 rows x 64 quads (4 per thread);
  // a thread's four [dgi | dhn] slots are the SAME column quad (512 = 8 rows x 64 quads), so one float4 carries its column sums
  // T1: one (row, column quad) per thread; pfy = d, h0, r, z, n, hn and one column-sum quad per block of [dgi | dhn]
  float4 pfa[2], pfy[T1 ? 6 : 4];
  float4 csum[T1 ? 4 : 1];
#pragma unroll
  for (int u = 0; u < (T1 ? 4 : 1); ++u) csum[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int qa = tid & 31, ra = tid >> 5, qy = tid & 63, ry = tid >> 6;
  const int q1 = tid & 15, r1 = tid >> 4;
  // T1: h0 may be a record read in place (one address per tile row and thread, two integer divisions; the loads stay 16 bytes)
  auto hrow = [&](int row) -> const float* {
    if constexpr (T1) { if (a.hmap.n_inner.d > 0) return gru_h0_map_row(a.hprev, a.hmap, row); }
    return a.hprev + (size_t)row * a.ldh;
  };
  auto fetch = [&](int m0) {            // rows clamped; masking happens in commit
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int row = m0 + u * 16 + ra;
      row = row < a.M ? row : a.M - 1;
      const float* src = qa < 16 ? a.x + (size_t)row * a.ldx + 4 * qa : hrow(row) + 4 * (qa - 16);
      pfa[u] = *reinterpret_cast<const float4*>(src);
    }
    if constexpr (T1) {
      int row = m0 + r1;
      row = row < a.M ? row : a.M - 1;
      pfy[0] = *reinterpret_cast<const float4*>(a.dhs + (size_t)row * 64 + 4 * q1);
      pfy[1] = *reinterpret_cast<const float4*>(hrow(row) + 4 * q1);
      const float* gs = a.gates + (size_t)row * 256 + 4 * q1;
#pragma unroll
      for (int g = 0; g < 4; ++g) pfy[2 + g] = *reinterpret_cast<const float4*>(gs + 64 * g);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int row = m0 + u * 8 + ry;
        row = row < a.M ? row : a.M - 1;
        const float* src = qy < 48 ? a.dgi + (size_t)row * 192 + 4 * qy : a.dhn + (size_t)row * 64 + 4 * (qy - 48);
        pfy[u] = *reinterpret_cast<const float4*>(src);
      }
    }
  };
  auto commit = [&](int m0, int b) {    // registers -> LDS buffer b; rows >= m_end become zeros
    float* as = sm + b * GW_BUF;
    float* ys = as + BW_ROWS * GW_AL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = u * 16 + ra;
      const float4 v = (m0 + r < m_end) ? pfa[u] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(as + r * GW_AL + 4 * qa) = v;
    }
    if constexpr (T1) {
      const bool in = m0 + r1 < m_end;
      // the scan's d = dh + dhs with its zero-initialised dh
      const GruGateGrad g0 = gru_gate_grad(gru_zero_carry(pfy[0].x), pfy[1].x, pfy[2].x, pfy[3].x, pfy[4].x, pfy[5].x);
      const GruGateGrad g1 = gru_gate_grad(gru_zero_carry(pfy[0].y), pfy[1].y, pfy[2].y, pfy[3].y, pfy[4].y, pfy[5].y);
      const GruGateGrad g2 = gru_gate_grad(gru_zero_carry(pfy[0].z), pfy[1].z, pfy[2].z, pfy[3].z, pfy[4].z, pfy[5].z);
      const GruGateGrad g3 = gru_gate_grad(gru_zero_carry(pfy[0].w), pfy[1].w, pfy[2].w, pfy[3].w, pfy[4].w, pfy[5].w);
      float4 v[4] = {make_float4(g0.dar, g1.dar, g2.dar, g3.dar), make_float4(g0.daz, g1.daz, g2.daz, g3.daz),
                     make_float4(g0.dan, g1.dan, g2.dan, g3.dan), make_float4(g0.dhn, g1.dhn, g2.dhn, g3.dhn)};
      if (in) {
        float* o = a.dgi_out + (size_t)(m0 + r1) * 192 + 4 * q1;
#pragma unroll
        for (int g = 0; g < 3; ++g) *reinterpret_cast<float4*>(o + 64 * g) = v[g];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (!in) v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(ys + r1 * GW_YL + 64 * g + 4 * q1) = v[g];
        csum[g].x += v[g].x; csum[g].y += v[g].y; csum[g].z += v[g].z; csum[g].w += v[g].w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = u * 8 + ry;
        const float4 v = (m0 + r < m_end) ? pfy[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(ys + r * GW_YL + 4 * qy) = v;
        csum[0].x += v.x; csum[0].y += v.y; csum[0].z += v.z; csum[0].w += v.w;
      }
    }
  };
  auto compute = [&](int b) {
    // A[i = k][kk = m] = [x | hprev][m][64 half + 16 wave + k], B[kk = m][j] = [dgi | dhn][m][column tile]
    const float* as = sm + b * GW_BUF + lq * GW_AL + half * 64 + wave * 16 + li;
    const float* ys = sm + b * GW_BUF + BW_ROWS * GW_AL + lq * GW_YL + li;
    const float* yh = ys + (half ? 64 : 0);              // dWh's column tiles 8..11 are dhn: LDS columns 192..255
#pragma unroll
    for (int s4 = 0; s4 < BW_ROWS / 4; ++s4) {
      float bv[12];
#pragma unroll
      for (int t = 0; t < 8; ++t) bv[t] = ys[s4 * 4 * GW_YL + t * 16];
#pragma unroll
      for (int t = 8; t < 12; ++t) bv[t] = yh[s4 * 4 * GW_YL + t * 16];
      const float av = as[s4 * 4 * GW_AL];
#pragma unroll
      for (int t = 0; t < 12; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
    }
  };
  fetch(m_begin);
  commit(m_begin, 0);
  __syncthreads();
  int cur = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += BW_ROWS) {
    fetch(m0 + BW_ROWS);                                   // past m_end on the last round: masked to zeros in commit
    __builtin_amdgcn_sched_barrier(0);
    compute(cur);
    commit(m0 + BW_ROWS, cur ^ 1);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    cur ^= 1;
  }
  float* slab = a.part ? a.part + (size_t)blockIdx.x * GW_SLAB : nullptr;
  {
    float* out = half ? a.dWh : a.dWi;
    const int ldo = half ? a.ldwh : a.ldwi;
    float* sl = slab ? slab + (half ? GW_SLAB_WH : GW_SLAB_WI) : nullptr;
#pragma unroll
    for (int t = 0; t < 12; ++t) {
      const int col = t * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = wave * 16 + lq * 4 + r;
        if (sl) sl[krow * 192 + col] = acc[t][r];
        else atomicAdd(out + (size_t)krow * ldo + col, acc[t][r]);
      }
    }
  }
  // column sums: red[row slot 0..7 (T1: 0..31)][256 columns] through LDS (the tile buffers are idle now)
  __syncthreads();
  if constexpr (T1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(sm + r1 * 256 + 64 * g + 4 * q1) = csum[g];
  } else {
    *reinterpret_cast<float4*>(sm + ry * 256 + 4 * qy) = csum[0];
  }
  __syncthreads();
  if (tid < 256) {
    float cs = 0.0f;
#pragma unroll
    for (int r = 0; r < (T1 ? 32 : 8); ++r) cs += sm[r * 256 + tid];
    if (tid < 192) {
      if (slab) slab[GW_SLAB_BI + tid] = cs;
      else atomicAdd(a.dbi + tid, cs);
    } else {
      if (slab) slab[GW_SLAB_BHN + tid - 192] = cs;
      else atomicAdd(a.dbhn + tid - 192, cs);
    }
  }
}

extern "C" int64_t dgppo_gru_bwd_w_workspace_bytes(void) { return (int64_t)GW_SLAB * sizeof(float) * device_cus(); }

template <bool T1>
static int32_t gru_bwd_w_launch(GruBwdWArgs a, float* workspace, int64_t workspace_bytes, dgppo_reduce_desc* pending,
                                hipStream_t s) {
  const int M = a.M;
  DGPPO_REQUIRE(M >= 0, "gru_bwd_w: bad M");
  DGPPO_REQUIRE(a.x && a.hprev && a.dWi && a.dbi && a.dWh && a.dbhn, "gru_bwd_w: NULL operand");
  DGPPO_REQUIRE(T1 ? (a.dhs && a.gates && a.dgi_out) : (a.dgi && a.dhn), "gru_bwd_w: NULL operand");
  DGPPO_REQUIRE(a.ldx >= 64 && a.ldh >= 64 && a.ldwi >= 192 && a.ldwh >= 192, "gru_bwd_w: leading dimensions too small");
  DGPPO_REQUIRE((a.ldx & 3) == 0 && (a.ldh & 3) == 0 &&
                ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.hprev) | reinterpret_cast<uintptr_t>(a.dgi) |
                  reinterpret_cast<uintptr_t>(a.dhn) | reinterpret_cast<uintptr_t>(a.dhs) | reinterpret_cast<uintptr_t>(a.gates) |
                  reinterpret_cast<uintptr_t>(a.dgi_out)) & 15) == 0,
                "gru_bwd_w: the row operands must be 16-byte aligned with leading dimensions that are multiples of 4");
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "gru_bwd_w: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "gru_bwd_w: workspace must be 16-byte aligned");
  if (pending) pending[0].pending = pending[1].pending = pending[2].pending = 0;
  if (M == 0) return 0;
  constexpr size_t smem = 2 * sizeof(float) * GW_BUF;
  static_assert(smem <= 160 * 1024, "gru_bwd_w tiles exceed the 160 KB LDS of a gfx950 CU");
  static_assert(32 * 256 <= 2 * GW_BUF, "gru_bwd_w: the column-sum exchange does not fit the tile buffers");
  static thread_local bool opted = false;
  if (!opted) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gru_bwd_w_kernel<T1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    opted = true;
  }
  // one workgroup per CU; rows per workgroup a multiple of the 32-row tile, at least two tiles
  int rpb = cdiv(M, device_cus());
  rpb = ((rpb + BW_ROWS - 1) / BW_ROWS) * BW_ROWS;
  if (rpb < 2 * BW_ROWS) rpb = 2 * BW_ROWS;
  float* ws = cdiv(M, rpb) > 4 ? workspace : nullptr;      // <= 4 workgroups: atomicAdd, as dense_bwd_w
  if (ws) {
    const long max_slabs = (long)(workspace_bytes / (sizeof(float) * GW_SLAB));
    if (max_slabs < 8) ws = nullptr;
    else if (cdiv(M, rpb) > max_slabs) rpb = ((cdiv(M, (int)max_slabs) + BW_ROWS - 1) / BW_ROWS) * BW_ROWS;
  }
  const int grid = cdiv(M, rpb);
  a.rows_per_block = rpb;
  a.part = ws;
  hipLaunchKernelGGL(gru_bwd_w_kernel<T1>, dim3(grid), dim3(512), smem, s, a);
  DGPPO_LAUNCH_CHECK();
  if (!ws) return 0;
  // second stage: dWi with its bias row, dWh without one, dbhn as a [1,64] matrix
  dgppo_reduce_desc d[3];
  d[0] = dgppo_reduce_desc{ws + GW_SLAB_WI, a.dWi, a.dbi, GW_SLAB, grid, a.ldwi, 64, 192, 1};
  d[1] = dgppo_reduce_desc{ws + GW_SLAB_WH, a.dWh, nullptr, GW_SLAB, grid, a.ldwh, 64, 192, 1};
  d[2] = dgppo_reduce_desc{ws + GW_SLAB_BHN, a.dbhn, nullptr, GW_SLAB, grid, 64, 1, 64, 1};
  if (pending) {
    pending[0] = d[0]; pending[1] = d[1]; pending[2] = d[2];
    return 0;
  }
  return dgppo_dense_bwd_w_reduce_batch(d, 3, (void*)s);
}

extern "C" int32_t dgppo_gru_bwd_w(const float* x, int32_t ldx, const float* hprev, int32_t ldh, const float* dgi,
                                   const float* dhn, float* dWi, int32_t ldwi, float* dbi, float* dWh, int32_t ldwh,
                                   float* dbhn, int32_t M, float* workspace, int64_t workspace_bytes,
                                   dgppo_reduce_desc* pending, void* stream) {
  GruBwdWArgs a{};
  a.x = x; a.ldx = ldx; a.hprev = hprev; a.ldh = ldh; a.dgi = dgi; a.dhn = dhn;
  a.dWi = dWi; a.ldwi = ldwi; a.dbi = dbi; a.dWh = dWh; a.ldwh = ldwh; a.dbhn = dbhn; a.M = M;
  return gru_bwd_w_launch<false>(a, workspace, workspace_bytes, pending, (hipStream_t)stream);
}

extern "C" int32_t dgppo_gru_bwd_w_t1(const float* x, int32_t ldx, const float* h0, int32_t ldh, const float* dhs,
                                      const float* gates, float* dgi, float* dWi, int32_t ldwi, float* dbi, float* dWh,
                                      int32_t ldwh, float* dbhn, int32_t M, float* workspace, int64_t workspace_bytes,
                                      dgppo_reduce_desc* pending, void* stream) {
  GruBwdWArgs a{};
  a.x = x; a.ldx = ldx; a.hprev = h0; a.ldh = ldh; a.dhs = dhs; a.gates = gates; a.dgi_out = dgi;
  a.dWi = dWi; a.ldwi = ldwi; a.dbi = dbi; a.dWh = dWh; a.ldwh = ldwh; a.dbhn = dbhn; a.M = M;
  return gru_bwd_w_launch<true>(a, workspace, workspace_bytes, pending, (hipStream_t)stream);
}

extern "C" int32_t dgppo_gru_bwd_w_t1_map(const float* x, int32_t ldx, const float* h0, const int32_t* ids, int32_t n_env,
                                          int32_t n_time, int32_t n_inner, int64_t env_stride, int64_t time_stride,
                                          const float* dhs, const float* gates, float* dgi, float* dWi, int32_t ldwi,
                                          float* dbi, float* dWh, int32_t ldwh, float* dbhn, int32_t M, float* workspace,
                                          int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream) {
  GruBwdWArgs a{};
  a.x = x; a.ldx = ldx; a.hprev = h0; a.ldh = 64; a.dhs = dhs; a.gates = gates; a.dgi_out = dgi;
  a.dWi = dWi; a.ldwi = ldwi; a.dbi = dbi; a.dWh = dWh; a.ldwh = ldwh; a.dbhn = dbhn; a.M = M;
  DGPPO_REQUIRE(n_env >= 1 && n_time >= 1 && n_inner >= 1, "gru_bwd_w_t1_map: bad sizes n_env=%d n_time=%d n_inner=%d", n_env,
                n_time, n_inner);
  DGPPO_REQUIRE(env_stride % 4 == 0 && time_stride % 4 == 0 && env_stride >= 0 && time_stride >= 0,
                "gru_bwd_w_t1_map: env_stride and time_stride must be non-negative multiples of 4 floats");
  DGPPO_REQUIRE((int64_t)M <= (int64_t)n_env * n_time * n_inner, "gru_bwd_w_t1_map: the map holds fewer than M = %d carries", M);
  a.hmap = gru_h0_map(ids, (long)env_stride, (long)time_stride, n_inner, n_time);
  return gru_bwd_w_launch<true>(a, workspace, workspace_bytes, pending, (hipStream_t)stream);
}

extern "C" int32_t dgppo_dense_fwd(const float* X, int32_t ldx, const float* W, int32_t ldw, const float* bias, float* Y,
                                   int32_t ldy, int32_t M, int32_t K, int32_t N, int32_t act, int32_t accumulate,
                                   int32_t trans_w, const float* relu_mask, int32_t ldm, void* stream) {
  DGPPO_REQUIRE(relu_mask == nullptr || ldm >= N, "dense: mask leading dimension too small");
  DenseArgs a{X, ldx, W, ldw, bias, Y, ldy, M, K, N, act, accumulate, trans_w, relu_mask, ldm};
  return dense_fwd_launch(a, (hipStream_t)stream);
}

extern "C" int32_t dgppo_dense_bwd_w(const float* X, int32_t ldx, const float* dY, int32_t ldy, float* dW, int32_t ldw,
                                     float* db, int32_t M, int32_t K, int32_t N, float* workspace, int64_t workspace_bytes,
                                     void* stream) {
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "dense_bwd_w: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dense_bwd_w: workspace must be 16-byte aligned");
  DenseBwdWArgs a{X, ldx, dY, ldy, dW, ldw, db, M, K, N, 0, workspace, 0, (size_t)workspace_bytes};
  return dense_bwd_w_launch(a, (hipStream_t)stream);
}

extern "C" int32_t dgppo_dense_bwd_w_deferred(const float* X, int32_t ldx, const float* dY, int32_t ldy, float* dW,
                                              int32_t ldw, float* db, int32_t M, int32_t K, int32_t N, float* workspace,
                                              int64_t workspace_bytes, dgppo_reduce_desc* pending, void* stream) {
  DGPPO_REQUIRE(pending != nullptr, "dense_bwd_w_deferred: pending is NULL");
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "dense_bwd_w: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dense_bwd_w: workspace must be 16-byte aligned");
  pending->pending = 0;
  DenseBwdWArgs a{X, ldx, dY, ldy, dW, ldw, db, M, K, N, 0, workspace, 0, (size_t)workspace_bytes};
  g_defer = pending;
  const int32_t rc = dense_bwd_w_launch(a, (hipStream_t)stream);
  g_defer = nullptr;
  return rc;
}

extern "C" int32_t dgppo_dense_bwd_xw(const float* X, int32_t ldx, const float* dY, int32_t ldy, const float* W, int32_t ldw,
                                      float* dX, int32_t lddx, int32_t accumulate_mask, float* dW, int32_t lddw, float* db,
                                      int32_t M, int32_t K, int32_t N, float* workspace, int64_t workspace_bytes,
                                      dgppo_reduce_desc* pending, void* stream) {
  DGPPO_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "dense_bwd_xw: bad workspace");
  DGPPO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dense_bwd_xw: workspace must be 16-byte aligned");
  if (pending) pending->pending = 0;
  DenseBwdWArgs a{X, ldx, dY, ldy, dW, lddw, db, M, K, N, 0, workspace, 0, (size_t)workspace_bytes, W, ldw, dX, lddx,
                  accumulate_mask ? 1 : 0};
  g_defer = pending;
  const int32_t rc = dense_bwd_xw_launch(a, (hipStream_t)stream);
  g_defer = nullptr;
  return rc;
}

extern "C" int32_t dgppo_dense_bwd_w_reduce_batch(const dgppo_reduce_desc* descs, int32_t n, void* stream) {
  DGPPO_REQUIRE(n >= 0 && (n == 0 || descs != nullptr), "dense_bwd_w_reduce_batch: bad arguments");
  for (int32_t i0 = 0; i0 < n; i0 += DGPPO_REDUCE_BATCH) {
    ReduceBatch b;
    b.n = 0;
    int emax = 0, gmax = 0;
    for (int32_t i = i0; i < n && b.n < DGPPO_REDUCE_BATCH; ++i) {
      if (!descs[i].pending) continue;
      DGPPO_REQUIRE(descs[i].part && descs[i].dW && descs[i].slabs >= 1 && descs[i].K >= 1 && descs[i].N >= 1,
                    "dense_bwd_w_reduce_batch: bad descriptor %d", i);
      b.d[b.n++] = descs[i];
      const int E = descs[i].K * descs[i].N + (descs[i].db ? descs[i].N : 0);
      emax = E > emax ? E : emax;
      gmax = descs[i].slabs > gmax ? descs[i].slabs : gmax;
    }
    if (b.n == 0) continue;
    int splits = cdiv(gmax, REDUCE_SLABS_PER_SPLIT);
    splits = splits < 1 ? 1 : (splits > 64 ? 64 : splits);
    hipLaunchKernelGGL(dense_bwd_w_reduce_batch_kernel, dim3(cdiv(emax, 256), splits, b.n), dim3(256), 0, (hipStream_t)stream, b);
  }
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// one slab of K*N + N floats (rounded to 64) per workgroup: the MFMA kernels launch at most one per CU, the narrow-K
// kernel up to 1024
extern "C" int64_t dgppo_dense_bwd_w_workspace_bytes(int32_t K, int32_t N) {
  if (K < 1 || N < 1) return 0;
  const int64_t stride = (((int64_t)K * N + N + 63) / 64) * 64;
  return stride * 1024 * (int64_t)sizeof(float);
}
