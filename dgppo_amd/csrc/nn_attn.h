// Attention side of the GraphTransformer layer (dgppo/nn/gnn.py:78-117) in per-agent fixed-fan-in form: what the kernel families
// (attn_wg.hip, attn_slot8.hip, attn_bd.hip, attn_tiled.hip) and their dispatch (attn.hip) share.  Device code only (HIP
// intrinsics): include it from the attention translation units, never from common.h.
//
// Only agents receive messages and every sender slot of an agent has a static node id (SURVEY F5/F7;
// dgppo/utils/graph.py:35-44, dgppo/env/lidar_env/lidar_spread.py:57-96), so jraph.segment_softmax / segment_sum over
// the flat edge list reduce to a masked softmax over S = n + goal_slots + obs_slots slots per agent.  Masked edges are
// re-routed pad->pad in the reference and therefore never reach an agent: here they are simply excluded.
//
// Algebraic form (same function, different summation order; see DESIGN.md "GNN layer"):
//   logit[i,s,h] = <q_h(x_i), k_h(x_s)>/sqrt(D) = qt[i,h,:] . x_s + const(i,h)   with qt = x_i Mcat + c   (dense, outside)
//   sum_s a[i,s,h] (v_h(x_s) + e_h(edge_is)) = (sum_s a[i,s,h] [x_s ; edge_is]) [Wv_h ; We_h] + bv_h   (dense, outside)
// so the attention kernels only do: logits against RAW sender features, masked softmax, aggregation of raw features, and the
// matching backward (the graph features come from graph_feats.hip).  const(i,h) (the key bias) cancels in the softmax.
#pragma once
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
// operands of every attention kernel
// ---------------------------------------------------------------------------------------------------------------------
#define ABD_DW_STRIDE 320              // 8 x 32 (dWo) + 32 (dbo), rounded to 64 floats
struct AttnArgs {
  Topo t;
  int F, H, Kp;          // feature width of this layer's inputs, heads, padded width of zcat
  const float* qt;       // [G*n, H*F]
  const float* Xa;       // [G*n, F]
  const float* Xo;       // [G*(Ns-n), F]
  const float* efeat;    // [G*n, S, 4]   (slot-sparse kernels, dgppo_attn_fwd_rows / _bwd_rows: NULL = differences of the node rows)
  const float* emask;    // [G*n, S]
  float* zcat;           // [G*n, Kp]   = [x_i | per head: sum a x_s (F), sum a e (4) | 1 | 0-pad]
  float* attn;           // [G*n, S, H]   (slot-sparse backward, dgppo_attn_bwd_rows: NULL = formed again from qt and emask)
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

using f32x4g = __attribute__((ext_vector_type(4))) float;

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

__device__ inline void put4(float* d, float4 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }

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

// ---- the kernel families: shape predicates and launchers, one translation unit each; attn_family (attn.hip) chooses ----
// (hidden: several translation units need them, the library exports the C ABI of include/dgppo_hip.h alone)
#pragma GCC visibility push(hidden)
size_t attn_image_bytes(const Topo& t, int F, int H, bool bwd);                // attn.hip: whole-graph LDS image of the VALU family
size_t attn_mfma_smem(const Topo& t, int F, int H, bool bwd);                  // attn_wg.hip
void launch_attn_wg(const AttnArgs& a, hipStream_t s, bool bwd, bool mfma);
bool attn_slot8_shape(const Topo& t, int F, int H);                            // attn_slot8.hip
bool attn_slot8_rows_ok(const dgppo_env_cfg& c, const Topo& t, int F, int H);   // may efeat (and, backward, attn) be left out?
bool launch_attn_slot8(const AttnArgs& a, hipStream_t s, bool bwd);
bool attn_bd_shape(const Topo& t, int F, int H, int& PS, bool& hits);          // attn_bd.hip
bool launch_attn_bd(const AttnArgs& a, hipStream_t s, bool bwd);
void launch_attn_xo_dw_reduce(const float* slab, int G, float* dWo, int lddwo, float* dbo, hipStream_t s);
int32_t launch_attn_tiled(AttnArgs& a, hipStream_t s, bool bwd);               // attn_tiled.hip
#pragma GCC visibility pop
