// Attention entry points: operand checks, the choice of the kernel family by shape, and the launch through the family's
// launcher (nn_attn.h).
#include "nn_attn.h"

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
//   SLOT8  F = 8, H = 3, n <= 32, S <= 64 (attn_slot8_shape); the backward writes no input gradient (first layer only);
//          the only family that can do without efeat and without saved weights (dgppo_attn_fwd_rows / _bwd_rows below)
//   BD     F = 32 block-diagonal topologies (attn_bd_shape)
//   MFMA   one workgroup per graph on the matrix cores: F % 4 == 0, Kp % 4 == 0, S <= 64, LDS image <= 64 KB; backward for
//          F >= 16 only
//   VALU   one workgroup per graph, every other shape (and the narrow backward, where it beats MFMA: measured)
// Before any of them:
//   TILED  one workgroup per graph, receivers in tiles: every shape whose whole-graph image (attn_image_bytes, the VALU family's)
//          exceeds 64 KB, i.e. teams above ~17-35 agents depending on the kind (such calls were refused before this family
//          existed, so every other shape keeps its family); forward and backward cross that line at different n, the attn /
//          zcat layouts are the contract between the families
// SLOT8, BD and MFMA move zcat / dzcat rows in 16-byte pieces, hence Kp % 4 == 0: any other width takes the VALU (or TILED)
// kernels, which address single floats.
enum class AttnFamily { SLOT8, BD, MFMA, VALU, TILED };
size_t attn_image_bytes(const Topo& t, int F, int H, bool bwd) {
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
  if ((F & 3) == 0 && (Kp & 3) == 0 && t.S <= 64 && attn_mfma_smem(t, F, H, bwd) <= 64 * 1024 && (!bwd || F >= 16)) return AttnFamily::MFMA;
  return AttnFamily::VALU;
}

// the launch through the family's launcher, once for both directions; who = the entry point's name in the messages
static int32_t attn_launch(AttnFamily fam, AttnArgs& a, void* stream, bool bwd, const char* who) {
  const hipStream_t s = (hipStream_t)stream;
  bool launched = true;
  switch (fam) {
    case AttnFamily::SLOT8: launched = launch_attn_slot8(a, s, bwd); break;
    case AttnFamily::BD: launched = launch_attn_bd(a, s, bwd); break;
    case AttnFamily::MFMA: launch_attn_wg(a, s, bwd, true); break;
    case AttnFamily::VALU: launch_attn_wg(a, s, bwd, false); break;
    case AttnFamily::TILED: {
      const int32_t rc = launch_attn_tiled(a, s, bwd);
      if (rc) return rc;
      break;
    }
  }
  DGPPO_REQUIRE(launched, "%s: dispatch failed", who);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
// operands of a forward / a backward call (Xo = NULL: rows recomputed, see attn_set_xo)
static void attn_set_fwd(AttnArgs& a, const float* qt, const float* Xa, const float* Xo, const float* efeat, const float* emask,
                         float* zcat, float* attn) {
  a.qt = qt; a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.emask = emask; a.zcat = zcat; a.attn = attn;
}
static void attn_set_bwd(AttnArgs& a, const float* dzcat, const float* attn, const float* qt, const float* Xa, const float* Xo,
                         const float* efeat, float* dqt, float* dXa, float* dXo) {
  a.dzcat = dzcat; a.attn = (float*)attn; a.qt = qt; a.Xa = Xa; a.Xo = Xo; a.efeat = efeat; a.dqt = dqt; a.dXa = dXa; a.dXo = dXo;
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
  attn_set_fwd(a, qt, Xa, Xo, efeat, emask, zcat, attn);
  return attn_launch(attn_family(a.t, F, H, Kp, false, false), a, stream, false, "attn_fwd");
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
  attn_set_bwd(a, dzcat, attn, qt, Xa, Xo, efeat, dqt, dXa, dXo);
  const AttnFamily fam = attn_family(a.t, F, H, Kp, true, dXa != nullptr);
  a.relu_xo = (relu_xo && dXo && fam == AttnFamily::BD) ? 1 : 0;     // fused into the block-diagonal kernel's dXo store
  rc = attn_launch(fam, a, stream, true, "attn_bwd");
  if (rc) return rc;
  if (relu_xo && dXo && !a.relu_xo)    // the workgroup kernels do not fuse the ReLU mask of the other nodes' gradient: separate pass
    return dgppo_relu_bwd(dXo, Xo, (int64_t)G * (a.t.Ns - a.t.n) * F, stream);
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
// the last check of the three entry points below, and the operands of the recomputation
static int32_t attn_set_xo(AttnArgs& a, const float* Xo_raw, const float* Wo, int ldwo, const float* bo, const char* who) {
  DGPPO_REQUIRE(attn_xo_ok(a.t, a.F, a.H, a.Kp), "%s: no fused kernel for this topology (ask dgppo_attn_xo_supported)", who);
  a.Xo_raw = Xo_raw; a.Wo = Wo; a.ldwo = ldwo; a.bo = bo;
  return 0;
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
  rc = attn_set_xo(a, Xo_raw, Wo, ldwo, bo, "attn_fwd_xo");
  if (rc) return rc;
  attn_set_fwd(a, qt, Xa, nullptr, efeat, emask, zcat, attn);
  return attn_launch(AttnFamily::BD, a, stream, false, "attn_fwd_xo");
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
  rc = attn_set_xo(a, Xo_raw, Wo, ldwo, bo, "attn_bwd_xo");
  if (rc) return rc;
  attn_set_bwd(a, dzcat, attn, qt, Xa, nullptr, efeat, dqt, dXa, dXo);
  a.relu_xo = (relu_xo && dXo) ? 1 : 0;
  return attn_launch(AttnFamily::BD, a, stream, true, "attn_bwd_xo");
}

// ---- the first layer without its redundant operands (slot-sparse kernels only) --------------------------------------------
// On the kinds with a 4-float state the node rows carry the state verbatim in columns 0..3, and graph_feats.hip / the act-step
// kernel form a slot's edge feature as the single rounded difference of those columns (z = w = 0 on a LiDAR hit slot).  The
// slot-sparse kernels hold both rows in registers, so they subtract instead of reading efeat; and their backward forms the
// weights again from qt and emask instead of reading what a training forward would have had to write.
// dgppo_attn_rows_supported tells the caller whether (cfg, F, H) has these modes; every other family and shape refuses them here.
static bool attn_rows_ok(const dgppo_env_cfg& c, const Topo& t, int F, int H, int Kp) {
  return attn_slot8_rows_ok(c, t, F, H) && attn_family(t, F, H, Kp, false, false) == AttnFamily::SLOT8 &&
         attn_family(t, F, H, Kp, true, false) == AttnFamily::SLOT8;
}
extern "C" int32_t dgppo_attn_rows_supported(const dgppo_env_cfg* cfg, int32_t F, int32_t H) {
  AttnArgs a{};
  const int Kp = (F + H * (F + 4) + 1 + 3) / 4 * 4;         // the width the callers pad zcat to; any Kp % 4 == 0 is taken
  if (F < 1 || H < 1 || attn_check(cfg, F, H, Kp, 0, a)) return 0;
  return attn_rows_ok(*cfg, a.t, F, H, Kp) ? 1 : 0;
}
extern "C" int32_t dgppo_attn_fwd_rows(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* qt,
                                       const float* Xa, const float* Xo, const float* emask, float* zcat, float* attn,
                                       int32_t G, void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  DGPPO_REQUIRE(attn_rows_ok(*cfg, a.t, F, H, Kp), "attn_fwd_rows: no such kernel for this configuration (ask dgppo_attn_rows_supported)");
  if (G == 0) return 0;
  DGPPO_REQUIRE(qt && Xa && emask && zcat, "attn_fwd_rows: NULL operand");
  DGPPO_REQUIRE(a.t.Ns == a.t.n || Xo, "attn_fwd_rows: Xo is NULL");
  attn_set_fwd(a, qt, Xa, Xo, nullptr, emask, zcat, attn);
  return attn_launch(AttnFamily::SLOT8, a, stream, false, "attn_fwd_rows");
}
extern "C" int32_t dgppo_attn_bwd_rows(const dgppo_env_cfg* cfg, int32_t F, int32_t H, int32_t Kp, const float* dzcat,
                                       const float* attn, const float* qt, const float* emask, const float* Xa, const float* Xo,
                                       float* dqt, int32_t G, void* stream) {
  AttnArgs a{};
  int32_t rc = attn_check(cfg, F, H, Kp, G, a);
  if (rc) return rc;
  DGPPO_REQUIRE(attn_rows_ok(*cfg, a.t, F, H, Kp), "attn_bwd_rows: no such kernel for this configuration (ask dgppo_attn_rows_supported)");
  if (G == 0) return 0;
  DGPPO_REQUIRE(dzcat && Xa && dqt, "attn_bwd_rows: NULL operand");
  DGPPO_REQUIRE(attn || (qt && emask), "attn_bwd_rows: without attn the weights need qt and emask");
  DGPPO_REQUIRE(a.t.Ns == a.t.n || Xo, "attn_bwd_rows: Xo is NULL");
  attn_set_bwd(a, dzcat, attn, qt, Xa, Xo, nullptr, dqt, nullptr, nullptr);
  a.emask = emask;
  return attn_launch(AttnFamily::SLOT8, a, stream, true, "attn_bwd_rows");
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
  rc = attn_set_xo(a, Xo_raw, Wo, ldwo, bo, "attn_bwd_xo_dw");
  if (rc) return rc;
  attn_set_bwd(a, dzcat, attn, qt, Xa, nullptr, efeat, dqt, dXa, nullptr);
  a.relu_xo = 1;
  a.dwo_slab = workspace;
  // the reduce is enqueued behind the backward before the one launch check, as it always was: a failed launch of either reports here
  const bool launched = launch_attn_bd(a, (hipStream_t)stream, true);
  DGPPO_REQUIRE(launched, "attn_bwd_xo_dw: dispatch failed");
  launch_attn_xo_dw_reduce(workspace, G, dWo, lddwo, dbo, (hipStream_t)stream);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
