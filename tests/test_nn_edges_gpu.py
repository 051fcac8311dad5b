"""The network kernels (nn_dense.hip, nn_elem.hip, nn_fused.hip, graph_feats.hip, attn*.hip, nn_prep.hip) at non-finite and edge inputs:
NaN / +-Inf through every ReLU as jax.nn.relu passes them, NaN sender rows behind masked slots, LayerNorm+ReLU at partial
waves / both grid-stride loops / constant and cancelling rows, the GRU gates at saturation, and dgppo_gnn_prep / _unprep
against their header formulas.  Every oracle is a float64 torch evaluation (oracle/nn_torch.py or a few lines here)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_nn_gpu import _attn_inputs, _attn_reference, _attn_run, _close, _feats, _scene  # noqa: E402

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pattern_matches(got, want64, name):
    """got carries exactly the oracle's non-finite pattern: NaN where it is NaN, +Inf / -Inf where it is, and exact zeros
    where the oracle has exact zeros in a row that holds non-finite values (a -Inf pre-activation behind the ReLU)"""
    got, want64 = got.detach().cpu(), want64.detach().cpu()
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    assert torch.equal(got.isnan(), want64.isnan()), f"{name}: NaN pattern differs ({int(got.isnan().sum())} vs {int(want64.isnan().sum())})"
    assert torch.equal(got == INF, want64 == INF), f"{name}: +Inf pattern differs"
    assert torch.equal(got == -INF, want64 == -INF), f"{name}: -Inf pattern differs"
    assert (got[want64 == 0] == 0).all(), f"{name}: non-zero where the oracle has an exact zero"


def _poison_rows(M):
    """first, middle and last row tile, the very last row included"""
    return sorted({0, M // 2, M - 1})


def _rest(M, rows):
    keep = torch.ones(M, dtype=torch.bool)
    keep[rows] = False
    return keep


# ----------------------------------------------------------------------------------------------------------------------
# 1. non-finite values through every ReLU
# ----------------------------------------------------------------------------------------------------------------------
DENSE_KN = [(64, 64), (144, 64), (8, 24), (7, 6)]


def _dense_operands(M, K, N, odd_ldx):
    """X is contiguous (tile kernel: vector staging when K % 4 == 0) or, odd_ldx, columns 1..K of a [M, K + 3] buffer whose
    leading dimension K + 3 is odd for every K here (64, 144, 8 are even; 7 + 3 = 10 is even but K % 4 != 0): the `vec`
    condition of dense_fwd_kernel, (K & 3) == 0 && (ldx & 3) == 0 && 16-byte aligned X, is then false -> scalar staging.
    K <= 16 takes dense_smallk_kernel whatever the layout: VECY with N = 24, the scalar epilogue with N = 6."""
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N + int(odd_ldx))
    Xw = torch.randn(M, K + 3, generator=g)
    W, b = torch.randn(K, N, generator=g), torch.randn(N, generator=g)
    Y0 = torch.randn(M, N, generator=g)
    mask = torch.randn(M, N, generator=g)
    mask[:, ::3] = 0.0                         # exact zeros are masked out
    if odd_ldx:
        assert ((K + 3) & 3) != 0 or (K & 3) != 0
    return Xw, W, b, Y0, mask


def _dense_run(K_, Xw, K, W, b, Y0, mask, act, acc, odd_ldx, cuda):
    Xd = Xw.to(cuda)
    X = Xd[:, 1:1 + K] if odd_ldx else Xd[:, 1:1 + K].contiguous()
    Y = Y0.to(cuda).clone() if acc else torch.full(Y0.shape, NAN, device=cuda)
    K_.dense_fwd(X, W.to(cuda), b.to(cuda), Y, act=act, accumulate=acc, relu_mask=None if mask is None else mask.to(cuda))
    return Y


def _dense_oracle(Xw, K, W, b, Y0, mask, acc):
    v = Xw[:, 1:1 + K].double() @ W.double() + b.double()
    if acc:
        v = v + Y0.double()
    v = torch.relu(v)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return v


@pytest.mark.parametrize("odd_ldx", [False, True], ids=["contiguous", "odd-ldx"])
@pytest.mark.parametrize("K,N", DENSE_KN)
@pytest.mark.parametrize("M", [1, 70, 513])
def test_dense_relu_passes_non_finite_values(cuda, M, K, N, odd_ldx):
    """dgppo_dense_fwd(act=1) — plain, accumulate (NaN / Inf in the old Y) and relu_mask — with NaN, +Inf and -Inf entries in a
    few rows: those rows carry the oracle's NaN / +Inf / 0 pattern (jax.nn.relu keeps a NaN; fmaxf dropped it), every other
    row keeps the bits of the clean run; and act=1 equals, bit for bit (the sign of a zero and the payload of a NaN included),
    torch.relu applied on the device to the same call's act=0 output."""
    from dgppo_amd import ops_nn as K_
    Xw, W, b, Y0, mask = _dense_operands(M, K, N, odd_ldx)
    rows = _poison_rows(M)
    vals = [NAN, INF, -INF]
    Xp, Yp = Xw.clone(), Y0.clone()
    for j, r in enumerate(rows):
        Xp[r, 1 + (5 * j + 2) % K] = vals[j % 3]
        Yp[r, (3 * j + 1) % N] = vals[(j + 1) % 3]
    keep = _rest(M, rows)
    for acc in (False, True):
        for mk in (None, mask):
            name = f"M={M} K={K} N={N} odd_ldx={odd_ldx} acc={acc} mask={mk is not None}"
            clean = _dense_run(K_, Xw, K, W, b, Y0, mk, 1, acc, odd_ldx, cuda)
            # poison X always; the old Y only where it is read
            got = _dense_run(K_, Xp, K, W, b, Yp if acc else Y0, mk, 1, acc, odd_ldx, cuda)
            torch.cuda.synchronize()
            assert torch.isfinite(clean).all(), name
            assert _bits_equal(got[keep.to(cuda)], clean[keep.to(cuda)]), f"{name}: a clean row changed"
            want = _dense_oracle(Xp, K, W, b, Yp, mk, acc)
            _pattern_matches(got[rows], want[rows], name)
            assert not torch.isfinite(want[rows]).all(), name
            if mk is not None:
                assert float(got[:, ::3].abs().max()) == 0.0, f"{name}: a zero mask entry let a value through"
            # the ReLU's bits: act=1 against torch.relu (NaN-propagating) of the act=0 output of the same call
            lin = _dense_run(K_, Xp, K, W, b, Yp if acc else Y0, None, 0, acc, odd_ldx, cuda)
            act1 = _dense_run(K_, Xp, K, W, b, Yp if acc else Y0, None, 1, acc, odd_ldx, cuda)
            assert _bits_equal(act1, torch.relu(lin)), f"{name}: act=1 is not, bit for bit, relu(act=0)"


def _ln_params(g):
    gam, bet = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    return gam, bet


def _poisoned_ln_rows(x, rows):
    """NaN entry, +Inf entry, -Inf entry, then rows of magnitude 3e19 (x^2 and mean^2 overflow: var = inf - inf)"""
    kinds = []
    for j, r in enumerate(rows):
        kind = ("nan", "big", "+inf", "-inf")[j % 4] if len(rows) > 1 else "nan"
        if kind == "big":
            x[r] = 3e19 * (1.0 + 0.1 * torch.rand(x.shape[1], generator=torch.Generator().manual_seed(r)))
        else:
            x[r, (7 * j + 3) % x.shape[1]] = {"nan": NAN, "+inf": INF, "-inf": -INF}[kind]
        kinds.append(kind)
    return kinds


@pytest.mark.parametrize("M", [1, 70, 513])
def test_ln_relu_fwd_passes_non_finite_values(cuda, M):
    """dgppo_ln_relu_fwd: a NaN / Inf entry, or a row of magnitude 3e19 (E[x^2] and E[x]^2 both overflow: the flax
    fast-variance form is inf - inf = NaN, and so is nn_torch.layer_norm in float32), makes the whole row NaN as in the
    reference; y and the saved (mean, rstd) of every other row keep the bits of the clean run."""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, 64, generator=g) * 2 + 0.3
    gam, bet = _ln_params(g)
    rows = sorted(set(_poison_rows(M) + ([M // 4] if M > 4 else [])))
    xp = x.clone()
    kinds = _poisoned_ln_rows(xp, rows)
    p = {"scale": gam, "bias": bet}
    want32 = torch.relu(T.layer_norm(p, xp))                                  # float32: the big rows overflow as on the device
    want64 = torch.relu(T.layer_norm({k: v.double() for k, v in p.items()}, xp.double()))
    for r, kind in zip(rows, kinds):
        assert want32[r].isnan().all(), (r, kind)
        assert kind == "big" or want64[r].isnan().all(), (r, kind)

    def run(xin):
        y, st = torch.full((M, 64), 7.0, device=cuda), torch.full((M, 2), 7.0, device=cuda)
        K_.ln_relu_fwd(xin.to(cuda), gam.to(cuda), bet.to(cuda), y, st)
        return y, st
    (yc, stc), (yp, stp) = run(x), run(xp)
    torch.cuda.synchronize()
    keep = _rest(M, rows).to(cuda)
    assert torch.isfinite(yc).all() and torch.isfinite(stc).all()
    assert _bits_equal(yp[keep], yc[keep]) and _bits_equal(stp[keep], stc[keep]), "a clean row changed"
    assert yp[rows].isnan().all(), f"rows {rows} ({kinds}): {yp[rows].isnan().all(1).tolist()}"


def _mlp_params(g, positive_w1=False):
    P = {k: torch.randn(*shp, generator=g) * sc for k, shp, sc in (
        ("W1", (64, 64), 0.2), ("b1", (64,), 0.1), ("g1", (64,), 1.0), ("be1", (64,), 0.1), ("W2", (64, 64), 0.2),
        ("b2", (64,), 0.1), ("g2", (64,), 1.0), ("be2", (64,), 0.1), ("Wi", (64, 192), 0.2), ("bi", (192,), 0.1))}
    if positive_w1:
        P["W1"] = P["W1"].abs() * 0.25
    return P


def _mlp_tree(P, dtype):
    c = lambda k: P[k].to(dtype)
    return {"Dense_0": {"kernel": c("W1"), "bias": c("b1")}, "LayerNorm_0": {"scale": c("g1"), "bias": c("be1")},
            "Dense_1": {"kernel": c("W2"), "bias": c("b2")}, "LayerNorm_1": {"scale": c("g2"), "bias": c("be2")}}


def _mlp_gi_oracle(P, X, dtype):
    y2 = T.mlp(_mlp_tree(P, dtype), X.to(dtype))
    return y2 @ P["Wi"].to(dtype) + P["bi"].to(dtype)


def _mlp_gi_run(K_, P, Xfull, off, save, cuda):
    M = Xfull.shape[0]
    d = {k: v.to(cuda) for k, v in P.items()}
    Xd = Xfull.to(cuda)[:, off:off + 64]
    gi = torch.full((M, 192), 7.0, device=cuda)
    saves = tuple(torch.full((M, w), 7.0, device=cuda) for w in (64, 64, 2, 64, 64, 2)) if save else None
    K_.mlp_gi_fwd(Xd, d["W1"], d["b1"], d["g1"], d["be1"], d["W2"], d["b2"], d["g2"], d["be2"], d["Wi"], d["bi"], gi, saves)
    return gi, saves


@pytest.mark.parametrize("save", [True, False], ids=["saves", "inference"])
@pytest.mark.parametrize("off", [8, 1], ids=["rows-per-wave", "tile-kernel"])
def test_mlp_gi_fwd_passes_non_finite_values(cuda, off, save):
    """dgppo_mlp_gi_fwd, both kernels (input rows 16-byte addressable: rows per wave; a view starting at column 1: the 32-row
    tile kernel), with and without saves: a NaN / Inf entry or a 3e19 row in X gives a NaN gi row (W1 > 0 here, so the 3e19 row
    gives a same-sign pre-activation row whose E[x^2] and E[x]^2 both overflow), as nn_torch.mlp does in float32; gi and every
    saved activation of the other rows keep the bits of the clean run."""
    from dgppo_amd import ops_nn as K_
    M = 70
    g = torch.Generator().manual_seed(17 + off)
    P = _mlp_params(g, positive_w1=True)
    Xfull = torch.randn(M, 80, generator=g)
    rows = [0, 17, 35, 69]
    Xp = Xfull.clone()
    sub = Xp[:, off:off + 64]                       # a view: the poison lands in Xp
    kinds = _poisoned_ln_rows(sub, rows)
    want32 = _mlp_gi_oracle(P, Xp[:, off:off + 64], torch.float32)
    want64 = _mlp_gi_oracle(P, Xp[:, off:off + 64], torch.float64)
    for r, kind in zip(rows, kinds):
        assert want32[r].isnan().all(), (r, kind)
        assert kind == "big" or want64[r].isnan().all(), (r, kind)
    (gc, sc), (gp, sp) = _mlp_gi_run(K_, P, Xfull, off, save, cuda), _mlp_gi_run(K_, P, Xp, off, save, cuda)
    torch.cuda.synchronize()
    keep = _rest(M, rows).to(cuda)
    assert torch.isfinite(gc).all()
    assert _bits_equal(gp[keep], gc[keep]), "gi of a clean row changed"
    assert gp[rows].isnan().all(), f"rows {rows} ({kinds}): {gp[rows].isnan().all(1).tolist()}"
    if save:
        for a, b, nm in zip(sp, sc, ("p1", "y1", "st1", "p2", "y2", "st2")):
            assert torch.isfinite(b).all(), nm
            assert _bits_equal(a[keep], b[keep]), f"{nm} of a clean row changed"
        assert sp[1][rows].isnan().all() and sp[4][rows].isnan().all(), "y1 / y2 of a poisoned row must be NaN"


def _xo_case(cuda, G, seed):
    """operands of dgppo_attn_fwd_xo / _bwd_xo at LidarSpread (8, 3), F = 32 (as test_attention_with_recomputed_other_nodes)"""
    from dgppo_amd import _native as N, ops_nn as K_
    cfg = N.make_env_cfg(0, 8, 3)
    F, Kp, H, S, n = 32, 144, 3, cfg.fan_in, cfg.n_agents
    n_other = cfg.num_nodes - 1 - n
    assert K_.attn_xo_supported(cfg, F, H, Kp)
    gen = torch.Generator().manual_seed(seed)
    inp = _attn_inputs(cfg, F, H, Kp, G, gen, 0.35, on=n)
    inp["raw"] = torch.randn(G * n_other, 8, generator=gen)
    inp["Wo"] = torch.randn(8, 32, generator=gen) * 0.5
    inp["bo"] = torch.randn(32, generator=gen) * 0.3
    return cfg, F, H, Kp, S, n, n_other, inp


def test_attn_fwd_xo_relu_passes_nan(cuda):
    """dgppo_attn_fwd_xo recomputes relu(raw Wo + bo): a NaN raw row behind an UNMASKED slot gives a NaN row, hence a NaN z for
    the receiver that reads it (fmaxf made the row bo's ReLU instead and z stayed finite); every other graph keeps its bits."""
    from dgppo_amd import ops_nn as K_
    G, gp, ip, m = 5, 2, 5, 1
    cfg, F, H, Kp, S, n, n_other, inp = _xo_case(cuda, G, 41)
    slot = n + cfg.goal_slots + m
    row = gp * n_other + cfg.n_goals + ip * cfg.obs_slots + m          # the private hit row of agent ip behind that slot
    inp["em"][gp * n + ip, slot] = 1.0
    inp["ef"][gp * n + ip, slot] = 0.25
    d = {k: v.to(cuda) for k, v in inp.items()}

    def run(raw):
        z = torch.full((G * n, Kp), 7.0, device=cuda)
        at = torch.full((G * n, S, H), 7.0, device=cuda)
        K_.attn_fwd_xo(cfg, F, H, Kp, d["qt"], d["Xa"], raw, d["Wo"], d["bo"], d["ef"], d["em"], z, at, G)
        return z, at
    zc, atc = run(d["raw"])
    rawp = d["raw"].clone()
    rawp[row, 3] = NAN
    zp, atp = run(rawp)
    torch.cuda.synchronize()
    assert torch.isfinite(zc).all() and torch.isfinite(atc).all()
    assert zp[gp * n + ip].isnan().any(), "the receiver of a NaN sender row has a finite z"
    others = torch.ones(G * n, dtype=torch.bool, device=cuda)
    others[gp * n:(gp + 1) * n] = False
    assert _bits_equal(zp[others], zc[others]) and _bits_equal(atp[others], atc[others]), "another graph changed"


def _non_finite_where_the_oracle_says(got, want64, name):
    got, want64 = got.detach().cpu(), want64.detach()
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    missed = ~torch.isfinite(want64) & torch.isfinite(got)
    assert not missed.any(), f"{name}: finite where the float64 oracle is not ({int(missed.sum())} entries)"


def test_net_forward_passes_a_nan_feature(cuda):
    """Net.forward of the policy and of Vl at LidarSpread (3, 2), 6 graphs of one step: one feature of agent 1 of graph 4 is
    NaN.  Graph 4's outputs are non-finite wherever oracle/nn_torch.py says so in float64 on the same inputs (the ReLU behind
    every GNN layer used to turn the NaN row into zeros: finite outputs); graphs 0-3 and 5 keep the bits of the clean forward."""
    from dgppo_amd import nets
    from oracle import env_np as E
    n, G, gp, ip, fp = 3, 6, 4, 1, 2
    cfg, ocfg, ag, goal, obst, hi, gr = _scene(E.LIDAR_SPREAD, n, 2, G, 1, seed=21)
    gen = torch.Generator().manual_seed(5)
    jit = lambda tr: T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), tr)
    trees = {"policy": jit(T.init_policy(1, cfg.node_dim)), "Vl": jit(T.init_value(2, cfg.node_dim, 1, 2))}
    trees["policy"]["params"]["ScaleHid"]["kernel"] = T.orthogonal(gen, 64, 64, 0.5)
    g64 = {k: (v.double() if v.is_floating_point() else v) for k, v in T.graph_to_torch(gr).items()}
    feats = _feats(cfg, ag, goal, obst, hi, cuda)
    torch.cuda.synchronize()
    assert torch.allclose(feats.Xa.view(G, n, -1)[..., :cfg.node_dim].cpu().double(), g64["nodes"][:, :n], atol=1e-6)
    clean_Xa = feats.Xa.clone()
    g64["nodes"] = g64["nodes"].clone()
    g64["nodes"][gp, ip, fp] = NAN
    t64 = {k: T.tree_map(lambda t: t.double(), v) for k, v in trees.items()}
    with torch.no_grad():
        mean64, std64, h64 = T.policy_dist(t64["policy"], g64, torch.zeros(G, n, 64, dtype=torch.float64), n)
        v64, _ = T.value_Vl(t64["Vl"], g64, torch.zeros(G, 1, 64, dtype=torch.float64), n)
    assert not torch.isfinite(mean64[gp, ip]).any() and not torch.isfinite(v64[gp]) and torch.isfinite(mean64[[0, 1, 2, 3, 5]]).all()
    rows = torch.ones(G * n, dtype=torch.bool, device=cuda)
    rows[gp * n:(gp + 1) * n] = False
    graphs = torch.ones(G, dtype=torch.bool, device=cuda)
    graphs[gp] = False
    for kind, layers, n_out in (("policy", 2, 2), ("Vl", 2, 1)):
        net = nets.Net(kind, cfg, layers, n_out, cuda)
        net.load_tree(trees[kind])
        outs = {}
        for tag, poison in (("clean", False), ("nan", True)):
            feats.Xa.copy_(clean_Xa)
            if poison:
                feats.Xa[gp * n + ip, fp] = NAN
            act = net.forward(feats, n_seq=G * n if kind == "policy" else G, T=1, h0=None)
            torch.cuda.synchronize()
            outs[tag] = {k: act[k].clone() for k in (("ms", "hs") if kind == "policy" else ("v", "hs"))}
        for k, v in outs["clean"].items():
            assert torch.isfinite(v).all(), (kind, k)
            keep = rows if v.shape[0] == G * n else graphs
            assert _bits_equal(outs["nan"][k][keep], v[keep]), f"{kind} {k}: another graph changed"
        if kind == "policy":
            ms = outs["nan"]["ms"].view(G, n, 4)
            _non_finite_where_the_oracle_says(ms[..., :2], mean64, "policy mean")
            _non_finite_where_the_oracle_says(ms[..., 2:], std64, "policy std_trans")
            _non_finite_where_the_oracle_says(outs["nan"]["hs"].view(G, n, 64), h64, "policy carry")
        else:
            _non_finite_where_the_oracle_says(outs["nan"]["v"].view(G), v64, "Vl")
    feats.Xa.copy_(clean_Xa)


def test_nan_observation_skips_exactly_the_poisoned_minibatch(cuda):
    """test_nan_cost_skips_exactly_the_poisoned_minibatch for a NaN that enters through the OBSERVATION: one coordinate of one
    agent's stored state in the stochastic rollout's record (env 3, step 5) is NaN.  oracle/dgppo_ref.py on the same batch says
    which networks' gradients are non-finite on the minibatch holding env 3 (the value targets and the advantage of env 3 turn
    NaN: Vl and the policy; Vh trains on the deterministic rollout): exactly those report has_nan == 1 and keep their
    parameters and Adam count for that minibatch, the clean minibatch trains all three, every parameter stays finite."""
    from oracle import dgppo_ref as R
    from test_engine_gpu import _np_rollout, _setup
    B, T_, rs, bs = 4, 8, 4, 16
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, bs, rs)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3)
    det = eng.rollout(seeds + 1000, False)
    ro.agent_tm[5, 3, 1, 0] = NAN                            # step 5, env 3, agent 1, x coordinate
    snap = {}

    def hook(name, net, mb):
        snap[(name, mb)] = (net.params.detach().clone(), eng.opt[name].state[:8].detach().clone())
    eng.grad_hook = hook
    before = {k: net.params.detach().clone() for k, net in eng.nets.items()}
    step, perm = 10, np.asarray([0, 1, 2, 3])                # minibatch 1 = envs {2, 3}
    info = eng.update(ro, det, step, perm)
    torch.cuda.synchronize()
    # the oracle on the same batch (initial parameters: which gradients are non-finite does not depend on minibatch 0's step)
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, alpha=hp.alpha, cbf_eps=hp.cbf_eps, rnn_step=rs,
               clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    r, d = _np_rollout(ro), _np_rollout(det)
    assert np.isnan(r["agent"][3, 5, 1, 0]) and np.isfinite(r["agent"][:3]).all() and np.isfinite(d["agent"]).all()
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), v) for k, v in trees.items()}
    with np.errstate(all="ignore"):
        wt = R.targets(leaf, ocfg, r, d, hpd, eng.cbf_weight_at(step))
        R.minibatch_losses(leaf, ocfg, r, d, wt, perm[2:], hpd, eng.eps_hat.cpu())
    bad = {k: any(not bool(torch.isfinite(t.grad).all()) for _, t in T.tree_leaves(leaf[k]) if t.grad is not None) for k in leaf}
    assert bad == {"policy": True, "Vl": True, "Vh": False}, bad
    flag = {"policy": "policy/has_nan", "Vl": "Vl/has_nan", "Vh": "Vh/grad_Vh_has_nan"}
    for k in ("policy", "Vl", "Vh"):
        assert torch.equal(snap[(k, 0)][0], before[k])                       # minibatch 0 is entered with the initial parameters
        assert not torch.equal(snap[(k, 1)][0], before[k]), f"minibatch 0 (clean) did not train {k}"
        assert float(snap[(k, 1)][1][2]) == 1.0
        assert info[flag[k]] == float(bad[k]), (k, info[flag[k]])
        if bad[k]:
            assert torch.equal(eng.nets[k].params, snap[(k, 1)][0]), f"the poisoned minibatch changed the {k} parameters"
            assert float(eng.opt[k].state[2]) == 1.0, f"{k}: Adam count moved on a skipped step"
        else:
            assert not torch.equal(eng.nets[k].params, snap[(k, 1)][0]) and float(eng.opt[k].state[2]) == 2.0
        assert torch.isfinite(eng.nets[k].params).all() and torch.isfinite(eng.opt[k].m).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. a masked slot's NaN sender row reaches nobody
# ----------------------------------------------------------------------------------------------------------------------
def _masked_private_rows(cfg, G, em):
    """Xo row indices (over all graphs) of the private LiDAR-hit rows whose one slot is masked"""
    n, S, n_other = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1 - cfg.n_agents
    assert cfg.is_lidar and cfg.obs_slots > 0
    first = n + cfg.goal_slots
    idx = (em.reshape(G, n, S)[:, :, first:] == 0).nonzero()                 # (g, i, m)
    return idx[:, 0] * n_other + cfg.n_goals + idx[:, 1] * cfg.obs_slots + idx[:, 2]


MASKED_CASES = [(8, 3, 8, 48), (8, 3, 32, 144), (8, 3, 16, 80), (8, 3, 12, 64), (8, 3, 6, 40),    # the five families at n = 8
                (18, 3, 8, 48), (18, 3, 32, 144)]                                                   # first tiled LiDAR shape


@pytest.mark.parametrize("fill", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("n,n_obs,F,Kp", MASKED_CASES)
def test_masked_slot_nan_sender_row_reaches_nobody(cuda, n, n_obs, F, Kp, fill):
    """for NaN LiDAR hit points "masked slots are skipped so they cannot poison agents".  A NaN hit point makes the
    node row of that hit NaN as well, not only the edge features.  Every private LiDAR-hit row of Xo whose slot is masked is
    set to NaN (+Inf): z, attn, dq, dXa and the dq-only backward must stay finite and equal, bit for bit, the same call with
    those rows set to 0.0 — which itself is within 2e-5 of the float64 reference.  (dXo at those rows is not asserted.)"""
    from dgppo_amd import _native as N
    cfg = N.make_env_cfg(0, n, n_obs)
    H, G = 3, 5
    inp = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(100 * n + F), 0.35, on=cfg.n_agents)
    rows = _masked_private_rows(cfg, G, inp["em"])
    assert len(rows) > G
    zero, bad = dict(inp), dict(inp)
    zero["Xo"], bad["Xo"] = inp["Xo"].clone(), inp["Xo"].clone()
    zero["Xo"][rows] = 0.0
    bad["Xo"][rows] = fill
    got0, got1, want = _attn_run(cfg, F, H, Kp, G, zero, cuda), _attn_run(cfg, F, H, Kp, G, bad, cuda), _attn_reference(cfg, F, H, Kp, G, zero)
    for k in ("z", "at", "dq", "dXa", "dq_only"):
        assert torch.isfinite(got0[k]).all(), f"F={F} zero-filled {k} not finite"
        _close(got0[k], want["dq" if k == "dq_only" else k], 2e-5, f"n={n} F={F} zero-filled {k}")
        assert torch.isfinite(got1[k]).all(), f"n={n} F={F}: a masked {fill} sender row reached {k} " \
                                              f"({int((~torch.isfinite(got1[k])).any(-1).sum())} rows)"
        assert _bits_equal(got1[k], got0[k]), f"n={n} F={F}: {k} differs from the zero-filled run"
    live = torch.ones(inp["Xo"].shape[0], dtype=torch.bool)
    live[rows] = False
    assert torch.isfinite(got1["dXo"][live.to(cuda)]).all(), "dXo of an unpoisoned row is not finite"


def test_masked_slot_nan_sender_row_persistent_forward(cuda):
    """the persistent block-diagonal forward (n <= 8, F = 32, more than 2 * cap workgroups: the rollout's launch; G as in
    test_attention_persistent_forward) zeroes the masked private rows in its own staging code: NaN Xo rows, and NaN raw rows
    of dgppo_attn_fwd_xo, behind masked slots leave z and attn finite and bit-equal to the zero-filled call."""
    from dgppo_amd import ops_nn as K_
    G = 4 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 2
    cfg, F, H, Kp, S, n, n_other, inp = _xo_case(cuda, G, 47)
    rows = _masked_private_rows(cfg, G, inp["em"]).to(cuda)
    d = {k: v.to(cuda) for k, v in inp.items() if k != "dz"}

    def run(fused, src):
        z, at = torch.full((G * n, Kp), NAN, device=cuda), torch.full((G * n, S, H), NAN, device=cuda)
        if fused:
            K_.attn_fwd_xo(cfg, F, H, Kp, d["qt"], d["Xa"], src, d["Wo"], d["bo"], d["ef"], d["em"], z, at, G)
        else:
            K_.attn_fwd(cfg, F, H, Kp, d["qt"], d["Xa"], src, d["ef"], d["em"], z, at, G)
        return z, at
    for fused, key in ((False, "Xo"), (True, "raw")):
        src0, src1 = d[key].clone(), d[key].clone()
        src0[rows] = 0.0
        src1[rows] = NAN
        (z0, at0), (z1, at1) = run(fused, src0), run(fused, src1)
        torch.cuda.synchronize()
        assert torch.isfinite(z0).all() and torch.isfinite(at0).all()
        assert torch.isfinite(z1).all(), f"fused={fused}: a masked NaN sender row reached z ({int((~torch.isfinite(z1)).any(-1).sum())} rows)"
        assert _bits_equal(z1, z0) and _bits_equal(at1, at0), f"fused={fused}: differs from the zero-filled run"


@pytest.mark.parametrize("fill", [NAN, INF], ids=["nan", "inf"])
def test_masked_slot_nan_raw_row_reaches_nobody_xo(cuda, fill):
    """the same for dgppo_attn_fwd_xo / _bwd_xo at F = 32: the RAW row of a masked private hit is NaN (+Inf), so the recomputed
    row relu(raw Wo + bo) is NaN (NaN or +Inf / 0 per column for +Inf); dXo of the poisoned rows and dWo / dbo are not asserted"""
    from dgppo_amd import ops_nn as K_
    G = 5
    cfg, F, H, Kp, S, n, n_other, inp = _xo_case(cuda, G, 43)
    rows = _masked_private_rows(cfg, G, inp["em"])
    assert len(rows) > G
    d = {k: v.to(cuda) for k, v in inp.items()}

    def run(raw):
        R = G * n
        z, at = torch.full((R, Kp), 7.0, device=cuda), torch.full((R, S, H), 7.0, device=cuda)
        dq, dXa = torch.full((R, H * F), 7.0, device=cuda), torch.full((R, F), 7.0, device=cuda)
        dXo = torch.full((G * n_other, F), 7.0, device=cuda)
        K_.attn_fwd_xo(cfg, F, H, Kp, d["qt"], d["Xa"], raw, d["Wo"], d["bo"], d["ef"], d["em"], z, at, G)
        K_.attn_bwd_xo(cfg, F, H, Kp, d["dz"], at, d["qt"], d["Xa"], raw, d["Wo"], d["bo"], d["ef"], dq, dXa, dXo, G)
        dq3 = torch.full((R, H * F), 7.0, device=cuda)
        K_.attn_bwd_xo(cfg, F, H, Kp, d["dz"], at, d["qt"], d["Xa"], raw, d["Wo"], d["bo"], d["ef"], dq3, None, None, G)
        torch.cuda.synchronize()
        return dict(z=z, at=at, dq=dq, dXa=dXa, dq_only=dq3)
    raw0, raw1 = d["raw"].clone(), d["raw"].clone()
    raw0[rows.to(cuda)] = 0.0
    raw1[rows.to(cuda)] = fill
    got0, got1 = run(raw0), run(raw1)
    ref_in = dict(inp)
    ref_in["Xo"] = torch.relu(raw0.cpu().double() @ inp["Wo"].double() + inp["bo"].double()).float()
    want = _attn_reference(cfg, F, H, Kp, G, ref_in)
    for k in got0:
        assert torch.isfinite(got0[k]).all(), f"zero-filled {k} not finite"
        _close(got0[k], want["dq" if k == "dq_only" else k], 2e-5, f"xo zero-filled {k}")
        assert torch.isfinite(got1[k]).all(), f"a masked {fill} raw row reached {k}"
        assert _bits_equal(got1[k], got0[k]), f"{k} differs from the zero-filled run"
    # reported, not asserted (the reference's own weight gradient is 0 * NaN there): dWo / dbo of the recomputed rows
    R = G * n
    dq, dXa = torch.empty(R, H * F, device=cuda), torch.empty(R, F, device=cuda)
    dWo, dbo = torch.zeros(8, 32, device=cuda), torch.zeros(32, device=cuda)
    ws = torch.empty(K_.attn_xo_workspace_floats(G), device=cuda)
    K_.attn_bwd_xo_dw(cfg, F, H, Kp, d["dz"], got1["at"], d["qt"], d["Xa"], raw1, d["Wo"], d["bo"], d["ef"], dq, dXa, dWo, dbo, ws, G)
    torch.cuda.synchronize()
    _close(dq, got0["dq"].cpu(), 2e-5, "dw variant dq")
    _close(dXa, got0["dXa"].cpu(), 2e-5, "dw variant dXa")
    print(f"masked {fill} raw rows: dWo finite {bool(torch.isfinite(dWo).all())}, dbo finite {bool(torch.isfinite(dbo).all())}")


# ----------------------------------------------------------------------------------------------------------------------
# 3. LayerNorm + ReLU at its edges
# ----------------------------------------------------------------------------------------------------------------------
LN_M = [1, 2, 3, 5, 1037, 4099, 32787]       # partial waves; ln_relu_bwd's grid-stride loop from 4097 rows, ln_relu_fwd's from 32769


def _ln_oracle(x, gam, bet, dy, dtype):
    xr = x.to(dtype).requires_grad_()
    p = {"scale": gam.to(dtype).requires_grad_(), "bias": bet.to(dtype).requires_grad_()}
    y = torch.relu(T.layer_norm(p, xr))
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, p["scale"].grad, p["bias"].grad


def _ln_device(K_, x, gam, bet, dy, dg0, db0, cuda):
    M = x.shape[0]
    xd, gd, bd = x.to(cuda), gam.to(cuda), bet.to(cuda)
    y, st = torch.full((M, 64), NAN, device=cuda), torch.full((M, 2), NAN, device=cuda)
    K_.ln_relu_fwd(xd, gd, bd, y, st)
    dx = torch.full((M, 64), NAN, device=cuda)
    dg, db = dg0.to(cuda).clone(), db0.to(cuda).clone()
    K_.ln_relu_bwd(xd, y, st, gd, dy.to(cuda), dx, dg, db)
    torch.cuda.synchronize()
    return y, st, dx, dg, db


@pytest.mark.parametrize("M", LN_M)
def test_ln_relu_shapes_against_float64(cuda, M):
    """dgppo_ln_relu_fwd / _bwd against float64 nn_torch.layer_norm + autograd at 1e-5 / 2e-5; dgamma and dbeta start from
    non-zero values and must end at start + gradient (the kernel adds)."""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, 64, generator=g) * 2 + 0.3
    gam, bet = _ln_params(g)
    dy = torch.randn(M, 64, generator=g)
    dg0, db0 = torch.randn(64, generator=g) * 3, torch.randn(64, generator=g) * 3
    y64, dx64, dg64, db64 = _ln_oracle(x, gam, bet, dy, torch.float64)
    y, st, dx, dg, db = _ln_device(K_, x, gam, bet, dy, dg0, db0, cuda)
    _close(y, y64, 1e-5, "ln fwd")
    mean64 = x.double().mean(-1)
    rstd64 = torch.rsqrt((x.double() ** 2).mean(-1) - mean64 ** 2 + 1e-6)
    _close(st[:, 0], mean64, 1e-5, "ln mean")
    _close(st[:, 1], rstd64, 1e-5, "ln rstd")
    _close(dx, dx64, 2e-5, "ln dx")
    _close(dg, dg0.double() + dg64, 2e-5, "ln dgamma (start + gradient)")
    _close(db, db0.double() + db64, 2e-5, "ln dbeta (start + gradient)")


def _special_rows(kind, M, g):
    if kind == "constant":          # var = 0, rstd = 1e3
        return (torch.randn(M, 1, generator=g) * 3).expand(M, 64).contiguous()
    return 100.0 + 0.1 * torch.randn(M, 64, generator=g)     # cancellation in E[x^2] - E[x]^2


# Bound of the special rows = 4 x the maximum error of nn_torch.layer_norm (+ autograd) evaluated in float32 on the CPU against
# float64 on the same rows (the margin of the float64-oracle tests of the algorithm kernels), computed by the test.  Measured on
# these 67 rows (maximum absolute error of the float32 evaluation):
#   constant rows:            y 7.0e-4   dx 2.0e+3 (values up to 5.4e3)   dgamma 2.8e-3   dbeta 3.0e-6
#   mean 100, std 0.1 rows:   y 4.3e-1   dx 3.2e+1 (values up to 4.4e1)   dgamma 2.7e+0   dbeta 2.4e+0
# The fast-variance form loses the variance of such rows in float32: E[x^2] ~ 1e4 carries an error of ~1e-3 against var = 1e-2,
# and on a constant row the rounded E[x^2] - E[x]^2 (exactly 0 in float64: rstd = 1e3) is compared with eps = 1e-6.
@pytest.mark.parametrize("kind", ["constant", "mean100-std0.1"])
def test_ln_relu_constant_and_cancelling_rows(cuda, kind):
    from dgppo_amd import ops_nn as K_
    M = 67
    g = torch.Generator().manual_seed(len(kind))
    x = _special_rows(kind, M, g)
    gam, bet = _ln_params(g)
    bet = bet + 0.5 * torch.sign(bet)                      # |beta| >= 0.5: the ReLU gate of a constant row (y = beta) is decided
    dy = torch.randn(M, 64, generator=g)
    dg0, db0 = torch.randn(64, generator=g), torch.randn(64, generator=g)
    w64 = _ln_oracle(x, gam, bet, dy, torch.float64)
    w32 = _ln_oracle(x, gam, bet, dy, torch.float32)
    y, st, dx, dg, db = _ln_device(K_, x, gam, bet, dy, dg0, db0, cuda)
    got = (y, dx, dg.cpu().double() - dg0.double(), db.cpu().double() - db0.double())
    # The float32 reference loses the variance of these rows, so its own error in dx (and in y of the mean-100 rows) is as large
    # as the values and 4 x that bound alone would let any dx pass.  So y, dx, dgamma and dbeta are also held, at the ordinary
    # 1e-5 / 2e-5, to the float64 LayerNorm formulas evaluated with the kernel's OWN saved (mean, rstd) and ReLU gate, which takes
    # the sensitivity to the variance out: x - mean is exact in float32 on these rows.
    m_, r_ = st[:, 0:1].cpu().double(), st[:, 1:2].cpu().double()
    xh = (x.double() - m_) * r_
    _close(y, torch.relu(xh * gam.double() + bet.double()), 1e-5, f"{kind} y from the saved (mean, rstd)")
    dl = torch.where(y.cpu() > 0, dy, torch.zeros_like(dy)).double()
    dxh = dl * gam.double()
    _close(dx, r_ * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True)), 2e-5, f"{kind} dx from the saved (mean, rstd)")
    _close(dg, dg0.double() + (dl * xh).sum(0), 2e-5, f"{kind} dgamma from the saved (mean, rstd)")
    _close(db, db0.double() + dl.sum(0), 2e-5, f"{kind} dbeta from the saved (mean, rstd)")
    for nm, a, b64, b32 in zip(("y", "dx", "dgamma", "dbeta"), got, w64, w32):
        ref_err = float((b32.double() - b64).abs().max())
        err = float((a.detach().cpu().double() - b64).abs().max())
        print(f"{kind} {nm}: float32 CPU max error {ref_err:.3e}, device max error {err:.3e}, scale {float(b64.abs().max()):.3e}")
        assert torch.isfinite(a).all(), nm
        assert err <= 4.0 * ref_err, f"{kind} {nm}: error {err:.3e} > 4 x {ref_err:.3e} (the float32 reference's own)"


@pytest.mark.parametrize("M", LN_M)
def test_mlp_gi_fused_shapes_against_float64_and_unfused(cuda, M):
    """dgppo_mlp_gi_fwd / _bwd at the same row counts against the float64 composition (nn_torch.mlp + the gate Dense) and its
    autograd, the LayerNorm gradients accumulated onto non-zero starts; and on the same rows the unfused dgppo_ln_relu_fwd /
    _bwd give what the fused kernels give (1e-5 / 2e-5)."""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(M + 5)
    P = _mlp_params(g)
    X = torch.randn(M, 64, generator=g)
    dgi = torch.randn(M, 192, generator=g)
    # float64 oracle with every intermediate kept
    Xr = X.double().requires_grad_()
    leaf = {k: v.double().requires_grad_() for k, v in P.items()}
    ln = lambda v, gk, bk: T.layer_norm({"scale": leaf[gk], "bias": leaf[bk]}, v)
    p1 = Xr @ leaf["W1"] + leaf["b1"]; p1.retain_grad()
    y1 = torch.relu(ln(p1, "g1", "be1"))
    p2 = y1 @ leaf["W2"] + leaf["b2"]; p2.retain_grad()
    y2 = torch.relu(ln(p2, "g2", "be2"))
    gi64 = y2 @ leaf["Wi"] + leaf["bi"]
    gi64.backward(dgi.double())
    assert torch.allclose(gi64.detach(), _mlp_gi_oracle(P, X, torch.float64))          # the same thing through nn_torch.mlp
    gi, sv = _mlp_gi_run(K_, P, X, 0, True, cuda)
    gi_inf, _ = _mlp_gi_run(K_, P, X, 0, False, cuda)
    _close(gi, gi64, 2e-5, "gi")
    assert _bits_equal(gi_inf, gi), "inference form differs from the training form"
    stat = lambda p: torch.stack([p.detach().mean(-1), torch.rsqrt((p.detach() ** 2).mean(-1) - p.detach().mean(-1) ** 2 + 1e-6)], 1)
    for got, want, nm in zip(sv, (p1, y1, stat(p1), p2, y2, stat(p2)), ("p1", "y1", "st1", "p2", "y2", "st2")):
        _close(got, want, 1e-5 if nm[0] != "p" else 2e-5, nm)
    d = {k: v.to(cuda) for k, v in P.items()}
    start = {k: torch.randn(64, generator=g) * 3 for k in ("dg2", "db2", "dg1", "db1")}
    pg = {k: v.to(cuda).clone() for k, v in start.items()}
    outs = {k: torch.full((M, 64), NAN, device=cuda) for k in ("dpre2", "dpre1", "dx")}
    K_.mlp_gi_bwd(dgi.to(cuda), d["Wi"], d["W2"], d["W1"], d["g2"], d["g1"], sv[3], sv[4], sv[5], sv[0], sv[1], sv[2], None,
                  outs["dpre2"], outs["dpre1"], outs["dx"], pg["dg2"], pg["db2"], pg["dg1"], pg["db1"])
    _close(outs["dpre2"], p2.grad, 2e-5, "dpre2")
    _close(outs["dpre1"], p1.grad, 2e-5, "dpre1")
    _close(outs["dx"], Xr.grad, 2e-5, "dx")
    for k, lk in (("dg2", "g2"), ("db2", "be2"), ("dg1", "g1"), ("db1", "be1")):
        _close(pg[k], start[k].double() + leaf[lk].grad, 2e-5, f"{k} (start + gradient)")
    # fused vs unfused on the same rows: LayerNorm+ReLU of the saved pre-activations, and its backward from the fused dy
    for i, (gk, bk) in ((1, ("g1", "be1")), (2, ("g2", "be2"))):
        p_i, y_i, st_i = sv[3 * (i - 1)], sv[3 * (i - 1) + 1], sv[3 * (i - 1) + 2]
        yu, stu = torch.full((M, 64), NAN, device=cuda), torch.full((M, 2), NAN, device=cuda)
        K_.ln_relu_fwd(p_i, d[gk], d[bk], yu, stu)
        _close(yu, y_i.cpu(), 1e-5, f"unfused y{i} vs fused")
        _close(stu, st_i.cpu(), 1e-5, f"unfused st{i} vs fused")
    dy2 = torch.empty(M, 64, device=cuda)
    K_.dense_fwd(dgi.to(cuda), d["Wi"], None, dy2, trans_w=True)
    dp2u = torch.full((M, 64), NAN, device=cuda)
    ug, ub = start["dg2"].to(cuda).clone(), start["db2"].to(cuda).clone()
    K_.ln_relu_bwd(sv[3], sv[4], sv[5], d["g2"], dy2, dp2u, ug, ub)
    _close(dp2u, outs["dpre2"].cpu(), 2e-5, "unfused dpre2 vs fused")
    _close(ug, pg["dg2"].cpu(), 2e-5, "unfused dg2 vs fused")
    _close(ub, pg["db2"].cpu(), 2e-5, "unfused db2 vs fused")


def test_mlp_gi_fused_constant_and_cancelling_rows(cuda):
    """the fused forward on pre-activation rows that are constant (X row = 0: p1 = b1 = 100 in every column) or have mean 100
    and std ~0.1 (small X): y1 within the bound measured as for dgppo_ln_relu_fwd's special rows, 4 x the float32 CPU
    evaluation's own error, for the fused and for the unfused kernel; y1 equals the float64 formula evaluated with the saved
    st1 (1e-5); and dgppo_mlp_gi_bwd on these rows gives what the unfused dgppo_ln_relu_bwd gives from the same saved
    activations (2e-5), the LayerNorm gradients accumulated onto non-zero starts."""
    from dgppo_amd import ops_nn as K_
    M = 67
    g = torch.Generator().manual_seed(9)
    P = _mlp_params(g)
    P["b1"] = torch.full((64,), 100.0)
    P["be1"] = P["be1"] + 0.5 * torch.sign(P["be1"])
    X = torch.randn(M, 64, generator=g) * (0.1 / (0.2 * 8.0))          # X W1 has std ~0.1
    X[::3] = 0.0
    gi, sv = _mlp_gi_run(K_, P, X, 0, True, cuda)
    torch.cuda.synchronize()
    p1 = sv[0].cpu()
    assert torch.equal(p1[::3], torch.full_like(p1[::3], 100.0))
    lnp = {"scale": P["g1"], "bias": P["be1"]}
    y64 = torch.relu(T.layer_norm({k: v.double() for k, v in lnp.items()}, p1.double()))
    y32 = torch.relu(T.layer_norm(lnp, p1))
    yu = torch.full((M, 64), NAN, device=cuda)
    K_.ln_relu_fwd(sv[0], P["g1"].to(cuda), P["be1"].to(cuda), yu, torch.empty(M, 2, device=cuda))
    for rows, nm in ((slice(0, None, 3), "constant"), (slice(1, None, 3), "cancelling")):
        ref_err = float((y32[rows].double() - y64[rows]).abs().max())
        for got, who in ((sv[1], "fused"), (yu, "unfused")):
            err = float((got.cpu()[rows].double() - y64[rows]).abs().max())
            print(f"{nm} rows, {who} y1: float32 CPU max error {ref_err:.3e}, device max error {err:.3e}")
            assert err <= 4.0 * ref_err, f"{nm} rows, {who} y1: error {err:.3e} > 4 x {ref_err:.3e}"
    assert torch.isfinite(gi).all() and all(torch.isfinite(t).all() for t in sv)
    m_, r_ = sv[2][:, 0:1].cpu().double(), sv[2][:, 1:2].cpu().double()
    assert torch.equal(m_[::3], torch.full_like(m_[::3], 100.0))
    _close(sv[1], torch.relu((p1.double() - m_) * r_ * P["g1"].double() + P["be1"].double()), 1e-5, "y1 from the saved st1")
    # the fused backward against the unfused one, stage 1 (the special rows), from the same saved activations
    d = {k: v.to(cuda) for k, v in P.items()}
    dgi = torch.randn(M, 192, generator=g).to(cuda)
    start = {k: torch.randn(64, generator=g) for k in ("dg2", "db2", "dg1", "db1")}
    pg = {k: v.to(cuda).clone() for k, v in start.items()}
    outs = {k: torch.full((M, 64), NAN, device=cuda) for k in ("dpre2", "dpre1", "dx")}
    K_.mlp_gi_bwd(dgi, d["Wi"], d["W2"], d["W1"], d["g2"], d["g1"], sv[3], sv[4], sv[5], sv[0], sv[1], sv[2], None,
                  outs["dpre2"], outs["dpre1"], outs["dx"], pg["dg2"], pg["db2"], pg["dg1"], pg["db1"])
    dy1 = torch.empty(M, 64, device=cuda)
    K_.dense_fwd(outs["dpre2"], d["W2"], None, dy1, trans_w=True)
    dp1u = torch.full((M, 64), NAN, device=cuda)
    ug, ub = start["dg1"].to(cuda).clone(), start["db1"].to(cuda).clone()
    K_.ln_relu_bwd(sv[0], sv[1], sv[2], d["g1"], dy1, dp1u, ug, ub)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in outs.values())
    _close(outs["dpre1"], dp1u.cpu(), 2e-5, "fused dpre1 vs unfused")
    _close(pg["dg1"], ug.cpu(), 2e-5, "fused dg1 vs unfused")
    _close(pg["db1"], ub.cpu(), 2e-5, "fused db1 vs unfused")


# ----------------------------------------------------------------------------------------------------------------------
# 4. GRU gates at saturation
# ----------------------------------------------------------------------------------------------------------------------
def _gru_case(n_grp, T_, n_inner, seed):
    """gate pre-activations far into saturation: a third of the rows of gi scaled to reach +-30, a third +-90, a few entries
    +-1e4 (the exponential of the fast sigmoid / tanh overflows) and +-1e-4; h0 entries are +-1"""
    g = torch.Generator().manual_seed(seed)
    n_seq, rows = n_grp * n_inner, n_grp * n_inner * T_
    gi = torch.randn(rows, 192, generator=g)
    scale = torch.tensor([1.0, 10.0, 30.0])[torch.arange(rows) % 3]
    gi = gi * scale[:, None]
    flat = gi.view(-1)
    pick = torch.randperm(flat.numel(), generator=g)[:8 * max(rows // 8, 1)]
    for j, v in enumerate((1e4, -1e4, 1e-4, -1e-4)):
        flat[pick[j::4]] = v
    if rows >= 3:
        assert float(gi.abs().max()) == 1e4 and float((gi.abs() < 1e3).float().mul(gi.abs()).max()) >= (90.0 if rows >= 20 else 30.0)
    h0 = torch.sign(torch.randn(n_seq, 64, generator=g))
    p = T.init_gru(g)
    Wh = torch.cat([p[k]["kernel"] for k in ("hr", "hz", "hn")], 1).contiguous()
    bhn = torch.randn(64, generator=g) * 0.1
    dhs = torch.randn(rows, 64, generator=g)
    return gi, h0, Wh, bhn, dhs


def _gru_oracle(gi, h0, Wh, bhn, dhs, n_grp, T_, n_inner):
    """float64 scan of nn_torch.gru_cell.  The cell's input Denses take a zero-width input and carry the r | z | n thirds of gi
    as their (per-row) bias, so its pre-activations are gi's entries exactly and a NaN entry stays in its column (a selector
    matrix would spread it: NaN * 0); the hn bias is a per-step leaf, whose gradient is d hn_lin = dgh[:, 128:]"""
    x = gi.double().view(n_grp, T_, n_inner, 192).clone().requires_grad_()
    h = h0.double().view(n_grp, n_inner, 64)
    Wh = Wh.double()
    none, k0 = torch.zeros(n_grp, n_inner, 0, dtype=torch.float64), torch.zeros(0, 64, dtype=torch.float64)
    outs, bl = [], []
    for tau in range(T_):
        b = bhn.double().expand(n_grp, n_inner, 64).clone().requires_grad_()
        p = {"ir": {"kernel": k0, "bias": x[:, tau, :, :64]}, "iz": {"kernel": k0, "bias": x[:, tau, :, 64:128]},
             "in": {"kernel": k0, "bias": x[:, tau, :, 128:]},
             "hr": {"kernel": Wh[:, :64]}, "hz": {"kernel": Wh[:, 64:128]}, "hn": {"kernel": Wh[:, 128:], "bias": b}}
        h = T.gru_cell(p, h, none)
        outs.append(h); bl.append(b)
    hs = torch.stack(outs, 1)
    if dhs is None:
        return hs.detach().reshape(-1, 64), None, None
    hs.backward(dhs.double().view(n_grp, T_, n_inner, 64))
    dgi = x.grad.reshape(-1, 192)
    dhn = torch.stack([b.grad for b in bl], 1).reshape(-1, 64)
    return hs.detach().reshape(-1, 64), dgi, dhn


GRU_SHAPES = [(1, 3, 1), (9, 7, 3), (2051, 2, 8)]          # the last: 16 408 sequences, the 32-sequence-tile kernels


@pytest.mark.parametrize("n_grp,T_,n_inner", GRU_SHAPES)
def test_gru_gates_at_saturation(cuda, n_grp, T_, n_inner):
    """dgppo_gru_fwd / _bwd / _bwd_dhn with the v_exp_f32 / v_rcp_f32 gate forms (gate_sigmoid, gate_tanh of nn_elem.hip) driven
    to |x| = 30, 90 and 1e4: hs finite and within 1e-5 of the float64 nn_torch.gru_cell scan, dgi / dgh / dhn finite and within
    2e-5; gru_bwd_dhn equals gru_bwd bit for bit where they overlap."""
    from dgppo_amd import ops_nn as K_
    gi, h0, Wh, bhn, dhs = _gru_case(n_grp, T_, n_inner, 7 * n_grp + T_)
    n_seq, rows = n_grp * n_inner, n_grp * n_inner * T_
    hs64, dgi64, dhn64 = _gru_oracle(gi, h0, Wh, bhn, dhs, n_grp, T_, n_inner)
    d = lambda t: t.to(cuda)
    hs, hprev = torch.full((rows, 64), NAN, device=cuda), torch.full((rows, 64), NAN, device=cuda)
    gates = torch.full((rows, 256), NAN, device=cuda)
    K_.gru_fwd(d(gi), d(Wh), d(bhn), d(h0), hs, hprev, gates, n_seq, T_, n_inner)
    assert torch.isfinite(hs).all() and torch.isfinite(gates).all()
    _close(hs, hs64, 1e-5, "gru hs")
    dgi, dgh = torch.full((rows, 192), NAN, device=cuda), torch.full((rows, 192), NAN, device=cuda)
    K_.gru_bwd(d(dhs), d(Wh), hprev, gates, dgi, dgh, n_seq, T_, n_inner)
    dgi2, dhn = torch.full((rows, 192), NAN, device=cuda), torch.full((rows, 64), NAN, device=cuda)
    K_.gru_bwd_dhn(d(dhs), d(Wh), hprev, gates, dgi2, dhn, n_seq, T_, n_inner)
    torch.cuda.synchronize()
    for t, nm in ((dgi, "dgi"), (dgh, "dgh"), (dhn, "dhn")):
        assert torch.isfinite(t).all(), nm
    _close(dgi, dgi64, 2e-5, "dgi")
    _close(dgh, torch.cat([dgi64[:, :128], dhn64], 1), 2e-5, "dgh")
    _close(dhn, dhn64, 2e-5, "dhn")
    assert _bits_equal(dgi2, dgi) and _bits_equal(dhn, dgh[:, 128:]), "gru_bwd_dhn differs from gru_bwd"


@pytest.mark.parametrize("n_grp,T_,n_inner", GRU_SHAPES)
def test_gru_fwd_nan_stays_in_its_sequence(cuda, n_grp, T_, n_inner):
    """one NaN entry in gi of one sequence at step 1: hs of that sequence is NaN exactly where the float64 scan says (the
    entry's column at step 1, every column afterwards), every other sequence keeps the bits of the clean run"""
    from dgppo_amd import ops_nn as K_
    gi, h0, Wh, bhn, _ = _gru_case(n_grp, T_, n_inner, 11 * n_grp + T_)
    n_seq, rows = n_grp * n_inner, n_grp * n_inner * T_
    s = n_seq - 1 if n_seq < 40 else n_seq - 5                 # (a sequence of the ragged last tile)
    grp, i = divmod(s, n_inner)
    row = (grp * T_ + 1) * n_inner + i
    gip = gi.clone()
    gip[row, 64 + 9] = NAN
    want, _, _ = _gru_oracle(gip, h0, Wh, bhn, None, n_grp, T_, n_inner)
    d = lambda t: t.to(cuda)

    def run(g_):
        hs = torch.full((rows, 64), 7.0, device=cuda)
        K_.gru_fwd(d(g_), d(Wh), d(bhn), d(h0), hs, None, None, n_seq, T_, n_inner)
        return hs
    hc, hp = run(gi), run(gip)
    torch.cuda.synchronize()
    assert torch.isfinite(hc).all()
    assert torch.equal(hp.isnan().cpu(), want.isnan()), "NaN pattern differs from the float64 scan"
    assert want.isnan().any() and int(want.isnan().any(1).sum()) == T_ - 1
    seq_rows = torch.tensor([(grp * T_ + tau) * n_inner + i for tau in range(T_)])
    keep = _rest(rows, seq_rows).to(cuda)
    assert _bits_equal(hp[keep], hc[keep]), "another sequence changed"


@pytest.mark.parametrize("two", [True, False], ids=["two-layer-head", "one-layer-head"])
@pytest.mark.parametrize("save", [True, False], ids=["tile-kernel", "rows-per-wave"])
def test_gru1_head_gates_at_saturation(cuda, two, save):
    """dgppo_gru1_head_fwd (its own copies of gate_sigmoid / gate_tanh in nn_fused.hip), both kernels (with saves: 32-row tiles;
    inference: rows per wave), on the saturated pre-activations: hs within 1e-5, the head output within 2e-5 of float64"""
    from dgppo_amd import ops_nn as K_
    M = 613
    gi, h0, Wh, bhn, _ = _gru_case(M, 1, 1, 23 + int(two))
    g = torch.Generator().manual_seed(5)
    n_out = 4 if two else 2
    if two:
        W1, b1 = torch.randn(64, 64, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1
        W2, b2 = torch.randn(64, n_out, generator=g) * 0.2, torch.randn(n_out, generator=g) * 0.1
    else:
        W1, b1, W2, b2 = torch.randn(64, n_out, generator=g) * 0.2, torch.randn(n_out, generator=g) * 0.1, None, None
    hs64, _, _ = _gru_oracle(gi, h0, Wh, bhn, None, M, 1, 1)
    u64 = hs64 @ W1.double() + b1.double()
    out64 = u64 @ W2.double() + b2.double() if two else u64
    d = lambda t: None if t is None else t.to(cuda)
    hs, out = torch.full((M, 64), NAN, device=cuda), torch.full((M, n_out), NAN, device=cuda)
    hprev = torch.full((M, 64), NAN, device=cuda) if save else None
    gates = torch.full((M, 256), NAN, device=cuda) if save else None
    u = torch.full((M, 64), NAN, device=cuda) if (save and two) else None
    K_.gru1_head_fwd(d(gi), d(Wh), d(bhn), d(h0), d(W1), d(b1), d(W2), d(b2), hs, hprev, gates, u, out)
    torch.cuda.synchronize()
    assert torch.isfinite(hs).all() and torch.isfinite(out).all()
    _close(hs, hs64, 1e-5, "hs")
    _close(out, out64, 2e-5, "out")
    if save:
        assert torch.isfinite(gates).all() and _bits_equal(hprev, d(h0))
        # the scan kernel on the same rows saves the same gates
        hs2, hp2, g2 = (torch.full(s_, NAN, device=cuda) for s_ in ((M, 64), (M, 64), (M, 256)))
        K_.gru_fwd(d(gi), d(Wh), d(bhn), d(h0), hs2, hp2, g2, M, 1, 1)
        _close(gates, g2.cpu(), 1e-5, "gates vs gru_fwd")
        _close(hs, hs2.cpu(), 1e-5, "hs vs gru_fwd")


# ----------------------------------------------------------------------------------------------------------------------
# 5. dgppo_gnn_prep / dgppo_gnn_unprep
# ----------------------------------------------------------------------------------------------------------------------
def _prep64(th, F, Fp, D, H, Kp):
    """the header comment of nn_prep.hip in float64"""
    Wq, bq, Wk, Wv, bv, We, Wu = th
    dt = Wq.dtype
    sc = 1.0 / math.sqrt(D)
    q, k = Wq.reshape(F, H, D), Wk.reshape(F, H, D)
    M = torch.zeros(Fp, H, Fp, dtype=dt)
    M[:F, :, :F] = sc * torch.einsum("fhd,ghd->fhg", q, k)
    c = torch.zeros(H, Fp, dtype=dt)
    c[:, :F] = sc * torch.einsum("hd,ghd->hg", bq.reshape(H, D), k)
    Wout = torch.zeros(Kp, D, dtype=dt)
    Wout[:F] = Wu
    for h in range(H):
        r0 = Fp + h * (Fp + 4)
        Wout[r0:r0 + F] = Wv.reshape(F, H, D)[:, h] / H
        Wout[r0 + Fp:r0 + Fp + 4] = We.reshape(4, H, D)[:, h] / H
    Wout[Fp + H * (Fp + 4)] = bv.reshape(H, D).mean(0)
    return M.reshape(Fp, H * Fp), c.reshape(H * Fp), Wout


def _prep_shapes():
    from dgppo_amd import _native as N, nets
    cfg = N.make_env_cfg(0, 8, 3)
    net = nets.Net("policy", cfg, 2, 2, torch.device("cpu"))
    shapes = [(f, fp, d, nets.H_HEADS, kp) for f, fp, d, kp in net.dims]
    assert len(shapes) == 2
    return shapes + [(5, 8, 32, 3, 48), (64, 64, 128, 8, 64 + 8 * 68 + 1 + 7)]


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["net-layer0", "net-layer1", "F5-Fp8", "F64-H8-Kp-tail"])
def test_gnn_prep_and_unprep_against_float64(cuda, which):
    """dgppo_gnn_prep: Mcat, cvec, Wout equal the header formulas in float64 (1e-6 of the tensor's maximum); padded rows /
    columns (f, g >= F) and the rows past Fp + H (Fp + 4) are exactly 0 although the buffers start as NaN.  dgppo_gnn_unprep
    adds, onto non-zero starts, the adjoint: equal to torch autograd of the float64 prep, and <prep'(theta) dtheta, dout> =
    <dtheta, unprep(dout)> to 1e-5.  The last shape has > 16 384 outputs (grid-stride pass) and Kp 7 above the minimum."""
    from dgppo_amd import ops_nn as K_
    F, Fp, D, H, Kp = _prep_shapes()[which]
    if which == 3:
        assert Fp * H * Fp + H * Fp + Kp * D > 16384 and Kp > Fp + H * (Fp + 4) + 1
    g = torch.Generator().manual_seed(which)
    shp = [(F, H * D), (H * D,), (F, H * D), (F, H * D), (H * D,), (4, H * D), (F, D)]
    th = [torch.randn(*s, generator=g) * 0.3 for s in shp]
    out_shp = [(Fp, H * Fp), (H * Fp,), (Kp, D)]
    outs = [torch.full(s, NAN, device=cuda) for s in out_shp]
    K_.gnn_prep(*[t.to(cuda) for t in th], *outs, F, Fp, D, H, Kp)
    torch.cuda.synchronize()
    th64 = [t.double().requires_grad_() for t in th]
    want = _prep64(th64, F, Fp, D, H, Kp)
    for got, w, nm in zip(outs, want, ("Mcat", "cvec", "Wout")):
        w = w.detach()
        assert torch.isfinite(got).all(), nm
        err, mx = float((got.cpu().double() - w).abs().max()), float(w.abs().max())
        assert err <= 1e-6 * mx, f"{nm}: {err:.3e} > 1e-6 x {mx:.3e}"
        assert torch.equal(got.cpu() == 0, w == 0) or float(got.cpu()[w == 0].abs().max()) == 0.0, f"{nm}: padding is not exactly 0"
    M_, c_, W_ = (o.cpu() for o in outs)
    M3 = M_.view(Fp, H, Fp)
    assert float(M3[F:].abs().sum()) == 0 and float(M3[:, :, F:].abs().sum()) == 0 and float(c_.view(H, Fp)[:, F:].abs().sum()) == 0
    assert float(W_[F:Fp].abs().sum()) == 0 and float(W_[Fp + H * (Fp + 4) + 1:].abs().sum()) == 0
    for h in range(H):
        assert float(W_[Fp + h * (Fp + 4) + F:Fp + h * (Fp + 4) + Fp].abs().sum()) == 0
    # ---- adjoint ----
    dout = [torch.randn(*s, generator=g) for s in out_shp]
    sum(((w * d.double()).sum() for w, d in zip(want, dout))).backward()
    start = [torch.randn(*s_, generator=g) for s_ in shp]              # dWq dbq dWk dWv dbv dWe dWu
    grads = [s.to(cuda).clone() for s in start]
    K_.gnn_unprep(*[t.to(cuda) for t in dout], th[0].to(cuda), th[1].to(cuda), th[2].to(cuda), *grads, F, Fp, D, H, Kp)
    torch.cuda.synchronize()
    names = ("dWq", "dbq", "dWk", "dWv", "dbv", "dWe", "dWu")
    un = []
    for got, s0, t64, nm in zip(grads, start, th64, names):
        delta = got.cpu().double() - s0.double()
        un.append(delta)
        wantg = t64.grad
        total = s0.double() + wantg
        err, mx = float((got.cpu().double() - total).abs().max()), float(max(total.abs().max(), wantg.abs().max()))
        assert err <= 1e-5 * mx, f"{nm}: start + gradient off by {err:.3e} (scale {mx:.3e})"
    dth = [torch.randn(*s, generator=g).double() for s in shp]
    _, jv = torch.autograd.functional.jvp(lambda *a: _prep64(a, F, Fp, D, H, Kp), tuple(t.detach() for t in th64), tuple(dth))
    lhs = sum(float((j * d.double()).sum()) for j, d in zip(jv, dout))
    rhs = sum(float((a * b).sum()) for a, b in zip(dth, un))
    print(f"adjoint identity: lhs {lhs!r} rhs {rhs!r}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), f"adjoint identity: {lhs!r} vs {rhs!r}"


def test_gnn_prep_refuses_a_short_kp(cuda):
    from dgppo_amd import ops_nn as K_
    F, Fp, D, H = 5, 8, 32, 3
    Kp = Fp + H * (Fp + 4) + 1 - 1
    z = lambda *s: torch.zeros(*s, device=cuda)
    th = [z(F, H * D), z(H * D), z(F, H * D), z(F, H * D), z(H * D), z(4, H * D), z(F, D)]
    with pytest.raises(ValueError, match="Kp too small"):
        K_.gnn_prep(*th, z(Fp, H * Fp), z(H * Fp), z(Kp + 1, D), F, Fp, D, H, Kp)
    with pytest.raises(ValueError, match="Kp too small"):
        K_.gnn_unprep(z(Fp, H * Fp), z(H * Fp), z(Kp + 1, D), th[0], th[1], th[2], *[t.clone() for t in th], F, Fp, D, H, Kp)
