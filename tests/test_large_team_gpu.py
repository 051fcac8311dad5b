"""Teams of up to 64 agents on the GPU: the tiled attention kernels (attn_tiled.hip, family TILED) against the float64
oracle at the smallest shapes that leave the whole-graph families, forward determinism, and the engine / rollout / API
paths at team sizes whose attention layers are tiled."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dgppo_ref as R
from oracle import env_np as E
from oracle import nn_torch as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_IMAGE = 64 * 1024


# ---- kernel level ---------------------------------------------------------------------------------------------------------
def _image_bytes(cfg, F, H, bwd):
    """the whole-graph LDS image of dgppo_attn_fwd / dgppo_attn_bwd (attn.hip attn_image_bytes): above 64 KB the call
    takes the tiled family (before this family existed it was refused: "graph too large for LDS")"""
    n, S, Ns = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1
    if bwd:
        return 4 * (Ns * (F + 1) + n * H * (F + 1) + n * S * 4 + 2 * n * S * H + n * H * (F + 5))
    return 4 * (Ns * (F + 1) + n * H * (F + 1) + n * S * 5 + n * S * H)


def _close(got, want, tol, name):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} (scale {scale:.3e})")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e})"


def _attn_inputs(cfg, F, H, Kp, G, gen, p_masked, on=1):
    """random operands of dgppo_attn_fwd / _bwd for G graphs of topology cfg: slots masked with probability p_masked except
    the first `on`; masked slots carry NaN edge features."""
    n, S = cfg.n_agents, cfg.fan_in
    n_other = cfg.num_nodes - 1 - n
    R_ = G * n
    em = (torch.rand(R_, S, generator=gen) > p_masked).float()
    em[:, :on] = 1.0
    ef = torch.randn(R_, S, 4, generator=gen)
    ef[em == 0] = float("nan")                 # masked slots must never be multiplied
    return dict(qt=torch.randn(R_, H * F, generator=gen), Xa=torch.randn(R_, F, generator=gen),
                Xo=torch.randn(G * n_other, F, generator=gen) if n_other > 0 else None, ef=ef, em=em,
                dz=torch.randn(R_, Kp, generator=gen))


def _attn_reference(cfg, F, H, Kp, G, inp):
    """float64 forward (oracle/nn_torch.py attn_fixed_fan_in) and its autograd backward, in the kernels' flat layouts."""
    n, S = cfg.n_agents, cfg.fan_in
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread)
    leaf = lambda t, *shp: t.double().reshape(*shp).requires_grad_()
    qt, Xa = leaf(inp["qt"], G, n, H, F), leaf(inp["Xa"], G, n, F)
    Xo = leaf(inp["Xo"], G, -1, F) if inp["Xo"] is not None else None
    z, a = T.attn_fixed_fan_in(snd, qt, Xa, Xo, inp["ef"].double().reshape(G, n, S, 4), inp["em"].double().reshape(G, n, S), Kp)
    (z * inp["dz"].double().reshape(G, n, Kp)).sum().backward()
    out = dict(z=z.reshape(G * n, Kp), at=a.reshape(G * n, S, H), dq=qt.grad.reshape(G * n, H * F), dXa=Xa.grad.reshape(G * n, F))
    if Xo is not None:
        out["dXo"] = Xo.grad.reshape(-1, F)
    return out


def _attn_run(cfg, F, H, Kp, G, inp, dev):
    """forward, backward with input gradients, the same backward with relu_xo, and the dqt-only backward (first-layer form)."""
    from dgppo_amd import ops_nn as K_
    n, S = cfg.n_agents, cfg.fan_in
    R_ = G * n
    d = {k: (v.to(dev) if v is not None else None) for k, v in inp.items()}
    z = torch.full((R_, Kp), float("nan"), device=dev)
    at = torch.full((R_, S, H), float("nan"), device=dev)
    K_.attn_fwd(cfg, F, H, Kp, d["qt"], d["Xa"], d["Xo"], d["ef"], d["em"], z, at, G)
    dq = torch.full((R_, H * F), float("nan"), device=dev)
    dXa = torch.full((R_, F), float("nan"), device=dev)
    dXo = torch.full_like(d["Xo"], float("nan")) if d["Xo"] is not None else None
    K_.attn_bwd(cfg, F, H, Kp, d["dz"], at, d["qt"], d["Xa"], d["Xo"], d["ef"], dq, dXa, dXo, G)
    out = dict(z=z, at=at, dq=dq, dXa=dXa, **({"dXo": dXo} if dXo is not None else {}))
    if dXo is not None:
        dq2, dXa2 = torch.empty_like(dq), torch.empty_like(dXa)
        dXo2 = torch.full_like(dXo, float("nan"))
        K_.attn_bwd(cfg, F, H, Kp, d["dz"], at, d["qt"], d["Xa"], d["Xo"], d["ef"], dq2, dXa2, dXo2, G, relu_xo=True)
        torch.cuda.synchronize()
        assert torch.equal(dq2, dq) and torch.equal(dXa2, dXa)
        assert torch.equal(dXo2, torch.where(d["Xo"] > 0, dXo, torch.zeros_like(dXo))), "relu_xo must equal masking afterwards"
    dq3 = torch.full((R_, H * F), float("nan"), device=dev)
    K_.attn_bwd(cfg, F, H, Kp, d["dz"], at, d["qt"], d["Xa"], d["Xo"], d["ef"], dq3, None, None, G)
    torch.cuda.synchronize()
    out["dq_only"] = dq3
    return out


# (kind, n, n_obs, the passes whose whole-graph image is beyond 64 KB at H = 3: exactly these take the tiled kernels)
ALL = {"fwd8", "bwd8", "fwd32", "bwd32"}
TILED_CASES = [
    ("LidarSpread", 18, 3, {"bwd32"}),                       # first tiled backward at F = 32; forward on an old family
    ("LidarSpread", 21, 3, {"fwd32", "bwd32"}),              # first tiled forward
    ("LidarSpread", 24, 3, {"bwd8", "fwd32", "bwd32"}),      # first tiled backward at F = 8
    ("LidarSpread", 27, 3, ALL),                             # first tiled forward at F = 8
    ("LidarSpread", 61, 3, ALL),                             # receiver tiles of 8 (16 up to n = 48 / 56), ragged last tile
    ("LidarSpread", 64, 3, ALL),
    ("LidarSpread", 23, 0, {"bwd32"}),                       # no private nodes on a LiDAR kind
    ("LidarTarget", 20, 3, {"bwd32"}),                       # private goal + private hits
    ("LidarBicycleTarget", 20, 8, {"bwd32"}),
    ("LidarLine", 21, 2, {"bwd32"}),                         # 2 shared landmarks
    ("MPESpread", 22, 3, {"bwd32"}),                         # every node shared
    ("MPETarget", 28, 3, {"bwd32"}),                         # private goal between the shared agents and obstacles
    ("MPETarget", 64, 13, ALL),
    ("MPEFormation", 29, 3, {"bwd32"}),                      # 1 shared landmark
    ("MPEConnectSpread", 23, 3, {"bwd32"}),
]


@pytest.mark.parametrize("kind,n,n_obs,tiled", TILED_CASES, ids=[f"{k}-{n}-{o}" for k, n, o, _ in TILED_CASES])
def test_tiled_attention_against_float64_oracle(cuda, kind, n, n_obs, tiled):
    """dgppo_attn_fwd / _bwd at the smallest team sizes whose whole-graph LDS image exceeds 64 KB (and at n = 64), F = 8
    and F = 32, every output against the float64 reference at 2e-5 of the output scale: z, attn, dqt, dXa, dXo, the
    dqt-only backward and the relu_xo identity.  Slots are masked with p = 0.3 except the first, NaN edge features behind
    the mask.  Most n values are no multiple of the receiver tile (16; 8 at n = 61 and 64): ragged last tiles.  Every case first proves,
    from the two image formulas, which passes are beyond the old limit, so that it cannot land on an old family."""
    from dgppo_amd import _native as N
    cfg = N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs)
    H, G = 3, 5
    beyond = {f"{p}{F}" for F in (8, 32) for p in ("fwd", "bwd") if _image_bytes(cfg, F, H, p == "bwd") > LDS_IMAGE}
    assert beyond == tiled and "bwd32" in beyond, (kind, n, n_obs, sorted(beyond))
    gen = torch.Generator().manual_seed(N.ENV_KINDS[kind] * 1000 + n * 10 + n_obs)
    for F, Kp in ((8, 48), (32, 144)):
        inp = _attn_inputs(cfg, F, H, Kp, G, gen, 0.3)
        got, want = _attn_run(cfg, F, H, Kp, G, inp, cuda), _attn_reference(cfg, F, H, Kp, G, inp)
        for k, v in got.items():
            assert torch.isfinite(v).all(), f"F={F}: non-finite values in {k}"
            _close(v, want["dq" if k == "dq_only" else k], 2e-5, f"{kind} n={n} F={F} {k}")


def test_tiled_forward_is_bit_reproducible(cuda):
    """rollout replay relies on it: two forward launches on the same inputs (LidarSpread n = 21, F = 32: tiled) give equal
    bits in zcat and attn."""
    from dgppo_amd import _native as N, ops_nn as K_
    cfg = N.make_env_cfg(0, 21, 3)
    F, H, Kp, G = 32, 3, 144, 64
    assert _image_bytes(cfg, F, H, False) > LDS_IMAGE
    inp = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(5), 0.3)
    d = {k: (v.to(cuda) if v is not None else None) for k, v in inp.items()}
    outs = []
    for _ in range(2):
        z = torch.full((G * 21, Kp), float("nan"), device=cuda)
        at = torch.full((G * 21, cfg.fan_in, H), float("nan"), device=cuda)
        K_.attn_fwd(cfg, F, H, Kp, d["qt"], d["Xa"], d["Xo"], d["ef"], d["em"], z, at, G)
        outs.append((z, at))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- engine level ---------------------------------------------------------------------------------------------------------
def _np_rollout(ro):
    c = lambda x: None if x is None else x.detach().cpu().numpy()
    return dict(agent=c(ro.agent), hits=c(ro.hits), goal=c(ro.goal), obst=c(ro.obst), actions=c(ro.actions),
                log_pis=c(ro.log_pis), rnn_states=c(ro.rnn_states.contiguous()), rewards=c(ro.rewards), costs=c(ro.costs))


def _setup(kind_name, n, n_obs, T_, cuda, batch_size, rnn_step, **engine_kw):
    from dgppo_amd import _native as N, engine as EN, init
    kind = N.ENV_KINDS[kind_name]
    cfg = N.make_env_cfg(kind, n, n_obs)
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs)
    hp = EN.Hyper(batch_size=batch_size, rnn_step=rnn_step, train_steps=100, use_rnn=True, rnn_layers=1, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_, **engine_kw)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, 1, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=1, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=1)}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(np.float32)), tr)
    trees = {k: jitter(v) for k, v in trees.items()}
    trees["policy"]["params"]["ScaleHid"]["kernel"] = T.orthogonal(torch.Generator().manual_seed(1), 64, 64, 0.5)
    for k, net in eng.nets.items():
        net.load_tree(trees[k])
    eng.set_entropy_noise(77)
    return cfg, ocfg, hp, eng, trees


def _close_np(got, want, name, tol=1e-5):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{name}: max error {err:.3e} (scale {scale:.3g})")
    assert err <= tol * scale, f"{name}: max error {err:.3e} > {tol:g} x scale {scale:.3g}"


def _check_advantage(tg, wt, dt, alpha, cbf_eps, w, label=""):
    """The three-part advantage check of tests/test_engine_gpu.py: (1) the advantage kernel on the device's own Vl / Vh / Ql
    equals the oracle formula on those inputs to 1e-5, gate flips only where |cdot| is at rounding level; (2) end to end a
    gate differs from the oracle's only inside the propagated error band of Vh, and rarely; (3) every entry whose gate
    agrees is within the propagated numeric bound."""
    from oracle import algo_ref as A
    g = {k: tg[k].cpu().numpy() for k in ("Vl", "Vh", "Ql", "adv")}
    same_in, _ = A.advantage(g["Ql"], g["Vl"], g["Vh"], dt, alpha, cbf_eps, w)
    deriv_g = (g["Vh"][:, 1:] - g["Vh"][:, :-1]) / np.float32(dt) + np.float32(alpha) * g["Vh"][:, :-1]
    rounding_level = (np.abs(deriv_g) < 1e-5).any(axis=-1)
    bad1 = np.abs(g["adv"] - same_in) > 1e-5 * np.maximum(1, np.abs(same_in))
    assert not (bad1 & ~rounding_level).any(), f"{label}: advantage kernel off by more than 1e-5 on identical inputs"
    errVh = float(np.abs(g["Vh"] - wt["Vh"]).max())
    band = errVh * (2.0 / dt + alpha) + 1e-6
    deriv_o = (wt["Vh"][:, 1:] - wt["Vh"][:, :-1]) / np.float32(dt) + np.float32(alpha) * wt["Vh"][:, :-1]
    safe_g, safe_o = (deriv_g <= 0).all(axis=-1), (deriv_o <= 0).all(axis=-1)
    flipped = safe_g != safe_o
    borderline = (np.abs(deriv_o) <= band).any(axis=-1)
    assert not (flipped & ~borderline).any(), f"{label}: a safe-gate decision differs away from the threshold (band {band:.2e})"
    assert flipped.mean() < 0.02, f"{label}: {flipped.sum()} of {flipped.size} gates flipped"
    Al_o = wt["Ql"] - wt["Vl"][:, :-1]
    std = Al_o.std(axis=1, keepdims=True) + 1e-8
    errAl = (np.abs(g["Ql"] - wt["Ql"]).max() + np.abs(g["Vl"] - wt["Vl"]).max()) * 4.0 / std
    bound = errAl[:, :, None] + w * band + 1e-5
    err = np.abs(g["adv"] - wt["adv"])
    assert (err[~flipped] <= np.broadcast_to(bound, err.shape)[~flipped]).all(), \
        f"{label}: advantage error {err[~flipped].max():.2e} exceeds the propagated bound"


def _check_first_minibatch_grads(leaf, grads, names, tol=5e-5):
    for name in names:
        w = dict(T.tree_leaves(T.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), leaf[name])))
        gt = dict(T.tree_leaves(T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), grads[name])))
        scale = max(float(v.abs().max()) for v in w.values())
        for k in w:
            err = float((gt[k].double() - w[k].double()).abs().max())
            assert err <= tol * max(scale, 1e-3), f"{name} grad {k}: err {err:.3e} scale {scale:.3e}"
        print(f"{name}: gradients within {tol:g} of scale {scale:.3e}")


@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 24, 3), ("MPETarget", 30, 2)])
def test_update_targets_and_gradients_large_team(cuda, kind, n, n_obs):
    """tests/test_engine_gpu.py test_update_targets_and_gradients at team sizes whose attention layers are tiled: targets
    within 1e-5, the three-part advantage check, first-minibatch gradients within 5e-5 of the oracle's."""
    from dgppo_amd import _native as N
    B, T_, rs, bs = 4, 8, 4, 16
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, T_, cuda, bs, rs)
    assert _image_bytes(cfg, 32, 3, True) > LDS_IMAGE
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3)
    det = eng.rollout(seeds + 1000, False)
    ro.finalize(); det.finalize()
    step = 60
    tg = eng.targets(ro, det, step)
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, alpha=hp.alpha, cbf_eps=hp.cbf_eps, rnn_step=rs,
               clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    r, d = _np_rollout(ro), _np_rollout(det)
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), v) for k, v in trees.items()}
    wt = R.targets(leaf, ocfg, r, d, hpd, eng.cbf_weight_at(step))
    for k in ("Vl", "Vh", "Vh_det", "Ql", "Qh", "Qh_det"):
        _close_np(tg[k], wt[k], k)
    _check_advantage(tg, wt, ocfg.dt, hp.alpha, hp.cbf_eps, eng.cbf_weight_at(step), kind)
    perm = np.array([2, 0, 3, 1])
    grads = {}

    def hook(name, net, mb):
        if mb == 0:
            grads[name] = net.to_tree(net.grads)
    eng.grad_hook = hook
    Eb = bs // T_
    tg_np = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in tg.items()}
    R.minibatch_losses(leaf, ocfg, r, d, tg_np, perm[:Eb], hpd, eng.eps_hat.cpu())
    info = eng.update(ro, det, step, perm)
    _check_first_minibatch_grads(leaf, grads, ("Vl", "Vh", "policy"))
    assert all(np.isfinite(v) for v in info.values()), info
    assert info["Vl/has_nan"] == 0.0 and float(eng.opt["policy"].state[2]) == B // Eb


# ---- rollout ----------------------------------------------------------------------------------------------------------------
def test_rollout_matches_oracle_stepwise_large_team(cuda):
    """tests/test_engine_gpu.py test_rollout_matches_oracle_stepwise at LidarSpread n = 21 (tiled forward in the second GNN
    layer): every stored quantity re-derived by the oracle from the same noise."""
    kind, n, n_obs, B, T_ = "LidarSpread", 21, 3, 3, 4
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, T_, cuda, 16, 4)
    assert _image_bytes(cfg, 32, 3, False) > LDS_IMAGE
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 104729
    for stochastic in (True, False):
        ro = eng.rollout(seeds, stochastic, noise_seed=5).finalize()
        r = _np_rollout(ro)
        wa, wg, wo = E.env_reset(ocfg, [int(s) for s in seeds.cpu().numpy()])
        np.testing.assert_array_equal(r["agent"][:, 0], wa)
        np.testing.assert_array_equal(r["goal"], wg)
        np.testing.assert_allclose(r["obst"], wo, atol=1e-6)       # trig-derived rectangle fields: <= 1 ulp (device cos/sin)
        wo = r["obst"]
        tab = E.ray_table(32)
        hits = E.lidar_sense(ocfg, wa[..., :2], wo, *tab)[0]
        eps = eng.arena.get("ro.eps", T_, B * n, 2).cpu().numpy().reshape(T_, B, n, 2) if stochastic else None
        h = torch.zeros(B, n, 64)
        for t in range(T_):
            g = T.graph_to_torch(E.get_graph(ocfg, r["agent"][:, t] if t else wa, wg, wo, hits))
            with torch.no_grad():
                if stochastic:
                    a, lp, h_new = T.policy_sample(trees["policy"], g, h, n, torch.from_numpy(eps[t]))
                    _close_np(r["log_pis"][:, t], lp.numpy(), "log_pi")
                else:
                    a, h_new = T.policy_mode(trees["policy"], g, h, n)
            np.testing.assert_allclose(r["actions"][:, t], a.numpy(), atol=1e-5)
            stored = h if stochastic else h_new
            np.testing.assert_allclose(r["rnn_states"][:, t], stored.numpy(), atol=1e-5)
            out = E.env_step(ocfg, r["agent"][:, t], wg, wo, r["hits"][:, t], r["actions"][:, t], tab)
            np.testing.assert_array_equal(r["agent"][:, t + 1], out["next_agent"])
            np.testing.assert_array_equal(r["rewards"][:, t], out["reward"])
            np.testing.assert_array_equal(r["costs"][:, t], out["cost"])
            hits, h = out["next_hits"], h_new
            np.testing.assert_array_equal(r["hits"][:, t + 1], hits)


def test_rollout_hip_graph_replay_is_bit_exact_large_team(cuda):
    """Engine(use_graphs=True) at LidarSpread n = 21: eager first call, captured second, replayed third — every rollout
    equals the eager engine's bit for bit (the tiled forward is deterministic and capturable)."""
    from dgppo_amd import engine as EN
    B, T_ = 3, 4
    cfg, ocfg, hp, eng_e, trees = _setup("LidarSpread", 21, 3, T_, cuda, 16, 4)
    eng_g = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=True)
    for k, net in eng_g.nets.items():
        net.load_tree(trees[k])
    for call in range(3):
        seeds = (torch.arange(1, B + 1, dtype=torch.int64, device=cuda) + 100 * call) * 7919
        for stochastic in (True, False):
            a = eng_e.rollout(seeds, stochastic, noise_seed=3 + call).finalize()
            b = eng_g.rollout(seeds, stochastic, noise_seed=3 + call).finalize()
            for name in ("agent", "hits", "actions", "log_pis", "rnn_states", "rewards", "costs"):
                x, y = getattr(a, name), getattr(b, name)
                if x is None:                                        # log_pis of a deterministic rollout
                    assert y is None
                    continue
                assert torch.equal(x, y), f"call {call} stochastic={stochastic}: {name} differs"
    assert eng_g._ro_cache[(B, True)]["graph"] is not None and eng_g._ro_cache[(B, False)]["graph"] is not None


# ---- API ----------------------------------------------------------------------------------------------------------------------
def test_trainer_iteration_at_24_agents(cuda, tmp_path):
    """make_env("LidarSpread", 24) -> make_algo("dgppo") -> one Trainer iteration with 8 envs: finite metrics."""
    import json
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    from dgppo.trainer.trainer import Trainer
    env, env_test = make_env("LidarSpread", 24, max_step=8, num_obs=3), make_env("LidarSpread", 24, max_step=8, num_obs=3)
    algo = make_algo(algo="dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=env.num_agents, cost_weight=0.0, cbf_weight=1.0, actor_gnn_layers=2,
                     Vl_gnn_layers=2, Vh_gnn_layers=1, rnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, lr_Vh=1e-3, max_grad_norm=2.0,
                     alpha=10.0, cbf_eps=1e-2, seed=0, batch_size=4 * 8, use_rnn=True, use_lstm=False, coef_ent=1e-2,
                     rnn_step=8, gamma=0.99, clip_eps=0.25, lagr_init=0.5, lr_lagr=1e-7, train_steps=2,
                     cbf_schedule=True, cost_schedule=False)
    tr = Trainer(env=env, env_test=env_test, algo=algo, gamma=0.99, n_env_train=8, n_env_test=4, log_dir=str(tmp_path / "run"),
                 seed=0, params={"run_name": "t", "training_steps": 0, "eval_interval": 1, "eval_epi": 1, "save_interval": 1})
    tr.train()
    assert tr.update_steps == 1
    rows = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    keys = set().union(*[set(r) for r in rows])
    for k in ("eval/reward", "eval/cost", "Vl/loss", "Vh/loss_Vh", "policy/loss"):
        assert k in keys, k
    for r in rows:
        assert all(np.isfinite(v) for v in r.values() if isinstance(v, float)), r


def test_test_py_evaluates_a_small_team_checkpoint_at_24_agents(cuda, tmp_path):
    """the scalability evaluation: a run trained at -n 3 is evaluated by test.py at -n 24 (the network weights do not depend
    on n) and prints the aggregate line."""
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "3",
           "--steps", "1", "--n-env-train", "16", "--batch-size", "2048", "--n-env-test", "4", "--eval-interval", "1",
           "--save-interval", "1", "--log-dir", str(tmp_path / "logs")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    run_dir = tmp_path / "logs" / "LidarSpread" / "dgppo"
    run_dir = run_dir / os.listdir(run_dir)[0]
    tcmd = [sys.executable, os.path.join(ROOT, "test.py"), "--path", str(run_dir), "-n", "24", "--epi", "2", "--no-video",
            "--max-step", "16"]
    tout = subprocess.run(tcmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert tout.returncode == 0, tout.stderr[-2000:]
    assert "epi: 1, reward:" in tout.stdout and "min/max reward:" in tout.stdout and "safe_rate:" in tout.stdout
