"""VMASReverseTransport on the GPU: the dgppo_vmas_* kernels against the NumPy restatement (tests/vmas_np.py), the networks on
VMAS graphs against oracle/nn_torch.py, the engine's rollout and update, and train.py / test.py with the reference's flags."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vmas_np as V  # noqa: E402
from oracle import nn_torch as T  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _cfg(n):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS["VMASReverseTransport"], n, 3)


def _close(got, want, tol, name, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    s = max(1.0, float(np.abs(want).max())) if scale is None else scale
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= tol * s, f"{name}: max abs err {err:.3e} (scale {s:.3e})"


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


@pytest.mark.parametrize("n", [1, 3, 4, 8])
def test_reset_matches_restatement(cuda, n):
    from dgppo_amd import ops_env as OE
    B = 64
    seeds = (np.arange(B, dtype=np.int64) + 1) * 104729 + n
    cfg = _cfg(n)
    agent, body, scene = torch.empty(B, n, 4, device=cuda), torch.empty(B, 4, device=cuda), torch.empty(B, 8, device=cuda)
    failed = torch.zeros(1, dtype=torch.int32, device=cuda)
    OE.vmas_reset(cfg, _dev(seeds, cuda), agent, body, scene, failed)
    a, b, s = agent.cpu().numpy(), body.cpu().numpy(), scene.cpu().numpy()
    wa, wb, ws, wf = V.reset(seeds, n)
    assert int(failed.item()) == 0 == wf
    np.testing.assert_array_equal(a[..., 2:], wa[..., 2:])                   # uniform draws: bit-exact
    _close(a[..., :2], wa[..., :2], 1e-6, "agent positions", 1.0)          # shifted by the trig-derived box position
    _close(b, wb, 1e-6, "body", 1.0)
    _close(s, ws, 1e-6, "scene", 1.0)
    rel = a[..., :2] - b[:, None, :2]
    assert (np.abs(rel) < 0.3 - 0.03).all()                                   # inside the box, clear of its sides
    if n > 1:
        d = np.linalg.norm(a[:, :, None, :2] - a[:, None, :, :2], axis=-1) + np.eye(n) * 9
        assert (d > 0.06).all()


def _random_states(rng, B, n, wall_frac=0.5):
    body = np.zeros((B, 4), f32)
    body[:, :2] = rng.uniform(-0.5, 0.5, (B, 2))
    body[:, 2:] = rng.uniform(-0.2, 0.2, (B, 2))
    rel = rng.uniform(-0.22, 0.22, (B, n, 2))
    walls = rng.random(B) < wall_frac
    for b in np.nonzero(walls)[0]:                        # agents at and near the sides: some in contact
        for i in range(n):
            ax = rng.integers(0, 2)
            rel[b, i, ax] = rng.choice([-1, 1]) * (0.3 - rng.uniform(0.0, 0.045))
    agent = np.zeros((B, n, 4), f32)
    agent[..., :2] = body[:, None, :2] + rel
    agent[..., 2:] = rng.uniform(-0.3, 0.3, (B, n, 2))
    scene = rng.uniform(-0.7, 0.7, (B, 8)).astype(f32)
    action = rng.uniform(-1.6, 1.6, (B, n, 2)).astype(f32)
    return agent, body, scene, action


def _step_dev(cfg, agent, body, scene, action, cuda, want_graph=True):
    from dgppo_amd import ops_env as OE
    B, n = agent.shape[:2]
    ad, bd, sd, ud = (_dev(x, cuda) for x in (agent, body, scene, action))
    nx, nb = torch.empty_like(ad), torch.empty_like(bd)
    rew, cost = torch.empty(B, device=cuda), torch.empty(B, n, 2, device=cuda)
    g = OE.alloc_graph(cfg, B, cuda) if want_graph else None
    OE.vmas_step(cfg, ad, bd, sd, ud, nx, nb, rew, cost, g)
    out = dict(next_agent=nx.cpu().numpy(), next_body=nb.cpu().numpy(), reward=rew.cpu().numpy(), cost=cost.cpu().numpy())
    if g is not None:
        out["graph"] = {k: v.cpu().numpy() for k, v in g.items()}
    return out


def _check_step(got, want, ctx):
    """bit-exact where the restatement saw no contact in any substep and for the integer graph fields; elsewhere within
    1e-5 of the scale; the in-contact flag exact away from the 0.59 threshold"""
    free = ~want["contact"]
    for k in ("next_agent", "next_body", "reward", "cost"):
        np.testing.assert_array_equal(got[k][free], want[k][free], err_msg=f"{ctx}: {k} (no contact)")
        _close(got[k], want[k], 1e-5, f"{ctx}: {k}")
    gg, wg = got["graph"], want["graph"]
    for k in ("receivers", "senders", "node_type", "n_node", "n_edge"):
        np.testing.assert_array_equal(gg[k], wg[k], err_msg=f"{ctx}: {k}")
    for k in ("nodes", "edges"):
        np.testing.assert_array_equal(gg[k][free], wg[k][free], err_msg=f"{ctx}: graph {k} (no contact)")
    n = want["next_agent"].shape[1]
    rel = np.abs(want["next_agent"][..., :2] - want["next_body"][:, None, :2])
    sure = (np.abs(rel - V.CONTACT_THR) > 1e-6).all(-1)
    np.testing.assert_array_equal(gg["nodes"][:, :n, 10][sure], wg["nodes"][:, :n, 10][sure], err_msg=f"{ctx}: in-contact flag")
    cols = [c for c in range(20) if c != 10]
    _close(gg["nodes"][..., cols], wg["nodes"][..., cols], 1e-5, f"{ctx}: nodes")
    _close(gg["edges"], wg["edges"], 1e-5, f"{ctx}: edges")


@pytest.mark.parametrize("n", [1, 4, 8])
def test_step_matches_restatement(cuda, n):
    rng = np.random.default_rng(100 + n)
    B = 512
    agent, body, scene, action = _random_states(rng, B, n)
    want = V.env_step(agent, body, scene, action)
    assert want["contact"].mean() >= 0.25, want["contact"].mean()
    got = _step_dev(_cfg(n), agent, body, scene, action, cuda)
    _check_step(got, want, f"n={n}")


def test_chained_steps_match_restatement_stepwise(cuda):
    from dgppo_amd import ops_env as OE
    n, B = 3, 64
    cfg = _cfg(n)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    a, b, s = torch.empty(B, n, 4, device=cuda), torch.empty(B, 4, device=cuda), torch.empty(B, 8, device=cuda)
    OE.vmas_reset(cfg, seeds, a, b, s)
    rng = np.random.default_rng(7)
    scene = s.cpu().numpy()
    agent, body = a.cpu().numpy(), b.cpu().numpy()
    n_contact = 0
    for t in range(128):
        # push the agents outwards half of the time so that the box gets pushed
        action = rng.uniform(-1.3, 1.3, (B, n, 2)).astype(f32)
        want = V.env_step(agent, body, scene, action)
        got = _step_dev(cfg, agent, body, scene, action, cuda)
        _check_step(got, want, f"t={t}")
        n_contact += int(want["contact"].sum())
        agent, body = got["next_agent"], got["next_body"]              # re-feed the device state
    assert n_contact > 0


def test_graph_feats_from_strided_record(cuda):
    from dgppo_amd import nets
    n, B, T1 = 4, 6, 5
    cfg = _cfg(n)
    rng = np.random.default_rng(3)
    rec_a = rng.uniform(-0.8, 0.8, (B, T1, n, 4)).astype(f32)
    rec_b = rng.uniform(-0.8, 0.8, (B, T1, 4)).astype(f32)
    scene = rng.uniform(-0.7, 0.7, (B, 8)).astype(f32)
    env_ids = np.array([4, 1, 5], np.int32)
    t0, nt = 1, 3
    f = nets.GraphFeats(cfg, len(env_ids) * nt, nets.Arena(cuda), "t")
    ad, bd = _dev(rec_a, cuda), _dev(rec_b, cuda)
    f.compute_vmas(ad[:, t0], T1 * n * 4, n * 4, bd[:, t0], T1 * 4, 4, _dev(scene, cuda), _dev(env_ids, cuda), len(env_ids), nt)
    sel = lambda x: x[env_ids][:, t0:t0 + nt].reshape((-1,) + x.shape[2:])
    ag, bo, sc = sel(rec_a), sel(rec_b), np.repeat(scene[env_ids], nt, axis=0)
    Xw = V.node_feats(ag, bo, sc)
    ew, mw = V.edge_feats(ag)
    assert f.Fp == 20 and f.n_other == 0
    np.testing.assert_array_equal(f.Xa.cpu().numpy(), Xw.reshape(-1, 20))
    np.testing.assert_array_equal(f.efeat.cpu().numpy(), ew.reshape(-1, n, 4))
    np.testing.assert_array_equal(f.emask.cpu().numpy(), mw[None].repeat(len(ag), 0).reshape(-1, n).astype(f32))


def _grads_per_leaf(net, tree, tol=5e-5):
    gt = net.to_tree(net.grads)
    want = dict(T.tree_leaves(T.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), tree)))
    got = dict(T.tree_leaves(T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), gt)))
    assert set(got) == set(want)
    bad = []
    for k in sorted(want):
        if "GraphTransformer_" in k and k.endswith("Dense_1/bias"):
            continue                                         # the key bias cancels in the softmax
        scale = max(float(want[k].abs().max()), 1e-4)
        err = float((got[k].double() - want[k].double()).abs().max())
        if err > tol * scale:
            bad.append(f"{k}: err {err:.3e} scale {scale:.3e}")
    assert not bad, bad


def _vmas_scene(n, G, seed):
    rng = np.random.default_rng(seed)
    agent, body, scene, _ = _random_states(rng, G, n, 0.3)
    return agent, body, scene, V.get_graph(agent, body, scene)


@pytest.mark.parametrize("kind,layers,n_out", [("policy", 2, 2), ("Vl", 2, 1), ("Vh", 1, 2), ("Vhg", 1, 2)])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_networks_on_vmas_graphs_match_oracle(cuda, kind, layers, n_out, n):
    from dgppo_amd import nets, ops_nn as K_
    n_env, T_ = 3, 4
    G = n_env * T_
    cfg = _cfg(n)
    agent, body, scene, gr = _vmas_scene(n, G, 11 * n + layers)
    gen = torch.Generator().manual_seed(n)
    base = T.init_policy(1, 20) if kind == "policy" else T.init_value(2, 20, n_out, layers, global_info=(kind == "Vhg"))
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), base)
    if kind == "policy":
        tree["params"]["ScaleHid"]["kernel"] = T.orthogonal(gen, 64, 64, 0.5)
    net = nets.Net(kind, cfg, layers, n_out, cuda)
    net.load_tree(tree)
    f = nets.GraphFeats(cfg, G, net.arena, "x")
    ad, bd, sd = _dev(agent, cuda), _dev(body, cuda), _dev(scene, cuda)
    f.compute_vmas(ad, n * 4, 0, bd, 4, 0, sd, None, G, 1)
    lt = T.tree_map(lambda t: t.clone().requires_grad_(), tree)
    g_t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gr.items()}
    if kind == "policy":
        act = net.forward(f, n_seq=n_env * n, T=T_, h0=None)
        g_seq = {k: v.view((n_env, T_) + v.shape[1:]) for k, v in g_t.items()}
        rng = torch.Generator().manual_seed(9)
        a_in = torch.tanh(torch.randn(n_env, T_, n, 2, generator=rng))
        eps_hat = torch.randn(n, 2, generator=rng)
        h, lps, ents = torch.zeros(n_env, n, 64), [], []
        for t in range(T_):
            lp, ent, h = T.policy_eval(lt, {k: v[:, t] for k, v in g_seq.items()}, a_in[:, t], h, n, eps_hat)
            lps.append(lp); ents.append(ent)
        lp_w, ent_w = torch.stack(lps, 1), torch.stack(ents, 1)
        R = G * n
        lp_old = lp_w.detach() + 0.2 * torch.randn(n_env, T_, n, generator=rng)
        adv = torch.randn(n_env, T_, n, generator=rng)
        rho = torch.exp(lp_w - lp_old)
        (torch.maximum(-rho * adv, -torch.clamp(rho, 0.75, 1.25) * adv).mean() - 0.01 * ent_w.mean()).backward()
        lp, ent = torch.empty(R, device=cuda), torch.empty(R, device=cuda)
        dms, stats = torch.empty(R, 4, device=cuda), torch.zeros(8, device=cuda)
        K_.policy_head(act["ms"], eps_hat.to(cuda), a_in.reshape(R, 2).to(cuda), None, lp, ent, n, 2,
                       lp_old.reshape(R).to(cuda), adv.reshape(R).to(cuda), dms, stats, 0.25, 0.01)
        _close(lp.view(n_env, T_, n).cpu(), lp_w.detach(), 1e-5, "log_pi")
        _close(ent.view(n_env, T_, n).cpu(), ent_w.detach(), 1e-5, "entropy")
        dout = dms
    elif kind == "Vl":
        act = net.forward(f, n_seq=n_env, T=T_, h0=None)
        g_seq = {k: v.view((n_env, T_) + v.shape[1:]) for k, v in g_t.items()}
        h, vs = torch.zeros(n_env, 1, 64), []
        for t in range(T_):
            v, h = T.value_Vl(lt, {k: vv[:, t] for k, vv in g_seq.items()}, h, n)
            vs.append(v)
        v_w = torch.stack(vs, 1)
        _close(act["v"].view(n_env, T_).cpu(), v_w.detach(), 1e-5, "Vl")
        target = torch.randn(n_env, T_, generator=gen)
        (0.5 * (v_w - target) ** 2).mean().backward()
        dout = torch.empty(G, 1, device=cuda)
        K_.value_loss(act["v"], target.reshape(-1, 1).to(cuda), dout, torch.zeros(8, device=cuda))
    else:
        h0 = torch.randn(G, n, 64, generator=gen) * 0.5
        act = net.forward(f, n_seq=G * n, T=1, h0=h0.reshape(G * n, 64).to(cuda))
        v_w, _ = T.value_Vh(lt, g_t, h0, n, global_info=(kind == "Vhg"))
        _close(act["v"].view(G, n, n_out).cpu(), v_w.detach(), 1e-5, kind)
        target = torch.randn(G, n, n_out, generator=gen)
        (0.5 * (v_w - target) ** 2).mean().backward()
        dout = torch.empty(G * n, n_out, device=cuda)
        K_.value_loss(act["v"], target.reshape(-1, n_out).to(cuda), dout, torch.zeros(8, device=cuda))
    net.zero_grads()
    net.backward(act, dout)
    torch.cuda.synchronize()
    _grads_per_leaf(net, lt)


class _VmasEnvOracle:
    """oracle/dgppo_ref.py forms its graphs through its env module (E.get_graph, E.env_step).  For VMASReverseTransport the
    record travels in that module's slots: goal <- scene [B, 8] (per env), hits <- body [B, T+1, 4] (per step), obst None,
    and this stand-in maps them onto the restatement."""

    @staticmethod
    def get_graph(ocfg, agent, goal, obst, hits):
        return V.get_graph(agent, hits, goal)

    @staticmethod
    def env_step(ocfg, agent, goal, obst, hits, action, tab):
        return V.env_step(agent, hits, goal, action)

    @staticmethod
    def ray_table(n_rays):
        return None


def _np_record(ro):
    c = lambda x: None if x is None else x.detach().cpu().numpy()
    return dict(agent=c(ro.agent), goal=c(ro.scene), obst=None, hits=c(ro.body), actions=c(ro.actions), log_pis=c(ro.log_pis),
                rnn_states=c(ro.rnn_states.contiguous()), rewards=c(ro.rewards), costs=c(ro.costs))


def _engine(cfg, cuda, algo, rnn, B, T_, bs, rs, use_graphs=False):
    from dgppo_amd import engine as EN, init
    hp = EN.Hyper(batch_size=bs, rnn_step=rs, train_steps=100, use_rnn=rnn)
    eng = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=use_graphs, algo=algo)
    nc = 1 if rnn else 0
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc), "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc),
             "Vh": init.init_value(0, cfg.node_dim, 2, 1, 3, rnn_layers=nc)}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(np.float32)), tr)
    trees = {k: jitter(v) for k, v in trees.items()}
    trees["policy"]["params"]["ScaleHid"]["kernel"] = T.orthogonal(torch.Generator().manual_seed(1), 64, 64, 0.5)
    for k, net in eng.nets.items():
        net.load_tree(trees[k])
    eng.set_entropy_noise(77)
    return hp, eng, trees


def _check_rollout_stepwise(eng, ro, trees, n, stochastic):
    """every stored quantity re-derived from the device's own recorded states: the policy (oracle networks on the
    restatement's graph of agent[t], body[t], scene) and the env step (the restatement, fed the device action)"""
    r = _np_record(ro)
    B, T_ = r["actions"].shape[:2]
    agent, body, scene = r["agent"], r["hits"], r["goal"]
    eps = eng.arena.get("ro.eps", T_, B * n, 2).cpu().numpy().reshape(T_, B, n, 2) if stochastic else None
    h = torch.zeros(B, n, T.carry_width(trees["policy"]))
    for t in range(T_):
        g = T.graph_to_torch(V.get_graph(agent[:, t], body[:, t], scene))
        with torch.no_grad():
            if stochastic:
                a, lp, h_new = T.policy_sample(trees["policy"], g, h, n, torch.from_numpy(eps[t]))
                _close(r["log_pis"][:, t], lp.numpy(), 1e-5, f"log_pi t={t}")
            else:
                a, h_new = T.policy_mode(trees["policy"], g, h, n)
        _close(r["actions"][:, t], a.numpy(), 1e-5, f"action t={t}", 1.0)
        _close(r["rnn_states"][:, t], (h if stochastic else h_new).numpy(), 1e-5, f"carry t={t}", 1.0)
        want = V.env_step(agent[:, t], body[:, t], scene, r["actions"][:, t])
        free = ~want["contact"]
        np.testing.assert_array_equal(agent[:, t + 1][free], want["next_agent"][free])
        np.testing.assert_array_equal(body[:, t + 1][free], want["next_body"][free])
        _close(agent[:, t + 1], want["next_agent"], 1e-5, f"agent t={t}")
        _close(body[:, t + 1], want["next_body"], 1e-5, f"body t={t}")
        np.testing.assert_array_equal(r["rewards"][:, t], want["reward"])
        np.testing.assert_array_equal(r["costs"][:, t], want["cost"])
        h = h_new
    return r


@pytest.mark.parametrize("algo,rnn", [("dgppo", True), ("dgppo", False), ("informarl", True), ("informarl", False),
                                      ("hcbfcrpo", True)])
def test_engine_rollout_targets_and_gradients(cuda, monkeypatch, algo, rnn):
    """Engine on VMASReverseTransport: rollouts stepwise against the restatement plus the oracle networks, the targets of
    the value pre-passes and the first minibatch's gradients against autograd on the oracle (oracle/dgppo_ref.py with the
    VMAS graphs), graph replay equal to eager, and two rollouts with the same seeds bit-identical."""
    from oracle import dgppo_ref as R
    from test_engine_gpu import _check_advantage, _check_first_minibatch_grads
    monkeypatch.setattr(R, "E", _VmasEnvOracle)
    n, B, T_, rs, bs = 3, 8, 32, 8, 64
    cfg = _cfg(n)
    ocfg = types.SimpleNamespace(n_agents=n, dt=cfg.dt, n_rays=0)
    hp, eng, trees = _engine(cfg, cuda, algo, rnn, B, T_, bs, rs)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 31
    ro = eng.rollout(seeds, True, noise_seed=5).finalize()
    assert int(eng.reset_failed.item()) == 0
    wa, wb, ws, _ = V.reset(seeds.cpu().numpy(), n)
    _close(ro.agent[:, 0].cpu().numpy(), wa, 1e-6, "reset agent", 1.0)
    _close(ro.body[:, 0].cpu().numpy(), wb, 1e-6, "reset body", 1.0)
    _close(ro.scene.cpu().numpy(), ws, 1e-6, "reset scene", 1.0)
    r = _check_rollout_stepwise(eng, ro, trees, n, True)
    det = eng.rollout(seeds + 100, False).finalize() if algo == "dgppo" else None
    d = _check_rollout_stepwise(eng, det, trees, n, False) if det is not None else None
    # the same seeds give the same rollout, and the captured graph replays it bit for bit
    ro2 = eng.rollout(seeds, True, noise_seed=5).finalize()
    _, graphed, _ = _engine(cfg, cuda, algo, rnn, B, T_, bs, rs, use_graphs=True)
    for _ in range(2):                                        # the second call replays the captured graph
        rg = graphed.rollout(seeds, True, noise_seed=5)
    assert graphed._ro_cache[(B, True)]["graph"] is not None          # replayed, not the eager fall-back
    rg.finalize()
    for name in ("agent", "body", "actions", "rewards", "costs", "log_pis"):
        assert torch.equal(getattr(ro2, name), getattr(ro, name)), name
        assert torch.equal(getattr(rg, name), getattr(ro, name)), name
    # targets of the value pre-passes (the strided body / scene record) against the oracle
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, alpha=hp.alpha, cbf_eps=hp.cbf_eps, rnn_step=rs,
               clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    names = ("Vl", "Vh", "policy") if algo == "dgppo" else ("Vl", "policy")
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), trees[k]) for k in names}
    step = 60
    if algo == "dgppo":
        tg = eng.targets(ro, det, step)
        wt = R.targets(leaf, ocfg, r, d, hpd, eng.cbf_weight_at(step))
        for k in ("Vl", "Vh", "Vh_det", "Ql", "Qh", "Qh_det"):
            _close(tg[k].cpu().numpy(), wt[k], 1e-5, k)
        _check_advantage(tg, wt, cfg.dt, hp.alpha, hp.cbf_eps, eng.cbf_weight_at(step), "VMAS")
    elif algo == "informarl":
        tg = eng.targets_informarl(ro, step)
        wt = R.targets_informarl(leaf, ocfg, r, hpd, eng.cost_weight_at(step))
        for k in ("Vl", "Ql"):
            _close(tg[k].cpu().numpy(), wt[k], 1e-5, k)
    else:
        tg = eng.targets_hcbfcrpo(ro, step)
        wt = R.targets_hcbfcrpo(leaf, ocfg, r, hpd, eng.cbf_weight_at(step))
        # Vh := get_cost(graph): the stored costs and the cost of next_graph[-1] (the zero-action VMAS step), bit-exact
        np.testing.assert_array_equal(tg["Vh"].cpu().numpy()[:, :T_], r["costs"])
        np.testing.assert_array_equal(tg["Vh"].cpu().numpy()[:, T_], wt["Vh"][:, T_])
        for k in ("Vl", "Ql", "Qh"):
            _close(tg[k].cpu().numpy(), wt[k], 1e-5, k)
        _check_advantage(tg, wt, cfg.dt, hp.alpha, hp.cbf_eps, eng.cbf_weight_at(step), "VMAS hcbfcrpo")
    # gradients of the FIRST minibatch (before any optimiser step) against autograd on the oracle
    perm = np.random.default_rng(0).permutation(B)
    grads = {}

    def hook(name, net, mb):
        if mb == 0:
            grads[name] = net.to_tree(net.grads)
    eng.grad_hook = hook
    tg_np = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in tg.items()}
    R.minibatch_losses(leaf, ocfg, r, d, tg_np, perm[:bs // T_], hpd, eng.eps_hat.cpu())
    info = eng.update(ro, det, step, perm)
    assert set(grads) == set(names)
    _check_first_minibatch_grads(leaf, grads, names)
    assert all(np.isfinite(v) for v in info.values()), info


def test_train_and_test_cli(cuda, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--env", "VMASReverseTransport", "-n", "3", "--algo", "dgppo",
           "--obs", "0", "--n-env-train", "16", "--steps", "2", "--batch-size", "2048", "--n-env-test", "4",
           "--eval-interval", "1", "--save-interval", "1", "--log-dir", str(tmp_path / "logs")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    run_dir = tmp_path / "logs" / "VMASReverseTransport" / "dgppo"
    run_dir = run_dir / os.listdir(run_dir)[0]
    assert (run_dir / "config.yaml").exists() and os.listdir(run_dir / "models")
    tcmd = [sys.executable, os.path.join(ROOT, "test.py"), "--path", str(run_dir), "--epi", "1", "--max-step", "6",
            "--dpi", "30"]
    tout = subprocess.run(tcmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert tout.returncode == 0, tout.stderr[-3000:]
    assert "epi: 0, reward:" in tout.stdout
    vids = [f for d, _, fs in os.walk(run_dir / "videos") for f in fs]
    assert len(vids) == 1 and vids[0].endswith((".gif", ".mp4")), vids
