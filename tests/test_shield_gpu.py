"""Barrier shield: dgppo_graph_feats_team_action_sweep against dgppo_graph_feats_action_sweep called once per (env, agent),
dgppo_shield_select against the rule restated in NumPy, Engine.rollout_shielded against action_landscape, values_prepass and
ops_env.step, the refusals, and test.py --shield in-process."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import nn_torch as T

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(kind_name, n, n_obs, area=None):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind_name], n, n_obs, **({} if area is None else dict(area_size=area)))


def _same_words(got, want, name):
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, f"{name}: {bad} of {got.numel()} words differ"


# ---- the shield's rule (barrier shield), in NumPy ---------------------------------------------------------------------------------------------------
def _clip(a):
    a = np.asarray(a, f32)
    return np.where(np.isnan(a), a, np.minimum(np.maximum(a, f32(-1)), f32(1))).astype(f32)


def _candidates(a_pol, us, vs):
    """[..., P, 2] clipped candidates: the policy action, then (us[iu], vs[iv]) at 1 + iv * nu + iu"""
    grid = np.stack(np.meshgrid(np.asarray(us, f32), np.asarray(vs, f32)), axis=-1).reshape(-1, 2)
    a_pol = np.asarray(a_pol, f32)
    full = np.concatenate([a_pol[..., None, :], np.broadcast_to(grid, a_pol.shape[:-1] + grid.shape)], axis=-2)
    return _clip(full)


def _rule(h, a_pol, us, vs, margin):
    """the selection rule on barrier values h [..., P] -> index, flag, action: candidate 0 if admissible (h <= -margin), else
    the nearest admissible one (lowest index on ties), else the smallest h (lowest index on ties, NaN skipped, 0 if all NaN)"""
    h = np.asarray(h, f32)
    cand = _candidates(a_pol, us, vs)
    lead, P = h.shape[:-1], h.shape[-1]
    index, flag = np.zeros(lead, np.int32), np.zeros(lead, np.int32)
    thr = f32(-f32(margin))
    for ix in np.ndindex(*lead):
        hh, cc = h[ix], cand[ix]
        adm = hh <= thr                                              # a NaN compares false
        if adm[0]:
            index[ix], flag[ix] = 0, 0
        elif adm.any():
            du, dv = cc[:, 0] - cc[0, 0], cc[:, 1] - cc[0, 1]
            d = (du * du).astype(f32) + (dv * dv).astype(f32)
            d = np.where(np.isnan(d), f32(np.inf), d).astype(f32)
            d = np.where(adm, d, f32(np.inf))
            best = d.min()
            index[ix], flag[ix] = int(np.flatnonzero(adm & (d == best))[0]), 1
        else:
            flag[ix] = 2
            ok = ~np.isnan(hh)
            index[ix] = int(np.flatnonzero(ok & (hh == hh[ok].min()))[0]) if ok.any() else 0
    action = np.take_along_axis(cand, index[..., None, None].astype(np.int64).repeat(2, -1), axis=-2)[..., 0, :]
    return index, flag, action


def _h_formula(Vn_own, Vt, dt, alpha):
    """the barrier value in fp32: Vn_own [..., P, nh] (the agent's own row), Vt [..., nh]; the maximum propagates NaN"""
    Vt = np.asarray(Vt, f32)[..., None, :]
    hc = (np.asarray(Vn_own, f32) - Vt) / f32(dt) + f32(alpha) * Vt
    return hc.astype(f32).max(axis=-1)                                 # np.max propagates NaN


# ---- 1. the feature kernel against the merged one -----------------------------------------------------------------------------------------
FEAT_CASES = [("LidarSpread", 3, 2, None, 2), ("LidarSpread", 3, 0, None, 2), ("MPESpread", 3, 3, None, 2),
              ("MPEConnectSpread", 4, 1, None, 2), ("LidarBicycleTarget", 3, 2, None, 2), ("LidarSpread", 1, 2, None, 2),
              ("LidarSpread", 24, 3, 4.0, 1), ("LidarSpread", 64, 3, 4.0, 1)]
GRIDS = [(1, 1), (8, 8), (16, 8)]                   # P = 2 (the smallest), 65 and 129: one past one and two tiles of 64


def _outs(cfg, G, cuda, Fp):
    n, S, n_other = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1 - cfg.n_agents
    return dict(Xa=torch.full((G * n, Fp), float("nan"), device=cuda), Xo=torch.full((G * n_other, Fp), float("nan"), device=cuda),
                ef=torch.full((G * n, S, 4), float("nan"), device=cuda), em=torch.full((G * n, S), float("nan"), device=cuda))


def _scene(cfg, B, cuda, seed=4242):
    """B envs stepped once with random policy actions; a_pol[0, 0] = (3, -2) lies outside the box and row (0, 0) of the state
    already moves at the velocity limit (bicycle: speed -0.5), so that clip_action and the state clip both fire"""
    from dgppo_amd import ops_env as OE
    n = cfg.n_agents
    st0 = OE.State.empty(cfg, B, cuda)
    OE.reset(cfg, torch.arange(B, dtype=torch.int64, device=cuda) + seed, st0)
    if cfg.state_dim == 5:
        st0.agent[0, 0, 4] = -0.5
    else:
        st0.agent[0, 0, 2], st0.agent[0, 0, 3] = float(cfg.vel_limit), -float(cfg.vel_limit)
    gen = torch.Generator().manual_seed(3)
    a_pol = (torch.rand(B, n, 2, generator=gen) * 2 - 1)
    a_pol[0, 0] = torch.tensor([3.0, -2.0])
    a_pol = a_pol.to(cuda)
    st1 = st0.like()
    OE.step(cfg, st0, a_pol, st1, torch.empty(B, device=cuda), torch.empty(B, n, cfg.n_cost, device=cuda))
    torch.cuda.synchronize()
    return st0, st1, a_pol


@pytest.mark.parametrize("kind,n,n_obs,area,B", FEAT_CASES, ids=["-".join(map(str, c[:3])) for c in FEAT_CASES])
def test_team_sweep_equals_the_action_sweep_per_agent(cuda, kind, n, n_obs, area, B):
    """all four outputs of graph (e, i, p) against dgppo_graph_feats_action_sweep on the two-frame record [state_t[e], next[e]]:
    the same grid for p >= 1, a 1 x 1 grid at a_pol[e, i] for p = 0.  Masks equal; node rows and unmasked edge features bit-equal
    (LidarBicycleTarget within 1e-6, the bound of tests/test_action_landscape_gpu.py for that kind)."""
    from dgppo_amd import ops_nn as K_
    cfg = _cfg(kind, n, n_obs, area)
    sd, k, S = cfg.state_dim, cfg.top_k, cfg.fan_in
    n_other = cfg.num_nodes - 1 - n
    st0, st1, a_pol = _scene(cfg, B, cuda)
    has_hits = cfg.is_lidar and cfg.n_obs > 0
    big = n > 8
    for nu, nv in (GRIDS[:2] if big else GRIDS):
        us = np.linspace(-1.0, 1.0, nu).astype(f32) if nu > 1 else np.array([0.3], f32)
        vs = np.linspace(-1.0, 1.0, nv).astype(f32) if nv > 1 else np.array([-0.7], f32)
        dus, dvs = K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda)
        P = 1 + nu * nv
        for Fp in ((8,) if big else (cfg.node_dim, 8)):
            got = _outs(cfg, B * n * P, cuda, Fp)
            K_.graph_feats_team_action_sweep(cfg, st0.agent, st1.agent, st0.goal, st0.obst, st1.hits, a_pol, dus, dvs, got["Xa"],
                                             got["Xo"] if n_other > 0 else None, got["ef"], got["em"], Fp)
            torch.cuda.synchronize()
            assert not torch.isnan(got["Xa"]).any() and not torch.isnan(got["em"]).any() and not torch.isnan(got["ef"]).any()
            want = {key: torch.empty_like(v) for key, v in got.items()}
            ref_p, ref_0 = _outs(cfg, nu * nv, cuda, Fp), _outs(cfg, 1, cuda, Fp)
            for e in range(B):
                agent = torch.stack([st0.agent[e], st1.agent[e]]).contiguous()
                hits = torch.stack([st0.hits[e], st1.hits[e]]).contiguous() if has_hits else None
                goal = st0.goal[e].contiguous()
                obst = st0.obst[e].contiguous() if cfg.n_obs > 0 else None
                for i in range(n):
                    a0 = a_pol[e, i].contiguous()
                    for ref, u_, v_ in ((ref_p, dus, dvs), (ref_0, a0[0:1].clone(), a0[1:2].clone())):
                        K_.graph_feats_action_sweep(cfg, agent, n * sd, goal, obst, hits, n * k * 2, [0], 1, i, u_, v_, ref["Xa"],
                                                    ref["Xo"] if n_other > 0 else None, ref["ef"], ref["em"], Fp)
                    for key in want:
                        if want[key].numel():
                            w = want[key].view(B, n, P, -1)
                            w[e, i, 1:] = ref_p[key].view(nu * nv, -1)
                            w[e, i, 0] = ref_0[key].view(-1)
            torch.cuda.synchronize()
            tag = f"{kind} n={n} grid {nu}x{nv} Fp={Fp}"
            assert torch.equal(got["em"], want["em"]), f"emask {tag}"
            assert (got["em"] == 0).any() or n == 1
            on = want["em"] > 0
            if cfg.state_dim == 5:
                for name, a, b in (("Xa", got["Xa"], want["Xa"]), ("efeat", got["ef"][on], want["ef"][on])):
                    err = float((a.double() - b.double()).abs().max())
                    print(f"{name} {tag}: max abs err {err:.3e}")
                    assert err <= 1e-6, f"{name} {tag}: {err:.3e}"
            else:
                _same_words(got["Xa"], want["Xa"], f"Xa {tag}")
                _same_words(got["ef"][on], want["ef"][on], f"efeat {tag}")
            if n_other > 0:
                _same_words(got["Xo"], want["Xo"], f"Xo {tag}")
            # both clips fire in graph (0, 0, 0): the action (3, -2) gives the row of (1, -1) and the velocity stays at its limit
            row = got["Xa"].view(B, n, P, n, Fp)[0, 0, 0, 0]
            if cfg.state_dim == 5:
                assert float(row[4]) == -0.5
            else:
                assert float(row[2]) == float(cfg.vel_limit) and float(row[3]) == -float(cfg.vel_limit)
            rows = got["Xa"].view(B, n, P, n, Fp)
            if P > 2:
                assert not torch.equal(rows[0, 0, 1, 0], rows[0, 0, P - 1, 0]), "different candidates give different rows"


# ---- 2. the select kernel against NumPy ---------------------------------------------------------------------------------------------------
def _select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, margin, want_h=True):
    from dgppo_amd import ops_nn as K_
    E, n, P = Vn.shape[:3]
    nh = Vn.shape[-1]
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, f32)).to(cuda)
    action = torch.full((E, n, 2), float("nan"), device=cuda)
    index = torch.full((E, n), -7, dtype=torch.int32, device=cuda)
    flag = torch.full((E, n), -7, dtype=torch.int32, device=cuda)
    h = torch.full((E, n, P), float("nan"), device=cuda) if want_h else None
    K_.shield_select(d(Vn).view(E * n * P * n, nh), d(Vt), d(a_pol), K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda),
                     dt, alpha, margin, action, index, flag, h)
    torch.cuda.synchronize()
    return (action.cpu().numpy(), index.cpu().numpy(), flag.cpu().numpy(), None if h is None else h.cpu().numpy())


def _check_select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, margin, name):
    """h within (2 / dt + alpha) * 1e-5 of the scale of Vh of the fp32 formula (the action landscape's bound: each Vh term of the
    quotient may be off by 1e-5 of scale, alpha * 1e-5 covers the rounding of the evaluation); index, flag and action exactly
    the rule applied to the kernel's own h"""
    E, n = Vn.shape[:2]
    action, index, flag, h = _select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, margin)
    own = Vn[:, np.arange(n), :, np.arange(n)].transpose(1, 0, 2, 3)          # [E, n, P, nh]: the agent's own row
    want_h = _h_formula(own, Vt, dt, alpha)
    np.testing.assert_array_equal(np.isnan(h), np.isnan(want_h), err_msg=f"{name}: NaN positions of h")
    fin = ~np.isnan(want_h)
    scale = max(1.0, float(np.nanmax(np.abs(Vn))), float(np.nanmax(np.abs(Vt))))
    bound = (2.0 / dt + alpha) * 1e-5 * scale
    err = float(np.abs(h[fin].astype(np.float64) - want_h[fin]).max()) if fin.any() else 0.0
    print(f"{name}: h max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: h max abs err {err:.3e} > {bound:.3e}"
    wi, wf, wa = _rule(h, a_pol, us, vs, margin)
    np.testing.assert_array_equal(index, wi, err_msg=f"{name}: index")
    np.testing.assert_array_equal(flag, wf, err_msg=f"{name}: flag")
    np.testing.assert_array_equal(action.view(np.uint32), wa.view(np.uint32), err_msg=f"{name}: action")
    a2, i2, f2, none = _select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, margin, want_h=False)
    assert none is None and np.array_equal(i2, index) and np.array_equal(f2, flag), f"{name}: without the h output"
    return action, index, flag, h


def _craft(hdes, n=2, nh=2, dt=0.03, alpha=10.0, agent=1):
    """Vh_next / Vh_t of ONE env whose agent `agent` has barrier values hdes [P] (component 0 carries them, the others lie 5
    lower; NaN stays NaN); every other entry, the other agents' rows of that agent's graphs included, says +50 (inadmissible)"""
    hdes = np.asarray(hdes, f32)
    P = hdes.size
    Vt = np.full((1, n, nh), 0.5, f32)
    Vn = np.full((1, n, P, n, nh), 50.0, f32)
    for c in range(nh):
        Vn[0, agent, :, agent, c] = f32(0.5) + f32(dt) * ((hdes - f32(5.0 * c)) - f32(alpha) * f32(0.5))
    return Vn, Vt


def test_select_hand_made_cases(cuda):
    dt, alpha = 0.03, 10.0
    us, vs = np.array([-0.5, 0.5], f32), np.array([0.0], f32)                  # P = 3: candidates 1 and 2 at distance 0.5 of (0, 0)
    a_pol = np.zeros((1, 2, 2), f32)
    nan = np.nan

    def run(hdes, margin=0.0, name="", a=a_pol, us_=us, vs_=vs, nh=2):
        Vn, Vt = _craft(hdes, nh=nh)
        action, index, flag, h = _check_select(cuda, Vn, Vt, a, us_, vs_, dt, alpha, margin, name)
        assert flag[0, 0] == 2, "the other agent sees +50 everywhere"
        return int(index[0, 1]), int(flag[0, 1]), action[0, 1]

    assert run([-1.0, -3.0, -3.0], name="kept")[:2] == (0, 0)
    i, f, a = run([1.0, -1.0, -1.0], name="nearest admissible, exact distance tie")
    assert (i, f) == (1, 1) and a.tolist() == [-0.5, 0.0]
    b = np.array([[[0.0, 0.0], [0.2, 0.0]]], f32)
    i, f, a = run([1.0, -1.0, -1.0], name="nearest admissible", a=b)
    assert (i, f) == (2, 1) and a.tolist() == [0.5, 0.0]
    assert run([1.0, -1.0, 2.0], name="the only admissible one", a=b)[:2] == (1, 1)
    assert run([3.0, 2.0, 2.0], name="nothing admissible, h tie")[:2] == (1, 2)
    assert run([3.0, 4.0, 2.0], name="nothing admissible")[:2] == (2, 2)
    assert run([1.0, -1.0, nan], name="one NaN candidate", a=b)[:2] == (1, 1)
    assert run([nan, 2.0, 1.0], name="NaN policy candidate, nothing admissible")[:2] == (2, 2)
    assert run([nan, nan, nan], name="all NaN")[:2] == (0, 2)
    assert run([-0.1, -1.0, -1.0], margin=0.0, name="margin 0")[:2] == (0, 0)
    assert run([-0.1, -1.0, -1.0], margin=0.5, name="margin 0.5 flips the decision")[:2] == (1, 1)
    assert run([-0.1, -0.2, -0.3], margin=0.5, name="margin 0.5, nothing admissible")[:2] == (2, 2)
    assert run([-1.0, -3.0, -3.0], name="kept, nh = 3", nh=3)[:2] == (0, 0)
    # the NaN sits in the second component only: the maximum propagates it
    Vn, Vt = _craft([1.0, -1.0, -1.0])
    Vn[0, 1, 1, 1, 1] = nan
    action, index, flag, h = _check_select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, 0.0, "NaN in component 1")
    assert np.isnan(h[0, 1, 1]) and (int(index[0, 1]), int(flag[0, 1])) == (2, 1)
    # a policy action outside the box: the distance is taken from its clipped value (1, 0), and so is the kept action
    c = np.array([[[0.0, 0.0], [7.0, 0.0]]], f32)
    i, f, a = run([-1.0, -3.0, -3.0], name="kept outside the box", a=c)
    assert (i, f) == (0, 0) and a.tolist() == [1.0, 0.0]
    assert run([1.0, -1.0, -1.0], name="replaced outside the box", a=c)[:2] == (2, 1)


@pytest.mark.parametrize("E,n,nh,nu,nv", [(3, 1, 2, 1, 1), (2, 64, 3, 8, 8), (2, 3, 2, 64, 64), (3, 3, 3, 8, 8), (5, 7, 2, 3, 2)],
                         ids=["n1-P2", "n64-nh3-P65", "n3-P4097", "n3-nh3-P65", "n7-P7"])
def test_select_random(cuda, E, n, nh, nu, nv):
    """random values around the threshold: every flag occurs; a sprinkle of NaN; the last env has nothing finite"""
    dt, alpha = 0.03, 10.0
    rng = np.random.default_rng(E * 1000 + n * 10 + nh)
    P = 1 + nu * nv
    us = np.linspace(-1.0, 1.0, nu).astype(f32) if nu > 1 else np.array([0.25], f32)
    vs = np.linspace(-1.0, 1.0, nv).astype(f32) if nv > 1 else np.array([-0.5], f32)
    Vt = rng.uniform(-1.0, 0.2, size=(E, n, nh)).astype(f32)
    # Vh_next - Vh_t of the order dt * alpha * |Vh_t|: h changes sign from candidate to candidate; agent-dependent shift so that
    # some agents admit everything and some nothing
    shift = rng.uniform(-0.3, 0.3, size=(E, n, 1, 1, 1)).astype(f32)
    Vn = (Vt[:, :, None, None, :] + shift + rng.uniform(-0.3, 0.3, size=(E, n, P, n, nh))).astype(f32)
    Vn[rng.uniform(size=Vn.shape) < 0.02] = np.nan
    Vn[E - 1, 0] = np.nan
    a_pol = rng.uniform(-1.3, 1.3, size=(E, n, 2)).astype(f32)
    for margin in (0.0, 2.0):
        action, index, flag, h = _check_select(cuda, Vn, Vt, a_pol, us, vs, dt, alpha, margin, f"random margin {margin}")
        assert flag[E - 1, 0] == 2 and index[E - 1, 0] == 0
    if E * n >= 9:
        assert set(np.unique(flag)) == {0, 1, 2}


# ---- 3. the engine ------------------------------------------------------------------------------------------------------------------------------
def _engine(n, n_obs, T_, cuda, use_rnn=True, rnn_layers=1, area=None, algo="dgppo"):
    from dgppo_amd import engine as EN, init
    cfg = _cfg("LidarSpread", n, n_obs, area)
    nc = rnn_layers if use_rnn else 0
    hp = EN.Hyper(batch_size=1024, rnn_step=2, train_steps=100, use_rnn=use_rnn, rnn_layers=rnn_layers, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo=algo)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=min(nc, 1))}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    for k_, net in eng.nets.items():
        net.load_tree(jitter(trees[k_]))
    eng.set_entropy_noise(77)
    return cfg, eng


def _close(got, want, tol, name):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})"


def _record_words(ro):
    """every word of a time-major record"""
    out = {f"step.{k}": v for k, v in ro.step_tm.items()}
    out.update(action=ro.action_tm, rnn=ro.rnn_tm, reward=ro.reward_tm, cost=ro.cost_tm)
    return out


ENGINE_CASES = [("n3", 3, 2, None, True, 1, 2, 3), ("n3-no-rnn", 3, 2, None, False, 1, 2, 3), ("n3-rnn-layers-2", 3, 2, None, True, 2, 2, 3),
                ("n24-tiled-attention", 24, 3, 4.0, True, 1, 1, 2)]


@pytest.mark.parametrize("name,n,n_obs,area,use_rnn,rnn_layers,B,grid", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_rollout_shielded(cuda, name, n, n_obs, area, use_rnn, rnn_layers, B, grid):
    """T = 4.  Step 0 sees the state of rollout(seeds, False): policy_action[0] is that record's action bit for bit, h[0, e, i, 1:]
    is action_landscape's h() within (2 / dt + alpha) * 1e-5 of scale and Vh[0] its Vh within 1e-5 (the bounds of
    tests/test_action_landscape_gpu.py).  Every step: values_prepass of the finished record gives log.Vh within 1e-5 of scale (the
    stored states and carries are the ones the shield used), states[t + 1] is ops_env.step(states[t], action[t]) bit for bit,
    action / index / flag are the NumPy rule on log.h.  A Vh output bias of -1000 admits everything: the record equals
    rollout(seeds, False) in every word; +1000 admits nothing: flag 2 and index = argmin h.  Blocks of one env are bit-equal."""
    from dgppo_amd import ops_env as OE
    T_ = 4
    cfg, eng = _engine(n, n_obs, T_, cuda, use_rnn, rnn_layers, area)
    nh, dt, alpha = cfg.n_cost, float(cfg.dt), float(eng.hp.alpha)
    seeds = torch.tensor([9, 10][:B], dtype=torch.int64, device=cuda)
    us = vs = np.linspace(-1.0, 1.0, grid).astype(f32)
    P = 1 + grid * grid
    ro_u = eng.rollout(seeds, False)
    ro, log = eng.rollout_shielded(seeds, us, vs)
    torch.cuda.synchronize()
    assert tuple(log["policy_action"].shape) == (T_, B, n, 2) and tuple(log["h"].shape) == (T_, B, n, P)
    assert tuple(log["index"].shape) == tuple(log["flag"].shape) == (T_, B, n) and tuple(log["Vh"].shape) == (T_, B, n, nh)
    assert log["index"].dtype == log["flag"].dtype == torch.int32 and not ro.stochastic and ro.log_pi_tm is None
    h_all = log["h"].cpu().numpy()
    assert np.isfinite(h_all).all()

    # ---- step 0 against action_landscape on the unshielded record ----
    _same_words(log["policy_action"][0], ro_u.action_tm[0], f"{name}: policy_action[0] vs rollout(seeds, False)")
    ro_u.finalize()
    for e, i in sorted({(0, 0), (B - 1, n - 1)}):
        cbf, Vn, Vh = eng.action_landscape(ro_u, e, i, [0], us, vs)
        want_h = cbf[0, :, :, i, :].max(dim=-1).values.reshape(-1)
        scale = max(1.0, float(Vn.abs().max()), float(Vh.abs().max()))
        bound = (2.0 / dt + alpha) * 1e-5 * scale
        err = float((log["h"][0, e, i, 1:].double() - want_h.double()).abs().max())
        print(f"{name}: h[0, {e}, {i}, 1:] vs action_landscape: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        _close(log["Vh"][0, e], Vh[0], 1e-5, f"{name}: Vh[0, {e}] vs action_landscape")

    # ---- every step ----
    ro.finalize()
    Vh_pre = eng.values_prepass(ro, want_Vl=False)[1]
    _close(log["Vh"].transpose(0, 1), Vh_pre[:, :T_], 1e-5, f"{name}: log.Vh vs values_prepass of the finished record")
    pol = log["policy_action"].cpu().numpy()
    for t in range(T_):
        nst = ro.states_tm[t].like()
        OE.step(cfg, ro.states_tm[t], ro.action_tm[t], nst, torch.empty(B, device=cuda), torch.empty(B, n, nh, device=cuda))
        for key, v in nst.step.items():
            _same_words(v, ro.states_tm[t + 1].step[key], f"{name}: {key}[{t + 1}] vs ops_env.step(states[{t}], action[{t}])")
        wi, wf, wa = _rule(h_all[t], pol[t], us, vs, 0.0)
        np.testing.assert_array_equal(log["index"][t].cpu().numpy(), wi, err_msg=f"{name}: index[{t}]")
        np.testing.assert_array_equal(log["flag"][t].cpu().numpy(), wf, err_msg=f"{name}: flag[{t}]")
        np.testing.assert_array_equal(ro.action_tm[t].cpu().numpy().view(np.uint32), wa.view(np.uint32),
                                      err_msg=f"{name}: action[{t}] is the candidate index[{t}] names")

    # ---- everything admissible / nothing admissible ----
    mine = {k: v.clone() for k, v in _record_words(ro).items()}
    bias = eng.Vh.p("head.bo")
    keep = bias.clone()
    try:
        bias.fill_(-1000.0)
        ro_a, log_a = eng.rollout_shielded(seeds, us, vs)
        assert int(log_a["flag"].abs().sum()) == 0 and int(log_a["index"].abs().sum()) == 0
        ro_u2 = eng.rollout(seeds, False)
        for (key, a), b in zip(_record_words(ro_a).items(), _record_words(ro_u2).values()):
            _same_words(a, b, f"{name}: everything admissible: {key} vs rollout(seeds, False)")
        bias.fill_(1000.0)
        ro_n, log_n = eng.rollout_shielded(seeds, us, vs)
        assert bool((log_n["flag"] == 2).all())
        hn = log_n["h"].cpu().numpy()
        assert np.isfinite(hn).all()
        np.testing.assert_array_equal(log_n["index"].cpu().numpy(), hn.argmin(axis=-1))
    finally:
        bias.copy_(keep)

    # ---- several blocks of environments ----
    if B > 1:
        cap = eng.prepass_graphs
        try:
            eng.prepass_graphs = n * P                                   # one env per block
            ro_b, log_b = eng.rollout_shielded(seeds, us, vs)
            eng.prepass_graphs = 1                                       # less than one env: still one env per block
            ro_c, log_c = eng.rollout_shielded(seeds, us, vs)
        finally:
            eng.prepass_graphs = cap
        for other_ro, other_log, what in ((ro_b, log_b, "blocks of one env"), (ro_c, log_c, "prepass_graphs = 1")):
            for key, b in _record_words(other_ro).items():
                _same_words(b, mine[key], f"{name}: {what}: {key}")
            for key in log:
                _same_words(other_log[key], log[key], f"{name}: {what}: log.{key}")


def test_engine_margin_moves_the_threshold(cuda):
    """with a margin above every h nothing is admissible; with one below every h everything is"""
    cfg, eng = _engine(3, 2, 4, cuda)
    seeds = torch.tensor([9, 10], dtype=torch.int64, device=cuda)
    us = vs = np.linspace(-1.0, 1.0, 3).astype(f32)
    _, log = eng.rollout_shielded(seeds, us, vs)
    top = float(log["h"].abs().max())
    _, hi = eng.rollout_shielded(seeds, us, vs, margin=2.0 * top + 1.0)
    assert bool((hi["flag"] == 2).all())
    _, lo = eng.rollout_shielded(seeds, us, vs, margin=-(2.0 * top + 1.0))
    assert bool((lo["flag"] == 0).all())


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["informarl", "hcbfcrpo", "informarl_lagr"])
def test_unsupported_algorithms_raise(cuda, algo):
    from dgppo_amd import _native as N, engine as EN
    eng = EN.Engine(N.make_env_cfg(0, 3, 2), EN.Hyper(batch_size=256), cuda, T=4, algo=algo)
    with pytest.raises(ValueError, match=f"rollout_shielded.*{algo}"):
        eng.rollout_shielded(torch.tensor([1], dtype=torch.int64, device=cuda), [0.5], [0.5])


def test_engine_refusals(cuda):
    from dgppo_amd import _native as N, engine as EN
    seeds = torch.tensor([1], dtype=torch.int64, device=cuda)
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="rollout_shielded.*VMASReverseTransport"):
        vmas.rollout_shielded(seeds, [0.5], [0.5])
    cfg, eng = _engine(3, 2, 4, cuda)
    for kw, match in ((dict(us=[]), "us"), (dict(vs=[0.5, float("inf")]), "vs"), (dict(us=[float("nan")]), "us"),
                      (dict(margin=float("nan")), "margin")):
        args = dict(us=[0.5], vs=[0.5])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            eng.rollout_shielded(seeds, **args)


def test_bindings_refuse_before_any_launch(cuda):
    from dgppo_amd import _native as N, ops_nn as K_
    cfg = _cfg("LidarSpread", 3, 2)
    st0, st1, a_pol = _scene(cfg, 2, cuda)
    us, vs = K_.sweep_axis([0.2, 0.4], "us", cuda), K_.sweep_axis([0.3], "vs", cuda)
    out = _outs(cfg, 2 * 3 * 3, cuda, 8)

    def call(cfg=cfg, us=us, vs=vs, hits=st1.hits, a=a_pol, Xa=out["Xa"]):
        K_.graph_feats_team_action_sweep(cfg, st0.agent, st1.agent, st0.goal, st0.obst, hits, a, us, vs, Xa, out["Xo"], out["ef"],
                                         out["em"], 8)
    with pytest.raises(ValueError, match="next_hits"):
        call(hits=None)
    with pytest.raises(ValueError, match="empty"):
        call(vs=torch.empty(0, device=cuda))
    with pytest.raises(ValueError, match="a_pol"):
        call(a=a_pol[:1])
    with pytest.raises(ValueError, match="Xa"):
        call(Xa=out["Xa"][:-1])
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        call(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0))
    sel = dict(Vh_next=torch.zeros(2 * 3 * 3 * 3, 2, device=cuda), Vh_t=torch.zeros(2, 3, 2, device=cuda), a_pol=a_pol, us=us, vs=vs,
               dt=0.03, alpha=10.0, margin=0.0, action=torch.full((2, 3, 2), float("nan"), device=cuda),
               index=torch.zeros(2, 3, dtype=torch.int32, device=cuda), flag=torch.zeros(2, 3, dtype=torch.int32, device=cuda))
    for kw, match in ((dict(Vh_next=sel["Vh_next"][:-1]), "Vh_next"), (dict(index=sel["index"].long()), "index"), (dict(dt=0.0), "dt"),
                      (dict(margin=float("nan")), "margin"), (dict(h=torch.zeros(2, 3, 2, device=cuda)), "h")):
        with pytest.raises(ValueError, match=match):
            K_.shield_select(**{**sel, **kw})
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in out.values()) and bool(torch.isnan(sel["action"]).all()), \
        "a refused call wrote to its outputs"
    call()
    K_.shield_select(**sel)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o).any()) for o in out.values()) and not bool(torch.isnan(sel["action"]).any())


# ---- 5. test.py --shield, in-process --------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_dir(tmp_path, algo_name, n, Tn, iterations, alpha):
    """a run directory as train.py leaves it after `iterations` collect / update rounds: config.yaml and models/{step}"""
    import yaml
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    conf = dict(env="LidarSpread", num_agents=n, obs=2, algo=algo_name, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, seed=3, use_rnn=True, rnn_layers=1, use_lstm=False, alpha=alpha)
    env = make_env(env_id=conf["env"], num_agents=n, num_obs=conf["obs"], max_step=Tn)
    algo = make_algo(algo=algo_name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=n, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                     Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, max_grad_norm=2.0, seed=3, use_rnn=True, rnn_layers=1,
                     use_lstm=False, alpha=alpha, batch_size=4 * Tn, rnn_step=Tn, train_steps=max(iterations, 1))
    for it in range(iterations):
        ro = algo.collect(None, np.arange(8, dtype=np.int64) + 100 * it + 1)
        info = algo.update(ro, it)
        assert all(np.isfinite(v) for v in info.values()), info
    run = tmp_path / f"run_{algo_name}"
    algo.save(str(run / "models"), iterations)
    with open(run / "config.yaml", "w") as f:
        yaml.safe_dump(conf, f)
    return run


def test_cli_writes_the_shield_log(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import ShieldLog
    n, grid, Tn, alpha = 3, 3, 6, 5.0
    run = _run_dir(tmp_path, "dgppo", n, Tn, 2, alpha)
    mod = _load_test_py()
    common = ["--path", str(run), "--epi", "2", "--no-video", "--max-step", str(Tn)]
    with pytest.raises(SystemExit, match="--shield --stochastic"):
        mod.main(common + ["--shield", "--stochastic"])
    capsys.readouterr()
    mod.main(common + ["--shield", "--shield-grid", str(grid), "--shield-margin", "0.5"])
    printed = capsys.readouterr().out
    for word in ("intervention_frac", "infeasible_frac", "mean_deviation"):
        assert printed.count(word) == 2, word
    assert printed.count("safe rate") == 2
    vdir = run / "videos" / "2"
    files = sorted(glob.glob(str(vdir / "*_shield.npz")))
    assert len(files) == 2 and len(glob.glob(str(vdir / "*"))) == 2
    lin = np.linspace(-1.0, 1.0, grid).astype(f32)
    P = 1 + grid * grid
    stats = ("intervention_frac", "infeasible_frac", "mean_deviation")
    for path in files:
        z = np.load(path)
        assert sorted(z.files) == sorted([*ShieldLog._fields, *stats])
        np.testing.assert_array_equal(z["us"], lin)
        np.testing.assert_array_equal(z["vs"], lin)
        assert z["policy_action"].shape == z["action"].shape == (Tn, n, 2) and z["h"].shape == (Tn, n, P)
        assert z["index"].shape == z["flag"].shape == (Tn, n) and z["Vh"].shape == (Tn, n, 2)
        assert float(z["margin"]) == 0.5 and float(z["alpha"]) == alpha and float(z["dt"]) == f32(0.03)
        wi, wf, wa = _rule(z["h"], z["policy_action"], lin, lin, 0.5)
        np.testing.assert_array_equal(z["index"], wi)
        np.testing.assert_array_equal(z["flag"], wf)
        np.testing.assert_array_equal(z["action"], wa)
        one = ShieldLog(*(z[k][None] if k in ("policy_action", "action", "index", "flag", "h", "Vh") else z[k] for k in ShieldLog._fields))
        for key, v in EV.shield_stats(one).items():
            np.testing.assert_array_equal(z[key], v[0])
    # the landscapes work on the shielded record unchanged
    mod.main(common + ["--shield", "--shield-grid", str(grid), "--action-landscape", "0", "--landscape-grid", "4"])
    assert len(glob.glob(str(vdir / "*_action.npz"))) == 2


def test_cli_refuses_an_algorithm_without_a_vh_net(cuda, tmp_path):
    run = _run_dir(tmp_path, "informarl", 3, 6, 0, 10.0)
    with pytest.raises(ValueError, match="informarl"):
        _load_test_py().main(["--path", str(run), "--epi", "2", "--no-video", "--max-step", "6", "--shield"])
