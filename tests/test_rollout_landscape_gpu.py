"""Rollout landscape on the GPU: dgppo_env_sweep_fork bit for bit against NumPy (the moved agent's hits: the oracle's
lidar_sense at the moved position, and the hits_out of dgppo_graph_feats_sweep for the same call), dgppo_constraint_return bit
for bit against the restatement of tests/test_rollout_landscape_cpu.py, every sub-grid record of Engine.rollout_landscape
re-derived step by step by the oracle policy and the oracle env (the bars of tests/test_engine_gpu.py: 1e-5 for actions and
carries, exact env outputs), the cross-check with Engine.cost_landscape, and the public interface down to test.py."""
import functools
import glob
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_act_step_gpu import INSTANCES  # noqa: E402
from test_cost_landscape_gpu import _checkpoint, _load_test_py, _to  # noqa: E402
from test_engine_gpu import _np_rollout, _setup  # noqa: E402
from test_rollout_landscape_cpu import fold_np  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
SENTINEL = 12345.0


def _same(got, want, name):
    """equal bits wherever `want` is no NaN, NaN exactly where it is one"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaN positions")
    bad = np.where(nan, f32(0), got).view(np.uint32) != np.where(nan, f32(0), want).view(np.uint32)
    where = np.argwhere(bad)[:4].tolist()
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {where}: got "
                           f"{[float(got[tuple(i)]) for i in where]}, want {[float(want[tuple(i)]) for i in where]}")


# ---- 1. the fork against NumPy, bit for bit -----------------------------------------------------------------------------------------
RECT = (f32(1.0), f32(1.2))          # centre of rectangle 0: a grid point inside it
HOME = {0: (f32(0.3), f32(1.2)), -1: (f32(0.55), f32(1.2))}      # where agents 0 and n - 1 stand in frame 5
FRAMES = [5, 0, 2]                   # out of order
# (kind, n, n_obs): the second and third have nothing to cast (no obst at all / disc records), the fourth has SD = 5, the rows of
# the last are wider than a wave (n * sd = 80, n * k * 2 = 320)
FORK_CASES = [("LidarSpread", 3, 2), ("MPETarget", 3, 0), ("MPESpread", 3, 3), ("LidarBicycleTarget", 2, 1), ("LidarSpread", 20, 4)]


@functools.lru_cache(maxsize=None)
def _record(kind_name, n, n_obs, n_rays=32, top_k=8):
    """a 6-frame record of one env built by hand (read-only): agents drawn from a fixed seed, drifting from frame to frame, agents
    0 and n - 1 at HOME in frame 5; rectangle 0 centred at RECT; goals; a carry of 128 columns per agent and frame"""
    from dgppo_amd import _native as N
    kind = N.ENV_KINDS[kind_name]
    kw = dict(n_rays=n_rays, top_k=top_k) if kind_name.startswith("Lidar") else {}
    cfg, ocfg = N.make_env_cfg(kind, n, n_obs, **kw), E.EnvCfg(kind, n_agents=n, n_obs=n_obs, **kw)
    assert (cfg.n_obs, cfg.n_goals, cfg.state_dim, cfg.num_nodes) == (ocfg.n_obs, ocfg.n_goals, ocfg.state_dim, ocfg.num_nodes)
    sd, Tn, A = ocfg.state_dim, 6, float(ocfg.area_size)
    rng = np.random.default_rng(100 * n + n_obs)
    base = rng.uniform(0.05, A - 0.05, size=(n, 2))
    agent = np.zeros((Tn, n, sd), f32)
    for t in range(Tn):
        agent[t, :, :2] = (base + 0.01 * t).astype(f32)
    agent[5, 0, :2], agent[5, n - 1, :2] = HOME[0], HOME[-1]
    if ocfg.is_bicycle:
        th = rng.uniform(-np.pi, np.pi, size=(Tn, n))
        agent[..., 2], agent[..., 3] = np.cos(th).astype(f32), np.sin(th).astype(f32)
        agent[..., 4] = rng.uniform(-0.5, 0.5, size=(Tn, n)).astype(f32)
    else:
        agent[..., 2:4] = rng.uniform(-0.5, 0.5, size=(Tn, n, 2)).astype(f32)
    goal = np.zeros((ocfg.n_goals, sd), f32)
    goal[:, :2] = rng.uniform(0.0, A, size=(ocfg.n_goals, 2)).astype(f32)
    obst = hits = None
    centres = np.array([RECT, (0.45, 0.5), (0.8, 0.3), (0.3, 0.9)][:n_obs], f32)
    if n_obs > 0 and ocfg.is_lidar:
        obst = E.make_rect(centres, np.array([0.3, 0.2, 0.1, 0.15][:n_obs], f32), np.array([0.2, 0.2, 0.3, 0.1][:n_obs], f32),
                           np.array([0.3, 0.0, 1.1, 2.0][:n_obs], f32))
        hits = E.lidar_sense(ocfg, agent[..., :2], np.broadcast_to(obst, (Tn,) + obst.shape), *E.ray_table(ocfg.n_rays))[0]
    elif n_obs > 0:
        obst = np.zeros((n_obs, sd), f32)
        obst[:, :2] = centres
    carry = rng.standard_normal((Tn, n, 128)).astype(f32)
    for a in (agent, goal, obst, hits, carry):
        if a is not None:
            a.setflags(write=False)
    return cfg, ocfg, agent, goal, obst, hits, carry


def _grids(A, home):
    """5 x 3 and 10 x 7 (more than one tile of 64 points and no multiple of it): both hold RECT (inside rectangle 0), the moved
    agent's recorded position of frame 5 and the four corners of the area"""
    small = (np.array([0.0, home[0], RECT[0], 0.7, A], f32), np.array([0.0, home[1], A], f32))
    big = (np.concatenate([small[0][:3], np.linspace(0.1, A - 0.1, 6), [A]]).astype(f32),
           np.concatenate([small[1][:2], np.linspace(0.2, A - 0.2, 4), [A]]).astype(f32))
    assert big[0].size * big[1].size == 70
    return [small, big]


def _moved(agent, frame_ids, aid, xs, ys):
    F, ny, nx, n = len(frame_ids), len(ys), len(xs), agent.shape[1]
    ag = np.repeat(agent[frame_ids], ny * nx, axis=0).reshape(F, ny, nx, n, -1).copy()
    ag[:, :, :, aid, 0] = xs[None, None, :]
    ag[:, :, :, aid, 1] = ys[None, :, None]
    return ag.reshape(F * ny * nx, n, -1)


@pytest.mark.parametrize("kind,n,n_obs", FORK_CASES, ids=["-".join(map(str, c)) for c in FORK_CASES])
def test_fork_matches_numpy(cuda, kind, n, n_obs):
    from dgppo_amd import nets, ops_env as OE, ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits, carry = _record(kind, n, n_obs)
    sd, k, A, F = ocfg.state_dim, ocfg.top_k, float(ocfg.area_size), len(FRAMES)
    cast = hits is not None
    step = dict(agent=_to(agent, cuda), hits=_to(hits, cuda))
    env = dict(goal=_to(goal, cuda), obst=_to(obst, cuda))
    tab = E.ray_table(ocfg.n_rays) if cast else None
    for aid in sorted({0, n - 1}):
        home = HOME[0 if aid == 0 else -1]
        for gi, (xs, ys) in enumerate(_grids(A, home)):
            nx, ny = len(xs), len(ys)
            G = F * ny * nx
            # ---- what NumPy says ----
            ag = _moved(agent, FRAMES, aid, xs, ys)
            tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (G,) + a.shape))
            rep = lambda a: np.repeat(a[FRAMES], ny * nx, axis=0)
            g_home = (0 * ny + 1) * nx + 1                          # frame 5 at (home x, home y)
            _same(ag[g_home], agent[5], "the grid point of the recorded position gives the recorded frame")
            want_hits = None
            if cast:
                sensed = E.lidar_sense(ocfg, ag[..., :2], tile(obst), *tab)[0]
                want_hits = rep(hits).copy()
                want_hits[:, aid] = sensed[:, aid]
                others = [i for i in range(n) if i != aid]
                _same(sensed[:, others], want_hits[:, others], "lidar_sense is a pure function of the position")
                _same(want_hits[g_home], hits[5], "the recorded position gives the recorded hits")
                inside = (0 * ny + 1) * nx + 2                      # (RECT x, RECT y): every ray starts inside rectangle 0
                assert (want_hits[inside, aid] == np.array(RECT, f32)).all(), "start inside: all hit points are the position"
            # ---- the device ----
            xs_d, ys_d = K_.sweep_axis(xs, "xs", cuda), K_.sweep_axis(ys, "ys", cuda)
            for HC in ((64, 128) if gi == 0 else (64,)):
                out = OE.State.empty(cfg, G, cuda)
                for v in (*out.step.values(), *out.env.values()):
                    v.fill_(SENTINEL)
                assert ("hits" in out.step) == cast and ("obst" in out.env) == (n_obs > 0)
                cd = _to(np.ascontiguousarray(carry[..., :HC]), cuda)
                c_out = torch.full((G * n, HC), SENTINEL, device=cuda)
                OE.sweep_fork(cfg, step, env, FRAMES, F, aid, xs_d, ys_d, out, cd, n * HC, c_out)
                torch.cuda.synchronize()
                label = f"agent {aid}, grid {nx}x{ny}, HC {HC}"
                _same(out.agent, ag, f"agent_out, {label}")
                _same(out.goal, tile(goal), f"goal_out, {label}")
                if n_obs > 0:
                    _same(out.obst, tile(obst), f"obst_out, {label}")
                if cast:
                    _same(out.hits, want_hits, f"hits_out, {label}")
                _same(c_out.view(G, n, HC), rep(carry[..., :HC]), f"carry_out, {label}")
            # no carry: the same state, carry_out untouched
            out2 = OE.State.empty(cfg, G, cuda)
            OE.sweep_fork(cfg, step, env, FRAMES, F, aid, xs_d, ys_d, out2)
            if cast:
                # the sweep's own hits_out for the same call
                feats = nets.GraphFeats(cfg, G, nets.Arena(cuda), "t")
                ho = torch.full((G, k, 2), SENTINEL, device=cuda)
                rc, rs = OE._rays(cfg, cuda)
                feats.compute_sweep(step, env, FRAMES, F, aid, xs_d, ys_d, rc, rs, hits_out=ho)
                torch.cuda.synchronize()
                assert torch.equal(out.hits[:, aid].contiguous().view(torch.int32), ho.view(torch.int32)), "fork vs sweep hits_out"
            torch.cuda.synchronize()
            for key in out.step:
                assert torch.equal(out2.step[key].view(torch.int32), out.step[key].view(torch.int32)), key


def test_fork_keeps_nan_rays(cuda):
    """8 rays, all 8 kept: the rays parallel to the axis-aligned rectangle's edges are NaN (det == 0) and stay NaN in the moved
    agent's row, in the oracle's slots"""
    from dgppo_amd import ops_env as OE, ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits, carry = _record("LidarSpread", 3, 2, 8, 8)
    xs, ys = _grids(float(ocfg.area_size), HOME[-1])[0]
    G = len(FRAMES) * len(ys) * len(xs)
    ag = _moved(agent, FRAMES, 2, xs, ys)
    want = E.lidar_sense(ocfg, ag[..., :2], np.ascontiguousarray(np.broadcast_to(obst, (G,) + obst.shape)), *E.ray_table(8))[0]
    assert np.isnan(want[:, 2]).any() and np.isfinite(want[:, 2]).any()
    out = OE.State.empty(cfg, G, cuda)
    OE.sweep_fork(cfg, dict(agent=_to(agent, cuda), hits=_to(hits, cuda)), dict(goal=_to(goal, cuda), obst=_to(obst, cuda)),
                  FRAMES, len(FRAMES), 2, K_.sweep_axis(xs, "xs", cuda), K_.sweep_axis(ys, "ys", cuda), out)
    torch.cuda.synchronize()
    _same(out.hits, want, "hits_out")


def test_fork_bindings_refuse_before_any_launch(cuda):
    from dgppo_amd import _native as N, ops_env as OE, ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits, carry = _record("LidarSpread", 3, 2)
    step = dict(agent=_to(agent, cuda), hits=_to(hits, cuda))
    env = dict(goal=_to(goal, cuda), obst=_to(obst, cuda))
    xs, ys = K_.sweep_axis([0.2, 0.4], "xs", cuda), K_.sweep_axis([0.3], "ys", cuda)
    out = OE.State.empty(cfg, 2, cuda)
    for v in (*out.step.values(), *out.env.values()):
        v.fill_(SENTINEL)
    cd, c_out = _to(np.ascontiguousarray(carry[..., :64]), cuda), torch.full((6, 64), SENTINEL, device=cuda)
    with pytest.raises(ValueError, match="agent_id"):
        OE.sweep_fork(cfg, step, env, [1], 1, 3, xs, ys, out)
    with pytest.raises(ValueError, match="out.agent"):
        OE.sweep_fork(cfg, step, env, [1], 1, 0, xs, ys, OE.State.empty(cfg, 3, cuda))
    with pytest.raises(ValueError, match="carry_out"):
        OE.sweep_fork(cfg, step, env, [1], 1, 0, xs, ys, out, cd, 3 * 64, None)
    with pytest.raises(ValueError, match="carry_out"):
        OE.sweep_fork(cfg, step, env, [1], 1, 0, xs, ys, out, cd, 3 * 64, c_out[:5])
    with pytest.raises(ValueError, match="storage"):
        OE.sweep_fork(cfg, step, env, [6], 1, 0, xs, ys, out)                       # the record holds frames 0 .. 5
    with pytest.raises(ValueError, match="hits"):
        OE.sweep_fork(cfg, dict(agent=step["agent"]), env, [1], 1, 0, xs, ys, out)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.sweep_fork(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), step, env, [1], 1, 0, xs, ys, out)
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in (*out.step.values(), *out.env.values(), c_out)), "a refused call wrote"


# ---- 2. the fold against the restatement, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 33])
def test_fold_matches_restatement(cuda, K, nh):
    """35 rows (less than a wave) and 335 (a second block, neither a multiple of 64), costs with NaN and +-inf, dense steps and
    steps that are slices of a wider allocation"""
    from dgppo_amd import ops_algo as OA
    for G, n in ((7, 5), (67, 5)):
        rng = np.random.default_rng(1000 * K + 10 * nh + G)
        h = rng.uniform(-1.0, 1.0, size=(K, G, n, nh)).astype(f32)
        # NaN, +inf and -inf in m words each, whatever K is: a NaN takes its whole (env, agent) row with it, so at most 3 m of
        # the G * n rows (three in eight) are touched and the others stay finite
        m = max(3, G * n // 8)
        special = rng.choice(h.size, size=3 * m, replace=False)
        for idx, v in zip(np.split(special, 3), (np.nan, np.inf, -np.inf)):
            h.reshape(-1)[idx] = v
        assert np.isnan(h).sum() == m and np.isposinf(h).sum() == m and np.isneginf(h).sum() == m
        for gamma in (0.99, 0.5):
            want_v, want_w = fold_np(h, gamma)
            assert np.isfinite(want_v).any() and np.isnan(want_v).sum() >= np.isnan(h[-1]).sum()
            wide = torch.full((K, G + 1, n, nh), float("nan"), device=cuda)
            wide[:, :G].copy_(_to(h, cuda))
            for cost in (_to(h, cuda), wide[:, :G]):
                v = torch.full((G, n, nh), SENTINEL, device=cuda)
                w = torch.full((G, n, nh), SENTINEL, device=cuda)
                OA.constraint_return(cost, gamma, v, w)
                torch.cuda.synchronize()
                _same(v, want_v, f"value, K {K}, nh {nh}, G {G}, gamma {gamma}")
                _same(w, want_w, f"worst, K {K}, nh {nh}, G {G}, gamma {gamma}")


# ---- 3. the engine, stepwise ----------------------------------------------------------------------------------------------------------
def _check_records(eng, ocfg, trees, ro, e, aid, frames, xs, ys, horizon, records, value, worst, n_obs):
    """every sub-grid record re-derived as _check_rollout_stepwise (tests/test_engine_gpu.py) does it, from the device's own step-0
    state and forked carry; then value / worst against the restatement of the record's own costs, at the right [f, iy, ix]"""
    n, K, HC = ocfg.n_agents, horizon, eng.HC
    tab = E.ray_table(32)
    src_agent, src_rnn = ro.agent[e].cpu().numpy(), ro._rnn_em[e].cpu().numpy()
    src_hits = ro.hits[e].cpu().numpy() if ro.hits is not None else None
    covered = np.zeros(tuple(value.shape[:3]), bool)
    for f0, f1, y0, y1, x0, x1, rec in records:
        Gb = (f1 - f0) * (y1 - y0) * (x1 - x0)
        assert rec.B == Gb and rec.T == K and not rec.stochastic and Gb * (K + 1) <= eng.prepass_graphs
        r = _np_rollout(rec)
        assert r["agent"].shape == (Gb, K + 1, n, ocfg.state_dim) and r["costs"].shape == (Gb, K, n, ocfg.n_cost)
        # ---- step 0 is the fork of the source record ----
        fr = [int(t) for t in frames[f0:f1]]
        P = (y1 - y0) * (x1 - x0)
        _same(r["agent"][:, 0], _moved(src_agent, fr, aid, xs[x0:x1], ys[y0:y1]), "step-0 state")
        _same(r["goal"], np.broadcast_to(ro.goal[e].cpu().numpy(), r["goal"].shape), "goals")
        carry0 = rec._rnn_em[:, 0].cpu().numpy()
        if eng.hp.use_rnn:
            _same(carry0, np.repeat(src_rnn[fr], P, axis=0), "forked carry: the actor's pre-step carry of the frame")
        else:
            assert not carry0.any()
        if src_hits is not None:
            others = [i for i in range(n) if i != aid]
            _same(r["hits"][:, 0][:, others], np.repeat(src_hits[fr], P, axis=0)[:, others], "step-0 hits of the unmoved agents")
            sensed = E.lidar_sense(ocfg, r["agent"][:, 0, :, :2], r["obst"], *tab)[0]
            _same(r["hits"][:, 0], sensed, "step-0 hits are the oracle's sensing of the step-0 state")
        # ---- every step ----
        h = torch.from_numpy(carry0.copy())
        for t in range(K):
            hits_t = r["hits"][:, t] if src_hits is not None else None
            g = T.graph_to_torch(E.get_graph(ocfg, r["agent"][:, t], r["goal"], r["obst"], hits_t))
            with torch.no_grad():
                a, h_new = T.policy_mode(trees["policy"], g, h, n)
            np.testing.assert_allclose(r["actions"][:, t], a.numpy(), atol=1e-5)
            if eng.hp.use_rnn:
                np.testing.assert_allclose(r["rnn_states"][:, t], h_new.numpy(), atol=1e-5)      # a deterministic record: post-step
            out = E.env_step(ocfg, r["agent"][:, t], r["goal"], r["obst"], hits_t, r["actions"][:, t], tab)
            np.testing.assert_array_equal(r["rewards"][:, t], out["reward"])
            np.testing.assert_array_equal(r["costs"][:, t], out["cost"])
            np.testing.assert_array_equal(r["agent"][:, t + 1], out["next_agent"])
            if src_hits is not None:
                np.testing.assert_array_equal(r["hits"][:, t + 1], out["next_hits"])
            h = h_new
        # ---- the fold of the record's own costs ----
        want_v, want_w = fold_np(np.ascontiguousarray(r["costs"].transpose(1, 0, 2, 3)), eng.hp.gamma)
        shape = (f1 - f0, y1 - y0, x1 - x0, n, ocfg.n_cost)
        _same(value[f0:f1, y0:y1, x0:x1], want_v.reshape(shape), "value")
        _same(worst[f0:f1, y0:y1, x0:x1], want_w.reshape(shape), "worst")
        assert not covered[f0:f1, y0:y1, x0:x1].any()
        covered[f0:f1, y0:y1, x0:x1] = True
    assert covered.all(), "the sub-grids cover the grid exactly once"


# (kind, n, n_obs, horizon, grid, engine keywords, _setup keywords)
ENGINE_CASES = [
    ("LidarSpread", 3, 2, 4, (3, 2), dict(fused_step=True), {}),     # no one-launch step for this shape: four launches either way
    ("LidarSpread", 3, 2, 4, (3, 2), dict(fused_step=False), {}),
    ("LidarSpread", 4, 2, 4, (3, 2), dict(fused_step=True), {}),     # an act-step instance (tests/test_act_step_gpu.py): one launch
    ("LidarSpread", 4, 2, 4, (3, 2), dict(fused_step=False), {}),
    ("MPETarget", 3, 0, 4, (3, 2), {}, {}),
    ("LidarSpread", 24, 2, 2, (2, 2), {}, {}),                          # the tiled attention path
    ("LidarSpread", 3, 2, 4, (3, 2), {}, dict(use_rnn=False)),
    ("LidarSpread", 3, 2, 4, (3, 2), {}, dict(rnn_layers=2)),
    ("LidarSpread", 3, 2, 4, (3, 2), dict(algo="informarl"), {}),        # it needs only the policy
]
_engine_id = lambda c: "-".join([c[0], str(c[1])] + [f"{k}={v}" for d in c[5:] for k, v in d.items()])


@pytest.mark.parametrize("case", ENGINE_CASES, ids=[_engine_id(c) for c in ENGINE_CASES])
def test_engine_rollout_landscape_stepwise(cuda, case):
    """T = 8, frames [0, 3, 7], so frame 7 rolls past the episode's end; from a stochastic and from a deterministic record; the
    first case once more with prepass_graphs small enough to force pieces of a row"""
    kind, n, n_obs, horizon, (nx, ny), engine_kw, setup_kw = case
    B, T_ = 2, 8
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, B, T_, cuda, 16, 4, **setup_kw, **engine_kw)
    if "fused_step" in engine_kw:                      # the one-launch step where the shape has one, and only when asked for
        assert eng.fused_step == (engine_kw["fused_step"] and (kind, n, n_obs) in INSTANCES)
    assert eng.HC == 64 * setup_kw.get("rnn_layers", 1)
    seeds = torch.tensor([9, 10], dtype=torch.int64, device=cuda) * 104729
    frames = np.array([0, 3, 7])
    A, e, aid = float(cfg.area_size), 1, n - 1
    xs = np.linspace(0.2, A - 0.2, nx).astype(f32)
    ys = np.linspace(0.3, A - 0.3, ny).astype(f32)
    splits = [None, 10] if case is ENGINE_CASES[0] else [None]
    for stochastic in (True, False):
        ro = eng.rollout(seeds, stochastic, noise_seed=5).finalize()
        assert int(eng.reset_failed) == 0
        for prepass in splits:
            keep = eng.prepass_graphs
            if prepass is not None:
                eng.prepass_graphs = prepass                     # 10 // (horizon + 1) = 2 envs per sub-grid: pieces of a row of 3
            records, events = [], []
            try:
                value, worst = eng.rollout_landscape(ro, e, aid, frames, xs, ys, horizon, events=events, records=records)
                torch.cuda.synchronize()
                assert len(records) == (1 if prepass is None else len(frames) * ny * 2) and len(events) == len(records)
                assert all(len(ev) == 4 and ev[0].elapsed_time(ev[3]) >= 0.0 for ev in events)
                assert tuple(value.shape) == tuple(worst.shape) == (len(frames), ny, nx, n, cfg.n_cost)
                _check_records(eng, ocfg, trees, ro, e, aid, frames, xs, ys, horizon, records, value.cpu().numpy(),
                               worst.cpu().numpy(), n_obs)
            finally:
                eng.prepass_graphs = keep
            # without the records the call gives the same bits (one record reused by every sub-grid)
            if prepass is not None:
                eng.prepass_graphs = prepass
                try:
                    v2, w2 = eng.rollout_landscape(ro, e, aid, frames, xs, ys, horizon)
                finally:
                    eng.prepass_graphs = keep
                _same(v2, value.cpu().numpy(), "value, records not kept")
                _same(w2, worst.cpu().numpy(), "worst, records not kept")
        # the source record is untouched and a later rollout of the engine still works
        again = eng.rollout(seeds, stochastic, noise_seed=5).finalize()
        assert torch.equal(again.agent, ro.agent) and torch.equal(again.costs, ro.costs)


# ---- 4. cross-check with cost_landscape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 3, 2), ("MPEConnectSpread", 4, 1)])
def test_horizon_one_is_the_cost_landscape(cuda, kind, n, n_obs):
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, 2, 6, cuda, 16, 2)
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), False).finalize()
    A = float(cfg.area_size)
    p = ro.agent[0, 2, 0, :2].cpu().numpy()                          # through agent 0's own position in frame 2
    xs = np.array([0.0, p[0], 0.5 * A, A], f32)
    ys = np.array([0.0, p[1], A], f32)
    frames = [2, 0, 5]
    cost = eng.cost_landscape(ro, 0, 0, frames, xs, ys).cpu().numpy()
    value, worst = eng.rollout_landscape(ro, 0, 0, frames, xs, ys, 1)
    _same(value, cost, "horizon 1: value")
    _same(worst, cost, "horizon 1: worst")
    _same(cost[0, 1, 1], ro.costs[0, 2].cpu().numpy(), "the recorded position gives the recorded cost")
    value, worst = (x.cpu().numpy() for x in eng.rollout_landscape(ro, 0, 0, frames, xs, ys, 5))
    ok = np.isfinite(worst) & np.isfinite(cost)
    assert ok.any() and (worst[ok] >= cost[ok]).all(), "the worst cost of the horizon includes the first"
    ok &= np.isfinite(value)
    assert (value[ok] >= cost[ok]).all(), "V[c] = max(h[0][c], ...): the discounted-to-max return includes the cost now"


# ---- 5. the public interface -------------------------------------------------------------------------------------------------------------
def test_algo_rollout_landscape(cuda, tmp_path):
    from dgppo_amd.trainer.data import Rollout, RolloutLandscape
    n, Tn = 3, 6
    run, build = _checkpoint(tmp_path, "dgppo", n, Tn)
    env, algo = build()
    sig = inspect.signature(algo.rollout_landscape).parameters
    assert [(k, sig[k].default) for k in ("frames", "nx", "ny", "xs", "ys", "horizon")] == \
        [("frames", None), ("nx", 64), ("ny", 64), ("xs", None), ("ys", None), ("horizon", 32)]
    keys = np.random.default_rng(3).integers(1, 2 ** 62, size=2)
    ro = algo.collect_deterministic(keys, env=env)
    rl = algo.rollout_landscape(ro, 1, 2, frames=[0, 4], nx=4, ny=3, horizon=3)
    assert isinstance(rl, RolloutLandscape) and rl.agent == 2 and rl.horizon == 3 and rl.gamma == float(algo.engine.hp.gamma)
    assert rl.value.shape == rl.worst.shape == (2, 3, 4, n, 2) and rl.value.dtype == rl.worst.dtype == f32
    np.testing.assert_array_equal(rl.xs, np.linspace(0.0, env.area_size, 4).astype(f32))
    np.testing.assert_array_equal(rl.ys, np.linspace(0.0, env.area_size, 3).astype(f32))
    assert rl.frames.tolist() == [0, 4] and rl.frames.dtype == np.int64 and rl.h().shape == rl.v().shape == (2, 3, 4)
    want = algo.engine.rollout_landscape(algo._last_rollouts[id(ro.actions)], 1, 2, [0, 4], rl.xs, rl.ys, 3)
    _same(want[0], rl.value, "value")
    _same(want[1], rl.worst, "worst")
    full = algo.rollout_landscape(ro, 0, 0, nx=2, ny=2, horizon=1)                    # frames default to all of them
    assert full.frames.tolist() == list(range(Tn)) and full.worst.shape == (Tn, 2, 2, n, 2)
    cost = algo.cost_landscape(ro, 0, 0, nx=2, ny=2)
    _same(full.worst, cost.cost, "horizon 1 is the cost landscape")
    st = algo.collect_stochastic(keys, env=env)                                       # a stochastic record serves as well
    assert algo.rollout_landscape(st, 0, 1, frames=[Tn - 1], nx=2, ny=2, horizon=2).value.shape == (1, 2, 2, n, 2)
    with pytest.raises(ValueError, match="needs a Rollout produced by this algo"):
        algo.rollout_landscape(Rollout(*ro)._replace(actions=ro.actions.clone()), 0, 0, nx=2, ny=2, horizon=1)
    for horizon in (0, -2):
        with pytest.raises(ValueError, match="horizon"):
            algo.rollout_landscape(ro, 0, 0, nx=2, ny=2, horizon=horizon)
    for kw, match in ((dict(index=2), "env_index"), (dict(agent=3), "agent_id"), (dict(frames=[Tn]), "frame_ids"),
                      (dict(frames=[]), "frame_ids"), (dict(nx=0), "xs"), (dict(ys=[0.5, float("nan")]), "ys")):
        args = dict(index=0, agent=0, frames=[0], nx=2, ny=2, horizon=1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            algo.rollout_landscape(ro, **args)


def test_vmas_engine_refuses(cuda):
    from dgppo_amd import _native as N, engine as EN
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="rollout_landscape.*VMASReverseTransport"):
        vmas.rollout_landscape(None, 0, 0, [0], [0.5], [0.5], 1)


BASE_KEYS = ["xs", "ys", "value", "worst", "agent", "frames", "horizon", "gamma", "points", "doomed", "doomed_frac"]
AGREEMENT_KEYS = ["missed", "conservative", "missed_frac", "conservative_frac", "value_error", "latent", "latent_frac"]


def test_cli_writes_the_rollout_landscape(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    n, grid, Tn, horizon = 3, 4, 6, 3
    run, build = _checkpoint(tmp_path, "dgppo", n, Tn)
    mod = _load_test_py()
    common = ["--path", str(run), "--rollout-landscape", "0", "--rollout-horizon", str(horizon), "--landscape-grid", str(grid),
              "--epi", "2", "--no-video", "--max-step", str(Tn)]
    mod.main(common)
    printed = capsys.readouterr().out
    assert printed.count("doomed_frac") == 2 and printed.count("rollout landscape: ") == 2 and "missed_frac" not in printed
    vdir = run / "videos" / "0"
    newest = lambda: sorted(glob.glob(str(vdir / "*_rollout.npz")), key=lambda p: (os.path.getmtime(p), p))[-2:]
    files = sorted(newest())
    assert len(files) == 2 and not [p for p in glob.glob(str(vdir / "*")) if p.endswith((".gif", ".mp4"))]
    env2, algo2 = build()                                       # the same episodes again, from the checkpoint
    algo2.load(str(run / "models"), 0)
    keys = np.random.default_rng([1234, 13]).integers(1, 2 ** 62, size=1000)[:2]
    ro = algo2.collect_deterministic(keys, env=env2)
    for i, path in enumerate(files):
        z = np.load(path)
        assert sorted(z.files) == sorted(BASE_KEYS)
        assert z["value"].shape == z["worst"].shape == (Tn, grid, grid, n, 2)
        assert int(z["agent"]) == 0 and int(z["horizon"]) == horizon and float(z["gamma"]) == float(algo2.engine.hp.gamma)
        np.testing.assert_array_equal(z["frames"], np.arange(Tn))
        np.testing.assert_array_equal(z["xs"], np.linspace(0.0, env2.area_size, grid).astype(f32))
        rl = algo2.rollout_landscape(ro, i, 0, nx=grid, ny=grid, horizon=horizon)
        _same(z["value"], rl.value, "value")
        _same(z["worst"], rl.worst, "worst")
        for key, v in EV.rollout_agreement(rl).items():
            np.testing.assert_array_equal(z[key], v)
    # with the learned and the true landscape of the same agent: the agreement statistics join the file and the line
    mod.main(common + ["--landscape", "0", "--cost-landscape", "0"])
    printed = capsys.readouterr().out
    for key in ("doomed_frac", "missed_frac", "conservative_frac", "value_error", "latent_frac"):
        assert printed.count(f"({key})") >= 2, key
    for i, path in enumerate(sorted(newest())):
        z = np.load(path)
        assert sorted(z.files) == sorted(BASE_KEYS + AGREEMENT_KEYS)
        rl = algo2.rollout_landscape(ro, i, 0, nx=grid, ny=grid, horizon=horizon)
        agree = EV.rollout_agreement(rl, land=algo2.vh_landscape(ro, i, 0, nx=grid, ny=grid),
                                     cost=algo2.cost_landscape(ro, i, 0, nx=grid, ny=grid))
        assert sorted(agree) == sorted(BASE_KEYS[8:] + AGREEMENT_KEYS)
        for key, v in agree.items():
            np.testing.assert_array_equal(z[key], v)
