"""Vh landscape: dgppo_graph_feats_sweep (one agent moved over a grid in frozen frames, its LiDAR cast again) against the
oracle's lidar_sense + get_graph and against the composition of the existing entry points, Engine.vh_landscape against the
oracle's value_Vh, the refusals, and test.py --landscape in-process."""
import ctypes as C
import functools
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _to(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits_equal(got, want, name):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}"


def _edge_of_slot(cfg):
    """[n, S] index into the oracle graph's edge list of slot s of agent i: E.get_graph lays its edges out as the agent-agent
    block (receiver-major), the agent-goal block, the agent-obstacle block"""
    n, gs, os_ = cfg.n_agents, cfg.goal_slots, cfg.obs_slots
    i = np.arange(n)[:, None]
    return np.concatenate([i * n + np.arange(n)[None], n * n + i * gs + np.arange(gs)[None],
                           n * n + n * gs + i * os_ + np.arange(os_)[None]], axis=1)


# ---- 1. the sweep against the oracle --------------------------------------------------------------------------------------
RECT = (f32(1.0), f32(1.2))          # centre of rectangle 0 / MPE obstacle 0: a grid point
FAR = (f32(1.3), f32(1.2))           # farther than comm_radius (0.5) from the corner cluster the other agents stand in
ORACLE_CASES = [("LidarSpread", 3, 2, 32, 8), ("LidarTarget", 3, 2, 32, 8), ("LidarBicycleTarget", 3, 2, 32, 8),
                ("LidarSpread", 3, 0, 32, 8), ("LidarSpread", 1, 1, 32, 8), ("LidarLine", 4, 2, 32, 8), ("MPETarget", 3, 3, 0, 0),
                ("MPEConnectSpread", 4, 1, 0, 0), ("LidarTarget", 3, 2, 12, 8)]


def _cfgs(kind_name, n, n_obs, n_rays, top_k):
    from dgppo_amd import _native as N
    kind = N.ENV_KINDS[kind_name]
    lidar = n_rays > 0
    cfg = N.make_env_cfg(kind, n, n_obs, **(dict(n_rays=n_rays, top_k=top_k) if lidar else {}))
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs, **(dict(n_rays=n_rays, top_k=top_k) if lidar else {}))
    assert (cfg.n_obs, cfg.n_goals, cfg.num_nodes, cfg.num_edges) == (ocfg.n_obs, ocfg.n_goals, ocfg.num_nodes, ocfg.num_edges)
    return cfg, ocfg


@functools.lru_cache(maxsize=None)
def _hand_scene(kind_name, n, n_obs, n_rays, top_k):
    """a 3-frame record of one env built by hand (read-only): agents clustered in the lower left corner, rectangle / disc 0
    centred at RECT, an axis-aligned rectangle next to the cluster so that recorded hits are unmasked too"""
    cfg, ocfg = _cfgs(kind_name, n, n_obs, n_rays, top_k)
    sd, Tn = ocfg.state_dim, 3
    rng = np.random.default_rng(5)
    agent = np.zeros((Tn, n, sd), f32)
    for t in range(Tn):
        for i in range(n):                                          # the cluster drifts a little from frame to frame
            agent[t, i, 0] = f32(0.1 + 0.12 * i + 0.01 * t)
            agent[t, i, 1] = f32(0.1 + 0.04 * i + 0.005 * t)
    if ocfg.is_bicycle:
        th = rng.uniform(-np.pi, np.pi, size=(Tn, n))
        agent[..., 2], agent[..., 3] = np.cos(th).astype(f32), np.sin(th).astype(f32)
        agent[..., 4] = rng.uniform(-0.5, 0.5, size=(Tn, n)).astype(f32)
    else:
        agent[..., 2:4] = rng.uniform(-0.5, 0.5, size=(Tn, n, 2)).astype(f32)
    goal = np.zeros((ocfg.n_goals, sd), f32)
    goal[:, :2] = rng.uniform(0.2, 1.3, size=(ocfg.n_goals, 2)).astype(f32)
    if ocfg.is_bicycle:
        goal[:, 2] = 1.0
    obst = hits = None
    no = ocfg.n_obs
    if no > 0 and ocfg.is_lidar:
        centres = np.array([RECT, (0.45, 0.5), (0.8, 0.3)][:no], f32)
        obst = E.make_rect(centres, np.array([0.3, 0.2, 0.1][:no], f32), np.array([0.2, 0.2, 0.3][:no], f32),
                           np.array([0.3, 0.0, 1.1][:no], f32))
        tab = E.ray_table(n_rays)
        hits = E.lidar_sense(ocfg, agent[..., :2], np.broadcast_to(obst, (Tn,) + obst.shape), *tab)[0]
    elif no > 0:
        obst = np.zeros((no, sd), f32)
        obst[:, :2] = np.array([RECT, (0.3, 0.45), (0.8, 0.3)][:no], f32)
    for a in (agent, goal, obst, hits):
        if a is not None:
            a.setflags(write=False)
    return cfg, ocfg, agent, goal, obst, hits


def _oracle_sweep(ocfg, agent, goal, obst, hits, frame_ids, aid, xs, ys):
    """the G = F * ny * nx swept graphs on the CPU: moved state -> lidar_sense of all agents -> get_graph"""
    F, ny, nx, n = len(frame_ids), len(ys), len(xs), ocfg.n_agents
    ag = np.repeat(agent[frame_ids], ny * nx, axis=0).reshape(F, ny, nx, n, -1).copy()
    ag[:, :, :, aid, 0] = xs[None, None, :]
    ag[:, :, :, aid, 1] = ys[None, :, None]
    ag = ag.reshape(F * ny * nx, n, -1)
    G = ag.shape[0]
    tile = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (G,) + a.shape))
    h = None
    if hits is not None:
        h = E.lidar_sense(ocfg, ag[..., :2], tile(obst), *E.ray_table(ocfg.n_rays))[0]
        rec = np.repeat(hits[frame_ids], ny * nx, axis=0)
        others = [i for i in range(n) if i != aid]
        _bits_equal(h[:, others], rec[:, others], "lidar_sense is a pure function: the unmoved agents' hits are the recorded ones")
    return ag, h, E.get_graph(ocfg, ag, tile(goal), tile(obst), h)


def _grid(agent, frame_ids, aid, n):
    """5 x 3 grid lines through (a) RECT, (b) another agent's position, (c) the moved agent's own, (d) FAR; the positions are
    those of the first swept frame"""
    t0 = frame_ids[0]
    pc = agent[t0, aid, :2]
    pb = agent[t0, (aid + 1) % n, :2] if n > 1 else np.array([0.55, 0.9], f32)
    xs = np.array([pb[0], pc[0], RECT[0], FAR[0], 0.7], f32)
    ys = np.array([pb[1] if n > 1 else 0.9, pc[1], RECT[1]], f32)
    return xs, ys, dict(a=(2, 2), b=(0, 0), c=(1, 1), d=(3, 2))     # (ix, iy) of the four points


@pytest.mark.parametrize("kind,n,n_obs,n_rays,top_k", ORACLE_CASES, ids=["-".join(map(str, c)) for c in ORACLE_CASES])
def test_sweep_matches_oracle(cuda, kind, n, n_obs, n_rays, top_k):
    """dgppo_graph_feats_sweep on a strided 3-frame record (a slice of a wider NaN-filled allocation), frame_ids [2, 0],
    agent_id 0 and n - 1, Fp = node_dim and 8: emask equals "the oracle edge is not routed to the pad node", efeat is
    bit-equal on unmasked slots, Xa / Xo bit-equal to the oracle's node rows zero padded, hits_out bit-equal to the oracle's
    hits of the moved agent.  The grid holds a rectangle centre, another agent's position, the agent's own recorded position
    and a point out of everyone's range; the oracle's output is asserted to show each of them before the GPU is used."""
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits, = _hand_scene(kind, n, n_obs, n_rays, top_k)
    frame_ids = [2, 0]
    sd, k, S, Tn = ocfg.state_dim, ocfg.top_k, cfg.fan_in, 3
    n_other, pad = cfg.num_nodes - 1 - n, cfg.num_nodes - 1
    cast = hits is not None
    eos = _edge_of_slot(cfg)
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread).numpy()
    want = {}
    for aid in sorted({0, n - 1}):
        xs, ys, pts = _grid(agent, frame_ids, aid, n)
        nx, ny = len(xs), len(ys)
        ag, h, gr = _oracle_sweep(ocfg, agent, goal, obst, hits, frame_ids, aid, xs, ys)
        recv, send, edges = gr["receivers"][:, eos], gr["senders"][:, eos], gr["edges"][:, eos]       # [G, n, S(, 4)]
        on = recv != pad
        assert (recv[on] == np.broadcast_to(np.arange(n)[:, None], recv.shape)[on]).all()
        assert (send[on] == np.broadcast_to(snd, send.shape)[on]).all() and ((send == pad) == ~on).all()
        # ---- the preconditions, on the oracle's output ----
        g_of = lambda f, p: (f * ny + pts[p][1]) * nx + pts[p][0]
        others = [i for i in range(n) if i != aid]
        for f in range(len(frame_ids)):
            if cast:
                pa = np.array([xs[pts["a"][0]], ys[pts["a"][1]]], f32)
                assert (h[g_of(f, "a"), aid] == pa).all(), "inside a rectangle every hit is the point itself"
            if n > 1:
                assert not on[g_of(f, "d"), aid][others].any() and not on[g_of(f, "d")][others, aid].any()
        if n > 1:
            assert on[g_of(0, "b"), aid][others].all(), "next to the cluster the moved agent hears every other agent"
        assert (ag[g_of(0, "c")] == agent[frame_ids[0]]).all(), "(c) is the recorded state"
        if cfg.obs_slots > 0 and kind != "MPEConnectSpread":          # ConnectSpread connects every obstacle (mask radius 50)
            ob = on[:, :, n + cfg.goal_slots:]
            assert ob.any() and (~ob).any() and ob[:, aid].any() and (~ob[:, aid]).any()
        want[aid] = (xs, ys, on, edges, gr["nodes"], h)

    d_goal, d_obst = _to(goal, cuda), _to(obst, cuda)
    wide_a = torch.full((Tn + 1, n + 2, sd), float("nan"), device=cuda)
    agd = wide_a[:Tn, 1:n + 1]
    agd.copy_(_to(agent, cuda))
    a_st = (n + 2) * sd
    hid, h_st = None, 0
    if cast:
        wide_h = torch.full((Tn, 2, n, k, 2), float("nan"), device=cuda)
        hid = wide_h[:, 1]
        hid.copy_(_to(hits, cuda))
        h_st = 2 * n * k * 2
    rc, rs = (_to(x, cuda) for x in E.ray_table(n_rays)) if cast else (None, None)
    for aid, (xs, ys, on, edges, nodes, h) in want.items():
        G = len(frame_ids) * len(ys) * len(xs)
        dxs, dys = K_.sweep_axis(xs, "xs", cuda), K_.sweep_axis(ys, "ys", cuda)
        for Fp in (cfg.node_dim, 8):
            Xa = torch.full((G * n, Fp), float("nan"), device=cuda)
            Xo = torch.full((G * n_other, Fp), float("nan"), device=cuda)
            ef = torch.full((G * n, S, 4), float("nan"), device=cuda)
            em = torch.full((G * n, S), float("nan"), device=cuda)
            ho = torch.full((G, k, 2), float("inf"), device=cuda) if cast else None
            K_.graph_feats_sweep(cfg, agd, a_st, d_goal, d_obst, hid, h_st, rc, rs, frame_ids, len(frame_ids), aid, dxs, dys,
                                 Xa, Xo if n_other > 0 else None, ef, em, Fp, ho)
            torch.cuda.synchronize()
            tag = f"agent {aid} Fp={Fp}"
            np.testing.assert_array_equal(em.cpu().numpy().reshape(G, n, S), on.astype(f32), err_msg=f"emask {tag}")
            _bits_equal(ef.cpu().numpy().reshape(G, n, S, 4)[on], np.ascontiguousarray(edges[on]), f"efeat {tag}")
            rows = np.zeros((G, cfg.num_nodes - 1, Fp), f32)
            rows[..., :cfg.node_dim] = nodes[:, :pad]
            _bits_equal(Xa.cpu().numpy().reshape(G, n, Fp), rows[:, :n], f"Xa {tag}")
            if n_other > 0:
                _bits_equal(Xo.cpu().numpy().reshape(G, n_other, Fp), rows[:, n:], f"Xo {tag}")
            if cast:
                _bits_equal(ho.cpu().numpy(), h[:, aid], f"hits_out {tag}")


# ---- 2. the sweep against the composition of the existing entry points --------------------------------------------------------
COMPOSE_CASES = [("LidarSpread", 8, 3, None), ("LidarBicycleTarget", 16, 8, None), ("LidarSpread", 20, 3, 4.0)]


def _compose(cfg, agent, goal, obst, frames, aid, xs, ys, cuda):
    """the record tiled G times, the agent row overwritten, ops_env.sense, ops_nn.graph_feats"""
    from dgppo_amd import nets, ops_env as OE, ops_nn as K_
    n, sd, k, S = cfg.n_agents, cfg.state_dim, cfg.top_k, cfg.fan_in
    F, ny, nx = len(frames), len(ys), len(xs)
    G = F * ny * nx
    ag = agent[frames].unsqueeze(1).unsqueeze(1).expand(F, ny, nx, n, sd).clone()
    ag[:, :, :, aid, 0] = xs.view(1, 1, nx)
    ag[:, :, :, aid, 1] = ys.view(1, ny, 1)
    ag = ag.view(G, n, sd)
    st = OE.State({"agent": ag}, {"goal": goal.unsqueeze(0).expand(G, -1, -1).contiguous(),
                                  "obst": obst.unsqueeze(0).expand(G, -1, -1).contiguous()})
    OE.sense(cfg, st)
    Fp, n_other = nets.input_width(cfg), cfg.num_nodes - 1 - n
    out = dict(Xa=torch.empty(G * n, Fp, device=cuda), Xo=torch.empty(G * n_other, Fp, device=cuda),
               ef=torch.empty(G * n, S, 4, device=cuda), em=torch.empty(G * n, S, device=cuda))
    K_.graph_feats(cfg, ag, n * sd, 0, st.goal, None, st.hits, n * k * 2, 0, None, G, 1, out["Xa"], out["Xo"], out["ef"], out["em"], Fp)
    out["hits"] = st.hits[:, aid].contiguous()
    return out


@pytest.mark.parametrize("kind,n,n_obs,area", COMPOSE_CASES, ids=["-".join(map(str, c)) for c in COMPOSE_CASES])
def test_sweep_equals_composition(cuda, kind, n, n_obs, area):
    """every word of every output, masked slots included, equals what tiling the record, overwriting the agent row, sensing
    all agents again and running dgppo_graph_feats gives — on a 16 x 16 grid over 2 frames, a 1 x 1 and a 1 x 7 grid"""
    from dgppo_amd import _native as N, nets, ops_env as OE, ops_nn as K_
    cfg = N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs, **({} if area is None else dict(area_size=area)))
    A, sd, k, S = float(cfg.area_size), cfg.state_dim, cfg.top_k, cfg.fan_in
    st0 = OE.State.empty(cfg, 1, cuda)
    OE.reset(cfg, torch.tensor([4242], dtype=torch.int64, device=cuda), st0)
    st1 = st0.like()
    gen = torch.Generator().manual_seed(3)
    act = (torch.rand(1, n, 2, generator=gen) * 2 - 1).to(cuda)
    OE.step(cfg, st0, act, st1, torch.empty(1, device=cuda), torch.empty(1, n, cfg.n_cost, device=cuda))
    agent = torch.cat([st0.agent, st1.agent], 0).contiguous()           # [2, n, sd]
    hits = torch.cat([st0.hits, st1.hits], 0).contiguous()
    goal, obst = st0.goal[0].contiguous(), st0.obst[0].contiguous()
    rc, rs = OE._rays(cfg, cuda)
    Fp, n_other = nets.input_width(cfg), cfg.num_nodes - 1 - n
    aid = n // 2
    grids = [(np.linspace(0.0, A, 16).astype(f32), np.linspace(0.0, A, 16).astype(f32), [0, 1]),
             (np.array([0.37 * A], f32), np.array([0.61 * A], f32), [1]),
             (np.linspace(0.1, A, 7).astype(f32), np.array([0.5 * A], f32), [1, 0])]
    for xs, ys, frames in grids:
        dxs, dys = K_.sweep_axis(xs, "xs", cuda), K_.sweep_axis(ys, "ys", cuda)
        G = len(frames) * len(ys) * len(xs)
        want = _compose(cfg, agent, goal, obst, frames, aid, dxs, dys, cuda)
        got = dict(Xa=torch.full((G * n, Fp), float("nan"), device=cuda), Xo=torch.full((G * n_other, Fp), float("nan"), device=cuda),
                   ef=torch.full((G * n, S, 4), float("nan"), device=cuda), em=torch.full((G * n, S), float("nan"), device=cuda),
                   hits=torch.full((G, k, 2), float("inf"), device=cuda))
        K_.graph_feats_sweep(cfg, agent, n * sd, goal, obst, hits, n * k * 2, rc, rs, frames, len(frames), aid, dxs, dys,
                             got["Xa"], got["Xo"], got["ef"], got["em"], Fp, got["hits"])
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), f"{key} grid {len(xs)}x{len(ys)}"
        assert (got["em"] == 0).any() and (got["em"] == 1).any()


# ---- 3. Engine.vh_landscape ----------------------------------------------------------------------------------------------------
def _close(got, want, tol=1e-5, name=""):
    """tests/test_nn_gpu.py's rule for the Vh forward: 1e-5 of the output scale"""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} (scale {scale:.3e})")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e})"


def _engine(kind_name, n, n_obs, T_, cuda, use_rnn=True, area=None):
    from dgppo_amd import _native as N, engine as EN, init
    kind = N.ENV_KINDS[kind_name]
    kw = {} if area is None else dict(area_size=area)
    cfg = N.make_env_cfg(kind, n, n_obs, **kw)
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs, **kw)
    nc = 1 if use_rnn else 0
    hp = EN.Hyper(batch_size=1024, rnn_step=2, train_steps=100, use_rnn=use_rnn, rnn_layers=1, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=nc)}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    trees = {k_: jitter(v) for k_, v in trees.items()}
    for k_, net in eng.nets.items():
        net.load_tree(trees[k_])
    eng.set_entropy_noise(77)
    return cfg, ocfg, eng, trees


@pytest.mark.parametrize("use_rnn", [True, False], ids=["gru", "no-rnn"])
def test_vh_landscape_matches_oracle(cuda, use_rnn):
    """LidarSpread n = 3, obs = 2, T = 4, B = 2, a 4 x 3 grid over frames [2, 0] holding the agent's recorded position of each:
    every value against value_Vh on the oracle's graph of the moved state with the carry of that step (tolerance of the Vh
    forward test), the value at the recorded position against values_prepass's Vh[e, t] — for a stochastic and a deterministic
    rollout, whose stored carries differ by one step — and prepass_graphs = 5 / 3 bit-equal to the unchunked call."""
    T_, B, e, aid = 4, 2, 1, 1
    cfg, ocfg, eng, trees = _engine("LidarSpread", 3, 2, T_, cuda, use_rnn)
    n = cfg.n_agents
    seeds = torch.tensor([9, 10], dtype=torch.int64, device=cuda)
    for stochastic in (True, False):
        ro = eng.rollout(seeds, stochastic, noise_seed=5).finalize()
        _, Vh_pre = eng.values_prepass(ro, want_Vl=False)
        Vh_pre = Vh_pre.clone()
        frames = [2, 0]
        agent = ro.agent[e].cpu().numpy()
        pos = agent[frames, aid, :2]
        xs = np.array([pos[0, 0], pos[1, 0], 0.3, 1.1], f32)
        ys = np.array([pos[0, 1], pos[1, 1], 0.8], f32)
        got = eng.vh_landscape(ro, e, aid, frames, xs, ys)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (2, 3, 4, n, cfg.n_cost)
        name = f"{'stochastic' if stochastic else 'deterministic'}"
        for f, t in enumerate(frames):
            _close(got[f, f, f], Vh_pre[e, t], 1e-5, f"{name}: landscape at the recorded position of frame {t} vs values_prepass")
        _, _, gr = _oracle_sweep(ocfg, agent, ro.goal[e].cpu().numpy(), ro.obst[e].cpu().numpy(), ro.hits[e].cpu().numpy(),
                                 frames, aid, xs, ys)
        h = ro.rnn_states[e].cpu()[frames]                                       # [F, n, 64]
        h = h[:, None].expand(-1, len(ys) * len(xs), -1, -1).reshape(-1, n, h.shape[-1])
        with torch.no_grad():
            want, _ = T.value_Vh(trees["Vh"], T.graph_to_torch(gr), h, n)
        _close(got.reshape(-1, n, cfg.n_cost), want, 1e-5, f"{name}: landscape vs value_Vh(get_graph)")
        keep = eng.prepass_graphs
        try:
            for cap in (5, 3):
                eng.prepass_graphs = cap
                again = eng.vh_landscape(ro, e, aid, frames, xs, ys)
                assert torch.equal(again.view(torch.int32), got.view(torch.int32)), f"{name}: prepass_graphs = {cap}"
        finally:
            eng.prepass_graphs = keep


def test_vh_landscape_large_team(cuda):
    """n = 24, area 4.0 (the attention runs the tiled kernels), 2 x 2 grid: the value at the recorded position equals
    values_prepass's Vh[e, t]"""
    cfg, ocfg, eng, trees = _engine("LidarSpread", 24, 3, 3, cuda, area=4.0)
    ro = eng.rollout(torch.tensor([3, 4], dtype=torch.int64, device=cuda), False).finalize()
    _, Vh_pre = eng.values_prepass(ro, want_Vl=False)
    Vh_pre = Vh_pre.clone()
    e, aid, t = 0, 23, 1
    p = ro.agent[e, t, aid, :2].cpu().numpy()
    got = eng.vh_landscape(ro, e, aid, [t], np.array([p[0], p[0] + f32(0.3)], f32), np.array([p[1] + f32(0.3), p[1]], f32))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 2, 2, 24, cfg.n_cost)
    _close(got[0, 1, 0], Vh_pre[e, t], 1e-5, "n = 24: landscape at the recorded position vs values_prepass")
    assert not torch.equal(got[0, 0, 1], got[0, 1, 0])


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["informarl", "hcbfcrpo", "informarl_lagr"])
def test_unsupported_algorithms_raise(cuda, algo):
    from dgppo_amd import _native as N, engine as EN
    eng = EN.Engine(N.make_env_cfg(0, 3, 2), EN.Hyper(batch_size=256), cuda, T=4, algo=algo)
    with pytest.raises(ValueError, match=algo):
        eng.vh_landscape(None, 0, 0, [0], [0.5], [0.5])


def test_bad_arguments_raise_before_any_launch(cuda):
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits = _hand_scene("LidarSpread", 3, 2, 32, 8)
    n, sd, k, S, Fp = 3, 4, 8, cfg.fan_in, 8
    n_other = cfg.num_nodes - 1 - n
    rc, rs = (_to(x, cuda) for x in E.ray_table(32))
    d = dict(agent=_to(agent, cuda), goal=_to(goal, cuda), obst=_to(obst, cuda), hits=_to(hits, cuda))
    xs, ys = K_.sweep_axis([0.2, 0.4], "xs", cuda), K_.sweep_axis([0.3], "ys", cuda)
    G = 2
    outs = [torch.full(s, float("nan"), device=cuda) for s in ((G * n, Fp), (G * n_other, Fp), (G * n, S, 4), (G * n, S))]

    def call(aid=0, xs=xs, ys=ys):
        K_.graph_feats_sweep(cfg, d["agent"], n * sd, d["goal"], d["obst"], d["hits"], n * k * 2, rc, rs, [1], 1, aid, xs, ys,
                             outs[0], outs[1], outs[2], outs[3], Fp)
    with pytest.raises(ValueError, match="agent_id"):
        call(aid=n)
    with pytest.raises(ValueError, match="finite"):
        K_.sweep_axis([0.2, float("nan")], "xs", cuda)
    with pytest.raises(ValueError, match="non-empty"):
        K_.sweep_axis([], "ys", cuda)
    with pytest.raises(ValueError, match="empty"):
        call(ys=torch.empty(0, device=cuda))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), "a refused call wrote to its outputs"
    call()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o).any()) for o in outs)


def test_vmas_kind_is_refused_through_ctypes():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    z, null = C.c_int64(0), None
    rc = lib.dgppo_graph_feats_sweep(C.byref(cfg), null, z, null, null, null, z, null, null, null, C.c_int32(1), C.c_int32(0),
                                     null, C.c_int32(1), null, C.c_int32(1), null, null, null, null, null, C.c_int32(20), null)
    assert rc != 0
    assert b"dgppo_graph_feats_sweep" in lib.dgppo_last_error()


# ---- 5. test.py --landscape, in-process ------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_writes_landscapes(cuda, tmp_path):
    import yaml
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    n, grid, Tn = 3, 6, 6
    conf = dict(env="LidarSpread", num_agents=n, obs=2, algo="dgppo", cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, seed=3, use_rnn=True, rnn_layers=1, use_lstm=False)

    def build():
        env = make_env(env_id=conf["env"], num_agents=n, num_obs=conf["obs"], max_step=Tn)
        algo = make_algo(algo="dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=n, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                         Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, max_grad_norm=2.0, seed=3, use_rnn=True, rnn_layers=1,
                         use_lstm=False)
        return env, algo
    env, algo = build()
    run = tmp_path / "run"
    algo.save(str(run / "models"), 0)
    with open(run / "config.yaml", "w") as f:
        yaml.safe_dump(conf, f)
    mod = _load_test_py()
    mod.main(["--path", str(run), "--landscape", "1", "--landscape-grid", str(grid), "--epi", "2", "--max-step", str(Tn),
              "--dpi", "30"])
    files = sorted(glob.glob(str(run / "videos" / "0" / "*_landscape.npz")))
    assert len(files) == 2
    videos = [p for p in glob.glob(str(run / "videos" / "0" / "*")) if p.endswith((".gif", ".mp4"))]
    assert len(videos) == 2 and all(os.path.getsize(p) > 1000 for p in videos)
    # the same episodes again, from the checkpoint
    env2, algo2 = build()
    algo2.load(str(run / "models"), 0)
    keys = np.random.default_rng([1234, 13]).integers(1, 2 ** 62, size=1000)[:2]
    ro = algo2.collect_deterministic(keys, env=env2)
    for i, path in enumerate(files):
        z = np.load(path)
        assert sorted(z.files) == ["Vh", "agent", "frames", "xs", "ys"]
        assert z["Vh"].shape == (Tn, grid, grid, n, env2.n_cost) and int(z["agent"]) == 1
        land = algo2.vh_landscape(ro, i, 1, nx=grid, ny=grid)
        np.testing.assert_array_equal(z["xs"], np.linspace(0.0, env2.area_size, grid).astype(f32))
        np.testing.assert_array_equal(z["frames"], np.arange(Tn))
        np.testing.assert_array_equal(z["Vh"], land.Vh)
        np.testing.assert_array_equal(land.h(), land.Vh[:, :, :, 1].max(-1))
