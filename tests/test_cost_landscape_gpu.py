"""Cost landscape: dgppo_cost_sweep (the environment's own cost of all agents with one agent moved over a grid in frozen
frames, its LiDAR cast again) bit for bit against the oracle's lidar_sense + get_cost, its NaN propagation and tile edges,
Engine.cost_landscape against the costs a real rollout recorded, the refusals, and test.py --cost-landscape in-process."""
import ctypes as C
import functools
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import env_np as E

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0


def _to(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits_equal(got, want, name):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    where = np.argwhere(bad)[:4].tolist()
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {where}: got "
                           f"{[float(got[tuple(i)]) for i in where]}, want {[float(want[tuple(i)]) for i in where]}")


def _same_cost(got, want, name):
    """equal bits wherever the oracle is finite, NaN exactly where the oracle is NaN"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaN positions")
    _bits_equal(np.where(nan, f32(0), got), np.where(nan, f32(0), want), name)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
RECT = (f32(1.0), f32(1.2))          # centre of rectangle 0 / MPE obstacle 0: a grid point
FAR = (f32(1.3), f32(1.2))           # farther than comm_radius (0.5) from the corner cluster the other agents stand in
# (kind, n, n_obs, n_rays, top_k, random): random = agents drawn in an area of 4.0 instead of the corner cluster
ORACLE_CASES = [("LidarSpread", 3, 2, 32, 8, False), ("LidarTarget", 3, 2, 32, 8, False), ("LidarBicycleTarget", 3, 2, 32, 8, False),
                ("LidarSpread", 3, 0, 32, 8, False), ("LidarSpread", 1, 1, 32, 8, False), ("LidarLine", 4, 2, 32, 8, False),
                ("LidarTarget", 3, 2, 12, 8, False), ("MPETarget", 3, 3, 0, 0, False), ("MPESpread", 3, 3, 0, 0, False),
                ("MPEConnectSpread", 4, 1, 0, 0, False), ("LidarSpread", 24, 3, 32, 8, False), ("LidarSpread", 64, 3, 32, 8, True)]
NO_NAN_CASES = 10                    # the first ten produce no NaN (checked on the oracle's output below)


def _cfgs(kind_name, n, n_obs, n_rays, top_k, area=None):
    from dgppo_amd import _native as N
    kind = N.ENV_KINDS[kind_name]
    kw = dict(n_rays=n_rays, top_k=top_k) if n_rays > 0 else {}
    if area is not None:
        kw["area_size"] = area
    cfg = N.make_env_cfg(kind, n, n_obs, **kw)
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs, **kw)
    assert (cfg.n_obs, cfg.n_cost, cfg.num_nodes) == (ocfg.n_obs, ocfg.n_cost, ocfg.num_nodes)
    return cfg, ocfg


@functools.lru_cache(maxsize=None)
def _hand_scene(kind_name, n, n_obs, n_rays, top_k, random=False):
    """a 3-frame record of one env built by hand (read-only): agents clustered in the lower left corner (random: drawn from a
    fixed seed in an area of 4.0), rectangle / disc 0 centred at RECT, an axis-aligned rectangle next to the cluster"""
    cfg, ocfg = _cfgs(kind_name, n, n_obs, n_rays, top_k, 4.0 if random else None)
    sd, Tn = ocfg.state_dim, 3
    rng = np.random.default_rng(5)
    agent = np.zeros((Tn, n, sd), f32)
    if random:
        base = np.random.default_rng(64).uniform(0.0, 4.0, size=(n, 2))
        for t in range(Tn):
            agent[t, :, :2] = (base + 0.01 * t).astype(f32)
    else:
        for t in range(Tn):
            for i in range(n):                                      # the cluster drifts a little from frame to frame
                agent[t, i, 0] = f32(0.1 + 0.12 * i + 0.01 * t)
                agent[t, i, 1] = f32(0.1 + 0.04 * i + 0.005 * t)
    if ocfg.is_bicycle:
        th = rng.uniform(-np.pi, np.pi, size=(Tn, n))
        agent[..., 2], agent[..., 3] = np.cos(th).astype(f32), np.sin(th).astype(f32)
        agent[..., 4] = rng.uniform(-0.5, 0.5, size=(Tn, n)).astype(f32)
    else:
        agent[..., 2:4] = rng.uniform(-0.5, 0.5, size=(Tn, n, 2)).astype(f32)
    obst = hits = None
    no = ocfg.n_obs
    if no > 0 and ocfg.is_lidar:
        centres = np.array([RECT, (0.45, 0.5), (0.8, 0.3)][:no], f32)
        obst = E.make_rect(centres, np.array([0.3, 0.2, 0.1][:no], f32), np.array([0.2, 0.2, 0.3][:no], f32),
                           np.array([0.3, 0.0, 1.1][:no], f32))
        hits = E.lidar_sense(ocfg, agent[..., :2], np.broadcast_to(obst, (Tn,) + obst.shape), *E.ray_table(n_rays))[0]
    elif no > 0:
        obst = np.zeros((no, sd), f32)
        obst[:, :2] = np.array([RECT, (0.3, 0.45), (0.8, 0.3)][:no], f32)
    for a in (agent, obst, hits):
        if a is not None:
            a.setflags(write=False)
    return cfg, ocfg, agent, obst, hits


def _oracle_sweep(ocfg, agent, obst, hits, frame_ids, aid, xs, ys):
    """the G = F * ny * nx swept states on the CPU: moved state -> lidar_sense of all agents -> get_cost.
    -> cost [G, n, n_cost], the moved agent's hits [G, k, 2] (or None)"""
    F, ny, nx, n = len(frame_ids), len(ys), len(xs), ocfg.n_agents
    ag = np.repeat(agent[frame_ids], ny * nx, axis=0).reshape(F, ny, nx, n, -1).copy()
    ag[:, :, :, aid, 0] = xs[None, None, :]
    ag[:, :, :, aid, 1] = ys[None, :, None]
    ag = ag.reshape(F * ny * nx, n, -1)
    G = ag.shape[0]
    tile = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (G,) + a.shape))
    if hits is None:
        return E.get_cost(ocfg, ag, tile(obst)), None
    h = E.lidar_sense(ocfg, ag[..., :2], tile(obst), *E.ray_table(ocfg.n_rays))[0]
    rec = np.repeat(hits[frame_ids], ny * nx, axis=0)
    others = [i for i in range(n) if i != aid]
    _bits_equal(h[:, others], rec[:, others], "lidar_sense is a pure function: the unmoved agents' hits are the recorded ones")
    return E.get_cost(ocfg, ag, h), h[:, aid]


def _grid(agent, frame_ids, aid, n):
    """5 x 3 grid lines through (a) RECT, (b) another agent's position, (c) the moved agent's own, (d) FAR; the positions are
    those of the first swept frame"""
    t0 = frame_ids[0]
    pc = agent[t0, aid, :2]
    pb = agent[t0, (aid + 1) % n, :2] if n > 1 else np.array([0.55, 0.9], f32)
    xs = np.array([pb[0], pc[0], RECT[0], FAR[0], 0.7], f32)
    ys = np.array([pb[1] if n > 1 else 0.9, pc[1], RECT[1]], f32)
    return xs, ys, dict(a=(2, 2), b=(0, 0), c=(1, 1), d=(3, 2))     # (ix, iy) of the four points


def _recorded_cost(ocfg, agent, obst, hits, t):
    return E.get_cost(ocfg, agent[t:t + 1], hits[t:t + 1] if hits is not None else (None if obst is None else obst[None]))[0]


def _strided_record(agent, hits, cuda):
    """the record as strided slices of wider NaN-filled allocations -> agent view, its frame stride, hits view, its stride"""
    Tn, n, sd = agent.shape
    wide_a = torch.full((Tn + 1, n + 2, sd), float("nan"), device=cuda)
    agd = wide_a[:Tn, 1:n + 1]
    agd.copy_(_to(agent, cuda))
    hid, h_st = None, 0
    if hits is not None:
        k = hits.shape[2]
        wide_h = torch.full((Tn, 2, n, k, 2), float("nan"), device=cuda)
        hid = wide_h[:, 1]
        hid.copy_(_to(hits, cuda))
        h_st = 2 * n * k * 2
    return agd, (n + 2) * sd, hid, h_st


def _run(cfg, rec, d_obst, rays, frame_ids, n_frames, aid, xs, ys, cuda, want_hits):
    from dgppo_amd import ops_nn as K_
    agd, a_st, hid, h_st = rec
    G = n_frames * len(ys) * len(xs)
    cost = torch.full((G, cfg.n_agents, cfg.n_cost), SENTINEL, device=cuda)
    ho = torch.full((G, cfg.top_k, 2), float("inf"), device=cuda) if want_hits else None
    K_.cost_sweep(cfg, agd, a_st, d_obst, hid, h_st, rays[0], rays[1], frame_ids, n_frames, aid,
                  K_.sweep_axis(xs, "xs", cuda), K_.sweep_axis(ys, "ys", cuda), cost, ho)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), (ho.cpu().numpy() if want_hits else None)


# ---- 1. the kernel against the oracle, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ORACLE_CASES)), ids=["-".join(map(str, c[:5])) for c in ORACLE_CASES])
def test_cost_sweep_matches_oracle(cuda, case):
    """dgppo_cost_sweep on a strided 3-frame record (a slice of a wider NaN-filled allocation), frame_ids [2, 0], agent_id 0 and
    n - 1, on the 5 x 3 grid through a rectangle / disc centre, another agent's position, the moved agent's recorded position
    and a point out of the cluster's range: cost has the oracle's bits (NaN exactly where the oracle has one), hits_out the
    oracle's hits of the moved agent.  What the grid is meant to show is asserted on the oracle's output before the GPU is used."""
    kind, n, n_obs, n_rays, top_k, random = ORACLE_CASES[case]
    cfg, ocfg, agent, obst, hits = _hand_scene(kind, n, n_obs, n_rays, top_k, random)
    frame_ids = [2, 0]
    cast = hits is not None
    want = {}
    for aid in sorted({0, n - 1}):
        xs, ys, pts = _grid(agent, frame_ids, aid, n)
        nx, ny = len(xs), len(ys)
        cost, h = _oracle_sweep(ocfg, agent, obst, hits, frame_ids, aid, xs, ys)
        assert cost.shape == (len(frame_ids) * ny * nx, n, ocfg.n_cost)
        # ---- the preconditions, on the oracle's output ----
        mine = cost[:, aid]
        assert (mine < 0).any() and (mine > 0).any(), "the swept agent's costs take both signs"
        if n > 1:
            others = [i for i in range(n) if i != aid]
            per_frame = cost.reshape(len(frame_ids), ny * nx, n, -1)[:, :, others]
            assert (per_frame != per_frame[:, :1]).any(), "the other agents' costs differ between grid points"
        for f, t in enumerate(frame_ids[:1]):                          # the grid lines run through frame_ids[0]'s positions
            g = (f * ny + pts["c"][1]) * nx + pts["c"][0]
            _same_cost(cost[g], _recorded_cost(ocfg, agent, obst, hits, t), "the cost at (c) is get_cost of the recorded frame")
        if case < NO_NAN_CASES:
            assert not np.isnan(cost).any()
        want[aid] = (xs, ys, cost, h)

    rec = _strided_record(agent, hits, cuda)
    rays = tuple(_to(x, cuda) for x in E.ray_table(n_rays)) if cast else (None, None)
    for aid, (xs, ys, cost, h) in want.items():
        got, ho = _run(cfg, rec, _to(obst, cuda), rays, frame_ids, len(frame_ids), aid, xs, ys, cuda, cast)
        if cast:
            _bits_equal(ho, h, f"hits_out, agent {aid}")
        _same_cost(got.reshape(cost.shape), cost, f"cost, agent {aid}")


# ---- 2. NaN propagation ---------------------------------------------------------------------------------------------------------
def test_nan_rays_reach_the_obstacle_component(cuda):
    """8 rays, all 8 kept: the rays parallel to the axis-aligned rectangle's edges are NaN (det == 0), so every agent's obstacle
    component is NaN at every point while the agent component stays finite — and no other word is left NaN or unwritten"""
    cfg, ocfg, agent, obst, hits = _hand_scene("LidarSpread", 3, 2, 8, 8)
    frame_ids = [2, 0]
    rec = _strided_record(agent, hits, cuda)
    rays = tuple(_to(x, cuda) for x in E.ray_table(8))
    for aid in (0, 2):
        xs, ys, _ = _grid(agent, frame_ids, aid, 3)
        cost, h = _oracle_sweep(ocfg, agent, obst, hits, frame_ids, aid, xs, ys)
        assert cost.shape[0] == 30 and np.isnan(cost[:, :, 1]).all() and np.isfinite(cost[:, :, 0]).all()
        got, ho = _run(cfg, rec, _to(obst, cuda), rays, frame_ids, 2, aid, xs, ys, cuda, True)
        assert not (got == SENTINEL).any()
        _same_cost(got, cost, f"cost, agent {aid}")
        _same_cost(ho, h, f"hits_out, agent {aid}")


# ---- 3. tile edges -----------------------------------------------------------------------------------------------------------------
# the cast shape (LiDAR with obstacles) walks tiles of 64 points, the lane-per-point shape (MPE, or no obstacles) tiles of 256
TILE_CASES = [(("LidarSpread", 3, 2, 32, 8), 1, 1), (("LidarSpread", 3, 2, 32, 8), 13, 5), (("LidarSpread", 3, 2, 32, 8), 64, 2),
              (("MPESpread", 3, 3, 0, 0), 257, 1), (("MPEConnectSpread", 4, 1, 0, 0), 64, 8), (("LidarSpread", 3, 0, 32, 8), 257, 1)]


@pytest.mark.parametrize("scene,nx,ny", TILE_CASES, ids=[f"{c[0][0]}-obs{c[0][2]}-{c[1]}x{c[2]}" for c in TILE_CASES])
def test_tile_edges(cuda, scene, nx, ny):
    """cast shape: a single point, 65 points (one tile of 64 and one point) and two full tiles per frame; lane shape: 257
    points (one tile of 256 and one point) and two full tiles — frame_ids = None over 3 frames"""
    cfg, ocfg, agent, obst, hits = _hand_scene(*scene)
    n, sd, k = ocfg.n_agents, ocfg.state_dim, ocfg.top_k
    cast = hits is not None
    xs = np.linspace(0.05, 1.45, nx).astype(f32) if nx > 1 else np.array([0.37], f32)
    ys = np.linspace(0.1, 1.4, ny).astype(f32) if ny > 1 else np.array([0.12], f32)   # through the cluster
    cost, h = _oracle_sweep(ocfg, agent, obst, hits, [0, 1, 2], 1, xs, ys)
    rec = (_to(agent, cuda), n * sd, _to(hits, cuda), n * k * 2)
    rays = tuple(_to(x, cuda) for x in E.ray_table(32)) if cast else (None, None)
    got, ho = _run(cfg, rec, _to(obst, cuda), rays, None, 3, 1, xs, ys, cuda, cast)
    assert not (got == SENTINEL).any()
    _same_cost(got, cost, "cost")
    if cast:
        _bits_equal(ho, h, "hits_out")


# ---- 4. Engine.cost_landscape on a real rollout ------------------------------------------------------------------------------------
def _engine(kind_name, n, n_obs, T_, cuda, area=None, algo="dgppo", use_rnn=True):
    from dgppo_amd import _native as N, engine as EN, init
    from oracle import nn_torch as T
    cfg = N.make_env_cfg(N.ENV_KINDS[kind_name], n, n_obs, **({} if area is None else dict(area_size=area)))
    nc = 1 if use_rnn else 0
    hp = EN.Hyper(batch_size=1024, rnn_step=2, train_steps=100, use_rnn=use_rnn, rnn_layers=1, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo=algo)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=nc)}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    trees = {k_: jitter(v) for k_, v in trees.items()}
    for k_, net in eng.nets.items():
        net.load_tree(trees[k_])
    eng.set_entropy_noise(77)
    return cfg, eng


def _anchor(eng, cfg, ro, e, aid, t):
    """a 2 x 2 grid whose lines run through the recorded positions of agent `aid` (at ix, iy = 0, 1) and of the next agent (at
    1, 0) in frame t: the first slice has the bits of the cost the rollout recorded for (e, t) — lidar_sense is a pure function —
    and standing on another agent is a collision, which the recorded frame (reset keeps agents apart) is not.  The two mixed
    points carry no such guarantee: away from everything both components sit at the lower clip."""
    n = cfg.n_agents
    p, q = (ro.agent[e, t, i, :2].cpu().numpy() for i in (aid, (aid + 1) % n))
    got = eng.cost_landscape(ro, e, aid, [t], np.array([p[0], q[0]], f32), np.array([q[1], p[1]], f32))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 2, 2, n, cfg.n_cost)
    assert torch.equal(got[0, 1, 0].view(torch.int32), ro.costs[e, t].view(torch.int32)), "the recorded position vs ro.costs"
    assert float(got[0, 0, 1, aid, 0]) > 0.0 and float(ro.costs[e, t, aid, 0]) < 0.0
    assert not torch.equal(got[0, 0, 1], got[0, 1, 0])
    return got


ANCHOR_CASES = [("LidarSpread", 3, 2, 6, None, True), ("MPEConnectSpread", 4, 1, 6, None, True), ("LidarSpread", 24, 3, 3, 4.0, True),
                ("LidarSpread", 3, 2, 6, None, False)]


@pytest.mark.parametrize("kind,n,n_obs,T_,area,use_rnn", ANCHOR_CASES,
                         ids=["-".join(map(str, c[:4])) + ("" if c[5] else "-no-rnn") for c in ANCHOR_CASES])
def test_engine_cost_landscape_anchor(cuda, kind, n, n_obs, T_, area, use_rnn):
    cfg, eng = _engine(kind, n, n_obs, T_, cuda, area, use_rnn=use_rnn)
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), False).finalize()
    for e, aid, t in ((1, n - 1, T_ - 1), (0, 0, 1)):
        _anchor(eng, cfg, ro, e, aid, t)


@pytest.mark.parametrize("algo", ["informarl", "hcbfcrpo"])
def test_engine_cost_landscape_other_algorithms(cuda, algo):
    """no refusal for the algorithms without a sweepable Vh net; with the same policy the deterministic record, and with it
    every value, is DGPPO's"""
    seeds = torch.tensor([9, 10], dtype=torch.int64, device=cuda)
    cfg, ref = _engine("LidarSpread", 3, 2, 6, cuda)
    ro_ref = ref.rollout(seeds, False).finalize()
    want = _anchor(ref, cfg, ro_ref, 1, 2, 4).clone()
    cfg, eng = _engine("LidarSpread", 3, 2, 6, cuda, algo=algo)
    assert "Vh" not in eng.nets
    ro = eng.rollout(seeds, False).finalize()
    assert torch.equal(ro.agent, ro_ref.agent), "the same policy and seeds give the same deterministic record"
    got = _anchor(eng, cfg, ro, 1, 2, 4)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_vmas_kind_is_refused_through_ctypes():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    z, null = C.c_int64(0), None
    rc = lib.dgppo_cost_sweep(C.byref(cfg), null, z, null, null, z, null, null, null, C.c_int32(1), C.c_int32(0), null,
                              C.c_int32(1), null, C.c_int32(1), null, null, null)
    assert rc != 0
    assert b"dgppo_cost_sweep" in lib.dgppo_last_error()


def test_bad_arguments_raise_before_any_launch(cuda):
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent, obst, hits = _hand_scene("LidarSpread", 3, 2, 32, 8)
    n, sd, k = 3, 4, 8
    rc, rs = (_to(x, cuda) for x in E.ray_table(32))
    d = dict(agent=_to(agent, cuda), obst=_to(obst, cuda), hits=_to(hits, cuda))
    xs, ys = K_.sweep_axis([0.2, 0.4], "xs", cuda), K_.sweep_axis([0.3], "ys", cuda)
    outs = [torch.full((2, n, 2), SENTINEL, device=cuda), torch.full((2, k, 2), SENTINEL, device=cuda)]

    def call(aid=0, xs=xs, ys=ys):
        K_.cost_sweep(cfg, d["agent"], n * sd, d["obst"], d["hits"], n * k * 2, rc, rs, [1], 1, aid, xs, ys, outs[0], outs[1])
    with pytest.raises(ValueError, match="agent_id"):
        call(aid=n)
    with pytest.raises(ValueError, match="finite"):
        K_.sweep_axis([0.2, float("nan")], "xs", cuda)
    with pytest.raises(ValueError, match="non-empty"):
        K_.sweep_axis([], "ys", cuda)
    with pytest.raises(ValueError, match="empty"):
        call(ys=torch.empty(0, device=cuda))
    mcfg, _, magent, mobst, _ = _hand_scene("MPESpread", 3, 3, 0, 0)
    with pytest.raises(ValueError, match="hits_out"):                  # nothing is cast in an MPE kind
        K_.cost_sweep(mcfg, _to(magent, cuda), n * sd, _to(mobst, cuda), None, 0, None, None, [1], 1, 0, xs, ys, outs[0], outs[1])
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs), "a refused call wrote to its outputs"
    call()
    torch.cuda.synchronize()
    assert not any(bool((o == SENTINEL).any()) for o in outs)


def test_engine_refusals(cuda):
    from dgppo_amd import _native as N, engine as EN
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        vmas.cost_landscape(None, 0, 0, [0], [0.5], [0.5])
    cfg, eng = _engine("LidarSpread", 3, 2, 4, cuda)
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), False).finalize()
    for kw, match in ((dict(env_index=2), "env_index"), (dict(agent_id=3), "agent_id"), (dict(frame_ids=[4]), "frame_ids"),
                      (dict(frame_ids=[]), "frame_ids"), (dict(xs=[]), "xs"), (dict(ys=[0.5, float("inf")]), "ys")):
        args = dict(env_index=0, agent_id=0, frame_ids=[0], xs=[0.5], ys=[0.5])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            eng.cost_landscape(ro, **args)


# ---- 6. test.py --cost-landscape, in-process -------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _checkpoint(tmp_path, algo_name, n, Tn):
    import yaml
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    conf = dict(env="LidarSpread", num_agents=n, obs=2, algo=algo_name, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, seed=3, use_rnn=True, rnn_layers=1, use_lstm=False)

    def build():
        env = make_env(env_id=conf["env"], num_agents=n, num_obs=conf["obs"], max_step=Tn)
        algo = make_algo(algo=algo_name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=n, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                         Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, max_grad_norm=2.0, seed=3, use_rnn=True, rnn_layers=1,
                         use_lstm=False)
        return env, algo
    env, algo = build()
    run = tmp_path / f"run_{algo_name}"
    algo.save(str(run / "models"), 0)
    with open(run / "config.yaml", "w") as f:
        yaml.safe_dump(conf, f)
    return run, build


def test_cli_writes_both_landscapes(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    n, grid, Tn = 3, 6, 6
    run, build = _checkpoint(tmp_path, "dgppo", n, Tn)
    _load_test_py().main(["--path", str(run), "--landscape", "1", "--cost-landscape", "1", "--landscape-grid", str(grid),
                          "--epi", "2", "--max-step", str(Tn), "--dpi", "30"])
    printed = capsys.readouterr().out
    assert printed.count("missed_frac") == 2 and printed.count("conservative_frac") == 2
    vdir = run / "videos" / "0"
    lands, costs = sorted(glob.glob(str(vdir / "*_landscape.npz"))), sorted(glob.glob(str(vdir / "*_cost.npz")))
    assert len(lands) == 2 and len(costs) == 2
    videos = [p for p in glob.glob(str(vdir / "*")) if p.endswith((".gif", ".mp4"))]
    assert len(videos) == 2 and all(os.path.getsize(p) > 1000 for p in videos)
    env2, algo2 = build()                                       # the same episodes again, from the checkpoint
    algo2.load(str(run / "models"), 0)
    keys = np.random.default_rng([1234, 13]).integers(1, 2 ** 62, size=1000)[:2]
    ro = algo2.collect_deterministic(keys, env=env2)
    for i in range(2):
        zl, zc = np.load(lands[i]), np.load(costs[i])
        assert sorted(zl.files) == ["Vh", "agent", "frames", "xs", "ys"]
        assert zc["cost"].shape == (Tn, grid, grid, n, 2) and int(zc["agent"]) == 1
        cost = algo2.cost_landscape(ro, i, 1, nx=grid, ny=grid)
        np.testing.assert_array_equal(zc["xs"], np.linspace(0.0, env2.area_size, grid).astype(f32))
        np.testing.assert_array_equal(zc["ys"], zc["xs"])
        np.testing.assert_array_equal(zc["frames"], np.arange(Tn))
        np.testing.assert_array_equal(zc["cost"], cost.cost)
        agree = EV.landscape_agreement(algo2.vh_landscape(ro, i, 1, nx=grid, ny=grid), cost)
        assert sorted(zc.files) == sorted(["xs", "ys", "cost", "agent", "frames", *agree])
        for key, v in agree.items():
            np.testing.assert_array_equal(zc[key], v)
        assert (agree["points"] + agree["nan"]).tolist() == [grid * grid] * Tn


def test_cli_cost_landscape_without_a_vh_net(cuda, tmp_path):
    n, grid, Tn = 3, 6, 6
    run, build = _checkpoint(tmp_path, "informarl", n, Tn)
    mod = _load_test_py()
    common = ["--path", str(run), "--landscape-grid", str(grid), "--epi", "2", "--max-step", str(Tn), "--no-video"]
    mod.main(common + ["--cost-landscape", "0"])
    vdir = run / "videos" / "0"
    costs = sorted(glob.glob(str(vdir / "*_cost.npz")))
    assert len(costs) == 2 and not glob.glob(str(vdir / "*_landscape.npz"))
    assert not [p for p in glob.glob(str(vdir / "*")) if p.endswith((".gif", ".mp4"))]
    for path in costs:
        z = np.load(path)
        assert sorted(z.files) == ["agent", "cost", "frames", "xs", "ys"]
        assert z["cost"].shape == (Tn, grid, grid, n, 2) and int(z["agent"]) == 0
    with pytest.raises(ValueError, match="informarl"):
        mod.main(common + ["--landscape", "0"])
