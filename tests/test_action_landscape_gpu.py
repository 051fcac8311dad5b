"""CBF action landscape: dgppo_graph_feats_action_sweep (the graph after the step with one agent's action swept over a grid)
against the oracle's clip_action + agent_step_euler + get_graph, against the step kernel's own bits and against the composition
of the existing entry points; Engine.action_landscape against values_prepass and the oracle's value_Vh; the refusals; and
test.py --action-landscape in-process."""
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
TILE = 64                               # grid points per workgroup of the kernel (ops_nn.ACTION_SWEEP_TILE)


def _to(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits_equal(got, want, name):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}"


def _same_words(got, want, name):
    """the cap is 0 differing words"""
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, f"{name}: {bad} of {got.numel()} words differ"


def _edge_of_slot(cfg):
    """[n, S] index into the oracle graph's edge list of slot s of agent i: E.get_graph lays its edges out as the agent-agent
    block (receiver-major), the agent-goal block, the agent-obstacle block"""
    n, gs, os_ = cfg.n_agents, cfg.goal_slots, cfg.obs_slots
    i = np.arange(n)[:, None]
    return np.concatenate([i * n + np.arange(n)[None], n * n + i * gs + np.arange(gs)[None],
                           n * n + n * gs + i * os_ + np.arange(os_)[None]], axis=1)


def _cfgs(kind_name, n, n_obs, area=None):
    from dgppo_amd import _native as N
    kind = N.ENV_KINDS[kind_name]
    kw = {} if area is None else dict(area_size=area)
    cfg = N.make_env_cfg(kind, n, n_obs, **kw)
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs, **kw)
    assert (cfg.n_obs, cfg.n_goals, cfg.num_nodes, cfg.num_edges) == (ocfg.n_obs, ocfg.n_goals, ocfg.num_nodes, ocfg.num_edges)
    return cfg, ocfg


# ---- 1. the features against the oracle ---------------------------------------------------------------------------------------------
US = np.array([0.0, -1.0, 1.0, 3.0], f32)           # (us[iu], vs[iv]): (0, 0), the four corners, and (3, -2) outside the box
VS = np.array([0.0, -1.0, 1.0, -2.0], f32)
ORACLE_CASES = [("LidarSpread", 3, 2, None), ("LidarTarget", 3, 2, None), ("LidarLine", 4, 2, None), ("MPESpread", 3, 3, None),
                ("MPEConnectSpread", 4, 1, None), ("LidarSpread", 3, 0, None), ("LidarSpread", 24, 3, 4.0),
                ("LidarSpread", 64, 3, 4.0), ("LidarBicycleTarget", 3, 2, None)]


@functools.lru_cache(maxsize=None)
def _hand_scene(kind_name, n, n_obs, area):
    """a 3-frame record of one env built by hand (read-only): the agents on a lattice of pitch 0.3 (neighbours hear each other,
    second neighbours do not) that drifts from frame to frame, rectangles / discs beside it.  In frame 1 the first and the last
    agent already move at the velocity limit (+limit, -limit; bicycle: speed 0.5), so that a full action makes the clamp fire;
    in MPEConnectSpread the last agent stands above y = area there (its y limit is 2 * area)."""
    cfg, ocfg = _cfgs(kind_name, n, n_obs, area)
    sd, Tn = ocfg.state_dim, 3
    rng = np.random.default_rng(5)
    side = int(np.ceil(np.sqrt(n)))
    agent = np.zeros((Tn, n, sd), f32)
    for t in range(Tn):
        for i in range(n):
            agent[t, i, 0] = f32(0.1 + 0.3 * (i % side) + 0.01 * t)
            agent[t, i, 1] = f32(0.1 + 0.3 * (i // side) + 0.005 * t)
    if ocfg.is_bicycle:
        th = rng.uniform(-np.pi, np.pi, size=(Tn, n))
        agent[..., 2], agent[..., 3] = np.cos(th).astype(f32), np.sin(th).astype(f32)
        agent[..., 4] = rng.uniform(-0.4, 0.4, size=(Tn, n)).astype(f32)
        agent[1, [0, n - 1], 4] = f32(0.5)
    else:
        vl = f32(ocfg.vel_limit)
        agent[..., 2:4] = (rng.uniform(-0.8, 0.8, size=(Tn, n, 2)) * vl).astype(f32)
        agent[1, [0, n - 1], 2], agent[1, [0, n - 1], 3] = vl, -vl
    if kind_name == "MPEConnectSpread":
        agent[1, n - 1, 1] = f32(1.5 * ocfg.area_size)
    goal = np.zeros((ocfg.n_goals, sd), f32)
    goal[:, :2] = rng.uniform(0.2, 1.3, size=(ocfg.n_goals, 2)).astype(f32)
    if ocfg.is_bicycle:
        goal[:, 2] = 1.0
    obst = hits = None
    no = ocfg.n_obs
    if no > 0 and ocfg.is_lidar:
        centres = np.array([(1.0, 1.2), (0.45, 0.5), (0.8, 0.3)][:no], f32)
        obst = E.make_rect(centres, np.array([0.3, 0.2, 0.1][:no], f32), np.array([0.2, 0.2, 0.3][:no], f32),
                           np.array([0.3, 0.0, 1.1][:no], f32))
        hits = E.lidar_sense(ocfg, agent[..., :2], np.broadcast_to(obst, (Tn,) + obst.shape), *E.ray_table(ocfg.n_rays))[0]
    elif no > 0:
        obst = np.zeros((no, sd), f32)
        obst[:, :2] = np.array([(1.0, 1.2), (0.3, 0.45), (0.8, 0.3)][:no], f32)
    for a in (agent, goal, obst, hits):
        if a is not None:
            a.setflags(write=False)
    return cfg, ocfg, agent, goal, obst, hits


def _oracle_sweep(ocfg, agent, goal, obst, hits, frame_ids, aid, us, vs):
    """the G = F * nv * nu what-if graphs on the CPU: frame t + 1 with row `aid` replaced by
    agent_step_euler(row aid of frame t, clip_action((us[iu], vs[iv]))) and the recorded hits of frame t + 1 -> get_graph"""
    F, nv, nu, n = len(frame_ids), len(vs), len(us), ocfg.n_agents
    nxt = np.asarray(frame_ids) + 1
    act = np.stack(np.meshgrid(us, vs), axis=-1).reshape(nv * nu, 1, 2)                      # [..., 0] = us[iu], [..., 1] = vs[iv]
    ag = np.repeat(agent[nxt], nv * nu, axis=0).reshape(F, nv * nu, n, -1).copy()
    for f, t in enumerate(frame_ids):
        row = np.ascontiguousarray(np.broadcast_to(agent[t, aid], (nv * nu, 1, agent.shape[-1])))
        ag[f, :, aid] = E.agent_step_euler(ocfg, row, E.clip_action(act))[:, 0]
    ag = ag.reshape(F * nv * nu, n, -1)
    G = ag.shape[0]
    tile = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (G,) + a.shape))
    h = None if hits is None else np.repeat(hits[nxt], nv * nu, axis=0)
    return ag, E.get_graph(ocfg, ag, tile(goal), tile(obst), h)


@pytest.mark.parametrize("kind,n,n_obs,area", ORACLE_CASES, ids=["-".join(map(str, c[:3])) for c in ORACLE_CASES])
def test_action_sweep_matches_oracle(cuda, kind, n, n_obs, area):
    """dgppo_graph_feats_action_sweep on a strided 3-frame record (a slice of a wider NaN-filled allocation), frame_ids [1, 0],
    agent_id 0 and n - 1, Fp = node_dim and 8: emask equals "the oracle edge is not routed to the pad node", efeat is bit-equal
    on unmasked slots, Xa / Xo bit-equal to the oracle's node rows zero padded.  The action (3, -2) gives the words of (1, -1).
    LidarBicycleTarget: masks equal, node rows and unmasked edge features within 1e-6 — the bound of
    tests/test_env_gpu.py::test_bicycle_dynamics_tolerance_then_exact_sensing for the device's atan2f / cosf / sinf against
    numpy's."""
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits = _hand_scene(kind, n, n_obs, area)
    frame_ids = [1, 0]
    sd, k, S, Tn = ocfg.state_dim, ocfg.top_k, cfg.fan_in, 3
    n_other, pad = cfg.num_nodes - 1 - n, cfg.num_nodes - 1
    nu, nv = len(US), len(VS)
    G = len(frame_ids) * nv * nu
    eos = _edge_of_slot(cfg)
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread).numpy()
    want = {}
    for aid in sorted({0, n - 1}):
        ag, gr = _oracle_sweep(ocfg, agent, goal, obst, hits, frame_ids, aid, US, VS)
        recv, send, edges = gr["receivers"][:, eos], gr["senders"][:, eos], gr["edges"][:, eos]       # [G, n, S(, 4)]
        on = recv != pad
        assert (recv[on] == np.broadcast_to(np.arange(n)[:, None], recv.shape)[on]).all()
        assert (send[on] == np.broadcast_to(snd, send.shape)[on]).all() and ((send == pad) == ~on).all()
        # ---- the preconditions, on the oracle's output ----
        rows = ag.reshape(len(frame_ids), nv, nu, n, sd)[:, :, :, aid]
        if ocfg.is_bicycle:
            assert (rows[0, 2, :, 4] == f32(0.5)).all() and (rows[0, 1, :, 4] < f32(0.5)).all(), "the speed clamp fires for v = +1"
        else:
            vl = f32(ocfg.vel_limit)
            assert (rows[0, :, 2, 2] == vl).all() and (rows[0, 1, :, 3] == -vl).all(), "the velocity clamp fires in frame 1"
            assert agent[1, aid, 2] + f32(10.0) * f32(ocfg.dt) > vl and (rows[0, :, 1, 2] < vl).all()
        if kind == "MPEConnectSpread" and aid == n - 1:
            assert (rows[0, ..., 1] > f32(ocfg.area_size)).all(), "y may pass area_size: the limit is 2 * area_size"
        assert not (rows[:, 0, 0] == rows[:, 2, 2]).all(), "different actions give different rows"
        if n > 1:
            others = [i for i in range(n) if i != aid]
            assert on[:, aid][:, others].any() and (n <= 4 or not on[:, aid][:, others].all())
        want[aid] = (on, edges, gr["nodes"])

    d_goal, d_obst = _to(goal, cuda), _to(obst, cuda)
    wide_a = torch.full((Tn + 1, n + 2, sd), float("nan"), device=cuda)
    agd = wide_a[:Tn, 1:n + 1]
    agd.copy_(_to(agent, cuda))
    a_st = (n + 2) * sd
    hid, h_st = None, 0
    if hits is not None:
        wide_h = torch.full((Tn, 2, n, k, 2), float("nan"), device=cuda)
        hid = wide_h[:, 1]
        hid.copy_(_to(hits, cuda))
        h_st = 2 * n * k * 2
    dus, dvs = K_.sweep_axis(US, "us", cuda), K_.sweep_axis(VS, "vs", cuda)
    for aid, (on, edges, nodes) in want.items():
        for Fp in (cfg.node_dim, 8):
            Xa = torch.full((G * n, Fp), float("nan"), device=cuda)
            Xo = torch.full((G * n_other, Fp), float("nan"), device=cuda)
            ef = torch.full((G * n, S, 4), float("nan"), device=cuda)
            em = torch.full((G * n, S), float("nan"), device=cuda)
            K_.graph_feats_action_sweep(cfg, agd, a_st, d_goal, d_obst, hid, h_st, frame_ids, len(frame_ids), aid, dus, dvs,
                                        Xa, Xo if n_other > 0 else None, ef, em, Fp)
            torch.cuda.synchronize()
            tag = f"agent {aid} Fp={Fp}"
            got_em = em.cpu().numpy().reshape(G, n, S)
            got_ef = ef.cpu().numpy().reshape(G, n, S, 4)
            got_xa = Xa.cpu().numpy().reshape(G, n, Fp)
            rows = np.zeros((G, cfg.num_nodes - 1, Fp), f32)
            rows[..., :cfg.node_dim] = nodes[:, :pad]
            np.testing.assert_array_equal(got_em, on.astype(f32), err_msg=f"emask {tag}")
            if ocfg.is_bicycle:
                for name, got, exp in (("efeat", got_ef[on], edges[on]), ("Xa", got_xa, rows[:, :n])):
                    err = float(np.abs(got.astype(np.float64) - exp).max())
                    print(f"{kind} {name} {tag}: max abs err {err:.3e}")
                    np.testing.assert_allclose(got, exp, atol=1e-6, rtol=0, err_msg=f"{name} {tag}")
            else:
                _bits_equal(got_ef[on], np.ascontiguousarray(edges[on]), f"efeat {tag}")
                _bits_equal(got_xa, rows[:, :n], f"Xa {tag}")
            if n_other > 0:
                _bits_equal(Xo.cpu().numpy().reshape(G, n_other, Fp), rows[:, n:], f"Xo {tag}")
            # (3, -2) is clipped to (1, -1): point (iv, iu) = (3, 3) against (1, 2), in every word of every output
            for name, arr in (("Xa", Xa), ("Xo", Xo), ("efeat", ef), ("emask", em)):
                if arr.numel():
                    v = arr.view(len(frame_ids), nv, nu, -1)
                    _same_words(v[:, 3, 3], v[:, 1, 2], f"{name} {tag}: (3, -2) vs (1, -1)")


@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 3, 2), ("MPESpread", 3, 3)])
def test_action_sweep_keeps_a_nan_action(cuda, kind, n, n_obs):
    """a NaN grid value stays NaN through the sweep's clip_action, as in the oracle's (jnp.clip; fminf / fmaxf would turn it into
    the action -1): NaN in the swept agent's velocity columns and in the edge features that subtract them, at exactly the
    oracle's places, every other word bit-equal.  sweep_axis refuses non-finite coordinates, so the axes are handed to the
    binding as plain device tensors."""
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits = _hand_scene(kind, n, n_obs, None)
    frame_ids, aid, Fp = [1, 0], n - 1, 8
    us, vs = np.array([0.0, np.nan, 1.0], f32), np.array([np.nan, 0.5], f32)
    nu, nv, S, pad = len(us), len(vs), cfg.fan_in, cfg.num_nodes - 1
    G, n_other = len(frame_ids) * nv * nu, cfg.num_nodes - 1 - n
    ag, gr = _oracle_sweep(ocfg, agent, goal, obst, hits, frame_ids, aid, us, vs)
    eos = _edge_of_slot(cfg)
    on, edges = gr["receivers"][:, eos] != pad, gr["edges"][:, eos]
    rows = np.zeros((G, pad, Fp), f32)
    rows[..., :cfg.node_dim] = gr["nodes"][:, :pad]
    swept = rows.reshape(len(frame_ids), nv, nu, pad, Fp)[:, :, :, aid]
    assert np.isnan(swept[:, :, 1, 2]).all() and np.isnan(swept[:, 0, :, 3]).all() and np.isfinite(swept[:, 1, 0]).all()
    assert np.isfinite(swept[..., :2]).all() and np.isnan(edges[on]).any()

    def same(got, want, name):
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaN positions")
        _bits_equal(np.where(nan, f32(0), got), np.where(nan, f32(0), want), name)

    Xa = torch.full((G * n, Fp), float("nan"), device=cuda)
    Xo = torch.full((G * n_other, Fp), float("nan"), device=cuda)
    ef = torch.full((G * n, S, 4), float("nan"), device=cuda)
    em = torch.full((G * n, S), float("nan"), device=cuda)
    k = ocfg.top_k
    K_.graph_feats_action_sweep(cfg, _to(agent, cuda), n * ocfg.state_dim, _to(goal, cuda), _to(obst, cuda), _to(hits, cuda),
                                0 if hits is None else n * k * 2, frame_ids, len(frame_ids), aid, _to(us, cuda), _to(vs, cuda),
                                Xa, Xo, ef, em, Fp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(em.cpu().numpy().reshape(G, n, S), on.astype(f32), err_msg="emask")
    same(ef.cpu().numpy().reshape(G, n, S, 4)[on], np.ascontiguousarray(edges[on]), "efeat")
    same(Xa.cpu().numpy().reshape(G, n, Fp), rows[:, :n], "Xa")
    same(Xo.cpu().numpy().reshape(G, n_other, Fp), rows[:, n:], "Xo")


# ---- 2. - 4. against the step kernel and the composition of the existing entry points -----------------------------------------------
def _stepped(cfg, cuda, aid, acts, seed=4242):
    """P copies of one env (same seed), stepped once by ops_env.step with the same actions for everyone but agent `aid`, who
    takes acts[p] in copy p -> (state before, state after, the 2-frame record of copy 0 as the sweep reads it)"""
    from dgppo_amd import ops_env as OE
    n, P = cfg.n_agents, len(acts)
    st0 = OE.State.empty(cfg, P, cuda)
    OE.reset(cfg, torch.full((P,), seed, dtype=torch.int64, device=cuda), st0)
    st1 = st0.like()
    gen = torch.Generator().manual_seed(3)
    act = (torch.rand(1, n, 2, generator=gen) * 2 - 1).expand(P, n, 2).clone()
    act[:, aid] = torch.from_numpy(np.ascontiguousarray(acts, f32))
    OE.step(cfg, st0, act.to(cuda), st1, torch.empty(P, device=cuda), torch.empty(P, n, cfg.n_cost, device=cuda))
    has_hits = cfg.is_lidar and cfg.n_obs > 0
    rec = dict(agent=torch.stack([st0.agent[0], st1.agent[0]]).contiguous(),
               hits=torch.stack([st0.hits[0], st1.hits[0]]).contiguous() if has_hits else None,
               goal=st0.goal[0].contiguous(), obst=st0.obst[0].contiguous() if cfg.n_obs > 0 else None)
    return st0, st1, rec


def _outs(cfg, G, cuda, Fp):
    n, S, n_other = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1 - cfg.n_agents
    return dict(Xa=torch.full((G * n, Fp), float("nan"), device=cuda), Xo=torch.full((G * n_other, Fp), float("nan"), device=cuda),
                ef=torch.full((G * n, S, 4), float("nan"), device=cuda), em=torch.full((G * n, S), float("nan"), device=cuda))


def _sweep(cfg, rec, aid, us, vs, cuda, frames=(0,)):
    from dgppo_amd import nets, ops_nn as K_
    n, sd, k = cfg.n_agents, cfg.state_dim, cfg.top_k
    Fp = nets.input_width(cfg)
    out = _outs(cfg, len(frames) * len(vs) * len(us), cuda, Fp)
    K_.graph_feats_action_sweep(cfg, rec["agent"], n * sd, rec["goal"], rec["obst"], rec["hits"], n * k * 2, list(frames),
                                len(frames), aid, K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda), out["Xa"],
                                out["Xo"] if out["Xo"].numel() else None, out["ef"], out["em"], Fp)
    torch.cuda.synchronize()
    return out


def _graph_feats(cfg, agent, hits, goal, obst, cuda):
    """dgppo_graph_feats of G dense states [G, n, sd] of one env"""
    from dgppo_amd import nets, ops_nn as K_
    n, sd, k = cfg.n_agents, cfg.state_dim, cfg.top_k
    G, Fp = agent.shape[0], nets.input_width(cfg)
    out = _outs(cfg, G, cuda, Fp)
    tile = lambda a: None if a is None else a.unsqueeze(0).expand(G, *a.shape).contiguous()
    K_.graph_feats(cfg, agent, n * sd, 0, tile(goal), tile(obst), hits, n * k * 2, 0, None, G, 1, out["Xa"],
                   out["Xo"] if out["Xo"].numel() else None, out["ef"], out["em"], Fp)
    torch.cuda.synchronize()
    return out


def _grid_acts(us, vs):
    return np.stack(np.meshgrid(us, vs), axis=-1).reshape(-1, 2).astype(f32)             # q = iv * nu + iu -> (us[iu], vs[iv])


STEP_CASES = [("LidarSpread", 8, 3), ("LidarBicycleTarget", 4, 3), ("MPESpread", 3, 3), ("MPEConnectSpread", 4, 1)]


@pytest.mark.parametrize("kind,n,n_obs", STEP_CASES, ids=["-".join(map(str, c)) for c in STEP_CASES])
def test_swept_row_has_the_step_kernels_bits(cuda, kind, n, n_obs):
    """for every grid action, columns < state_dim of the swept agent's Xa row are row `agent` of ops_env.step's next_agent for
    that action, bit for bit (the bicycle too: the same device code), and so are the position columns of the record"""
    cfg, _ = _cfgs(kind, n, n_obs)
    sd = cfg.state_dim
    us, vs = np.array([0.0, -1.0, 1.0, 3.0, 0.37], f32), np.array([0.0, -1.0, 1.0, -2.0, -0.61], f32)
    for aid in sorted({0, n - 1}):
        _, st1, rec = _stepped(cfg, cuda, aid, _grid_acts(us, vs))
        got = _sweep(cfg, rec, aid, us, vs, cuda)
        row = got["Xa"].view(len(vs) * len(us), n, -1)[:, aid, :sd]
        _same_words(row, st1.agent[:, aid], f"{kind} agent {aid}: swept row vs ops_env.step")
        distinct = {tuple(r) for r in np.ascontiguousarray(row.cpu().numpy()).view(np.uint32).tolist()}
        assert len(distinct) >= 4, "the actions give different rows"      # a bicycle at rest turns for no u: 4 speeds at least
        _same_words(row[:, :2], rec["agent"][1, aid, :2].expand(row.shape[0], 2), "the next position does not depend on the action")


@pytest.mark.parametrize("kind,n,n_obs", STEP_CASES, ids=["-".join(map(str, c)) for c in STEP_CASES])
def test_recorded_action_reproduces_the_record(cuda, kind, n, n_obs):
    """with us[0], vs[0] the recorded action of (t, agent), all four outputs at that point equal dgppo_graph_feats of frame
    t + 1 in every word; a point with another action differs in the agent's row"""
    cfg, _ = _cfgs(kind, n, n_obs)
    aid = n // 2
    taken = np.array([[0.43, -0.81]], f32)
    _, _, rec = _stepped(cfg, cuda, aid, taken)
    us, vs = np.array([taken[0, 0], -0.2], f32), np.array([taken[0, 1], 0.6, 1.0], f32)
    got = _sweep(cfg, rec, aid, us, vs, cuda)
    want = _graph_feats(cfg, rec["agent"][1:2], None if rec["hits"] is None else rec["hits"][1:2], rec["goal"], rec["obst"], cuda)
    P = len(us) * len(vs)
    for key in want:
        if want[key].numel():
            _same_words(got[key].view(P, -1)[0], want[key].view(-1), f"{kind} {key} at the recorded action")
    assert (got["em"] == 0).any() and (got["em"] == 1).any()
    rows = got["Xa"].view(P, n, -1)
    others = [i for i in range(n) if i != aid]
    for p in range(len(us), P):                      # another v (a bicycle at rest turns for no u: rows of vs[0] may coincide)
        assert not torch.equal(rows[p, aid], rows[0, aid]), f"point {p} has the recorded row"
        assert torch.equal(rows[p, others], rows[0, others])
        assert not torch.equal(got["ef"].view(P, -1)[p], got["ef"].view(P, -1)[0])


TILE_GRIDS = [(1, 1), (TILE + 1, 1), (16, 2 * TILE // 16)]


@pytest.mark.parametrize("kind,n,n_obs,area", [("LidarSpread", 8, 3, None), ("LidarBicycleTarget", 4, 3, None),
                                               ("MPEConnectSpread", 4, 1, None), ("LidarSpread", 20, 3, 4.0)],
                         ids=["LidarSpread-8-3", "LidarBicycleTarget-4-3", "MPEConnectSpread-4-1", "LidarSpread-20-3"])
def test_tile_edges_equal_composition(cuda, kind, n, n_obs, area):
    """grids of 1 point, one more than the kernel's tile and two full tiles: every word of every output, masked slots included,
    equals the point-by-point composition — frame t + 1 tiled per point, the agent's row overwritten with ops_env.step's for
    that action, dgppo_graph_feats"""
    from dgppo_amd import ops_nn as K_
    assert K_.ACTION_SWEEP_TILE == TILE
    cfg, _ = _cfgs(kind, n, n_obs, area)
    aid = n - 1
    for nu, nv in TILE_GRIDS:
        us = np.linspace(-1.0, 1.0, nu).astype(f32) if nu > 1 else np.array([0.3], f32)
        vs = np.linspace(-1.0, 1.0, nv).astype(f32) if nv > 1 else np.array([-0.7], f32)
        P = nu * nv
        _, st1, rec = _stepped(cfg, cuda, aid, _grid_acts(us, vs))
        got = _sweep(cfg, rec, aid, us, vs, cuda)
        ag = rec["agent"][1:2].expand(P, -1, -1).clone()
        ag[:, aid] = st1.agent[:, aid]
        hits = None if rec["hits"] is None else rec["hits"][1:2].expand(P, -1, -1, -1).contiguous()
        want = _graph_feats(cfg, ag, hits, rec["goal"], rec["obst"], cuda)
        for key in want:
            _same_words(got[key], want[key], f"{kind} {key} grid {nu} x {nv}")
        assert not torch.isnan(got["Xa"]).any() and not torch.isnan(got["em"]).any()


# ---- 5. Engine.action_landscape -------------------------------------------------------------------------------------------------------
def _close(got, want, tol, name):
    """tests/test_nn_gpu.py's rule for the network outputs: `tol` of the output scale"""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})"


def _engine(kind_name, n, n_obs, T_, cuda, use_rnn=True, rnn_layers=1, area=None, algo="dgppo"):
    from dgppo_amd import engine as EN, init
    cfg, ocfg = _cfgs(kind_name, n, n_obs, area)
    nc = rnn_layers if use_rnn else 0
    hp = EN.Hyper(batch_size=1024, rnn_step=2, train_steps=100, use_rnn=use_rnn, rnn_layers=rnn_layers, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo=algo)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=min(nc, 1))}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    trees = {k_: jitter(v) for k_, v in trees.items()}
    for k_, net in eng.nets.items():
        if k_ in trees:
            net.load_tree(trees[k_])
    eng.set_entropy_noise(77)
    return cfg, ocfg, eng, trees


ENGINE_CASES = [("n3-stochastic", 3, 2, 4, None, True, 1, True), ("n3-deterministic", 3, 2, 4, None, True, 1, False),
                ("n3-no-rnn", 3, 2, 4, None, False, 1, False), ("n3-rnn-layers-2", 3, 2, 4, None, True, 2, True),
                ("n24-tiled-attention", 24, 3, 3, 4.0, True, 1, False)]


@pytest.mark.parametrize("name,n,n_obs,T_,area,use_rnn,rnn_layers,stochastic", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_action_landscape_at_the_recorded_action(cuda, name, n, n_obs, T_, area, use_rnn, rnn_layers, stochastic):
    """frames {0, T-2, T-1}, a 4 x 4 grid whose point (f, f) is the recorded action of frame f.  There Vh_next equals
    values_prepass' Vh[e, t + 1] within 1e-5 of scale (the project's network tolerance; t = T - 1 reads the final carry), Vh
    equals Vh[e, t] bit for bit, and cbf equals (Vh[t+1] - Vh[t]) / dt + alpha * Vh[t] within (2 / dt + alpha) * 1e-5 of scale:
    each of the two Vh terms of the quotient may be off by 1e-5 of scale, the alpha term uses the exact Vh[t], so the bound is
    2e-5 / dt, and alpha * 1e-5 more covers the rounding of the fp32 evaluation itself.  Another grid point gives another
    Vh_next; a prepass_graphs of 20, 5 and 3 (whole frames, rows, pieces of a row) is bit-equal to the unchunked call."""
    cfg, ocfg, eng, trees = _engine("LidarSpread", n, n_obs, T_, cuda, use_rnn, rnn_layers, area)
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), stochastic, noise_seed=5).finalize()
    Vh_pre = eng.values_prepass(ro, want_Vl=False)[1].clone()
    e, aid = 1, n - 1
    frames = sorted({0, T_ - 2, T_ - 1})
    assert len(frames) == 3
    taken = ro.actions[e, frames, aid].cpu().numpy()
    assert (np.abs(taken) <= 1.0).all()
    us, vs = np.append(taken[:, 0], f32(0.3)).astype(f32), np.append(taken[:, 1], f32(-0.7)).astype(f32)
    cbf, Vn, Vh = eng.action_landscape(ro, e, aid, frames, us, vs)
    torch.cuda.synchronize()
    nc = cfg.n_cost
    assert tuple(cbf.shape) == tuple(Vn.shape) == (3, 4, 4, n, nc) and tuple(Vh.shape) == (3, n, nc)
    again = eng.values_prepass(ro, want_Vl=False)[1]
    assert torch.equal(again.view(torch.int32), Vh_pre.view(torch.int32)), "values_prepass' own output is unchanged"
    dt, alpha = float(cfg.dt), float(eng.hp.alpha)
    for f, t in enumerate(frames):
        _close(Vn[f, f, f], Vh_pre[e, t + 1], 1e-5, f"{name}: Vh_next at the recorded action of frame {t} vs values_prepass")
        assert torch.equal(Vh[f].view(torch.int32), Vh_pre[e, t].view(torch.int32)), f"{name}: Vh of frame {t}"
        want = (Vh_pre[e, t + 1].double() - Vh_pre[e, t].double()) / dt + alpha * Vh_pre[e, t].double()
        got = cbf[f, f, f].double().cpu()
        scale = max(1.0, float(Vh_pre[e].abs().max()))
        err = float((got - want.cpu()).abs().max())
        bound = (2.0 / dt + alpha) * 1e-5 * scale
        print(f"{name}: cbf at the recorded action of frame {t}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"{name}: cbf of frame {t}: max abs err {err:.3e} > {bound:.3e}"
        assert not torch.equal(Vn[f, 3, 3], Vn[f, f, f]), "another action gives another Vh_next"
    assert bool(torch.isfinite(cbf).all())
    if n > 3:
        return
    keep = eng.prepass_graphs
    try:
        for cap in (20, 5, 3):
            eng.prepass_graphs = cap
            c2, n2, h2 = eng.action_landscape(ro, e, aid, frames, us, vs)
            for a, b, what in ((c2, cbf, "cbf"), (n2, Vn, "Vh_next"), (h2, Vh, "Vh")):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: {what} with prepass_graphs = {cap}"
    finally:
        eng.prepass_graphs = keep


# ---- 6. against the oracle's value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stochastic", [True, False], ids=["stochastic", "deterministic"])
def test_engine_action_landscape_matches_oracle_value(cuda, stochastic):
    """LidarSpread n = 3, T = 4, frames [2, 0], a 3 x 3 grid holding an action outside the box: Vh_next at every point is
    within 1e-5 of scale of value_Vh on the oracle's graph (stepped row, recorded hits of t + 1) with the carry of step t + 1"""
    T_, e, aid = 4, 0, 1
    cfg, ocfg, eng, trees = _engine("LidarSpread", 3, 2, T_, cuda)
    n = cfg.n_agents
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), stochastic, noise_seed=5).finalize()
    frames = [2, 0]
    us, vs = np.array([-1.0, 0.2, 1.7], f32), np.array([-0.4, 0.0, 1.0], f32)
    _, Vn, _ = eng.action_landscape(ro, e, aid, frames, us, vs)
    torch.cuda.synchronize()
    _, gr = _oracle_sweep(ocfg, ro.agent[e].cpu().numpy(), ro.goal[e].cpu().numpy(), ro.obst[e].cpu().numpy(),
                          ro.hits[e].cpu().numpy(), frames, aid, us, vs)
    h = ro.rnn_states[e].cpu()[[t + 1 for t in frames]][..., :64]                  # [F, n, 64]: the carry of step t + 1
    h = h[:, None].expand(-1, len(vs) * len(us), -1, -1).reshape(-1, n, 64)
    with torch.no_grad():
        want, _ = T.value_Vh(trees["Vh"], T.graph_to_torch(gr), h, n)
    _close(Vn.reshape(-1, n, cfg.n_cost), want, 1e-5, "Vh_next vs value_Vh(get_graph)")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["informarl", "hcbfcrpo", "informarl_lagr"])
def test_unsupported_algorithms_raise(cuda, algo):
    from dgppo_amd import _native as N, engine as EN
    eng = EN.Engine(N.make_env_cfg(0, 3, 2), EN.Hyper(batch_size=256), cuda, T=4, algo=algo)
    with pytest.raises(ValueError, match=f"action_landscape.*{algo}"):
        eng.action_landscape(None, 0, 0, [0], [0.5], [0.5])


def test_engine_refusals(cuda):
    from dgppo_amd import _native as N, engine as EN
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="action_landscape.*VMASReverseTransport"):
        vmas.action_landscape(None, 0, 0, [0], [0.5], [0.5])
    cfg, ocfg, eng, _ = _engine("LidarSpread", 3, 2, 4, cuda)
    ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), False).finalize()
    for kw, match in ((dict(env_index=2), "env_index"), (dict(agent_id=3), "agent_id"), (dict(frame_ids=[4]), "frame_ids"),
                      (dict(frame_ids=[-1]), "frame_ids"), (dict(frame_ids=[]), "frame_ids"), (dict(us=[]), "us"),
                      (dict(vs=[0.5, float("inf")]), "vs"), (dict(us=[float("nan")]), "us")):
        args = dict(env_index=0, agent_id=0, frame_ids=[0], us=[0.5], vs=[0.5])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            eng.action_landscape(ro, **args)


def test_bad_arguments_raise_before_any_launch(cuda):
    from dgppo_amd import _native as N, ops_nn as K_
    cfg, ocfg, agent, goal, obst, hits = _hand_scene("LidarSpread", 3, 2, None)
    n, sd, k, S, Fp = 3, 4, 8, cfg.fan_in, 8
    n_other = cfg.num_nodes - 1 - n
    d = dict(agent=_to(agent, cuda), goal=_to(goal, cuda), hits=_to(hits, cuda))
    us, vs = K_.sweep_axis([0.2, 0.4], "us", cuda), K_.sweep_axis([0.3], "vs", cuda)
    G = 2
    outs = [torch.full(s, float("nan"), device=cuda) for s in ((G * n, Fp), (G * n_other, Fp), (G * n, S, 4), (G * n, S))]

    def call(aid=0, us=us, vs=vs, frames=(1,), cfg=cfg, hits=d["hits"]):
        K_.graph_feats_action_sweep(cfg, d["agent"], n * sd, d["goal"], None, hits, n * k * 2, list(frames), len(frames), aid,
                                    us, vs, outs[0], outs[1], outs[2], outs[3], Fp)
    with pytest.raises(ValueError, match="agent_id"):
        call(aid=n)
    with pytest.raises(ValueError, match="storage"):                # frame 2 is the record's last: its successor is outside
        call(frames=(2,))
    with pytest.raises(ValueError, match="hits"):
        call(hits=None)
    with pytest.raises(ValueError, match="finite"):
        K_.sweep_axis([0.2, float("nan")], "us", cuda)
    with pytest.raises(ValueError, match="non-empty"):
        K_.sweep_axis([], "vs", cuda)
    with pytest.raises(ValueError, match="empty"):
        call(vs=torch.empty(0, device=cuda))
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        call(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), "a refused call wrote to its outputs"
    call()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o).any()) for o in outs)


# ---- 8. test.py --action-landscape, in-process ---------------------------------------------------------------------------------------------
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


def test_cli_writes_action_landscapes(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import ActionLandscape
    n, grid, Tn, alpha = 3, 4, 6, 5.0
    run = _run_dir(tmp_path, "dgppo", n, Tn, 2, alpha)
    mod = _load_test_py()
    common = ["--path", str(run), "--epi", "2", "--no-video", "--landscape-grid", str(grid), "--max-step", str(Tn)]
    mod.main(common + ["--action-landscape", "0"])
    printed = capsys.readouterr().out
    for word in ("admissible_frac", "empty_frac", "taken_admitted_frac"):
        assert printed.count(word) == 2, word
    vdir = run / "videos" / "2"
    files = sorted(glob.glob(str(vdir / "*_action.npz")))
    assert len(files) == 2 and len(glob.glob(str(vdir / "*"))) == 2
    lin = np.linspace(-1.0, 1.0, grid).astype(f32)
    for path in files:
        z = np.load(path)
        A = ActionLandscape(*(z[k] for k in ActionLandscape._fields))
        adm = EV.action_admissibility(A)
        assert sorted(z.files) == sorted([*ActionLandscape._fields, *adm])
        np.testing.assert_array_equal(z["us"], lin)
        np.testing.assert_array_equal(z["vs"], lin)
        assert z["cbf"].shape == z["Vh_next"].shape == (Tn, grid, grid, n, 2) and z["Vh"].shape == (Tn, n, 2)
        assert z["actions"].shape == (Tn, 2) and (np.abs(z["actions"]) <= 1.0).all()
        assert int(z["agent"]) == 0 and float(z["alpha"]) == alpha and float(z["dt"]) == f32(0.03)
        np.testing.assert_array_equal(z["frames"], np.arange(Tn))
        want = (z["Vh_next"] - z["Vh"][:, None, None]) / f32(z["dt"]) + f32(alpha) * z["Vh"][:, None, None]
        np.testing.assert_allclose(z["cbf"], want, rtol=1e-5, atol=1e-5)
        for key, v in adm.items():
            np.testing.assert_array_equal(z[key], v)
        assert z["points"].tolist() == [grid * grid] * Tn and (z["taken"][:-1] >= 0).all() and z["taken"][-1] == -1
    mod.main(common + ["--action-landscape", "0", "--landscape", "0", "--cost-landscape", "0"])
    for suffix in ("landscape", "cost"):
        assert len(glob.glob(str(vdir / f"*_{suffix}.npz"))) == 2, suffix
    assert len(glob.glob(str(vdir / "*_action.npz"))) in (2, 4)      # the stamp carries the minute: the first two may be rewritten
    assert not [p for p in glob.glob(str(vdir / "*")) if p.endswith((".gif", ".mp4"))]


def test_cli_refuses_an_algorithm_without_a_vh_net(cuda, tmp_path):
    run = _run_dir(tmp_path, "informarl", 3, 6, 0, 10.0)
    with pytest.raises(ValueError, match="informarl"):
        _load_test_py().main(["--path", str(run), "--epi", "2", "--no-video", "--landscape-grid", "4", "--max-step", "6",
                              "--action-landscape", "0"])
