"""dgppo_graph_feats, the wave-per-graph kernel: Xa, Xo, efeat and emask bit for bit against the oracle's graph (E.get_graph
regrouped per (agent, slot), as tests/test_large_team_kernels_gpu.py does for the large teams) at the small shapes where the
kernel's paths differ: fewer agents than one group of 8 lanes, a team that crosses it, state_dim 5, MPE obstacle rows, no
obstacle nodes at all, and a 17-agent team whose record no longer fits the registers that stage the next graph.  Each at one
graph, at five (a workgroup of four waves and the striding loop end unevenly), through record strides with n_time = 3, and
through env_ids with a repeated id — with the production row width (16-byte stores) and with Fp = node_dim."""
import functools
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
from test_env_gpu import _random_state, _to  # noqa: E402
from test_large_team_kernels_gpu import _edge_of_slot  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
B, SLOTS = 8, 4                      # the record: 8 envs x (T + 1 = 4) steps

# (kind, n, n_obs, area_size)
CASES = [("LidarSpread", 3, 2, 1.5), ("LidarSpread", 8, 3, 1.5), ("LidarTarget", 9, 3, 2.0), ("LidarBicycleTarget", 4, 3, 1.5),
         ("MPESpread", 3, 3, 1.5), ("MPETarget", 3, 0, 1.5), ("LidarSpread", 17, 3, 3.0)]
# (name, n_env, n_time, env_ids)
MODES = [("G1", 1, 1, None), ("G5", 5, 1, None), ("time3", 4, 3, None), ("ids", 6, 1, (5, 2, 7, 0, 2, 3))]


def _same(got, want, name):
    """NaN exactly where the oracle is NaN, equal bits everywhere else"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaN positions")
    bad = np.where(nan, f32(0), got).view(np.uint32) != np.where(nan, f32(0), want).view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}"


def _cfgs(kind, n, n_obs, area):
    from dgppo_amd import _native as N
    k = N.ENV_KINDS[kind]
    return N.make_env_cfg(k, n, n_obs, area_size=area), E.EnvCfg(k, n_agents=n, n_obs=n_obs, area_size=area)


def _expected(cfg, ocfg, ag, goal, obst, hi):
    """the oracle's graph of every (env, slot) of a record, regrouped per (agent, slot): on [B, SLOTS, n, S], edges
    [B, SLOTS, n, S, 4], node rows [B, SLOTS, Ns, node_dim]"""
    n = cfg.n_agents
    graphs = [E.get_graph(ocfg, ag[:, t], goal, obst, None if hi is None else hi[:, t]) for t in range(ag.shape[1])]
    gr = {key: np.stack([g[key] for g in graphs], 1) for key in ("nodes", "edges", "receivers", "senders")}
    eos, pad = _edge_of_slot(cfg), cfg.num_nodes - 1
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread).numpy()
    recv, send, edges = gr["receivers"][:, :, eos], gr["senders"][:, :, eos], gr["edges"][:, :, eos]
    on = recv != pad
    # the regrouping is pinned by the oracle itself: an unmasked edge runs from the slot's static sender to the agent
    assert (recv[on] == np.broadcast_to(np.arange(n)[:, None], recv.shape)[on]).all()
    assert (send[on] == np.broadcast_to(snd, send.shape)[on]).all() and ((send == pad) == ~on).all()
    return on, edges, gr["nodes"][:, :, :pad]


@functools.lru_cache(maxsize=None)
def _record(kind, n, n_obs, area):
    """one record per case and the oracle's graphs of all its (env, slot) pairs, shared by the modes and never written to"""
    cfg, ocfg = _cfgs(kind, n, n_obs, area)
    agent0, goal, obst, action = _random_state(ocfg, B, seed=4000 + 10 * n + n_obs)
    tab = E.ray_table(ocfg.n_rays)
    has_hits = ocfg.is_lidar and ocfg.n_obs > 0
    hits0 = E.lidar_sense(ocfg, agent0[..., :2], obst, *tab)[0] if has_hits else None
    nxt = E.env_step(ocfg, agent0, goal, obst, hits0, action, tab)["next_agent"]
    ag = np.stack([agent0, nxt, agent0, nxt], 1).copy()
    ag[:, 2, :, :2] += f32(0.03)
    ag[:, 3, :, :2] -= f32(0.02)
    hi = np.stack([E.lidar_sense(ocfg, ag[:, t, :, :2], obst, *tab)[0] for t in range(SLOTS)], 1) if has_hits else None
    on, edges, rows = _expected(cfg, ocfg, ag, goal, obst, hi)
    return cfg, ag, goal, obst, hi, on, edges, rows


def _run_and_check(cuda, cfg, ag, goal, obst, hi, on, edges, rows, modes=MODES):
    from dgppo_amd import ops_nn as K
    n, sd, k, S = cfg.n_agents, cfg.state_dim, cfg.top_k, cfg.fan_in
    n_other = cfg.num_nodes - 1 - n
    d_ag, d_goal, d_obst, d_hi = _to(ag, cuda), _to(goal, cuda), _to(obst, cuda), _to(hi, cuda)
    a_se, a_st, h_se, h_st = SLOTS * n * sd, n * sd, SLOTS * n * k * 2, n * k * 2
    for name, n_env, n_time, env_ids in modes:
        envs = np.arange(n_env) if env_ids is None else np.asarray(env_ids)
        ids = None if env_ids is None else torch.tensor(env_ids, dtype=torch.int32, device=cuda)
        G = n_env * n_time
        want_on, want_e, want_rows = on[envs, :n_time], edges[envs, :n_time], rows[envs, :n_time]
        for Fp in sorted({cfg.node_dim, 8}):
            Xa = torch.full((G * n, Fp), float("nan"), device=cuda)
            Xo = torch.full((max(G * n_other, 1), Fp), float("nan"), device=cuda)[:G * n_other]
            ef = torch.full((G * n, S, 4), float("nan"), device=cuda)
            em = torch.full((G * n, S), float("nan"), device=cuda)
            K.graph_feats(cfg, d_ag, a_se, a_st, d_goal, d_obst, d_hi, h_se if hi is not None else 0,
                          h_st if hi is not None else 0, ids, n_env, n_time, Xa, Xo if n_other > 0 else None, ef, em, Fp)
            torch.cuda.synchronize()
            tag = f"{name} Fp={Fp}"
            np.testing.assert_array_equal(em.cpu().numpy().reshape(n_env, n_time, n, S), want_on.astype(f32), err_msg=f"emask {tag}")
            ef_np = ef.cpu().numpy().reshape(n_env, n_time, n, S, 4)
            _same(ef_np[want_on], np.ascontiguousarray(want_e[want_on]), f"efeat {tag}")
            full = np.zeros((n_env, n_time, cfg.num_nodes - 1, Fp), f32)
            full[..., :cfg.node_dim] = want_rows
            _same(Xa.cpu().numpy().reshape(n_env, n_time, n, Fp), full[:, :, :n], f"Xa {tag}")
            if n_other > 0:
                _same(Xo.cpu().numpy().reshape(n_env, n_time, n_other, Fp), full[:, :, n:], f"Xo {tag}")


@pytest.mark.parametrize("kind,n,n_obs,area", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_graph_feats_wave_matches_oracle_graph(cuda, kind, n, n_obs, area):
    cfg, ag, goal, obst, hi, on, edges, rows = _record(kind, n, n_obs, area)
    assert on.any() and (~on).any(), "masks must vary in this scene, otherwise it proves little"
    _run_and_check(cuda, cfg, ag, goal, obst, hi, on, edges, rows)


def test_graph_feats_wave_nan_coordinate_and_exact_comm_radius(cuda):
    """a NaN agent coordinate leaves NaNs and closed masks exactly where the oracle has them (its agent-agent and LiDAR
    comparisons are false, its goal slots stay open with NaN features), and two agents exactly comm_radius apart are NOT
    connected (d < comm_radius) while a pair one ulp closer is"""
    cfg, ag, goal, obst, hi, _, _, _ = _record("LidarSpread", 3, 2, 1.5)
    _, ocfg = _cfgs("LidarSpread", 3, 2, 1.5)
    ag = ag.copy()
    ag[1, 0, 1, 0] = np.nan                                        # env 1, slot 0, agent 1: x
    r = f32(cfg.comm_radius)
    ag[2, :, 0, :2] = (f32(0.5), f32(0.5))                         # env 2: agents 0 and 1 exactly comm_radius apart in x ...
    ag[2, :, 1, :2] = (f32(0.5) + r, f32(0.5))
    ag[2, :, 2, :2] = (np.nextafter(f32(0.5) + r, f32(0)), f32(0.75))   # ... agent 2 far enough in y to matter little
    ag[3, :, 0, :2] = (f32(0.5), f32(0.5))                         # env 3: one ulp closer
    ag[3, :, 1, :2] = (np.nextafter(f32(0.5) + r, f32(0)), f32(0.5))
    assert f32(ag[2, 0, 1, 0] - ag[2, 0, 0, 0]) == r
    on, edges, rows = _expected(cfg, ocfg, ag, goal, obst, hi)
    assert not on[2, 0, 0, 1] and not on[2, 0, 1, 0] and on[3, 0, 0, 1] and on[3, 0, 1, 0]
    assert not on[1, 0, 1, :3].any() and not on[1, 0, :, 1].any() and on[1, 0, 1, 3:6].all()   # NaN: agent slots shut, goal slots open
    assert np.isnan(edges[1, 0, 1, 3:6, 0]).all() and np.isnan(rows[1, 0, 1, 0])
    _run_and_check(cuda, cfg, ag, goal, obst, hi, on, edges, rows, modes=[("all8", 8, 1, None), ("time3", 4, 3, None)])
