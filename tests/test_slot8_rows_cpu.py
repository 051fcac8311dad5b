"""The identity the first-layer attention kernels rely on when they read no edge features (dgppo_attn_fwd_rows / _bwd_rows): on
every kind for which dgppo_attn_rows_supported says yes, the edge feature of (receiver i, slot s) in the oracle's GraphsTuple is,
bit for bit, the single rounded fp32 difference of columns 0..3 of the two node rows; on a LiDAR hit slot the first two columns,
then zeros.  And the query says no for every bicycle and VMAS configuration.  No GPU: the query is host code."""
import numpy as np
import pytest

from dgppo_amd import _native as N
from oracle import env_np as E

H_HEADS, FP = 3, 8
# (kind, n_agents, n_obs): every non-VMAS kind, the team sizes of the GPU tests (partial slot passes, two agent passes)
CASES = [(name, n, n_obs) for name in N.ENV_KINDS if name != "VMASReverseTransport"
         for n, n_obs in ((8, 3), (3, 2), (5, 0), (16, 3))]


def _static_edges(ocfg):
    """(receiver node, sender node, is LiDAR hit) of every edge of get_graph, in its block order, from the topology alone (the
    GraphsTuple's own senders / receivers point masked edges at the pad node)"""
    n, ng, k = ocfg.n_agents, ocfg.n_goals, ocfg.top_k
    out = [(i, j, False) for i in range(n) for j in range(n)]
    if ocfg.is_spread:
        out += [(i, n + g, False) for i in range(n) for g in range(ng)]
    else:
        out += [(i, n + i, False) for i in range(n)]
    if ocfg.is_lidar:
        if ocfg.n_obs_nodes > 0:
            out += [(i, n + ng + i * k + m, True) for i in range(n) for m in range(k)]
    else:
        out += [(i, n + ng + m, False) for i in range(n) for m in range(ocfg.n_obs)]
    return out


def _scene(ocfg, B, seed):
    """random records rather than reset states: non-zero velocities everywhere (goals and obstacles included), so that no
    column of the identity holds trivially; positions crowded enough that masks of both values occur"""
    rng = np.random.default_rng(seed)
    u = lambda *shape: rng.uniform(-0.7, 0.7, size=shape).astype(np.float32)
    n, sd = ocfg.n_agents, ocfg.state_dim
    agent, goal = u(B, n, sd), u(B, ocfg.n_goals, sd)
    hits = obst = None
    if ocfg.is_lidar:
        if ocfg.n_obs > 0:
            hits = (agent[:, :, None, :2] + 0.6 * u(B, n, ocfg.top_k, 2)).astype(np.float32)
    elif ocfg.n_obs > 0:
        obst = u(B, ocfg.n_obs, sd)
    return agent, goal, obst, hits


@pytest.mark.parametrize("name,n,n_obs", CASES)
def test_edge_features_are_row_differences_where_the_query_says_yes(name, n, n_obs):
    import ctypes
    kind = N.ENV_KINDS[name]
    cfg = N.make_env_cfg(kind, n, n_obs)
    yes = bool(N.lib().dgppo_attn_rows_supported(ctypes.byref(cfg), FP, H_HEADS))
    if kind == N.ENV_KINDS["LidarBicycleTarget"]:
        assert not yes, "the bicycle's edge features are products of its 5-float state"
        return
    assert yes, f"{name} n={n}: a slot-sparse shape on a 4-float state"
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs)
    agent, goal, obst, hits = _scene(ocfg, 4, seed=kind * 100 + n)
    g = E.get_graph(ocfg, agent, goal, obst, hits)
    nodes, edges = g["nodes"], g["edges"]
    stat = _static_edges(ocfg)
    assert len(stat) == edges.shape[1] == cfg.num_edges
    recv, send, hit = (np.array(c) for c in zip(*stat))
    want = (nodes[:, recv, :4] - nodes[:, send, :4]).astype(np.float32)
    want[:, hit, 2:] = 0.0
    assert edges.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(edges.view(np.uint32), want.view(np.uint32)), \
        f"{name} n={n}: {int((edges.view(np.uint32) != want.view(np.uint32)).sum())} edge words differ from the row differences"
    if hit.any():          # a hit row is (hx, hy, 0, 0 | ...): without the rule for hit slots columns 2, 3 would be the velocity
        assert np.array_equal(edges[:, hit, :2], (nodes[:, recv[hit], :2] - nodes[:, send[hit], :2]).astype(np.float32))
        assert (nodes[:, send[hit], 2:4] == 0).all() and (edges[:, hit, 2:] == 0).all()


def test_query_refuses_bicycle_vmas_and_other_shapes():
    import ctypes
    q = lambda cfg, F=FP, H=H_HEADS: bool(N.lib().dgppo_attn_rows_supported(ctypes.byref(cfg), F, H))
    for n, n_obs in ((3, 0), (4, 2), (8, 3), (16, 8)):
        assert not q(N.make_env_cfg(N.ENV_KINDS["LidarBicycleTarget"], n, n_obs))
    for n in (2, 4, 8, 16):
        vm = N.make_vmas_cfg(n)
        assert not q(vm) and not q(vm, F=20)
    ls = N.make_env_cfg(0, 8, 3)
    assert q(ls)
    assert not q(ls, F=32) and not q(ls, H=2) and not q(ls, F=0) and not q(ls, H=0)
    assert not q(N.make_env_cfg(0, 33, 3)), "above 32 agents the slot-sparse family does not run"
