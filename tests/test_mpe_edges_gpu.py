"""dgppo_env_step / dgppo_graph_materialize / dgppo_graph_feats on the hand-built MPE scenes of tests/mpe_edge_scenes.py —
distances one ulp around the mask radii, cost margins on the jump of cost_value and on the -1 clip, coincident bodies, the
connectivity cost at its radius, goals one ulp around dist2goal, walls, velocity limits, actions on the clip, non-finite states,
actions, obstacles and goals — through env_step_kernel at both of its block widths, against oracle/env_np.py.
tests/test_mpe_edges_cpu.py shows on the oracle that the scenes reach those paths.  Convention (tests/test_env_edges_gpu.py):
integer graph fields equal, floats equal bit for bit, except that a NaN equals a NaN whatever its bits.  The one tolerance is
the one test_variant_step_matches_oracle grants MPEFormation's reward (its goals come from device cosf / sinf)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import env_np as E

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mpe_edge_scenes as S  # noqa: E402
from test_env_gpu import _mk, _run_step, _to  # noqa: E402
from test_env_edges_gpu import _freeze, _graph_same, _materialize, _same  # noqa: E402
from test_graph_feats_wave_gpu import SLOTS, _expected, _run_and_check  # noqa: E402
from test_large_team_kernels_gpu import _edge_of_slot  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable"),
              pytest.mark.filterwarnings("ignore:invalid value encountered")]      # the oracle subtracting NaN and inf
f32 = np.float32
CONFIGS = [("MPESpread", 4, 2), ("MPETarget", 3, 0), ("MPETarget", 4, 2), ("MPELine", 3, 2), ("MPELine", 5, 2),
           ("MPEFormation", 4, 2), ("MPECorridor", 4, 2), ("MPEConnectSpread", 4, 1), ("MPESpread", 9, 3)]
IDS = ["-".join(map(str, c)) for c in CONFIGS]
OUT = ("next_agent", "reward", "cost")


def _block_width(ocfg, with_graph):
    """the launch width of env_step_kernel (launch_step, csrc/env_step.hip): roundup64(max(n, E if a graph is written))"""
    work = max(ocfg.n_agents, ocfg.num_edges) if with_graph else ocfg.n_agents
    return min(max(-(-work // 64) * 64, 64), 512)


@functools.lru_cache(maxsize=None)
def _ref(kind, n, n_obs):
    """the catalogue of one config and the oracle's answers for it — a step, the graph of the state itself, and a second
    step from the first one's state with fresh actions — computed once and shared read-only"""
    ocfg = E.EnvCfg(E.KIND_NAMES[kind], n_agents=n, n_obs=n_obs)
    agent, goal, obst, action, tags = S.build(ocfg, 11)
    with np.errstate(all="ignore"):
        step = E.env_step(ocfg, agent, goal, obst, None, action)
        sense = dict(next_agent=agent, graph=E.get_graph(ocfg, agent, goal, obst, None))
        action2 = np.random.default_rng(3).uniform(-1.5, 1.5, size=action.shape).astype(f32)
        step2 = E.env_step(ocfg, step["next_agent"], goal, obst, None, action2)
    step.pop("next_hits"), step2.pop("next_hits")
    return _freeze(dict(ocfg=ocfg, agent=agent, goal=goal, obst=obst, action=action, action2=action2, tags=tuple(tags),
                        step=step, sense=sense, step2=step2))


def _outputs_same(ocfg, got, want, name, keys=OUT, graph=True):
    for k in keys:
        if k == "reward" and ocfg.kind == E.MPE_FORMATION:
            np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=f"{name} reward: NaN positions")
            np.testing.assert_allclose(got[k], want[k], atol=1e-7, rtol=1e-6, equal_nan=True, err_msg=f"{name} reward")
        else:
            _same(got[k], want[k], f"{name} {k}")
    if graph:
        _graph_same(got["graph"], want["graph"], name)


def _step(cfg, r, dev, **kw):
    return _run_step(cfg, r["ocfg"], r["agent"], r["goal"], r["obst"], None, r["action"], dev, **kw)


def test_both_block_widths_of_the_generic_kernel_occur():
    """phases 1a and 1c of env_step_kernel branch on blockDim == 64 (nt <= 64 against tid - 64): the small configs run at 64
    threads, the 9-agent one at more when it writes a graph and at 64 when it does not"""
    cfgs = [E.EnvCfg(E.KIND_NAMES[k], n_agents=n, n_obs=o) for k, n, o in CONFIGS]
    with_graph = [_block_width(c, True) for c in cfgs]
    assert set(with_graph[:-1]) == {64} and with_graph[-1] == 192
    assert {_block_width(c, False) for c in cfgs} == {64}


@pytest.mark.parametrize("kind,n,n_obs", CONFIGS, ids=IDS)
def test_mpe_edge_scenes_match_oracle_in_every_mode(cuda, kind, n, n_obs):
    """the whole catalogue as a step with graph, a step without (which narrows the block of the 9-agent config to 64), sense-only,
    and the materialised graph of the step's own next_agent; then all of it with the agent operand one float off a 16-byte
    boundary"""
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    ocfg, want = r["ocfg"], r["step"]
    assert (cfg.n_goals, cfg.n_cost, cfg.n_obs, cfg.num_edges) == (ocfg.n_goals, ocfg.n_cost, ocfg.n_obs, ocfg.num_edges)
    assert np.isnan(want["cost"]).any() and np.isnan(want["reward"]).any() and np.isnan(want["next_agent"]).any()
    for misalign in (False, True):
        name = f"{kind}-{n}-{n_obs}" + (" misaligned" if misalign else "")
        step = _step(cfg, r, cuda, misalign=misalign)
        _outputs_same(ocfg, step, want, f"{name} step")
        nog = _step(cfg, r, cuda, want_graph=False, misalign=misalign)
        assert "graph" not in nog
        _outputs_same(ocfg, nog, want, f"{name} step without graph", graph=False)
        sense = _run_step(cfg, ocfg, r["agent"], r["goal"], r["obst"], None, None, cuda, misalign=misalign)
        _outputs_same(ocfg, sense, r["sense"], f"{name} sense", keys=("next_agent",))
        mat = _materialize(cfg, step["next_agent"], r["goal"], r["obst"], None, cuda, misalign)
        _graph_same(mat, step["graph"], f"{name} materialise vs its step")


@pytest.mark.parametrize("kind,n,n_obs", CONFIGS, ids=IDS)
def test_second_step_from_the_devices_own_nan_state(cuda, kind, n, n_obs):
    """a second step chained from the device's own outputs with fresh actions: the NaN positions the first step produced
    (a NaN velocity) or kept (a NaN position) give exactly the oracle's NaN costs, reward and graph"""
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    ocfg = r["ocfg"]
    nx = _step(cfg, r, cuda)["next_agent"]
    _same(nx, r["step"]["next_agent"], "first step next_agent")
    with np.errstate(all="ignore"):
        want2 = E.env_step(ocfg, nx, r["goal"], r["obst"], None, r["action2"])
    by = {t.split("/")[1]: b for b, t in enumerate(r["tags"]) if t.startswith("non-finite/")}
    for name in ("position-nan", "velocity-nan"):                        # both are NaN positions by now
        assert np.isnan(nx[by[name], S.NF_AGENT, 0]) and np.isnan(want2["cost"][by[name], :, 0]).all(), name
    assert np.isnan(want2["reward"][by["velocity-nan"]]) and np.isnan(want2["graph"]["edges"][by["velocity-nan"]]).any()
    got2 = _run_step(cfg, ocfg, nx, r["goal"], r["obst"], None, r["action2"], cuda)
    _outputs_same(ocfg, got2, want2, "second step")


@pytest.mark.parametrize("kind,n,n_obs", CONFIGS, ids=IDS)
def test_non_finite_envs_do_not_leak_into_their_neighbours(cuda, kind, n, n_obs):
    """the outputs of the clean envs are bit-equal whether or not the non-finite envs sit between them in the batch"""
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    tags = r["tags"]
    keep = [b for b, t in enumerate(tags) if not t.startswith("non-finite")]
    clean = S.env_ids(tags, "clean")
    nf = S.env_ids(tags, "non-finite")
    assert len(clean) == S.N_CLEAN and any(nf[0] < b < nf[-1] for b in clean) and clean[-1] == nf[-1] + 1
    sub = lambda x: None if x is None else x[keep]
    full = _step(cfg, r, cuda)
    part = _run_step(cfg, r["ocfg"], sub(r["agent"]), sub(r["goal"]), sub(r["obst"]), None, sub(r["action"]), cuda)
    at = [keep.index(b) for b in clean]
    for k in OUT:
        assert np.isfinite(full[k][clean]).all()
        _same(full[k][clean], part[k][at], f"clean envs {k}")
    _graph_same({k: v[clean] for k, v in full["graph"].items()}, {k: v[at] for k, v in part["graph"].items()}, "clean envs")
    for k in OUT:                                                        # ... and so is every other finite env
        _same(full[k][keep], part[k], f"finite envs {k}")


@pytest.mark.parametrize("kind,n,n_obs", CONFIGS, ids=IDS)
def test_graph_feats_on_the_edge_scenes(cuda, kind, n, n_obs):
    """dgppo_graph_feats on the catalogue's states — the state itself, the first and the second step's, the state again as
    the four slots of a record — at Fp = node_dim and Fp = 8: emask, efeat, Xa and Xo against the oracle's graph through the
    NaN-aware helper of tests/test_graph_feats_wave_gpu.py, non-finite envs included.  Then its mask decisions against the
    graph the step kernel wrote for the same state: the two kernels agree at every threshold scene"""
    from dgppo_amd import ops_nn as K
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    ocfg, B = r["ocfg"], len(r["tags"])
    ag = np.stack([r["agent"], r["step"]["next_agent"], r["step2"]["next_agent"], r["agent"]], 1)
    assert ag.shape[1] == SLOTS
    with np.errstate(all="ignore"):
        on, edges, rows = _expected(cfg, ocfg, ag, r["goal"], r["obst"], None)
    assert on.any() and (~on).any() and np.isnan(rows).any() and np.isnan(edges[on]).any()
    _run_and_check(cuda, cfg, ag, r["goal"], r["obst"], None, on, edges, rows, modes=[("catalogue", B, SLOTS, None)])
    # the step kernel's own graph of slot 1, regrouped per (agent, slot)
    S_, sd = cfg.fan_in, cfg.state_dim
    n_other = cfg.num_nodes - 1 - n
    step = _step(cfg, r, cuda)
    recv = step["graph"]["receivers"][:, _edge_of_slot(cfg)]
    Xa = torch.empty(B * n, 8, device=cuda)
    Xo = torch.empty(B * n_other, 8, device=cuda)
    ef = torch.empty(B * n, S_, 4, device=cuda)
    em = torch.full((B * n, S_), float("nan"), device=cuda)
    K.graph_feats(cfg, _to(step["next_agent"], cuda), n * sd, n * sd, _to(r["goal"], cuda), _to(r["obst"], cuda), None, 0, 0,
                  None, B, 1, Xa, Xo, ef, em, 8)
    torch.cuda.synchronize()
    em = em.cpu().numpy().reshape(B, n, S_)
    for b, t in enumerate(r["tags"]):
        np.testing.assert_array_equal(em[b], (recv[b] != cfg.num_nodes - 1).astype(f32), err_msg=f"mask decisions, env {b} ({t})")
    flips = S.env_ids(r["tags"], "comm-radius")
    assert em[flips, 0, 1].tolist() == [1.0, 0.0, 0.0] and em[flips, 1, 0].tolist() == [1.0, 0.0, 0.0]
    if S.supports(ocfg, "obs-mask-radius") and not S.always_connected(ocfg):
        assert em[S.env_ids(r["tags"], "obs-mask-radius"), 0, n + cfg.goal_slots].tolist() == [1.0, 0.0, 0.0]
