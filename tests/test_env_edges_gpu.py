"""dgppo_env_step / dgppo_graph_materialize on the hand-built scenes of tests/env_edge_scenes.py — rays parallel to an edge (det == 0,
NaN alphas), clipped determinants, tied alphas, obstacles either side of the cull thresholds, distances one ulp around the mask
radii, non-finite actions and states — through the wave-per-env kernel, the workgroup-per-env kernel (operands one float off
a 16-byte boundary) and the generic kernel, against oracle/env_np.py.  tests/test_env_edges_cpu.py shows on the oracle that the
scenes reach those paths.  Convention: integer graph fields equal, floats equal bit for bit, except that a NaN equals a NaN
whatever its bits.  The bicycle's dynamics go by the route of test_bicycle_dynamics_tolerance_then_exact_sensing."""
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
import env_edge_scenes as S  # noqa: E402
from test_env_gpu import _bits, _misaligned, _mk, _run_step, _step_dev, _to  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable"),
              pytest.mark.filterwarnings("ignore:invalid value encountered")]      # the oracle subtracting NaN features
f32 = np.float32
WAVE = [("LidarSpread", 4, 2), ("LidarTarget", 4, 2), ("LidarBicycleTarget", 4, 3), ("LidarSpread", 8, 3)]
GENERIC = ("LidarLine", 4, 3)
OUT = ("next_agent", "next_hits", "reward", "cost")
INT_KEYS, FLOAT_KEYS = ("receivers", "senders", "node_type", "n_node", "n_edge"), ("nodes", "edges", "states")


def _same(got, want, name):
    """NaN exactly where `want` is NaN, equal bits everywhere else"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaN positions")
    bad = np.where(nan, f32(0), got).view(np.uint32) != np.where(nan, f32(0), want).view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}"


def _graph_same(got, want, name):
    """_assert_graph_equal of tests/test_env_gpu.py with NaN == NaN in the float fields"""
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {k}")
    for k in FLOAT_KEYS:
        _same(got[k], want[k], f"{name} {k}")


def _outputs_same(got, want, keys, name):
    for k in keys:
        _same(got[k], want[k], f"{name} {k}")
    _graph_same(got["graph"], want["graph"], name)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def _ref(kind, n, n_obs, n_rays=32, top_k=8, only=None):
    """the catalogue of one config and the oracle's answers for it, computed once and shared read-only"""
    ocfg = E.EnvCfg(E.KIND_NAMES[kind], n_agents=n, n_obs=n_obs, n_rays=n_rays, top_k=top_k)
    agent, goal, obst, action, tags = S.build(ocfg, 11, only=only)
    tab = E.ray_table(n_rays)
    hits, _ = E.lidar_sense(ocfg, agent[..., :2], obst, *tab)            # graph_t: NaN hit points where a ray is parallel
    step = E.env_step(ocfg, agent, goal, obst, hits, action, tab)
    sense = dict(next_agent=agent, next_hits=hits, graph=E.get_graph(ocfg, agent, goal, obst, hits))
    return _freeze(dict(ocfg=ocfg, agent=agent, goal=goal, obst=obst, action=action, hits=hits, tags=tuple(tags), tab=tab,
                        step=step, sense=sense))


def _materialize(cfg, agent, goal, obst, hits, dev, misalign=False):
    from dgppo_amd import ops_env as O
    g = O.alloc_graph(cfg, agent.shape[0], dev)
    a = _to(agent, dev)
    O.graph_materialize(cfg, _misaligned(a) if misalign else a, _to(goal, dev), _to(obst, dev), _to(hits, dev), g)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def _bicycle_against_oracle(r, got, name):
    """dynamics within the 1e-6 of test_bicycle_dynamics_tolerance_then_exact_sensing (device atan2f / cosf / sinf), then the
    oracle's sensing and graph on the device's own state, bit for bit"""
    ocfg, want = r["ocfg"], r["step"]
    np.testing.assert_array_equal(np.isnan(got["next_agent"]), np.isnan(want["next_agent"]), err_msg=f"{name} next_agent NaN")
    np.testing.assert_allclose(got["next_agent"], want["next_agent"], atol=1e-6, rtol=0, equal_nan=True, err_msg=name)
    _same(got["cost"], want["cost"], f"{name} cost")
    _same(got["reward"], want["reward"], f"{name} reward")
    nx = got["next_agent"]
    h2, _ = E.lidar_sense(ocfg, nx[..., :2], r["obst"], *r["tab"])
    _same(got["next_hits"], h2, f"{name} next_hits on the device's state")
    _graph_same(got["graph"], E.get_graph(ocfg, nx, r["goal"], r["obst"], h2), f"{name} graph on the device's state")


def _three_modes(cfg, r, dev, misalign):
    """step, sense-only and materialise (of the step's own outputs) through one kernel family"""
    a = (r["agent"], r["goal"], r["obst"])
    step = _run_step(cfg, r["ocfg"], *a, r["hits"], r["action"], dev, misalign=misalign)
    sense = _run_step(cfg, r["ocfg"], *a, None, None, dev, misalign=misalign)
    mat = _materialize(cfg, step["next_agent"], r["goal"], r["obst"], step["next_hits"], dev, misalign)
    return step, sense, mat


def _check_family_against_oracle(r, step, sense, mat, name):
    if r["ocfg"].is_bicycle:
        _bicycle_against_oracle(r, step, f"{name} step")
    else:
        _outputs_same(step, r["step"], OUT, f"{name} step")
    _outputs_same(sense, r["sense"], ("next_agent", "next_hits"), f"{name} sense")
    _graph_same(mat, step["graph"], f"{name} materialise vs its step")


@pytest.mark.parametrize("kind,n,n_obs", WAVE)
def test_edge_scenes_every_family_matches_oracle(cuda, kind, n, n_obs):
    """the whole catalogue in step, sense-only and materialise mode: wave kernel == workgroup kernel == oracle"""
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    assert np.isnan(r["hits"]).any() and np.isnan(r["step"]["cost"]).any() and np.isnan(r["step"]["next_hits"]).any()
    wave = _three_modes(cfg, r, cuda, misalign=False)
    wg = _three_modes(cfg, r, cuda, misalign=True)
    _outputs_same(wave[0], wg[0], OUT, "wave vs workgroup: step")
    _outputs_same(wave[1], wg[1], ("next_agent", "next_hits"), "wave vs workgroup: sense")
    _graph_same(wave[2], wg[2], "wave vs workgroup: materialise")
    _check_family_against_oracle(r, *wave, "wave")
    _check_family_against_oracle(r, *wg, "workgroup")


def test_edge_scenes_generic_kernel(cuda):
    """LidarLine (not a base kind: 32 rays / top-8 go to the generic kernel) on the whole catalogue in all three modes; then
    a 16-ray, top-16 fan on the axis-aligned and symmetric-ties scenes rebuilt for its table: every ray is a hit point there,
    so NaN alphas land in next_hits, and a second step chained from the device's own outputs holds the NaN obstacle cost and
    the graph of NaN hit points to the oracle"""
    from dgppo_amd import _native as N
    cfg, _ = _mk(*GENERIC)
    r = _ref(*GENERIC)
    _check_family_against_oracle(r, *_three_modes(cfg, r, cuda, misalign=False), "generic")

    cfg16 = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 5, 2, n_rays=16, top_k=16)
    r16 = _ref("LidarSpread", 5, 2, 16, 16, ("axis-aligned", "symmetric-ties"))
    o16 = r16["ocfg"]
    step, sense, mat = _three_modes(cfg16, r16, cuda, misalign=False)
    _check_family_against_oracle(r16, step, sense, mat, "generic 16 rays")
    assert np.isnan(step["next_hits"]).any(axis=(1, 2, 3)).all(), "a NaN hit point in every env"
    action2 = np.random.default_rng(3).uniform(-1.5, 1.5, size=r16["action"].shape).astype(f32)
    want2 = E.env_step(o16, step["next_agent"], r16["goal"], r16["obst"], step["next_hits"], action2, r16["tab"])
    got2 = _run_step(cfg16, o16, step["next_agent"], r16["goal"], r16["obst"], step["next_hits"], action2, cuda)
    assert np.isnan(want2["cost"][..., 1]).any() and np.isfinite(want2["cost"][..., 0]).all()
    _outputs_same(got2, want2, OUT, "generic 16 rays, second step")


def _is_prime(p):
    return p > 1 and all(p % q for q in range(2, int(p ** 0.5) + 1))


@pytest.mark.parametrize("kind,n,n_obs", WAVE)
def test_nan_env_does_not_leak_into_the_next_env_of_a_wave(cuda, kind, n, n_obs):
    """the catalogue tiled to 3 x 8 x 4 x CU-count envs: every persistent wave walks from NaN / tie envs to clean ones and
    back (the ray marks, the NaN branch and the key lists are per-wave LDS state).  A wave's consecutive envs are one grid of
    waves apart — a multiple of the CU count — so the tile length is made a prime (clean envs repeated at its end): no grid
    size then maps a wave onto one scene only.  Wave against workgroup kernel, both against the tiled oracle, on the device."""
    from dgppo_amd import ops_env as O
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    B = len(r["tags"])
    order = list(range(B))
    clean = S.env_ids(r["tags"], "clean")
    while not _is_prime(len(order)):
        order.append(clean[len(order) % 2])
    P = len(order)
    Bw = 3 * 8 * 4 * torch.cuda.get_device_properties(cuda).multi_processor_count
    idx = torch.tensor(order, device=cuda)[torch.arange(Bw, device=cuda) % P]
    tile = lambda x: _to(x, cuda)[idx].contiguous()
    A, G, Ob, H, Ac = (tile(r[k]) for k in ("agent", "goal", "obst", "hits", "action"))

    def dev_same(got, want, name):
        nan = torch.isnan(want) if want.dtype == torch.float32 else torch.zeros_like(want, dtype=torch.bool)
        if want.dtype == torch.float32:
            assert torch.equal(torch.isnan(got), nan), f"{name}: NaN positions"
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), name

    for tag, h_in, act, want in (("step", H, Ac, r["step"]), ("sense", None, None, r["sense"])):
        keys = OUT if tag == "step" else OUT[:2]
        w = _step_dev(cfg, A, G, Ob, h_in, act)
        v = _step_dev(cfg, A, G, Ob, h_in, act, misalign=True)
        for k in keys:
            dev_same(w[k], v[k], f"{Bw} envs {tag} {k}: wave vs workgroup")
        for k in w["graph"]:
            dev_same(w["graph"][k], v["graph"][k], f"{Bw} envs {tag} graph {k}: wave vs workgroup")
        del v
        if not (r["ocfg"].is_bicycle and tag == "step"):                 # the bicycle's dynamics are held to 1e-6 elsewhere
            for k in keys:
                dev_same(w[k], tile(want[k]), f"{Bw} envs {tag} {k}: wave vs oracle")
            for k, x in want["graph"].items():
                dev_same(w["graph"][k], tile(x), f"{Bw} envs {tag} graph {k}: wave vs oracle")
        for k in keys:                                                   # every copy of a scene gives what its first copy gives
            dev_same(w[k], w[k][:P][torch.arange(Bw, device=cuda) % P], f"{Bw} envs {tag} {k}: copies differ")
        if tag == "step":
            g1, g2 = O.alloc_graph(cfg, Bw, cuda), O.alloc_graph(cfg, Bw, cuda)
            O.graph_materialize(cfg, w["next_agent"], G, Ob, w["next_hits"], g1)
            O.graph_materialize(cfg, _misaligned(w["next_agent"]), G, Ob, w["next_hits"], g2)
            for k in g1:
                dev_same(g1[k], g2[k], f"{Bw} envs materialise {k}: wave vs workgroup")
                dev_same(g1[k], w["graph"][k], f"{Bw} envs materialise {k} vs step")
            del g1, g2
        del w
    torch.cuda.synchronize()


def _expected_nan(ocfg, tags):
    """where the reference's clip (jnp.clip keeps a NaN) leaves NaN in the outputs of the five non-finite envs, spelled out for
    the double integrator; a = the agent that got the value.  Masks over [B, n, ...]"""
    n, sd, k, a = ocfg.n_agents, ocfg.state_dim, ocfg.top_k, S.NF_AGENT
    B = len(tags)
    nx, hits = np.zeros((B, n, sd), bool), np.zeros((B, n, k, 2), bool)
    rew, cost = np.zeros(B, bool), np.zeros((B, n, 2), bool)
    for b, t in enumerate(tags):
        name = t.split("/")[1]
        if name == "action-nan":            # u0 = NaN: the x velocity, and the action term of the reward
            nx[b, a, 2] = True
            rew[b] = True
        elif name == "position-nan":        # x = NaN: stays; every ray of a is NaN; every distance to a is NaN
            nx[b, a, 0] = True
            hits[b, a] = True
            rew[b] = True
            cost[b, :, 0] = True            # each agent's nearest-neighbour minimum meets the NaN distance
            cost[b, a, 1] = True
        elif name == "velocity-nan":        # vx = NaN: x and vx of t + 1, and the rays cast from there
            nx[b, a, 0] = nx[b, a, 2] = True
            hits[b, a] = True
        # action-inf clips to (1, -1); velocity-inf clips to the bounds: all finite
    return dict(next_agent=nx, next_hits=hits, reward=rew, cost=cost)


@pytest.mark.parametrize("kind,n,n_obs", WAVE + [GENERIC])
def test_non_finite_action_and_state_follow_the_reference_clip(cuda, kind, n, n_obs):
    """a NaN action or state stays NaN through clip_action and the state clip (jnp.clip; fminf / fmaxf would hand back a bound),
    +-inf clip to the bounds — in every kernel family, NaN at exactly the named places and nowhere else"""
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs, only=("non-finite",))
    ocfg, tags, want = r["ocfg"], r["tags"], r["step"]
    assert tuple(t.split("/")[1] for t in tags) == S.NON_FINITE
    by = {t.split("/")[1]: b for b, t in enumerate(tags)}
    a, sd, k = S.NF_AGENT, ocfg.state_dim, ocfg.top_k
    families = [("generic", False)] if (kind, n, n_obs) == GENERIC else [("wave", False), ("workgroup", True)]
    for fam, mis in families:
        got = _run_step(cfg, ocfg, r["agent"], r["goal"], r["obst"], r["hits"], r["action"], cuda, misalign=mis)
        if ocfg.is_bicycle:
            _bicycle_against_oracle(r, got, fam)
            exp = {key: np.isnan(want[key]) for key in ("next_agent", "reward", "cost")}
            assert exp["next_agent"][by["velocity-inf"], a, 2:4].all()   # cos / sin of an infinite heading
            assert exp["next_agent"][by["velocity-nan"], a].all() and exp["next_agent"][by["action-nan"], a, 2:4].all()
            exp["next_hits"] = np.isnan(got["next_hits"])
            assert exp["next_hits"][by["velocity-nan"], a].all() and exp["next_hits"][by["position-nan"], a].all()
        else:
            exp = _expected_nan(ocfg, tags)
            vi = got["next_agent"][by["velocity-inf"], a]
            assert vi[0] == f32(ocfg.area_size) and vi[2] == f32(ocfg.vel_limit), f"{fam}: +inf clips to the bounds"
            ai = got["next_agent"][by["action-inf"]]
            base = r["agent"][by["action-inf"]]
            assert ai[a, 2] == min(base[a, 2] + f32(f32(10.0) * f32(ocfg.dt)), f32(ocfg.vel_limit)), f"{fam}: +inf acts as +1"
            assert ai[a, 3] == max(base[a, 3] - f32(f32(10.0) * f32(ocfg.dt)), -f32(ocfg.vel_limit)), f"{fam}: -inf acts as -1"
        for key, mask in exp.items():
            np.testing.assert_array_equal(np.isnan(got[key]), mask, err_msg=f"{fam} {key}: NaN positions")
        # the graph carries exactly these: agent rows from next_agent, hit rows from next_hits, pad and goal rows finite
        g = got["graph"]
        node_nan = np.zeros(g["nodes"].shape, bool)
        node_nan[:, :n, :sd] = exp["next_agent"]
        node_nan[:, n + ocfg.n_goals:-1, :2] = exp["next_hits"].reshape(len(tags), n * k, 2)
        np.testing.assert_array_equal(np.isnan(g["nodes"]), node_nan, err_msg=f"{fam} graph nodes: NaN positions")
        np.testing.assert_array_equal(np.isnan(g["states"]), node_nan[..., :sd], err_msg=f"{fam} graph states: NaN positions")
        b = by["position-nan"]
        pad = ocfg.num_nodes - 1
        assert (g["receivers"][b, a * n:(a + 1) * n] == pad).all() and (g["receivers"][b, a:n * n:n] == pad).all(), \
            f"{fam}: no agent-agent edge to or from an agent at NaN"
        assert np.isnan(g["edges"][b, a * n:(a + 1) * n, 0]).all() and not np.isnan(g["edges"][b, a * n:(a + 1) * n, 1]).any()
        if not ocfg.is_bicycle:
            _outputs_same(got, want, OUT, fam)
