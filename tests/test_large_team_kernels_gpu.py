"""Teams of 17 to 64 agents, kernel by kernel: env step / sense-only / materialise and reset against oracle/env_np.py,
dgppo_graph_feats against the oracle's graph, dgppo_gae / dgppo_advantage_lagr / dgppo_lagr_update against
oracle/algo_ref.py, and the informarl / hcbfcrpo / informarl_lagr engines against oracle/dgppo_ref.py — at the sizes where
these kernels change family, change their LDS budget or used to stop.  Every case first asserts, from a restatement of the
host's own formulas, which family its shape selects: a moved boundary fails loudly instead of testing something else.

Scenes: host-side reset refuses a disc coverage above 0.50 and the oracle's unbounded rejection loops do not finish just
below it, so every case here passes an explicit area_size (to the native cfg and to the oracle) with coverage <= 0.15."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import algo_ref as A
from oracle import dgppo_ref as R
from oracle import env_np as E
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_env_gpu import _assert_graph_equal, _random_state, _run_step, _to  # noqa: E402
from test_large_team_gpu import (_check_advantage, _check_first_minibatch_grads, _close_np, _image_bytes, _np_rollout,  # noqa: E402
                                 LDS_IMAGE)

# the shared scenes are read-only arrays; torch.from_numpy warns about those, and nothing here writes through the tensors
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
KB = 1024
WAVE_MAX_AGENTS = 16            # csrc/env_wave.hip: the wave-per-env kernel has no instance above 16 agents
LIDAR_WG_LDS = 60 * KB          # csrc/env_step.hip step_family: lidar_step_kernel while its stage fits
STEP_LDS = 64 * KB              # launch_step: the generic stage is computed for every launch and refused above this
GAE_STATIC_LDS = 64 * KB        # dgppo_gae: above it the generic kernel opts in to more dynamic LDS; the rows family falls through
GAE_MAX_LDS = 150 * KB          # dgppo_gae: refused above
ADV_LAGR_MAX_COLS = 192         # csrc/gae.hip: 64 agents x 3 costs
MAX_COVERAGE = 0.15


# ---- the host's formulas, restated ------------------------------------------------------------------------------------------
def _lidar_smem_bytes(cfg):
    """csrc/env_step.hip lidar_smem_bytes"""
    n, no, k, SD = cfg.n_agents, cfg.n_obs, cfg.top_k, cfg.state_dim
    NR, Nn = n * 32, 2 * n + n * k + 1
    w = (no * 16 + n * no * 16 + NR + n * 8 + no * 16 + n * SD * 3 + n * 2 + n * k * 4 + (2 * n * n + n * k) + n * no + 2 * n +
         Nn * (SD + 3) + Nn * SD)
    return 4 * w


def _step_smem_bytes(cfg):
    """csrc/env_step.hip step_smem_bytes"""
    n, ng, no, SD = cfg.n_agents, cfg.n_goals, cfg.n_obs, cfg.state_dim
    lidar = cfg.is_lidar
    kk = (cfg.top_k if no > 0 else 0) if lidar else 0
    nrg = ng if cfg.reward_goals == 0 else n                       # cfg_reward_goals: the goal nodes, or n derived goals
    fl = ((no * 16 if lidar else 0) + n * SD * 2 + ng * SD + n * 2 + no * cfg.obst_stride + n * kk * 4 +
          (n * cfg.n_rays if lidar else 0) + n * 4 + ng * 4 + 3 * nrg + 3 * n + n * no + n * n + n * max(kk, no) + nrg * n)
    return 4 * fl


def _step_family(cfg):
    """csrc/env_step.hip step_family for aligned operands and the default thresholds (eye_offset >= comm_radius)"""
    base = cfg.kind <= 4 and cfg.n_goals == cfg.n_agents and cfg.reward_goals == 0 and cfg.n_cost == 2
    lidar32 = cfg.is_lidar and base and cfg.n_obs > 0 and cfg.n_rays == 32
    if lidar32 and cfg.top_k == 8 and cfg.n_agents <= WAVE_MAX_AGENTS:
        return "wave-or-workgroup"                                 # the instantiation list decides; no case here is that small
    if lidar32 and _lidar_smem_bytes(cfg) <= LIDAR_WG_LDS:
        return "lidar_wg"
    return "generic"


def _gae_family(T_, n, nh, lam):
    """csrc/gae.hip dgppo_gae: (family, bytes of LDS it asks for)"""
    AH, oml = n * nh, float(f32(1.0) - f32(lam))
    generic = 4 * ((T_ + 1) * AH + (T_ + 1) + 2 * AH)
    if T_ <= 256 and 0.0 <= oml <= 0.5:
        return "cols", 0
    if T_ + 1 <= 256 and AH <= 32:
        ahp = 8 if AH <= 8 else (16 if AH <= 16 else 32)
        fsm = 4 * (T_ * AH + (T_ + 1) * AH + (T_ + 1) + T_ + 2 * 16 * (ahp + 1))
        if fsm <= GAE_STATIC_LDS:
            return "rows", fsm
        return "generic-after-rows", generic
    return ("generic" if generic <= GAE_MAX_LDS else "refused"), generic


def _coverage(cfg):
    """csrc/env_reset.hip dgppo_env_reset_checked: disc coverage of the rejection sampling"""
    d, ax = cfg.reset_min_dist, cfg.area_size
    ay = cfg.reset_side_y if cfg.reset_side_y > 0 else ax
    return cfg.n_agents * math.pi * (d / 2) ** 2 / ((ax + d) * (ay + d))


def _mk(kind_name, n, n_obs, area):
    from dgppo_amd import _native as N
    kind = N.ENV_KINDS[kind_name]
    cfg = N.make_env_cfg(kind, n, n_obs, area_size=area)
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs, area_size=area)
    assert _coverage(cfg) <= MAX_COVERAGE, (kind_name, n, area, _coverage(cfg))
    assert (cfg.n_obs, cfg.n_goals, cfg.n_cost, cfg.num_nodes, cfg.num_edges) == \
        (ocfg.n_obs, ocfg.n_goals, ocfg.n_cost, ocfg.num_nodes, ocfg.num_edges)
    return cfg, ocfg


@functools.lru_cache(maxsize=None)
def _scene(kind, n, n_obs, area, B=8):
    """one random scene and the oracle's step on it per case, shared by every test that needs it and never written to"""
    cfg, ocfg = _mk(kind, n, n_obs, area)
    agent, goal, obst, action = _random_state(ocfg, B, seed=1000 + 10 * n + n_obs)
    tab = E.ray_table(ocfg.n_rays)
    hits = E.lidar_sense(ocfg, agent[..., :2], obst, *tab)[0] if (ocfg.is_lidar and ocfg.n_obs > 0) else None
    want = E.env_step(ocfg, agent, goal, obst, hits, action, tab)
    for a in (agent, goal, obst, action, hits, *[v for v in want.values() if isinstance(v, np.ndarray)], *want["graph"].values()):
        if a is not None:
            a.setflags(write=False)
    return cfg, ocfg, agent, goal, obst, hits, action, want


def _bits_equal(got, want, name):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=name)


def _masks_vary(ocfg, graph):
    r, n, pad = graph["receivers"], ocfg.n_agents, ocfg.num_nodes - 1
    assert (r == pad).any() and (r[:, :n * n] != pad).any(), "masks must vary in this scene, otherwise it proves little"


# ---- 1. env step ------------------------------------------------------------------------------------------------------------
# (kind, n, n_obs, area_size, family).  The boundary pairs sit on both sides of lidar_smem_bytes = 60 KB; the n are re-derived
# from the formula by test_step_family_boundaries_follow_from_the_formula.
BOUNDARY = [("LidarSpread", 44, 3, 3.0, "lidar_wg"), ("LidarSpread", 45, 3, 3.0, "generic"),
            ("LidarTarget", 44, 3, 3.0, "lidar_wg"), ("LidarTarget", 45, 3, 3.0, "generic"),
            ("LidarBicycleTarget", 34, 8, 2.5, "lidar_wg"), ("LidarBicycleTarget", 35, 8, 2.5, "generic"),
            ("LidarSpread", 27, 16, 2.5, "lidar_wg"), ("LidarSpread", 28, 16, 2.5, "generic")]
# the Line kinds keep their landmarks (n - 2) * 6 * car_radius = 18.6 apart at 64 agents: no smaller area is admitted
CEILING = [("LidarSpread", 64, 3, 4.0, "generic"), ("LidarTarget", 64, 3, 4.0, "generic"),
           ("LidarBicycleTarget", 64, 8, 4.0, "generic"), ("LidarSpread", 64, 0, 4.0, "generic"),
           ("LidarLine", 64, 2, 20.0, "generic"), ("MPESpread", 64, 3, 4.0, "generic"), ("MPETarget", 64, 13, 4.0, "generic"),
           ("MPEConnectSpread", 48, 3, 3.0, "generic"), ("MPEFormation", 64, 3, 4.0, "generic"),
           ("MPELine", 64, 3, 20.0, "generic"), ("LidarSpread", 61, 3, 4.0, "generic")]
_ids = lambda cases: [f"{c[0]}-{c[1]}-{c[2]}" for c in cases]


def _assert_family(cfg, family):
    assert cfg.n_agents > WAVE_MAX_AGENTS
    assert _step_family(cfg) == family, (family, _lidar_smem_bytes(cfg))
    assert _step_smem_bytes(cfg) <= STEP_LDS, "the generic stage is checked on every launch"
    if cfg.is_lidar and cfg.kind <= 2 and cfg.n_obs > 0:
        assert (_lidar_smem_bytes(cfg) <= LIDAR_WG_LDS) == (family == "lidar_wg")


def test_step_family_boundaries_follow_from_the_formula():
    """the first team size whose lidar_step_kernel stage exceeds 60 KB, per (n_obs, state_dim): the boundary pairs above are
    exactly (that n - 1, that n), and n_obs = 1 keeps the workgroup kernel up to 48 agents"""
    from dgppo_amd import _native as N

    def first_generic(kind, n_obs):
        return next(n for n in range(17, 65) if _lidar_smem_bytes(N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs)) > LIDAR_WG_LDS)
    derived = {("LidarSpread", 3): first_generic("LidarSpread", 3), ("LidarTarget", 3): first_generic("LidarTarget", 3),
               ("LidarBicycleTarget", 8): first_generic("LidarBicycleTarget", 8), ("LidarSpread", 16): first_generic("LidarSpread", 16)}
    for (kind, n_obs), n in derived.items():
        assert (kind, n - 1, n_obs) in [c[:3] for c in BOUNDARY if c[4] == "lidar_wg"], (kind, n_obs, n)
        assert (kind, n, n_obs) in [c[:3] for c in BOUNDARY if c[4] == "generic"], (kind, n_obs, n)
    assert first_generic("LidarSpread", 1) == 49
    print("first generic n:", derived)


@pytest.mark.parametrize("kind,n,n_obs,area,family", BOUNDARY + CEILING, ids=_ids(BOUNDARY + CEILING))
def test_step_matches_oracle_large_team(cuda, kind, n, n_obs, area, family):
    """dgppo_env_step with the full graph, B = 8, under the rules of tests/test_env_gpu.py: every output and the whole graph
    bit-exact; the bicycle's dynamics within 1e-6 and its sensing bit-exact on the device's own next state; MPEFormation's
    reward (device cosf / sinf) within the tolerance of test_variant_step_matches_oracle."""
    cfg, ocfg, agent, goal, obst, hits, action, want = _scene(kind, n, n_obs, area)
    _assert_family(cfg, family)
    got = _run_step(cfg, ocfg, agent, goal, obst, hits, action, cuda)
    assert got["cost"].shape == (8, n, ocfg.n_cost)
    _bits_equal(got["cost"], want["cost"], "cost")
    if kind == "MPEFormation":
        np.testing.assert_allclose(got["reward"], want["reward"], atol=1e-7, rtol=1e-6)
    else:
        _bits_equal(got["reward"], want["reward"], "reward")
    if ocfg.is_bicycle:
        np.testing.assert_allclose(got["next_agent"], want["next_agent"], atol=1e-6, rtol=0)      # device atan2 / sincos
        nx = got["next_agent"]
        h2, _ = E.lidar_sense(ocfg, nx[..., :2], obst, *E.ray_table(32))
        _bits_equal(got["next_hits"], h2, "next_hits on the device's next state")
        g2 = E.get_graph(ocfg, nx, goal, obst, h2)
        _assert_graph_equal(got["graph"], g2)
        _masks_vary(ocfg, g2)
    else:
        _bits_equal(got["next_agent"], want["next_agent"], "next_agent")
        if want["next_hits"] is not None:
            _bits_equal(got["next_hits"], want["next_hits"], "next_hits")
        _assert_graph_equal(got["graph"], want["graph"])
        _masks_vary(ocfg, want["graph"])
    assert got["graph"]["nodes"].shape == (8, ocfg.num_nodes, ocfg.node_dim)
    if kind == "MPEConnectSpread":
        c2 = got["cost"][..., 2]
        assert (c2 == c2[:, :1]).all(), "the connectivity cost is one value per env"


def test_step_reads_misaligned_inputs_at_45_agents(cuda):
    """`agent` one float past a 16-byte boundary at LidarSpread 45 / 3 (generic) and 44 / 3 (workgroup LiDAR kernel): the
    workgroup kernels read it correctly — same bits as the oracle"""
    for n, family in ((45, "generic"), (44, "lidar_wg")):
        cfg, ocfg, agent, goal, obst, hits, action, want = _scene("LidarSpread", n, 3, 3.0)
        _assert_family(cfg, family)
        got = _run_step(cfg, ocfg, agent, goal, obst, hits, action, cuda, misalign=True)
        for k in ("next_agent", "next_hits", "reward", "cost"):
            _bits_equal(got[k], want[k], f"n={n} {k}")
        _assert_graph_equal(got["graph"], want["graph"])


def test_three_chained_steps_at_64_agents(cuda):
    """LidarSpread 64 / 3: three steps feeding the device's own outputs back, each against the oracle on the same inputs"""
    cfg, ocfg, agent, goal, obst, hits, _, _ = _scene("LidarSpread", 64, 3, 4.0)
    _assert_family(cfg, "generic")
    rng, tab = np.random.default_rng(64), E.ray_table(32)
    a_np, h_np = agent, hits
    for t in range(3):
        action = rng.uniform(-1.2, 1.2, size=(8, 64, 2)).astype(f32)
        got = _run_step(cfg, ocfg, a_np, goal, obst, h_np, action, cuda)
        want = E.env_step(ocfg, a_np, goal, obst, h_np, action, tab)
        for k in ("next_agent", "next_hits", "reward", "cost"):
            _bits_equal(got[k], want[k], f"{k} t={t}")
        _assert_graph_equal(got["graph"], want["graph"])
        a_np, h_np = got["next_agent"], got["next_hits"]
    g, pad = got["graph"], ocfg.num_nodes - 1
    assert np.all(g["n_node"] == ocfg.num_nodes) and np.all(g["n_edge"] == ocfg.num_edges)
    assert np.all((g["receivers"] == pad) == (g["senders"] == pad)) and np.all(g["states"][:, pad] == -1)


@pytest.mark.parametrize("n,area,family", [(44, 3.0, "lidar_wg"), (45, 3.0, "generic"), (64, 4.0, "generic")])
def test_sense_only_and_materialize_large_team(cuda, n, area, family):
    """sense-only dgppo_env_step and dgppo_graph_materialize at LidarSpread n / 3: hits and graph of the given state"""
    from dgppo_amd import ops_env as O
    cfg, ocfg, agent, goal, obst, hits, _, _ = _scene("LidarSpread", n, 3, area)
    _assert_family(cfg, family)
    want_g = E.get_graph(ocfg, agent, goal, obst, hits)
    got = _run_step(cfg, ocfg, agent, goal, obst, None, None, cuda)
    np.testing.assert_array_equal(got["next_agent"], agent)
    _bits_equal(got["next_hits"], hits, "sensed hits")
    _assert_graph_equal(got["graph"], want_g)
    g = O.alloc_graph(cfg, 8, cuda)
    O.graph_materialize(cfg, _to(agent, cuda), _to(goal, cuda), _to(obst, cuda), _to(hits, cuda), g)
    torch.cuda.synchronize()
    _assert_graph_equal({k: v.cpu().numpy() for k, v in g.items()}, want_g)
    _masks_vary(ocfg, want_g)


def _smallest_refused_step_cfg():
    """the admitted config (n <= 64, n_obs <= 64) with the fewest agents, then the fewest obstacles, whose generic stage
    exceeds 64 KB"""
    from dgppo_amd import _native as N
    best = None
    for kind in ("LidarSpread", "LidarTarget", "LidarBicycleTarget", "MPESpread", "MPETarget"):
        for n in range(1, 65):
            no = next((o for o in range(0, 65) if _step_smem_bytes(N.make_env_cfg(N.ENV_KINDS[kind], n, o)) > STEP_LDS), None)
            if no is not None and (best is None or (n, no) < best[1:]):
                best = (kind, n, no)
                break
    return best


def test_step_refuses_a_config_beyond_its_lds_stage(cuda):
    """step_smem_bytes > 64 KB is refused on the host, with its message, before anything is launched: outputs untouched"""
    from dgppo_amd import _native as N, ops_env as O
    found = _smallest_refused_step_cfg()
    assert found is not None
    kind, n, no = found
    cfg = N.make_env_cfg(N.ENV_KINDS[kind], n, no, area_size=4.0)
    assert _step_smem_bytes(cfg) > STEP_LDS
    smaller = N.make_env_cfg(N.ENV_KINDS[kind], n, no - 1, area_size=4.0)
    assert _step_smem_bytes(smaller) <= STEP_LDS
    print("smallest refused config:", found, _step_smem_bytes(cfg), "bytes")
    B = 2
    z = lambda *s: torch.zeros(*s, device=cuda)
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    rc, rs = O.ray_tables(32, cuda)
    nx, nh, rew, cost = nan(B, n, cfg.state_dim), nan(B, n, 8, 2), nan(B), nan(B, n, 2)
    with pytest.raises(ValueError, match="env too large for the per-env LDS stage"):
        O.env_step(cfg, z(B, n, cfg.state_dim), z(B, n, 2), z(B, n, cfg.state_dim), z(B, no, cfg.obst_stride),
                   z(B, n, 8, 2) if cfg.is_lidar else None, rc if cfg.is_lidar else None, rs if cfg.is_lidar else None,
                   nx, nh if cfg.is_lidar else None, rew, cost, None)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (nx, nh, rew, cost))


# ---- 2. reset ---------------------------------------------------------------------------------------------------------------
RESET_CASES = [("LidarSpread", 45, 3, 3.0), ("LidarSpread", 64, 3, 4.0), ("LidarBicycleTarget", 64, 8, 4.0),
               ("MPETarget", 64, 13, 4.0), ("MPEConnectSpread", 48, 3, 3.0), ("LidarLine", 64, 2, 20.0),
               ("MPEFormation", 64, 3, 4.0)]


@pytest.mark.parametrize("kind,n,n_obs,area", RESET_CASES, ids=_ids(RESET_CASES))
def test_reset_matches_oracle_stream_large_team(cuda, kind, n, n_obs, area):
    """dgppo_env_reset_checked, B = 16, under the rules of test_reset_matches_oracle_stream / test_variant_reset_...: agent
    and goal positions from the integer stream bit-exact, trig-derived fields within 1e-6, the failure counter zero"""
    from dgppo_amd import ops_env as O
    cfg, ocfg = _mk(kind, n, n_obs, area)
    B = 16
    seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    agent = torch.full((B, n, cfg.state_dim), float("nan"), device=cuda)
    goal = torch.full((B, cfg.n_goals, cfg.state_dim), float("nan"), device=cuda)
    obst = torch.full((B, cfg.n_obs, cfg.obst_stride), float("nan"), device=cuda)
    nf = torch.zeros(1, dtype=torch.int32, device=cuda)
    O.env_reset(cfg, torch.from_numpy(seeds.view(np.int64)).to(cuda), agent, goal, obst, nf)
    torch.cuda.synchronize()
    assert int(nf.item()) == 0
    wa, wg, wo = E.env_reset(ocfg, [int(s) for s in seeds])
    ga, gg, go = agent.cpu().numpy(), goal.cpu().numpy(), obst.cpu().numpy()
    if ocfg.is_bicycle:
        np.testing.assert_array_equal(ga[..., :2], wa[..., :2])
        np.testing.assert_allclose(ga, wa, atol=1e-6)
    else:
        np.testing.assert_array_equal(ga, wa)                       # integer RNG stream + exact fp32 arithmetic
    np.testing.assert_array_equal(gg, wg)
    if kind == "MPEFormation":
        np.testing.assert_allclose(go, wo, atol=0, rtol=0)
    elif kind == "LidarLine":
        # rectangle corners from device cosf / sinf.  The 1e-6 of test_variant_reset_matches_oracle_stream is for coordinates
        # below 2; here they reach 20 (one fp32 ulp there is 1.9e-6).  The oracle's own fp32 corners are 9.41e-7 from a float64
        # evaluation of the same formula on these 16 scenes: 4 x that
        np.testing.assert_array_equal(go[..., :5], wo[..., :5])     # centre, w, h, theta from the integer stream
        np.testing.assert_allclose(go, wo, atol=4 * 9.41e-7, rtol=0)
    elif ocfg.is_lidar:
        np.testing.assert_array_equal(go[..., :5], wo[..., :5])     # centre, w, h, theta from the integer stream
        np.testing.assert_allclose(go, wo, atol=1e-6)               # cos / sin / corner points: device trig
    else:
        np.testing.assert_array_equal(go, wo)
    d = np.linalg.norm(ga[:, :, None, :2] - ga[:, None, :, :2], axis=-1) + 10.0 * np.eye(n)
    assert d.min() >= cfg.reset_min_dist * (1 - 1e-6), "agents closer than the reset distance"


def test_reset_refusal_follows_the_coverage_formula(cuda):
    """coverage above 0.50 is refused on the host before any launch.  At the default area of 1.5 the formula admits every
    team up to 64 agents (coverage 0.23 at 64: n * pi * 0.055^2 / 1.61^2), so no LiDAR / MPE base kind is refused there; the
    first refusal inside the admitted team sizes is MPEConnectSpread at its default area of 1.0, whose agents start in a strip
    0.175 high: 16 agents.  Its message is asserted, and its outputs stay untouched."""
    from dgppo_amd import _native as N, ops_env as O
    assert all(_coverage(N.make_env_cfg(kind, 64, 3)) <= 0.5 for kind in range(8))
    first = next(n for n in range(1, 65) if _coverage(N.make_env_cfg(9, n, 3)) > 0.5)
    assert first == 16
    cfg = N.make_env_cfg(9, first, 3)
    agent = torch.full((4, first, 4), float("nan"), device=cuda)
    goal = torch.full((4, first, 4), float("nan"), device=cuda)
    obst = torch.full((4, 1, 4), float("nan"), device=cuda)
    with pytest.raises(ValueError, match=r"16 agents with minimum separation 0\.115 cannot be placed in 1\.00 x 0\.1\d by rejection "
                                         r"sampling \(disc coverage 0\.5\d of the area; the limit used here is 0\.50\)"):
        O.env_reset(cfg, torch.arange(1, 5, dtype=torch.int64, device=cuda), agent, goal, obst)
    torch.cuda.synchronize()
    assert torch.isnan(agent).all() and torch.isnan(goal).all() and torch.isnan(obst).all()


# ---- 3. dgppo_graph_feats ---------------------------------------------------------------------------------------------------
FEATS_CASES = [("LidarSpread", 64, 3, 4.0), ("LidarTarget", 64, 3, 4.0), ("LidarBicycleTarget", 64, 8, 4.0),
               ("MPETarget", 64, 13, 4.0), ("MPEConnectSpread", 48, 3, 3.0), ("LidarSpread", 61, 3, 4.0)]


def _edge_of_slot(cfg):
    """[n, S] index into the oracle graph's edge list of slot s of agent i: E.get_graph lays its edges out as the agent-agent
    block (receiver-major), the agent-goal block, the agent-obstacle block"""
    n, gs, os_ = cfg.n_agents, cfg.goal_slots, cfg.obs_slots
    i = np.arange(n)[:, None]
    return np.concatenate([i * n + np.arange(n)[None], n * n + i * gs + np.arange(gs)[None],
                           n * n + n * gs + i * os_ + np.arange(os_)[None]], axis=1)


@pytest.mark.parametrize("kind,n,n_obs,area", FEATS_CASES, ids=_ids(FEATS_CASES))
def test_graph_feats_matches_oracle_graph_large_team(cuda, kind, n, n_obs, area):
    """dgppo_graph_feats through ops_nn.graph_feats on a [B, T, ...] record with n_time = 3, a permuted env_ids, contiguous
    and strided agent / hits views, Fp = node_dim and Fp = 32, against E.get_graph on the same states regrouped per
    (agent, slot): emask == "the edge's receiver is not the pad node" exactly, efeat bit-equal on unmasked slots, Xa / Xo
    bit-equal to the graph's node rows with zero padding to Fp.  The regrouping is pinned by the oracle itself: on every
    unmasked edge its sender is T.attn_sender_nodes' node for that slot and its receiver the agent."""
    from dgppo_amd import ops_nn as K_
    cfg, ocfg, agent0, goal, obst, hits0, action, want = _scene(kind, n, n_obs, area)
    B, Tn, sd, k = 8, 3, cfg.state_dim, cfg.top_k
    assert (cfg.num_nodes - 1) * 32 < 65536 and n * cfg.fan_in < 65536       # the reciprocal-multiply index divisions are exact
    has_hits = hits0 is not None
    # record: the scene, its oracle successor, and the scene with agents moved a little (sensed again)
    ag = np.stack([agent0, want["next_agent"], agent0], 1).copy()
    ag[:, 2, :, :2] += f32(0.03)
    tab = E.ray_table(32)
    hi = None
    if has_hits:
        hi = np.stack([hits0, want["next_hits"], E.lidar_sense(ocfg, ag[:, 2, :, :2], obst, *tab)[0]], 1)
    env_ids = np.array([5, 2, 7, 0, 3], dtype=np.int32)
    Ne = len(env_ids)
    graphs = [E.get_graph(ocfg, ag[env_ids, t], goal[env_ids], None if obst is None else obst[env_ids],
                          hi[env_ids, t] if has_hits else None) for t in range(Tn)]
    gr = {key: np.stack([g[key] for g in graphs], 1) for key in ("nodes", "edges", "receivers", "senders")}   # [Ne, Tn, ...]
    eos, pad = _edge_of_slot(cfg), cfg.num_nodes - 1
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread).numpy()
    recv, send, edges = gr["receivers"][:, :, eos], gr["senders"][:, :, eos], gr["edges"][:, :, eos]          # [Ne, Tn, n, S(, 4)]
    on = recv != pad
    assert on.any() and (~on).any()
    assert (recv[on] == np.broadcast_to(np.arange(n)[:, None], recv.shape)[on]).all()
    assert (send[on] == np.broadcast_to(snd, send.shape)[on]).all() and ((send == pad) == ~on).all()
    G, S, n_other = Ne * Tn, cfg.fan_in, cfg.num_nodes - 1 - n
    d_goal, d_obst = _to(goal, cuda), _to(obst, cuda)
    ids = torch.from_numpy(env_ids).to(cuda)
    for strided in (False, True):
        if strided:                                    # the record as a slice of a wider allocation: larger env / time strides
            wide_a = torch.full((B, Tn + 1, n + 2, sd), float("nan"), device=cuda)
            agd = wide_a[:, :Tn, 1:n + 1]
            agd.copy_(_to(ag, cuda))
            a_se, a_st = (Tn + 1) * (n + 2) * sd, (n + 2) * sd
            hid = h_se = h_st = None
            if has_hits:
                wide_h = torch.full((B, Tn + 2, n, k, 2), float("nan"), device=cuda)
                hid = wide_h[:, 1:Tn + 1]
                hid.copy_(_to(hi, cuda))
                h_se, h_st = (Tn + 2) * n * k * 2, n * k * 2
        else:
            agd, hid = _to(ag, cuda), _to(hi, cuda)
            a_se, a_st, h_se, h_st = Tn * n * sd, n * sd, Tn * n * k * 2, n * k * 2
        for Fp in (cfg.node_dim, 32):
            Xa = torch.full((G * n, Fp), float("nan"), device=cuda)
            Xo = torch.full((G * n_other, Fp), float("nan"), device=cuda)
            ef = torch.full((G * n, S, 4), float("nan"), device=cuda)
            em = torch.full((G * n, S), float("nan"), device=cuda)
            K_.graph_feats(cfg, agd, a_se, a_st, d_goal, d_obst, hid, h_se or 0, h_st or 0, ids, Ne, Tn, Xa, Xo, ef, em, Fp)
            torch.cuda.synchronize()
            tag = f"strided={strided} Fp={Fp}"
            em_np = em.cpu().numpy().reshape(Ne, Tn, n, S)
            np.testing.assert_array_equal(em_np, on.astype(f32), err_msg=f"emask {tag}")
            ef_np = ef.cpu().numpy().reshape(Ne, Tn, n, S, 4)
            _bits_equal(ef_np[on], np.ascontiguousarray(edges[on]), f"efeat {tag}")
            rows = np.zeros((Ne, Tn, cfg.num_nodes - 1, Fp), f32)
            rows[..., :cfg.node_dim] = gr["nodes"][:, :, :pad]
            _bits_equal(Xa.cpu().numpy().reshape(Ne, Tn, n, Fp), np.ascontiguousarray(rows[:, :, :n]), f"Xa {tag}")
            _bits_equal(Xo.cpu().numpy().reshape(Ne, Tn, n_other, Fp), np.ascontiguousarray(rows[:, :, n:]), f"Xo {tag}")


# ---- 4. dgppo_gae -----------------------------------------------------------------------------------------------------------
def _gae_inputs(B, T_, n, nh, seed):
    r = np.random.default_rng(seed)
    return (r.uniform(-1, 1, size=(B, T_, n, nh)).astype(f32), (-r.uniform(0, 0.02, size=(B, T_))).astype(f32),
            r.uniform(-1, 1, size=(B, T_ + 1, n, nh)).astype(f32), r.uniform(0, 1, size=(B, T_ + 1)).astype(f32))


GAE_CASES = [
    # column family at wide rows: 129 / 193 columns per env, every (rows per lane, lanes per column) instance
    (2, 128, 64, 2, 0.95, "cols"), (2, 129, 64, 2, 0.95, "cols"), (2, 256, 64, 3, 0.5, "cols"), (3, 1, 64, 2, 0.95, "cols"),
    (3, 33, 61, 2, 1.0, "cols"),
    (3, 40, 24, 2, 0.3, "generic"),                  # lambda < 0.5 and n * nh > 32: generic below 64 KB
    (2, 128, 64, 2, 0.3, "generic"),                 # generic through the dynamic-LDS opt-in
    (2, 255, 16, 2, 0.3, "generic-after-rows"),      # the rows family's own stage exceeds 64 KB
    (2, 257, 64, 2, 0.95, "generic"),                # just past the column family, also above 64 KB
]


@pytest.mark.parametrize("B,T_,n,nh,lam,family", GAE_CASES, ids=[f"T{c[1]}-n{c[2]}-nh{c[3]}-lam{c[4]}" for c in GAE_CASES])
def test_gae_large_team(cuda, B, T_, n, nh, lam, family):
    """dgppo_gae against A.gae_batch at atol 1e-5 on NaN-prefilled outputs, as tests/test_algo_gpu.py test_gae"""
    from dgppo_amd import ops_algo as O
    fam, lds = _gae_family(T_, n, nh, lam)
    assert fam == family, (fam, lds)
    if (T_, n, nh, lam) == (128, 64, 2, 0.3):
        assert GAE_STATIC_LDS < lds == 4 * (129 * 128 + 129 + 256) and round(lds / 1000, 1) == 67.6
    if family == "generic-after-rows":
        assert n * nh == 32 and 4 * (T_ * 32 + (T_ + 1) * 32 + (T_ + 1) + T_ + 2 * 16 * 33) > GAE_STATIC_LDS
    if T_ == 257:
        assert lds > GAE_STATIC_LDS
    costs, rew, Vh, Vl = _gae_inputs(B, T_, n, nh, B + T_ + n)
    Qh_w, Ql_w = A.gae_batch(costs, rew, Vh, Vl, 0.99, lam)
    d = lambda x: torch.from_numpy(x).to(cuda)
    Qh = torch.full((B, T_, n, nh), float("nan"), device=cuda)
    Ql = torch.full((B, T_), float("nan"), device=cuda)
    O.gae(d(costs), d(rew), d(Vh), d(Vl), O.lam_pow_table(lam, T_, cuda), 0.99, lam, Qh, Ql)
    np.testing.assert_allclose(Qh.cpu().numpy(), Qh_w, rtol=0, atol=1e-5)
    np.testing.assert_allclose(Ql.cpu().numpy(), Ql_w, rtol=0, atol=1e-5)


def test_gae_refuses_more_than_150_kb(cuda):
    """(T, n, nh) = (300, 64, 2) needs 4 * (301 * 128 + 301 + 256) = 156 340 bytes in the generic kernel: refused on the host,
    outputs still all NaN"""
    from dgppo_amd import ops_algo as O
    B, T_, n, nh = 1, 300, 64, 2
    fam, lds = _gae_family(T_, n, nh, 0.95)
    assert fam == "refused" and lds == 156340 > GAE_MAX_LDS
    costs, rew, Vh, Vl = _gae_inputs(B, T_, n, nh, 1)
    d = lambda x: torch.from_numpy(x).to(cuda)
    Qh = torch.full((B, T_, n, nh), float("nan"), device=cuda)
    Ql = torch.full((B, T_), float("nan"), device=cuda)
    with pytest.raises(ValueError, match="too large for LDS"):
        O.gae(d(costs), d(rew), d(Vh), d(Vl), O.lam_pow_table(0.95, T_, cuda), 0.99, 0.95, Qh, Ql)
    torch.cuda.synchronize()
    assert torch.isnan(Qh).all() and torch.isnan(Ql).all()


# ---- 5. dgppo_advantage_lagr / dgppo_lagr_update ----------------------------------------------------------------------------
def _lagr_inputs(B, T_, n, nh, seed):
    r = np.random.default_rng(seed)
    Ql = r.normal(size=(B, T_)).astype(f32); Vl = r.normal(size=(B, T_ + 1)).astype(f32)
    Qh = r.normal(size=(B, T_, n, nh)).astype(f32); Vh = r.normal(size=(B, T_ + 1, n, nh)).astype(f32)
    lagr = r.uniform(0, 1, size=(n, nh)).astype(f32)
    return r, Ql, Vl, Qh, Vh, lagr


@pytest.mark.parametrize("B,T_,n,nh", [(3, 32, 33, 2), (2, 128, 64, 2), (2, 16, 64, 3), (2, 7, 22, 3)])
def test_advantage_lagr_wide_teams(cuda, B, T_, n, nh):
    """66 to 192 columns — the first refused before the per-series arrays held every admitted team — against A.advantage_lagr"""
    from dgppo_amd import ops_algo as O
    assert 64 < n * nh <= ADV_LAGR_MAX_COLS
    _, Ql, Vl, Qh, Vh, lagr = _lagr_inputs(B, T_, n, nh, B + T_ + n)
    d = lambda x: torch.from_numpy(x).to(cuda)
    adv = torch.full((B, T_, n), float("nan"), device=cuda); Ah = torch.full((B, T_, n, nh), float("nan"), device=cuda)
    O.advantage_lagr(d(Ql), d(Vl), d(Qh), d(Vh), d(lagr), adv, Ah)
    wA, wAh = A.advantage_lagr(Ql, Vl, Qh, Vh, lagr)
    np.testing.assert_allclose(Ah.cpu().numpy(), wAh, atol=1e-5)
    np.testing.assert_allclose(adv.cpu().numpy(), wA, atol=1e-5)


def test_advantage_lagr_keeps_its_bits_up_to_64_columns(cuda):
    """(B, T, n, nh) = (7, 32, 8, 2), the inputs of test_lagrangian_kernels: bit-equal to the outputs of the kernel as it
    was while its per-series arrays held 64 columns (tests/golden/advantage_lagr_7x32x8x2.npz, recorded on an MI355X from
    that build next to this one in the same session) — sizing the arrays for 192 columns changed no arithmetic."""
    from dgppo_amd import ops_algo as O
    _, Ql, Vl, Qh, Vh, lagr = _lagr_inputs(7, 32, 8, 2, 3)
    d = lambda x: torch.from_numpy(x).to(cuda)
    adv = torch.full((7, 32, 8), float("nan"), device=cuda); Ah = torch.full((7, 32, 8, 2), float("nan"), device=cuda)
    O.advantage_lagr(d(Ql), d(Vl), d(Qh), d(Vh), d(lagr), adv, Ah)
    rec = np.load(os.path.join(HERE, "golden", "advantage_lagr_7x32x8x2.npz"))
    _bits_equal(adv.cpu().numpy(), rec["adv"], "adv")
    _bits_equal(Ah.cpu().numpy(), rec["Ah"], "Ah")


@pytest.mark.parametrize("n,nh", [(64, 2), (64, 3)])
def test_lagr_update_wide_teams(cuda, n, nh):
    """dgppo_lagr_update and its halves dgppo_lagr_sums / dgppo_lagr_apply at 128 and 192 columns against A.lagr_update,
    with the tolerance of test_lagrangian_kernels; the second step drives some multipliers to the clip at 0"""
    from dgppo_amd import _native as N, ops_algo as O
    B, T_ = 5, 16
    r, _, _, _, Vh, lagr0 = _lagr_inputs(B, T_, n, nh, 7 + nh)
    Ah = r.normal(size=(B, T_, n, nh)).astype(f32)
    lp_new = (r.normal(size=(B, T_, n)) * 0.3).astype(f32); lp_old = (r.normal(size=(B, T_, n)) * 0.3).astype(f32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    lg, sums = d(lagr0.copy()), torch.zeros(n * nh, device=cuda)
    lg2, sums2 = d(lagr0.copy()), torch.zeros(n * nh, device=cuda)
    lagr = lagr0
    dVh, dAh, dn, do = d(Vh), d(Ah), d(lp_new), d(lp_old)
    st = N.stream_ptr
    for lr in (0.5, 50.0):
        O.lagr_update(dn, do, dVh, dAh, lg, sums, 0.99, lr)
        for e0, e1 in ((0, 2), (2, B)):                         # two unequal shares into one `sums`, then one apply
            rc = N.lib().dgppo_lagr_sums(N.ptr(dn[e0:e1].contiguous()), N.ptr(do[e0:e1].contiguous()), N.ptr(dVh[e0:e1].contiguous()),
                                         (T_ + 1) * n * nh, N.ptr(dAh[e0:e1].contiguous()), N.ptr(sums2), e1 - e0, T_, n, nh,
                                         N.C.c_float(1.0 - 0.99), st())
            N.check(rc, "dgppo_lagr_sums")
        torch.cuda.synchronize()
        rc = N.lib().dgppo_lagr_apply(N.ptr(lg2), N.ptr(sums2), n * nh, N.C.c_int64(B * T_), N.C.c_float(lr), st())
        N.check(rc, "dgppo_lagr_apply")
        lagr = A.lagr_update(lagr, lp_new, lp_old, Vh[:, :T_], Ah, 0.99, lr)
        tol = 1e-5 * max(1.0, float(np.abs(lagr).max()))
        np.testing.assert_allclose(lg.cpu().numpy(), lagr, atol=tol)
        np.testing.assert_allclose(lg2.cpu().numpy(), lagr, atol=tol)
        assert float(sums.abs().max()) == 0.0 and float(sums2.abs().max()) == 0.0
    assert (lagr == 0).any() and (lagr > 0).any()


# ---- 6. engine level --------------------------------------------------------------------------------------------------------
def _setup_engine(kind_name, n, n_obs, area, T_, cuda, batch_size, rnn_step, algo, **hyper):
    """tests/test_large_team_gpu.py _setup with an explicit area and algorithm"""
    from dgppo_amd import _native as N, engine as EN, init
    kind = N.ENV_KINDS[kind_name]
    if area is None:
        cfg, ocfg = N.make_env_cfg(kind, n, n_obs), E.EnvCfg(kind, n_agents=n, n_obs=n_obs)
    else:
        cfg, ocfg = _mk(kind_name, n, n_obs, area)
    hp = EN.Hyper(batch_size=batch_size, rnn_step=rnn_step, train_steps=100, use_rnn=True, rnn_layers=1, use_lstm=False, **hyper)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo=algo, multi_stream=(algo == "informarl_lagr"))
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, 1, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=1, lstm=False)}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    trees = {k: jitter(v) for k, v in trees.items()}
    trees["policy"]["params"]["ScaleHid"]["kernel"] = T.orthogonal(torch.Generator().manual_seed(1), 64, 64, 0.5)
    if algo == "informarl_lagr":
        gen = torch.Generator().manual_seed(21)
        trees["Vh"] = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen),
                                 T.init_value(5, cfg.node_dim, cfg.n_cost, 1, global_info=True))
    for k, net in eng.nets.items():
        net.load_tree(trees[k])
    eng.set_entropy_noise(77)
    return cfg, ocfg, hp, eng, trees


def _grad_hook(eng):
    grads = {}

    def hook(name, net, mb):
        if mb == 0:
            grads[name] = net.to_tree(net.grads)
    eng.grad_hook = hook
    return grads


@pytest.mark.parametrize("kind,n,n_obs,area", [("LidarSpread", 33, 3, 2.5), ("MPEConnectSpread", 22, 3, 2.0)],
                         ids=["LidarSpread-33", "MPEConnectSpread-22"])
def test_informarl_lagr_large_team(cuda, kind, n, n_obs, area):
    """test_informarl_lagr_targets_gradients_and_multipliers at the first team sizes whose n * n_cost exceeds 64 (66 columns
    both): targets 1e-5, the Lagrangian advantage on identical inputs 1e-5 and end to end within the propagated bound,
    first-minibatch gradients 5e-5 of scale, the multiplier step after the policy update."""
    B, T_, rs = 4, 8, 4
    bs = B * T_                                                       # ONE minibatch: the multiplier is checked after it
    cfg, ocfg, hp, eng, trees = _setup_engine(kind, n, n_obs, area, T_, cuda, bs, rs, "informarl_lagr", lagr_init=0.4, lr_lagr=0.05)
    assert n * cfg.n_cost == 66 > 64
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3).finalize()
    r = _np_rollout(ro)
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, rnn_step=rs, clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    lagr0 = eng.lagr.cpu().numpy().copy()
    assert lagr0.shape == (n, cfg.n_cost) and np.all(lagr0 == f32(0.4))
    tg = eng.targets_lagr(ro, 0)
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), v) for k, v in trees.items()}
    wt = R.targets_lagr(leaf, ocfg, r, hpd, lagr0)
    for k in ("Vl", "Vh", "Ql", "Qh"):
        _close_np(tg[k], wt[k], k)
    g = {k: tg[k].cpu().numpy() for k in ("Vl", "Vh", "Ql", "Qh", "adv", "Ah")}
    same_A, same_Ah = A.advantage_lagr(g["Ql"], g["Vl"], g["Qh"], g["Vh"], lagr0)
    _close_np(g["adv"], same_A, "lagr advantage kernel on identical inputs")
    _close_np(g["Ah"], same_Ah, "Ah kernel on identical inputs")
    stdh = (wt["Qh"] - wt["Vh"][:, :-1]).std(axis=1, keepdims=True) + 1e-8
    bound_h = 4.0 * (np.abs(g["Qh"] - wt["Qh"]).max() + np.abs(g["Vh"] - wt["Vh"]).max()) / stdh + 1e-5
    assert (np.abs(g["Ah"] - wt["Ah"]) <= bound_h).all()
    perm = np.arange(B)
    grads = _grad_hook(eng)
    tg_np = {k: v.cpu().numpy() for k, v in tg.items()}
    R.minibatch_losses_lagr(leaf, ocfg, r, tg_np, perm, hpd, eng.eps_hat.cpu())
    info = eng.update(ro, None, 0, perm)
    torch.cuda.synchronize()
    _check_first_minibatch_grads(leaf, grads, ("Vl", "Vh", "policy"))
    for k in ("Vh/loss", "Vh/grad_norm", "Vh/has_nan", "policy/lagr_mean", "Vl/loss", "policy/loss"):
        assert k in info and np.isfinite(info[k]), k
    new_pol = T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), eng.policy.to_tree())
    lp_new = R.log_pi_full_episode({"policy": new_pol}, ocfg, r, perm, eng.eps_hat.cpu())
    want = A.lagr_update(lagr0, lp_new, r["log_pis"], tg_np["Vh"][:, :T_], tg_np["Ah"], hp.gamma, hp.lr_lagr)
    got = eng.lagr.cpu().numpy()
    assert not np.array_equal(got, lagr0)
    np.testing.assert_allclose(got, want, atol=2e-6)
    assert abs(info["policy/lagr_mean"] - float(want.mean())) < 1e-5


def test_informarl_large_team(cuda):
    """test_informarl_targets_and_gradients at MPETarget 30 / 2 (tiled attention backward)"""
    kind, n, n_obs, B, T_, rs, bs = "MPETarget", 30, 2, 4, 8, 4, 16
    cfg, ocfg, hp, eng, trees = _setup_engine(kind, n, n_obs, None, T_, cuda, bs, rs, "informarl", cost_weight=0.3, cost_schedule=True)
    assert set(eng.nets) == {"policy", "Vl"} and _image_bytes(cfg, 32, 3, True) > LDS_IMAGE
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3).finalize()
    step = 60
    w = eng.cost_weight_at(step)
    assert w == pytest.approx(1.5)
    tg = eng.targets_informarl(ro, step)
    r = _np_rollout(ro)
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, rnn_step=rs, clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), trees[k]) for k in ("policy", "Vl")}
    wt = R.targets_informarl(leaf, ocfg, r, hpd, w)
    _close_np(tg["Vl"], wt["Vl"], "Vl")
    _close_np(tg["Ql"], wt["Ql"], "Ql")
    gQl, gVl, gadv = (tg[k].cpu().numpy() for k in ("Ql", "Vl", "adv"))
    Al = gQl - gVl[:, :-1]
    same_in = -((Al - Al.mean(1, keepdims=True)) / (Al.std(1, keepdims=True) + 1e-8))
    _close_np(gadv, np.repeat(same_in[:, :, None], n, axis=-1), "advantage kernel on identical inputs")
    Al_o = wt["Ql"] - wt["Vl"][:, :-1]
    bound = 4.0 * (np.abs(gQl - wt["Ql"]).max() + np.abs(gVl - wt["Vl"]).max()) / (Al_o.std(1, keepdims=True) + 1e-8) + 1e-5
    assert (np.abs(gadv - wt["adv"]) <= bound[:, :, None]).all()
    perm = np.array([2, 0, 3, 1])
    grads = _grad_hook(eng)
    Eb = bs // T_
    tg_np = {k: v.cpu().numpy() for k, v in tg.items()}
    R.minibatch_losses(leaf, ocfg, r, None, tg_np, perm[:Eb], hpd, eng.eps_hat.cpu())
    info = eng.update(ro, None, step, perm)
    assert set(grads) == {"Vl", "policy"} and "Vh/loss_Vh" not in info
    _check_first_minibatch_grads(leaf, grads, ("Vl", "policy"))
    for k in ("Vl/loss", "Vl/grad_norm", "policy/loss", "policy/entropy", "policy/clip_frac"):
        assert k in info and np.isfinite(info[k]), k
    assert float(eng.opt["policy"].state[2]) == B // Eb


def test_hcbfcrpo_large_team(cuda):
    """test_hcbfcrpo_targets_and_gradients at LidarSpread 24 / 3: Vh := get_cost(graph), the final one from an env step"""
    kind, n, n_obs, B, T_, rs, bs = "LidarSpread", 24, 3, 4, 8, 4, 16
    cfg, ocfg, hp, eng, trees = _setup_engine(kind, n, n_obs, None, T_, cuda, bs, rs, "hcbfcrpo")
    assert _image_bytes(cfg, 32, 3, True) > LDS_IMAGE and _step_family(cfg) == "lidar_wg"
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3).finalize()
    step = 80                                                       # past 75 %: schedule weight x4
    tg = eng.targets_hcbfcrpo(ro, step)
    r = _np_rollout(ro)
    hpd = dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, alpha=hp.alpha, cbf_eps=hp.cbf_eps, rnn_step=rs,
               clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)
    leaf = {k: T.tree_map(lambda t: t.clone().requires_grad_(), trees[k]) for k in ("policy", "Vl")}
    assert eng.cbf_weight_at(step) == 4.0
    wt = R.targets_hcbfcrpo(leaf, ocfg, r, hpd, 4.0)
    np.testing.assert_array_equal(tg["Vh"].cpu().numpy()[:, :T_], r["costs"])            # stored costs ARE get_cost(graph)
    np.testing.assert_allclose(tg["Vh"].cpu().numpy()[:, T_], wt["Vh"][:, T_], atol=1e-6)   # cost of next_graph[-1]
    for k in ("Vl", "Ql", "Qh"):
        _close_np(tg[k], wt[k], k)
    _check_advantage(tg, wt, ocfg.dt, hp.alpha, hp.cbf_eps, 4.0, "hcbfcrpo " + kind)
    perm = np.array([2, 0, 3, 1])
    grads = _grad_hook(eng)
    Eb = bs // T_
    tg_np = {k: v.cpu().numpy() for k, v in tg.items()}
    R.minibatch_losses(leaf, ocfg, r, None, tg_np, perm[:Eb], hpd, eng.eps_hat.cpu())
    info = eng.update(ro, None, step, perm)
    _check_first_minibatch_grads(leaf, grads, ("Vl", "policy"))
    assert "eval/safe_data" in info and "Vh/loss_Vh" not in info and abs(info["eval/safe_data"] - wt["safe"]) < 0.05
