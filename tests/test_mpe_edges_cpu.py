"""The scene catalogue of tests/mpe_edge_scenes.py really reaches the paths it is built for — decided on the oracle alone, before
any kernel is involved: masks that flip one ulp around the radii, costs either side of the jump of cost_value and of the -1
clip, the connectivity cost at its radius, goals one ulp around dist2goal, walls and velocity limits that engage, actions on
the clip, NaN exactly where a non-finite input puts it — and every scene present for every config that supports it."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import env_np as E

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mpe_edge_scenes as S  # noqa: E402

f32 = np.float32
# (kind, n_agents, n_obs): the configs of tests/test_mpe_edges_gpu.py
CONFIGS = [("MPESpread", 4, 2), ("MPETarget", 3, 0), ("MPETarget", 4, 2), ("MPELine", 3, 2), ("MPELine", 5, 2),
           ("MPEFormation", 4, 2), ("MPECorridor", 4, 2), ("MPEConnectSpread", 4, 1), ("MPESpread", 9, 3)]
IDS = ["-".join(map(str, c)) for c in CONFIGS]
THREE = ("below", "on", "above")
pytestmark = pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)


@functools.lru_cache(maxsize=None)
def _catalogue(kind, n, n_obs):
    ocfg = E.EnvCfg(E.KIND_NAMES[kind], n_agents=n, n_obs=n_obs)
    agent, goal, obst, action, tags = S.build(ocfg, 11)
    with np.errstate(all="ignore"):
        step = E.env_step(ocfg, agent, goal, obst, None, action)
    d = dict(ocfg=ocfg, agent=agent, goal=goal, obst=obst, action=action, tags=tags, **step)
    for v in list(d.values()) + list(step["graph"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _env(c, tag):
    (b,) = [b for b, t in enumerate(c["tags"]) if t == tag]
    return b


def _expected_tags(ocfg):
    """every scene instance a config must hold, from the table of mpe_edge_scenes.supports"""
    t = [f"comm-radius/{k}" for k in THREE] + [f"agent-cost-zero/{k}" for k in THREE]
    if S.supports(ocfg, "obs-mask-radius"):
        t += ["obs-mask-radius/far"] if S.always_connected(ocfg) else [f"obs-mask-radius/{k}" for k in THREE]
    t += [f"obs-cost-zero/{k}" for k in THREE] if ocfg.n_obs > 0 else ["obs-cost-zero/no-obstacle"]
    t += [f"cost-floor/{k}" for k in THREE + ("kept", "clipped")]
    t += ["coincident/agents"] + (["coincident/on-obstacle"] if S.supports(ocfg, "coincident/on-obstacle") else [])
    if S.supports(ocfg, "connectivity"):
        t += [f"connectivity/{k}" for k in THREE + ("straggler", "cluster")]
    t += [f"goal-reached/{k}" for k in (("inside", "outside") if ocfg.kind == E.MPE_FORMATION else ("zero",) + THREE)]
    t += ["goal-reached/tie"] if S.supports(ocfg, "goal-reached/tie") else []
    t += ["walls/position", "walls/velocity", "action-clip", "clean"]
    t += [f"non-finite/{k}" for k in S.NON_FINITE if S.supports(ocfg, f"non-finite/{k}")]
    return t


def test_every_scene_is_present_and_at_rest(cfg):
    c = _catalogue(*cfg)
    ocfg, tags, B = c["ocfg"], c["tags"], len(c["tags"])
    n = ocfg.n_agents
    assert c["agent"].shape == (B, n, 4) and c["goal"].shape == (B, ocfg.n_goals, 4) and c["action"].shape == (B, n, 2)
    assert (c["obst"] is None) if ocfg.n_obs == 0 else (c["obst"].shape == (B, ocfg.n_obs, 4))
    assert all(a.dtype == f32 for a in (c["agent"], c["goal"], c["action"]))
    # no scene dropped silently: the scenes of SCENES the config supports, and every instance of each
    assert {t.split("/")[0] for t in tags} == {s for s in S.SCENES if S.supports(ocfg, s)}
    assert set(tags) == set(_expected_tags(ocfg)), set(_expected_tags(ocfg)) ^ set(tags)
    assert 24 <= B <= 48
    if cfg[0] != "MPEConnectSpread":
        assert "connectivity" not in {t.split("/")[0] for t in tags}
    clean, nf = S.env_ids(tags, "clean"), S.env_ids(tags, "non-finite")
    assert len(clean) == S.N_CLEAN and clean[0] < nf[0] and clean[-1] == nf[-1] + 1 == B - 1
    assert clean[1] == nf[0] - 1 and nf[0] < clean[2] < nf[-1], "clean envs before, inside and after the non-finite block"
    # exact-position scenes are at rest: a step leaves every agent where the scene put it
    still = [b for b, t in enumerate(tags) if t.split("/")[0] not in ("walls", "clean", "non-finite")]
    assert (c["agent"][still][..., 2:] == 0).all()
    np.testing.assert_array_equal(c["next_agent"][still][..., :2].view(np.uint32), c["agent"][still][..., :2].view(np.uint32))
    # the agents a scene does not use keep out of everybody's comm_radius
    for b in still:
        if c["tags"][b].startswith(("connectivity", "goal-reached")):
            continue
        p = c["agent"][b, 2:, :2].astype(np.float64)
        d = np.linalg.norm(p[:, None] - c["agent"][b][None, :, :2], axis=-1)
        assert (d[d > 0] > ocfg.comm_radius + 0.1).all(), tags[b]


def _pair_distance(c, b, i=0, j=1):
    a = c["agent"][b]
    return E.norm2(a[i, 0] - a[j, 0], a[i, 1] - a[j, 1])


def _obst_distance(c, b, o, i=0):
    return E.norm2(c["agent"][b, i, 0] - c["obst"][b, o, 0], c["agent"][b, i, 1] - c["obst"][b, o, 1])


def test_mask_radius_scenes_flip_the_oracles_masks(cfg):
    c = _catalogue(*cfg)
    ocfg, g = c["ocfg"], c["graph"]
    n, pad = ocfg.n_agents, ocfg.num_nodes - 1
    ids = [_env(c, f"comm-radius/{k}") for k in THREE]
    assert [_pair_distance(c, b) for b in ids] == list(S.three(ocfg.comm_radius))
    for e in (0 * n + 1, 1 * n + 0):                                  # edges agent 0 <- agent 1 and back
        assert (g["receivers"][ids, e] != pad).tolist() == [True, False, False], "d < comm_radius one ulp below it only"
    diag = [i * n + i for i in range(n)]
    assert (g["receivers"][:, diag] == pad).all(), "eye_offset shuts the diagonal"
    ob0 = n * n + ocfg.n_goal_edges                                   # agent 0's edge from obstacle 0
    if not S.supports(ocfg, "obs-mask-radius"):
        assert ocfg.n_obs == 0 and g["receivers"].shape[1] == ob0
    elif S.always_connected(ocfg):
        b = _env(c, "obs-mask-radius/far")
        dist = [_obst_distance(c, b, o, i) for o in range(ocfg.n_obs) for i in range(n)]
        assert min(dist) > 2 * ocfg.comm_radius and max(dist) < ocfg.obs_mask_radius
        assert (g["receivers"][b, ob0:] != pad).all(), "obstacle edges are always connected in this kind"
    else:
        ids = [_env(c, f"obs-mask-radius/{k}") for k in THREE]
        assert [_obst_distance(c, b, 0) for b in ids] == list(S.three(ocfg.obs_mask_radius))
        assert (g["receivers"][ids, ob0] != pad).tolist() == [True, False, False]
        assert (g["senders"][ids, ob0] == [n + ocfg.n_goals, pad, pad]).all()


def test_costs_land_on_both_sides_of_the_jump_and_on_the_floor(cfg):
    c = _catalogue(*cfg)
    ocfg, cost = c["ocfg"], c["cost"]
    r2 = f32(ocfg.car_radius * 2)
    ids = [_env(c, f"agent-cost-zero/{k}") for k in THREE]
    d = [_pair_distance(c, b) for b in ids]
    assert d == list(S.three(r2)) and r2 - d[0] > 0 and r2 - d[1] == 0 and r2 - d[2] < 0, "margin: one ulp above, zero, below"
    for i in (0, 1):
        assert cost[ids, i, 0].tolist() == [0.5, -0.5, -0.5], "the cost jumps by 1.0 at a zero margin"
    if ocfg.n_obs == 0:
        assert (cost[..., 1] == f32(-0.5)).all(), "no obstacle: a zero margin everywhere"
        assert "obs-cost-zero/no-obstacle" in c["tags"]
    else:
        ids = [_env(c, f"obs-cost-zero/{k}") for k in THREE]
        ro, o = S.car_plus_obs(ocfg), ocfg.n_obs - 1
        d = [_obst_distance(c, b, o) for b in ids]
        assert d == list(S.three(ro)) and ro - d[0] > 0 and ro - d[1] == 0 and ro - d[2] < 0
        assert cost[ids, 0, 1].tolist() == [0.5, -0.5, -0.5]
    # the lower clip: before it, values above -1, on it and below it; after it -1.0 exactly, and one value kept
    ids = [_env(c, f"cost-floor/{k}") for k in THREE + ("kept", "clipped")]
    d = [_pair_distance(c, b) for b in ids]
    assert d[:3] == list(S.three(S.floor_radius(ocfg)))
    before = [S.agent_cost_before_clip(ocfg, x) for x in d]
    assert f32(-1.0) in before[:3] and before[3] > -1 and before[4] < -1, before
    assert not S.agent_cost_before_clip(ocfg, np.nextafter(d[3], f32(1))) > -1, "the farthest distance whose cost is kept"
    for i in (0, 1):
        np.testing.assert_array_equal(cost[ids, i, 0], np.maximum(np.asarray(before, f32), f32(-1)))
    assert (cost[ids[:3] + ids[4:], 0, 0] == -1.0).all() and cost[ids[3], 0, 0] == before[3]
    if ocfg.kind != E.MPE_CONNECT_SPREAD:
        b = _env(c, "coincident/agents")
        assert cost[b, 0, 0] == f32(r2 + f32(0.5)) and cost[b, 0, 0] < 1, "nothing clips an MPE cost from above"


def test_coincident_bodies(cfg):
    c = _catalogue(*cfg)
    ocfg, g = c["ocfg"], c["graph"]
    n, pad = ocfg.n_agents, ocfg.num_nodes - 1
    b = _env(c, "coincident/agents")
    assert _pair_distance(c, b) == 0 and (c["next_agent"][b, 0] == c["next_agent"][b, 1]).all()
    for e in (0 * n + 1, 1 * n + 0):
        assert g["receivers"][b, e] != pad and (g["edges"][b, e].view(np.uint32) == 0).all(), "mask on, four +0 features"
    if S.supports(ocfg, "coincident/on-obstacle"):
        b = _env(c, "coincident/on-obstacle")
        ob0 = n * n + ocfg.n_goal_edges
        assert _obst_distance(c, b, 0) == 0 and g["receivers"][b, ob0] == 0 and (g["edges"][b, ob0, :2] == 0).all()
        want = f32(S.car_plus_obs(ocfg) + f32(0.5))
        assert c["cost"][b, 0, 1] == (min(want, f32(1)) if ocfg.kind == E.MPE_CONNECT_SPREAD else want)


def test_connectivity_cost_at_its_radius(cfg):
    c = _catalogue(*cfg)
    ocfg = c["ocfg"]
    if not S.supports(ocfg, "connectivity"):
        assert ocfg.n_cost == 2 and c["cost"].shape[-1] == 2 and not S.env_ids(c["tags"], "connectivity")
        return
    ids = [_env(c, f"connectivity/{k}") for k in THREE + ("straggler", "cluster")]
    c2 = c["cost"][ids, :, 2]
    assert (c2 == c2[:, :1]).all(), "one value for the whole team"
    d = [_pair_distance(c, b, 2, 3) for b in ids[:3]]
    assert d == list(S.three(ocfg.connect_radius))
    for b in ids[:3]:                                                 # ... and it is the largest nearest-neighbour distance
        assert _pair_distance(c, b, 0, 1) < f32(0.25) and _pair_distance(c, b, 1, 2) > 0.5
    assert c2[:, 0].tolist()[:4] == [-0.5, -0.5, 0.5, 1.0], "the jump at connect_radius, the straggler on the +1 clip"
    assert -1 < c2[4, 0] < -0.5, "a tight cluster: negative and unclipped"


def _goals_not_reached(ocfg, agent, goal):
    """the reward's indicator sum and the distances it is taken of, as E.get_reward forms them"""
    gp, ap = E.reward_goal_positions(ocfg, goal[None]), agent[None, :, :2]
    if ocfg.is_spread:
        d = E.nan_min(E.norm2(gp[:, :, None, 0] - ap[:, None, :, 0], gp[:, :, None, 1] - ap[:, None, :, 1]), 2)[0]
    else:
        d = E.norm2(gp[..., 0] - ap[..., 0], gp[..., 1] - ap[..., 1])[0]
    return int((d > f32(ocfg.dist2goal)).sum()), d


def test_goal_reached_count_differs_across_the_distances(cfg):
    c = _catalogue(*cfg)
    ocfg, g = c["ocfg"], S.goal_index(c["ocfg"])
    count = lambda b: _goals_not_reached(ocfg, c["agent"][b], c["goal"][b])
    if ocfg.kind == E.MPE_FORMATION:
        (ci, di), (co, do) = count(_env(c, "goal-reached/inside")), count(_env(c, "goal-reached/outside"))
        assert co == ci + 1 and di[g] == f32(ocfg.dist2goal * 0.5) and do[g] == f32(ocfg.dist2goal * 2)
        assert abs(float(di[g]) - ocfg.dist2goal) > 1e-3 and abs(float(do[g]) - ocfg.dist2goal) > 1e-3, "well clear of the threshold"
        return
    ids = [_env(c, f"goal-reached/{k}") for k in ("zero",) + THREE]
    got = [count(b) for b in ids]
    assert [d[g] for _, d in got] == [f32(0)] + list(S.three(ocfg.dist2goal))
    cnt = [k for k, _ in got]
    assert cnt[0] == cnt[1] == cnt[2] == cnt[3] - 1, "reached at d <= dist2goal, not one ulp beyond"
    np.testing.assert_array_equal(c["goal"][ids[1]], c["goal"][ids[3]])
    if S.supports(ocfg, "goal-reached/tie"):
        b = _env(c, "goal-reached/tie")
        a, gl = c["agent"][b], c["goal"][b]
        d0, d1 = (E.norm2(gl[0, 0] - a[i, 0], gl[0, 1] - a[i, 1]) for i in (0, 1))
        assert d0.view(np.uint32) == d1.view(np.uint32) and d0 == f32(0.125) and count(b)[1][0] == d0
    else:
        assert not (ocfg.is_spread and ocfg.reward_goals == E.GOALS_NODES)


def test_wall_velocity_and_action_clips_engage(cfg):
    c = _catalogue(*cfg)
    ocfg, nx = c["ocfg"], c["next_agent"]
    A, Y, v, dt = f32(ocfg.area_size), f32(ocfg.y_limit), f32(ocfg.vel_limit), f32(ocfg.dt)
    b = _env(c, "walls/position")
    a = c["agent"][b]
    free = (a[:, 2:4] * dt + a[:, :2]).astype(f32)                    # before the state clip
    assert (free[0] < 0).all() and (nx[b, 0, :2].view(np.uint32) == 0).all(), "outward at 0: clipped onto +0"
    assert free[1, 0] > A and free[1, 1] > Y and nx[b, 1, 0] == A and nx[b, 1, 1] == Y, "outward at the upper limits"
    assert 0 < nx[b, 2, 0] == free[2, 0] < A, "inward: leaves the wall"
    if Y > A:
        assert Y == 2 * A and a[1, 1] == Y and a[2, 1] == A
        assert A < nx[b, 2, 1] == free[2, 1] < Y and A < nx[b, 3, 1] == free[3, 1] < Y, "y between A and 2 A survives"
    else:
        assert (nx[..., :2][np.isfinite(nx[..., :2])] <= A).all() and nx[b, 2, 1] == free[2, 1] < A
    b = _env(c, "walls/velocity")
    a, u = c["agent"][b], E.clip_action(c["action"][b])
    freev = ((u * f32(10.0)).astype(f32) * dt + a[:, 2:4]).astype(f32)
    assert freev[0, 0] > v and freev[0, 1] < -v and nx[b, 0, 2:].tolist() == [v, -v]
    assert freev[1, 0] < -v and freev[1, 1] > v and nx[b, 1, 2:].tolist() == [-v, v]
    assert np.signbit(a[2, 2:]).all() and np.signbit(c["action"][b, 2, 0])
    assert nx[b, 2, 2].view(np.uint32) == 0x80000000 and nx[b, 2, 3].view(np.uint32) == 0, "-0 + -0 = -0 and +0 + -0 = +0"
    ids = S.env_ids(c["tags"], "action-clip")
    raw = np.concatenate([c["action"][i].reshape(-1) for i in ids])
    clipped = np.concatenate([E.clip_action(c["action"][i]).reshape(-1) for i in ids])
    for val in S.ACTION_VALUES:
        (at,) = np.nonzero(raw.view(np.uint32) == np.asarray(val, f32).view(np.uint32))[:1]
        assert len(at) >= 1, f"{val!r} is in no action"
        want = f32(np.sign(val)) if abs(val) >= 1 else val
        assert (clipped[at].view(np.uint32) == np.asarray(want, f32).view(np.uint32)).all(), val
    assert np.isfinite(c["reward"][ids]).all() and np.isfinite(nx[ids]).all()


def test_non_finite_scenes_put_nan_exactly_where_expected(cfg):
    c = _catalogue(*cfg)
    ocfg, tags, a = c["ocfg"], c["tags"], S.NF_AGENT
    n = ocfg.n_agents
    cost, rew, nx, g = c["cost"], c["reward"], c["next_agent"], c["graph"]
    finite_envs = [b for b, t in enumerate(tags) if not t.startswith("non-finite")]
    for x in (cost, rew, nx, g["nodes"], g["edges"], g["states"]):
        assert np.isfinite(x[finite_envs]).all(), "the other envs stay finite"
    others = [i for i in range(n) if i != a]
    by = {t.split("/")[1]: b for b, t in enumerate(tags) if t.startswith("non-finite/")}
    assert tuple(by) == tuple(k for k in S.NON_FINITE if S.supports(ocfg, f"non-finite/{k}"))

    b = by["position-nan"]                          # every nearest-neighbour minimum meets the NaN distance
    assert np.isnan(cost[b, :, 0]).all() and np.isnan(rew[b])
    if ocfg.n_obs > 0:
        assert np.isnan(cost[b, a, 1]) and np.isfinite(cost[b, others, 1]).all()
    if ocfg.n_cost == 3:
        assert np.isnan(cost[b, :, 2]).all()
    assert np.isnan(nx[b, a, 0]) and np.isnan(nx[b]).sum() == 1
    pad = ocfg.num_nodes - 1
    assert (g["receivers"][b, a * n:(a + 1) * n] == pad).all() and (g["receivers"][b, a:n * n:n] == pad).all(), \
        "no agent-agent edge to or from an agent at NaN"

    for name, col, lim in (("position-inf", 0, f32(ocfg.area_size)), ("position-neg-inf", 1, f32(0))):
        b = by[name]                                # clips onto the wall; its own diagonal distance is inf - inf
        assert nx[b, a, col] == lim and np.isfinite(nx[b]).all()
        assert np.isnan(cost[b, a, 0]) and (cost[b, others, 0] >= -1).all() and np.isfinite(cost[b, others, :2]).all()
        assert ocfg.n_cost == 2 or np.isnan(cost[b, :, 2]).all(), "the team's largest nearest-neighbour distance meets the NaN"

    b = by["velocity-nan"]                          # this step's cost and reward read positions only
    assert np.isfinite(cost[b]).all() and np.isfinite(rew[b])
    assert np.isnan(nx[b, a, [0, 2]]).all() and np.isnan(nx[b]).sum() == 2

    b = by["action-nan"]
    assert np.isnan(nx[b, a, 2]) and np.isnan(nx[b]).sum() == 1 and np.isnan(rew[b]) and np.isfinite(cost[b]).all()

    if "obstacle-nan" in by:
        b = by["obstacle-nan"]
        assert np.isnan(cost[b, :, 1]).all() and np.isfinite(cost[b, :, 0]).all() and np.isfinite(rew[b]) and np.isfinite(nx[b]).all()
        ob0 = n * n + ocfg.n_goal_edges
        assert (g["receivers"][b, ob0::ocfg.n_obs] == pad).all(), "a NaN distance connects nobody, whatever the mask radius"
    b = by["goal-nan"]
    assert np.isnan(rew[b]) and np.isfinite(cost[b]).all() and np.isfinite(nx[b]).all() and np.isnan(g["edges"][b]).any()
