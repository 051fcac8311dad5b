"""The scene catalogue of tests/env_edge_scenes.py really reaches the paths it is built for — decided on the oracle alone, before
any kernel is involved: det == 0 and NaN alphas, clipped determinants, obstacles either side of the wave kernel's 4e-4
robustness test, 32 tied +0 alphas outside every obstacle, tied hits next to NaN rays, the three graze alphas, agents either
side of the reach and ray-cull thresholds, masks that flip one ulp around the radii, NaN exactly where a non-finite input puts it."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import env_np as E

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import env_edge_scenes as S  # noqa: E402

f32 = np.float32
# (kind, n_agents, n_obs, n_rays, top_k): the four wave instances, the generic kernel's 32-ray config, its 16-ray config
CONFIGS = [("LidarSpread", 4, 2, 32, 8), ("LidarTarget", 4, 2, 32, 8), ("LidarBicycleTarget", 4, 3, 32, 8),
           ("LidarSpread", 8, 3, 32, 8), ("LidarLine", 4, 3, 32, 8), ("LidarSpread", 5, 2, 16, 16)]
IDS = ["-".join(map(str, c)) for c in CONFIGS]
FULL = CONFIGS[:5]


def det0_table(ocfg, pos, obst, rc, rs):
    """det0 of every (env, agent, ray, obstacle, segment) before the clip, in the oracle's fp32 order (lidar_alphas)"""
    sr = f32(ocfg.comm_radius)
    x1, y1 = pos[..., 0][..., None], pos[..., 1][..., None]
    x2 = (x1 + (rc * sr).astype(f32)).astype(f32)
    y2 = (y1 + (rs * sr).astype(f32)).astype(f32)
    out = np.zeros(x2.shape + (ocfg.n_obs, 4), f32)
    with np.errstate(all="ignore"):
        for o in range(ocfg.n_obs):
            rec = obst[:, o][:, None, None, :]
            for m in range(4):
                mm = (m - 1) % 4
                x3, y3, x4, y4 = rec[..., 8 + 2 * m], rec[..., 9 + 2 * m], rec[..., 8 + 2 * mm], rec[..., 9 + 2 * mm]
                out[..., o, m] = (((x1 - x2).astype(f32) * (y4 - y3).astype(f32)).astype(f32)
                                  - ((y1 - y2).astype(f32) * (x4 - x3).astype(f32)).astype(f32)).astype(f32)
    return out


@functools.lru_cache(maxsize=None)
def _catalogue(kind, n, n_obs, n_rays, top_k):
    ocfg = E.EnvCfg(E.KIND_NAMES[kind], n_agents=n, n_obs=n_obs, n_rays=n_rays, top_k=top_k)
    only = None if n_rays == 32 else ("axis-aligned", "symmetric-ties")
    agent, goal, obst, action, tags = S.build(ocfg, 11, only=only)
    tab = E.ray_table(n_rays)
    alphas, _ = E.lidar_alphas(ocfg, agent[..., :2], obst, *tab)
    inside = np.zeros(agent.shape[:2], bool)
    for o in range(n_obs):
        inside |= E.rect_inside(agent[..., 0], agent[..., 1], obst[:, o][:, None, :], 0.0)
    d = dict(ocfg=ocfg, agent=agent, goal=goal, obst=obst, action=action, tags=tags, tab=tab, alphas=alphas, inside=inside,
             det0=det0_table(ocfg, agent[..., :2], obst, *tab))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _hit(alphas):
    with np.errstate(invalid="ignore"):
        return alphas < f32(1e6)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_catalogue_shapes_tags_and_rest(cfg):
    c = _catalogue(*cfg)
    ocfg, B = c["ocfg"], len(c["tags"])
    assert c["agent"].shape == (B, ocfg.n_agents, ocfg.state_dim) and c["goal"].shape == (B, ocfg.n_goals, ocfg.state_dim)
    assert c["obst"].shape == (B, ocfg.n_obs, 16) and c["action"].shape == (B, ocfg.n_agents, 2)
    assert all(a.dtype == f32 for a in (c["agent"], c["goal"], c["obst"], c["action"]))
    if cfg in FULL:
        assert {t.split("/")[0] for t in c["tags"]} == set(S.SCENES) and 20 <= B <= 48
        clean = S.env_ids(c["tags"], "clean")
        assert len(clean) == 2 and 0 < clean[0] and clean[1] < B - 1 and clean[1] - clean[0] > 1, "clean envs sit between the others"
    # exact-position scenes are at rest: a step leaves every agent where the scene put it
    still = [b for b, t in enumerate(c["tags"]) if t != "clean" and not t.startswith("non-finite")]
    nxt = E.agent_step_euler(ocfg, c["agent"], E.clip_action(c["action"]))
    np.testing.assert_array_equal(nxt[still][..., :2].view(np.uint32), c["agent"][still][..., :2].view(np.uint32))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_axis_aligned_and_parallel_scenes_reach_det_zero_and_nan(cfg):
    c = _catalogue(*cfg)
    names = ("axis-aligned", "parallel-to-ray") if cfg in FULL else ("axis-aligned",)
    for name in names:
        for b in S.env_ids(c["tags"], name):
            assert (c["det0"][b] == 0).any(), f"{name} env {b}: no det0 == 0"
            assert np.isnan(c["alphas"][b]).any(), f"{name} env {b}: no NaN alpha"
    for b in S.env_ids(c["tags"], "axis-aligned"):
        al, nan = c["alphas"][b], np.isnan(c["alphas"][b])
        no_hit = ~_hit(al).any(axis=1) & ~c["inside"][b]
        assert (no_hit & nan.any(axis=1)).any(), f"env {b}: no agent with zero hits and a NaN ray"
        # ... among its rays 0 .. k-1: the NaN, sorted behind the misses, changes which rays the top-k hands back
        assert (no_hit & nan[:, :c["ocfg"].top_k].any(axis=1)).any(), f"env {b}: the NaN ray does not change the top-k"
        assert c["inside"][b].any(), f"env {b}: no agent inside an obstacle"
        assert nan[c["inside"][b]].any(), "NaN * 0 stays NaN for the agent inside"


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_clipped_determinants_occur(cfg):
    c = _catalogue(*cfg)
    ids = sum((S.env_ids(c["tags"], t) for t in ("axis-aligned", "parallel-to-ray", "weak-threshold")), [])
    a = np.abs(c["det0"][ids])
    assert ((a > 0) & (a < f32(1e-7))).any()


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_weak_threshold_scene_has_obstacles_on_both_sides_of_the_robustness_test(cfg):
    c = _catalogue(*cfg)
    weak = [S.is_weak(c["obst"][b, o], *c["tab"]) for b in S.env_ids(c["tags"], "weak-threshold") for o in range(c["ocfg"].n_obs)]
    assert any(weak) and not all(weak)
    for b in S.env_ids(c["tags"], "weak-threshold"):
        assert _hit(c["alphas"][b]).any(), "somebody sees these obstacles"
    # the robust angle of the other scenes is robust, the axis-aligned ones are not
    assert not S.is_weak(c["obst"][S.env_ids(c["tags"], "cull-boundary")[0], 0], *c["tab"])
    assert S.is_weak(c["obst"][S.env_ids(c["tags"], "axis-aligned")[0], 0], *c["tab"])


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_on_vertex_agent_has_32_zero_alphas_outside_every_obstacle(cfg):
    c = _catalogue(*cfg)
    (b,) = S.env_ids(c["tags"], "on-vertex")
    assert not np.isnan(c["alphas"][b]).any()
    for i in (0, 1):
        assert (c["alphas"][b, i].view(np.uint32) == 0).all(), f"agent {i}: 32 alphas equal to +0"
        assert not c["inside"][b, i]
    assert (c["obst"][b, :, 4] == f32(S.ROBUST)).all(), "no axis-aligned obstacle in this env"


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_ties_beside_a_nan_agent(cfg):
    """agents 2 and 3 (one pair of the wave kernel) hold 32 tied +0 alphas and no NaN, agent 0 of the same env only NaN"""
    c = _catalogue(*cfg)
    (b,) = S.env_ids(c["tags"], "ties-beside-nan-agent")
    assert np.isnan(c["alphas"][b, 0]).all() and not np.isnan(c["alphas"][b, 1:]).any()
    assert (c["alphas"][b, 2:4].view(np.uint32) == 0).all() and not c["inside"][b].any()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_symmetric_ties_next_to_nan_rays(cfg):
    c = _catalogue(*cfg)
    (b,) = S.env_ids(c["tags"], "symmetric-ties")
    groups = 0
    for i in range(c["ocfg"].n_agents):
        al = c["alphas"][b, i]
        vals, counts = np.unique(al[_hit(al)].view(np.uint32), return_counts=True)
        if (counts >= 2).any() and np.isnan(al).any() and not c["inside"][b, i]:
            groups += 1
    assert groups >= 1, "no agent with bit-identical hit alphas and a NaN ray"


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_graze_alphas(cfg):
    c = _catalogue(*cfg)
    (b,) = S.env_ids(c["tags"], "graze")
    got = c["alphas"][b, :3, 16]
    want = np.array([np.nextafter(f32(1), f32(0)), f32(1.0), f32(1e6)], f32)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), got.tolist()
    assert want[0] == f32(0.99999994)


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_cull_boundary_agents_straddle_both_thresholds(cfg):
    c = _catalogue(*cfg)
    ocfg, ids = c["ocfg"], S.env_ids(c["tags"], "cull-boundary")
    n = ocfg.n_agents
    pos = np.concatenate([c["agent"][b, :n - 1, :2] for b in ids])[:10]
    rec = c["obst"][ids[0], 0]
    assert all((c["obst"][b, 0] == rec).all() for b in ids)
    cx, cy, hm = S.cull_circle(rec)
    thr = f32(f32(ocfg.comm_radius) + hm)
    # pair cull, as the kernel evaluates it: dx * dx + dy * dy > thr * thr
    dx, dy = (pos[:5, 0] - cx).astype(f32), (pos[:5, 1] - cy).astype(f32)
    d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
    dist = np.sqrt(d2.astype(np.float64))
    assert len(set(np.sqrt(d2).astype(f32).tolist())) == 5 and (np.diff(dist) > 0).all(), dist.tolist()
    far = d2 > f32(thr * thr)
    assert not far[0] and not far[1] and far[3] and far[4], far.tolist()
    # ray cull of ray 16 for the second set: |cr * pc.y - sn * pc.x| > h_o + 0.05, all five within reach
    rc, rs = c["tab"]
    px, py = (cx - pos[5:, 0]).astype(f32), (cy - pos[5:, 1]).astype(f32)
    cross = np.abs(((rc[16] * py).astype(f32) - (rs[16] * px).astype(f32)).astype(f32))
    assert len(set(cross.tolist())) == 5
    miss = cross > hm
    assert not miss[0] and not miss[1] and miss[3] and miss[4], cross.tolist()
    assert (((px * px).astype(f32) + (py * py).astype(f32)).astype(f32) < f32(thr * thr)).all()
    for b in ids:                                                    # the agent next to the obstacle really hits it
        al = c["alphas"][b, n - 1]
        assert _hit(al).any() and (al[_hit(al)] > 0).all() and not c["inside"][b, n - 1]


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_mask_radius_scenes_flip_the_oracles_masks(cfg):
    c = _catalogue(*cfg)
    ocfg, ids = c["ocfg"], S.env_ids(c["tags"], "mask-radius")
    assert len(ids) == 3
    n, pad = ocfg.n_agents, ocfg.num_nodes - 1
    hits, _ = E.lidar_sense(ocfg, c["agent"][ids][..., :2], c["obst"][ids], *c["tab"])
    g = E.get_graph(ocfg, c["agent"][ids], c["goal"][ids], c["obst"][ids], hits)
    aa = g["receivers"][:, 0 * n + 1] != pad                          # edge agent 0 <- agent 1
    assert aa.tolist() == [True, False, False], "d < comm_radius one ulp below it only"
    ob0 = n * n + ocfg.n_goal_edges + 2 * ocfg.top_k                  # agent 2's nearest hit
    ah = g["receivers"][:, ob0] != pad
    ld = E.norm2(c["agent"][ids, 2, 0] - hits[:, 2, 0, 0], c["agent"][ids, 2, 1] - hits[:, 2, 0, 1])
    assert ah[0] and not ah[2], (ah.tolist(), ld.tolist())
    assert len(set(ld.tolist())) == 3 and ld[0] < S.lidar_radius(ocfg) <= ld[2], ld.tolist()
    # agent 0 - goal 0 at the same three distances (the goal edge is always open; the distance enters the reward)
    dg = E.norm2(c["agent"][ids, 0, 0] - c["goal"][ids, 0, 0], c["agent"][ids, 0, 1] - c["goal"][ids, 0, 1])
    assert dg.tolist() == [float(x) for x in S.three(ocfg.comm_radius)]


@pytest.mark.parametrize("cfg", FULL, ids=IDS[:5])
def test_non_finite_scenes_put_nan_exactly_where_expected(cfg):
    c = _catalogue(*cfg)
    ocfg, a = c["ocfg"], S.NF_AGENT
    n, sd = ocfg.n_agents, ocfg.state_dim
    nxt = E.agent_step_euler(ocfg, c["agent"], E.clip_action(c["action"]))
    by = {t.split("/")[1]: b for b, t in enumerate(c["tags"]) if t.startswith("non-finite/")}
    assert tuple(by) == S.NON_FINITE
    bic = ocfg.is_bicycle
    want = {"action-nan": [2, 3] if bic else [2], "action-inf": [], "position-nan": [0],
            "velocity-nan": [0, 1, 2, 3, 4] if bic else [0, 2], "velocity-inf": [2, 3] if bic else []}
    for name, cols in want.items():
        exp = np.zeros((n, sd), bool)
        exp[a, cols] = True
        np.testing.assert_array_equal(np.isnan(nxt[by[name]]), exp, err_msg=name)
    assert np.isfinite(nxt[by["action-inf"]]).all()
    others = [b for b, t in enumerate(c["tags"]) if not t.startswith("non-finite") and t != "ties-beside-nan-agent"]
    assert np.isfinite(nxt[others]).all()
    # a NaN position: every alpha of that agent is NaN, and the stable sort hands back rays 0 .. k-1, all NaN
    b = by["position-nan"]
    hits, idx = E.lidar_sense(ocfg, c["agent"][b:b + 1, :, :2], c["obst"][b:b + 1], *c["tab"])
    assert idx[0, a].tolist() == list(range(ocfg.top_k)) and np.isnan(hits[0, a]).all()
    assert np.isfinite(hits[0, [i for i in range(n) if i != a]]).all()
