"""CBF action landscape, host side: action_admissibility on hand-made arrays, the renderer's inset on a short oracle episode,
the --action-landscape flag of test.py, and the C entry point's declaration, export and host-side refusals — CPU only."""
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from oracle import env_np as E
from dgppo_amd.env import plot as P
from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import ActionLandscape, CostLandscape, Landscape, Rollout
from dgppo_amd.utils.graph import GraphsTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FIELDS = ("us", "vs", "cbf", "Vh_next", "Vh", "actions", "agent", "frames", "alpha", "dt")


def _record(h, frames, Vh=None, agent=1, n=3, alpha=10.0, dt=0.03):
    """an ActionLandscape whose h() is `h` [F, nv, nu]: the swept agent's first cbf component carries it, the second and the
    other agents' entries are lower"""
    h = np.asarray(h, f32)
    F, nv, nu = h.shape
    cbf = np.full((F, nv, nu, n, 2), -9.0, f32)
    cbf[:, :, :, agent, 0] = h
    Vh = np.full((F, n, 2), -1.0, f32) if Vh is None else np.asarray(Vh, f32)
    return ActionLandscape(np.linspace(-1, 1, nu).astype(f32), np.linspace(-1, 1, nv).astype(f32), cbf, np.zeros_like(cbf), Vh,
                           np.zeros((F, 2), f32), agent, np.asarray(frames, np.int64), alpha, dt)


def test_action_landscape_record():
    assert ActionLandscape._fields == FIELDS
    A = _record(np.arange(12, dtype=f32).reshape(2, 2, 3) - 6.0, [3, 4])
    A.cbf[0, 0, 0, 1, 1] = 5.0                            # the largest component of the swept agent counts
    A.cbf[0, 0, 1, 0, :] = 7.0                            # another agent's values never show
    h = A.h()
    assert h.shape == (2, 2, 3) and h[0, 0, 0] == 5.0 and h[0, 0, 1] == -5.0
    np.testing.assert_array_equal(h <= 0.0, (A.cbf[:, :, :, 1] <= 0.0).all(-1))


def test_action_admissibility_counts():
    """4 frames of a 2 x 3 grid, every count known in advance: all admitted (an exact 0 is admitted), none, a sign change, a
    NaN slice"""
    nan = np.nan
    h = np.array([[[-1.0, -0.5, 0.0], [-2.0, -1.0, -3.0]],
                  [[0.5, 1.0, 2.0], [1e-6, 3.0, 0.25]],
                  [[-1.0, -0.5, 0.5], [-2.0, 1.0, 3.0]],
                  [[nan, nan, nan], [nan, -1.0, nan]]], f32)
    got = EV.action_admissibility(_record(h, [0, 2, 5, 7]))
    np.testing.assert_array_equal(got["points"], [6, 6, 6, 6])
    np.testing.assert_array_equal(got["admitted"], [6, 0, 3, 1])
    np.testing.assert_array_equal(got["empty_frames"], [2])
    assert got["admissible_frac"] == 10 / 24 and got["empty_frac"] == 1 / 4
    np.testing.assert_array_equal(got["taken"], [-1, -1, -1, -1])       # no frame's successor is held
    assert got["taken_admitted_frac"] == 0.0
    all_nan = EV.action_admissibility(_record(np.full((1, 2, 2), nan, f32), [0]))
    assert all_nan["admitted"].tolist() == [0] and all_nan["empty_frames"].tolist() == [0] and all_nan["admissible_frac"] == 0.0


def test_taken_action_is_judged_from_the_records_values():
    """frames 0, 1, 2, 4 with alpha = 10, dt = 0.5: cbf_deriv of the action taken is (Vh[t + 1] - Vh[t]) / dt + alpha * Vh[t] of
    the swept agent, whatever the grid says; frame 2 (3 is not held) and frame 4 (the last) are unknown"""
    n, agent = 3, 1
    Vh = np.full((4, n, 2), 50.0, f32)                    # the other agents never count
    # step 0 -> 1: (-1.5 + 1) / 0.5 - 10 = -11 and (-1 + 2) / 0.5 - 20 = -18: admitted
    # step 1 -> 2: (4 + 1.5) / 0.5 - 15 = -4 and (-1 + 1) / 0.5 - 10 = -10: admitted
    Vh[0, agent] = [-1.0, -2.0]
    Vh[1, agent] = [-1.5, -1.0]
    Vh[2, agent] = [4.0, -1.0]
    Vh[3, agent] = [-1.0, -1.0]
    h = np.full((4, 2, 2), 1.0, f32)                      # the grid admits nothing
    got = EV.action_admissibility(_record(h, [0, 1, 2, 4], Vh, agent=agent, alpha=10.0, dt=0.5))
    np.testing.assert_array_equal(got["taken"], [1, 1, -1, -1])
    assert got["taken_admitted_frac"] == 1.0 and got["admitted"].tolist() == [0, 0, 0, 0] and got["empty_frac"] == 1.0
    # alpha = 0: step 0 -> 1 rises by (-0.2 + 1) / 0.5 = 1.6 > 0, step 1 -> 2 by (-0.1 + 0.2) / 0.5 = 0.2 > 0: neither is admitted;
    # alpha = 10 adds -10 and -2: both are
    Vh[1, agent] = [-0.2, -1.0]
    Vh[2, agent] = [-0.1, -1.0]
    got = EV.action_admissibility(_record(h, [0, 1, 2, 4], Vh, agent=agent, alpha=0.0, dt=0.5))
    np.testing.assert_array_equal(got["taken"], [0, 0, -1, -1])
    assert got["taken_admitted_frac"] == 0.0
    got = EV.action_admissibility(_record(h, [0, 1, 2, 4], Vh, agent=agent, alpha=10.0, dt=0.5))
    np.testing.assert_array_equal(got["taken"], [1, 1, -1, -1])
    with pytest.raises(ValueError, match="frame"):
        EV.action_admissibility(_record(h, [0, 1, 2]))


# ---- renderer ------------------------------------------------------------------------------------------------------------------------
def _episode(n, n_obs, T, seed=3):
    """T oracle steps of one LidarSpread env as the Rollout the renderer reads"""
    cfg = E.EnvCfg(E.LIDAR_SPREAD, n_agents=n, n_obs=n_obs)
    agent, goal, obst = E.env_reset(cfg, np.array([seed], dtype=np.int64))
    tab = E.ray_table(32)
    hits = E.lidar_sense(cfg, agent[..., :2], obst, *tab)[0]
    rng = np.random.default_rng(seed)
    gs, rewards, costs = [], [], []
    for t in range(T):
        act = rng.uniform(-1, 1, size=(1, n, 2)).astype(f32)
        out = E.env_step(cfg, agent, goal, obst, hits, act, tab)
        gs.append(E.get_graph(cfg, agent, goal, obst, hits))
        rewards.append(out["reward"][0]); costs.append(out["cost"][0])
        agent, hits = out["next_agent"], out["next_hits"]
    stack = lambda k: np.stack([g[k][0] for g in gs])
    pts = obst[0, :, 8:16].reshape(n_obs, 4, 2)
    es = types.SimpleNamespace(obstacle=types.SimpleNamespace(points=np.broadcast_to(pts, (T,) + pts.shape)))
    g = GraphsTuple(stack("n_node"), stack("n_edge"), stack("nodes"), stack("edges"), stack("states"), stack("receivers"),
                    stack("senders"), stack("node_type"), es)
    return cfg, Rollout(g, None, None, np.array(rewards), np.stack(costs), None, None, None)


def _synthetic(frames, signs, agent=1, n=3):
    """per frame a plane over the 7 x 5 action grid changing sign at u = 0.25 (+1), an all-negative bowl (-1), an all-positive
    one (+2)"""
    us, vs = np.linspace(-1, 1, 7).astype(f32), np.linspace(-1, 1, 5).astype(f32)
    U, V = np.meshgrid(us, vs)
    h = np.stack([(U - 0.25) if s == 1 else ((-0.1 - U ** 2 - V ** 2) if s < 0 else (0.1 + U ** 2 + V ** 2)) for s in signs])
    A = _record(h, frames, agent=agent, n=n)
    taken = np.stack([[0.1 * k - 0.5, 0.5 - 0.2 * k] for k in range(len(frames))]).astype(f32)
    return A._replace(us=us, vs=vs, actions=taken)


def _scene(cfg, ro, **kw):
    return P._Scene(P.episode_from_rollout(ro), float(cfg.area_size), 3, 3, 0.05, 0.0, ("agent collisions", "obs collisions"),
                    None, 30, **kw)


def test_scene_action_inset_only_on_held_frames():
    T = 5
    cfg, ro = _episode(3, 2, T)
    A = _synthetic([0, 2, 4], [+1, -1, +2])
    scene = _scene(cfg, ro, action_landscape=A)
    try:
        assert scene.act_ax is not None and scene.act_ax in scene.ax.child_axes and scene.act_ax in scene.artists()
        assert scene.act_ax.get_xlim() == (-1.0, 1.0) and scene.act_ax.get_ylim() == (-1.0, 1.0)
        assert scene._act_norm.vcenter == 0.0 and len(scene._act_levels) == 15
        np.testing.assert_allclose(scene._act_norm.halfrange, np.abs(A.h()).max())
        assert scene.contours is None and not hasattr(scene, "cbf_text")          # no position landscape was asked for
        scene.draw(0)                                                    # sign change: filled contours, zero line, marker
        assert scene.act_ax.get_visible() and scene.act_contours is not None and scene.act_zero_line is not None
        assert list(scene.act_zero_line.levels) == [0.0]
        zero_u = np.concatenate([p.vertices for p in scene.act_zero_line.get_paths()])[:, 0]
        np.testing.assert_allclose(zero_u, 0.25, atol=1e-6)
        np.testing.assert_allclose(np.asarray(scene.act_marker.get_data()).reshape(-1), A.actions[0])
        scene.draw(1)                                                    # not held: nothing
        assert not scene.act_ax.get_visible() and scene.act_contours is None and scene.act_zero_line is None
        scene.draw(2)                                                    # everything admitted: no boundary
        assert scene.act_ax.get_visible() and scene.act_contours is not None and scene.act_zero_line is None
        np.testing.assert_allclose(np.asarray(scene.act_marker.get_data()).reshape(-1), A.actions[1])
        scene.draw(3)
        assert not scene.act_ax.get_visible()
        scene.draw(4)                                                    # nothing admitted: no boundary either
        assert scene.act_ax.get_visible() and scene.act_contours is not None and scene.act_zero_line is None
    finally:
        scene.close()


def test_scene_action_inset_combines_with_the_position_landscapes():
    T = 3
    cfg, ro = _episode(3, 2, T)
    area = cfg.area_size
    xs, ys = np.linspace(0, area, 6).astype(f32), np.linspace(0, area, 4).astype(f32)
    v = np.full((2, 4, 6, 3, 2), -9.0, f32)
    v[:, :, :, 1, 0] = np.meshgrid(xs, ys)[0] - 0.5 * area
    land = Landscape(xs, ys, v, 1, np.array([0, 1]))
    cost = CostLandscape(xs, ys, v.copy(), 1, np.array([0, 1]))
    A = _synthetic([1, 2], [+1, +1])
    scene = _scene(cfg, ro, landscape=land, cost_landscape=cost, action_landscape=A)
    try:
        scene.draw(0)
        assert scene.contours is not None and scene.cost_zero_line is not None and not scene.act_ax.get_visible()
        scene.draw(1)
        assert scene.contours is not None and scene.act_ax.get_visible() and scene.act_zero_line is not None
        scene.draw(2)
        assert scene.contours is None and scene.act_ax.get_visible()
    finally:
        scene.close()
    for kw in (dict(landscape=land), dict(cost_landscape=cost), dict(landscape=land, cost_landscape=cost)):
        with pytest.raises(ValueError, match="agent"):
            _scene(cfg, ro, action_landscape=_synthetic([0], [+1], agent=2), **kw)


def test_render_with_action_landscape_writes_every_frame(tmp_path):
    from PIL import Image, ImageSequence
    T = 4
    cfg, ro = _episode(3, 2, T)
    A = _synthetic([0, 2], [+1, -1])
    out = P.render_lidar(video_path=tmp_path / "action.mp4", rollout=ro, side_length=cfg.area_size, dim=2, n_agent=3, n_rays=8,
                         r=0.05, cost_components=("agent collisions", "obs collisions"), dpi=30, action_landscape=A)
    assert out.exists() and out.stat().st_size > 1000
    if out.suffix == ".gif":
        with Image.open(out) as im:
            assert sum(1 for _ in ImageSequence.Iterator(im)) == T


# ---- test.py ---------------------------------------------------------------------------------------------------------------------------
def test_cli_action_flag():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.ACTION_FLAGS == [(("--action-landscape",), "int", None)]
    assert mod.COST_FLAGS == [(("--cost-landscape",), "int", None)] and len(mod.FLAGS) == 18
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.action_landscape is None and args.cost_landscape is None and args.landscape is None and args.landscape_grid == 64
    args = ap.parse_args(["--path", "x", "--action-landscape", "2", "--landscape-grid", "8", "--no-video"])
    assert args.action_landscape == 2 and args.landscape_grid == 8 and args.no_video


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
NAME = "dgppo_graph_feats_action_sweep"


def _call(lib, cfg, agent_id=0, ptrs=1, efeat=None, Fp=8):
    """the entry point with every pointer operand non-NULL (never dereferenced on the host) unless `ptrs` says otherwise"""
    p = lambda name: None if name == ptrs else C.c_void_p(0x1000)
    return lib.dgppo_graph_feats_action_sweep(
        C.byref(cfg), p("agent"), C.c_int64(12), p("goal"), p("obst"), p("hits"), C.c_int64(48), None, C.c_int32(1),
        C.c_int32(agent_id), p("us"), C.c_int32(2), p("vs"), C.c_int32(2), p("Xa"), p("Xo"),
        C.c_void_p(0x1000 if efeat is None else efeat), p("emask"), C.c_int32(Fp), None)


def test_entry_point_is_declared_exported_and_refuses_on_the_host():
    from dgppo_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dgppo_hip.h")).read()
    assert re.search(r"\bint32_t\s+" + NAME + r"\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    lib = N.lib()
    assert hasattr(lib, NAME)
    err = lambda: lib.dgppo_last_error().decode()
    assert _call(lib, N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)) == -1
    assert NAME in err() and "VMASReverseTransport" in err()
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    for aid in (3, -1):
        assert _call(lib, cfg, agent_id=aid) == -1
        assert NAME in err() and "agent_id" in err() and "[0, 3)" in err()
    for name in ("agent", "goal", "us", "vs", "Xa", "emask"):
        assert _call(lib, cfg, ptrs=name) == -1
        assert NAME in err() and "NULL operand" in err(), name
    assert _call(lib, cfg, ptrs="Xo") == -1 and "Xo is NULL" in err()
    assert _call(lib, cfg, ptrs="hits") == -1 and "hits is NULL" in err()
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    assert _call(lib, mpe, ptrs="obst") == -1 and "obst is NULL" in err()
    assert _call(lib, cfg, efeat=0x1008) == -1
    assert NAME in err() and "16-byte aligned" in err()
    assert _call(lib, cfg, Fp=cfg.node_dim - 1) == -1 and "Fp" in err()
