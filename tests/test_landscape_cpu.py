"""Vh landscape, host side: the Landscape record, the renderer's contour overlay on a short oracle episode and the two flags
of test.py — CPU only."""
import importlib.util
import os
import types

import numpy as np

from oracle import env_np as E
from dgppo_amd.env import plot as P
from dgppo_amd.trainer.data import Landscape, Rollout
from dgppo_amd.utils.graph import GraphsTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _episode(n, n_obs, T, seed=3):
    """T oracle steps of one LidarSpread env as the Rollout the renderer reads"""
    cfg = E.EnvCfg(E.LIDAR_SPREAD, n_agents=n, n_obs=n_obs)
    agent, goal, obst = E.env_reset(cfg, np.array([seed], dtype=np.int64))
    tab = E.ray_table(32)
    hits = E.lidar_sense(cfg, agent[..., :2], obst, *tab)[0]
    rng = np.random.default_rng(seed)
    gs, rewards, costs = [], [], []
    for t in range(T):
        act = rng.uniform(-1, 1, size=(1, n, 2)).astype(np.float32)
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


def _landscape(area, n, frames, signs):
    """h(x, y) = sign-changing plane (+1), all-negative bowl (-1) or a bowl whose maximum is exactly 0 (0) per frame, for
    agent 1; the other entries are lower"""
    xs = np.linspace(0.0, area, 7).astype(np.float32)
    ys = np.linspace(0.0, area, 5).astype(np.float32)
    X, Y = np.meshgrid(xs, ys)
    Vh = np.full((len(frames), len(ys), len(xs), n, 2), -9.0, np.float32)
    for k, s in enumerate(signs):
        Vh[k, :, :, 1, 0] = (X - 0.5 * area) if s > 0 else ((-0.1 if s < 0 else 0.0) - (X - 0.5 * area) ** 2 - Y ** 2)
    return Landscape(xs, ys, Vh, 1, np.asarray(frames, np.int64))


def test_landscape_h_is_the_swept_agents_worst_component():
    Vh = np.zeros((2, 2, 3, 3, 2), np.float32)
    Vh[..., 0, :] = 7.0                                   # another agent's values never show
    Vh[0, :, :, 1] = [-1.0, -0.25]
    Vh[1, :, :, 1] = [0.5, -2.0]
    Vh[1, 1, 2, 1] = [-3.0, 0.0]
    land = Landscape(np.arange(3, dtype=np.float32), np.arange(2, dtype=np.float32), Vh, 1, np.array([4, 9]))
    h = land.h()
    assert h.shape == (2, 2, 3)
    assert (h[0] == -0.25).all() and h[1, 0, 0] == 0.5 and h[1, 1, 2] == 0.0
    # >= 0 exactly where any component is: test.py's unsafe rule
    np.testing.assert_array_equal(h >= 0.0, (Vh[:, :, :, 1] >= 0.0).any(-1))


def test_scene_draws_contours_only_on_covered_frames():
    T = 4
    cfg, ro = _episode(3, 2, T)
    land = _landscape(cfg.area_size, 3, frames=[0, 2], signs=[+1, -1])
    ep = P.episode_from_rollout(ro)
    scene = P._Scene(ep, float(cfg.area_size), 3, 3, 0.05, 0.0, ("agent collisions", "obs collisions"), None, 30, land)
    try:
        assert scene.cbf_text.get_text() == "CBF for 1"
        assert len(scene.fig.axes) == 2                                   # the colour bar
        assert scene._norm.vcenter == 0.0 and len(scene._levels) == 15
        np.testing.assert_allclose(scene._norm.halfrange, np.abs(land.h()).max())
        scene.draw(0)                                                     # values change sign: filled contours and the zero line
        assert scene.contours is not None and scene.zero_line is not None
        assert list(scene.zero_line.levels) == [0.0]
        assert scene.contours in scene.artists() and scene.zero_line in scene.artists()
        first = scene.contours
        scene.draw(1)                                                     # not covered
        assert scene.contours is None and scene.zero_line is None
        scene.draw(2)                                                     # all negative: no zero line
        assert scene.contours is not None and scene.contours is not first and scene.zero_line is None
        scene.draw(3)
        assert scene.contours is None and scene.zero_line is None
    finally:
        scene.close()


def test_render_with_landscape_writes_every_frame(tmp_path):
    from PIL import Image, ImageSequence
    T = 4
    cfg, ro = _episode(3, 2, T)
    land = _landscape(cfg.area_size, 3, frames=[0, 2], signs=[+1, -1])
    out = P.render_lidar(rollout=ro, video_path=tmp_path / "epi.mp4", side_length=cfg.area_size, dim=2, n_agent=3, n_rays=8,
                         r=0.05, cost_components=("agent collisions", "obs collisions"), dpi=30, landscape=land)
    assert out.exists() and out.stat().st_size > 1000
    if out.suffix == ".gif":
        with Image.open(out) as im:
            assert sum(1 for _ in ImageSequence.Iterator(im)) == T


def test_cli_flags():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    earlier = [
        (("--path",), "req:str", None), (("--no-video",), "flag", False), (("--epi",), "int", 5), (("--step",), "int", None),
        (("--obs",), "int", None), (("--stochastic",), "flag", False), (("--full-observation",), "flag", False),
        (("--debug",), "flag", False), (("--cpu",), "flag", False), (("--max-step",), "int", None), (("--log",), "flag", False),
        (("-n", "--num-agents"), "int", None), (("--seed",), "int", 1234), (("--env",), "str", None), (("--offset",), "int", 0),
        (("--dpi",), "int", 100)]
    assert mod.FLAGS[:len(earlier)] == earlier
    assert mod.FLAGS[len(earlier):] == [(("--landscape",), "int", None), (("--landscape-grid",), "int", 64)]
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.landscape is None and args.landscape_grid == 64
    assert (args.epi, args.seed, args.dpi, args.no_video, args.offset) == (5, 1234, 100, False, 0)
    args = ap.parse_args(["--path", "x", "--landscape", "2", "--landscape-grid", "16", "--no-video"])
    assert args.landscape == 2 and args.landscape_grid == 16 and args.no_video


def test_zero_line_when_the_maximum_is_exactly_zero():
    """h >= 0 is unsafe, so a frame that only touches 0 from below still gets its zero contour"""
    cfg, ro = _episode(3, 2, 2)
    land = _landscape(cfg.area_size, 3, frames=[1], signs=[0])
    assert land.h().max() == 0.0 and land.h().min() < 0.0
    scene = P._Scene(P.episode_from_rollout(ro), float(cfg.area_size), 3, 3, 0.05, 0.0, ("a", "b"), None, 30, land)
    try:
        scene.draw(1)
        assert scene.contours is not None and scene.zero_line is not None
    finally:
        scene.close()
