"""Cost landscape, host side: the CostLandscape record, landscape_agreement, the renderer's overlays (the true cost alone and
its dashed zero line over the learned Vh) on a short oracle episode, and the --cost-landscape flag of test.py — CPU only."""
import importlib.util
import os
import types

import numpy as np
import pytest

from oracle import env_np as E
from dgppo_amd.env import plot as P
from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import CostLandscape, Landscape, Rollout
from dgppo_amd.utils.graph import GraphsTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


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


def _values(area, n, frames, signs, agent=1, shift=0.5):
    """[F, ny, nx, n, 2] on a 7 x 5 grid: per frame a plane changing sign at x = shift * area (+1), an all-negative bowl (-1)
    or a bowl whose maximum is exactly 0 (0) for `agent`; the other entries are lower"""
    xs = np.linspace(0.0, area, 7).astype(f32)
    ys = np.linspace(0.0, area, 5).astype(f32)
    X, Y = np.meshgrid(xs, ys)
    v = np.full((len(frames), len(ys), len(xs), n, 2), -9.0, f32)
    for k, s in enumerate(signs):
        v[k, :, :, agent, 0] = (X - shift * area) if s > 0 else ((-0.1 if s < 0 else 0.0) - (X - 0.5 * area) ** 2 - Y ** 2)
    return xs, ys, v


def _cost(area, n, frames, signs, agent=1, shift=0.5):
    xs, ys, v = _values(area, n, frames, signs, agent, shift)
    return CostLandscape(xs, ys, v, agent, np.asarray(frames, np.int64))


def _land(area, n, frames, signs, agent=1, shift=0.5):
    xs, ys, v = _values(area, n, frames, signs, agent, shift)
    return Landscape(xs, ys, v, agent, np.asarray(frames, np.int64))


def test_cost_landscape_h_is_the_swept_agents_worst_component():
    cost = np.zeros((2, 2, 3, 3, 2), f32)
    cost[..., 0, :] = 7.0                                 # another agent's values never show
    cost[0, :, :, 1] = [-1.0, -0.25]
    cost[1, :, :, 1] = [0.5, -2.0]
    cost[1, 1, 2, 1] = [-3.0, 0.0]                        # a component of exactly 0 is unsafe
    c = CostLandscape(np.arange(3, dtype=f32), np.arange(2, dtype=f32), cost, 1, np.array([4, 9]))
    assert c._fields == ("xs", "ys", "cost", "agent", "frames")
    assert Landscape._fields == ("xs", "ys", "Vh", "agent", "frames")
    h = c.h()
    assert h.shape == (2, 2, 3)
    assert (h[0] == -0.25).all() and h[1, 0, 0] == 0.5 and h[1, 1, 2] == 0.0
    np.testing.assert_array_equal(h >= 0.0, (cost[:, :, :, 1] >= 0.0).any(-1))


def test_landscape_agreement_counts():
    """3 frames of a 2 x 3 grid, every count known in advance"""
    xs, ys = np.arange(3, dtype=f32), np.arange(2, dtype=f32)

    def rec(cls, h0):
        v = np.full((3, 2, 3, 2, 2), -5.0, f32)
        v[:, :, :, 1, 0] = h0
        return cls(xs, ys, v, 1, np.array([0, 2, 5]))
    nan = np.nan
    # frame 0: true unsafe at 3 points, the net misses 2 of them and is conservative at 1 of the 3 safe ones
    # frame 1: no truly unsafe point; the net is conservative at 2 of 5 finite points, one point is NaN in the net
    # frame 2: a true NaN and a true exact 0 (unsafe) that the net catches with an exact 0
    hc = np.array([[[0.5, 0.0, 1.0], [-1.0, -1.0, -1.0]],
                   [[-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]],
                   [[nan, 0.0, -1.0], [-1.0, -1.0, -1.0]]], f32)
    hv = np.array([[[-0.5, -0.1, 2.0], [0.0, -1.0, -1.0]],
                   [[0.5, 0.5, -1.0], [nan, -1.0, -1.0]],
                   [[1.0, 0.0, -1.0], [-1.0, -1.0, -1.0]]], f32)
    land, cost = rec(Landscape, hv), rec(CostLandscape, hc)
    np.testing.assert_array_equal(land.h(), hv)
    np.testing.assert_array_equal(cost.h(), hc)
    got = EV.landscape_agreement(land, cost)
    np.testing.assert_array_equal(got["points"], [6, 5, 5])
    np.testing.assert_array_equal(got["nan"], [0, 1, 1])
    np.testing.assert_array_equal(got["unsafe"], [3, 0, 1])
    np.testing.assert_array_equal(got["missed"], [2, 0, 0])
    np.testing.assert_array_equal(got["conservative"], [1, 2, 0])
    assert got["missed_frac"] == 2 / 4 and got["conservative_frac"] == 3 / 12
    # a frame with no unsafe point on its own: the denominators clamp to 1
    one = lambda r, arr: type(r)(r.xs, r.ys, arr[1:2], 1, np.array([2]))
    got = EV.landscape_agreement(one(land, land.Vh), one(cost, cost.cost))
    assert got["missed_frac"] == 0.0 and got["unsafe"].tolist() == [0] and got["conservative_frac"] == 2 / 5
    all_unsafe = CostLandscape(xs, ys, np.ones((1, 2, 3, 2, 2), f32), 1, np.array([2]))
    got = EV.landscape_agreement(one(land, land.Vh), all_unsafe)
    assert got["conservative_frac"] == 0.0 and got["conservative"].tolist() == [0] and got["missed_frac"] == 3 / 5
    # mismatches
    with pytest.raises(ValueError, match="differ"):
        EV.landscape_agreement(land, CostLandscape(xs + 1, ys, cost.cost, 1, cost.frames))
    with pytest.raises(ValueError, match="differ"):
        EV.landscape_agreement(land, CostLandscape(xs[:2], ys, cost.cost[:, :, :2], 1, cost.frames))
    with pytest.raises(ValueError, match="differ"):
        EV.landscape_agreement(land, CostLandscape(xs, ys, cost.cost, 0, cost.frames))
    with pytest.raises(ValueError, match="differ"):
        EV.landscape_agreement(land, CostLandscape(xs, ys, cost.cost, 1, np.array([0, 2, 4])))


def _scene(cfg, ro, **kw):
    return P._Scene(P.episode_from_rollout(ro), float(cfg.area_size), 3, 3, 0.05, 0.0, ("agent collisions", "obs collisions"),
                    None, 30, **kw)


def test_scene_cost_only():
    T = 5
    cfg, ro = _episode(3, 2, T)
    cost = _cost(cfg.area_size, 3, frames=[0, 2, 4], signs=[+1, -1, 0])
    scene = _scene(cfg, ro, cost_landscape=cost)
    try:
        assert scene.cbf_text.get_text() == "Cost for 1"
        assert len(scene.fig.axes) == 2                                   # the colour bar
        assert scene._norm.vcenter == 0.0 and len(scene._levels) == 15
        np.testing.assert_allclose(scene._norm.halfrange, np.abs(cost.h()).max())
        scene.draw(0)                                                     # values change sign: filled contours and the zero line
        assert scene.contours is not None and scene.zero_line is not None and scene.cost_zero_line is None
        assert list(scene.zero_line.levels) == [0.0]
        assert scene.contours in scene.artists() and scene.zero_line in scene.artists()
        scene.draw(1)                                                     # not covered
        assert scene.contours is None and scene.zero_line is None
        scene.draw(2)                                                     # all negative: no zero line
        assert scene.contours is not None and scene.zero_line is None
        scene.draw(3)
        assert scene.contours is None and scene.zero_line is None
        scene.draw(4)                                                     # a maximum of exactly 0 is unsafe: zero line
        assert scene.contours is not None and scene.zero_line is not None
    finally:
        scene.close()


def test_scene_both():
    T = 4
    cfg, ro = _episode(3, 2, T)
    A = cfg.area_size
    land = _land(A, 3, frames=[0, 1, 2, 3], signs=[+1, +1, -1, +1])
    cost = _cost(A, 3, frames=[0, 1, 3], signs=[+1, -1, +1], shift=0.25)
    cost.cost[2, 0, 0, 1, 0] = np.nan                                    # frame 3: a NaN in the cost slice
    scene = _scene(cfg, ro, landscape=land, cost_landscape=cost)
    try:
        assert scene.cbf_text.get_text() == "CBF for 1"
        np.testing.assert_allclose(scene._norm.halfrange, np.abs(land.h()).max())     # the colour scale is Vh's
        scene.draw(0)                                                     # both change sign
        n0 = len(scene.artists())
        assert scene.contours is not None and scene.zero_line is not None and scene.cost_zero_line is not None
        assert list(scene.cost_zero_line.levels) == [0.0] and scene.cost_zero_line in scene.artists()
        assert scene.cost_zero_line is not scene.zero_line
        zero_x = lambda cs: np.concatenate([p.vertices for p in cs.get_paths()])[:, 0]
        np.testing.assert_allclose(zero_x(scene.zero_line), 0.5 * A, atol=1e-6)        # the filled contours are Vh's
        np.testing.assert_allclose(zero_x(scene.cost_zero_line), 0.25 * A, atol=1e-6)
        scene.draw(1)                                                     # the cost is negative everywhere
        assert scene.contours is not None and scene.zero_line is not None and scene.cost_zero_line is None
        assert len(scene.artists()) == n0 - 1                             # the cost adds exactly one artist
        scene.draw(2)                                                     # the cost does not cover the frame
        assert scene.contours is not None and scene.zero_line is None and scene.cost_zero_line is None
        scene.draw(3)                                                     # a NaN in the cost slice: no cost contour
        assert scene.contours is not None and scene.zero_line is not None and scene.cost_zero_line is None
    finally:
        scene.close()
    only = _scene(cfg, ro, landscape=land)
    try:
        only.draw(0)
        assert only.cbf_text.get_text() == "CBF for 1" and len(only.artists()) == n0 - 1
    finally:
        only.close()
    with pytest.raises(ValueError, match="agent"):
        _scene(cfg, ro, landscape=land, cost_landscape=_cost(A, 3, frames=[0], signs=[+1], agent=2))
    other = _cost(A, 3, frames=[0], signs=[+1])
    with pytest.raises(ValueError, match="grid"):
        _scene(cfg, ro, landscape=land, cost_landscape=other._replace(xs=other.xs + f32(0.5)))


def test_render_with_cost_landscape_writes_every_frame(tmp_path):
    from PIL import Image, ImageSequence
    T = 4
    cfg, ro = _episode(3, 2, T)
    cost = _cost(cfg.area_size, 3, frames=[0, 2], signs=[+1, -1])
    land = _land(cfg.area_size, 3, frames=[0, 1], signs=[+1, -1], shift=0.75)
    common = dict(rollout=ro, side_length=cfg.area_size, dim=2, n_agent=3, n_rays=8, r=0.05,
                  cost_components=("agent collisions", "obs collisions"), dpi=30)
    for name, kw in (("cost", dict(cost_landscape=cost)), ("both", dict(landscape=land, cost_landscape=cost))):
        out = P.render_lidar(video_path=tmp_path / f"{name}.mp4", **common, **kw)
        assert out.exists() and out.stat().st_size > 1000
        if out.suffix == ".gif":
            with Image.open(out) as im:
                assert sum(1 for _ in ImageSequence.Iterator(im)) == T
    with pytest.raises(NotImplementedError):
        P.render_lidar(video_path=tmp_path / "no.mp4", viz_opts={"cbf": 1}, cost_landscape=cost, **common)


def test_cli_cost_flag():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert [f[0] for f in mod.FLAGS] == [
        ("--path",), ("--no-video",), ("--epi",), ("--step",), ("--obs",), ("--stochastic",), ("--full-observation",), ("--debug",),
        ("--cpu",), ("--max-step",), ("--log",), ("-n", "--num-agents"), ("--seed",), ("--env",), ("--offset",), ("--dpi",),
        ("--landscape",), ("--landscape-grid",)]
    assert mod.COST_FLAGS == [(("--cost-landscape",), "int", None)]
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.cost_landscape is None and args.landscape is None and args.landscape_grid == 64
    assert (args.epi, args.seed, args.dpi, args.no_video, args.offset) == (5, 1234, 100, False, 0)
    args = ap.parse_args(["--path", "x", "--cost-landscape", "2", "--landscape", "1", "--landscape-grid", "16", "--no-video",
                          "--epi", "3", "--step", "4", "--obs", "1", "--stochastic", "--full-observation", "--debug", "--cpu",
                          "--max-step", "9", "--log", "-n", "5", "--seed", "7", "--env", "LidarSpread", "--offset", "1", "--dpi", "50"])
    assert args.cost_landscape == 2 and args.landscape == 1 and args.landscape_grid == 16 and args.no_video
    assert (args.epi, args.step, args.obs, args.max_step, args.num_agents, args.seed, args.env, args.offset, args.dpi) == \
        (3, 4, 1, 9, 5, 7, "LidarSpread", 1, 50)
    assert args.stochastic and args.full_observation and args.debug and args.cpu and args.log
