"""Rollout landscape, host side: the two C entry points' declaration, export and host-side refusals, the NumPy restatement of
the constraint-return fold (pinned by known answers; tests/test_rollout_landscape_gpu.py holds the kernel to it), the
RolloutLandscape record, rollout_agreement on hand-made arrays, the renderer's dotted overlay and the --rollout-landscape flags
of test.py — CPU only."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from dgppo_amd.env import plot as P
from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import CostLandscape, Landscape, RolloutLandscape

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_cost_landscape_cpu import _episode  # noqa: E402

ROOT = os.path.dirname(HERE)
f32 = np.float32


# ---- the fold, restated ----------------------------------------------------------------------------------------------------------
def fold_np(cost, gamma):
    """cost [K, ..., nh] fp32, time-major -> (value, worst) [..., nh]: compute_dec_ocp_gae's Vhs_row recursion at
    gae_lambda = 1 started from the last cost (V = h[K-1]; V[c] = max(h[k][c], (1 - gamma) * max_c h[k] + gamma * V[c]), one
    multiply, one multiply and one add, every operation rounded to fp32) and the running maximum.  np.maximum / np.max
    propagate NaN as jnp.maximum / jnp.max do.  gamma and 1 - gamma are Python doubles rounded to fp32, as the binding hands
    them to the kernel."""
    h = np.asarray(cost, dtype=f32)
    g, omg = f32(gamma), f32(1 - gamma)
    V, W = h[-1].copy(), h[-1].copy()
    with np.errstate(all="ignore"):
        for k in range(h.shape[0] - 2, -1, -1):
            m = h[k].max(axis=-1, keepdims=True)
            a = (omg * m).astype(f32)
            b = (g * V).astype(f32)
            V = np.maximum(h[k], (a + b).astype(f32))
            W = np.maximum(W, h[k])
    return V, W


def test_fold_known_answers():
    v, w = fold_np(np.array([-1.0, 0.5, -1.0], f32).reshape(3, 1, 1, 1), 0.5)
    assert v.shape == w.shape == (1, 1, 1) and v.dtype == w.dtype == f32
    assert v[0, 0, 0] == f32(-0.25) and w[0, 0, 0] == f32(0.5)
    h = np.array([[0.25, -3.0, np.inf]], f32).reshape(1, 1, 1, 3)            # K = 1: nothing is folded
    v, w = fold_np(h, 0.99)
    np.testing.assert_array_equal(v, h[0])
    np.testing.assert_array_equal(w, h[0])
    # two components: alone, component 0 would stay at max(-0.8, 0.5 * -0.8 + 0.5 * -1) = -0.8; the step's largest component
    # (0.4) lifts it to 0.5 * 0.4 + 0.5 * -1 = -0.3
    h = np.array([[-0.8, 0.4], [-1.0, -1.0]], f32).reshape(2, 1, 1, 2)
    v, w = fold_np(h, 0.5)
    assert v[0, 0, 0] == f32(f32(0.5) * f32(0.4)) + f32(-0.5) and abs(float(v[0, 0, 0]) + 0.3) < 1e-7
    assert v[0, 0, 1] == f32(0.4)
    np.testing.assert_array_equal(w[0, 0], [f32(-0.8), f32(0.4)])
    alone, _ = fold_np(h[..., :1], 0.5)
    assert alone[0, 0, 0] == f32(-0.8)


def test_fold_nan_stays_with_its_agent():
    rng = np.random.default_rng(0)
    h = rng.uniform(-1, 1, size=(4, 2, 3, 2)).astype(f32)
    ref_v, ref_w = fold_np(h, 0.9)
    bad = h.copy()
    bad[1, 0, 2, 1] = np.nan                                  # step 1, env 0, agent 2, component 1
    v, w = fold_np(bad, 0.9)
    assert np.isnan(v[0, 2]).all()                            # max_c carries it into every component of that agent's value
    assert np.isnan(w[0, 2, 1]) and w[0, 2, 0] == ref_w[0, 2, 0]
    keep = np.ones((2, 3), bool)
    keep[0, 2] = False
    np.testing.assert_array_equal(v[keep], ref_v[keep])
    np.testing.assert_array_equal(w[keep], ref_w[keep])
    last = h.copy()
    last[3, 1, 0, 0] = np.nan                                 # in the last step: only that component starts from a NaN
    v, w = fold_np(last, 0.9)
    assert np.isnan(v[1, 0, 0]) and np.isnan(w[1, 0, 0]) and v[1, 0, 1] == ref_v[1, 0, 1]


# ---- the record and its statistics -----------------------------------------------------------------------------------------------
FIELDS = ("xs", "ys", "value", "worst", "agent", "frames", "horizon", "gamma")
XS, YS = np.arange(3, dtype=f32), np.arange(2, dtype=f32)


def _rl(h, frames, v=None, agent=1, n=2):
    """a RolloutLandscape whose h() is `h` and whose v() is `v` [F, 2, 3]: component 0 of the swept agent carries them"""
    h = np.asarray(h, f32)
    worst = np.full(h.shape + (n, 2), -5.0, f32)
    worst[..., agent, 0] = h
    value = np.full(h.shape + (n, 2), -5.0, f32)
    value[..., agent, 0] = h if v is None else np.asarray(v, f32)
    return RolloutLandscape(XS, YS, value, worst, agent, np.asarray(frames), 4, 0.99)


def _of(cls, h, frames, agent=1, n=2):
    v = np.full(np.shape(h) + (n, 2), -5.0, f32)
    v[..., agent, 0] = h
    return cls(XS, YS, v, agent, np.asarray(frames))


def test_rollout_landscape_record():
    assert RolloutLandscape._fields == FIELDS
    worst = np.zeros((2, 2, 3, 3, 2), f32)
    value = np.zeros((2, 2, 3, 3, 2), f32)
    worst[..., 0, :] = 7.0                                    # another agent's values never show
    value[..., 2, :] = 9.0
    worst[0, :, :, 1] = [-1.0, -0.25]
    worst[1, :, :, 1] = [0.5, -2.0]
    worst[1, 1, 2, 1] = [-3.0, 0.0]                           # a component of exactly 0 is unsafe
    value[:, :, :, 1] = [-0.75, -0.5]
    value[0, 0, 1, 1] = [0.125, -4.0]
    r = RolloutLandscape(XS, YS, value, worst, 1, np.array([4, 9]), 32, 0.99)
    h, v = r.h(), r.v()
    assert h.shape == v.shape == (2, 2, 3)
    assert (h[0] == -0.25).all() and h[1, 0, 0] == 0.5 and h[1, 1, 2] == 0.0
    np.testing.assert_array_equal(h >= 0.0, (worst[:, :, :, 1] >= 0.0).any(-1))
    assert v[0, 0, 1] == 0.125 and v[1, 1, 1] == -0.5 and (np.delete(v.reshape(-1), 1) == -0.5).all()


def test_rollout_agreement_counts():
    """3 frames of a 2 x 3 grid, every count known in advance"""
    nan = np.nan
    frames = [0, 2, 5]
    # frame 0: doomed at 3 points; the net misses 2 of them and is conservative at 1 of the 3 others; 1 doomed point is safe now
    # frame 1: nothing doomed; the net is conservative at 2 of its 5 finite points; the cost holds a NaN elsewhere
    # frame 2: a NaN in the rollout, an exact 0 (doomed) that the net meets with an exact 0 and the cost calls safe
    hr = np.array([[[0.5, 0.0, 1.0], [-1.0, -1.0, -1.0]],
                   [[-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]],
                   [[nan, 0.0, -1.0], [-1.0, -1.0, -1.0]]], f32)
    hv = np.array([[[-0.5, -0.1, 2.0], [0.0, -1.0, -1.0]],
                   [[0.5, 0.5, -1.0], [nan, -1.0, -1.0]],
                   [[1.0, 0.0, -1.0], [-1.0, -1.0, -1.0]]], f32)
    hc = np.array([[[0.5, 0.25, -0.5], [-1.0, -1.0, -1.0]],
                   [[-1.0, -1.0, nan], [-1.0, -1.0, -1.0]],
                   [[-1.0, -0.5, -1.0], [-1.0, -1.0, -1.0]]], f32)
    rl = _rl(hr, frames, v=hv + f32(0.25))
    got = EV.rollout_agreement(rl)
    assert sorted(got) == ["doomed", "doomed_frac", "points"]
    np.testing.assert_array_equal(got["points"], [6, 6, 5])
    np.testing.assert_array_equal(got["doomed"], [3, 0, 1])
    assert got["doomed_frac"] == 4 / 17
    land, cost = _of(Landscape, hv, frames), _of(CostLandscape, hc, frames)
    got = EV.rollout_agreement(rl, land=land)
    np.testing.assert_array_equal(got["points"], [6, 6, 5])
    np.testing.assert_array_equal(got["missed"], [2, 0, 0])
    np.testing.assert_array_equal(got["conservative"], [1, 2, 0])
    assert got["missed_frac"] == 2 / 4 and got["conservative_frac"] == 3 / (3 + 5 + 4)
    assert "latent" not in got
    # |Vh - value| on the swept agent's row: component 0 differs by 0.25 at its 17 finite points, component 1 (-5 in both) by 0
    # at all 18
    assert int(np.isfinite(hv).sum()) == 17
    np.testing.assert_allclose(got["value_error"], 0.25 * 17 / (17 + 18), rtol=1e-6)
    got = EV.rollout_agreement(rl, cost=cost)
    np.testing.assert_array_equal(got["latent"], [1, 0, 1])
    assert got["latent_frac"] == 2 / (4 + 5 + 5) and "missed" not in got
    both = EV.rollout_agreement(rl, land=land, cost=cost)
    assert both["missed_frac"] == 0.5 and both["latent"].tolist() == [1, 0, 1] and both["doomed"].tolist() == [3, 0, 1]
    # nothing doomed, nothing safe: the denominators clamp to 1
    none = EV.rollout_agreement(_rl(np.full((1, 2, 3), -1.0), [2]), land=_of(Landscape, np.full((1, 2, 3), -1.0), [2]),
                                cost=_of(CostLandscape, np.full((1, 2, 3), 1.0), [2]))
    assert none["missed_frac"] == 0.0 and none["doomed_frac"] == 0.0 and none["latent_frac"] == 0.0
    # mismatches
    for kw in (dict(land=Landscape(XS + 1, YS, land.Vh, 1, land.frames)), dict(land=Landscape(XS, YS, land.Vh, 0, land.frames)),
               dict(land=Landscape(XS, YS, land.Vh, 1, np.array([0, 2, 4]))),
               dict(cost=CostLandscape(XS[:2], YS, cost.cost[:, :, :2], 1, cost.frames)),
               dict(cost=CostLandscape(XS, YS + 1, cost.cost, 1, cost.frames)), dict(land=land, cost=_of(CostLandscape, hc, frames, 0))):
        with pytest.raises(ValueError, match="differ"):
            EV.rollout_agreement(rl, **kw)


# ---- renderer --------------------------------------------------------------------------------------------------------------------
def _values(area, n, frames, signs, agent=1, shift=0.5):
    """[F, ny, nx, n, 2] on a 7 x 5 grid: per frame a plane changing sign at x = shift * area (+1) or an all-negative bowl (-1)
    for `agent`; the other entries are lower"""
    xs, ys = np.linspace(0.0, area, 7).astype(f32), np.linspace(0.0, area, 5).astype(f32)
    X, Y = np.meshgrid(xs, ys)
    v = np.full((len(frames), len(ys), len(xs), n, 2), -9.0, f32)
    for k, s in enumerate(signs):
        v[k, :, :, agent, 0] = (X - shift * area) if s > 0 else (-0.1 - (X - 0.5 * area) ** 2 - Y ** 2)
    return xs, ys, v


def _synthetic(area, n, frames, signs, agent=1, shift=0.5):
    xs, ys, v = _values(area, n, frames, signs, agent, shift)
    return RolloutLandscape(xs, ys, v - f32(0.5), v, agent, np.asarray(frames, np.int64), 8, 0.99)


def _scene(cfg, ro, **kw):
    return P._Scene(P.episode_from_rollout(ro), float(cfg.area_size), 3, 3, 0.05, 0.0, ("agent collisions", "obs collisions"),
                    None, 30, **kw)


def test_scene_rollout_overlay():
    T = 4
    cfg, ro = _episode(3, 2, T)
    A = cfg.area_size
    rl = _synthetic(A, 3, frames=[0, 1, 3], signs=[+1, -1, +1], shift=0.25)
    rl.worst[2, 0, 0, 1, 0] = np.nan                                     # frame 3: a NaN in the slice
    scene = _scene(cfg, ro, rollout_landscape=rl)
    try:
        assert scene.contours is None and not hasattr(scene, "cbf_text") and len(scene.fig.axes) == 1    # no fill, no colour bar
        scene.draw(0)
        n0 = len(scene.artists())
        assert scene.rollout_zero_line is not None and scene.rollout_zero_line in scene.artists()
        assert list(scene.rollout_zero_line.levels) == [0.0]
        zero_x = np.concatenate([p.vertices for p in scene.rollout_zero_line.get_paths()])[:, 0]
        np.testing.assert_allclose(zero_x, 0.25 * A, atol=1e-6)
        scene.draw(1)                                                    # nothing doomed in the frame
        assert scene.rollout_zero_line is None and len(scene.artists()) == n0 - 1
        scene.draw(2)                                                    # not held
        assert scene.rollout_zero_line is None
        scene.draw(3)                                                    # a NaN: no contour
        assert scene.rollout_zero_line is None
    finally:
        scene.close()
    # over the learned contours and the true cost's dashed line
    xs, ys, v = _values(A, 3, [0, 1], [+1, +1])
    land, cost = Landscape(xs, ys, v, 1, np.array([0, 1])), CostLandscape(xs, ys, v.copy(), 1, np.array([0, 1]))
    scene = _scene(cfg, ro, landscape=land, cost_landscape=cost, rollout_landscape=rl)
    try:
        scene.draw(0)
        lines = (scene.zero_line, scene.cost_zero_line, scene.rollout_zero_line)
        assert scene.contours is not None and all(a is not None for a in lines) and len({id(a) for a in lines}) == 3
        scene.draw(1)
        assert scene.zero_line is not None and scene.rollout_zero_line is None
    finally:
        scene.close()


def test_scene_rollout_overlay_mismatches():
    cfg, ro = _episode(3, 2, 3)
    A = cfg.area_size
    rl = _synthetic(A, 3, frames=[0], signs=[+1])
    xs, ys, v = _values(A, 3, [0], [+1], agent=2)
    for kw in (dict(landscape=Landscape(xs, ys, v, 2, np.array([0]))), dict(cost_landscape=CostLandscape(xs, ys, v, 2, np.array([0])))):
        with pytest.raises(ValueError, match="agent"):
            _scene(cfg, ro, rollout_landscape=rl, **kw)
    from test_action_landscape_cpu import _synthetic as _action
    with pytest.raises(ValueError, match="agent"):
        _scene(cfg, ro, rollout_landscape=rl, action_landscape=_action([0], [+1], agent=2))
    xs, ys, v = _values(A, 3, [0], [+1])
    with pytest.raises(ValueError, match="grid"):
        _scene(cfg, ro, rollout_landscape=rl, landscape=Landscape(xs + f32(0.5), ys, v, 1, np.array([0])))
    with pytest.raises(ValueError, match="grid"):
        _scene(cfg, ro, rollout_landscape=rl, cost_landscape=CostLandscape(xs, ys[:3], v[:, :3], 1, np.array([0])))


def test_render_with_rollout_landscape_writes_every_frame(tmp_path):
    from PIL import Image, ImageSequence
    T = 4
    cfg, ro = _episode(3, 2, T)
    rl = _synthetic(cfg.area_size, 3, frames=[0, 2], signs=[+1, -1])
    xs, ys, v = _values(cfg.area_size, 3, [0, 1], [+1, -1], shift=0.75)
    land = Landscape(xs, ys, v, 1, np.array([0, 1]))
    common = dict(rollout=ro, side_length=cfg.area_size, dim=2, n_agent=3, n_rays=8, r=0.05,
                  cost_components=("agent collisions", "obs collisions"), dpi=30)
    for name, kw in (("rollout", {}), ("both", dict(landscape=land))):
        out = P.render_lidar(video_path=tmp_path / f"{name}.mp4", rollout_landscape=rl, **common, **kw)
        assert out.exists() and out.stat().st_size > 1000
        if out.suffix == ".gif":
            with Image.open(out) as im:
                assert sum(1 for _ in ImageSequence.Iterator(im)) == T
    with pytest.raises(ValueError, match="agent"):
        P.render_lidar(video_path=tmp_path / "no.mp4", rollout_landscape=rl._replace(agent=2), landscape=land, **common)


# ---- test.py ---------------------------------------------------------------------------------------------------------------------
def test_cli_rollout_flags():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.ROLLOUT_FLAGS == [(("--rollout-landscape",), "int", None), (("--rollout-horizon",), "int", 32)]
    # the four lists that were there stay what they are
    assert mod.FLAGS == [
        (("--path",), "req:str", None), (("--no-video",), "flag", False), (("--epi",), "int", 5), (("--step",), "int", None),
        (("--obs",), "int", None), (("--stochastic",), "flag", False), (("--full-observation",), "flag", False),
        (("--debug",), "flag", False), (("--cpu",), "flag", False), (("--max-step",), "int", None), (("--log",), "flag", False),
        (("-n", "--num-agents"), "int", None), (("--seed",), "int", 1234), (("--env",), "str", None), (("--offset",), "int", 0),
        (("--dpi",), "int", 100), (("--landscape",), "int", None), (("--landscape-grid",), "int", 64)]
    assert mod.COST_FLAGS == [(("--cost-landscape",), "int", None)]
    assert mod.ACTION_FLAGS == [(("--action-landscape",), "int", None)]
    assert mod.SHIELD_FLAGS == [(("--shield",), "flag", False), (("--shield-grid",), "int", 8), (("--shield-margin",), "float", 0.0)]
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.rollout_landscape is None and args.rollout_horizon == 32 and args.landscape_grid == 64
    assert args.landscape is None and args.cost_landscape is None and args.action_landscape is None and not args.shield
    args = ap.parse_args(["--path", "x", "--rollout-landscape", "2", "--rollout-horizon", "5", "--landscape-grid", "8", "--no-video",
                          "--shield", "--landscape", "2", "--cost-landscape", "2"])
    assert args.rollout_landscape == 2 and args.rollout_horizon == 5 and args.landscape_grid == 8 and args.no_video
    assert args.shield and args.landscape == 2 and args.cost_landscape == 2
    assert "UNSHIELDED" in mod.__doc__ and "--rollout-horizon" in mod.__doc__


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
FORK, FOLD = "dgppo_env_sweep_fork", "dgppo_constraint_return"
_P = 0x1000                      # a pointer that is never dereferenced on the host


def _fork(lib, cfg, agent_id=0, null=(), n_frames=1, nx=2, ny=2, carry=True, HC=64):
    """the entry point with every pointer operand non-NULL unless named in `null`"""
    p = lambda name: None if name in null else C.c_void_p(_P)
    return lib.dgppo_env_sweep_fork(
        C.byref(cfg), p("agent"), 12, p("goal"), p("obst"), p("hits"), 48, p("ray_cos"), p("ray_sin"), None, n_frames, agent_id,
        p("xs"), nx, p("ys"), ny, p("carry") if carry else None, 192, HC, p("agent_out"), p("goal_out"), p("obst_out"),
        p("hits_out"), p("carry_out"), None)


def _fold(lib, K=2, G=3, n=2, nh=2, null=()):
    p = lambda name: None if name in null else C.c_void_p(_P)
    return lib.dgppo_constraint_return(p("cost"), G * n * nh, K, G, n, nh, 0.99, 0.01, p("value"), p("worst"), None)


def test_entry_points_are_declared_and_exported():
    from dgppo_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgppo_hip.h")).read(), flags=re.S)
    lib = N.lib()
    for name in (FORK, FOLD):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int32
    # the header cites the reference lines, as every entry point does
    full = open(os.path.join(ROOT, "include", "dgppo_hip.h")).read()
    for name in (FORK, FOLD):
        comment = full[:full.index("int32_t " + name)].rsplit("/*", 1)[1]
        assert "dgppo/algo/utils.py:38-45" in comment, name


def test_fork_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    bad = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    bad.kind = 17
    assert _fork(lib, bad) == -1 and FORK in err() and "unknown env kind" in err()   # dgppo_validate_cfg, under this name
    assert _fork(lib, N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)) == -1
    assert FORK in err() and "VMASReverseTransport" in err()
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    for aid in (3, -1):
        assert _fork(lib, cfg, agent_id=aid) == -1
        assert FORK in err() and "agent_id" in err() and "[0, 3)" in err()
    for kw in (dict(nx=-1), dict(ny=-2), dict(n_frames=-1)):
        assert _fork(lib, cfg, **kw) == -1
        assert FORK in err() and "negative counts" in err(), kw
    everything = ("agent", "goal", "obst", "hits", "ray_cos", "ray_sin", "xs", "ys", "carry", "agent_out", "goal_out", "obst_out",
                  "hits_out", "carry_out")
    for kw in (dict(nx=0), dict(ny=0), dict(n_frames=0)):                        # zero counts: nothing to do, nothing is read
        assert _fork(lib, cfg, null=everything, **kw) == 0, kw
    for name in ("agent", "goal", "xs", "ys", "agent_out", "goal_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and "NULL operand" in err(), name
    for name, text in (("obst", "obst is NULL"), ("obst_out", "obst_out is NULL"), ("hits", "hits / ray_cos / ray_sin is NULL"),
                       ("ray_cos", "hits / ray_cos / ray_sin is NULL"), ("ray_sin", "hits / ray_cos / ray_sin is NULL"),
                       ("hits_out", "hits_out is NULL"), ("carry_out", "carry_out is NULL")):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and text in err(), name
    assert _fork(lib, cfg, HC=0) == -1 and FORK in err() and "HC" in err()
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    assert _fork(lib, mpe, null=("obst",)) == -1 and FORK in err() and "obst is NULL" in err()
    assert _fork(lib, mpe, null=("obst_out",)) == -1 and "obst_out is NULL" in err()
    # the frame has to fit the LDS: 64 agents x 256 hit points alone are 128 KB
    big = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 64, 64, n_rays=256, top_k=256)
    assert _fork(lib, big) == -1
    assert FORK in err() and "does not fit the LDS" in err()
    assert _fork(lib, cfg, nx=4097, ny=4096) == -1
    assert FORK in err() and "grid too large" in err() and "2^24" in err()


def test_fold_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    for K in (0, -3):
        assert _fold(lib, K=K) == -1
        assert FOLD in err() and "K must be >= 1" in err()
    for nh in (0, 4, -1):
        assert _fold(lib, nh=nh) == -1
        assert FOLD in err() and "outside [1, 3]" in err()
    for kw in (dict(G=-1), dict(n=-1)):
        assert _fold(lib, **kw) == -1
        assert FOLD in err() and "negative counts" in err()
    for kw in (dict(G=0), dict(n=0)):
        assert _fold(lib, null=("cost", "value", "worst"), **kw) == 0
    for name in ("cost", "value", "worst"):
        assert _fold(lib, null=(name,)) == -1
        assert FOLD in err() and "NULL operand" in err(), name
