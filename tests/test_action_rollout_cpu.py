"""Action rollout landscape, host side: the fork's layout restated in NumPy on a hand-written example, the ActionRolloutLandscape
record and action_rollout_agreement on hand-made arrays, the C entry point's declaration, export and host-side refusals, the
binding's refusals, the --action-rollout-landscape flag of test.py and the renderer's inset — CPU only."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from dgppo_amd.env import plot as P
from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import ActionRolloutLandscape

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import action_rollout_np as AR  # noqa: E402
from test_action_landscape_cpu import _episode, _scene, _synthetic  # noqa: E402

ROOT = os.path.dirname(HERE)
f32 = np.float32
nan = np.nan
FIELDS = ("us", "vs", "value", "worst", "actions", "agent", "frames", "horizon", "gamma")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_fork_layout():
    """2 frames of a 3-frame record, n = 2, a 2 x 3 grid (nu = 2, nv = 3): env (f * nv + iv) * nu + iu copies frame frame_ids[f],
    and only row agent_id of its action is the grid action (us[iu], vs[iv])"""
    n, T = 2, 3
    us, vs = np.array([0.25, 5.0], f32), np.array([-1.0, nan, 0.5], f32)      # copied as words: nothing is clipped, a NaN stays
    agent = np.arange((T + 1) * n * 4, dtype=f32).reshape(T + 1, n, 4)
    goal = -np.arange(n * 4, dtype=f32).reshape(n, 4)
    actions = np.array([[[1.0, 2.0], [3.0, 4.0]], [[-7.0, nan], [0.5, 0.5]], [[9.0, 9.5], [8.0, 8.5]]], f32)
    carry = np.arange((T + 1) * n * 3, dtype=f32).reshape(T + 1, n, 3) + 100
    out, act, c = AR.fork_np(dict(agent=agent), dict(goal=goal), actions, [2, 0], 2, 1, us, vs, carry)
    G = 2 * 3 * 2
    assert out["agent"].shape == (G, n, 4) and out["goal"].shape == (G, n, 4) and act.shape == (G, n, 2) and c.shape == (G * n, 3)
    assert all(a.dtype == np.uint32 for a in (out["agent"], out["goal"], act, c))
    for f, t in enumerate([2, 0]):
        for iv in range(3):
            for iu in range(2):
                g = (f * 3 + iv) * 2 + iu
                np.testing.assert_array_equal(out["agent"][g].view(f32), agent[t])
                np.testing.assert_array_equal(out["goal"][g].view(f32), goal)
                np.testing.assert_array_equal(c.reshape(G, n, 3)[g].view(f32), carry[t])
                np.testing.assert_array_equal(act[g, 0], actions[t, 0].view(np.uint32))         # the other agent: as recorded
                np.testing.assert_array_equal(act[g, 1], np.array([us[iu], vs[iv]], f32).view(np.uint32))
    # frame_ids None: frames 0 .. n_frames - 1; no carry
    out, act, c = AR.fork_np(dict(agent=agent), dict(goal=goal), actions, None, 2, 0, us, vs[:1])
    assert c is None and act.shape == (4, n, 2)
    np.testing.assert_array_equal(out["agent"].view(f32), agent[[0, 0, 1, 1]])
    np.testing.assert_array_equal(act[:, 0].view(f32), [[0.25, -1.0], [5.0, -1.0]] * 2)
    np.testing.assert_array_equal(act[:, 1].view(f32), actions[[0, 0, 1, 1], 1])


def test_fold_restatement_known_answers():
    v, w = AR.fold_np(np.array([-1.0, 0.5, -1.0], f32).reshape(3, 1, 1, 1), 0.5)
    assert v[0, 0, 0] == f32(-0.25) and w[0, 0, 0] == f32(0.5)
    v, w = AR.fold_np(np.array([[-1.0, nan], [-0.5, -1.0]], f32).reshape(2, 1, 1, 2), 0.99)
    assert np.isnan(v).all() and np.isnan(w[0, 0, 1]) and w[0, 0, 0] == f32(-0.5)      # the row maximum carries the NaN over


# ---- the record and its statistics ---------------------------------------------------------------------------------------------------
def _record(h, frames, others=None, agent=1, n=3):
    """an ActionRolloutLandscape whose h() is `h` [F, nv, nu] — component 1 of the swept agent's row of `worst` carries it, the
    other is lower — and whose h_others() is `others` (default -0.75), carried by the last other agent's component 0"""
    h = np.asarray(h, f32)
    F, nv, nu = h.shape
    worst = np.full((F, nv, nu, n, 2), -9.0, f32)
    worst[:, :, :, agent, 1] = h
    if n > 1:
        worst[:, :, :, [i for i in range(n) if i != agent][-1], 0] = -0.75 if others is None else np.asarray(others, f32)
    return ActionRolloutLandscape(np.linspace(-1, 1, nu).astype(f32), np.linspace(-1, 1, nv).astype(f32), worst - f32(0.5), worst,
                                  np.zeros((F, 2), f32), agent, np.asarray(frames, np.int64), 4, 0.99)


def test_record():
    assert ActionRolloutLandscape._fields == FIELDS
    R = _record(np.arange(12, dtype=f32).reshape(2, 2, 3) - 6.0, [3, 4])
    R.worst[0, 0, 0, 1, 0] = 5.0                          # the largest component of the swept agent counts
    R.worst[0, 0, 1, 0, :] = 7.0                          # another agent's values never show in h(), and do in h_others()
    R.worst[1, 1, 2, 2, 1] = nan
    h, ho = R.h(), R.h_others()
    assert h.shape == ho.shape == (2, 2, 3) and h[0, 0, 0] == 5.0 and h[0, 0, 1] == -5.0
    assert ho[0, 0, 1] == 7.0 and ho[0, 0, 0] == f32(-0.75) and np.isnan(ho[1, 1, 2]) and np.isfinite(h).all()
    R.worst[1, 0, 0, 1, 0] = nan
    assert np.isnan(R.h()[1, 0, 0])                       # a NaN component propagates
    one = _record(np.zeros((1, 2, 2), f32), [0], agent=0, n=1)
    assert one.h_others().shape == (1, 2, 2) and np.isnan(one.h_others()).all()


H4 = np.array([[[-1.0, -0.5, 0.0], [-2.0, 0.5, 1.0]],           # decisive: 3 of 6 doomed (an exact 0 is doomed)
               [[0.5, 1.0, 2.0], [1e-6, 3.0, nan]],            # everything finite is doomed: 5 of 5
               [[-1.0, -0.5, -0.5], [-2.0, -1.0, -3.0]],       # nothing doomed
               [[nan, nan, nan], [nan, nan, nan]]], f32)        # nothing finite: neither empty nor decisive


def test_agreement_counts():
    got = EV.action_rollout_agreement(_record(H4, [0, 2, 5, 7]))
    np.testing.assert_array_equal(got["points"], [6, 5, 6, 0])
    np.testing.assert_array_equal(got["doomed"], [3, 5, 0, 0])
    np.testing.assert_array_equal(got["empty_frames"], [2])
    assert got["doomed_frac"] == 8 / 17 and got["empty_frac"] == 1 / 4 and got["decisive_frac"] == 1 / 4
    assert got["others_doomed_frac"] == 0.0 and got["others_decisive_frac"] == 0.0
    assert sorted(got) == sorted(["points", "doomed", "doomed_frac", "empty_frames", "empty_frac", "decisive_frac",
                                  "others_doomed_frac", "others_decisive_frac"])
    others = np.full(H4.shape, -0.75, f32)
    others[0, 0, :2] = 0.5                                 # decisive for the neighbours in frame 0 only
    others[3] = 0.5                                        # all doomed where the own row holds nothing finite
    others[2, 1, 1] = nan
    got = EV.action_rollout_agreement(_record(H4, [0, 2, 5, 7], others))
    assert got["others_doomed_frac"] == 8 / 23 and got["others_decisive_frac"] == 1 / 4
    with pytest.raises(ValueError, match="frame"):
        EV.action_rollout_agreement(_record(H4, [0, 2, 5]))


def test_agreement_of_a_single_agent_has_no_others():
    got = EV.action_rollout_agreement(_record(H4, [0, 1, 2, 3], agent=0, n=1))
    assert "others_doomed_frac" not in got and "others_decisive_frac" not in got
    np.testing.assert_array_equal(got["doomed"], [3, 5, 0, 0])


def test_agreement_with_the_learned_barrier():
    """the barrier's h over the same 4 x (2 x 3) points: missed = admitted (<= 0, an exact 0 is admitted) and doomed,
    conservative = rejected and not doomed, both only where both are finite"""
    from test_action_landscape_cpu import _record as barrier
    a = np.array([[[-1.0, 1.0, 0.0], [1.0, -1.0, nan]],        # doomed (0,2) admitted -> missed; (0,1), (1,0) rejected, free -> 2
                  [[-1.0, 1.0, 1.0], [1.0, 1.0, -1.0]],        # (0,0) missed; (1,2) is a NaN in R
                  [[1.0, 1.0, -1.0], [-1.0, -1.0, -1.0]],      # 2 conservative
                  [[-1.0] * 3, [1.0] * 3]], f32)               # R holds nothing finite here
    R = _record(H4, [0, 2, 5, 7])
    A = barrier(a, [0, 2, 5, 7])
    got = EV.action_rollout_agreement(R, A)
    np.testing.assert_array_equal(got["missed"], [2, 1, 0, 0])          # frame 0: (0, 2) and (1, 1)
    np.testing.assert_array_equal(got["conservative"], [2, 0, 2, 0])
    # counted where both are finite: doomed 2 (frame 0; (1, 2) has no barrier value) + 5, free 3 + 6
    assert got["missed_frac"] == 3 / 7 and got["conservative_frac"] == 4 / 9
    np.testing.assert_array_equal(got["doomed"], [3, 5, 0, 0])          # the unconditional counts stay
    for other in (barrier(a, [0, 2, 5, 8]), barrier(a, [0, 2, 5, 7], agent=2),
                  barrier(a, [0, 2, 5, 7])._replace(us=np.array([-1.0, 0.0, 0.5], f32)),
                  barrier(a, [0, 2, 5, 7])._replace(vs=np.array([-1.0, 0.5], f32))):
        with pytest.raises(ValueError, match="differ"):
            EV.action_rollout_agreement(R, other)


# ---- test.py ---------------------------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag():
    mod = _load_test_py()
    assert mod.ACTION_ROLLOUT_FLAGS == [(("--action-rollout-landscape",), "int", None)]
    # every older list is unchanged
    assert mod.COST_FLAGS == [(("--cost-landscape",), "int", None)] and len(mod.FLAGS) == 18
    assert mod.FLAGS[-2:] == [(("--landscape",), "int", None), (("--landscape-grid",), "int", 64)]
    assert mod.ACTION_FLAGS == [(("--action-landscape",), "int", None)]
    assert mod.SHIELD_FLAGS == [(("--shield",), "flag", False), (("--shield-grid",), "int", 8), (("--shield-margin",), "float", 0.0)]
    assert mod.ROLLOUT_FLAGS == [(("--rollout-landscape",), "int", None), (("--rollout-horizon",), "int", 32)]
    assert mod.LOOKAHEAD_FLAGS == [(("--shield-horizon",), "int", 0)]
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.action_rollout_landscape is None and args.action_landscape is None and args.rollout_landscape is None
    assert args.landscape_grid == 64 and args.rollout_horizon == 32 and args.shield_horizon == 0 and not args.shield
    args = ap.parse_args(["--path", "x", "--action-rollout-landscape", "1", "--landscape-grid", "3", "--rollout-horizon", "2",
                          "--no-video", "--stochastic"])
    assert args.action_rollout_landscape == 1 and args.landscape_grid == 3 and args.rollout_horizon == 2 and args.stochastic
    assert "--action-rollout-landscape" in mod.__doc__ and "_action_rollout.npz" in mod.__doc__


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
NAME = "dgppo_env_action_sweep_fork"
FAKE = 0x1000                                               # a non-NULL pointer: never dereferenced on the host


def _fork(lib, cfg, null=(), nu=2, nv=3, n_frames=2, agent_id=0, HC=64, carry=True, strides=None):
    p = lambda name: None if name in null else C.c_void_p(FAKE)
    n = cfg.n_agents
    st = dict(agent=n * cfg.state_dim, hits=n * cfg.top_k * 2, action=n * 2, carry=n * HC)
    st.update(strides or {})
    return lib.dgppo_env_action_sweep_fork(
        C.byref(cfg), p("agent"), st["agent"], p("goal"), p("obst"), p("hits"), st["hits"], p("action"), st["action"],
        p("carry") if carry else None, st["carry"], HC, p("frame_ids"), n_frames, agent_id, p("us"), nu, p("vs"), nv,
        p("agent_out"), p("goal_out"), p("obst_out"), p("hits_out"), p("action_out"), p("carry_out"), None)


def test_entry_point_is_declared_and_exported():
    from dgppo_amd import _native as N
    full = open(os.path.join(ROOT, "include", "dgppo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    lib = N.lib()
    assert re.search(r"\bint32_t\s+" + NAME + r"\s*\(", src)
    assert hasattr(lib, NAME) and getattr(lib, NAME).restype is C.c_int32
    assert len(getattr(lib, NAME).argtypes) == 26
    decl = src[src.index("int32_t " + NAME):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 25                            # header and binding agree on the number of operands
    comment = full[:full.index("int32_t " + NAME)].rsplit("/*", 1)[1]
    assert "AFTER each frame's policy forward" in comment and "env/base.py" in comment and "NOT clipped" in comment
    assert N.ABI_VERSION == 3 and lib.dgppo_abi_version() == 3          # the ABI is additive


def test_fork_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    bad = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    bad.kind = 17
    assert _fork(lib, bad) == -1 and NAME in err() and "unknown env kind" in err()   # dgppo_validate_cfg, under this name
    assert _fork(lib, N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)) == -1
    assert NAME in err() and "VMASReverseTransport" in err()
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    for kw in (dict(nu=0), dict(nv=0), dict(nu=-1)):
        assert _fork(lib, cfg, **kw) == -1 and NAME in err() and "nu and nv" in err(), kw
    assert _fork(lib, cfg, nu=4096, nv=4096) == -1 and NAME in err() and "grid too large" in err()
    for kw in (dict(agent_id=3), dict(agent_id=-1)):
        assert _fork(lib, cfg, **kw) == -1 and NAME in err() and "agent_id" in err(), kw
    for kw in (dict(n_frames=0), dict(n_frames=-2)):
        assert _fork(lib, cfg, **kw) == -1 and NAME in err() and "n_frames" in err(), kw
    # G * n = n_frames * nv * nu * n: 2^20 frames of 1023 actions and 3 agents
    assert _fork(lib, cfg, n_frames=1 << 20, nu=1023, nv=1) == -1 and NAME in err() and "G * n < 2^31" in err()
    assert _fork(lib, cfg, HC=0) == -1 and NAME in err() and "HC" in err()
    for field, block in (("agent", 12), ("hits", 3 * cfg.top_k * 2), ("action", 6), ("carry", 3 * 64)):
        assert _fork(lib, cfg, strides={field: block - 1}) == -1
        assert NAME in err() and "frame stride" in err() and field in err(), field
    assert _fork(lib, cfg, strides=dict(agent=13, hits=1000, action=7, carry=3 * 64 + 5), null=("agent",)) == -1
    assert "NULL operand" in err()                                                  # longer strides are fine
    for name in ("agent", "goal", "action", "us", "vs", "agent_out", "goal_out", "action_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert NAME in err() and "NULL operand" in err(), name
    for name in ("obst", "obst_out", "hits", "hits_out", "carry_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert NAME in err() and f"{name} is NULL" in err(), name
    # hits / hits_out exactly where the kind casts rays: a LiDAR kind without obstacles and an MPE kind take none
    for other in (N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 0), N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)):
        assert _fork(lib, other) == -1 and NAME in err() and "cast rays" in err()
        assert _fork(lib, other, null=("hits",)) == -1 and "cast rays" in err()
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    assert _fork(lib, mpe, null=("hits", "hits_out", "obst")) == -1 and NAME in err() and "obst is NULL" in err()


def test_binding_refuses_before_anything_is_launched():
    """host tensors: the logical refusals come first; with everything else right the operands are refused for not being on
    the device — either way nothing reaches the library"""
    import torch
    from dgppo_amd import _native as N, ops_env as OE
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    n, nu, nv, HC, T, F = 3, 2, 3, 64, 4, 2
    G = F * nv * nu
    z = torch.zeros
    step = dict(agent=z(T + 1, n, 4), hits=z(T + 1, n, cfg.top_k, 2))
    env = dict(goal=z(n, 4), obst=z(2, cfg.obst_stride))
    ok = dict(step=step, env=env, actions=z(T, n, 2), frame_ids=None, n_frames=F, agent_id=1, us=z(nu), vs=z(nv),
              out=OE.State.empty(cfg, G, "cpu"), action_out=z(G, n, 2), carry=z(T + 1, n, HC), carry_st=n * HC,
              carry_out=z(G * n, HC))

    def fork(cfg=cfg, **kw):
        OE.action_sweep_fork(cfg, **{**ok, **kw})
    for kw, match in ((dict(agent_id=n), "agent_id"), (dict(agent_id=-1), "agent_id"), (dict(n_frames=0), "n_frames"),
                      (dict(us=z(0)), "us"), (dict(vs=z(2, 2)), "vs"), (dict(carry_out=None), "carry_out"),
                      (dict(carry_out=z(G * n + 1, HC)), "carry_out"), (dict(step=dict(agent=step["agent"])), "hits"),
                      (dict(env=dict(goal=env["goal"])), "obst"), (dict(carry_st=n * HC - 1), "frame stride of carry"),
                      (dict(actions=z(T, n, 4)[:, :, :2].transpose(0, 1)), "frame stride of actions"),
                      (dict(action_out=z(G, n + 1, 2)), "action_out"),
                      (dict(out=OE.State({"agent": ok["out"].agent}, ok["out"].env)), "out has no hits")):
        with pytest.raises(ValueError, match=match):
            fork(**kw)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        fork(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0))
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    with pytest.raises(ValueError, match="cast rays"):                    # hits given for an MPE kind
        fork(cfg=mpe, env=dict(goal=env["goal"], obst=z(3, mpe.obst_stride)))
    with pytest.raises(ValueError, match="CUDA"):
        fork()


# ---- renderer ------------------------------------------------------------------------------------------------------------------------
def _synthetic_R(frames, signs, agent=1, n=3):
    """the synthetic action landscape's planes (test_action_landscape_cpu._synthetic: a sign change at u = 0.25, an all-negative
    bowl, an all-positive one) as the h() of an ActionRolloutLandscape over the same 7 x 5 grid"""
    A = _synthetic(frames, signs, agent=agent, n=n)
    R = _record(A.h(), frames, agent=agent, n=n)
    return R._replace(us=A.us, vs=A.vs, actions=A.actions)


def test_scene_alone_gets_its_own_inset():
    T = 4
    cfg, ro = _episode(3, 2, T)
    R = _synthetic_R([0, 2, 3], [+1, -1, +2])
    scene = _scene(cfg, ro, action_rollout_landscape=R)
    try:
        assert scene.action_landscape is None and scene.act_ax is not None and scene.act_ax in scene.artists()
        assert "worst cost of 1 within 4 steps" in scene.act_ax.get_title()
        scene.draw(0)                                                    # sign change: filled contours, solid zero line, marker
        assert scene.act_ax.get_visible() and scene.act_contours is not None and scene.act_ro_zero_line is not None
        zero_u = np.concatenate([p.vertices for p in scene.act_ro_zero_line.get_paths()])[:, 0]
        np.testing.assert_allclose(zero_u, 0.25, atol=1e-6)
        np.testing.assert_allclose(np.asarray(scene.act_marker.get_data()).reshape(-1), R.actions[0])
        scene.draw(1)                                                    # not held: nothing
        assert not scene.act_ax.get_visible() and scene.act_contours is None and scene.act_ro_zero_line is None
        scene.draw(2)                                                    # nothing doomed: no boundary
        assert scene.act_ax.get_visible() and scene.act_contours is not None and scene.act_ro_zero_line is None
        scene.draw(3)                                                    # everything doomed: no boundary either
        assert scene.act_contours is not None and scene.act_ro_zero_line is None
    finally:
        scene.close()


def _artist_counts(scene):
    return (len(scene.ax.get_children()), len(scene.act_ax.get_children()), len(scene.act_ax.collections))


def test_scene_dashes_the_doomed_boundary_inside_the_action_inset():
    T = 3
    cfg, ro = _episode(3, 2, T)
    A = _synthetic([0, 1, 2], [+1, +1, -1])
    R = _synthetic_R([0, 2], [+1, -1])
    plain = _scene(cfg, ro, action_landscape=A)
    both = _scene(cfg, ro, action_landscape=A, action_rollout_landscape=R)
    try:
        assert "cbf_deriv of 1" in both.act_ax.get_title() and len(both.fig.axes) == len(plain.fig.axes)
        for t, dashed in ((0, True), (1, False), (2, False)):
            plain.draw(t)
            both.draw(t)
            assert (both.act_ro_zero_line is not None) == dashed, t
            # the keyword adds the dashed contour and nothing else; without it not one artist changes
            a, b = _artist_counts(plain), _artist_counts(both)
            assert b[0] == a[0] and b[1] == a[1] + int(dashed) and b[2] == a[2] + int(dashed), t
            np.testing.assert_array_equal(np.asarray(both.act_marker.get_data()), np.asarray(plain.act_marker.get_data()))
            assert (both.act_zero_line is None) == (plain.act_zero_line is None)
        both.draw(0)
        assert both.act_ro_zero_line.get_linestyle()[0][1] is not None                 # a dash pattern, not a solid line
        assert plain.action_rollout_landscape is None and plain.act_ro_zero_line is None
    finally:
        plain.close()
        both.close()
    with pytest.raises(ValueError, match="agent"):
        _scene(cfg, ro, action_landscape=A, action_rollout_landscape=_synthetic_R([0], [+1], agent=2))
    with pytest.raises(ValueError, match="different grids"):
        _scene(cfg, ro, action_landscape=A, action_rollout_landscape=R._replace(us=R.us * f32(0.5)))


def test_render_writes_every_frame(tmp_path):
    from PIL import Image, ImageSequence
    T = 3
    cfg, ro = _episode(3, 2, T)
    common = dict(rollout=ro, side_length=cfg.area_size, dim=2, n_agent=3, n_rays=8, r=0.05,
                  cost_components=("agent collisions", "obs collisions"), dpi=30)
    for name, kw in (("alone", dict(action_rollout_landscape=_synthetic_R([0, 2], [+1, -1]))),
                     ("both", dict(action_landscape=_synthetic([0, 1], [+1, -1]),
                                   action_rollout_landscape=_synthetic_R([0, 1], [+1, +1])))):
        out = P.render_lidar(video_path=tmp_path / f"{name}.mp4", **common, **kw)
        assert out.exists() and out.stat().st_size > 1000
        if out.suffix == ".gif":
            with Image.open(out) as im:
                assert sum(1 for _ in ImageSequence.Iterator(im)) == T
