"""Start scenes without a GPU: the NumPy restatement of dgppo_env_scene_load (tests/scenes_np.py) on known answers, the jitter's
draw table and retry rule, the host refusals of the entry point and of its bindings, the Scenes file format, test.py's flags and the
committed fixtures."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lookahead_np as L  # noqa: E402
import lookahead_rounds_np as R  # noqa: E402
import scenes_np as SN  # noqa: E402
from oracle import env_np as EN  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "scenes")
f32 = np.float32


def _cfg(kind_name, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind_name], n, n_obs)


def _lidar_scene():
    """LidarSpread n = 2, one 0.2 x 0.4 rectangle at (1.0, 0.5) turned by 0.3: a valid scene"""
    agent = np.array([[[0.3, 0.3, 0.1, 0.0], [0.6, 1.2, 0.0, -0.1]]], f32)
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[1.2, 1.2], [0.2, 0.9]]
    rect = np.array([[[1.0, 0.5, 0.2, 0.4, 0.3]]], f32)
    return agent, goal, rect


def _flags(cfg, agent, goal, obst):
    out = SN.scene_load_np(cfg, agent, goal, obst, None, None, 0.0, agent.shape[0])
    assert out["n_failed"] == 0 and (out["attempt"] == -1).all(), "no jitter: nothing is drawn or counted"
    return out["flags"].tolist()


# ---- validity bits ------------------------------------------------------------------------------------------------------------------
def test_each_validity_bit_alone():
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    assert _flags(cfg, agent, goal, rect) == [0]
    # 1: a non-finite word anywhere in the template rows — a goal, an agent's velocity, an obstacle's height
    for which, idx, val in (("goal", (0, 1, 3), np.nan), ("agent", (0, 0, 2), np.inf), ("rect", (0, 0, 3), -np.inf)):
        rows = dict(agent=agent.copy(), goal=goal.copy(), rect=rect.copy())
        rows[which][idx] = val
        assert _flags(cfg, rows["agent"], rows["goal"], rows["rect"]) == [SN.NONFINITE], which
    # 2: outside [0, area] in x or y, on either side; the border itself is inside
    for col, val, want in ((0, 1.6, SN.OUT_OF_AREA), (0, -0.01, SN.OUT_OF_AREA), (1, 1.51, SN.OUT_OF_AREA), (1, -1e-6, SN.OUT_OF_AREA),
                           (0, 1.5, 0), (1, 0.0, 0)):
        a = agent.copy()
        a[0, 1, col] = val
        assert _flags(cfg, a, goal, rect) == [want], (col, val)
    # 4: closer than 2 car_radius = 0.1
    a = agent.copy()
    a[0, 1, :2] = [0.3 + 0.06, 0.3 + 0.07]                  # 0.0922 apart
    assert _flags(cfg, a, goal, rect) == [SN.AGENTS_OVERLAP]
    a[0, 1, :2] = [0.3 + 0.08, 0.3 + 0.07]                  # 0.1063 apart
    assert _flags(cfg, a, goal, rect) == [0]
    # 8: the centre of the rectangle; 0.03 off its long side (inside the car_radius margin); 0.08 off it (outside)
    c, s = np.cos(0.3), np.sin(0.3)
    for off, want in ((0.0, SN.AGENT_IN_OBSTACLE), (0.1 + 0.03, SN.AGENT_IN_OBSTACLE), (0.1 + 0.08, 0)):
        a = agent.copy()
        a[0, 0, :2] = [1.0 + off * c, 0.5 + off * s]       # along the rectangle's own x axis (its width 0.2: half 0.1)
        assert _flags(cfg, a, goal, rect) == [want], off
    # goals are checked for finiteness only: one in the middle of the rectangle, one outside the area
    g = goal.copy()
    g[0, :, :2] = [[1.0, 0.5], [7.0, -3.0]]
    assert _flags(cfg, agent, g, rect) == [0]
    # several at once, and per scene
    a = np.concatenate([agent, agent, agent])
    a[1, 0, :2], a[1, 1, :2] = [1.0, 0.5], [1.0, 0.52]
    a[2, 1, 0] = 2.0
    assert _flags(cfg, a, np.concatenate([goal] * 3), np.concatenate([rect] * 3)) == [0, SN.AGENTS_OVERLAP | SN.AGENT_IN_OBSTACLE,
                                                                                     SN.OUT_OF_AREA]


def test_validity_of_the_mpe_kinds():
    """discs: closer than car_radius + obs_radius = 0.1 to a centre; MPECorridor's y limit is twice the area (1.0)"""
    cfg = _cfg("MPESpread", 2, 2)
    agent = np.array([[[0.3, 0.3, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]], f32)
    goal = np.zeros((1, 2, 4), f32)
    disc = np.array([[[0.3, 0.42], [0.9, 0.2]]], f32)
    assert _flags(cfg, agent, goal, disc) == [0]
    disc[0, 0] = [0.3, 0.39]
    assert _flags(cfg, agent, goal, disc) == [SN.AGENT_IN_OBSTACLE]
    out = SN.scene_load_np(cfg, agent, goal, disc, None, None, 0.0, 1)
    np.testing.assert_array_equal(out["obst"], np.array([[[0.3, 0.39, 0, 0], [0.9, 0.2, 0, 0]]], f32))
    cor = _cfg("MPECorridor", 2, 0)
    assert cor.n_obs == 2 and cor.y_limit == 2.0
    far = np.array([[[0.5, 0.5], [0.5, 0.5]]], f32)
    far[0, :, 1] = [-5.0, 5.0]                                 # discs far from everyone
    a = agent.copy()
    a[0, 1, :2] = [0.9, 1.9]
    assert _flags(cor, a, goal, far) == [0]
    a[0, 1, 1] = 2.1
    assert _flags(cor, a, goal, far) == [SN.OUT_OF_AREA]
    a[0, 1, :2] = [1.1, 1.0]
    assert _flags(cor, a, goal, far) == [SN.OUT_OF_AREA]


def test_rectangle_record_is_the_reset_oracle_record():
    """the record of a scene's rectangle is Rectangle.create as oracle/env_np.py states it for the reset"""
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    out = SN.scene_load_np(cfg, agent, goal, rect, None, None, 0.0, 1)
    want = EN.make_rect(rect[..., :2], rect[..., 2], rect[..., 3], rect[..., 4])
    np.testing.assert_array_equal(out["obst"].view(np.uint32), want.view(np.uint32))
    rec = out["obst"][0, 0]
    assert rec[7] == 0 and rec[5] == f32(np.cos(f32(0.3))) and rec[6] == f32(np.sin(f32(0.3)))
    np.testing.assert_allclose(rec[8:].reshape(4, 2).mean(axis=0), [1.0, 0.5], atol=1e-6)


# ---- jitter ---------------------------------------------------------------------------------------------------------------------------
def test_draw_table():
    """attempt a, agent i -> draw a * n + i of the reset's stream; x from word 0, y from word 1, the other columns untouched"""
    assert [SN.draw_index(a, i, 3) for a in range(3) for i in range(3)] == list(range(9))
    assert SN.draw_index(15, 63, 64) == 16 * 64 - 1
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    seeds, J = np.array([12345678901234567, 5], np.int64), 0.05
    out = SN.scene_load_np(cfg, agent, goal, rect, None, seeds, J, 2)
    assert out["attempt"].tolist() == [0, 0] and out["flags"].tolist() == [0, 0] and out["n_failed"] == 0
    for b in range(2):
        st = EN._Stream(int(seeds[b]))                       # the reset oracle's own stream object, drawn in order
        for i in range(2):
            u0, u1 = st.uniform2()
            assert (u0, u1) == SN.uniforms(seeds[b], i)
            want = (f32(agent[0, i, 0] + f32(f32(f32(2) * u0 - f32(1)) * f32(J))), f32(agent[0, i, 1] + f32(f32(f32(2) * u1 - f32(1)) * f32(J))))
            assert (out["agent"][b, i, 0], out["agent"][b, i, 1]) == want
            assert abs(float(want[0]) - float(agent[0, i, 0])) <= J and abs(float(want[1]) - float(agent[0, i, 1])) <= J
        np.testing.assert_array_equal(out["agent"][b, :, 2:], agent[0, :, 2:])
    assert not np.array_equal(out["agent"][0], out["agent"][1]), "the seed keys the stream"
    np.testing.assert_array_equal(out["goal"], np.concatenate([goal, goal]))


RETRY_SEEDS = np.arange(1, 25, dtype=np.int64) * 7919


def retry_case():
    """LidarSpread n = 2 without obstacles: both agents on one spot, jitter 4 car_radius = 0.2"""
    cfg = _cfg("LidarSpread", 2, 0)
    agent = np.array([[[0.75, 0.75, 0.0, 0.0], [0.75, 0.75, 0.0, 0.0]]], f32)
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[0.2, 0.2], [1.3, 1.3]]
    return cfg, agent, goal, None, RETRY_SEEDS, 4 * 0.05


def stuck_case():
    """LidarSpread n = 2, one 0.4 x 0.4 square: agent 0 at its centre, jitter 1e-3"""
    cfg = _cfg("LidarSpread", 2, 1)
    agent = np.array([[[0.75, 0.75, 0.0, 0.0], [0.2, 0.2, 0.0, 0.0]]], f32)
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[0.2, 1.3], [1.3, 1.3]]
    rect = np.array([[[0.75, 0.75, 0.4, 0.4, 0.0]]], f32)
    return cfg, agent, goal, rect, RETRY_SEEDS[:5], 1e-3


def test_retry_until_valid_and_not_cumulative():
    """coincident agents become a valid scene on the first attempt that draws them >= 0.1 apart: the restatement's attempt is the
    first one an independent float64 look at the draws calls clear of the threshold, and the positions kept are the template plus
    that attempt's offset alone, never a sum over attempts"""
    cfg, agent, goal, _, seeds, J = retry_case()
    assert _flags(cfg, agent, goal, None) == [SN.AGENTS_OVERLAP]
    out = SN.scene_load_np(cfg, agent, goal, None, None, seeds, J, len(seeds))
    assert out["flags"].tolist() == [0] * len(seeds) and out["n_failed"] == 0
    assert out["attempt"].max() >= 1 and out["attempt"].min() == 0, "the case became trivial: no seed needs a second attempt"
    for b, seed in enumerate(seeds):
        first = None
        for a in range(SN.ATTEMPTS):
            (u0, u1), (w0, w1) = SN.uniforms(seed, SN.draw_index(a, 0, 2)), SN.uniforms(seed, SN.draw_index(a, 1, 2))
            dist = 2 * J * np.hypot(float(u0) - float(w0), float(u1) - float(w1))
            assert abs(dist - 0.1) > 1e-5, "a draw at the threshold: float64 cannot referee it"
            if dist >= 0.1:
                first = a
                break
        assert out["attempt"][b] == first, (b, first)
        for i in range(2):
            u0, u1 = SN.uniforms(seed, SN.draw_index(first, i, 2))
            assert (out["agent"][b, i, 0], out["agent"][b, i, 1]) == SN.jittered(agent[0, i], u0, u1, J)
        assert np.abs(out["agent"][b, :, :2].astype(np.float64) - 0.75).max() <= J + 1e-7, "never further than J from the template"


def test_retries_run_out_deep_inside_a_rectangle():
    cfg, agent, goal, rect, seeds, J = stuck_case()
    assert _flags(cfg, agent, goal, rect) == [SN.AGENT_IN_OBSTACLE]
    out = SN.scene_load_np(cfg, agent, goal, rect, None, seeds, J, len(seeds))
    assert out["flags"].tolist() == [SN.AGENT_IN_OBSTACLE] * len(seeds) and out["n_failed"] == len(seeds)
    assert out["attempt"].tolist() == [SN.ATTEMPTS - 1] * len(seeds)
    for b, seed in enumerate(seeds):                         # the last attempt stays
        for i in range(2):
            u0, u1 = SN.uniforms(seed, SN.draw_index(SN.ATTEMPTS - 1, i, 2))
            assert (out["agent"][b, i, 0], out["agent"][b, i, 1]) == SN.jittered(agent[0, i], u0, u1, J)


def test_scene_ids_and_the_default_wrap():
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    A = np.concatenate([agent, agent + f32(0.01), agent + f32(0.02)])
    G, Rc = np.concatenate([goal] * 3), np.concatenate([rect] * 3)
    out = SN.scene_load_np(cfg, A, G, Rc, None, None, 0.0, 5)
    np.testing.assert_array_equal(out["agent"], A[[0, 1, 2, 0, 1]])
    out = SN.scene_load_np(cfg, A, G, Rc, [2, 2, 0, 1, 2], None, 0.0, 5)
    np.testing.assert_array_equal(out["agent"], A[[2, 2, 0, 1, 2]])


# ---- the entry point's host refusals: nothing is launched, so they run without a GPU -------------------------------------------------------
def test_entry_point_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = _cfg("LidarSpread", 2, 1)
    buf = (C.c_float * 64)()                                  # never read: every call below returns before a launch
    p = C.cast(buf, C.c_void_p)

    def call(cfg=cfg, agent_t=p, goal_t=p, obst_t=p, S=1, ids=None, seeds=p, jitter=0.0, agent=p, goal=p, obst=p, flags=None,
             n_failed=None, B=1):
        return lib.dgppo_env_scene_load(C.byref(cfg), agent_t, goal_t, obst_t, S, ids, seeds, jitter, agent, goal, obst, flags, n_failed,
                                        B, None)
    assert call(B=0) == 0 and call(B=0, seeds=None) == 0       # a valid call of no envs launches nothing either
    bad_cfg = _cfg("LidarSpread", 2, 1)
    bad_cfg.kind = 17
    cases = [(dict(cfg=bad_cfg), b"unknown env kind"), (dict(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)), b"VMASReverseTransport"),
             (dict(S=0), b"S must be"), (dict(B=-1), b"B must be"), (dict(jitter=-0.1), b"jitter"), (dict(jitter=float("nan")), b"jitter"),
             (dict(agent_t=None), b"NULL"), (dict(goal_t=None), b"NULL"), (dict(agent=None), b"NULL"), (dict(goal=None), b"NULL"),
             (dict(obst_t=None), b"obst_t"), (dict(obst=None), b"obst must be NULL exactly"),
             (dict(cfg=_cfg("LidarSpread", 2, 0)), b"obst_t"), (dict(cfg=_cfg("LidarSpread", 2, 0), obst_t=None), b"obst must be NULL exactly"),
             (dict(jitter=0.1, seeds=None), b"seeds"),
             (dict(cfg=_cfg("LidarSpread", 65, 1)), b"64")]      # dgppo_validate_cfg has the same bound and speaks first
    for kw, word in cases:
        assert call(**kw) != 0, kw
        assert word in lib.dgppo_last_error(), (kw, lib.dgppo_last_error())
    assert call(cfg=_cfg("LidarSpread", 2, 0), obst_t=None, obst=None, B=0) == 0
    assert call(cfg=_cfg("LidarSpread", 64, 1), B=0) == 0


def test_binding_refusals():
    """ops_env.scene_load raises before it asks for a device pointer: host tensors get as far as the refusals"""
    from dgppo_amd import ops_env as OE
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    rows = dict(agent=torch.from_numpy(np.concatenate([agent] * 3)), goal=torch.from_numpy(np.concatenate([goal] * 3)),
                obst=torch.from_numpy(np.concatenate([rect] * 3)))
    st = OE.State.empty(cfg, 4, "cpu")
    seeds = torch.arange(4, dtype=torch.int64)
    for kw, match in ((dict(scene_ids=[0, 1, 3, 0]), r"scene_ids outside \[0, 3\)"), (dict(scene_ids=[0, -1, 2, 0]), "scene_ids outside"),
                      (dict(scene_ids=[0, 1]), "scene_ids must be 4 ints"), (dict(scene_ids=[0.0, 1.0, 2.0, 0.0]), "scene_ids must be 4 ints"),
                      (dict(jitter=-1.0), "jitter"), (dict(jitter=float("nan")), "jitter"), (dict(jitter=0.1, seeds=None), "seeds are required"),
                      (dict(seeds=seeds[:3]), "seeds"), (dict(flags=torch.zeros(3, dtype=torch.int32)), "flags"),
                      (dict(scenes_dev={k: v for k, v in rows.items() if k != "obst"}), "no obst"),
                      (dict(scenes_dev=dict(rows, goal=rows["goal"][:2])), "scenes_dev.goal")):
        args = dict(scenes_dev=rows, scene_ids=None, seeds=seeds, jitter=0.0, flags=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_load(cfg, args["scenes_dev"], args["scene_ids"], args["seeds"], args["jitter"], st, args["flags"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the refusals: the product path has no host kernel
        OE.scene_load(cfg, rows, [0, 1, 2, 0], seeds, 0.0, st)
    from dgppo_amd import _native as N
    vm = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.scene_load(vm, rows, None, None, 0.0, OE.State.empty(vm, 2, "cpu"))


# ---- Scenes: shapes, kinds, the file ---------------------------------------------------------------------------------------------------------
def test_template_shape_and_kind_refusals():
    from dgppo.env import Scenes, make_env
    from dgppo_amd.env import scenes as SC
    agent, goal, rect = _lidar_scene()
    cfg = _cfg("LidarSpread", 2, 1)
    rows = SC.check_templates(cfg, agent, goal, rect=rect)
    assert sorted(rows) == ["agent", "goal", "names", "obst"] and rows["names"] == ["scene0"] and rows["obst"].dtype == f32
    for kw, match in ((dict(agent=agent[:, :1]), "agent: expected shape"), (dict(agent=agent[0]), r"agent must be \[S, n, sd\]"),
                      (dict(goal=goal[:, :, :3]), "goal: expected shape"), (dict(rect=rect[..., :4]), "rect: expected shape"),
                      (dict(rect=None), "rect .* is required"), (dict(disc=rect[..., :2]), "disc rows are for the MPE kinds"),
                      (dict(goal=np.concatenate([goal, goal])), "goal: expected shape"), (dict(names=["a", "b"]), "2 names for 1 scenes")):
        args = dict(agent=agent, goal=goal, rect=rect, disc=None, names=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            SC.check_templates(cfg, **args)
    with pytest.raises(ValueError, match="no obstacles"):
        SC.check_templates(_cfg("LidarSpread", 2, 0), agent, goal, rect=rect)
    mpe = _cfg("MPESpread", 2, 1)
    with pytest.raises(ValueError, match="rect rows are for the LiDAR kinds"):
        SC.check_templates(mpe, agent, goal, rect=rect)
    assert SC.check_templates(mpe, agent, goal, disc=rect[..., :2])["obst"].shape == (1, 1, 2)
    line = _cfg("LidarLine", 3, 0)                           # two landmark rows whatever the team size
    with pytest.raises(ValueError, match=r"goal: expected shape \(1, 2, 4\)"):
        SC.check_templates(line, np.zeros((1, 3, 4), f32), np.zeros((1, 3, 4), f32))
    from dgppo_amd import _native as N
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        SC.check_templates(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), np.zeros((1, 4, 4), f32), np.zeros((1, 0, 4), f32))
    # through the class: refused before the device is asked for
    env = make_env("LidarSpread", 2, num_obs=1)
    with pytest.raises(ValueError, match="agent: expected shape"):
        Scenes(env, agent[:, :1], goal, rect=rect)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        Scenes(make_env("VMASReverseTransport", 4), np.zeros((1, 4, 4), f32), np.zeros((1, 0, 4), f32))
    assert SC.decode_flags(0) == "valid" and SC.decode_flags(5) == "NONFINITE | AGENTS_OVERLAP"
    assert SC.decode_flags(10) == "OUT_OF_AREA | AGENT_IN_OBSTACLE"


def test_npz_round_trip(tmp_path):
    from dgppo_amd.env import scenes as SC
    agent, goal, rect = _lidar_scene()
    agent = np.concatenate([agent, agent + f32(0.125)])
    agent.view(np.uint32)[1, 1, 3] = 0x7FC12345               # the file keeps words
    path = tmp_path / "two.npz"
    SC.write_npz(path, "LidarSpread", 2, agent, np.concatenate([goal] * 2), np.concatenate([rect] * 2), "rect", ["first", "second"])
    assert os.path.exists(path) and sorted(np.load(path).files) == ["agent", "env_id", "goal", "names", "num_agents", "rect"]
    z = SC.read_npz(path)
    assert z["env_id"] == "LidarSpread" and z["num_agents"] == 2 and z["names"] == ["first", "second"] and z["disc"] is None
    np.testing.assert_array_equal(z["agent"].view(np.uint32), agent.view(np.uint32))
    np.testing.assert_array_equal(z["rect"], np.concatenate([rect] * 2))
    SC.write_npz(path, "MPESpread", 2, agent, np.concatenate([goal] * 2), None, None, ["a", "b"])
    z = SC.read_npz(path)
    assert z["rect"] is None and z["disc"] is None and z["env_id"] == "MPESpread"
    np.savez(tmp_path / "other.npz", agent=agent)
    with pytest.raises(ValueError, match="not a scenes file"):
        SC.read_npz(tmp_path / "other.npz")


def test_bicycle_rows():
    from dgppo.env import Scenes
    rows = Scenes.bicycle_rows([0.2, 0.9], [0.3, 1.1], [0.0, np.pi / 2], 0.25)
    assert rows.shape == (2, 5) and rows.dtype == f32
    np.testing.assert_array_equal(rows[0], np.array([0.2, 0.3, 1.0, 0.0, 0.25], f32))
    np.testing.assert_array_equal(rows[1], np.array([0.9, 1.1, np.cos(f32(np.pi / 2)), 1.0, 0.25], f32))
    assert Scenes.bicycle_rows(np.zeros((3, 2)), 0.5, 0.1, 0.0).shape == (3, 2, 5)


# ---- the committed fixtures --------------------------------------------------------------------------------------------------------------
def test_headon_fixture_is_scene_a_word_for_word():
    from dgppo_amd.env import scenes as SC
    z = SC.read_npz(os.path.join(GOLDEN, "lidarspread_n2_headon.npz"))
    _, agent, goal, obst = R.scene_a()
    assert z["env_id"] == "LidarSpread" and z["num_agents"] == 2 and z["names"] == ["headon"] and z["disc"] is None
    for got, want in ((z["agent"], agent), (z["goal"], goal), (z["rect"], obst[..., :5])):
        assert got.dtype == f32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    cfg = _cfg("LidarSpread", 2, 1)
    out = SN.scene_load_np(cfg, z["agent"], z["goal"], z["rect"], None, None, 0.0, 1)
    assert out["flags"].tolist() == [0]
    np.testing.assert_array_equal(out["obst"].view(np.uint32), obst.view(np.uint32))           # the whole record, corners included


def test_the_other_fixtures():
    from dgppo_amd.env import scenes as SC
    z = SC.read_npz(os.path.join(GOLDEN, "lidarspread_n2_lookahead.npz"))
    assert z["names"] == ["mover0", "mover1"]
    for mover in (0, 1):
        _, agent, goal, obst = L.scene(mover)
        for got, want in ((z["agent"], agent), (z["goal"], goal), (z["rect"], obst[..., :5])):
            assert np.array_equal(got[mover:mover + 1].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert SN.scene_load_np(_cfg("LidarSpread", 2, 1), z["agent"], z["goal"], z["rect"], None, None, 0.0, 2)["flags"].tolist() == [0, 0]
    z = SC.read_npz(os.path.join(GOLDEN, "mpespread_n3_swap_wall.npz"))
    assert z["env_id"] == "MPESpread" and z["num_agents"] == 3 and z["names"] == ["swap", "wall"] and z["rect"] is None
    assert z["disc"].shape == (2, 2, 2)
    assert SN.scene_load_np(_cfg("MPESpread", 3, 2), z["agent"], z["goal"], z["disc"], None, None, 0.0, 2)["flags"].tolist() == [0, 0]


# ---- test.py ---------------------------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_scene_flags():
    mod = _load_test_py()
    assert mod.SCENE_FLAGS == [(("--scenes",), "str", None), (("--scene-jitter",), "float", 0.0)]
    assert len(mod.FLAGS) == 18
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.scenes is None and args.scene_jitter == 0.0
    args = ap.parse_args(["--path", "x", "--scenes", "a.npz", "--scene-jitter", "0.05", "--shield", "--shield-horizon", "4"])
    assert args.scenes == "a.npz" and args.scene_jitter == 0.05 and args.shield
    assert "--scenes" in mod.__doc__ and "--scene-jitter" in mod.__doc__
    # before anything is loaded: the path does not exist
    with pytest.raises(SystemExit, match="--scene-jitter needs --scenes"):
        mod.main(["--path", "/nonexistent/run", "--scene-jitter", "0.05"])
    with pytest.raises(SystemExit, match="--scene-jitter must be >= 0"):
        mod.main(["--path", "/nonexistent/run", "--scenes", "a.npz", "--scene-jitter", "-0.1"])


def test_algo_scene_start_defaults_use_the_global_env_index():
    """_scene_start: without scenes nothing changes and stray arguments are refused; one rank leaves the default to the kernel
    (b % S); several ranks spell out (rank * B + b) % S"""
    from dgppo_amd.algo.dgppo import DGPPO
    from dgppo_amd.env.scenes import SceneStart

    class FakeScenes:
        S, cfg = 3, _cfg("LidarSpread", 2, 1)

        def start(self, ids, jitter):
            return SceneStart(self, ids, jitter)

    class FakeEnv:
        cfg = _cfg("LidarSpread", 2, 1)
    algo = DGPPO.__new__(DGPPO)
    algo._env, algo.world, algo.rank = FakeEnv(), 1, 0
    assert algo._scene_start(None, None, 0.0, 4) is None
    for kw in (dict(scene_ids=[0]), dict(jitter=0.1)):
        with pytest.raises(ValueError, match="need scenes"):
            algo._scene_start(None, kw.get("scene_ids"), kw.get("jitter", 0.0), 4)
    sc = FakeScenes()
    assert algo._scene_start(sc, None, 0.0, 4) == SceneStart(sc, None, 0.0)
    assert algo._scene_start(sc, [2, 2, 1, 0], 0.25, 4) == SceneStart(sc, [2, 2, 1, 0], 0.25)
    algo.world, algo.rank = 2, 1
    assert algo._scene_start(sc, None, 0.0, 4).scene_ids.tolist() == [1, 2, 0, 1]          # global envs 4 .. 7
    algo._env.cfg = _cfg("LidarSpread", 3, 1)
    with pytest.raises(ValueError, match="do not fit"):
        algo._scene_start(sc, None, 0.0, 4)
