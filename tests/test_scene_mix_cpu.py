"""The scene mix of a training batch without a GPU: the assignment rule (env/scenes.mix_assignment), the host refusals of
dgppo_env_scene_mix and of its bindings, and train.py's three flags with their checks before any rank starts."""
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
from test_scenes_cpu import GOLDEN, _cfg, _lidar_scene  # noqa: E402

ROOT = os.path.dirname(HERE)
f32 = np.float32
HEADON = os.path.join(GOLDEN, "lidarspread_n2_headon.npz")


# ---- the assignment ---------------------------------------------------------------------------------------------------------------------
def _mix(*a):
    from dgppo_amd.env.scenes import mix_assignment
    return mix_assignment(*a)


@pytest.mark.parametrize("n_total,n_scene,S", [(16, 8, 3), (16, 5, 3), (16, 1, 1), (128, 13, 4), (12, 11, 5), (7, 3, 2)])
def test_assignment_counts_order_and_rotation(n_total, n_scene, S):
    for step in (0, 1, 7):
        of = _mix(n_total, n_scene, S, step, 0, n_total)
        assert of.dtype == np.int32 and of.shape == (n_total,)
        assert int((of >= 0).sum()) == n_scene and set(of[of < 0].tolist()) <= {-1}
        # the rule itself, spelled out per env
        k = 0
        for g in range(n_total):
            scene_env = (g + 1) * n_scene // n_total > g * n_scene // n_total
            assert (of[g] >= 0) == scene_env
            if scene_env:
                assert g * n_scene // n_total == k and of[g] == (k + step) % S, "ordinals 0 .. n_scene - 1 in order"
                k += 1
        assert k == n_scene
        np.testing.assert_array_equal(of[of >= 0], (np.arange(n_scene) + step) % S)
    # the scenes rotate with the step and come round after S steps
    a, b = _mix(n_total, n_scene, S, 0, 0, n_total), _mix(n_total, n_scene, S, S, 0, n_total)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal((_mix(n_total, n_scene, S, 1, 0, n_total) >= 0), a >= 0)
    # evenly spread: between two scene envs lie floor or ceil (n_total / n_scene) - 1 others
    idx = np.flatnonzero(a >= 0)
    if n_scene > 1:
        gaps = np.diff(idx)
        assert gaps.min() >= n_total // n_scene and gaps.max() <= -(-n_total // n_scene)


def test_assignment_windows_of_the_ranks_are_the_one_rank_result():
    for n_total, n_scene, S, step in ((16, 8, 3, 0), (16, 5, 3, 2), (128, 13, 4, 9), (8, 8, 2, 1)):
        whole = _mix(n_total, n_scene, S, step, 0, n_total)
        for world in (1, 2, 4):
            share = n_total // world
            parts = [_mix(n_total, n_scene, S, step, r * share, (r + 1) * share) for r in range(world)]
            assert all(p.shape == (share,) for p in parts)
            np.testing.assert_array_equal(np.concatenate(parts), whole)
    np.testing.assert_array_equal(_mix(5, 5, 2, 0, 0, 5), [0, 1, 0, 1, 0])         # n_scene == n_total: every env
    np.testing.assert_array_equal(_mix(5, 5, 2, 3, 0, 5), [1, 0, 1, 0, 1])
    assert _mix(6, 0, 2, 0, 0, 6).tolist() == [-1] * 6 and _mix(6, 3, 2, 0, 2, 2).shape == (0,)
    for bad in ((4, 5, 1, 0, 0, 4), (4, 2, 0, 0, 0, 4), (4, 2, 1, 0, 3, 2), (4, 2, 1, 0, 0, 5), (4, -1, 1, 0, 0, 4)):
        with pytest.raises(ValueError, match="mix_assignment"):
            _mix(*bad)


def test_scene_mix_tuple_and_scenes_mix():
    from dgppo.env import SceneMix, SceneStart
    from dgppo_amd.env.scenes import Scenes
    assert SceneMix._fields == ("scenes", "scene_of", "jitter") and SceneStart._fields == ("scenes", "scene_ids", "jitter")
    sc = Scenes.__new__(Scenes)
    m = sc.mix([0, -1, 1], 0.25)
    assert isinstance(m, SceneMix) and m.scenes is sc and m.scene_of.tolist() == [0, -1, 1] and m.jitter == 0.25
    assert not isinstance(sc.start(), SceneMix) and len(sc.start()) == 3


# ---- the entry point's host refusals: nothing is launched, so they run without a GPU ----------------------------------------------------
def test_entry_point_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = _cfg("LidarSpread", 2, 1)
    buf = (C.c_float * 64)()                                  # never read: every call below returns before a launch
    p = C.cast(buf, C.c_void_p)

    def call(cfg=cfg, agent_t=p, goal_t=p, obst_t=p, S=1, scene_of=p, seeds=p, jitter=0.0, agent=p, goal=p, obst=p, flags=None,
             n_fallback=None, B=1):
        return lib.dgppo_env_scene_mix(C.byref(cfg), agent_t, goal_t, obst_t, S, scene_of, seeds, jitter, agent, goal, obst, flags,
                                       n_fallback, B, None)
    assert call(B=0) == 0
    bad_cfg = _cfg("LidarSpread", 2, 1)
    bad_cfg.kind = 17
    cases = [(dict(cfg=bad_cfg), b"unknown env kind"), (dict(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)), b"VMASReverseTransport"),
             (dict(S=0), b"S must be"), (dict(S=-2), b"S must be"), (dict(B=-1), b"B must be"), (dict(jitter=-0.1), b"jitter"),
             (dict(jitter=float("nan")), b"jitter"), (dict(agent_t=None), b"NULL"), (dict(goal_t=None), b"NULL"),
             (dict(agent=None), b"NULL"), (dict(goal=None), b"NULL"), (dict(scene_of=None), b"scene_of"), (dict(seeds=None), b"seeds"),
             (dict(obst_t=None), b"obst_t"), (dict(obst=None), b"obst must be NULL exactly"),
             (dict(cfg=_cfg("LidarSpread", 2, 0)), b"obst_t"), (dict(cfg=_cfg("LidarSpread", 2, 0), obst_t=None), b"obst must be NULL exactly"),
             (dict(cfg=_cfg("LidarSpread", 65, 1)), b"64")]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        err = lib.dgppo_last_error()
        assert word in err and b"dgppo_env_scene_mix" in err, (kw, err)
    assert call(cfg=_cfg("LidarSpread", 2, 0), obst_t=None, obst=None, B=0) == 0
    assert call(cfg=_cfg("LidarSpread", 64, 1), B=0) == 0


def test_binding_refusals():
    """ops_env.scene_mix and mixed_start raise before they ask for a device pointer: host tensors get as far as the refusals"""
    from dgppo_amd import _native as N
    from dgppo_amd import ops_env as OE
    cfg = _cfg("LidarSpread", 2, 1)
    agent, goal, rect = _lidar_scene()
    rows = dict(agent=torch.from_numpy(np.concatenate([agent] * 3)), goal=torch.from_numpy(np.concatenate([goal] * 3)),
                obst=torch.from_numpy(np.concatenate([rect] * 3)))
    st = OE.State.empty(cfg, 4, "cpu")
    seeds = torch.arange(4, dtype=torch.int64)
    cases = ((dict(scene_of=[0, 1, 3, -1]), r"scene_of outside \[-inf, 3\)"), (dict(scene_of=[0, 1]), "scene_of must be 4 ints"),
             (dict(scene_of=[0.0, -1.0, 2.0, 0.0]), "scene_of must be 4 ints"), (dict(scene_of=None), "scene_of is required"),
             (dict(jitter=-1.0), "jitter"), (dict(jitter=float("nan")), "jitter"), (dict(seeds=None), "seeds are required"),
             (dict(seeds=seeds[:3]), "seeds"), (dict(flags=torch.zeros(3, dtype=torch.int32)), "flags"),
             (dict(n_fallback=torch.zeros(2, dtype=torch.int32)), "n_fallback"),
             (dict(scenes_dev={k: v for k, v in rows.items() if k != "obst"}), "no obst"),
             (dict(scenes_dev=dict(rows, goal=rows["goal"][:2])), "scenes_dev.goal"))
    for kw, match in cases:
        args = dict(scenes_dev=rows, scene_of=[0, -1, 2, -5], seeds=seeds, jitter=0.0, flags=None, n_fallback=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_mix(cfg, args["scenes_dev"], args["scene_of"], args["seeds"], args["jitter"], st, args["flags"], args["n_fallback"])
        if "flags" not in kw:                                 # mixed_start: the same refusals, before its reset is launched
            with pytest.raises(ValueError, match=match):
                OE.mixed_start(cfg, args["seeds"], st, args["scenes_dev"], args["scene_of"], args["jitter"], None, args["n_fallback"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the refusals: the product path has no host kernel
        OE.scene_mix(cfg, rows, [0, -1, 2, -7], seeds, 0.0, st)
    vm = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.scene_mix(vm, rows, [0, 0], seeds[:2], 0.0, OE.State.empty(vm, 2, "cpu"))
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.mixed_start(vm, seeds[:2], OE.State.empty(vm, 2, "cpu"), rows, [0, 0], 0.0)


def test_algo_scene_of_refusals():
    """_scene_start: scene_of needs scenes, excludes scene_ids and has one entry per key; with it the start is a SceneMix"""
    from dgppo_amd.algo.dgppo import DGPPO
    from dgppo_amd.algo.informarl import InforMARL
    from dgppo_amd.env.scenes import SceneMix, SceneStart

    class FakeScenes:
        S, cfg = 3, _cfg("LidarSpread", 2, 1)

        def start(self, ids, jitter):
            return SceneStart(self, ids, jitter)

        def mix(self, of, jitter):
            return SceneMix(self, np.asarray(of), jitter)

    class FakeEnv:
        cfg = _cfg("LidarSpread", 2, 1)
    for cls in (DGPPO, InforMARL):
        algo = cls.__new__(cls)
        algo._env, algo.world, algo.rank = FakeEnv(), 1, 0
        sc = FakeScenes()
        with pytest.raises(ValueError, match="need scenes"):
            algo._scene_start(None, None, 0.0, 4, scene_of=[0, -1, 0, -1])
        with pytest.raises(ValueError, match="scene_of and scene_ids exclude each other"):
            algo._scene_start(sc, [0, 0, 0, 0], 0.0, 4, scene_of=[0, -1, 0, -1])
        with pytest.raises(ValueError, match="one entry per key"):
            algo._scene_start(sc, None, 0.0, 4, scene_of=[0, -1, 0])
        m = algo._scene_start(sc, None, 0.05, 4, scene_of=[2, -1, 0, -1])
        assert isinstance(m, SceneMix) and m.scene_of.tolist() == [2, -1, 0, -1] and m.jitter == 0.05
        algo.world, algo.rank = 2, 1                           # a mix is the caller's window: no default to spell out
        assert algo._scene_start(sc, None, 0.0, 4, scene_of=[-1, -1, 1, -1]).scene_of.tolist() == [-1, -1, 1, -1]
        assert algo._scene_start(sc, None, 0.0, 4).scene_ids.tolist() == [1, 2, 0, 1]          # and today's path is today's
    import inspect
    for cls in (DGPPO, InforMARL):
        assert list(inspect.signature(cls.collect).parameters)[1:] == ["params", "keys", "scenes", "scene_ids", "jitter", "scene_of"]


# ---- train.py -----------------------------------------------------------------------------------------------------------------------------
def _load_train_py():
    spec = importlib.util.spec_from_file_location("dgppo_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--env", "LidarSpread", "-n", "2", "--algo", "dgppo", "--obs", "1"]


def test_train_py_flags():
    mod = _load_train_py()
    names = [n[-1] for n, _, _ in mod.FLAGS]
    assert names[-2:] == ["--gpus", "--resume"] and names[-5:-2] == ["--scenes", "--scene-frac", "--scene-jitter"]
    assert [(k, d) for n, k, d in mod.FLAGS if n[-1].startswith("--scene")] == [("str", None), ("float", 0.0), ("float", 0.0)]
    ap = mod.build_parser()
    a = ap.parse_args(BASE)
    assert a.scenes is None and a.scene_frac == 0.0 and a.scene_jitter == 0.0
    mod.check_scenes(a)                                       # without the flags nothing is asked
    a = ap.parse_args(BASE + ["--scenes", HEADON, "--scene-frac", "0.5", "--scene-jitter", "0.05"])
    assert a.scenes == HEADON and a.scene_frac == 0.5 and a.scene_jitter == 0.05
    mod.check_scenes(a)
    stored = mod._flags_to_store(a)
    assert stored["scenes"] == HEADON and stored["scene_frac"] == 0.5 and stored["scene_jitter"] == 0.05


def test_train_py_scene_checks_fire_before_any_rank_starts(tmp_path):
    mod = _load_train_py()
    ap = mod.build_parser()
    mpe = os.path.join(GOLDEN, "mpespread_n3_swap_wall.npz")
    cases = [(["--scene-frac", "0.5"], "--scene-frac needs --scenes"), (["--scene-jitter", "0.05"], "--scene-jitter needs --scenes"),
             (["--scenes", HEADON], r"--scene-frac must be in \(0, 1\]"), (["--scenes", HEADON, "--scene-frac", "1.5"], "--scene-frac must be"),
             (["--scenes", HEADON, "--scene-frac", "-0.5"], "--scene-frac must be"),
             (["--scenes", HEADON, "--scene-frac", "nan"], "--scene-frac must be"),
             (["--scenes", HEADON, "--scene-frac", "0.5", "--scene-jitter", "-0.1"], "--scene-jitter must be >= 0"),
             (["--scenes", str(tmp_path / "none.npz"), "--scene-frac", "0.5"], "--scenes .*none.npz: no such file"),
             (["--scenes", mpe, "--scene-frac", "0.5"], "--scenes: .*scenes of MPESpread with 3 agents, the env is LidarSpread with 2"),
             (["--scenes", HEADON, "--scene-frac", "0.5", "-n", "3"], "--scenes: .*with 2 agents, the env is LidarSpread with 3"),
             (["--scenes", HEADON, "--scene-frac", "0.5", "--env", "VMASReverseTransport"], "--scenes: VMASReverseTransport"),
             (["--scenes", HEADON, "--scene-frac", "0.03", "--n-env-train", "16"], "--scene-frac 0.03 of --n-env-train 16"),
             ]
    for extra, match in cases:
        with pytest.raises(SystemExit, match=match):
            mod.check_scenes(ap.parse_args(BASE + extra))
    mod.check_scenes(ap.parse_args(BASE + ["--scenes", HEADON, "--scene-frac", "0.04", "--n-env-train", "16"]))     # floor(0.64 + 0.5) = 1
    mod.check_scenes(ap.parse_args(BASE + ["--scenes", HEADON, "--scene-frac", "1.0"]))
    from dgppo.trainer.trainer import scene_count
    assert [scene_count(p, 16) for p in (0.03, 0.04, 0.5, 1.0)] == [0, 1, 8, 16]


def test_resume_names_the_scene_flag_that_differs():
    mod = _load_train_py()
    ap = mod.build_parser()
    a = ap.parse_args(BASE + ["--scenes", HEADON, "--scene-frac", "0.5", "--scene-jitter", "0.05"])
    stored = mod._flags_to_store(a)
    mod.check_resume_flags(a, stored)
    b = ap.parse_args(BASE + ["--scenes", HEADON, "--scene-frac", "0.25", "--scene-jitter", "0.05"])
    with pytest.raises(SystemExit, match=r"--scene-frac \(0.5 in the stopped run, 0.25 now\)") as ex:
        mod.check_resume_flags(b, stored)
    assert "--scene-jitter" not in str(ex.value) and "--scenes" not in str(ex.value)
    c = ap.parse_args(BASE + ["--scenes", HEADON + ".other", "--scene-frac", "0.5", "--scene-jitter", "0.0"])
    with pytest.raises(SystemExit) as ex:                     # the path is compared, not the file's content
        mod.check_resume_flags(c, stored)
    assert "--scenes (" in str(ex.value) and "--scene-jitter (" in str(ex.value) and "--scene-frac" not in str(ex.value)
    old = {k: v for k, v in stored.items() if not k.startswith("scene")}          # a run stopped before the flags existed ran
    mod.check_resume_flags(ap.parse_args(BASE), old)                                # without them: it resumes without them only
    with pytest.raises(SystemExit, match=r"--scene-frac \(0.0 in the stopped run, 0.5 now\)"):
        mod.check_resume_flags(a, old)
