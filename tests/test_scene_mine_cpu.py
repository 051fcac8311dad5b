"""Scene mining without a GPU: the NumPy restatement of dgppo_env_scene_mine / dgppo_env_scene_pool_push (tests/scene_mine_np.py) on
hand-written cost arrays and ring sequences, the host refusals of the two entry points, of their bindings, of ScenePool and of the
flags of train.py and test.py, and — by the oracle env step — the precondition of the head-on GPU test.  Everything compared is
integers or copied words."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_mine_np as MN  # noqa: E402
import scenes_np as SN  # noqa: E402
from test_scene_mix_cpu import BASE, HEADON, _load_train_py  # noqa: E402
from test_scenes_cpu import _cfg, _lidar_scene, _load_test_py  # noqa: E402

f32 = np.float32
SENT = 0xDEADBEEF


# ---- the cost scan --------------------------------------------------------------------------------------------------------------------
def _hand_record():
    cases = MN.hand_cases()
    cost_tm = np.stack([c for c, _, _ in cases.values()], axis=1)              # [T, B, 2, 2]
    return list(cases), cost_tm, [f for _, f, _ in cases.values()], [w for _, _, w in cases.values()]


def test_first_unsafe_known_answers():
    names, cost_tm, first, who = _hand_record()
    assert {"never", "at_start", "at_end", "equal_to_thresh", "one_ulp_below", "nan_and_minus_inf", "plus_inf", "two_agents"} <= set(names)
    got_first, got_who = MN.first_unsafe(cost_tm, MN.THRESH)
    assert dict(zip(names, got_first.tolist())) == dict(zip(names, first))
    assert dict(zip(names, got_who.tolist())) == dict(zip(names, who))
    below = np.nextafter(MN.THRESH, f32(-1), dtype=f32)
    assert below < MN.THRESH and cost_tm[2, names.index("one_ulp_below"), 1, 1] == below
    assert cost_tm[2, names.index("equal_to_thresh"), 1, 1] == MN.THRESH
    # test.py's rule: thresh 0.0 sees the same steps here (every planted cost is > 0 or far below)
    f0, _ = MN.first_unsafe(cost_tm, 0.0)
    assert f0[names.index("one_ulp_below")] == 2 and f0[names.index("never")] == -1


def _hand_mined(back):
    """the hand record over LidarSpread 2 / 1 rows: every step's agents valid and distinct, but the `two_agents` env, whose agents
    overlap at step 2 and at no other"""
    names, cost_tm, first, who = _hand_record()
    cfg = _cfg("LidarSpread", 2, 1)
    a0, g0, r0 = _lidar_scene()
    T, B = cost_tm.shape[:2]
    agent_tm = np.tile(a0[None], (T + 1, B, 1, 1)).astype(f32)
    agent_tm[..., 0] += (0.01 * np.arange(T + 1, dtype=f32))[:, None, None]     # step t is told apart by its x
    agent_tm[..., 2] += (0.001 * np.arange(B, dtype=f32))[None, :, None]        # env b by its vx
    b2 = names.index("two_agents")
    agent_tm[2, b2, 1, :2] = agent_tm[2, b2, 0, :2] + f32(0.01)
    goal = np.tile(g0, (B, 1, 1)).astype(f32)
    obst = SN.obstacle_rows(cfg, r0[0])[None].repeat(B, axis=0).astype(f32)
    return names, cfg, agent_tm, cost_tm, goal, obst, MN.mine_np(cfg, agent_tm, cost_tm, goal, obst, back, MN.THRESH, SENT)


def test_mined_rows_flags_and_take_rule():
    for back in (0, 2, 100):
        names, cfg, agent_tm, cost_tm, goal, obst, m = _hand_mined(back)
        ix = names.index
        for b, name in enumerate(names):
            f = m["first"][b]
            if f < 0:
                assert m["t0"][b] == -1 and m["who"][b] == -1 and m["flags"][b] == 0
                for k in ("agent", "goal", "obst"):
                    assert (m[k][b].view(np.uint32) == SENT).all(), f"{name}: {k} of a never-unsafe env was written"
                continue
            assert m["t0"][b] == max(f - back, 0)
            assert np.array_equal(m["agent"][b].view(np.uint32), agent_tm[m["t0"][b], b].view(np.uint32))
            assert np.array_equal(m["goal"][b].view(np.uint32), goal[b].view(np.uint32))
            assert np.array_equal(m["obst"][b].view(np.uint32), obst[b, :, :5].view(np.uint32))
        if back == 100:
            assert set(m["t0"][m["first"] >= 0].tolist()) == {0}
        if back == 0:
            assert np.array_equal(m["t0"], m["first"])
        # two_agents fails at step 4: back = 2 lands on the overlapping pair, the other offsets do not
        assert m["flags"][ix("two_agents")] == (SN.AGENTS_OVERLAP if back == 2 else 0)
        took = MN.taken(m["first"], m["flags"])
        assert not took[ix("at_start")] and not took[ix("never")] and took[ix("at_end")] and took[ix("equal_to_thresh")]
        assert took[ix("two_agents")] == (back != 2)


# ---- the ring -------------------------------------------------------------------------------------------------------------------------
def _rows(B, salt):
    return {"agent": (np.arange(B * 8, dtype=f32).reshape(B, 2, 4) + salt), "goal": (np.arange(B * 8, dtype=f32).reshape(B, 2, 4) - salt),
            "obst": None}


def _empty_pool(M):
    return {"agent": np.full((M, 2, 4), np.nan, f32), "goal": np.full((M, 2, 4), np.nan, f32), "obst": None}


def _mask(B, taken_envs):
    first, flags = np.full(B, -1, np.int32), np.zeros(B, np.int32)
    first[list(taken_envs)] = 3
    return first, flags


def test_ring_known_answers():
    B, M = 8, 4
    rows = _rows(B, 100)
    # count = 0: nothing moves
    pool, st, slot = MN.push_np(*_mask(B, []), rows, _empty_pool(M), 0, [0, 0, 0, 0])
    assert st == [0, 0, 0, 0] and slot.tolist() == [-1] * B and np.isnan(pool["agent"]).all()
    # count < R
    pool, st, slot = MN.push_np(*_mask(B, [1, 5]), rows, _empty_pool(M), 0, [0, 0, 0, 0])
    assert st == [2, 2, 2, 2] and slot.tolist() == [-1, 0, -1, -1, -1, 1, -1, -1]
    assert np.array_equal(pool["agent"][0], rows["agent"][1]) and np.array_equal(pool["goal"][1], rows["goal"][5])
    assert np.isnan(pool["agent"][2:]).all(), "unwritten slots keep their NaN words"
    # count = R
    pool, st, slot = MN.push_np(*_mask(B, [0, 2, 4, 6]), rows, _empty_pool(M), 0, [0, 0, 0, 0])
    assert st == [0, 4, 4, 4] and slot[[0, 2, 4, 6]].tolist() == [0, 1, 2, 3]
    # count > R: later ranks dropped, taken_last still counts them
    pool, st, slot = MN.push_np(*_mask(B, [0, 1, 2, 3, 4, 7]), rows, _empty_pool(M), 0, [0, 0, 0, 0])
    assert st == [0, 4, 4, 6] and slot.tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    # two pushes that wrap: 3, then 3 more from head 3
    pool, st, _ = MN.push_np(*_mask(B, [0, 1, 2]), rows, _empty_pool(M), 0, [0, 0, 0, 0])
    rows2 = _rows(B, 500)
    pool, st, slot = MN.push_np(*_mask(B, [3, 4, 5]), rows2, pool, 0, st)
    assert st == [2, 4, 6, 3] and slot[[3, 4, 5]].tolist() == [3, 0, 1]
    assert np.array_equal(pool["agent"][0], rows2["agent"][4]) and np.array_equal(pool["agent"][2], rows["agent"][2])
    # fixed > 0 is never written: M = 4, fixed = 2 -> a ring of two slots behind two pinned ones
    start = _empty_pool(M)
    start["agent"][:2], start["goal"][:2] = 7.0, 9.0
    pool, st, slot = MN.push_np(*_mask(B, [1, 2, 6]), rows, start, 2, [1, 0, 0, 0])
    assert st == [1, 2, 2, 3] and slot[[1, 2, 6]].tolist() == [3, 2, -1]
    assert (pool["agent"][:2] == 7.0).all() and (pool["goal"][:2] == 9.0).all()
    # the take rule inside the push: a failure at step 0 and a flagged env are passed over
    first, flags = np.array([0, 3, 3, -1], np.int32), np.array([0, 4, 0, 0], np.int32)
    _, st, slot = MN.push_np(first, flags, _rows(4, 0), _empty_pool(2), 0, [0, 0, 0, 0])
    assert st == [1, 1, 1, 1] and slot.tolist() == [-1, -1, 0, -1]


# ---- refusals that touch no device -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = _cfg("LidarSpread", 2, 1)
    x = C.c_void_p(64)                                        # never dereferenced: every call below is refused before a launch

    def mine(cfg=cfg, Bs=4, T=5, back=2, thresh=1e-6, B=4, **over):
        q = dict(agent_tm=x, cost_tm=x, goal=x, obst=x, first=x, who=x, t0=x, flags=x, agent_t=x, goal_t=x, obst_t=x)
        q.update(over)
        return lib.dgppo_env_scene_mine(C.byref(cfg), q["agent_tm"], q["cost_tm"], Bs, q["goal"], q["obst"], T, back, thresh, q["first"],
                                        q["who"], q["t0"], q["flags"], q["agent_t"], q["goal_t"], q["obst_t"], B, None)

    def push(cfg=cfg, M=4, fixed=0, B=4, **over):
        q = dict(first=x, flags=x, agent_t=x, goal_t=x, obst_t=x, pool_agent=x, pool_goal=x, pool_obst=x, state=x, slot_of=x)
        q.update(over)
        return lib.dgppo_env_scene_pool_push(C.byref(cfg), q["first"], q["flags"], q["agent_t"], q["goal_t"], q["obst_t"],
                                             q["pool_agent"], q["pool_goal"], q["pool_obst"], M, fixed, q["state"], q["slot_of"], B, None)
    bad = _cfg("LidarSpread", 2, 1)
    bad.kind = 17
    vmas = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 2, 0)
    no_obs = _cfg("LidarSpread", 2, 0)
    for kw in (dict(cfg=bad), dict(cfg=vmas), dict(B=-1), dict(Bs=3), dict(T=0), dict(T=-2), dict(back=-1), dict(thresh=float("nan")),
               dict(thresh=float("inf")), dict(agent_tm=None), dict(cost_tm=None), dict(goal=None), dict(obst=None), dict(first=None),
               dict(who=None), dict(t0=None), dict(flags=None), dict(agent_t=None), dict(goal_t=None), dict(obst_t=None),
               dict(cfg=no_obs), dict(cfg=no_obs, obst=None), dict(cfg=_cfg("LidarSpread", 65, 1)), dict(T=2 ** 30)):
        assert mine(**kw) != 0, kw
        assert b"dgppo_env_scene_mine" in lib.dgppo_last_error(), (kw, lib.dgppo_last_error())
    for kw in (dict(cfg=bad), dict(cfg=vmas), dict(B=-1), dict(M=0), dict(M=-4), dict(fixed=-1), dict(fixed=4), dict(M=1, fixed=1),
               dict(first=None), dict(flags=None), dict(agent_t=None), dict(goal_t=None), dict(obst_t=None), dict(pool_agent=None),
               dict(pool_goal=None), dict(pool_obst=None), dict(state=None), dict(cfg=no_obs), dict(cfg=no_obs, obst_t=None),
               dict(cfg=_cfg("LidarSpread", 65, 1))):
        assert push(**kw) != 0, kw
        assert b"dgppo_env_scene_pool_push" in lib.dgppo_last_error(), (kw, lib.dgppo_last_error())
    assert mine(B=0) == 0                                     # nothing to mine: no launch


def test_binding_and_class_refusals():
    from dgppo_amd import _native as N
    from dgppo_amd import ops_env as OE
    from dgppo_amd.algo.dgppo import DGPPO
    from dgppo_amd.algo.informarl import HCBFCRPO, InforMARL, InforMARLLagr
    from dgppo_amd.env import scenes as SC
    cfg = _cfg("LidarSpread", 2, 1)
    T, B = 4, 3
    agent_tm, cost_tm = torch.zeros(T + 1, B, 2, 4), torch.zeros(T, B, 2, 2)
    goal, obst = torch.zeros(B, 2, 4), torch.zeros(B, 1, 16)
    out = OE.alloc_mined(cfg, B, "cpu")
    assert {k: tuple(v.shape) for k, v in out.items()} == {"first": (B,), "who": (B,), "t0": (B,), "flags": (B,), "agent": (B, 2, 4),
                                                           "goal": (B, 2, 4), "obst": (B, 1, 5)}
    wide_a, wide_c = torch.zeros(T + 1, B + 2, 2, 4), torch.zeros(T, B + 2, 2, 2)
    assert OE._time_major(wide_a[:, :B], T + 1, B, (2, 4), "agent_tm") == B + 2 and OE._time_major(agent_tm, T + 1, B, (2, 4), "a") == B
    for kw, match in ((dict(agent_tm=agent_tm[:, :, :, :3]), "agent_tm"), (dict(cost_tm=cost_tm[:3]), "cost_tm"),
                      (dict(agent_tm=agent_tm.transpose(0, 1).contiguous().transpose(0, 1)), "time-major"),
                      (dict(agent_tm=wide_a[:, :B]), "same number of envs"), (dict(goal=goal[:2]), "goal"), (dict(obst=None), "obst"),
                      (dict(back=-1), "back must be >= 0"), (dict(thresh=float("nan")), "thresh must be finite"),
                      (dict(out={**out, "first": out["first"][:2]}), "out.first"), (dict(out={**out, "obst": out["agent"]}), "out.obst")):
        a = dict(agent_tm=agent_tm, cost_tm=cost_tm, goal=goal, obst=obst, back=2, thresh=1e-6, out=out)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_mine(cfg, a["agent_tm"], a["cost_tm"], a["goal"], a["obst"], a["back"], a["thresh"], a["out"])
    with pytest.raises((RuntimeError, TypeError), match="GPU"):                   # past the refusals: there is no host kernel
        OE.scene_mine(cfg, agent_tm, cost_tm, goal, obst, 2, 1e-6, out)
    pool = {k: torch.zeros((4,) + tuple(v.shape[1:])) for k, v in out.items() if k in ("agent", "goal", "obst")}
    state = torch.zeros(4, dtype=torch.int32)
    for kw, match in ((dict(fixed=4), "fixed"), (dict(fixed=-1), "fixed"), (dict(state=state[:3]), "state"),
                      (dict(pool={**pool, "goal": pool["goal"][:3]}), "pool.goal"), (dict(slot_of=torch.zeros(2, dtype=torch.int32)), "slot_of")):
        a = dict(pool=pool, fixed=0, state=state, slot_of=None)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_pool_push(cfg, out, a["pool"], a["fixed"], a["state"], a["slot_of"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OE.scene_pool_push(cfg, out, pool, 0, state)
    vm = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.scene_mine(vm, agent_tm, cost_tm, goal, None, 2, 1e-6, out)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.scene_pool_push(vm, out, pool, 0, state)

    class FakeEnv:
        KIND, device = "LidarSpread", "cpu"

        def __init__(self, cfg):
            self.cfg = cfg

    class FakeScenes:
        S, names = 3, ["a", "b", "c"]
    FakeScenes.cfg = cfg
    for cap in (0, -1, 2, 3):                                 # capacity <= pinned leaves the ring no slot
        with pytest.raises(ValueError, match="ScenePool: capacity"):
            SC.ScenePool(FakeEnv(cfg), cap, pinned=FakeScenes())
    with pytest.raises(ValueError, match="ScenePool: capacity"):
        SC.ScenePool(FakeEnv(cfg), 0)
    SC.check_pool(4, 3), SC.check_pool(1, 0)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        SC.ScenePool(FakeEnv(vm), 4)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        SC.Scenes.mine(FakeEnv(vm), None)
    for cls in (DGPPO, InforMARL, InforMARLLagr, HCBFCRPO):       # every algorithm class has the door, and it is shut for VMAS
        algo = cls.__new__(cls)
        algo._env = FakeEnv(vm)
        with pytest.raises(ValueError, match="VMASReverseTransport"):
            algo.mine_scenes(None)
        algo._env = FakeEnv(cfg)
        with pytest.raises(ValueError, match="mine_scenes\\(\\) needs a Rollout"):
            algo.mine_scenes(type("R", (), {"actions": torch.zeros(1)})())


def test_train_py_mining_flags(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mod = _load_train_py()
    ap = mod.build_parser()
    a = ap.parse_args(BASE)
    assert a.mine_scenes == 0 and a.mine_back == 8
    mod.check_scenes(a)
    cases = [(["--scene-frac", "0.5"], "--scene-frac needs --scenes"), (["--mine-scenes", "4"], "--mine-scenes needs --scene-frac"),
             (["--mine-back", "4"], "--mine-back needs --mine-scenes"), (["--mine-scenes", "-2", "--scene-frac", "0.5"], "--mine-scenes must be >= 1"),
             (["--mine-scenes", "4", "--mine-back", "-1", "--scene-frac", "0.5"], "--mine-back must be >= 0"),
             (["--mine-scenes", "4", "--scene-frac", "1.5"], "--scene-frac must be"),
             (["--mine-scenes", "4", "--scene-frac", "0.5", "--gpus", "2"], "--mine-scenes runs on one rank"),
             (["--mine-scenes", "4", "--scene-frac", "0.5", "--env", "VMASReverseTransport"], "--mine-scenes: VMASReverseTransport"),
             (["--mine-scenes", "4", "--scene-frac", "0.03", "--n-env-train", "16"], "--scene-frac 0.03 of --n-env-train 16"),
             (["--mine-scenes", "1", "--scene-frac", "0.5", "--scenes", HEADON], "--mine-scenes: ScenePool: capacity")]
    for extra, match in cases:
        with pytest.raises(SystemExit, match=match):
            mod.check_scenes(ap.parse_args(BASE + extra))
    mod.check_scenes(ap.parse_args(BASE + ["--mine-scenes", "4", "--scene-frac", "0.5"]))
    mod.check_scenes(ap.parse_args(BASE + ["--mine-scenes", "2", "--mine-back", "0", "--scene-frac", "0.5", "--scene-jitter", "0.05",
                                           "--scenes", HEADON]))
    monkeypatch.setenv("WORLD_SIZE", "2")                     # a launch under a launcher: refused like --gpus 2
    with pytest.raises(SystemExit, match="--mine-scenes runs on one rank"):
        mod.check_scenes(ap.parse_args(BASE + ["--mine-scenes", "4", "--scene-frac", "0.5"]))


def test_resume_compares_the_mining_flags():
    mod = _load_train_py()
    ap = mod.build_parser()
    assert {"mine_scenes", "mine_back"} <= set(mod._RESUME_LATER)
    a = ap.parse_args(BASE + ["--mine-scenes", "4", "--mine-back", "6", "--scene-frac", "0.5"])
    stored = mod._flags_to_store(a)
    assert stored["mine_scenes"] == 4 and stored["mine_back"] == 6
    mod.check_resume_flags(a, stored)
    with pytest.raises(SystemExit, match=r"--mine-scenes \(4 in the stopped run, 8 now\)"):
        mod.check_resume_flags(ap.parse_args(BASE + ["--mine-scenes", "8", "--mine-back", "6", "--scene-frac", "0.5"]), stored)
    with pytest.raises(SystemExit, match=r"--mine-back \(6 in the stopped run, 8 now\)"):
        mod.check_resume_flags(ap.parse_args(BASE + ["--mine-scenes", "4", "--scene-frac", "0.5"]), stored)
    old = {k: v for k, v in stored.items() if not k.startswith("mine")}          # a run stopped before the flags existed ran without
    mod.check_resume_flags(ap.parse_args(BASE + ["--scene-frac", "0.5"]), old)   # them, and resumes without them only
    with pytest.raises(SystemExit, match=r"--mine-scenes \(0 in the stopped run, 4 now\)"):
        mod.check_resume_flags(a, old)


def test_trainer_refusals():
    from dgppo.trainer.trainer import Trainer
    params = {"run_name": "x", "training_steps": 1, "eval_interval": 1, "eval_epi": 1, "save_interval": 1}

    class Algo:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="mine_scenes runs on one rank"):
        Trainer(None, None, Algo(), 0.99, 16, 4, "/nonexistent", 0, params, save_log=False, rank=0, world=2, scene_frac=0.5, mine_scenes=4)
    Algo.world = 1
    with pytest.raises(ValueError, match="need scenes"):
        Trainer(None, None, Algo(), 0.99, 16, 4, "/nonexistent", 0, params, save_log=False, scene_frac=0.5)
    with pytest.raises(ValueError, match="mine_back must be >= 0"):
        Trainer(None, None, Algo(), 0.99, 16, 4, "/nonexistent", 0, params, save_log=False, scene_frac=0.5, mine_scenes=4, mine_back=-1)


def test_test_py_mining_flags():
    mod = _load_test_py()
    assert mod.MINE_FLAGS == [(("--mine-scenes",), "str", None), (("--mine-back",), "int", None)] and mod.MINE_BACK_DEFAULT == 8
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.mine_scenes is None and args.mine_back is None
    args = ap.parse_args(["--path", "x", "--mine-scenes", "out.npz", "--mine-back", "4", "--shield", "--scenes", "a.npz", "--stochastic"])
    assert args.mine_scenes == "out.npz" and args.mine_back == 4
    assert "--mine-scenes" in mod.__doc__ and "--mine-back" in mod.__doc__
    with pytest.raises(SystemExit, match="--mine-back needs --mine-scenes"):
        mod.main(["--path", "/nonexistent/run", "--mine-back", "4"])
    with pytest.raises(SystemExit, match="--mine-back must be >= 0"):
        mod.main(["--path", "/nonexistent/run", "--mine-scenes", "o.npz", "--mine-back", "-1"])
    with pytest.raises(SystemExit, match="--mine-scenes: VMASReverseTransport"):
        mod.main(["--path", "/nonexistent/run", "--mine-scenes", "o.npz", "--env", "VMASReverseTransport"])


# ---- the precondition of the head-on GPU test ---------------------------------------------------------------------------------------------
def test_headon_agents_collide_under_constant_actions():
    """the oracle env step alone: from the committed head-on scene, with both agents accelerating at each other, the cost first
    reaches 1e-6 at a step t* with 4 <= t* < 32 (4: the GPU test mines with back = 4 and expects the failure at step 4 again)"""
    cost, t_star = MN.headon_oracle()
    assert cost.shape == (MN.HEADON_T, 2, 2) and np.isfinite(cost).all()
    print(f"[scene mine] head-on: t* = {t_star}, cost there {cost[t_star].tolist()}, the step before {cost[t_star - 1].tolist()}")
    assert 1 <= t_star < 32 and t_star >= 4
    assert (cost[:t_star] < MN.THRESH).all() and (cost[t_star] >= MN.THRESH).any()
    assert float(cost[t_star].max()) > 1e-3 and float(cost[t_star - 1].max()) < -1e-3, "far from the threshold on both sides"
