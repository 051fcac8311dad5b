"""The scene mix on the device: dgppo_env_scene_mix against the reset it runs over and against dgppo_env_scene_load of the same
build word for word (both run the same expressions on the same device, so no tolerance), with flags and kept attempts held to
the NumPy restatement (tests/scene_mix_np.py); then through Engine.rollout, the algorithms' collect / update and train.py."""
import ctypes as C
import json
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_mix_np as M  # noqa: E402
import scenes_np as SN  # noqa: E402
from test_lookahead_shield_gpu import _record_words, _same_words  # noqa: E402
from test_scenes_cpu import retry_case, stuck_case  # noqa: E402
from test_scenes_gpu import _d, _templates, _words  # noqa: E402
from test_scene_mix_cpu import HEADON, _load_train_py  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
SENT = -7
TEMPLATE_SEED = {("LidarSpread", 1, 0): 1, ("LidarSpread", 2, 1): 3, ("LidarSpread", 3, 3): 2, ("LidarSpread", 33, 2): 1,
                 ("LidarSpread", 64, 2): 1, ("LidarBicycleTarget", 2, 1): 3, ("MPESpread", 3, 2): 1, ("LidarLine", 2, 1): 3,
                 ("MPEFormation", 3, 1): 1}          # picked on the CPU so that the conditions asserted below hold


def _rows(cuda, agent_t, goal_t, obst_t):
    rows = {"agent": _d(agent_t, cuda), "goal": _d(goal_t, cuda)}
    if obst_t is not None:
        rows["obst"] = _d(obst_t, cuda)
    return rows


def _fields(st):
    return {k: v for k, v in (("agent", st.agent), ("goal", st.goal), ("obst", st.obst)) if v is not None}


def _run(cuda, cfg, rows, scene_of, seeds, jitter, n_fb0=3):
    """reset -> copy -> scene_mix; scene_load of the same ids and seeds into a second record.
    -> (record words after the mix, copy words, flags, n_fallback, scene_load's record words, its flags)"""
    from dgppo_amd import ops_env as OE
    B = len(scene_of)
    sd = _d(seeds, cuda, np.int64)
    st = OE.State.empty(cfg, B, cuda)
    OE.env_reset(cfg, sd, st.agent, st.goal, st.obst)
    copy = {k: _words(v).copy() for k, v in _fields(st).items()}
    flags = torch.full((B,), SENT, dtype=torch.int32, device=cuda)
    n_fb = torch.full((1,), n_fb0, dtype=torch.int32, device=cuda)
    OE.scene_mix(cfg, rows, scene_of, sd, jitter, st, flags, n_fb)
    st2 = OE.State.empty(cfg, B, cuda)
    for v in _fields(st2).values():
        v.fill_(float("nan"))
    flags2 = torch.full((B,), SENT, dtype=torch.int32, device=cuda)
    OE.scene_load(cfg, rows, np.maximum(scene_of, 0), sd, jitter, st2, flags2)
    torch.cuda.synchronize()
    return ({k: _words(v) for k, v in _fields(st).items()}, copy, flags.cpu().numpy(), int(n_fb.item()),
            {k: _words(v) for k, v in _fields(st2).items()}, flags2.cpu().numpy())


def _check(name, cfg, scene_of, got, copy, flags, n_fb, load, load_flags, want, n_fb0=3):
    """the assertions of one run; want: scene_mix_np.mix_np of the same inputs on the copy"""
    assigned = scene_of >= 0
    np.testing.assert_array_equal(flags[~assigned], SENT, err_msg=f"{name}: a kept env's flag was written")
    np.testing.assert_array_equal(flags[assigned], load_flags[assigned], err_msg=f"{name}: flags against scene_load's")
    np.testing.assert_array_equal(flags[assigned], want["flags"][assigned], err_msg=f"{name}: flags against the restatement")
    taken = assigned & (flags == 0)
    for k in got:
        np.testing.assert_array_equal(got[k][~taken], copy[k][~taken], err_msg=f"{name}: {k} of a kept or fallback env was written")
        np.testing.assert_array_equal(got[k][taken], load[k][taken], err_msg=f"{name}: {k} against scene_load's record")
    # the kept attempt: the attempts' positions all differ, so equal agent words mean the same attempt (goals too: plain copies)
    np.testing.assert_array_equal(got["agent"][taken], want["agent"].view(np.uint32)[taken], err_msg=f"{name}: agent against the restatement")
    np.testing.assert_array_equal(got["goal"][taken], want["goal"].view(np.uint32)[taken], err_msg=f"{name}: goal against the restatement")
    assert n_fb == n_fb0 + int((flags[assigned] != 0).sum()) == n_fb0 + want["n_fallback"], f"{name}: n_fallback {n_fb}"
    return int((~assigned).sum()), int(taken.sum()), int((assigned & (flags != 0)).sum())


# ---- 1. the kernel against the reset and scene_load ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,n_obs", M.CASES, ids=["-".join(map(str, c)) for c in M.CASES])
def test_mix_equals_reset_and_scene_load(cuda, kind, n, n_obs):
    cfg = M.make_cfg(kind, n, n_obs)
    assert (cfg.state_dim, cfg.n_goals) == {"LidarBicycleTarget": (5, 2), "LidarLine": (4, 2), "MPEFormation": (4, 1)}.get(kind, (4, n))
    agent_t, goal_t, obst_t = M.templates(cfg, _templates, TEMPLATE_SEED[(kind, n, n_obs)])
    rows = _rows(cuda, agent_t, goal_t, obst_t)
    if n >= 33:                                                # scene 1: valid but for one pair of agents, in the upper half-wave
        i, j = M.high_pair(n)
        assert max(i, j) >= 32 and (n < 64 or min(i, j) >= 32) and M.overlap_only_between(cfg, agent_t[1], i, j)
        assert SN.scene_load_np(cfg, agent_t, goal_t, obst_t, None, None, 0.0, 3)["flags"].tolist()[:2] == [0, SN.AGENTS_OVERLAP]
    kept = valid = fallback = 0
    for B, scene_of in M.SCENE_OF.items():
        assert (scene_of < 0).any() and len(set(scene_of[scene_of >= 0].tolist())) < int((scene_of >= 0).sum())
        seeds = M.seeds_of(B, 7)
        for jitter in M.JITTERS:
            name = f"{kind} {n}/{n_obs} B={B} jitter={jitter}"
            got, copy, flags, n_fb, load, load_flags = _run(cuda, cfg, rows, scene_of, seeds, jitter)
            record = {k: copy[k].view(f32) if k in copy else None for k in ("agent", "goal", "obst")}
            want = M.mix_np(cfg, agent_t, goal_t, obst_t, scene_of, seeds, jitter, record)
            k_, v_, f_ = _check(name, cfg, scene_of, got, copy, flags, n_fb, load, load_flags, want)
            if n >= 33:                                        # the overlap of the two high agents is seen at every jitter
                np.testing.assert_array_equal(flags[scene_of == 1], SN.AGENTS_OVERLAP)
            kept, valid, fallback = kept + k_, valid + v_, fallback + f_
    print(f"{kind} {n}/{n_obs}: kept {kept}, scene envs taken {valid}, fallen back {fallback}")
    assert kept >= 1 and valid >= 1
    assert n_obs == 0 or fallback >= 1, "the case became trivial: no env falls back"


def test_retry_and_stuck_cases(cuda):
    """the two cases of tests/test_scenes_cpu.py, every env assigned: coincident agents are kept at the first attempt that
    separates them (some at attempt >= 1), an agent deep inside a square never is, and every env falls back"""
    cfg, agent, goal, rect, seeds, J = retry_case()
    of = np.zeros(len(seeds), np.int32)
    got, copy, flags, n_fb, load, load_flags = _run(cuda, cfg, _rows(cuda, agent, goal, rect), of, seeds, J)
    want = M.mix_np(cfg, agent, goal, rect, of, seeds, J, {"agent": copy["agent"].view(f32), "goal": copy["goal"].view(f32), "obst": None})
    assert want["attempt"].max() >= 1 and want["n_fallback"] == 0
    assert _check("coincident agents", cfg, of, got, copy, flags, n_fb, load, load_flags, want) == (0, len(seeds), 0)
    # at jitter 0 the same scene is invalid: scene_load writes it and leaves its counter alone, the mix keeps the reset and counts
    got, copy, flags, n_fb, load, load_flags = _run(cuda, cfg, _rows(cuda, agent, goal, rect), of, seeds, 0.0)
    assert flags.tolist() == [SN.AGENTS_OVERLAP] * len(seeds) and n_fb == 3 + len(seeds)
    assert all(np.array_equal(got[k], copy[k]) for k in got)
    cfg, agent, goal, rect, seeds, J = stuck_case()
    of = np.zeros(len(seeds), np.int32)
    got, copy, flags, n_fb, load, load_flags = _run(cuda, cfg, _rows(cuda, agent, goal, rect), of, seeds, J)
    want = M.mix_np(cfg, agent, goal, rect, of, seeds, J, {k: copy[k].view(f32) for k in copy})
    assert want["attempt"].tolist() == [SN.ATTEMPTS - 1] * len(seeds)
    assert _check("inside a rectangle", cfg, of, got, copy, flags, n_fb, load, load_flags, want) == (0, 0, len(seeds))
    assert flags.tolist() == [SN.AGENT_IN_OBSTACLE] * len(seeds)


# ---- 2. edge cases -------------------------------------------------------------------------------------------------------------------------
def test_nan_payload_falls_back_and_all_kept_is_a_no_op(cuda):
    cfg = M.make_cfg("LidarSpread", 2, 1)
    agent = np.tile(np.array([[[0.3, 0.3, 0.1, 0.0], [0.6, 1.2, 0.0, -0.1]]], f32), (4, 1, 1))
    goal = np.zeros((4, 2, 4), f32)
    goal[:, :, :2] = [[1.2, 1.2], [0.2, 0.9]]
    rect = np.tile(np.array([[[1.0, 0.5, 0.2, 0.4, 0.3]]], f32), (4, 1, 1))
    goal.view(np.uint32)[1, 1, 2] = 0x7FC12345                # a NaN with a payload in a goal row,
    agent[2, 0, 3] = np.inf                                   # an infinite velocity,
    rect[3, 0, 4] = np.nan                                    # a NaN heading: each alone makes its scene NONFINITE
    of = np.array([1, 0, 2, 3, -1, 1], np.int32)
    seeds = M.seeds_of(6, 3)
    for jitter in (0.0, 0.02):
        got, copy, flags, n_fb, load, load_flags = _run(cuda, cfg, _rows(cuda, agent, goal, rect), of, seeds, jitter)
        assert flags.tolist() == [SN.NONFINITE, 0, SN.NONFINITE, SN.NONFINITE, SENT, SN.NONFINITE] and n_fb == 3 + 4
        assert int(load["goal"][0, 1, 2]) == 0x7FC12345, "scene_load copies the payload; the mix must not"
        for k in got:
            np.testing.assert_array_equal(got[k][[0, 2, 3, 4, 5]], copy[k][[0, 2, 3, 4, 5]], err_msg=f"{k}: written for a non-finite scene")
            np.testing.assert_array_equal(got[k][1], load[k][1])
    # every env kept: the record is the reset's bit for bit, flags and counter are the caller's
    none = np.array([-1, -2, -1, -1, -100, -1], np.int32)
    got, copy, flags, n_fb, _, _ = _run(cuda, cfg, _rows(cuda, agent, goal, rect), none, seeds, 0.02)
    assert all(np.array_equal(got[k], copy[k]) for k in got) and flags.tolist() == [SENT] * 6 and n_fb == 3


def test_host_refusals_launch_nothing(cuda):
    """every refusal of the entry point returns non-zero, names it, and leaves the outputs as they were"""
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = M.make_cfg("LidarSpread", 2, 1)
    agent_t, goal_t, obst_t = _templates(cfg, 1, 5)
    B = 4
    t = dict(agent_t=_d(agent_t, cuda), goal_t=_d(goal_t, cuda), obst_t=_d(obst_t, cuda),
             scene_of=torch.zeros(B, dtype=torch.int32, device=cuda), seeds=torch.arange(1, B + 1, dtype=torch.int64, device=cuda),
             agent=torch.full((B, 2, 4), float("nan"), device=cuda), goal=torch.full((B, 2, 4), float("nan"), device=cuda),
             obst=torch.full((B, 1, 16), float("nan"), device=cuda), flags=torch.full((B,), SENT, dtype=torch.int32, device=cuda),
             n_fallback=torch.full((1,), SENT, dtype=torch.int32, device=cuda))
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}

    def call(cfg=cfg, S=1, jitter=0.0, B=B, **over):
        q = {**p, **over}
        return lib.dgppo_env_scene_mix(C.byref(cfg), q["agent_t"], q["goal_t"], q["obst_t"], S, q["scene_of"], q["seeds"], jitter,
                                       q["agent"], q["goal"], q["obst"], q["flags"], q["n_fallback"], B, N.stream_ptr())
    bad_cfg = M.make_cfg("LidarSpread", 2, 1)
    bad_cfg.kind = 17
    for kw in (dict(cfg=bad_cfg), dict(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 2, 0)), dict(S=0), dict(S=-3), dict(B=-1),
               dict(jitter=-0.1), dict(jitter=float("nan")), dict(agent_t=None), dict(goal_t=None), dict(agent=None), dict(goal=None),
               dict(scene_of=None), dict(seeds=None), dict(obst_t=None), dict(obst=None), dict(cfg=M.make_cfg("LidarSpread", 2, 0)),
               dict(cfg=M.make_cfg("LidarSpread", 2, 0), obst_t=None), dict(cfg=M.make_cfg("LidarSpread", 65, 1))):
        assert call(**kw) != 0, kw
        assert b"dgppo_env_scene_mix" in lib.dgppo_last_error(), (kw, lib.dgppo_last_error())
    torch.cuda.synchronize()
    for k in ("agent", "goal", "obst"):
        assert bool(torch.isnan(t[k]).all()), f"{k} was written by a refused call"
    assert t["flags"].tolist() == [SENT] * B and t["n_fallback"].tolist() == [SENT]
    assert call() == 0                                      # and the call they were all one step away from
    torch.cuda.synchronize()
    assert SENT not in t["flags"].tolist()


# ---- 3. through the engine ---------------------------------------------------------------------------------------------------------------
def _n3_scenes(cuda):
    """two valid scenes of LidarSpread n = 3 with one rectangle: a line-up left of it, a triangle round it"""
    from dgppo.env import Scenes, make_env
    env = make_env("LidarSpread", 3, num_obs=1)
    agent = np.zeros((2, 3, 4), f32)
    agent[0, :, :2] = [[0.2, 0.3], [0.2, 0.75], [0.2, 1.2]]
    agent[1, :, :2] = [[0.3, 0.3], [1.2, 0.3], [0.75, 1.3]]
    goal = np.zeros((2, 3, 4), f32)
    goal[0, :, :2] = [[1.3, 1.2], [1.3, 0.75], [1.3, 0.3]]
    goal[1, :, :2] = [[1.2, 1.2], [0.3, 1.2], [0.75, 0.2]]
    rect = np.array([[[0.75, 0.75, 0.3, 0.2, 0.4]], [[0.75, 0.75, 0.2, 0.2, 0.0]]], f32)
    return Scenes(env, agent, goal, rect=rect, names=["lineup", "triangle"])


def _clone(ro):
    """every word of a rollout's record, with the env axis of each field: time-major fields have it second"""
    out = {k: (v.clone(), 1) for k, v in _record_words(ro.finalize()).items()}
    out.update({f"env.{k}": (v.clone(), 0) for k, v in ro.env.items()})
    return out


def _envs(field, mask):
    v, axis = field
    return v[mask] if axis == 0 else v[:, mask]


def test_engine_rollout_mixes_reset_and_scene_trajectories(cuda, monkeypatch):
    """LidarSpread 3 / 1, B = 8, T = 4, deterministic: the kept envs' trajectories are those of the plain rollout, the scene envs'
    those of the rollout that starts every env in a scene (every word of the time-major record); the HIP-graph engine gives what
    the eager one gives, on the capturing call and on the replay with another assignment"""
    from dgppo_amd import engine as EN
    from test_engine_gpu import _setup
    B, T_, J = 8, 4, 0.01
    monkeypatch.setenv("DGPPO_HIPGRAPH", "0")
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 1, B, T_, cuda, 16, 4, use_graphs=True)
    monkeypatch.delenv("DGPPO_HIPGRAPH")
    eng_g = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=True)
    assert not eng.use_graphs and eng_g.use_graphs
    for k, net in eng_g.nets.items():
        net.load_tree(trees[k])
    sc = _n3_scenes(cuda)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    plain = _clone(eng.rollout(seeds, False))
    for call, of in enumerate((np.array([0, -1, 1, -1, 0, -1, 1, -1], np.int32), np.array([-1, 1, -1, 0, -1, 1, -1, 1], np.int32))):
        ids = np.maximum(of, 0)
        scene = _clone(eng.rollout(seeds, False, start=sc.start(ids, J)))
        mixed = _clone(eng.rollout(seeds, False, start=sc.mix(of, J)))
        kept = torch.from_numpy(of < 0).to(cuda)
        for name, field in mixed.items():
            _same_words(_envs(field, kept), _envs(plain[name], kept), f"call {call}: kept envs, {name}")
            _same_words(_envs(field, ~kept), _envs(scene[name], ~kept), f"call {call}: scene envs, {name}")
        graphed = _clone(eng_g.rollout(seeds, False, start=sc.mix(of, J)))
        for name, (v, _) in mixed.items():
            _same_words(graphed[name][0], v, f"call {call}: HIP-graph engine, {name}")
        assert {"step.agent", "step.hits", "env.goal", "env.obst", "action", "rnn", "reward", "cost"} <= set(mixed)
        assert not torch.equal(mixed["step.agent"][0][0, 0], mixed["step.agent"][0][0, 1]), "a scene env next to a kept one"
    torch.cuda.synchronize()
    assert eng_g._ro_cache[(B, False)]["graph"] is not None and eng_g._ro_cache[(B, False)]["calls"] == 2
    for e in (eng, eng_g):
        assert int(e.reset_failed.item()) == 0 and int(e.scene_fallback.item()) == 0 and e._mix_used


def test_stuck_scene_lands_in_scene_fallback(cuda):
    """the stuck case as bare rows (Scenes() would refuse it): under a mix every assigned env keeps its reset and is counted in
    scene_fallback, none in reset_failed — the record is the plain rollout's"""
    from dgppo.env import SceneMix
    from test_engine_gpu import _setup
    cfg, agent, goal, rect, seeds, J = stuck_case()
    _, _, _, eng, _ = _setup("LidarSpread", 2, 1, 4, 2, cuda, 16, 2)
    rows = types.SimpleNamespace(dev=_rows(cuda, agent, goal, rect))
    sd = torch.from_numpy(seeds[:4]).to(cuda)
    plain = _clone(eng.rollout(sd, False))
    for jitter, of in ((J, [0, -1, 0, 0]), (0.0, [0, 0, -1, -1])):
        eng.scene_fallback.zero_()
        mixed = _clone(eng.rollout(sd, False, start=SceneMix(rows, np.array(of, np.int32), jitter)))
        assert int(eng.scene_fallback.item()) == sum(x >= 0 for x in of) and int(eng.reset_failed.item()) == 0
        for name, (v, _) in mixed.items():
            _same_words(v, plain[name][0], f"jitter {jitter}: {name}")
    with pytest.raises(ValueError, match="scene_of outside"):
        eng.rollout(sd, False, start=SceneMix(rows, np.array([0, 1, 0, 0], np.int32), 0.0))


# ---- 4. the algorithms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo_name", ["dgppo", "informarl"])
def test_collect_with_a_mix_then_update(cuda, algo_name):
    from dgppo.algo import make_algo
    from dgppo.env import SceneMix, Scenes, make_env
    env = make_env("LidarSpread", 2, num_obs=1, max_step=16)
    algo = make_algo(algo=algo_name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=env.num_agents, batch_size=128, rnn_step=8, train_steps=10, seed=3)
    sc = Scenes.load(HEADON, env)
    keys = np.arange(1, 17) + 50
    info0 = algo.update(algo.collect(None, keys), 0)
    assert "rollout/scene_fallback" not in info0
    of = np.array([0, -1, 0, -1, -1, 0, -1, 0] * 2, np.int32)
    info1 = algo.update(algo.collect(None, keys + 10, scenes=sc, jitter=0.05, scene_of=of), 1)
    assert sorted(info1) == sorted(list(info0) + ["rollout/scene_fallback"]), "a mix adds one key and changes no other"
    assert all(np.isfinite(v) for v in info1.values()), info1
    n_ro = 2 if algo_name == "dgppo" else 1                  # dgppo: the deterministic companion rollout gets the same mix
    assert 0 <= info1["rollout/scene_fallback"] <= n_ro * int((of >= 0).sum())
    info2 = algo.update(algo.collect(None, keys + 20), 2)
    assert sorted(info2) == sorted(info0), "without a mix the keys are today's"
    # a scene that stays invalid costs no run its life: every assigned env of every rollout is counted, info() does not raise
    cfg, agent, goal, rect, _, J = stuck_case()
    stuck = types.SimpleNamespace(dev=_rows(cuda, agent, goal, rect), cfg=cfg, S=1)
    stuck.mix = lambda scene_of, jitter: SceneMix(stuck, np.asarray(scene_of), float(jitter))
    info3 = algo.update(algo.collect(None, keys + 30, scenes=stuck, jitter=J, scene_of=of), 3)
    assert info3["rollout/scene_fallback"] == n_ro * int((of >= 0).sum()) and all(np.isfinite(v) for v in info3.values())
    assert int(algo.engine.reset_failed.item()) == 0 and int(algo.engine.scene_fallback.item()) == 0
    for kw, match in ((dict(scene_of=of), "need scenes"), (dict(scenes=sc, scene_of=of, scene_ids=[0] * 16), "exclude each other"),
                      (dict(scenes=sc, scene_of=of[:4]), "one entry per key")):
        with pytest.raises(ValueError, match=match):
            algo.collect(None, keys, **kw)


# ---- 5. train.py end to end ----------------------------------------------------------------------------------------------------------------
def _train(mod, tmp_path, extra):
    argv = ["--env", "LidarSpread", "-n", "2", "--algo", "dgppo", "--obs", "1", "--scenes", HEADON, "--scene-frac", "0.5",
            "--scene-jitter", "0.05", "--steps", "2", "--n-env-train", "16", "--batch-size", "2048", "--n-env-test", "4",
            "--eval-interval", "1", "--save-interval", "1", "--log-dir", str(tmp_path / "logs")]
    saved = np.random.get_state()
    try:
        mod.main(argv + extra)
    finally:
        np.random.set_state(saved)


def _metrics(run_dir):
    return [json.loads(ln) for ln in open(os.path.join(run_dir, "metrics.jsonl"))]


def test_train_py_with_scenes_and_resume(cuda, tmp_path):
    """train.py in-process with half of 16 envs in the jittered head-on scene: the run ends, logs the scene evaluation and the
    fallback count, and records the flags.  Stopped after step 1 and resumed, it writes the records of the uninterrupted run: the
    same steps and keys, and bit for bit everything DESIGN.md §7 calls a function of the restored state — the records before the
    resume step, the evaluation (scenes included) at it, and the fallback count of its iteration, which only the flags, the step and
    the restored key stream decide.  The losses of updates are not compared: their gradient reductions use float atomics, so no two
    runs agree in them bit for bit, resumed or not"""
    import yaml
    mod = _load_train_py()
    _train(mod, tmp_path, [])
    root = tmp_path / "logs" / "LidarSpread" / "dgppo"
    runs = os.listdir(root)
    assert len(runs) == 1
    run_a, run_b = root / runs[0], tmp_path / "stopped"
    rows_a = _metrics(run_a)
    evals = [r for r in rows_a if "eval/reward" in r]
    updates = [r for r in rows_a if "policy/loss" in r]
    assert len(evals) == 3 and len(updates) == 3
    for r in evals:
        assert {"eval/scene_reward", "eval/scene_cost", "eval/scene_unsafe_frac"} <= set(r) and all(np.isfinite(v) for v in r.values())
    for r in updates:
        assert 0 <= r["rollout/scene_fallback"] <= 16 and all(np.isfinite(v) for v in r.values())
    conf = yaml.safe_load(open(run_a / "config.yaml"))
    assert conf["scenes"] == HEADON and conf["scene_frac"] == 0.5 and conf["scene_jitter"] == 0.05
    flags = yaml.safe_load(open(run_a / "resume" / "flags.yaml"))
    assert flags["scenes"] == HEADON and flags["scene_frac"] == 0.5 and flags["scene_jitter"] == 0.05
    # the stopped run: A's directory with step 1 as the newest state
    assert sorted(os.listdir(run_a / "resume")) == ["1.pkl", "2.pkl", "flags.yaml"]
    shutil.copytree(run_a, run_b)
    shutil.rmtree(run_b / "models" / "2")
    os.remove(run_b / "resume" / "2.pkl")
    _train(mod, tmp_path, ["--resume", str(run_b)])
    assert os.listdir(root) == runs
    rows_b = _metrics(run_b)
    assert [(r["step"], sorted(r)) for r in rows_b] == [(r["step"], sorted(r)) for r in rows_a]
    assert [r for r in rows_b if r["step"] < 1] == [r for r in rows_a if r["step"] < 1]
    at = lambda rows, key: [r for r in rows if r["step"] == 1 and key in r]
    assert len(at(rows_a, "eval/scene_reward")) == 1 and at(rows_b, "eval/scene_reward") == at(rows_a, "eval/scene_reward")
    assert at(rows_b, "policy/loss")[0]["rollout/scene_fallback"] == at(rows_a, "policy/loss")[0]["rollout/scene_fallback"]
    print("[scene mix] final records equal bit for bit:", rows_b[-2:] == rows_a[-2:])
    with pytest.raises(SystemExit, match=r"--scene-frac \(0.5 in the stopped run, 0.25 now\)"):
        _train(mod, tmp_path, ["--resume", str(run_b), "--scene-frac", "0.25"])


def test_two_ranks_count_the_fallbacks_of_the_one_rank_run(cuda, tmp_path):
    """`--gpus 2` (two gloo ranks on this GPU, started by train.py itself) against the same command on one rank.  The scene puts
    both agents 1e-3 from a corner of the area, so with a jitter of 0.05 an attempt is valid with probability ~0.07 and about a
    third of the scene envs fall back.  Which ones do is a function of the global keys, the global assignment and the step alone,
    so the count summed over the two ranks is the one-rank run's in every iteration; so are the evaluations of step 0"""
    import subprocess
    from dgppo_amd.env import scenes as SC
    agent = np.zeros((1, 2, 4), f32)
    agent[0, :, :2] = [[0.001, 0.001], [1.499, 1.499]]
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[1.2, 0.3], [0.3, 1.2]]
    path = str(tmp_path / "corners.npz")
    SC.write_npz(path, "LidarSpread", 2, agent, goal, np.array([[[0.75, 0.75, 0.2, 0.2, 0.0]]], f32), "rect", ["corners"])
    extra = ["--scenes", path, "--steps", "1"]
    mod = _load_train_py()
    _train(mod, tmp_path, extra + ["--log-dir", str(tmp_path / "one")])
    argv = ["--env", "LidarSpread", "-n", "2", "--algo", "dgppo", "--obs", "1", "--scene-frac", "0.5", "--scene-jitter", "0.05",
            "--n-env-train", "16", "--batch-size", "2048", "--n-env-test", "4", "--eval-interval", "1", "--save-interval", "1",
            "--gpus", "2", "--log-dir", str(tmp_path / "two")] + extra
    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(root, "train.py")] + argv, capture_output=True, text=True, timeout=600, cwd=root,
                         env=dict(os.environ, DGPPO_DIST_BACKEND="gloo"))
    assert out.returncode == 0, out.stderr[-3000:]
    rows = {}
    for name in ("one", "two"):
        runs = os.listdir(tmp_path / name / "LidarSpread" / "dgppo")
        assert len(runs) == 1, runs
        rows[name] = _metrics(tmp_path / name / "LidarSpread" / "dgppo" / runs[0])
    count = lambda rs: [r["rollout/scene_fallback"] for r in rs if "policy/loss" in r]
    print("[scene mix] fallbacks per iteration, one rank / two ranks:", count(rows["one"]), count(rows["two"]))
    assert len(count(rows["one"])) == 2 and count(rows["two"]) == count(rows["one"])
    assert all(1 <= c <= 15 for c in count(rows["one"])), "of 8 scene envs in each of the two rollouts some fall back, not all"
    ev = lambda rs: [r for r in rs if "eval/scene_reward" in r][0]
    assert ev(rows["two"]) == ev(rows["one"])
