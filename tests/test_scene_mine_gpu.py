"""Scene mining on the device: dgppo_env_scene_mine and dgppo_env_scene_pool_push against their NumPy restatement
(tests/scene_mine_np.py) word for word, the round trip through dgppo_env_scene_load, the pool's empty slots under the scene mix, the
head-on record against the oracle's step, and the flags of train.py and test.py end to end.  Everything compared is integers or
copied words: no tolerance appears."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_mine_np as MN  # noqa: E402
import scenes_np as SN  # noqa: E402
from test_scene_mix_cpu import HEADON, _load_train_py  # noqa: E402
from test_scenes_cpu import _load_test_py  # noqa: E402
from test_scenes_gpu import _d, _words  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
SENT = 0xDEADBEEF
SENT_I32 = SENT - (1 << 32)
# (kind, n, n_obs, area): sd 5 (bicycle), discs (MPE), no obstacles, three cost columns and a cost row of 66 words (ConnectSpread 22),
# teams that fill more than half a wave; None: the kind's default area
CASES = [("LidarSpread", 1, 0, None), ("LidarSpread", 2, 1, None), ("LidarSpread", 3, 3, None), ("LidarSpread", 33, 2, 4.0),
         ("LidarSpread", 64, 2, 4.0), ("LidarBicycleTarget", 2, 1, None), ("MPESpread", 3, 2, None), ("MPEConnectSpread", 22, 3, 2.0)]
# (T, B, Bs, backs): Bs > B is a RolloutData.prefix view; four waves per block: B = 5 and 65 leave a tail
SHAPES = [(1, 1, 1, (0, 3)), (5, 3, 4, (0, 3, 200)), (64, 5, 5, (0, 3, 200)), (130, 65, 70, (3,))]


def _make_cfg(kind, n, n_obs, area):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs, **({} if area is None else {"area_size": area}))


def _record(cuda, cfg, T, B, Bs, back, rng):
    """a time-major record of Bs envs: the agent rows of step t are those of a real reset (its own seeds per step and env, so every
    row is a valid start; against the obstacles of step 0 it need not be), goals and obstacles the reset's of step 0; the costs are
    planted, by b % 8 (the cases of tests/scene_mine_np.hand_cases):
      0 never unsafe, with NaN and -inf on the way      1 unsafe at T - 1, a random word       2 unsafe at step 0: not taken
      3 flagged: overlap / out of area at t0            4 +inf, two agents at the same step    5 one ulp below thresh, then thresh
      6 the last word of the row, unsafe again later    7 never unsafe
    so the first five envs already hold a taken, an untaken, a never-unsafe and a flagged one"""
    from dgppo_amd import ops_env as OE
    n, sd, W = cfg.n_agents, cfg.state_dim, cfg.n_agents * cfg.n_cost
    st = OE.State.empty(cfg, (T + 1) * Bs, cuda)
    n_failed = torch.zeros(1, dtype=torch.int32, device=cuda)
    seeds = torch.arange(1, (T + 1) * Bs + 1, dtype=torch.int64, device=cuda) * 7919 + int(rng.integers(1, 1000))
    OE.env_reset(cfg, seeds, st.agent, st.goal, st.obst, n_failed)
    assert int(n_failed.item()) == 0
    agent_tm = st.agent.view(T + 1, Bs, n, sd).cpu().numpy().copy()
    goal = st.goal[:Bs].cpu().numpy().copy()
    obst = None if st.obst is None else st.obst[:Bs].cpu().numpy().copy()
    cost = rng.uniform(-1.0, -0.1, size=(T, Bs, W)).astype(f32)
    below = np.nextafter(MN.THRESH, f32(-1), dtype=f32)
    for b in range(Bs):
        k, w = b % 8, int(rng.integers(0, W))
        if k == 0:
            cost[rng.integers(0, T), b, w] = np.nan
            cost[rng.integers(0, T), b, (w + 1) % W] = -np.inf
        elif k == 1:
            cost[T - 1, b, w] = 0.25
        elif k == 2:
            cost[0, b, w] = 0.25
        elif k == 5:
            cost[min(1, T - 1), b, w] = below
            cost[min(2, T - 1), b, w] = MN.THRESH
        elif k == 4:
            t = min(3, T - 1)
            cost[t, b, [W - 1, W // 2]] = [np.inf, 0.5]
        elif k == 3:
            t = min(back + 1, T - 1)
            cost[t, b, w] = 0.25
            t0 = max(t - back, 0)
            if n >= 2:
                agent_tm[t0, b, n - 1, :2] = agent_tm[t0, b, 0, :2] + f32(0.01)
            else:
                agent_tm[t0, b, 0, 0] = -0.5
        elif k == 6:
            cost[T // 2, b, W - 1] = 1.0
            cost[T - 1, b, 0] = 2.0
    return agent_tm, cost.reshape(T, Bs, n, cfg.n_cost), goal, obst


def _mine(cuda, cfg, agent_tm, cost_tm, goal, obst, B, back, thresh):
    """OE.scene_mine on the first B envs of the record, outputs pre-filled with the sentinel -> dict of host arrays (rows as uint32)"""
    from dgppo_amd import ops_env as OE
    a, c = _d(agent_tm, cuda), _d(cost_tm, cuda)
    out = OE.alloc_mined(cfg, B, cuda)
    for v in out.values():
        v.view(torch.int32).fill_(SENT_I32)
    OE.scene_mine(cfg, a[:, :B], c[:, :B], _d(goal[:B], cuda), None if obst is None else _d(obst[:B], cuda), back, thresh, out)
    torch.cuda.synchronize()
    return out, {k: (v.cpu().numpy() if k in OE.MINED_FIELDS else _words(v)) for k, v in out.items()}


# ---- 1, 2. the kernel against the restatement, and the round trip through scene_load ----------------------------------------------------
@pytest.mark.parametrize("kind,n,n_obs,area", CASES, ids=["-".join(map(str, c[:3])) for c in CASES])
def test_mine_equals_the_restatement_and_loads_back(cuda, kind, n, n_obs, area):
    from dgppo_amd import ops_env as OE
    cfg = _make_cfg(kind, n, n_obs, area)
    rng = np.random.default_rng(n * 100 + n_obs)
    seen = {"taken": 0, "flagged": 0, "never": 0, "at_start": 0}
    for T, B, Bs, backs in SHAPES:
        for back in backs:
            name = f"{kind} {n}/{n_obs} T={T} B={B} Bs={Bs} back={back}"
            agent_tm, cost_tm, goal, obst = _record(cuda, cfg, T, B, Bs, back, rng)
            want = MN.mine_np(cfg, agent_tm[:, :B], cost_tm[:, :B], goal[:B], None if obst is None else obst[:B], back, MN.THRESH, SENT)
            dev, got = _mine(cuda, cfg, agent_tm, cost_tm, goal, obst, B, back, float(MN.THRESH))
            for k in OE.MINED_FIELDS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")
            never = want["first"] < 0
            for k in ("agent", "goal", "obst"):
                if want[k] is None:
                    assert k not in got
                    continue
                np.testing.assert_array_equal(got[k], want[k].view(np.uint32), err_msg=f"{name}: {k} rows")
                assert (got[k][never] == SENT).all(), f"{name}: {k} of a never-unsafe env was written"
            took = MN.taken(want["first"], want["flags"])
            counts = dict(taken=int(took.sum()), flagged=int((want["flags"] != 0).sum()), never=int(never.sum()),
                          at_start=int((want["first"] == 0).sum()))
            if B >= 5 and T >= 5:                              # every such batch has all four kinds of env
                assert all(v >= 1 for v in counts.values()), (name, counts)
            for k, v in counts.items():
                seen[k] += v
            # the round trip: scene_load of the mined rows gives the record's state back, the whole obstacle record included
            idx = np.flatnonzero(~never)
            if len(idx) == 0:
                continue
            ix = torch.from_numpy(idx).to(cuda)
            rows = {k: v[ix].contiguous() for k, v in dev.items() if k in ("agent", "goal", "obst")}
            st = OE.State.empty(cfg, len(idx), cuda)
            flags = torch.full((len(idx),), -7, dtype=torch.int32, device=cuda)
            OE.scene_load(cfg, rows, np.arange(len(idx)), None, 0.0, st, flags)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(flags.cpu().numpy(), got["flags"][idx], err_msg=f"{name}: flags against scene_load's")
            np.testing.assert_array_equal(_words(st.agent), agent_tm[want["t0"][idx], idx].view(np.uint32), err_msg=f"{name}: agent back")
            np.testing.assert_array_equal(_words(st.goal), goal[idx].view(np.uint32), err_msg=f"{name}: goal back")
            if obst is not None:
                np.testing.assert_array_equal(_words(st.obst), obst[idx].view(np.uint32), err_msg=f"{name}: obstacle record back")
    print(f"{kind} {n}/{n_obs}: {seen}")
    assert all(v >= 1 for v in seen.values()), f"the case became trivial: {seen}"


def test_mine_threshold_is_an_argument(cuda):
    """test.py's rule (thresh 0.0) and the trainer's (1e-6) on the hand-written cases: a cost of 5e-7 is unsafe for the one only"""
    cfg = _make_cfg("LidarSpread", 2, 1, None)
    cases = MN.hand_cases()
    cost_tm = np.stack([c for c, _, _ in cases.values()], axis=1)
    cost_tm[1, list(cases).index("never"), 0, 1] = 5e-7
    T, B = cost_tm.shape[:2]
    agent_tm, _, goal, obst = _record(cuda, cfg, T, B, B, 0, np.random.default_rng(0))
    for thresh in (0.0, float(MN.THRESH)):
        _, got = _mine(cuda, cfg, agent_tm, cost_tm, goal, obst, B, 2, thresh)
        first, who = MN.first_unsafe(cost_tm, thresh)
        np.testing.assert_array_equal(got["first"], first)
        np.testing.assert_array_equal(got["who"], who)
    assert dict(zip(cases, got["first"].tolist())) == {k: f for k, (_, f, _) in cases.items()}


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------------------
def _push_sequence(cuda, cfg, B, M, fixed, seed):
    """pushes of 0, < R, R, > R and 1 taken envs (as far as B allows) from head 0: after each, pool words, state and slot_of against
    the restatement.  -> the pool words after the last push"""
    from dgppo_amd import ops_env as OE
    rng = np.random.default_rng(seed)
    R = M - fixed
    shapes = OE.scene_template_shapes(cfg)
    pool = {k: torch.full((M,) + s, float("nan"), device=cuda) for k, s in shapes.items()}
    for k, v in pool.items():
        v[:fixed] = 3.0
    state = torch.zeros(4, dtype=torch.int32, device=cuda)
    want_pool = {k: (pool[k].cpu().numpy() if k in pool else None) for k in ("agent", "goal", "obst")}
    want_state = [0, 0, 0, 0]
    counts = [c for c in (0, R - 1, R, R + 2, 1, R + 1) if 0 <= c <= B]
    assert 0 in counts and (B < R or R in counts)
    for count in counts:
        pick = rng.choice(B, size=count, replace=False)
        other = rng.integers(0, 3, size=B)                      # the untaken: never unsafe, unsafe at the start, flagged
        first = np.where(other == 0, -1, np.where(other == 1, 0, 5)).astype(np.int32)
        flags = np.where(other == 2, 4, 0).astype(np.int32)
        first[pick], flags[pick] = rng.integers(1, 100, size=count), 0
        rows = {k: rng.standard_normal((B,) + s).astype(f32) for k, s in shapes.items()}
        mined = {k: _d(v, cuda) for k, v in rows.items()}
        mined.update(first=_d(first, cuda, np.int32), flags=_d(flags, cuda, np.int32))
        slot_of = torch.full((B,), -9, dtype=torch.int32, device=cuda)
        OE.scene_pool_push(cfg, mined, pool, fixed, state, slot_of)
        torch.cuda.synchronize()
        want_pool, want_state, want_slot = MN.push_np(first, flags, {**{"obst": None}, **rows}, want_pool, fixed, want_state)
        name = f"B={B} M={M} fixed={fixed} count={count}"
        assert state.cpu().tolist() == want_state, name
        np.testing.assert_array_equal(slot_of.cpu().numpy(), want_slot, err_msg=name)
        for k, v in pool.items():
            np.testing.assert_array_equal(_words(v), want_pool[k].view(np.uint32), err_msg=f"{name}: pool.{k}")
        assert want_state[3] == count and (_words(pool["agent"])[:fixed] == np.float32(3.0).view(np.uint32)).all()
    return {k: _words(v) for k, v in pool.items()}, want_state


@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_pool_push_equals_the_restatement_and_repeats(cuda, B):
    cfg = _make_cfg("LidarSpread", 2, 1, None)
    for M in (1, 4, 7):
        for fixed in (0, 2):
            if fixed >= M:
                continue
            a, sa = _push_sequence(cuda, cfg, B, M, fixed, seed=B * 100 + M * 10 + fixed)
            b, sb = _push_sequence(cuda, cfg, B, M, fixed, seed=B * 100 + M * 10 + fixed)
            assert sa == sb and all(np.array_equal(a[k], b[k]) for k in a), "two runs of the same sequence differ"
            empty = np.isnan(a["agent"].view(f32)).all(axis=(1, 2))   # the slots nothing was pushed to keep their NaN words
            assert int(empty.sum()) == (M - fixed) - sa[1] and not np.isnan(a["agent"].view(f32)[~empty]).any()


@pytest.mark.parametrize("kind,n,n_obs,area", [("LidarSpread", 1, 0, None), ("LidarSpread", 64, 2, 4.0), ("MPESpread", 3, 2, None)],
                         ids=["no-obstacles", "rows-of-256-words", "discs"])
def test_pool_push_row_shapes(cuda, kind, n, n_obs, area):
    _push_sequence(cuda, _make_cfg(kind, n, n_obs, area), 65, 4, 1, seed=n)


# ---- 5. the head-on record -------------------------------------------------------------------------------------------------------------------
def _headon_rollout(env, scenes, B, T, cuda):
    """the scenes (env b in scene b % S) stepped T times with HEADON_ACTION by the env kernels into a RolloutData"""
    from dgppo_amd import engine as EN, ops_env as OE
    ro = EN.RolloutData(env.cfg, B, T, cuda, False)
    OE.scene_start(env.cfg, scenes.dev, None, None, 0.0, ro.states_tm[0])
    ro.action_tm.copy_(torch.from_numpy(MN.HEADON_ACTION).to(cuda).expand(T, B, 2, 2))
    for t in range(T):
        OE.step(env.cfg, ro.states_tm[t], ro.action_tm[t], ro.states_tm[t + 1], ro.reward_tm[t], ro.cost_tm[t])
    torch.cuda.synchronize()
    return ro


@pytest.fixture(scope="module")
def headon(cuda):
    from dgppo.env import Scenes, make_env
    env = make_env("LidarSpread", 2, num_obs=1)
    sc = Scenes.load(HEADON, env)
    return env, sc, _headon_rollout(env, sc, 3, MN.HEADON_T, cuda)


def test_headon_record_is_mined_at_the_oracles_step(cuda, headon):
    from dgppo.env import Scenes
    env, sc, ro = headon
    _, t_star = MN.headon_oracle()
    assert t_star >= 4
    first, who = MN.first_unsafe(ro.cost_tm.cpu().numpy(), MN.THRESH)
    assert first.tolist() == [t_star] * 3 and who.tolist() == [0] * 3
    mined = Scenes.mine(env, ro, back=4)
    assert mined is not None and mined.S == 3
    assert mined.names == [f"env{b}_t{t_star - 4}_first{t_star}_a0" for b in range(3)]
    assert {k: v.tolist() for k, v in mined.mined.items()} == {"env": [0, 1, 2], "first": [t_star] * 3, "t0": [t_star - 4] * 3, "who": [0] * 3}
    np.testing.assert_array_equal(mined.rows["agent"].view(np.uint32), _words(ro.agent_tm[t_star - 4]))
    np.testing.assert_array_equal(mined.rows["goal"].view(np.uint32), _words(ro.goal))
    np.testing.assert_array_equal(mined.rows["obst"].view(np.uint32), _words(ro.obst[..., :5]))
    assert Scenes.mine(env, ro, back=4, max_scenes=2).S == 2 and Scenes.mine(env, ro, back=4, max_scenes=0) is None
    assert Scenes.mine(env, ro, back=4, names=["a", "b", "c"]).names == ["a", "b", "c"]
    assert Scenes.mine(env, ro, back=4, thresh=10.0) is None, "no cost reaches 10: nothing is taken"
    assert Scenes.mine(env, ro.prefix(2), back=4).S == 2, "a prefix view of the record"
    # the mined scenes are valid (Scenes() validated them) and, rolled again with the same actions, fail at step 4
    again = _headon_rollout(env, mined, 3, 8, cuda)
    assert MN.first_unsafe(again.cost_tm.cpu().numpy(), MN.THRESH)[0].tolist() == [4] * 3
    np.testing.assert_array_equal(_words(again.agent_tm[4]), _words(ro.agent_tm[t_star]))


# ---- 4. empty slots mean sampled reset -------------------------------------------------------------------------------------------------------
def test_empty_pool_slots_leave_the_sampled_reset(cuda, headon):
    from dgppo.env import ScenePool
    from dgppo_amd import ops_env as OE
    env, sc, ro = headon
    cfg, B = env.cfg, 6
    _, t_star = MN.headon_oracle()
    pool = ScenePool(env, 4)
    assert pool.S == 4 and pool.fill() == (0, 0, 0) and pool.to_scenes() is None and len(pool.names) == 4
    assert all(bool(torch.isnan(v).all()) for v in pool.dev.values())
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 104729
    plain = OE.State.empty(cfg, B, cuda)
    OE.reset(cfg, seeds, plain)
    of = np.array([0, 1, -1, 3, 0, 2], np.int32)

    def mixed():
        st, n_fb = OE.State.empty(cfg, B, cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
        m = pool.mix(of, 0.0)
        OE.mixed_start(cfg, seeds, st, m.scenes.dev, m.scene_of, m.jitter, None, n_fb)
        torch.cuda.synchronize()
        return st, int(n_fb.item())
    st, n_fb = mixed()
    assert n_fb == int((of >= 0).sum()), "every assigned env drew an empty slot and is counted"
    for k in ("agent", "goal", "obst", "hits"):
        np.testing.assert_array_equal(_words(getattr(st, k)), _words(getattr(plain, k)), err_msg=f"{k}: a fresh pool changed the reset")
    # one push: the three head-on envs are taken, slots 0..2 fill in env order, slot 3 stays empty
    pool.push_from(ro, back=4, thresh=1e-6)
    assert pool.fill() == (3, 3, 3) and pool.state.cpu().tolist() == [3, 3, 3, 3]
    np.testing.assert_array_equal(_words(pool.dev["agent"][:3]), _words(ro.agent_tm[t_star - 4]))
    assert bool(torch.isnan(pool.dev["agent"][3]).all())
    st, n_fb = mixed()
    assert n_fb == 1, "only the env that drew slot 3"
    for b, s in enumerate(of):
        src = plain.agent[b] if s < 0 or s == 3 else pool.dev["agent"][s]
        np.testing.assert_array_equal(_words(st.agent[b]), _words(src), err_msg=f"env {b} (slot {s})")
    held = pool.to_scenes()
    assert held.S == 3 and held.names == ["pool0", "pool1", "pool2"]
    # the state survives a round trip, pinned scenes sit in front of the ring and are never written
    pinned = ScenePool(env, 3, pinned=sc)
    assert pinned.P == 1 and pinned.names == ["headon", "pool1", "pool2"] and pinned.to_scenes().S == 1
    pinned.push_from(ro, back=4, thresh=1e-6)                  # three taken, a ring of two: the third is dropped
    assert pinned.fill() == (2, 2, 3)
    np.testing.assert_array_equal(_words(pinned.dev["agent"][0]), _words(sc.dev["agent"][0]))
    np.testing.assert_array_equal(_words(pinned.dev["agent"][1:]), _words(ro.agent_tm[t_star - 4, :2]))
    other = ScenePool(env, 3, pinned=sc)
    other.load_state_dict(pinned.state_dict())
    assert other.fill() == (2, 2, 3) and all(np.array_equal(_words(other.dev[k]), _words(pinned.dev[k])) for k in pinned.dev)
    with pytest.raises(ValueError, match="does not fit"):
        ScenePool(env, 4, pinned=sc).load_state_dict(pinned.state_dict())


# ---- 6. train.py --------------------------------------------------------------------------------------------------------------------------------
MINE = ["--mine-scenes", "4", "--mine-back", "4", "--scene-frac", "0.5", "--scenes", HEADON, "--scene-jitter", "0.05"]
POOL_KEYS = ("rollout/scene_pool_fill", "rollout/scene_pool_pushed", "rollout/scene_pool_taken")


def _train(mod, log_dir, extra):
    argv = ["--env", "LidarSpread", "-n", "2", "--algo", "dgppo", "--obs", "1", "--steps", "2", "--n-env-train", "16", "--batch-size",
            "2048", "--n-env-test", "4", "--eval-interval", "1", "--save-interval", "1", "--log-dir", str(log_dir)]
    saved = np.random.get_state()
    try:
        mod.main(argv + extra)
    finally:
        np.random.set_state(saved)


def _run_of(log_dir):
    root = os.path.join(str(log_dir), "LidarSpread", "dgppo")
    runs = os.listdir(root)
    assert len(runs) == 1, runs
    return os.path.join(root, runs[0])


def _metrics(run_dir):
    return [json.loads(ln) for ln in open(os.path.join(run_dir, "metrics.jsonl"))]


@pytest.fixture(scope="module")
def mined_run(cuda, tmp_path_factory):
    """train.py in-process: 16 envs of LidarSpread n = 2, half of them in the pool, whose first slot is the jittered head-on scene —
    an untrained policy flies its agents into each other there, so the ring fills from the first iteration on"""
    base = tmp_path_factory.mktemp("mined")
    _train(_load_train_py(), base / "a", MINE)
    return base, _run_of(base / "a")


def _npz_words(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].view(np.uint32) if z[k].dtype == f32 else z[k]) for k in z.files}


def test_train_py_mines_logs_saves_and_resumes(cuda, mined_run, tmp_path):
    """the run ends, logs the three pool keys, fills its ring, and writes scenes files that load.  A second, identical run and a run
    stopped after step 1 and resumed are held to it in everything DESIGN.md §7 calls a function of the state alone — the records
    before the first update resp. before the resume step, the pool keys and the fallback count of the iteration that starts from
    that state, the evaluation there, the scenes files written up to there — bit for bit; the steps and key sets of every record.
    What follows an update is not compared bit for bit: the updates' gradient reductions use float atomics, so no two runs of this
    project agree in them (tests/test_scene_mix_gpu.py makes the same cut), and the mined words inherit that."""
    from dgppo.env import Scenes, make_env
    base, run_a = mined_run
    rows_a = _metrics(run_a)
    updates = [r for r in rows_a if "policy/loss" in r]
    assert len(updates) == 3
    for r in updates:
        assert set(POOL_KEYS) <= set(r) and "rollout/scene_fallback" in r and all(np.isfinite(v) for v in r.values())
        assert 0 <= r["rollout/scene_pool_fill"] <= 3 and r["rollout/scene_pool_pushed"] >= r["rollout/scene_pool_fill"]
    print("[scene mine] pool keys per iteration:", [[r[k] for k in POOL_KEYS] + [r["rollout/scene_fallback"]] for r in updates])
    assert updates[-1]["rollout/scene_pool_fill"] >= 1, "the pool stayed empty: the test shows nothing"
    assert all("eval/scene_reward" in r for r in rows_a if "eval/reward" in r), "the pinned scene is evaluated from step 0 on"
    assert sorted(os.listdir(os.path.join(run_a, "scenes"))) == ["0.npz", "1.npz", "2.npz"]
    env = make_env("LidarSpread", 2, num_obs=1)
    for step in (0, 1, 2):
        sc = Scenes.load(os.path.join(run_a, "scenes", f"{step}.npz"), env)
        assert sc.names[0] == "headon" and sc.names[1:] == [f"pool{m}" for m in range(1, sc.S)]
    assert Scenes.load(os.path.join(run_a, "scenes", "0.npz"), env).S == 1
    assert Scenes.load(os.path.join(run_a, "scenes", "2.npz"), env).S == 1 + int(updates[1]["rollout/scene_pool_fill"])
    # an identical run
    mod = _load_train_py()
    _train(mod, base / "b", MINE)
    run_b = _run_of(base / "b")
    rows_b = _metrics(run_b)
    assert [(r["step"], sorted(r)) for r in rows_b] == [(r["step"], sorted(r)) for r in rows_a]
    first = lambda rows: [r for r in rows if r["step"] == 0]
    assert [r for r in first(rows_b) if "eval/reward" in r] == [r for r in first(rows_a) if "eval/reward" in r]
    pool_of = lambda r: [r[k] for k in POOL_KEYS + ("rollout/scene_fallback",)]
    assert pool_of([r for r in rows_b if "policy/loss" in r][0]) == pool_of(updates[0])
    for step in (0, 1):
        wa, wb = _npz_words(os.path.join(run_a, "scenes", f"{step}.npz")), _npz_words(os.path.join(run_b, "scenes", f"{step}.npz"))
        assert sorted(wa) == sorted(wb) and all(np.array_equal(wa[k], wb[k]) for k in wa), f"scenes/{step}.npz differs between two runs"
    print("[scene mine] two runs: all records equal bit for bit:", rows_a == rows_b, "; scenes/2.npz:",
          all(np.array_equal(v, _npz_words(os.path.join(run_b, "scenes", "2.npz")).get(k)) for k, v in
              _npz_words(os.path.join(run_a, "scenes", "2.npz")).items()))
    # stopped after step 1 and resumed
    run_c = str(tmp_path / "stopped")
    shutil.copytree(run_a, run_c)
    shutil.rmtree(os.path.join(run_c, "models", "2"))
    os.remove(os.path.join(run_c, "resume", "2.pkl"))
    os.remove(os.path.join(run_c, "scenes", "2.npz"))
    before = _npz_words(os.path.join(run_c, "scenes", "1.npz"))
    os.remove(os.path.join(run_c, "scenes", "1.npz"))
    _train(mod, base / "a", MINE + ["--resume", run_c])
    rows_c = _metrics(run_c)
    assert [(r["step"], sorted(r)) for r in rows_c] == [(r["step"], sorted(r)) for r in rows_a]
    assert [r for r in rows_c if r["step"] < 1] == [r for r in rows_a if r["step"] < 1]
    at = lambda rows, key: [r for r in rows if r["step"] == 1 and key in r]
    assert at(rows_c, "eval/scene_reward") == at(rows_a, "eval/scene_reward") and len(at(rows_a, "eval/scene_reward")) == 1
    assert pool_of(at(rows_c, "policy/loss")[0]) == pool_of(at(rows_a, "policy/loss")[0])
    after = _npz_words(os.path.join(run_c, "scenes", "1.npz"))
    assert sorted(after) == sorted(before) and all(np.array_equal(after[k], before[k]) for k in before), "the restored pool differs"
    assert os.path.exists(os.path.join(run_c, "scenes", "2.npz"))
    with pytest.raises(SystemExit, match=r"--mine-back \(4 in the stopped run, 8 now\)"):
        _train(mod, base / "a", MINE[:2] + MINE[4:] + ["--resume", run_c])


def test_train_py_without_the_flags_logs_no_pool_key(cuda, tmp_path):
    _train(_load_train_py(), tmp_path / "plain", ["--scenes", HEADON, "--scene-frac", "0.5", "--steps", "1"])
    run = _run_of(tmp_path / "plain")
    rows = _metrics(run)
    assert any("rollout/scene_fallback" in r for r in rows) and not any(k.startswith("rollout/scene_pool") for r in rows for k in r)
    assert not os.path.exists(os.path.join(run, "scenes"))


# ---- 7. test.py ---------------------------------------------------------------------------------------------------------------------------------
def test_test_py_mines_what_the_restatement_predicts(cuda, mined_run, tmp_path, capsys, monkeypatch):
    """test.py --mine-scenes on the trained checkpoint, episodes started in the head-on scene: the records the CLI mined are caught on
    the way, the restatement says which episodes are taken, and the file (or the line saying there is none) must agree"""
    from dgppo.env import Scenes, make_env
    _, run = mined_run
    mod = _load_test_py()
    caught = {}
    inner = mod.mine

    def spy(args, algo, env, ro):
        rec = algo.rollout_record(ro)
        caught.update(cfg=env.cfg, agent_tm=rec.agent_tm.cpu().numpy(), cost_tm=rec.cost_tm.cpu().numpy(), goal=rec.goal.cpu().numpy(),
                      obst=rec.obst.cpu().numpy())
        return inner(args, algo, env, ro)
    monkeypatch.setattr(mod, "mine", spy)
    out = str(tmp_path / "mined.npz")
    mod.main(["--path", run, "--no-video", "--max-step", "16", "--epi", "4", "--offset", "1", "--scenes", HEADON, "--scene-jitter", "0.05",
              "--mine-scenes", out, "--mine-back", "4"])
    printed = capsys.readouterr().out
    want = MN.mine_np(caught["cfg"], caught["agent_tm"], caught["cost_tm"], caught["goal"], caught["obst"], 4, 0.0, SENT)
    took = np.flatnonzero(MN.taken(want["first"], want["flags"]))
    print(f"[scene mine] test.py: first {want['first'].tolist()}, flags {want['flags'].tolist()}, taken {took.tolist()}")
    assert caught["cost_tm"].shape[:2] == (16, 3)
    if len(took) == 0:
        assert "mined scenes: none" in printed and not os.path.exists(out)
        return
    assert f"mined scenes: {len(took)} of 3 episodes -> {out}" in printed
    sc = Scenes.load(out, make_env("LidarSpread", 2, num_obs=1))
    assert sc.names == [f"epi{1 + b}_t{want['t0'][b]}_a{want['who'][b] // 2}" for b in took]
    np.testing.assert_array_equal(sc.rows["agent"].view(np.uint32), want["agent"][took].view(np.uint32))
    for b in took:
        assert f"epi: {b}, mined: first unsafe at step {want['first'][b]}, scene starts at step {want['t0'][b]}, agent {want['who'][b] // 2}" in printed
