"""The pool by priority on the device: dgppo_env_scene_pool_score, dgppo_env_scene_pool_draw and dgppo_env_scene_pool_push_evict
against their restatement (tests/scene_priority_np.py) word for word, ScenePool(priority=True) on the head-on record, the drawn mix of
the engine against SceneMix with the same assignment on the host, and train.py --scene-priority end to end.  Everything compared is
integers, copied words, or fp32 values formed by the same single operations: no tolerance appears."""
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
import scene_priority_np as PN  # noqa: E402
from test_scene_mix_cpu import HEADON, _load_train_py  # noqa: E402
from test_scenes_gpu import _d, _words  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
SENT_I32 = 0xDEADBEEF - (1 << 32)
# (kind, n, n_obs, area): rectangles, no obstacle at all (obst NULL) with discs' kind, rows of 256 words
CFGS = [("LidarSpread", 2, 1, None), ("MPESpread", 3, 0, None), ("LidarSpread", 64, 2, 4.0)]
MS = [1, 2, 5, 64, 65, 257, 1025]                            # one block is 256 slots: 257 and 1025 carry over chunks
BS = [1, 5, 65, 300]


def _make_cfg(kind, n, n_obs, area):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs, **({} if area is None else {"area_size": area}))


def _fixeds(M):
    return sorted({0, min(1, M - 1), M - 1})


def _filleds(R):
    return sorted({0, R // 2, R})


def _stats(cuda, M, rng, step, filled, head=None):
    """device statistics (ops_env.alloc_pool_stats) with random content: scores on and off [0, 1] and NaN, visits round min_visits,
    last on both sides of step -> (stats, host copies)"""
    from dgppo_amd import ops_env as OE
    score = rng.choice(np.array([0.0, 0.02, 0.1, 0.25, 0.5, 0.65, 0.9, 0.98, 1.0, 1.25, -0.5, np.nan], f32), size=M)
    score = np.where(rng.random(M) < 0.5, rng.random(M).astype(f32), score).astype(f32)
    visits = rng.integers(0, 5, size=M).astype(np.int32)
    last = (step + rng.integers(-40, 4, size=M)).astype(np.int32)
    state = np.array([0 if head is None else head, filled, 11, 0, -3, -3, -3, -3], np.int32)
    st = OE.alloc_pool_stats(M, cuda)
    st["score"].copy_(_d(score, cuda)), st["visits"].copy_(_d(visits, cuda, np.int32)), st["last"].copy_(_d(last, cuda, np.int32))
    st["state"].copy_(_d(state, cuda, np.int32))
    st["cum"].fill_(-1), st["order"].fill_(SENT_I32)
    return st, dict(score=score, visits=visits, last=last, state=state.tolist())


# ---- 1. the draw -----------------------------------------------------------------------------------------------------------------------
def _draw(cuda, cfg, st, host, fixed, age_cap, step, seed, n_total, n_scene, lo, B, name):
    from dgppo_amd import ops_env as OE
    of = torch.full((B,), SENT_I32, dtype=torch.int32, device=cuda)
    OE.scene_pool_draw(cfg, st, fixed, age_cap, step, seed, n_total, n_scene, lo, of)
    torch.cuda.synchronize()
    want = PN.draw_np(host["score"], host["last"], host["state"], fixed, age_cap, step, seed, n_total, n_scene, lo, B)
    got = of.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=name)
    for k in ("score", "last"):
        np.testing.assert_array_equal(_words(st[k]), host[k].view(np.uint32), err_msg=f"{name}: the draw wrote {k}")
    assert st["state"].cpu().tolist() == host["state"], f"{name}: the draw wrote the state"
    return got


@pytest.mark.parametrize("M", MS)
def test_draw_equals_the_restatement(cuda, M):
    rng = np.random.default_rng(M)
    seen = {"drawn": 0, "none_live": 0, "stale": 0}
    for ci, fixed in enumerate(_fixeds(M)):
        cfg = _make_cfg(*CFGS[ci % len(CFGS)])
        for filled in _filleds(M - fixed):
            step = int(rng.integers(0, 1000))
            st, host = _stats(cuda, M, rng, step, filled)
            for B in BS:
                for n_scene in sorted({0, 1, B}):
                    for age_cap in ((16, 1) if B == 65 else (16,)):
                        seed = int(rng.integers(0, 2 ** 63)) * 2 + 1
                        name = f"M={M} fixed={fixed} filled={filled} B={B} n_scene={n_scene} age_cap={age_cap} step={step}"
                        got = _draw(cuda, cfg, st, host, fixed, age_cap, step, seed, B, n_scene, 0, B, name)
                        assert int((got >= 0).sum()) == (n_scene if fixed + filled > 0 else 0), name
                        assert (got < fixed + filled).all(), f"{name}: an empty slot was drawn"
                        seen["drawn"] += int((got >= 0).sum())
                        seen["none_live"] += int(fixed + filled == 0 and n_scene > 0)
            seen["stale"] += int((host["last"][:fixed + filled] > step).any())
            # once per pool: a window in the middle of a larger batch, and again word for word
            a = _draw(cuda, cfg, st, host, fixed, 16, step, 77, 1000, 333, 123, 300, f"M={M} fixed={fixed} filled={filled} window")
            b = _draw(cuda, cfg, st, host, fixed, 16, step, 77, 1000, 333, 123, 300, f"M={M} fixed={fixed} filled={filled} window again")
            np.testing.assert_array_equal(a, b)
    print(f"M={M}: {seen}")
    assert seen["drawn"] > 0 and seen["none_live"] > 0 and (M < 5 or seen["stale"] > 0), f"the case became trivial: {seen}"


def test_draw_from_the_largest_pool(cuda):
    """M = 65536, every score 0.5, age_cap 1024 and a step far past every `last`: every weight is 2^26 and the total 2^42"""
    from dgppo_amd import ops_env as OE
    M, step = 65536, 1_000_000
    cfg = _make_cfg(*CFGS[0])
    st = OE.alloc_pool_stats(M, cuda)
    st["state"][1] = M
    host = dict(score=np.full(M, 0.5, f32), last=np.zeros(M, np.int32), state=[0, M, 0, 0, 0, 0, 0, 0])
    assert sum(PN.weights(host["score"], host["last"], 0, M, step, 1024)) == 1 << 42
    got = _draw(cuda, cfg, st, host, 0, 1024, step, (5 << 32) | 9, 300, 300, 0, 300, "M=65536")
    assert got.min() >= 0 and got.max() > 60000 and len(set(got.tolist())) > 290
    assert st["cum"][-1].item() == 1 << 42 and st["cum"][0].item() == 1 << 26


# ---- 2. the score ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
def test_score_equals_the_restatement(cuda, M):
    from dgppo_amd import ops_env as OE
    cfg = _make_cfg(*CFGS[M % len(CFGS)])
    rng = np.random.default_rng(1000 + M)
    st, host = _stats(cuda, M, rng, 50, M)
    seen = {"replays": 0, "fails": 0, "fell_back": 0, "untouched": 0}
    for call, B in enumerate(BS + [0]):
        step = 60 + call
        scene_of = rng.integers(-1, min(M, 1 + B // 3), size=B).astype(np.int32)       # several envs per slot, slots nobody replayed
        first = rng.choice(np.array([-1, 0, 7], np.int32), size=B)
        flags = np.where(rng.random(B) < 0.25, rng.choice(np.array([1, 2, 4, 8], np.int32), size=B), 0).astype(np.int32)
        flags[scene_of < 0] = SENT_I32                         # not read there: whatever it holds changes nothing
        OE.scene_pool_score(cfg, _d(scene_of, cuda, np.int32), _d(flags, cuda, np.int32), _d(first, cuda, np.int32), st, 0.3, step)
        torch.cuda.synchronize()
        score, visits, last, state = PN.score_np(scene_of, flags, first, host["score"], host["visits"], host["last"], 0.3, step, host["state"])
        name = f"M={M} B={B}"
        np.testing.assert_array_equal(_words(st["score"]), score.view(np.uint32), err_msg=f"{name}: score")
        np.testing.assert_array_equal(st["visits"].cpu().numpy(), visits, err_msg=f"{name}: visits")
        np.testing.assert_array_equal(st["last"].cpu().numpy(), last, err_msg=f"{name}: last")
        assert st["state"].cpu().tolist() == state, name
        assert not bool(st["tally"].any()), f"{name}: the tally is not zero afterwards"
        seen["replays"] += state[6]
        seen["fails"] += state[7]
        seen["fell_back"] += int(((scene_of >= 0) & (flags != 0)).sum())
        seen["untouched"] += int((last == host["last"]).sum())
        host.update(score=score, visits=visits, last=last, state=state)
    print(f"M={M}: {seen}")
    assert seen["replays"] > seen["fails"] > 0 and seen["fell_back"] > 0 and (M == 1 or seen["untouched"] > 0), seen
    assert host["state"][6:] == [0, 0], "B == 0 counts no replay"


# ---- 3. the evicting push ----------------------------------------------------------------------------------------------------------------
def _push_once(cuda, cfg, M, fixed, filled, B, count, seed):
    """one push of `count` taken envs among B into a pool with `filled` ring slots -> every word of the result, for the repeat"""
    from dgppo_amd import ops_env as OE
    rng = np.random.default_rng(seed)
    R = M - fixed
    shapes = OE.scene_template_shapes(cfg)
    step = 200
    st, host = _stats(cuda, M, rng, step, filled, head=int(rng.integers(0, R)))
    pool_h = {k: rng.standard_normal((M,) + s).astype(f32) for k, s in shapes.items()}
    for v in pool_h.values():
        v[fixed + filled:] = np.nan
    pool = {k: _d(v, cuda) for k, v in pool_h.items()}
    other = rng.integers(0, 3, size=B)                          # the untaken: never unsafe, unsafe at the start, flagged
    first = np.where(other == 0, -1, np.where(other == 1, 0, 5)).astype(np.int32)
    flags = np.where(other == 2, 4, 0).astype(np.int32)
    pick = rng.choice(B, size=count, replace=False) if B else np.zeros(0, np.int64)
    first[pick], flags[pick] = rng.integers(1, 100, size=count), 0
    rows = {k: rng.standard_normal((B,) + s).astype(f32) for k, s in shapes.items()}
    mined = {k: _d(v, cuda) for k, v in rows.items()}
    mined.update(first=_d(first, cuda, np.int32), flags=_d(flags, cuda, np.int32))
    slot_of = torch.full((B,), SENT_I32, dtype=torch.int32, device=cuda)
    OE.scene_pool_push_evict(cfg, mined, pool, fixed, st, 2, 0.36, step, slot_of)
    torch.cuda.synchronize()
    want = PN.push_evict_np(first, flags, {"obst": None, **rows}, {"obst": None, **pool_h}, fixed, host["score"], host["visits"],
                            host["last"], 2, 0.36, step, host["state"])
    name = f"M={M} fixed={fixed} filled={filled} B={B} count={count}"
    got = {"slot_of": slot_of.cpu().numpy(), "state": np.array(st["state"].cpu().tolist()), "score": _words(st["score"]),
           "visits": st["visits"].cpu().numpy(), "last": st["last"].cpu().numpy(), **{f"pool.{k}": _words(v) for k, v in pool.items()}}
    assert got["state"].tolist() == want[4], name
    np.testing.assert_array_equal(got["slot_of"], want[5], err_msg=name)
    np.testing.assert_array_equal(got["score"], want[1].view(np.uint32), err_msg=f"{name}: score")
    np.testing.assert_array_equal(got["visits"], want[2], err_msg=f"{name}: visits")
    np.testing.assert_array_equal(got["last"], want[3], err_msg=f"{name}: last")
    for k in pool:
        np.testing.assert_array_equal(got[f"pool.{k}"], want[0][k].view(np.uint32), err_msg=f"{name}: pool.{k}")
        np.testing.assert_array_equal(got[f"pool.{k}"][:fixed], pool_h[k][:fixed].view(np.uint32), err_msg=f"{name}: a pinned slot was written")
    assert want[4][3] == count and want[4][6:] == [-3, -3], name
    return got, dict(evicted=want[4][4], dropped=want[4][5], to_empty=want[4][1] - filled, head_moved=int(want[4][0] != host["state"][0]))


@pytest.mark.parametrize("M", MS)
def test_push_evict_equals_the_restatement_and_repeats(cuda, M):
    seen = {"evicted": 0, "dropped": 0, "to_empty": 0, "head_moved": 0}
    for ci, fixed in enumerate(_fixeds(M)):
        cfg = _make_cfg(*CFGS[(ci + M) % len(CFGS)])
        R = M - fixed
        for filled in _filleds(R):
            for B in BS + [0]:
                # none taken, a few, and — where B allows — more than the empties and the evictable together can take
                for count in sorted({0, min(B, 2), min(B, (R - filled) + 1), B}):
                    seed = ((M * 7 + fixed) * 11 + filled) * 13 + B * 5 + count
                    a, what = _push_once(cuda, cfg, M, fixed, filled, B, count, seed)
                    for k, v in what.items():
                        seen[k] += v
            b, _ = _push_once(cuda, cfg, M, fixed, filled, 300, 300, 9)
            c, _ = _push_once(cuda, cfg, M, fixed, filled, 300, 300, 9)
            assert all(np.array_equal(b[k], c[k]) for k in b), "two runs of the same push differ"
    print(f"M={M}: {seen}")
    assert seen["to_empty"] > 0 and seen["dropped"] > 0 and (M < 5 or (seen["evicted"] > 0 and seen["head_moved"] > 0)), seen


# ---- 4. ScenePool(priority=True) on the head-on record ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def headon(cuda):
    from dgppo.env import Scenes, make_env
    from test_scene_mine_gpu import _headon_rollout
    env = make_env("LidarSpread", 2, num_obs=1)
    sc = Scenes.load(HEADON, env)
    return env, sc, _headon_rollout(env, sc, 3, MN.HEADON_T, cuda)


def test_priority_pool_scores_pushes_and_round_trips(cuda, headon):
    from dgppo.env import ScenePool
    env, sc, ro = headon
    _, t_star = MN.headon_oracle()
    pool = ScenePool(env, 4, pinned=sc, priority=True, draw_seed=3)
    assert pool.P == 1 and pool.fill() == (0, 0, 0) and pool.stats()["state"].tolist() == [0] * 8
    of = pool.draw(3, 3, 0, 0, 3)
    assert of.is_cuda and of.dtype == torch.int32 and of.cpu().tolist() == [0, 0, 0], "only the pinned slot is live: the empties are never drawn"
    assert ScenePool(env, 4, priority=True).draw(3, 3, 0, 0, 3).cpu().tolist() == [-1, -1, -1], "no live slot: the sampled reset"
    flags = pool.mix_flags(3)
    flags.copy_(torch.tensor([0, 0, 4], dtype=torch.int32))   # the third env fell back: no replay
    mined = pool.score_from(ro, of, flags, step=5, back=4)
    pool.push_from(ro, back=4, thresh=1e-6, step=5, mined=mined)
    st = pool.stats()
    half = f32(0.5)
    assert st["score"].view(np.uint32).tolist() == [f32(half + f32(f32(0.3) * f32(f32(1) - half))).view(np.uint32)] + [half.view(np.uint32)] * 3
    assert st["visits"].tolist() == [2, 0, 0, 0] and st["last"].tolist() == [5, 5, 5, 5]
    assert st["state"].tolist() == [0, 3, 3, 3, 0, 0, 2, 2] and pool.fill() == (3, 3, 3)
    np.testing.assert_array_equal(_words(pool.dev["agent"][1:]), _words(ro.agent_tm[t_star - 4]))
    np.testing.assert_array_equal(_words(pool.dev["agent"][0]), _words(sc.dev["agent"][0]))
    # a second push finds no empty slot and nothing evictable (no slot has two visits yet): all three are dropped, head stays
    before = {k: _words(v) for k, v in pool.dev.items()}
    pool.push_from(ro, back=4, thresh=1e-6, step=6)
    assert pool.stats()["state"].tolist() == [0, 3, 3, 3, 0, 3, 2, 2]
    assert all(np.array_equal(_words(v), before[k]) for k, v in pool.dev.items())
    # five score calls: slot 1 is replayed by one env that fails every other time (its score stays near 0.5: protected), slot 3 by
    # two envs that never fail, score 0.5 -> 0.35 -> 0.245 -> 0.1715 -> 0.12 (w = 0.42) -> 0.084 (w = 0.31): solved, evictable
    zero = torch.zeros(3, dtype=torch.int32, device=cuda)
    from dgppo_amd import ops_env as OE
    for step in range(7, 12):
        OE.scene_pool_score(env.cfg, torch.tensor([3, 3, 1], dtype=torch.int32, device=cuda), zero,
                            torch.tensor([-1, -1, 2 if step % 2 else -1], dtype=torch.int32, device=cuda), pool._stats, pool.beta, step)
    assert float(PN.w(pool.stats()["score"][3])) <= 0.36 < float(PN.w(pool.stats()["score"][1]))
    pool.push_from(ro, back=4, thresh=1e-6, step=12)
    st = pool.stats()
    assert st["state"].tolist() == [0, 3, 4, 3, 1, 2, 3, 1], "one evicted (position 2), two dropped; head one past it: (2 + 1) % 3"
    assert st["visits"].tolist() == [2, 5, 0, 0] and st["last"].tolist() == [5, 11, 5, 12] and st["score"][3] == half
    np.testing.assert_array_equal(_words(pool.dev["agent"][3]), _words(ro.agent_tm[t_star - 4, 0]))
    # the draw follows the restatement on the pool's own statistics
    got = pool.draw(64, 64, 13, 0, 64).cpu().numpy()
    np.testing.assert_array_equal(got, PN.draw_np(st["score"], st["last"], st["state"], 1, 16, 13, 3, 64, 64, 0, 64))
    assert set(got.tolist()) <= {0, 1, 2, 3} and len(set(got.tolist())) >= 2
    # the state round trip
    other = ScenePool(env, 4, pinned=sc, priority=True, draw_seed=3)
    other.load_state_dict(pool.state_dict())
    assert all(np.array_equal(other.stats()[k], st[k]) for k in st) and all(np.array_equal(_words(other.dev[k]), _words(pool.dev[k])) for k in pool.dev)
    np.testing.assert_array_equal(other.draw(64, 64, 13, 0, 64).cpu().numpy(), got)
    with pytest.raises(ValueError, match="the stored pool is a priority pool"):
        ScenePool(env, 4, pinned=sc).load_state_dict(pool.state_dict())
    # the plain ring is what it was: a [4] state, the ring push
    ring = ScenePool(env, 4, pinned=sc)
    ring.push_from(ro, back=4, thresh=1e-6)
    assert ring.state.cpu().tolist() == [0, 3, 3, 3]


# ---- 5. the drawn mix of the engine ------------------------------------------------------------------------------------------------------
def test_engine_drawn_mix_equals_the_host_mix(cuda, monkeypatch):
    """LidarSpread 3 / 1, B = 8, T = 4: the rollout started through SceneMixDrawn is the rollout started through SceneMix with the
    same scene_of copied to the host, every word of the record; the flags go to the given buffer for the envs scene_of names, and
    rollout_pair's deterministic twin writes none"""
    from dgppo.env import ScenePool
    from dgppo_amd.env.scenes import SceneMixDrawn
    from test_engine_gpu import _setup
    from test_scene_mix_gpu import _clone, _n3_scenes, _same_words
    B, T_, J = 8, 4, 0.01
    monkeypatch.setenv("DGPPO_HIPGRAPH", "0")
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 1, B, T_, cuda, 16, 4, use_graphs=True)
    sc = _n3_scenes(cuda)
    pool = ScenePool(sc_env(sc), 5, pinned=sc, priority=True, draw_seed=11)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    for step in (0, 1):
        of = pool.draw(B, 5, step, 0, B)
        host = of.cpu().numpy()
        assert int((host >= 0).sum()) == 5 and set(host[host >= 0].tolist()) <= {0, 1}, "the three empty slots are never drawn"
        for stochastic in (False, True):
            flags = torch.full((B,), SENT_I32, dtype=torch.int32, device=cuda)
            drawn = _clone(eng.rollout(seeds, stochastic, 17, start=SceneMixDrawn(pool, of, flags, J)))
            mixed = _clone(eng.rollout(seeds, stochastic, 17, start=pool.mix(host, J)))
            for name, (v, _) in mixed.items():
                _same_words(drawn[name][0], v, f"step {step} stochastic={stochastic}: {name}")
            assert flags.cpu().tolist() == [0 if s >= 0 else SENT_I32 for s in host]
        flags = torch.full((B,), SENT_I32, dtype=torch.int32, device=cuda)
        ro, det = eng.rollout_pair(seeds, seeds + 1, 17, start=pool.mix_drawn(of, flags, J))
        torch.cuda.synchronize()
        assert flags.cpu().tolist() == [0 if s >= 0 else SENT_I32 for s in host]
        flags.fill_(SENT_I32)
        twin = _clone(eng.rollout(seeds + 1, False, start=pool.mix_drawn(of, None, J)))
        assert (flags == SENT_I32).all(), "a start without a flags buffer writes none"
        for name, (v, _) in _clone(det).items():
            _same_words(v, twin[name][0], f"step {step}: the deterministic twin, {name}")
    assert int(eng.reset_failed.item()) == 0 and int(eng.scene_fallback.item()) == 0 and eng._mix_used and eng._mix_pool is pool


def sc_env(sc):
    from dgppo.env import make_env
    return make_env("LidarSpread", sc.num_agents, num_obs=sc.cfg.n_obs)


# ---- 6. train.py -----------------------------------------------------------------------------------------------------------------------------
PRIORITY_KEYS = ("rollout/scene_replay_fail_frac", "rollout/scene_pool_evicted", "rollout/scene_pool_dropped", "rollout/scene_pool_score_mean")
ISSUE = ["--mine-scenes", "8", "--scene-frac", "0.25"]
PINNED = ["--mine-scenes", "4", "--mine-back", "4", "--scene-frac", "0.5", "--scenes", HEADON, "--scene-jitter", "0.05", "--scene-priority"]


def _train(mod, log_dir, extra):
    argv = ["--env", "LidarSpread", "-n", "2", "--algo", "dgppo", "--obs", "1", "--steps", "3", "--n-env-train", "16", "--batch-size",
            "2048", "--n-env-test", "4", "--eval-interval", "100", "--save-interval", "1", "--log-dir", str(log_dir)]
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


def _updates(run_dir):
    rows = [json.loads(ln) for ln in open(os.path.join(run_dir, "metrics.jsonl"))]
    return [r for r in rows if "policy/loss" in r]


def test_train_py_never_draws_an_empty_slot(cuda, tmp_path):
    """the issue's command: with --scene-priority no env falls back at step 0, because empty slots are never drawn; without it the
    four scene envs of both rollouts draw empty ring slots and are counted"""
    mod = _load_train_py()
    _train(mod, tmp_path / "prio", ISSUE + ["--scene-priority"])
    _train(mod, tmp_path / "ring", ISSUE)
    prio, ring = _updates(_run_of(tmp_path / "prio")), _updates(_run_of(tmp_path / "ring"))
    assert [r["step"] for r in prio] == [0, 1, 2, 3] == [r["step"] for r in ring]
    print("[scene priority] fallback per iteration:", [r["rollout/scene_fallback"] for r in prio], "against the ring's",
          [r["rollout/scene_fallback"] for r in ring])
    assert prio[0]["rollout/scene_fallback"] == 0 and ring[0]["rollout/scene_fallback"] > 0
    pushed = 0
    for r in prio:
        assert set(PRIORITY_KEYS) <= set(r) and all(np.isfinite(r[k]) for k in PRIORITY_KEYS)
        assert 0 <= r["rollout/scene_replay_fail_frac"] <= 1 and 0 <= r["rollout/scene_pool_score_mean"] <= 1
        assert r["rollout/scene_pool_taken"] == r["rollout/scene_pool_pushed"] - pushed + r["rollout/scene_pool_dropped"]
        pushed = r["rollout/scene_pool_pushed"]
    assert prio[0]["rollout/scene_replay_fail_frac"] == 0 and prio[0]["rollout/scene_pool_evicted"] == 0, "nothing to replay at step 0"
    assert not any(k in r for r in ring for k in PRIORITY_KEYS)


def _npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].view(np.uint32) if z[k].dtype == f32 else z[k]) for k in z.files}


def test_train_py_logs_saves_and_resumes_the_statistics(cuda, tmp_path):
    """a run with the head-on scene pinned (so that the pool has replays from step 0 on and fills): the new keys are logged, the
    scenes files carry score, visits and last and still load; a run stopped after step 2 (the newest state but one: older ones are
    not kept) and resumed carries on with the same pool and statistics: everything the iteration from the restored state does to
    the pool happens before its update, so scenes/3.npz — the pool after iteration 2 — is compared word for word (what follows
    an update is not: DESIGN.md §7)"""
    from dgppo.env import Scenes, make_env
    mod = _load_train_py()
    _train(mod, tmp_path / "a", PINNED)
    run_a = _run_of(tmp_path / "a")
    ups = _updates(run_a)
    assert len(ups) == 4 and all(set(PRIORITY_KEYS) <= set(r) for r in ups)
    print("[scene priority] per iteration:", [[r[k] for k in PRIORITY_KEYS] + [r["rollout/scene_pool_fill"], r["rollout/scene_fallback"]] for r in ups])
    assert ups[0]["rollout/scene_replay_fail_frac"] > 0 or ups[-1]["rollout/scene_pool_fill"] >= 1, "no replay failed and nothing was mined"
    env = make_env("LidarSpread", 2, num_obs=1)
    assert sorted(os.listdir(os.path.join(run_a, "scenes"))) == ["0.npz", "1.npz", "2.npz", "3.npz"]
    for step in range(4):
        path = os.path.join(run_a, "scenes", f"{step}.npz")
        z = _npz(path)
        S = z["agent"].shape[0]
        assert {"score", "visits", "last"} <= set(z) and z["score"].shape == z["visits"].shape == z["last"].shape == (S,)
        assert z["visits"].dtype == np.int32 and z["last"].dtype == np.int32
        assert Scenes.load(path, env).S == S, "the file loads as before"
    z0 = _npz(os.path.join(run_a, "scenes", "0.npz"))
    assert z0["score"].view(f32).tolist() == [0.5] and z0["visits"].tolist() == [0] and z0["last"].tolist() == [0]
    z1 = _npz(os.path.join(run_a, "scenes", "1.npz"))
    assert z1["visits"][0] > 0, "the pinned slot was replayed at step 0: it was the only live one"
    # stopped after step 2 and resumed
    run_c = str(tmp_path / "stopped")
    shutil.copytree(run_a, run_c)
    shutil.rmtree(os.path.join(run_c, "models", "3"))
    os.remove(os.path.join(run_c, "resume", "3.pkl"))
    os.remove(os.path.join(run_c, "scenes", "3.npz"))
    os.remove(os.path.join(run_c, "scenes", "2.npz"))
    _train(mod, tmp_path / "a", PINNED + ["--resume", run_c])
    ups_c = _updates(run_c)
    assert [(r["step"], sorted(r)) for r in ups_c] == [(r["step"], sorted(r)) for r in ups]
    pool_of = lambda r: [r[k] for k in PRIORITY_KEYS + ("rollout/scene_pool_fill", "rollout/scene_pool_pushed", "rollout/scene_pool_taken",
                                                        "rollout/scene_fallback")]
    assert pool_of(ups_c[2]) == pool_of(ups[2]), "the iteration from the restored state"
    for step in (2, 3):
        a, c = _npz(os.path.join(run_a, "scenes", f"{step}.npz")), _npz(os.path.join(run_c, "scenes", f"{step}.npz"))
        assert sorted(a) == sorted(c) and all(np.array_equal(a[k], c[k]) for k in a), f"scenes/{step}.npz: the resumed pool differs"
    with pytest.raises(SystemExit, match=r"--scene-priority \(True in the stopped run, False now\)"):
        _train(mod, tmp_path / "a", PINNED[:-1] + ["--resume", run_c])
