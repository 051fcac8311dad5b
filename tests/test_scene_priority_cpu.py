"""The pool by priority without a GPU: the restatement (tests/scene_priority_np.py) on known answers — q at its clamps, the pick, the
scene envs against mix_assignment, the distribution of the draw, the evicting push by hand — and every refusal that touches no
device: the entry points', the bindings', ScenePool's, the Trainer's and train.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_priority_np as PN  # noqa: E402
from test_scene_mix_cpu import BASE, HEADON, _load_train_py  # noqa: E402
from test_scenes_cpu import _cfg  # noqa: E402

f32 = np.float32
DRAW_SEED = 2024                                             # the distribution test below checks that the restatement passes with it


# ---- q -------------------------------------------------------------------------------------------------------------------------------
def test_q_known_answers_and_clamps():
    nan, inf = f32(np.nan), f32(np.inf)
    assert [int(PN.q(s)) for s in (0.0, 0.5, 1.0, nan)] == [1, 65536, 1, 1]
    assert int(PN.q(0.25)) == 49152 and int(PN.q(0.75)) == 49152           # w = 0.75: (uint32)49151.25 + 1
    # either side of the lower clamp of w: below 0 (s outside [0, 1], and the infinities, whose w is -inf) and just above it
    assert [int(PN.q(s)) for s in (-0.25, 1.25, inf, -inf, np.nextafter(f32(0), f32(-1)))] == [1, 1, 1, 1, 1]
    tiny = np.nextafter(f32(0), f32(1))
    assert float(PN.w(tiny)) > 0.0 and int(PN.q(tiny)) == 1
    assert int(PN.q(f32(1e-3))) == int(f32(f32(4e-3) * f32(f32(1) - f32(1e-3))) * f32(65535)) + 1 > 1
    below_one = np.nextafter(f32(1), f32(0))
    assert float(PN.w(below_one)) > 0.0 and float(PN.w(np.nextafter(f32(1), f32(2)))) == 0.0
    # the clamp itself, on w: a NaN and a negative value give 0, a value above 1 gives 1, the values in between stay
    vals = [nan, -inf, f32(-1e-30), f32(-0.0), f32(0), tiny, below_one, f32(1), np.nextafter(f32(1), f32(2)), f32(7), inf]
    got = PN.w_clamp(np.array(vals, f32)).tolist()
    assert got == [0.0, 0.0, 0.0, 0.0, 0.0, float(tiny), float(below_one), 1.0, 1.0, 1.0, 1.0]
    assert PN.q_w(np.array([0, tiny, below_one, 1], f32)).tolist() == [1, 1, 65535, 65536]
    # w never leaves [0, 1] and q never [1, 65536], whatever the score
    s = np.concatenate([np.linspace(-2, 3, 100001).astype(f32), np.array([nan, inf, -inf], f32)])
    wv, qv = PN.w(s), PN.q(s)
    assert wv.min() >= 0 and wv.max() <= 1 and qv.min() == 1 and qv.max() == 65536
    assert int(qv[np.nanargmin(np.abs(s - f32(0.5)))]) == 65536


# ---- the pick, the scene envs, the distribution ---------------------------------------------------------------------------------------
def test_pick_known_answers():
    Q = [5, 0, 3, 2]
    assert PN.pick(Q, 0) == 0 and PN.pick(Q, 4) == 0 and PN.pick(Q, 5) == 2, "the zero-weight slot in the middle is stepped over"
    assert PN.pick(Q, 7) == 2 and PN.pick(Q, 8) == 3 and PN.pick(Q, sum(Q) - 1) == 3
    assert PN.pick([0, 0, 4], 0) == 2 and PN.pick([4, 0, 0], 3) == 0
    with pytest.raises(AssertionError):
        PN.pick(Q, sum(Q))
    # the binary search of draw_Q and the linear pick agree for every t of a small table
    Q = [3, 0, 0, 1, 7, 0]
    total = sum(Q)
    for k in range(64):
        t = PN.draw_t(k, 5, DRAW_SEED, total)
        assert 0 <= t < total and PN.draw_Q(Q, [k], 5, DRAW_SEED) == [PN.pick(Q, t)]
    assert PN.draw_Q([0, 0, 0], [0, 1], 5, DRAW_SEED) == [-1, -1]


@pytest.mark.parametrize("n_total,n_scene,lo,hi", [(16, 8, 0, 16), (16, 5, 0, 16), (16, 5, 4, 12), (128, 13, 64, 128), (12, 11, 0, 12),
                                                   (7, 3, 2, 7), (16, 0, 0, 16), (16, 16, 0, 16), (1, 1, 0, 1), (300, 77, 299, 300)])
def test_scene_envs_are_those_of_mix_assignment(n_total, n_scene, lo, hi):
    from dgppo_amd.env.scenes import mix_assignment
    score, last = np.full(3, 0.5, f32), np.zeros(3, np.int32)
    of = PN.draw_np(score, last, [0, 3, 0, 0, 0, 0, 0, 0], 0, 16, 4, DRAW_SEED, n_total, n_scene, lo, hi - lo)
    want = mix_assignment(n_total, n_scene, 3, 4, lo, hi)
    np.testing.assert_array_equal(of >= 0, want >= 0)
    assert of.dtype == np.int32 and set(of[of < 0].tolist()) <= {-1} and (of < 3).all()
    is_scene, ks = PN.scene_envs(n_total, n_scene, lo, hi - lo)
    mine = [ks[b] for b in np.flatnonzero(is_scene)]
    assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True, "consecutive ordinals, in env order"
    for b in np.flatnonzero(is_scene):
        assert (want[b] - 4) % 3 == ks[b] % 3, "the ordinal is mix_assignment's k"


def test_draw_distribution():
    Q, n = [1, 0, 3], 4096
    got = np.array(PN.draw_Q(Q, list(range(n)), 3, DRAW_SEED))
    assert not (got == 1).any(), "a zero-weight slot was drawn"
    share = float((got == 2).mean())
    sd = (0.75 * 0.25 / n) ** 0.5
    print(f"[scene priority] share of slot 2: {share:.4f} (0.75 +- {4 * sd:.4f})")
    assert abs(share - 0.75) <= 4 * sd
    assert got.tolist() != PN.draw_Q(Q, list(range(n)), 4, DRAW_SEED), "the step is part of the counter"
    assert got.tolist() != PN.draw_Q(Q, list(range(n)), 3, DRAW_SEED + (1 << 32)), "the high word of the seed is part of the key"


def test_weights_liveness_and_staleness():
    score = np.array([0.5, 0.5, 0.25, 0.5, 0.5], f32)
    last = np.array([0, 10, 3, 3, 3], np.int32)
    # fixed 1, filled 2: slots 0 (pinned), 1, 2 are live; age = min(1 + max(step - last, 0), cap)
    assert PN.weights(score, last, 1, 2, 5, 16) == [65536 * 6, 65536 * 1, 49152 * 3, 0, 0], "step < last counts as age 1"
    assert PN.weights(score, last, 1, 2, 5, 1) == [65536, 65536, 49152, 0, 0]
    assert PN.weights(score, last, 1, 2, 5000, 1024)[0] == 65536 * 1024
    assert PN.weights(score, last, 0, 0, 5, 16) == [0] * 5, "an empty pool has no live slot"


# ---- the score ---------------------------------------------------------------------------------------------------------------------------
def test_score_by_hand():
    scene_of = np.array([0, 0, 0, 2, -1, 2, 1, 0], np.int32)
    mix_flags = np.array([0, 0, 0, 0, 77, 1, 2, 0], np.int32)       # env 4 fell outside the mix, envs 5 and 6 fell back
    first = np.array([3, -1, 0, -1, 5, 5, 5, -1], np.int32)
    score, visits, last, state = PN.score_np(scene_of, mix_flags, first, np.full(4, 0.5, f32), [1, 1, 1, 1], [9, 9, 9, 9], 0.3, 12,
                                             [1, 2, 3, 4, 5, 6, -1, -1])
    # slot 0: four replays, two failed (first 3 and first 0); slot 2: one replay, none failed; slots 1 and 3: nobody
    assert score[0] == f32(0.5) and score[2] == f32(f32(0.5) + f32(f32(0.3) * f32(f32(0) - f32(0.5)))) and score[1] == score[3] == f32(0.5)
    assert visits.tolist() == [5, 1, 2, 1] and last.tolist() == [12, 9, 12, 9] and state == [1, 2, 3, 4, 5, 6, 5, 2]


# ---- the evicting push, by hand ------------------------------------------------------------------------------------------------------------
def _push(first, score, visits, state, fixed=1, min_visits=2, evict_w=0.36, step=7):
    M, B = len(score), len(first)
    rows = {"agent": (np.arange(B, dtype=f32) + 100).reshape(B, 1), "obst": None}
    pool = {"agent": -np.arange(M, dtype=f32).reshape(M, 1) - 1, "obst": None}
    out = PN.push_evict_np(np.asarray(first, np.int32), np.zeros(B, np.int32), rows, pool, fixed, np.asarray(score, f32),
                           np.asarray(visits, np.int32), np.zeros(M, np.int32), min_visits, evict_w, step, state)
    return out[0]["agent"][:, 0].tolist(), out[1].tolist(), out[2].tolist(), out[3].tolist(), out[4], out[5].tolist()


def test_evicting_push_by_hand():
    # M = 6, one pinned slot, ring of 5; positions 0..2 are filled (slots 1..3), head at position 1.
    # slot 1: solved (score 0.02 -> w = 0.0784), visited: evictable     slot 2: w(0.5) = 1 > evict_w: protected
    # slot 3: hopeless (0.98), but visits 1 < min_visits: protected
    score, visits = [0.02, 0.02, 0.5, 0.98, 0.5, 0.5], [9, 5, 5, 1, 0, 0]
    state = [1, 3, 10, 0, -1, -1, 40, 20]
    # one taken env: the first empty (position 3 = slot 4) takes it; head stays while only empties are written
    agent, sc, vis, last, st, slot_of = _push([0, 4, -1], score, visits, state)
    assert slot_of == [-1, 4, -1] and agent == [-1, -2, -3, -4, 101, -6]
    assert st == [1, 4, 11, 1, 0, 0, 40, 20] and vis == [9, 5, 5, 1, 0, 0] and last == [0, 0, 0, 0, 7, 0]
    # four taken envs: empties first (slots 4, 5), then the one evictable (slot 1), the fourth is dropped; head passes position 0
    agent, sc, vis, last, st, slot_of = _push([2, 0, 3, 1, -1, 9, 8], score, visits, state)
    assert slot_of == [4, -1, 5, 1, -1, -1, -1]
    assert agent == [-1, 103, -3, -4, 100, 102] and st == [1, 5, 13, 5, 1, 2, 40, 20]
    assert [f32(v) for v in sc] == [f32(v) for v in (0.02, 0.5, 0.5, 0.98, 0.5, 0.5)] and vis == [9, 0, 5, 1, 0, 0]
    assert last == [0, 7, 0, 0, 7, 7]
    assert agent[0] == -1 and sc[0] == float(f32(0.02)), "the pinned slot is untouched, solved as it is"
    # a full ring: ring order from head; min_visits 0 and evict_w 1 make every filled slot evictable
    full = [3, 5, 10, 0, 0, 0, 0, 0]
    agent, _, vis, _, st, slot_of = _push([1, 1, 1], score, visits, full, min_visits=0, evict_w=1.0)
    assert slot_of == [4, 5, 1] and st[:6] == [1, 5, 13, 3, 3, 0], "positions 3, 4, 0: head ends one past position 0"
    # the protections, each alone: nothing evictable, so everything is dropped and head stays
    _, _, _, _, st, slot_of = _push([1, 1], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [9] * 6, full)
    assert slot_of == [-1, -1] and st[:6] == [3, 5, 10, 2, 0, 2], "w > evict_w protects"
    _, _, _, _, st, slot_of = _push([1, 1], [0.0] * 6, [1] * 6, full)
    assert slot_of == [-1, -1] and st[:6] == [3, 5, 10, 2, 0, 2], "visits < min_visits protects"
    # w == evict_w is evictable; a NaN score has w = 0
    e = float(PN.w(f32(0.1)))
    _, _, _, _, st, slot_of = _push([1, 1], [0.5, 0.1, float("nan"), 0.5, 0.5, 0.5], [9] * 6, [0, 5, 0, 0, 0, 0, 0, 0], evict_w=e)
    assert slot_of == [1, 2] and st[:6] == [2, 5, 2, 2, 2, 0]
    # none taken, and no env at all
    for first in ([0, -1, 0], []):
        agent, _, _, _, st, slot_of = _push(first, score, visits, state)
        assert slot_of == [-1] * len(first) and agent == [-1, -2, -3, -4, -5, -6] and st == [1, 3, 10, 0, 0, 0, 40, 20]


# ---- refusals that touch no device ---------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = _cfg("LidarSpread", 2, 1)
    x = C.c_void_p(64)                                        # never dereferenced: every call below is refused before a launch
    bad = _cfg("LidarSpread", 2, 1)
    bad.kind = 17
    vmas = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 2, 0)
    no_obs = _cfg("LidarSpread", 2, 0)

    def score(cfg=cfg, M=4, beta=0.3, B=4, **over):
        q = dict(scene_of=x, mix_flags=x, first=x, score=x, visits=x, last=x, tally=x, state=x)
        q.update(over)
        return lib.dgppo_env_scene_pool_score(C.byref(cfg), q["scene_of"], q["mix_flags"], q["first"], q["score"], q["visits"], q["last"],
                                              q["tally"], M, beta, 3, q["state"], B, None)

    def draw(cfg=cfg, M=4, fixed=0, age_cap=16, n_total=8, n_scene=4, lo=0, B=4, **over):
        q = dict(score=x, last=x, state=x, cum=x, scene_of=x)
        q.update(over)
        return lib.dgppo_env_scene_pool_draw(C.byref(cfg), q["score"], q["last"], q["state"], M, fixed, age_cap, 3, 7, n_total, n_scene,
                                             lo, q["cum"], q["scene_of"], B, None)

    def push(cfg=cfg, M=4, fixed=0, min_visits=2, evict_w=0.36, B=4, **over):
        q = dict(first=x, flags=x, agent_t=x, goal_t=x, obst_t=x, pool_agent=x, pool_goal=x, pool_obst=x, score=x, visits=x, last=x,
                 order=x, state=x, slot_of=x)
        q.update(over)
        return lib.dgppo_env_scene_pool_push_evict(C.byref(cfg), q["first"], q["flags"], q["agent_t"], q["goal_t"], q["obst_t"],
                                                   q["pool_agent"], q["pool_goal"], q["pool_obst"], q["score"], q["visits"], q["last"],
                                                   q["order"], M, fixed, min_visits, evict_w, 3, q["state"], q["slot_of"], B, None)
    nan = float("nan")
    for fn, name, cases in (
            (score, b"dgppo_env_scene_pool_score",
             [dict(cfg=bad), dict(B=-1), dict(M=0), dict(M=65537), dict(beta=0.0), dict(beta=1.5), dict(beta=nan)] +
             [{k: None} for k in ("scene_of", "mix_flags", "first", "score", "visits", "last", "tally", "state")]),
            (draw, b"dgppo_env_scene_pool_draw",
             [dict(cfg=bad), dict(B=-1), dict(M=0), dict(M=65537), dict(fixed=-1), dict(fixed=4), dict(age_cap=0), dict(age_cap=1025),
              dict(n_total=0), dict(n_scene=9), dict(n_scene=-1), dict(lo=-1), dict(lo=5), dict(n_total=2 ** 31)] +
             [{k: None} for k in ("score", "last", "state", "cum", "scene_of")]),
            (push, b"dgppo_env_scene_pool_push_evict",
             [dict(cfg=bad), dict(B=-1), dict(M=0), dict(M=65537), dict(fixed=-1), dict(fixed=4), dict(M=1, fixed=1), dict(min_visits=-1),
              dict(evict_w=-0.1), dict(evict_w=1.1), dict(evict_w=nan), dict(cfg=no_obs), dict(cfg=no_obs, obst_t=None),
              dict(cfg=_cfg("LidarSpread", 65, 1))] +
             [{k: None} for k in ("first", "flags", "agent_t", "goal_t", "obst_t", "pool_agent", "pool_goal", "pool_obst", "score",
                                  "visits", "last", "order", "state")])):
        for kw in cases:
            assert fn(**kw) != 0, (name, kw)
            assert name in lib.dgppo_last_error(), (kw, lib.dgppo_last_error())
        assert fn(cfg=vmas) != 0                              # every scene entry point names the kind it does not take
        assert name in lib.dgppo_last_error() and b"VMASReverseTransport" in lib.dgppo_last_error()
    assert draw(B=0) == 0 and draw(B=0, lo=8) == 0            # nothing to draw: no launch


def test_binding_and_class_refusals():
    from dgppo_amd import _native as N
    from dgppo_amd import ops_env as OE
    from dgppo_amd.algo.dgppo import DGPPO
    from dgppo_amd.env import scenes as SC
    cfg = _cfg("LidarSpread", 2, 1)
    vm = N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)
    M, B = 4, 3
    stats = OE.alloc_pool_stats(M, "cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in stats.items()} == {
        "score": ((M,), torch.float32), "visits": ((M,), torch.int32), "last": ((M,), torch.int32), "state": ((8,), torch.int32),
        "tally": ((2 * M,), torch.int32), "cum": ((M,), torch.int64), "order": ((M,), torch.int32)}
    assert stats["score"].tolist() == [0.5] * M and not stats["visits"].any() and not stats["last"].any() and not stats["tally"].any()
    of = torch.zeros(B, dtype=torch.int32)
    for kw, match in ((dict(age_cap=0), "age_cap"), (dict(age_cap=1025), "age_cap"), (dict(fixed=4), "fixed"), (dict(n_scene=9), "n_scene"),
                      (dict(n_total=0), "n_total"), (dict(lo=6), "window"), (dict(lo=-1), "window"),
                      (dict(stats={**stats, "cum": stats["cum"][:2]}), "stats.cum"),
                      (dict(stats={**stats, "state": stats["state"][:4]}), "stats.state"), (dict(cfg=vm), "VMASReverseTransport")):
        a = dict(cfg=cfg, stats=stats, fixed=0, age_cap=16, n_total=8, n_scene=4, lo=0)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_pool_draw(a["cfg"], a["stats"], a["fixed"], a["age_cap"], 3, 7, a["n_total"], a["n_scene"], a["lo"], of)
    big = OE.alloc_pool_stats(65537, "cpu")
    with pytest.raises(ValueError, match=r"M must be in \[1, 65536\]"):
        OE.scene_pool_draw(cfg, big, 0, 16, 3, 7, 8, 4, 0, of)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # past the refusals: there is no host kernel
        OE.scene_pool_draw(cfg, stats, 0, 16, 3, 7, 8, 4, 0, of)
    for kw, match in ((dict(beta=0.0), "beta"), (dict(beta=1.5), "beta"), (dict(beta=float("nan")), "beta"),
                      (dict(first=of[:2]), "first"), (dict(mix_flags=of[:2]), "mix_flags"), (dict(cfg=vm), "VMASReverseTransport"),
                      (dict(stats={**stats, "tally": stats["tally"][:M]}), "stats.tally")):
        a = dict(cfg=cfg, mix_flags=of, first=of, stats=stats, beta=0.3)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_pool_score(a["cfg"], of, a["mix_flags"], a["first"], a["stats"], a["beta"], 3)
    mined = OE.alloc_mined(cfg, B, "cpu")
    pool = {k: torch.zeros((M,) + tuple(v.shape[1:])) for k, v in mined.items() if k in ("agent", "goal", "obst")}
    for kw, match in ((dict(fixed=4), "fixed"), (dict(min_visits=-1), "min_visits"), (dict(evict_w=1.5), "evict_w"),
                      (dict(evict_w=float("nan")), "evict_w"), (dict(pool={**pool, "goal": pool["goal"][:3]}), "pool.goal"),
                      (dict(stats={**stats, "order": stats["order"][:2]}), "stats.order"), (dict(cfg=vm), "VMASReverseTransport"),
                      (dict(slot_of=of[:2]), "slot_of")):
        a = dict(cfg=cfg, pool=pool, fixed=0, stats=stats, min_visits=2, evict_w=0.36, slot_of=None)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            OE.scene_pool_push_evict(a["cfg"], mined, a["pool"], a["fixed"], a["stats"], a["min_visits"], a["evict_w"], 3, a["slot_of"])

    class FakeEnv:
        KIND, device = "LidarSpread", "cpu"

        def __init__(self, cfg):
            self.cfg = cfg
    for kw, match in ((dict(capacity=65537), "with priority, capacity must be <= 65536"), (dict(beta=0.0), "beta"), (dict(beta=1.01), "beta"),
                      (dict(age_cap=0), "age_cap"), (dict(age_cap=1025), "age_cap"), (dict(age_cap=2.5), "age_cap"),
                      (dict(min_visits=-1), "min_visits"), (dict(evict_w=-0.1), "evict_w"), (dict(evict_w=1.1), "evict_w"),
                      (dict(draw_seed=-1), "draw_seed"), (dict(draw_seed=2 ** 64), "draw_seed")):
        a = dict(capacity=8, priority=True)
        a.update(kw)
        with pytest.raises(ValueError, match="ScenePool: " + match):
            SC.ScenePool(FakeEnv(cfg), a.pop("capacity"), **a)
    SC.ScenePool(FakeEnv(cfg), 65537)                          # the plain ring has no such limit, and ignores the priority arguments
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        SC.ScenePool(FakeEnv(vm), 4, priority=True)
    ring, prio = SC.ScenePool(FakeEnv(cfg), 4), SC.ScenePool(FakeEnv(cfg), 4, priority=True, draw_seed=5)
    assert tuple(ring.state.shape) == (4,) and tuple(prio.state.shape) == (8,) and ring._stats is None
    assert prio.fill() == (0, 0, 0) and ring.fill() == (0, 0, 0)
    for call in (lambda: ring.draw(8, 4, 0, 0, 8), lambda: ring.stats(), lambda: ring.score_from(None, of, of, 0),
                 lambda: ring.mix_flags(3), lambda: ring.mix_drawn(of), lambda: ring.drawn(of)):
        with pytest.raises(ValueError, match="needs ScenePool\\(..., priority=True\\)"):
            call()
    with pytest.raises(ValueError, match="lo <= hi"):
        prio.draw(8, 4, 0, 5, 3)
    st = prio.stats()
    assert st["score"].tolist() == [0.5] * 4 and st["visits"].tolist() == [0] * 4 and st["last"].tolist() == [0] * 4
    assert st["state"].tolist() == [0] * 8 and st["score"].dtype == f32 and st["visits"].dtype == np.int32
    # the state round trip carries the statistics; the two modes do not load each other
    prio._stats["score"][1], prio._stats["visits"][2], prio._stats["last"][3], prio.state[4] = 0.25, 7, 9, 3
    other = SC.ScenePool(FakeEnv(cfg), 4, priority=True)
    other.load_state_dict(prio.state_dict())
    assert all(np.array_equal(other.stats()[k], prio.stats()[k]) for k in ("score", "visits", "last", "state"))
    with pytest.raises(ValueError, match="the stored pool is a priority pool, this one is a plain ring"):
        ring.load_state_dict(prio.state_dict())
    with pytest.raises(ValueError, match="the stored pool is a plain ring, this one is a priority pool"):
        prio.load_state_dict(ring.state_dict())
    # collect's keyword
    algo = DGPPO.__new__(DGPPO)
    algo._env, algo.world, algo.rank = FakeEnv(cfg), 1, 0
    draw = prio.drawn(of)
    assert isinstance(draw, SC.SceneDraw) and draw.scene_of is of and draw.flags is prio.mix_flags(3)
    with pytest.raises(ValueError, match="need scenes"):
        algo._scene_start(None, None, 0.0, 3, draw)
    with pytest.raises(ValueError, match="scene_of and scene_ids exclude each other"):
        algo._scene_start(prio, np.zeros(3, np.int32), 0.0, 3, draw)
    with pytest.raises(ValueError, match="a drawn scene_of needs scenes=ScenePool"):
        algo._scene_start(ring, None, 0.0, 3, draw)
    with pytest.raises(ValueError, match="one entry per key"):
        algo._scene_start(prio, None, 0.0, 4, draw)
    start = algo._scene_start(prio, None, 0.05, 3, draw)
    assert isinstance(start, SC.SceneMixDrawn) and start.scene_of is of and start.flags is prio.mix_flags(3) and start.jitter == 0.05
    assert start._replace(flags=None).flags is None and not isinstance(start, SC.SceneMix)
    with pytest.raises(ValueError, match="device int32 tensor"):                    # the drawn start takes no host list
        OE.mixed_start_drawn(cfg, torch.zeros(3, dtype=torch.int64), OE.State.empty(cfg, 3, "cpu"), prio.dev, of, 0.0)


def test_train_py_priority_flag(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mod = _load_train_py()
    ap = mod.build_parser()
    assert ap.parse_args(BASE).scene_priority is False and "scene_priority" in mod._RESUME_LATER
    ok = ["--mine-scenes", "4", "--scene-frac", "0.5", "--scene-priority"]
    mod.check_scenes(ap.parse_args(BASE + ok))
    assert ap.parse_args(BASE + ok).scene_priority is True and ap.parse_args(BASE + ok[:-1] + ["--mine-priority"]).scene_priority is True
    mod.check_scenes(ap.parse_args(BASE + ok + ["--scenes", HEADON, "--scene-jitter", "0.05"]))
    for extra, match in ((["--scene-priority"], "--scene-priority needs --mine-scenes"),
                         (["--scene-priority", "--scenes", HEADON, "--scene-frac", "0.5"], "--scene-priority needs --mine-scenes"),
                         (["--mine-scenes", "65537", "--scene-frac", "0.5", "--scene-priority"], "at most 65536"),
                         (ok + ["--gpus", "2"], "--mine-scenes runs on one rank"),
                         (ok + ["--env", "VMASReverseTransport"], "VMASReverseTransport")):
        with pytest.raises(SystemExit, match=match):
            mod.check_scenes(ap.parse_args(BASE + extra))
    mod.check_scenes(ap.parse_args(BASE + ["--mine-scenes", "65537", "--scene-frac", "0.5"]))
    monkeypatch.setattr(mod, "train", lambda a: pytest.fail("a rank was started"))
    with pytest.raises(SystemExit, match="--scene-priority needs --mine-scenes"):
        mod.main(BASE + ["--scene-priority"])


def test_resume_compares_the_priority_flag():
    mod = _load_train_py()
    ap = mod.build_parser()
    a = ap.parse_args(BASE + ["--mine-scenes", "4", "--scene-frac", "0.5", "--scene-priority"])
    stored = mod._flags_to_store(a)
    assert stored["scene_priority"] is True
    mod.check_resume_flags(a, stored)
    plain = ap.parse_args(BASE + ["--mine-scenes", "4", "--scene-frac", "0.5"])
    with pytest.raises(SystemExit, match=r"--scene-priority \(True in the stopped run, False now\)"):
        mod.check_resume_flags(plain, stored)
    old = {k: v for k, v in mod._flags_to_store(plain).items() if k != "scene_priority"}      # a run stopped before the flag existed
    mod.check_resume_flags(plain, old)
    with pytest.raises(SystemExit, match=r"--scene-priority \(False in the stopped run, True now\)"):
        mod.check_resume_flags(a, old)


def test_trainer_refusals():
    from dgppo.trainer.trainer import Trainer
    params = {"run_name": "x", "training_steps": 1, "eval_interval": 1, "eval_epi": 1, "save_interval": 1}

    class Algo:
        world, rank = 1, 0
    with pytest.raises(ValueError, match="scene_priority needs mine_scenes"):
        Trainer(None, None, Algo(), 0.99, 16, 4, "/nonexistent", 0, params, save_log=False, scene_frac=0.5, scene_priority=True)
    Algo.world = 2
    with pytest.raises(ValueError, match="mine_scenes runs on one rank"):
        Trainer(None, None, Algo(), 0.99, 16, 4, "/nonexistent", 0, params, save_log=False, rank=0, world=2, scene_frac=0.5, mine_scenes=4,
                scene_priority=True)
