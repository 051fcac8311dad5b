"""Lookahead shield rounds, host side: the two C entry points' declaration, export and host-side refusals, the bindings'
refusals, the reselect rule restated in NumPy on hand-made values, scene A rolled with the oracle alone, joint_shield_stats and the
--shield-rounds flag of test.py — CPU only."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lookahead_np as L  # noqa: E402
import lookahead_rounds_np as R  # noqa: E402

ROOT = os.path.dirname(HERE)
f32 = np.float32
nan = np.nan
FORK, RESELECT = "dgppo_env_team_action_fork_ids", "dgppo_lookahead_reselect"
FAKE = 0x1000                                               # a non-NULL pointer: never dereferenced on the host


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def _fork(lib, cfg, null=(), nu=2, nv=2, n_env=3, n_ids=2, HC=64, carry=True):
    p = lambda name: None if name in null else C.c_void_p(FAKE)
    return lib.dgppo_env_team_action_fork_ids(
        C.byref(cfg), p("agent"), p("goal"), p("obst"), p("hits"), p("a_base"), p("carry") if carry else None, HC, n_env,
        p("env_ids"), n_ids, p("us"), nu, p("vs"), nv, p("agent_out"), p("goal_out"), p("obst_out"), p("hits_out"),
        p("action_out"), p("carry_out"), None)


def _reselect(lib, null=(), K=2, n_ids=1, n=3, nh=2, nu=2, nv=2, margin=0.0, mode=1, cost_st=None):
    p = lambda name: None if name in null else C.c_void_p(FAKE)
    dense = n_ids * n * (1 + nu * nv) * n * nh
    return lib.dgppo_lookahead_reselect(p("cost"), dense if cost_st is None else cost_st, K, n_ids, n, nh, p("env_ids"), p("a_ref"),
                                        p("us"), nu, p("vs"), nv, margin, mode, p("action"), p("index"), p("flag"), p("s"),
                                        p("joint"), p("changed"), None)


def test_entry_points_are_declared_and_exported():
    from dgppo_amd import _native as N
    full = open(os.path.join(ROOT, "include", "dgppo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    lib = N.lib()
    for name in (FORK, RESELECT):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int32
        comment = full[:full.index("int32_t " + name)].rsplit("/*", 1)[1]
        assert "env/base.py" in comment and "The reference ships no runtime filter" in comment, name
    assert len(lib.dgppo_env_team_action_fork_ids.argtypes) == len(lib.dgppo_env_team_action_fork.argtypes) + 2
    assert len(lib.dgppo_lookahead_reselect.argtypes) == 21


def test_fork_ids_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    bad = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    bad.kind = 17
    assert _fork(lib, bad) == -1 and FORK in err() and "unknown env kind" in err()   # dgppo_validate_cfg, under this name
    assert _fork(lib, N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)) == -1
    assert FORK in err() and "VMASReverseTransport" in err()
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    for kw in (dict(nu=0), dict(nv=0), dict(nu=-1)):
        assert _fork(lib, cfg, **kw) == -1 and FORK in err() and "nu and nv" in err(), kw
    assert _fork(lib, cfg, nu=4096, nv=4096) == -1 and FORK in err() and "grid too large" in err()
    for kw in (dict(n_env=-1), dict(n_ids=-1)):
        assert _fork(lib, cfg, **kw) == -1 and FORK in err() and "negative counts" in err(), kw
    assert _fork(lib, cfg, null=("env_ids",), n_env=3, n_ids=2) == -1 and FORK in err() and "without env_ids" in err()
    assert _fork(lib, cfg, n_env=0, n_ids=1) == -1 and FORK in err() and "listed of none" in err()
    assert _fork(lib, cfg, n_env=1 << 20, n_ids=1 << 20, nu=1023, nv=1) == -1 and FORK in err() and "G * n < 2^31" in err()
    assert _fork(lib, cfg, HC=0) == -1 and FORK in err() and "HC" in err()
    everything = ("agent", "goal", "obst", "hits", "a_base", "carry", "us", "vs", "agent_out", "goal_out", "obst_out", "hits_out",
                  "action_out", "carry_out")
    assert _fork(lib, cfg, null=everything, n_ids=0, carry=False) == 0          # nothing to do, nothing is read
    for name in ("agent", "goal", "a_base", "us", "vs", "agent_out", "goal_out", "action_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and "NULL operand" in err(), name
    for name in ("obst", "obst_out", "hits", "hits_out", "carry_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and f"{name} is NULL" in err(), name
    for other in (N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 0), N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)):
        assert _fork(lib, other) == -1 and FORK in err() and "cast rays" in err()


def test_reselect_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    for nh in (0, 4, -1):
        assert _reselect(lib, nh=nh) == -1 and RESELECT in err() and "outside [1, 3]" in err(), nh
    for K in (0, -2):
        assert _reselect(lib, K=K) == -1 and RESELECT in err() and "K must be >= 1" in err(), K
    for mode in (2, -1):
        assert _reselect(lib, mode=mode) == -1 and RESELECT in err() and "mode" in err(), mode
    assert _reselect(lib, margin=float("nan")) == -1 and RESELECT in err() and "margin" in err()
    assert _reselect(lib, cost_st=1 * 3 * 5 * 3 * 2 - 1) == -1 and RESELECT in err() and "step stride" in err()
    for kw in (dict(nu=0), dict(nv=-1)):
        assert _reselect(lib, **kw) == -1 and RESELECT in err() and "nu and nv" in err(), kw
    assert _reselect(lib, nu=4096, nv=4096) == -1 and RESELECT in err() and "grid too large" in err()
    for kw in (dict(n=0), dict(n_ids=-1)):
        assert _reselect(lib, **kw) == -1 and RESELECT in err() and "n_ids" in err(), kw
    assert _reselect(lib, n=4097) == -1 and RESELECT in err() and "4096" in err()
    assert _reselect(lib, n_ids=1 << 20, nu=1023, nv=1) == -1 and RESELECT in err() and "G * n < 2^31" in err()
    for name in ("cost", "a_ref", "us", "vs", "action", "index", "flag", "joint", "changed"):
        assert _reselect(lib, null=(name,)) == -1
        assert RESELECT in err() and "NULL operand" in err(), name
    everything = ("cost", "env_ids", "a_ref", "us", "vs", "action", "index", "flag", "s", "joint", "changed")
    assert _reselect(lib, n_ids=0, null=everything) == 0                                 # no launch


# ---- the bindings ----------------------------------------------------------------------------------------------------------------
def test_bindings_refuse_before_anything_is_launched():
    """host tensors: the env list, the mode and the shapes are looked at first; with everything right the operands are refused for
    not being on the device — either way nothing reaches the library"""
    import torch
    from dgppo_amd import _native as N, ops_env as OE, ops_nn as K
    assert "team_action_fork_ids" in dir(OE) and "lookahead_reselect" in dir(K)
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    B, n, nu, nv, HC = 4, 3, 2, 1, 64
    P = 1 + nu * nv
    ids = np.array([1, 3])
    G = ids.size * n * P
    us, vs = torch.zeros(nu), torch.zeros(nv)
    st, out = OE.State.empty(cfg, B, "cpu"), OE.State.empty(cfg, G, "cpu")
    ok = dict(a_base=torch.zeros(B, n, 2), env_ids=ids, action_out=torch.zeros(G, n, 2), carry=torch.zeros(B * n, HC),
              carry_out=torch.zeros(G * n, HC))

    def fork(st=st, out=out, us=us, vs=vs, **kw):
        a = {**ok, **kw}
        OE.team_action_fork_ids(cfg, st, a["a_base"], a["env_ids"], us, vs, out, a["action_out"], a["carry"], a["carry_out"])
    for kw, match in ((dict(env_ids=np.array([1, B])), r"env_ids outside \[0, 4\)"), (dict(env_ids=np.array([-1, 2])), "env_ids outside"),
                      (dict(env_ids=np.array([[1, 2]])), "env_ids must be a 1-D"), (dict(env_ids=np.array([0.0, 1.0])), "ints"),
                      (dict(env_ids=np.array([0, 1, 2])), "action_out"), (dict(a_base=torch.zeros(B, n + 1, 2)), "a_base"),
                      (dict(action_out=torch.zeros(G - 1, n, 2)), "action_out"), (dict(carry=torch.zeros(B * n + 1, HC)), "carry"),
                      (dict(carry_out=torch.zeros(G * n, HC + 1)), "carry_out"), (dict(carry_out=None), "carry_out"),
                      (dict(out=OE.State.empty(cfg, G + 1, "cpu")), r"out\.agent"),
                      (dict(st=OE.State.empty(cfg, B + 1, "cpu")), "agent"), (dict(us=torch.zeros(0)), "us")):
        with pytest.raises(ValueError, match=match):
            fork(**kw)
    with pytest.raises(ValueError, match="CUDA"):
        fork()
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.team_action_fork_ids(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), st, ok["a_base"], ids, us, vs, out, ok["action_out"])

    nh, K_ = cfg.n_cost, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    sel = dict(cost_tm=torch.zeros(K_, G, n, nh), env_ids=ids, a_ref=torch.zeros(B, n, 2), us=us, vs=vs, margin=0.0, mode=1,
               action=torch.zeros(B, n, 2), index=i32(B, n), flag=i32(B, n), joint=i32(B), changed=i32(B), s=torch.zeros(B, n, P))
    for kw, match in ((dict(env_ids=np.array([1, B])), "env_ids outside"), (dict(env_ids=np.array([2, 2])), "repeats"),
                      (dict(mode=2), "mode"), (dict(margin=float("nan")), "margin"), (dict(cost_tm=torch.zeros(K_, G + 1, n, nh)), "cost_tm"),
                      (dict(cost_tm=torch.zeros(0, G, n, nh)), "K must"), (dict(cost_tm=torch.zeros(K_, G, n, 4)), "n_cost"),
                      (dict(env_ids=None), "cost_tm"), (dict(a_ref=torch.zeros(B, n, 3)), "a_ref"),
                      (dict(action=torch.zeros(B, n)), "action"), (dict(index=i32(B, n + 1)), "index"), (dict(flag=i32(B)), "flag"),
                      (dict(joint=i32(B + 1)), "joint"), (dict(changed=i32(B, 1)), "changed"), (dict(s=torch.zeros(B, n, P + 1)), "s:"),
                      (dict(us=torch.zeros(0)), "us")):
        with pytest.raises(ValueError, match=match):
            K.lookahead_reselect(**{**sel, **kw})
    with pytest.raises(ValueError, match="CUDA"):
        K.lookahead_reselect(**sel)


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------
US, VS = np.array([-0.5, 0.5], f32), np.array([0.0], f32)              # P = 3: candidates 1 and 2 at (-0.5, 0) and (0.5, 0)


def test_reselect_rule_on_hand_made_values():
    """one env, three agents.  Mode 0 commits every pick; mode 1 only the lowest-numbered mover's.  The distance is taken from the
    policy's action, not from the action held; an agent that stays leaves its index alone and gets the flag of what it holds"""
    a_ref = np.array([[[0.4, 0.0], [0.0, 0.0], [7.0, 0.0]]], f32)
    held = np.array([[[-0.5, 0.0], [0.0, 0.0], [7.0, 0.0]]], f32)       # agent 0 holds grid candidate 1 from an earlier round
    index = np.array([[1, 0, 0]], np.int32)
    s = np.array([[[1.0, 1.0, -1.0], [-1.0, -2.0, -2.0], [nan, 2.0, 1.0]]], f32)
    a0, i0, f0, j0, c0 = R.reselect_np(s, None, a_ref, US, VS, 0.0, 0, held, index)
    assert i0.tolist() == [[2, 0, 2]] and f0.tolist() == [[1, 0, 2]] and j0.tolist() == [0] and c0.tolist() == [1]
    np.testing.assert_array_equal(a0, [[[0.5, 0.0], [0.0, 0.0], [0.5, 0.0]]])
    a1, i1, f1, j1, c1 = R.reselect_np(s, None, a_ref, US, VS, 0.0, 1, held, index)
    assert i1.tolist() == [[2, 0, 0]] and f1.tolist() == [[1, 0, 2]] and j1.tolist() == [0] and c1.tolist() == [1]
    np.testing.assert_array_equal(a1, [[[0.5, 0.0], [0.0, 0.0], [1.0, 0.0]]])     # the one that stays is written back clipped
    # nearest to the POLICY's action: both grid candidates admissible, the held action (-0.5, 0) nearer to candidate 1
    s2 = np.array([[[1.0, -1.0, -1.0], [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]]], f32)
    _, i2, f2, j2, c2 = R.reselect_np(s2, None, a_ref, US, VS, 0.0, 1, held, index)
    assert i2.tolist() == [[2, 0, 0]] and f2.tolist() == [[1, 0, 0]] and (j2.tolist(), c2.tolist()) == ([0], [1])
    # nobody moves: rolled; admissible for everyone -> joint 2; agent 0 keeps index 1 and reads flag 1
    s3 = np.full((1, 3, 3), -1.0, f32)
    a3, i3, f3, j3, c3 = R.reselect_np(s3, None, a_ref, US, VS, 0.0, 1, held, index)
    assert i3.tolist() == [[1, 0, 0]] and f3.tolist() == [[1, 0, 0]] and (j3.tolist(), c3.tolist()) == ([2], [0])
    # nobody moves and someone is unsafe with nothing better (every s NaN: the pick is 0) -> joint 1
    s4 = s3.copy()
    s4[0, 1] = nan
    _, i4, f4, j4, c4 = R.reselect_np(s4, None, a_ref, US, VS, 0.0, 0, held, index)
    assert i4.tolist() == [[1, 0, 0]] and f4.tolist() == [[1, 2, 0]] and (j4.tolist(), c4.tolist()) == ([1], [0])
    # a list: the rows of the env that is not listed are kept
    keep = R.reselect_np(s, [1], np.repeat(a_ref, 2, 0), US, VS, 0.0, 0, np.repeat(held, 2, 0), np.repeat(index, 2, 0),
                         flag=np.full((2, 3), -7), joint=np.full(2, -7), changed=np.full(2, -7))
    assert keep[1].tolist() == [[1, 0, 0], [2, 0, 2]] and keep[2].tolist() == [[-7] * 3, [1, 0, 2]]
    assert keep[3].tolist() == [-7, 0] and keep[4].tolist() == [-7, 1]
    np.testing.assert_array_equal(keep[0][0], held[0])


def test_round_zero_is_the_one_shot_rule():
    """mode 0 from A = a_pol, index 0: action, index and flag are rule_np's"""
    rng = np.random.default_rng(5)
    E, n, P = 4, 3, 3
    s = np.where(rng.uniform(size=(E, n, P)) < 0.4, 0.7, -0.7).astype(f32)
    s[rng.uniform(size=s.shape) < 0.1] = nan
    a_pol = rng.uniform(-1.3, 1.3, size=(E, n, 2)).astype(f32)
    for margin in (0.0, 0.75):
        wi, wf, wa = L.rule_np(s, a_pol, US, VS, margin)
        a, i, f, j, c = R.reselect_np(s, None, a_pol, US, VS, margin, 0, a_pol, np.zeros((E, n), np.int32))
        np.testing.assert_array_equal(i, wi)
        np.testing.assert_array_equal(f, wf)
        np.testing.assert_array_equal(a.view(np.uint32), wa.view(np.uint32))
        np.testing.assert_array_equal(c, (wi != 0).any(axis=1))


def test_fork_ids_layout():
    B, n = 3, 2
    us, vs = np.array([0.25, 5.0], f32), np.array([nan], f32)
    agent = np.arange(B * n * 4, dtype=f32).reshape(B, n, 4)
    a_base = np.arange(B * n * 2, dtype=f32).reshape(B, n, 2) + 100
    carry = np.arange(B * n * 3, dtype=f32).reshape(B * n, 3)
    out, action, c = R.fork_ids_np(dict(agent=agent), a_base, [2, 0], us, vs, carry)
    P = 3
    assert out["agent"].shape == (2 * n * P, n, 4) and action.shape == (2 * n * P, n, 2) and c.shape == (2 * n * P * n, 3)
    act = action.view(f32).reshape(2, n, P, n, 2)
    for m, e in enumerate([2, 0]):
        for i in range(n):
            for p in range(P):
                g = (m * n + i) * P + p
                np.testing.assert_array_equal(out["agent"][g].view(f32), agent[e])
                np.testing.assert_array_equal(c.view(f32).reshape(-1, n, 3)[g], carry.reshape(B, n, 3)[e])
                np.testing.assert_array_equal(act[m, i, p, 1 - i], a_base[e, 1 - i])
                np.testing.assert_array_equal(act[m, i, p, i], a_base[e, i] if p == 0 else [us[p - 1], vs[0]])
    all_out, all_action, _ = R.fork_ids_np(dict(agent=agent), a_base, None, us, vs)
    want, want_action, _ = L.fork_np(dict(agent=agent), a_base, us, vs)
    np.testing.assert_array_equal(all_out["agent"], want["agent"])
    np.testing.assert_array_equal(all_action, want_action)


# ---- scene A, by the oracle alone -----------------------------------------------------------------------------------------------------
def test_scene_a_needs_the_rounds():
    """own rows throughout.  Left alone both agents are unsafe within H; round 0 (today's shield) picks candidate 2, (0, -1), for
    both, each admissible on its own; rolled jointly that action is as unsafe as doing nothing; the rounds reach (0, 0) / (0, -1),
    rolled and admissible for both, in the third"""
    us, vs, H = R.SCENE_A_US, R.SCENE_A_VS, R.SCENE_A_H
    cfg, agent, goal, obst = R.scene_a()
    zero = np.zeros((1, 2, 2), f32)
    alone = R.roll_joint(cfg, agent, goal, obst, zero[0], H)
    assert alone.tolist() == [R.SCENE_A_UNSAFE, R.SCENE_A_UNSAFE] and R.SCENE_A_UNSAFE == f32(0.5660001)
    one = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 1)
    assert one["index"].tolist() == [[2, 2]] and one["flag"].tolist() == [[1, 1]]
    assert one["joint"].tolist() == [0] and one["rounds_used"].tolist() == [1]         # not rolled: and it collides
    np.testing.assert_array_equal(one["action"], [[[0.0, -1.0], [0.0, -1.0]]])
    wi, wf, wa = L.rule_np(one["s"], zero, us, vs, 0.0)
    assert wi.tolist() == [[2, 2]] and np.array_equal(wa, one["action"])
    both = R.roll_joint(cfg, agent, goal, obst, one["action"][0], H)
    assert both.tolist() == [R.SCENE_A_UNSAFE, R.SCENE_A_UNSAFE]
    assert ((one["s"] <= -0.5) | (one["s"] >= 0.5)).all()                               # nothing near the threshold
    four = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 4)
    np.testing.assert_array_equal(four["action"], [[[0.0, 0.0], [0.0, -1.0]]])
    assert four["rounds_used"].tolist() == [3] and four["joint"].tolist() == [2] and len(four["trace"]) == 3
    assert four["s"][0, :, 0].tolist() == [R.SCENE_A_SAFE, R.SCENE_A_SAFE] and R.SCENE_A_SAFE == f32(-0.50394225)
    assert four["index"].tolist() == [[5, 2]] and four["flag"].tolist() == [[1, 1]]     # 5 is the grid's (0, 0)
    # round 1 rolled the double dodge as candidate 0 and found it unsafe for both; agent 0, the lowest mover, went back alone
    ids1, s1, a1, i1, f1, j1, c1 = four["trace"][1]
    assert s1[0, :, 0].tolist() == [R.SCENE_A_UNSAFE, R.SCENE_A_UNSAFE] and c1.tolist() == [1] and j1.tolist() == [0]
    np.testing.assert_array_equal(a1, four["action"])
    held = R.roll_joint(cfg, agent, goal, obst, four["action"][0], H)
    assert held.tolist() == [R.SCENE_A_SAFE, R.SCENE_A_SAFE]
    three = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 3)
    assert three["joint"].tolist() == [2] and three["rounds_used"].tolist() == [3]
    two = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 2)
    assert two["joint"].tolist() == [0] and two["rounds_used"].tolist() == [2]          # ran out: held but not rolled


def test_simultaneous_rounds_cycle_in_scene_a():
    """why later rounds let one agent move: with mode 0 in every round both agents return to (0, 0), dodge again, and so on"""
    us, vs = R.SCENE_A_US, R.SCENE_A_VS
    fold = R.scene_a_fold()
    zero = np.zeros((1, 2, 2), f32)
    action, index = zero.copy(), np.zeros((1, 2), np.int32)
    seen = []
    for r in range(4):
        action, index, flag, joint, changed = R.reselect_np(fold([0], action), None, zero, us, vs, 0.0, 0, action, index)
        seen.append(action[0].tolist())
        assert changed.tolist() == [1]
    dodge, back = [[0.0, -1.0], [0.0, -1.0]], [[0.0, 0.0], [0.0, 0.0]]
    assert seen == [dodge, back, dodge, back]


# ---- the statistics ----------------------------------------------------------------------------------------------------------------
def test_joint_shield_stats():
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import JointLookaheadShieldLog, LookaheadShieldLog
    assert JointLookaheadShieldLog._fields == LookaheadShieldLog._fields + ("joint", "rounds_used", "rounds")
    joint = np.array([[2, 2, 0, 1], [2, 2, 2, 2]], np.int32)
    used = np.array([[1, 2, 3, 2], [1, 1, 1, 1]], np.int32)
    z = np.zeros((2, 4, 2, 2), f32)
    log = JointLookaheadShieldLog(z, z, np.zeros((2, 4, 2), np.int32), np.zeros((2, 4, 2), np.int32), np.zeros((2, 4, 2, 3), f32),
                                  US, VS, 0.0, 4, joint, used, 3)
    got = EV.joint_shield_stats(log)
    assert sorted(got) == ["joint_unrolled_frac", "joint_verified_frac", "mean_rounds"]
    np.testing.assert_array_equal(got["joint_verified_frac"], [0.5, 1.0])
    np.testing.assert_array_equal(got["joint_unrolled_frac"], [0.25, 0.0])
    np.testing.assert_array_equal(got["mean_rounds"], [2.0, 1.0])
    assert sorted(EV.shield_stats(log)) == ["infeasible_frac", "intervention_frac", "mean_deviation"]    # unchanged, and takes it
    with pytest.raises(ValueError, match="joint_shield_stats"):
        EV.joint_shield_stats(log._replace(rounds_used=used[:, :3]))


# ---- test.py ---------------------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_shield_rounds_flag():
    mod = _load_test_py()
    assert mod.ROUNDS_FLAGS == [(("--shield-rounds",), "int", 1)]
    ap = mod.build_parser()
    assert ap.parse_args(["--path", "x"]).shield_rounds == 1
    args = ap.parse_args(["--path", "x", "--shield", "--shield-horizon", "6", "--shield-rounds", "3"])
    assert args.shield and args.shield_horizon == 6 and args.shield_rounds == 3
    assert "--shield-rounds" in mod.__doc__ and "joint_unrolled_frac" in mod.__doc__


def test_cli_refusals():
    """before anything is loaded: the path does not exist"""
    mod = _load_test_py()
    with pytest.raises(SystemExit, match=r"--shield-rounds needs --shield and --shield-horizon"):
        mod.main(["--path", "/nonexistent/run", "--shield-rounds", "3"])
    with pytest.raises(SystemExit, match=r"--shield-rounds needs --shield and --shield-horizon"):
        mod.main(["--path", "/nonexistent/run", "--shield", "--shield-rounds", "3"])
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit, match="--shield-rounds must be >= 1"):
            mod.main(["--path", "/nonexistent/run", "--shield", "--shield-horizon", "4", "--shield-rounds", bad])
