"""Lookahead shield, host side: the selection rule restated in NumPy on hand-made values, the fork's layout, the hand-made scene
of the GPU test rolled with the oracle alone, the two C entry points' declaration, export and host-side refusals, the bindings'
shape checks, the --shield-horizon flag of test.py and shield_stats on a LookaheadShieldLog — CPU only."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import LookaheadShieldLog

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lookahead_np as L  # noqa: E402

ROOT = os.path.dirname(HERE)
f32 = np.float32
nan = np.nan
US, VS = np.array([-0.5, 0.5], f32), np.array([0.0], f32)          # P = 3: candidates 1 and 2 at distance 0.5 of (0, 0)
# (name, s [P], margin, a_pol, (index, flag)): shared with the GPU test, which holds the kernel to the same answers
B_POL = [0.2, 0.0]
HAND_CASES = [
    ("candidate 0 admissible", [-1.0, -3.0, -3.0], 0.0, [0.0, 0.0], (0, 0)),
    ("distance tie goes to the lowest index", [1.0, -1.0, -1.0], 0.0, [0.0, 0.0], (1, 1)),
    ("the nearest wins", [1.0, -1.0, -1.0], 0.0, B_POL, (2, 1)),
    ("the only admissible one", [1.0, -1.0, 2.0], 0.0, B_POL, (1, 1)),
    ("nothing admissible, tie", [3.0, 2.0, 2.0], 0.0, [0.0, 0.0], (1, 2)),
    ("nothing admissible", [3.0, 4.0, 2.0], 0.0, [0.0, 0.0], (2, 2)),
    ("a NaN candidate", [1.0, -1.0, nan], 0.0, B_POL, (1, 1)),
    ("a NaN policy candidate", [nan, 2.0, 1.0], 0.0, [0.0, 0.0], (2, 2)),
    ("all NaN", [nan, nan, nan], 0.0, [0.0, 0.0], (0, 2)),
    ("margin below the value", [-0.6, -1.0, -1.0], 0.5, [0.0, 0.0], (0, 0)),
    ("margin above the value", [-0.6, -1.0, -1.0], 0.75, [0.0, 0.0], (1, 1)),
    ("margin above every value", [-0.6, -0.7, -0.8], 0.9, [0.0, 0.0], (2, 2)),
    ("the value itself is admissible", [-0.5, 1.0, 1.0], 0.5, [0.0, 0.0], (0, 0)),
    ("kept outside the box", [-1.0, -3.0, -3.0], 0.0, [7.0, 0.0], (0, 0)),
    ("replaced outside the box", [1.0, -1.0, -1.0], 0.0, [7.0, 0.0], (2, 1)),
]


@pytest.mark.parametrize("name,s,margin,a_pol,want", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_rule_on_hand_made_values(name, s, margin, a_pol, want):
    index, flag, action = L.rule_np(np.array([s], f32), np.array([a_pol], f32), US, VS, margin)
    assert (int(index[0]), int(flag[0])) == want
    cand = L.clip(L.candidates(np.array(a_pol, f32), US, VS))
    np.testing.assert_array_equal(action[0], cand[want[0]])
    assert np.abs(action).max() <= 1.0                                  # what is executed is clipped


def test_fold_is_the_own_row_maximum():
    """E = 2, n = 2, P = 3, K = 2, nh = 2: the largest word of the agent's own row wins, another agent's row never shows, a NaN in
    the own row propagates and one elsewhere does not"""
    E, n, P, K, nh = 2, 2, 3, 2, 2
    cost = np.full((K, E * n * P, n, nh), -1.0, f32)
    g = lambda e, i, p: (e * n + i) * P + p
    cost[1, g(0, 1, 2), 1, 0] = 0.75
    cost[0, g(0, 1, 2), 0, 1] = 9.0                                    # agent 0's row of agent 1's what-if env
    cost[0, g(1, 0, 1), 0, 1] = nan
    cost[1, g(1, 1, 0), 0, 0] = nan                                    # not the own row
    s = L.fold_np(cost, E, n, P)
    assert s.shape == (E, n, P) and s.dtype == f32
    want = np.full((E, n, P), -1.0, f32)
    want[0, 1, 2] = 0.75
    want[1, 0, 1] = nan
    np.testing.assert_array_equal(s, want)


def test_fork_layout():
    """B = 2, n = 2, a 2 x 1 grid: env (e * n + i) * P + p copies env e, and only row i of its action is the candidate"""
    B, n = 2, 2
    us, vs = np.array([0.25, 5.0], f32), np.array([nan], f32)          # copied as words: nothing is clipped, a NaN stays
    agent = np.arange(B * n * 4, dtype=f32).reshape(B, n, 4)
    a_pol = np.array([[[1.0, 2.0], [3.0, 4.0]], [[-7.0, nan], [0.5, 0.5]]], f32)
    carry = np.arange(B * n * 3, dtype=f32).reshape(B * n, 3)
    out, action, c = L.fork_np(dict(agent=agent), a_pol, us, vs, carry)
    P = 3
    assert out["agent"].shape == (B * n * P, n, 4) and action.shape == (B * n * P, n, 2) and c.shape == (B * n * P * n, 3)
    act = action.view(f32).reshape(B, n, P, n, 2)
    for e in range(B):
        for i in range(n):
            for p in range(P):
                g = (e * n + i) * P + p
                np.testing.assert_array_equal(out["agent"][g].view(f32), agent[e])
                np.testing.assert_array_equal(c.view(f32).reshape(-1, n, 3)[g], carry.reshape(B, n, 3)[e])
                np.testing.assert_array_equal(act[e, i, p, 1 - i], a_pol[e, 1 - i])
                np.testing.assert_array_equal(act[e, i, p, i], a_pol[e, i] if p == 0 else [us[p - 1], vs[0]])


@pytest.mark.parametrize("mover", [0, 1])
def test_the_hand_made_scene_is_not_trivial(mover):
    """what the GPU test relies on, by the oracle alone: left alone the mover becomes unsafe within the horizon, some grid action
    keeps it safe, and no value sits near the threshold (every cost is <= -0.5 or >= 0.5, lidar_env/base.py:203-205)"""
    s = L.scene_oracle(mover)
    assert s.shape == (1, 2, 10) and np.isfinite(s).all()
    assert s[0, mover, 0] >= 0.5
    assert (s[0, mover, 1:] <= -0.5).any()
    assert ((s <= -0.5) | (s >= 0.5)).all()
    assert (s[0, 1 - mover] <= -0.5).all()
    index, flag, action = L.rule_np(s, np.zeros((1, 2, 2), f32), L.SCENE_US, L.SCENE_VS, 0.0)
    assert flag[0, mover] == 1 and flag[0, 1 - mover] == 0 and index[0, 1 - mover] == 0
    assert action[0, mover].tolist() == [-1.0, 0.0]                     # the brake nearest to (0, 0)


# ---- the record and its statistics -----------------------------------------------------------------------------------------------
def test_shield_stats_takes_a_lookahead_log():
    assert LookaheadShieldLog._fields == ("policy_action", "action", "index", "flag", "s", "us", "vs", "margin", "horizon")
    flag = np.array([[[0, 1], [2, 0]], [[0, 0], [0, 0]]], np.int32)
    pol = np.zeros((2, 2, 2, 2), f32)
    act = np.zeros((2, 2, 2, 2), f32)
    pol[0, 0, 1], act[0, 0, 1] = [0.1, -0.2], [0.4, 0.2]                # |(0.3, 0.4)| = 0.5
    pol[0, 1, 0], act[0, 1, 0] = [-3.0, 0.5], [0.0, 0.5]                # clipped to -1 first: 1.0
    log = LookaheadShieldLog(pol, act, np.zeros_like(flag), flag, np.zeros((2, 2, 2, 3), f32), US, VS, 0.0, 4)
    got = EV.shield_stats(log)
    np.testing.assert_array_equal(got["intervention_frac"], [0.5, 0.0])
    np.testing.assert_array_equal(got["infeasible_frac"], [0.25, 0.0])
    np.testing.assert_allclose(got["mean_deviation"], [(0.5 + 1.0) / 4, 0.0], rtol=0, atol=1e-7)


# ---- test.py ---------------------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_shield_horizon_flag():
    mod = _load_test_py()
    assert mod.LOOKAHEAD_FLAGS == [(("--shield-horizon",), "int", 0)]
    ap = mod.build_parser()
    assert ap.parse_args(["--path", "x"]).shield_horizon == 0
    args = ap.parse_args(["--path", "x", "--shield", "--shield-horizon", "6", "--shield-grid", "3", "--shield-margin", "0.1"])
    assert args.shield and args.shield_horizon == 6 and args.shield_grid == 3 and args.shield_margin == 0.1
    assert "--shield-horizon" in mod.__doc__ and "collect_lookahead_shielded" in mod.__doc__


def test_cli_refusals():
    """before anything is loaded: the path does not exist"""
    mod = _load_test_py()
    with pytest.raises(SystemExit, match=r"--shield-horizon.*--shield\b"):
        mod.main(["--path", "/nonexistent/run", "--shield-horizon", "4"])
    with pytest.raises(SystemExit, match="--shield-horizon"):
        mod.main(["--path", "/nonexistent/run", "--shield", "--shield-horizon", "-1"])
    with pytest.raises(SystemExit, match="--shield-horizon"):
        mod.main(["--path", "/nonexistent/run", "--shield-horizon", "-2"])
    with pytest.raises(SystemExit, match="--shield --stochastic"):
        mod.main(["--path", "/nonexistent/run", "--shield", "--shield-horizon", "4", "--stochastic"])


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
FORK, SELECT = "dgppo_env_team_action_fork", "dgppo_lookahead_select"
FAKE = 0x1000                                               # a non-NULL pointer: never dereferenced on the host


def _fork(lib, cfg, null=(), nu=2, nv=2, n_env=1, HC=64, carry=True):
    p = lambda name: None if name in null else C.c_void_p(FAKE)
    return lib.dgppo_env_team_action_fork(
        C.byref(cfg), p("agent"), p("goal"), p("obst"), p("hits"), p("a_pol"), p("carry") if carry else None, HC, n_env, p("us"),
        nu, p("vs"), nv, p("agent_out"), p("goal_out"), p("obst_out"), p("hits_out"), p("action_out"), p("carry_out"), None)


def _select(lib, null=(), K=2, n_env=1, n=3, nh=2, nu=2, nv=2, margin=0.0, cost_st=None):
    p = lambda name: None if name in null else C.c_void_p(FAKE)
    dense = n_env * n * (1 + nu * nv) * n * nh
    return lib.dgppo_lookahead_select(p("cost"), dense if cost_st is None else cost_st, K, n_env, n, nh, p("a_pol"), p("us"), nu,
                                      p("vs"), nv, margin, p("action"), p("index"), p("flag"), p("s"), None)


def test_entry_points_are_declared_and_exported():
    from dgppo_amd import _native as N
    full = open(os.path.join(ROOT, "include", "dgppo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    lib = N.lib()
    for name in (FORK, SELECT):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int32
        comment = full[:full.index("int32_t " + name)].rsplit("/*", 1)[1]
        assert "env/base.py" in comment and "The reference ships no runtime filter" in comment, name
    assert "lidar_env/base.py:203-205" in full[:full.index("int32_t " + SELECT)].rsplit("/*", 1)[1]


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
    for kw in (dict(nu=0), dict(nv=0), dict(nu=-1)):
        assert _fork(lib, cfg, **kw) == -1 and FORK in err() and "nu and nv" in err(), kw
    assert _fork(lib, cfg, nu=4096, nv=4096) == -1 and FORK in err() and "grid too large" in err()
    assert _fork(lib, cfg, n_env=-1) == -1 and FORK in err() and "negative counts" in err()
    # G * n = n_env * n * P * n: 2^20 envs of 3 agents and 1 + 1023 * 1 candidates are 9 * 2^30 rows
    assert _fork(lib, cfg, n_env=1 << 20, nu=1023, nv=1) == -1 and FORK in err() and "G * n < 2^31" in err()
    assert _fork(lib, cfg, HC=0) == -1 and FORK in err() and "HC" in err()
    everything = ("agent", "goal", "obst", "hits", "a_pol", "carry", "us", "vs", "agent_out", "goal_out", "obst_out", "hits_out",
                  "action_out", "carry_out")
    assert _fork(lib, cfg, null=everything, n_env=0, carry=False) == 0          # nothing to do, nothing is read
    for name in ("agent", "goal", "a_pol", "us", "vs", "agent_out", "goal_out", "action_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and "NULL operand" in err(), name
    for name in ("obst", "obst_out", "hits", "hits_out", "carry_out"):
        assert _fork(lib, cfg, null=(name,)) == -1
        assert FORK in err() and f"{name} is NULL" in err(), name
    # hits / hits_out exactly where the kind casts rays: a LiDAR kind without obstacles and an MPE kind take none
    for other in (N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 0), N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)):
        assert _fork(lib, other) == -1 and FORK in err() and "cast rays" in err()
        assert _fork(lib, other, null=("hits",)) == -1 and "cast rays" in err()
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    assert _fork(lib, mpe, null=("hits", "hits_out", "obst")) == -1 and FORK in err() and "obst is NULL" in err()
    assert _fork(lib, mpe, null=("hits", "hits_out", "obst_out")) == -1 and "obst_out is NULL" in err()


def test_select_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    for nh in (0, 4, -1):
        assert _select(lib, nh=nh) == -1 and SELECT in err() and "outside [1, 3]" in err(), nh
    for K in (0, -2):
        assert _select(lib, K=K) == -1 and SELECT in err() and "K must be >= 1" in err(), K
    assert _select(lib, margin=float("nan")) == -1 and SELECT in err() and "margin" in err()
    assert _select(lib, cost_st=1 * 3 * 5 * 3 * 2 - 1) == -1 and SELECT in err() and "step stride" in err()
    for kw in (dict(nu=0), dict(nv=-1)):
        assert _select(lib, **kw) == -1 and SELECT in err() and "nu and nv" in err(), kw
    assert _select(lib, nu=4096, nv=4096) == -1 and SELECT in err() and "grid too large" in err()
    for kw in (dict(n=0), dict(n_env=-1)):
        assert _select(lib, **kw) == -1 and SELECT in err() and "n_env" in err(), kw
    assert _select(lib, n_env=1 << 20, nu=1023, nv=1) == -1 and SELECT in err() and "G * n < 2^31" in err()
    for name in ("cost", "a_pol", "us", "vs", "action", "index", "flag"):
        assert _select(lib, null=(name,)) == -1
        assert SELECT in err() and "NULL operand" in err(), name
    assert _select(lib, n_env=0, null=("cost", "a_pol", "us", "vs", "action", "index", "flag", "s")) == 0   # no launch


# ---- the bindings ----------------------------------------------------------------------------------------------------------------
def test_bindings_raise_on_wrong_shapes_before_anything_else():
    """host tensors: a wrong shape is named first; with every shape right the operands are refused for not being on the device —
    either way nothing reaches the library"""
    import torch
    from dgppo_amd import _native as N, ops_env as OE, ops_nn as K
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    B, n, nu, nv, HC = 2, 3, 2, 1, 64
    P = 1 + nu * nv
    G = B * n * P
    us, vs = torch.zeros(nu), torch.zeros(nv)
    st, out = OE.State.empty(cfg, B, "cpu"), OE.State.empty(cfg, G, "cpu")
    ok = dict(a_pol=torch.zeros(B, n, 2), action_out=torch.zeros(G, n, 2), carry=torch.zeros(B * n, HC),
              carry_out=torch.zeros(G * n, HC))

    def fork(st=st, out=out, us=us, vs=vs, **kw):
        a = {**ok, **kw}
        OE.team_action_fork(cfg, st, a["a_pol"], us, vs, out, a["action_out"], a["carry"], a["carry_out"])
    for kw, match in ((dict(a_pol=torch.zeros(B, n + 1, 2)), "a_pol"), (dict(action_out=torch.zeros(G - 1, n, 2)), "action_out"),
                      (dict(carry=torch.zeros(B * n + 1, HC)), "carry"), (dict(carry_out=torch.zeros(G * n, HC + 1)), "carry_out"),
                      (dict(carry_out=None), "carry_out"), (dict(out=OE.State.empty(cfg, G + 1, "cpu")), r"out\.agent"),
                      (dict(st=OE.State.empty(cfg, B + 1, "cpu")), "agent"), (dict(us=torch.zeros(0)), "us"),
                      (dict(vs=torch.zeros(2, 2)), "vs")):
        with pytest.raises(ValueError, match=match):
            fork(**kw)
    no_hits = OE.State({"agent": st.agent}, st.env)
    with pytest.raises(ValueError, match="hits"):
        fork(st=no_hits)
    with pytest.raises(ValueError, match="CUDA"):
        fork()
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        OE.team_action_fork(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), st, ok["a_pol"], us, vs, out, ok["action_out"])

    nh, K_ = cfg.n_cost, 3
    sel = dict(cost_tm=torch.zeros(K_, G, n, nh), a_pol=torch.zeros(B, n, 2), us=us, vs=vs, margin=0.0, action=torch.zeros(B, n, 2),
               index=torch.zeros(B, n, dtype=torch.int32), flag=torch.zeros(B, n, dtype=torch.int32), s=torch.zeros(B, n, P))
    for kw, match in ((dict(cost_tm=torch.zeros(K_, G + 1, n, nh)), "cost_tm"), (dict(cost_tm=torch.zeros(0, G, n, nh)), "K must"),
                      (dict(cost_tm=torch.zeros(K_, G, n, 4)), "n_cost"), (dict(cost_tm=torch.zeros(G, n, nh)), "cost_tm"),
                      (dict(a_pol=torch.zeros(B, n, 3)), "a_pol"), (dict(action=torch.zeros(B, n)), "action"),
                      (dict(index=torch.zeros(B, n + 1, dtype=torch.int32)), "index"),
                      (dict(flag=torch.zeros(B, dtype=torch.int32)), "flag"), (dict(s=torch.zeros(B, n, P + 1)), "s:"),
                      (dict(us=torch.zeros(0)), "us"), (dict(margin=float("nan")), "margin")):
        with pytest.raises(ValueError, match=match):
            K.lookahead_select(**{**sel, **kw})
    with pytest.raises(ValueError, match="CUDA"):
        K.lookahead_select(**sel)
