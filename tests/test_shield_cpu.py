"""Barrier shield, host side: shield_stats on hand-made logs, the --shield flags of test.py, and the two C entry points'
declaration, export and host-side refusals — CPU only."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from dgppo_amd.trainer import evaluate as EV
from dgppo_amd.trainer.data import ShieldLog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FIELDS = ("policy_action", "action", "index", "flag", "h", "Vh", "us", "vs", "margin", "alpha", "dt")


def _log(flag, action, policy_action):
    flag = np.asarray(flag, np.int32)
    B, T, n = flag.shape
    return ShieldLog(np.asarray(policy_action, f32), np.asarray(action, f32), np.zeros_like(flag), flag,
                     np.zeros((B, T, n, 2), f32), np.zeros((B, T, n, 2), f32), np.array([0.0], f32), np.array([0.0], f32), 0.0,
                     10.0, 0.03)


def test_shield_log_record():
    assert ShieldLog._fields == FIELDS


def test_shield_stats_counts():
    """2 episodes of 2 steps and 2 agents, every number known in advance: episode 0 keeps 2 of its 4 actions, replaces one by an
    admissible candidate (moved by the 3-4-5 triangle scaled to 0.5) and finds nothing for one (moved by 1 along u); episode 1
    keeps everything"""
    flag = [[[0, 1], [2, 0]], [[0, 0], [0, 0]]]
    pol = np.zeros((2, 2, 2, 2), f32)
    act = np.zeros((2, 2, 2, 2), f32)
    pol[0, 0, 1] = [0.1, -0.2]
    act[0, 0, 1] = [0.4, 0.2]                              # |(0.3, 0.4)| = 0.5
    pol[0, 1, 0] = [-1.0, 0.5]
    act[0, 1, 0] = [0.0, 0.5]                              # 1.0
    pol[1] = act[1] = 0.25
    got = EV.shield_stats(_log(flag, act, pol))
    assert sorted(got) == ["infeasible_frac", "intervention_frac", "mean_deviation"]
    np.testing.assert_array_equal(got["intervention_frac"], [0.5, 0.0])
    np.testing.assert_array_equal(got["infeasible_frac"], [0.25, 0.0])
    np.testing.assert_allclose(got["mean_deviation"], [(0.5 + 1.0) / 4, 0.0], rtol=0, atol=1e-7)


def test_shield_stats_clips_like_the_environment_and_checks_shapes():
    """a policy action outside the box counts as its clipped value: (3, 0) executed as (1, 0) has not moved"""
    pol = np.array([[[[3.0, 0.0]]]], f32)
    act = np.array([[[[1.0, 0.0]]]], f32)
    got = EV.shield_stats(_log([[[0]]], act, pol))
    assert got["mean_deviation"].tolist() == [0.0] and got["intervention_frac"].tolist() == [0.0]
    with pytest.raises(ValueError, match="flag"):
        EV.shield_stats(_log([[[0]]], act, pol)._replace(flag=np.zeros((1, 1), np.int32)))
    with pytest.raises(ValueError, match="action"):
        EV.shield_stats(_log([[[0]]], act, pol)._replace(action=np.zeros((1, 1, 2, 2), f32)))


# ---- test.py ---------------------------------------------------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_shield_flags():
    mod = _load_test_py()
    assert mod.SHIELD_FLAGS == [(("--shield",), "flag", False), (("--shield-grid",), "int", 8), (("--shield-margin",), "float", 0.0)]
    assert mod.ACTION_FLAGS == [(("--action-landscape",), "int", None)]
    assert mod.COST_FLAGS == [(("--cost-landscape",), "int", None)] and len(mod.FLAGS) == 18
    ap = mod.build_parser()
    args = ap.parse_args(["--path", "x"])
    assert args.shield is False and args.shield_grid == 8 and args.shield_margin == 0.0 and args.action_landscape is None
    args = ap.parse_args(["--path", "x", "--shield", "--shield-grid", "5", "--shield-margin", "0.25", "--no-video"])
    assert args.shield is True and args.shield_grid == 5 and args.shield_margin == 0.25 and args.no_video


def test_cli_refuses_a_stochastic_shield():
    """before anything is loaded: the path does not exist"""
    with pytest.raises(SystemExit, match="--shield --stochastic"):
        _load_test_py().main(["--path", "/nonexistent/run", "--shield", "--stochastic"])


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
TEAM, SELECT = "dgppo_graph_feats_team_action_sweep", "dgppo_shield_select"
FAKE = 0x1000                                               # a non-NULL pointer: never dereferenced on the host


def _team(lib, cfg, null=None, efeat=FAKE, Fp=8, nu=2, nv=2, n_env=1):
    p = lambda name: None if name == null else C.c_void_p(FAKE)
    return lib.dgppo_graph_feats_team_action_sweep(
        C.byref(cfg), p("agent"), p("next_agent"), p("goal"), p("obst"), p("next_hits"), p("a_pol"), C.c_int32(n_env), p("us"),
        C.c_int32(nu), p("vs"), C.c_int32(nv), p("Xa"), p("Xo"), C.c_void_p(efeat), p("emask"), C.c_int32(Fp), None)


def _select(lib, null=None, n_env=1, n=3, nh=2, nu=2, nv=2, dt=0.03, alpha=10.0, margin=0.0):
    p = lambda name: None if name == null else C.c_void_p(FAKE)
    return lib.dgppo_shield_select(p("Vh_next"), p("Vh_t"), p("a_pol"), C.c_int32(n_env), C.c_int32(n), C.c_int32(nh), p("us"),
                                   C.c_int32(nu), p("vs"), C.c_int32(nv), C.c_float(dt), C.c_float(alpha), C.c_float(margin),
                                   p("action"), p("index"), p("flag"), p("h"), None)


def test_entry_points_are_declared_and_exported():
    from dgppo_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgppo_hip.h")).read(), flags=re.S)
    lib = N.lib()
    for name in (TEAM, SELECT):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name


def test_team_sweep_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    assert _team(lib, N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0)) == -1
    assert TEAM in err() and "VMASReverseTransport" in err()
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    for name in ("agent", "next_agent", "goal", "a_pol", "us", "vs", "Xa", "emask"):
        assert _team(lib, cfg, null=name) == -1
        assert TEAM in err() and "NULL operand" in err(), name
    assert _team(lib, cfg, null="Xo") == -1 and "Xo is NULL" in err()
    assert _team(lib, cfg, null="next_hits") == -1 and "next_hits is NULL" in err()
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 3, 3)
    assert _team(lib, mpe, null="obst") == -1 and "obst is NULL" in err()
    assert _team(lib, cfg, efeat=FAKE + 8) == -1 and TEAM in err() and "16-byte aligned" in err()
    assert _team(lib, cfg, Fp=cfg.node_dim - 1) == -1 and "Fp" in err()
    for kw in (dict(nu=0), dict(nv=0), dict(n_env=-1)):
        assert _team(lib, cfg, **kw) == -1 and "nu and nv" in err(), kw
    assert _team(lib, cfg, nu=4096, nv=4096) == -1 and "grid too large" in err()
    assert _team(lib, cfg, n_env=0) == 0                    # nothing to do: no launch


def test_shield_select_refuses_on_the_host():
    from dgppo_amd import _native as N
    lib = N.lib()
    err = lambda: lib.dgppo_last_error().decode()
    for name in ("Vh_next", "Vh_t", "a_pol", "us", "vs", "action", "index", "flag"):
        assert _select(lib, null=name) == -1
        assert SELECT in err() and "NULL operand" in err(), name
    for kw in (dict(nu=0), dict(nv=-1)):
        assert _select(lib, **kw) == -1 and "nu and nv" in err(), kw
    for kw in (dict(n=0), dict(nh=0), dict(n_env=-1)):
        assert _select(lib, **kw) == -1 and "n_env" in err(), kw
    for kw in (dict(dt=0.0), dict(dt=float("nan")), dict(alpha=float("nan")), dict(margin=float("nan"))):
        assert _select(lib, **kw) == -1 and "dt must be" in err(), kw
    assert _select(lib, nu=4096, nv=4096) == -1 and "grid too large" in err()
    assert _select(lib, n_env=0) == 0                       # nothing to do: no launch


def test_bindings_refuse_host_tensors():
    """the Python bindings check their operands before the library is called: axes and operands that are not CUDA tensors"""
    import torch
    from dgppo_amd import _native as N, ops_nn as K
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 3, 2)
    ax = torch.zeros(2)
    z = torch.zeros(1, 3, 4)
    with pytest.raises(ValueError, match="graph_feats_team_action_sweep: us"):
        K.graph_feats_team_action_sweep(cfg, z, z, z, None, None, z, ax, ax, z, z, z, z, 8)
    with pytest.raises(ValueError, match="shield_select: us"):
        K.shield_select(z, z, z, ax, ax, 0.03, 10.0, 0.0, z, z, z)
    with pytest.raises(ValueError, match="VMASReverseTransport"):
        K.graph_feats_team_action_sweep(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), z, z, z, None, None, z, ax, ax, z, z, z, z, 8)
