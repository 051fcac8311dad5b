"""The compiled instances of the one-launch rollout step (the INST list of csrc/env_wave.hip up to ACT_MAX_NA agents, as
dgppo_env_act_step_feats_supported reports them: host code, no device needed) against INSTANCES of tests/test_act_step_gpu.py,
the list every kernel-level test of that launch is parametrised over.  An instance added to the kernel without a line there,
or a line there whose instance is gone, fails here by name."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_act_step_gpu import FP, H, INSTANCES  # noqa: E402

N_AGENTS, N_OBS = range(1, 17), range(0, 9)


def _supported(cfg, fp, h):
    from dgppo_amd import _native as N
    return bool(N.lib().dgppo_env_act_step_feats_supported(C.byref(cfg), C.c_int32(fp), C.c_int32(h)))


def _sweep():
    """-> {(kind name, n, n_obs): cfg} of every non-VMAS configuration make_env_cfg builds as asked"""
    from dgppo_amd import _native as N
    out = {}
    for name, kind in N.ENV_KINDS.items():
        if kind == N.VMAS_REVERSE_TRANSPORT:
            continue
        for n in N_AGENTS:
            for n_obs in N_OBS:
                try:
                    cfg = N.make_env_cfg(kind, n, n_obs)
                except (ValueError, AssertionError):
                    continue
                if (cfg.kind, cfg.n_agents, cfg.n_obs) != (kind, n, n_obs):      # a kind that fixes its own obstacle count
                    continue
                out[(name, n, n_obs)] = cfg
    return out


def test_supported_configurations_are_exactly_the_tested_instances():
    assert (FP, H) == (8, 3)
    assert len(set(INSTANCES)) == len(INSTANCES), "INSTANCES lists a configuration twice"
    cfgs = _sweep()
    assert len(cfgs) > 1000                                              # the sweep is not vacuous
    have = {k for k, cfg in cfgs.items() if _supported(cfg, FP, H)}
    want = set(INSTANCES)
    untested, gone = sorted(have - want), sorted(want - have)
    assert not untested, f"act-step instances that no test of tests/test_act_step_gpu.py launches (add them to INSTANCES): {untested}"
    assert not gone, f"INSTANCES of tests/test_act_step_gpu.py names configurations without an act-step instance: {gone}"
    for k in sorted(have):                                               # the epilogues are written for Fp = 8, H = 3 alone
        assert not _supported(cfgs[k], 12, 3), f"{k}: Fp = 12 reported as supported"
        assert not _supported(cfgs[k], 8, 2), f"{k}: H = 2 reported as supported"


def test_vmas_and_null_are_not_supported():
    from dgppo_amd import _native as N
    assert not _supported(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), FP, H)
    assert N.lib().dgppo_env_act_step_feats_supported(None, C.c_int32(FP), C.c_int32(H)) == 0
