"""dgppo_env_act_step_feats — head sampling, env.step and the next state's graph features and layer-0 queries in one launch —
against the four launches it replaces (dgppo_policy_head -> dgppo_env_step -> dgppo_graph_feats -> dgppo_dense_fwd) on copies of
the same inputs.  Convention: every output compared with torch.equal on the raw bits (-0.0 differs from 0.0, NaNs must sit in the
same places with the same bits); every output buffer lies between sentinel words that must come back untouched."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import env_np as E

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import env_edge_scenes as S  # noqa: E402
from test_env_edges_gpu import _ref  # noqa: E402  (the scene catalogue and its pre-step hit points, computed once per config)
from test_env_gpu import _mk, _to  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable"),
              pytest.mark.filterwarnings("ignore:invalid value encountered")]
f32 = np.float32
# every compiled instance of the act-step kernel (the INST list of csrc/env_wave.hip up to ACT_MAX_NA agents):
# tests/test_act_step_instances_cpu.py holds this list to what dgppo_env_act_step_feats_supported answers
INSTANCES = [("LidarSpread", 8, 3), ("LidarTarget", 8, 3), ("LidarSpread", 4, 2), ("LidarTarget", 4, 2),
             ("LidarBicycleTarget", 4, 3)]
FP, H = 8, 3
GUARD = 64                 # sentinel floats either side of an output (a multiple of 4: the outputs stay 16-byte aligned)
SENTINEL = 0x7FC0BEEF      # as a float: a quiet NaN with a payload no kernel produces
OUTS = ("action", "log_pi", "next_agent", "next_hits", "reward", "cost", "Xa", "Xo", "efeat", "emask", "qt0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(shape, dev):
    """an uninitialised-looking tensor of `shape` inside a flat buffer with GUARD sentinel words before and after it"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + numel].view(torch.float32).view(*shape)


def _guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == SENTINEL).all())


def _shapes(cfg, B):
    n, S_ = cfg.n_agents, cfg.fan_in
    return dict(action=(B, n, 2), log_pi=(B, n), next_agent=(B, n, cfg.state_dim), next_hits=(B, n, cfg.top_k, 2),
                reward=(B,), cost=(B, n, cfg.n_cost), Xa=(B * n, FP), Xo=(B * (cfg.num_nodes - 1 - n), FP),
                efeat=(B * n, S_, 4), emask=(B * n, S_), qt0=(B * n, H * FP))


def _weights(dev, seed=5):
    rng = np.random.default_rng(seed)
    return _to(rng.normal(0, 1, (FP, H * FP)).astype(f32), dev), _to(rng.normal(0, 1, (H * FP,)).astype(f32), dev)


def _four_launches(cfg, st, ms, eps, Mcat, cvec):
    """today's route: policy_head -> OE.step -> GraphFeats.compute_record -> dense_fwd"""
    from dgppo_amd import nets, ops_env as OE, ops_nn as K
    dev = ms.device
    B, n = st.step["agent"].shape[0], cfg.n_agents
    out = {k: torch.empty(*s, device=dev) for k, s in _shapes(cfg, B).items() if k in ("action", "log_pi", "reward", "cost", "qt0")}
    if eps is not None:
        K.policy_head(ms, eps, None, out["action"].view(B * n, 2), out["log_pi"].view(B * n), None, n, 0)
    else:
        K.policy_head(ms, None, None, out["action"].view(B * n, 2), None, None, n, 1)
        del out["log_pi"]
    nst = st.like()
    OE.step(cfg, st, out["action"], nst, out["reward"], out["cost"])
    feats = nets.GraphFeats(cfg, B, nets.Arena(dev), "ref").compute_record(nst.step, 1, nst.env, None, B, 1)
    K.dense_fwd(feats.Xa, Mcat, cvec, out["qt0"])
    out.update(next_agent=nst.step["agent"], next_hits=nst.step["hits"], Xa=feats.Xa, Xo=feats.Xo, efeat=feats.efeat,
               emask=feats.emask)
    return out


def _one_launch(cfg, st, ms, eps, Mcat, cvec, max_blocks=0):
    """the new route on copies of the inputs, every output between guards -> (outputs, guard buffers)"""
    from dgppo_amd import ops_env as OE
    dev = ms.device
    B = st.step["agent"].shape[0]
    st = OE.State({k: v.clone() for k, v in st.step.items()}, {k: v.clone() for k, v in st.env.items()})
    bufs, out = {}, {}
    for k, s in _shapes(cfg, B).items():
        bufs[k], out[k] = _guarded(s, dev)
    nst = OE.State(dict(agent=out["next_agent"], hits=out["next_hits"]), st.env)
    OE.act_step_feats(cfg, st, ms.clone(), None if eps is None else eps.clone(), out["action"],
                      out["log_pi"] if eps is not None else None, nst, out["reward"], out["cost"], out["Xa"], out["Xo"],
                      out["efeat"], out["emask"], FP, Mcat.clone(), cvec.clone(), out["qt0"], H, max_blocks)
    torch.cuda.synchronize()
    if eps is None:          # nothing may write log pi in mode `mode`: the whole buffer is guard
        assert bool((bufs["log_pi"] == SENTINEL).all()), "log_pi written without sampling"
        del out["log_pi"]
    return out, bufs


def _assert_same(got, want, bufs, tag):
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), \
            f"{tag} {k}: {int((_bits(got[k]) != _bits(want[k])).sum())} of {want[k].numel()} words differ"
    for k, b in bufs.items():
        assert _guards_intact(b), f"{tag} {k}: guard words overwritten"


def _random_state(cfg, B, dev, seed):
    from dgppo_amd import ops_env as OE
    st = OE.State.empty(cfg, B, dev)
    OE.reset(cfg, torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919 + seed, st)
    return st


def _random_head(cfg, B, dev, seed):
    rng = np.random.default_rng(seed)
    n = cfg.n_agents
    ms = np.concatenate([rng.normal(0, 1.5, (B * n, 2)), rng.normal(0, 1.0, (B * n, 2))], axis=1).astype(f32)
    return _to(ms, dev), _to(rng.normal(0, 1, (B * n, 2)).astype(f32), dev)


@pytest.mark.parametrize("sample", [True, False], ids=["sample", "mode"])
@pytest.mark.parametrize("B", [1, 5, 261])
@pytest.mark.parametrize("kind,n,n_obs", INSTANCES)
def test_one_launch_equals_the_four_bit_for_bit(cuda, kind, n, n_obs, B, sample):
    """B = 261 is no multiple of the four waves of a workgroup; with the grid capped at 8 workgroups every wave also walks nine
    envs, so the one-env-ahead prefetch of the inputs and of the head rows runs past the batch's end"""
    from dgppo_amd import ops_env as OE
    cfg, _ = _mk(kind, n, n_obs)
    assert OE.act_step_feats_supported(cfg, FP, H)
    st = _random_state(cfg, B, cuda, 3)
    ms, eps = _random_head(cfg, B, cuda, 17 + B)
    Mcat, cvec = _weights(cuda)
    want = _four_launches(cfg, st, ms, eps if sample else None, Mcat, cvec)
    for cap in ((0, 8) if B == 261 else (0,)):
        got, bufs = _one_launch(cfg, st, ms, eps if sample else None, Mcat, cvec, max_blocks=cap)
        _assert_same(got, want, bufs, f"{kind} n={n} B={B} cap={cap}")


@pytest.mark.parametrize("kind,n,n_obs", INSTANCES)
def test_folds_can_be_left_out(cuda, kind, n, n_obs):
    """Xa = NULL / qt0 = NULL: the record is written as before and the buffers of the fold left out stay untouched"""
    from dgppo_amd import ops_env as OE
    cfg, _ = _mk(kind, n, n_obs)
    B = 9
    st = _random_state(cfg, B, cuda, 4)
    ms, eps = _random_head(cfg, B, cuda, 23)
    Mcat, cvec = _weights(cuda)
    want = _four_launches(cfg, st, ms, eps, Mcat, cvec)
    for drop in (("Xa", "Xo", "efeat", "emask"), ("qt0",), ("Xa", "Xo", "efeat", "emask", "qt0")):
        bufs, out = {}, {}
        for k, s in _shapes(cfg, B).items():
            bufs[k], out[k] = _guarded(s, cuda)
        arg = {k: (None if k in drop else v) for k, v in out.items()}
        nst = OE.State(dict(agent=out["next_agent"], hits=out["next_hits"]), st.env)
        OE.act_step_feats(cfg, st, ms, eps, out["action"], out["log_pi"], nst, out["reward"], out["cost"], arg["Xa"], arg["Xo"],
                          arg["efeat"], arg["emask"], FP, Mcat, cvec, arg["qt0"], H)
        torch.cuda.synchronize()
        for k in drop:
            assert bool((bufs[k] == SENTINEL).all()), f"{kind} without {drop}: {k} was written"
        _assert_same(out, {k: v for k, v in want.items() if k not in drop}, bufs, f"{kind} without {drop}")


# ---- hand-built scenes and head rows -----------------------------------------------------------------------------------
STD_INIT_INV, STD_MIN, THRESH, INV_THRESH = f32(-0.43275212956718856), f32(1e-5), f32(0.999), f32(3.8002011672502)
# tag -> (mean, std_trans, eps, the branch of tn_log_prob_dim it must reach)
HEAD_ROWS = {
    "bulk": (0.3, 0.0, 0.5, "atanh"),
    "bulk-negative-zero-mean": (-0.0, 0.0, 0.0, "atanh"),
    "upper-thresh": (6.0, 0.0, 0.0, "hi"),
    "lower-thresh": (-6.0, 0.0, 0.0, "lo"),
    "upper-thresh-series-tail": (-2.0, 0.0, 14.0, "hi-series"),      # z = -(atanh(.999) + 2) / 0.5 = -11.6 <= -10
    "lower-thresh-series-tail": (2.0, 0.0, -14.0, "lo-series"),
    "softplus-linear": (0.1, 30.0, 0.01, "atanh"),                   # std_trans + c > 20: softplus returns its argument
    "mean-nan": (np.nan, 0.0, 0.3, "nan"),
    "mean-plus-inf": (np.inf, 0.0, 0.3, "hi-nan"),                   # action 1, z = -(c - inf) / sd = +inf: log Phi = 0
    "mean-minus-inf": (-np.inf, 0.0, 0.3, "lo-nan"),
    "std-nan": (0.2, np.nan, 0.3, "nan"),
    "std-plus-inf": (0.2, np.inf, 0.0, "nan"),                       # inf * 0 = NaN
    "std-minus-inf": (0.2, -np.inf, 0.3, "atanh"),                   # softplus(-inf) = 0: sd = STD_MIN
    "eps-inf": (0.2, 0.0, np.inf, "hi"),
}


def _branch(mu, st, eps):
    """which return of tn_log_prob_dim a (mean, std_trans, eps) reaches, in fp32 on the CPU"""
    with np.errstate(all="ignore"):
        mu, st, eps = f32(mu), f32(st), f32(eps)
        x = f32(st + STD_INIT_INV)
        sd = f32((x if x > 20 else np.log1p(np.exp(x, dtype=f32), dtype=f32)) + STD_MIN)
        act = np.tanh(f32(mu + sd * eps), dtype=f32)
        if np.isnan(act):
            return "nan"
        ac = min(max(act, -THRESH), THRESH)
        if ac <= -THRESH:
            z = f32((-INV_THRESH - mu) / sd)
            return "lo-nan" if not np.isfinite(z) else ("lo-series" if z <= -10 else "lo")
        if ac >= THRESH:
            z = f32(-(INV_THRESH - mu) / sd)
            return "hi-nan" if not np.isfinite(z) else ("hi-series" if z <= -10 else "hi")
        return "atanh"


def test_head_rows_reach_their_branches():
    """(no GPU needed, but it belongs with the rows) each tag's row takes the branch it is named for, and all are covered"""
    got = {tag: _branch(*row[:3]) for tag, row in HEAD_ROWS.items()}
    assert got == {tag: row[3] for tag, row in HEAD_ROWS.items()}
    assert {"atanh", "hi", "lo", "hi-series", "lo-series", "nan"} <= set(got.values())


@pytest.mark.parametrize("sample", [True, False], ids=["sample", "mode"])
@pytest.mark.parametrize("kind,n,n_obs", INSTANCES)
def test_edge_scenes_and_head_rows(cuda, kind, n, n_obs, sample):
    """the scene catalogue (ties, NaN rays, cull thresholds, mask radii, non-finite actions and states) with its actions fed
    through the head (mean = 2 x action: NaN stays NaN, +-Inf saturates), then the head rows of HEAD_ROWS on both action
    dimensions of agents of the catalogue's envs"""
    from dgppo_amd import ops_env as OE
    cfg, _ = _mk(kind, n, n_obs)
    r = _ref(kind, n, n_obs)
    B = r["agent"].shape[0]
    for name in ("parallel-to-ray", "symmetric-ties", "cull-boundary", "mask-radius", "non-finite"):
        assert S.env_ids(r["tags"], name), f"no scene tagged {name}"
    st = OE.State(dict(agent=_to(r["agent"], cuda), hits=_to(r["hits"], cuda)), dict(goal=_to(r["goal"], cuda), obst=_to(r["obst"], cuda)))
    rng = np.random.default_rng(2)
    with np.errstate(all="ignore"):
        ms = np.concatenate([r["action"].reshape(B * n, 2) * f32(2), rng.normal(0, 1, (B * n, 2)).astype(f32)], axis=1).astype(f32)
    eps = rng.normal(0, 1, (B * n, 2)).astype(f32)
    tags = list(HEAD_ROWS)
    assert len(tags) <= B, "one env per head row"
    for j, tag in enumerate(tags):                 # env j, agent j % n: the row on dimension 0, its mirror image on dimension 1
        mu, stt, ep, want_branch = HEAD_ROWS[tag]
        assert _branch(mu, stt, ep) == want_branch, tag
        row = j * n + (j % n)
        ms[row] = (mu, -mu, stt, stt)
        eps[row] = (ep, -ep)
    ms_d, eps_d = _to(ms, cuda), _to(eps, cuda)
    Mcat, cvec = _weights(cuda)
    want = _four_launches(cfg, st, ms_d, eps_d if sample else None, Mcat, cvec)
    got, bufs = _one_launch(cfg, st, ms_d, eps_d if sample else None, Mcat, cvec)
    _assert_same(got, want, bufs, f"{kind} scenes")
    assert bool(torch.isnan(want["action"]).any()) and bool(torch.isnan(want["next_hits"]).any()), "the catalogue lost its NaNs"


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_unsupported_configurations_are_refused(cuda):
    from dgppo_amd import _native as N, ops_env as OE
    ok, _ = _mk("LidarSpread", 4, 2)
    assert OE.act_step_feats_supported(ok, FP, H)
    assert not OE.act_step_feats_supported(ok, 12, H) and not OE.act_step_feats_supported(ok, FP, 2)
    odd, _ = _mk("LidarSpread", 3, 2)                                   # no wave-per-env instance for three agents
    mpe = N.make_env_cfg(N.ENV_KINDS["MPESpread"], 4, 2)
    vmas = N.make_env_cfg(N.ENV_KINDS["VMASReverseTransport"], 4, 0)
    # the 16-agent wave instances keep the four launches (above ACT_MAX_NA): no act-step form is compiled for them
    big = [_mk("LidarSpread", 16, 8)[0], _mk("LidarBicycleTarget", 16, 8)[0]]
    for cfg in (odd, mpe, vmas, *big):
        assert not OE.act_step_feats_supported(cfg, FP, H)
    B = 2
    for cfg, fp, h in ((odd, FP, H), (ok, 12, H), (ok, FP, 2), (big[0], FP, H), (big[1], FP, H)):
        n = cfg.n_agents
        st = _random_state(cfg, B, cuda, 1)
        z = lambda *s: torch.zeros(*s, device=cuda)
        before = {k: v.clone() for k, v in st.step.items()}
        with pytest.raises(ValueError, match="no kernel for this configuration"):
            OE.act_step_feats(cfg, st, z(B * n, 4), None, z(B, n, 2), None, st.like(), z(B), z(B, n, 2), z(B * n, fp),
                              z(B * (cfg.num_nodes - 1 - n), fp), z(B * n, cfg.fan_in, 4), z(B * n, cfg.fan_in), fp,
                              z(fp, h * fp), z(h * fp), z(B * n, h * fp), h)
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(v), _bits(before[k])) for k, v in st.step.items())
    # an operand off its 16-byte boundary never reaches the kernel either
    n = ok.n_agents
    st = _random_state(ok, B, cuda, 1)
    z = lambda *s: torch.zeros(*s, device=cuda)
    off = torch.zeros(B * n * FP + 1, device=cuda)[1:].view(B * n, FP)
    with pytest.raises(ValueError, match="16-byte aligned"):
        OE.act_step_feats(ok, st, z(B * n, 4), None, z(B, n, 2), None, st.like(), z(B), z(B, n, 2), off,
                          z(B * (ok.num_nodes - 1 - n), FP), z(B * n, ok.fan_in, 4), z(B * n, ok.fan_in), FP)
    # and an engine asked for the fused step on them takes the four launches
    from dgppo_amd import engine as EN
    for cfg in big:
        assert EN.Engine(cfg, EN.Hyper(batch_size=8, rnn_step=4, train_steps=10), cuda, T=4, fused_step=True).fused_step is False


# ---- engine level --------------------------------------------------------------------------------------------------------
def _engine(cfg, dev, fused, graphs, B=37, T=4):
    from dgppo_amd import engine as EN, init
    eng = EN.Engine(cfg, EN.Hyper(batch_size=B * T, rnn_step=T, train_steps=10), dev, T=T, use_graphs=graphs, multi_stream=graphs,
                    fused_step=fused)
    eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
    eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
    eng.Vh.load_tree(init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3))
    eng.set_entropy_noise(1)
    return eng


def _record(ro):
    ro.finalize()
    out = {k: v for k, v in ro.step.items()}
    out.update({"env." + k: v for k, v in ro.env.items()})
    out.update(actions=ro.actions, rewards=ro.rewards, costs=ro.costs, rnn=ro._rnn_em[:, :ro.T + 1])
    if ro.stochastic:
        out["log_pis"] = ro.log_pis
    return out


def _fused_on_off_identical(cuda, kind, n, n_obs, B, T, graphs):
    """every array of both records and both value pre-passes, fused_step on against off; with HIP graphs the second call of
    each engine replays its captured loop"""
    cfg, _ = _mk(kind, n, n_obs)
    sd = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    res = {}
    for fused in (True, False):
        eng = _engine(cfg, cuda, fused, graphs, B, T)
        assert eng.fused_step == fused
        for it in range(2 if graphs else 1):
            ro, det = eng.rollout_pair(sd + it, sd + 5 + it, noise_seed=3 + it)
        arrays = {}
        for name, rec in (("ro", ro), ("det", det)):
            arrays.update({f"{name}.{k}": v.clone() for k, v in _record(rec).items()})
            Vl, Vh = eng.values_prepass(rec, want_Vl=(name == "ro"))
            arrays[f"{name}.Vh"] = Vh.clone()
            if Vl is not None:
                arrays[f"{name}.Vl"] = Vl.clone()
        torch.cuda.synchronize()
        res[fused] = arrays
        if graphs:
            assert all(s["graph"] is not None for s in eng._ro_cache.values()), "the rollout loop was not captured"
    assert res[True].keys() == res[False].keys()
    for k in res[False]:
        assert torch.equal(_bits(res[True][k]), _bits(res[False][k])), f"{k} differs between fused_step=True and False"


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
def test_engine_rollouts_identical_with_and_without_the_fused_step(cuda, graphs):
    """LidarSpread n = 4, B = 37, T = 4"""
    _fused_on_off_identical(cuda, "LidarSpread", 4, 2, 37, 4, graphs)


def _more_than_one_pass(dev):
    """a batch no grid of the act-step kernel covers in one pass.  The engine leaves the grid at its cap, CUs x resident
    workgroups with one env per wave; 4 waves per workgroup and 8 workgroups per CU (32 waves, the most a CU holds of a
    256-thread workgroup) bound every instance's cap from above.  The 37 envs on top give some waves a second env and
    others none, and leave the last workgroup ragged (37 = 9 x 4 + 1)"""
    return 4 * 8 * torch.cuda.get_device_properties(dev).multi_processor_count + 37


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("kind,n,n_obs,B,T", [("LidarSpread", 8, 3, 37, 4),               # the benchmark's topology
                                              ("LidarBicycleTarget", 4, 3, 37, 4),        # state_dim 5
                                              ("LidarSpread", 4, 2, None, 3)],            # B = _more_than_one_pass
                         ids=["spread8", "bicycle4", "spread4-two-passes"])
def test_engine_fused_step_identical_at_more_shapes(cuda, kind, n, n_obs, B, T, graphs):
    """the same comparison where the engine's loop differs from the kernel tests' own buffers: the instance bench.py times,
    the five-word state, and a batch at which every persistent wave walks on to a second env inside the engine's loop — the
    features and qt0 each step's launch leaves in place are then written and read env-strided, and the step at t = T - 1
    passes no feature buffers"""
    if B is None:
        B = _more_than_one_pass(cuda)
        assert B > 4 * 8 * torch.cuda.get_device_properties(cuda).multi_processor_count
    _fused_on_off_identical(cuda, kind, n, n_obs, B, T, graphs)
