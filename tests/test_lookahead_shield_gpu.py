"""Lookahead shield on the device: dgppo_env_team_action_fork and dgppo_lookahead_select against the NumPy restatement
(tests/lookahead_np.py), Engine.lookahead_select on a hand-made scene against oracle/env_np.py, Engine.rollout_lookahead_shielded
re-derived step by step from its block records, and test.py --shield --shield-horizon in-process."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lookahead_np as L  # noqa: E402
from test_lookahead_shield_cpu import HAND_CASES, US as HAND_US, VS as HAND_VS  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
ROOT = os.path.dirname(HERE)


def _cfg(kind_name, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind_name], n, n_obs)


def _words(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _same_words(got, want, name):
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, f"{name}: {bad} of {got.numel()} words differ"


# ---- 1. the fork against the restatement --------------------------------------------------------------------------------------------
# rows of 12 / 48 / 32 words (16-byte vectors), of 10 (8-byte: the bicycle's five columns, two agents) and of 15 (single words)
FORK_KINDS = [("LidarSpread", 3, 2), ("MPESpread", 3, 3), ("LidarBicycleTarget", 2, 1), ("LidarSpread", 3, 0),
              ("LidarBicycleTarget", 3, 2)]
FORK_SHAPES = [(1, 1, 1, 64), (3, 2, 3, 128), (3, 1, 1, None), (1, 2, 3, None)]        # n_env, nu, nv, HC (None: no carry)


@pytest.mark.parametrize("kind,n,n_obs", FORK_KINDS, ids=["-".join(map(str, c)) for c in FORK_KINDS])
def test_fork_equals_the_restatement(cuda, kind, n, n_obs):
    """every word of every output; a_pol holds a value outside [-1, 1] and a NaN with a payload, the grid a value outside the
    box: the fork moves words, it does not clip"""
    from dgppo_amd import ops_env as OE, ops_nn as K_
    cfg = _cfg(kind, n, n_obs)
    for B, nu, nv, HC in FORK_SHAPES:
        st = OE.State.empty(cfg, B, cuda)
        OE.reset(cfg, torch.arange(B, dtype=torch.int64, device=cuda) + 31, st)
        rng = np.random.default_rng(B * 100 + nu * 10 + nv)
        a_pol = rng.uniform(-1.0, 1.0, size=(B, n, 2)).astype(f32)
        a_pol[0, 0, 0] = 3.5
        a_pol.view(np.uint32)[B - 1, n - 1, 1] = 0x7FC12345                      # a NaN with a payload
        us = np.linspace(-1.0, 1.0, nu).astype(f32) if nu > 1 else np.array([1.75], f32)
        vs = np.linspace(-1.0, 1.0, nv).astype(f32) if nv > 1 else np.array([-0.3], f32)
        carry = rng.standard_normal((B * n, HC)).astype(f32) if HC else None
        P = 1 + nu * nv
        G = B * n * P
        out = OE.State.empty(cfg, G, cuda)
        for v in list(out.step.values()) + list(out.env.values()):
            v.fill_(float("nan"))
        # without a carry the action buffer starts at an odd word: the rows go out as single words there
        action = torch.full((G * n * 2 + 1,), float("nan"), device=cuda)[0 if HC else 1:][:G * n * 2].view(G, n, 2)
        d_carry = torch.from_numpy(carry).to(cuda) if HC else None
        carry_out = torch.full((G * n, HC), float("nan"), device=cuda) if HC else None
        OE.team_action_fork(cfg, st, torch.from_numpy(a_pol).to(cuda), K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda),
                            out, action, d_carry, carry_out)
        torch.cuda.synchronize()
        fields = {k: v.cpu().numpy() for k, v in {**st.step, **st.env}.items()}
        assert ("hits" in fields) == (cfg.is_lidar and n_obs > 0) and ("obst" in fields) == (n_obs > 0)
        want, want_action, want_carry = L.fork_np(fields, a_pol, us, vs, carry)
        tag = f"{kind} B={B} grid {nu}x{nv} HC={HC}"
        for k, v in {**out.step, **out.env}.items():
            np.testing.assert_array_equal(_words(v), want[k], err_msg=f"{k} {tag}")
        np.testing.assert_array_equal(_words(action), want_action, err_msg=f"action {tag}")
        if HC:
            np.testing.assert_array_equal(_words(carry_out), want_carry, err_msg=f"carry {tag}")
        assert float(action[0, 0, 0]) == 3.5 and int(_words(action)[G - P, n - 1, 1]) == 0x7FC12345


# ---- 2. the select kernel against the restatement -------------------------------------------------------------------------------------
def _select(cuda, cost, stride_pad, a_pol, us, vs, margin, want_s=True):
    """cost [K, G, n, nh] handed over as slots 1 .. K of a [K + 1, G * n * nh + stride_pad] buffer"""
    from dgppo_amd import ops_nn as K_
    Kk, G, n, nh = cost.shape
    E = a_pol.shape[0]
    P = G // (E * n)
    buf = torch.full((Kk + 1, G * n * nh + stride_pad), float("nan"), device=cuda)
    cost_tm = buf[1:, :G * n * nh].view(Kk, G, n, nh)
    cost_tm.copy_(torch.from_numpy(np.ascontiguousarray(cost, f32)).to(cuda))
    action = torch.full((E, n, 2), float("nan"), device=cuda)
    index = torch.full((E, n), -7, dtype=torch.int32, device=cuda)
    flag = torch.full((E, n), -7, dtype=torch.int32, device=cuda)
    s = torch.full((E, n, P), float("nan"), device=cuda) if want_s else None
    K_.lookahead_select(cost_tm, torch.from_numpy(np.ascontiguousarray(a_pol, f32)).to(cuda), K_.sweep_axis(us, "us", cuda),
                        K_.sweep_axis(vs, "vs", cuda), margin, action, index, flag, s)
    torch.cuda.synchronize()
    return action.cpu().numpy(), index.cpu().numpy(), flag.cpu().numpy(), None if s is None else s.cpu().numpy()


def _check_select(cuda, cost, stride_pad, a_pol, us, vs, margin, name):
    E, n = a_pol.shape[:2]
    P = cost.shape[1] // (E * n)
    action, index, flag, s = _select(cuda, cost, stride_pad, a_pol, us, vs, margin)
    want_s = L.fold_np(cost, E, n, P)
    L.assert_same_words(s, want_s, f"{name}: s")
    wi, wf, wa = L.rule_np(want_s, a_pol, us, vs, margin)
    np.testing.assert_array_equal(index, wi, err_msg=f"{name}: index")
    np.testing.assert_array_equal(flag, wf, err_msg=f"{name}: flag")
    np.testing.assert_array_equal(action.view(np.uint32), wa.view(np.uint32), err_msg=f"{name}: action")
    a2, i2, f2, none = _select(cuda, cost, stride_pad, a_pol, us, vs, margin, want_s=False)
    assert none is None and np.array_equal(i2, index) and np.array_equal(f2, flag), f"{name}: without the s output"
    return index, flag, s


def test_select_hand_made_cases(cuda):
    """the CPU test's cases through the kernel: agent 1 of a two-agent env carries the values — its largest word sits in a
    different (step, component) per candidate — and agent 0 sees +5 on its own rows: nothing admissible"""
    n, P, Kk, nh = 2, 3, 2, 2
    for name, s, margin, a1, want in HAND_CASES:
        cost = np.full((Kk, n * P, n, nh), -9.0, f32)
        cost[:, :P, 0, :] = 5.0                                            # agent 0's own rows
        cost[:, :P, 1, :] = np.nan                                          # agent 1's rows of agent 0's envs: never read
        for p in range(P):
            cost[p % Kk, P + p, 1, (p + 1) % nh] = s[p]
        a_pol = np.array([[[0.0, 0.0], a1]], f32)
        index, flag, got_s = _check_select(cuda, cost, 0, a_pol, HAND_US, HAND_VS, margin, name)
        assert (int(index[0, 1]), int(flag[0, 1])) == want, name
        assert flag[0, 0] == 2 and index[0, 0] == 0


SELECT_CASES = [(1, 1, 1, 1, 1, 0), (5, 2, 3, 2, 3, 0), (5, 3, 5, 3, 3, 24), (1, 3, 3, 2, 8, 0), (5, 1, 2, 3, 8, 8), (5, 2, 3, 1, 3, 4)]


@pytest.mark.parametrize("Kk,nh,E,n,grid,pad", SELECT_CASES, ids=[f"K{c[0]}-nh{c[1]}-E{c[2]}-n{c[3]}-grid{c[4]}-pad{c[5]}" for c in SELECT_CASES])
def test_select_random(cuda, Kk, nh, E, n, grid, pad):
    """costs of the environment's kind (-1 .. -0.5 and 0.5 .. 1) with a sprinkle of NaN; P = 2, 10 and 65 (the second pass over
    the lanes); E * n = 1, 6, 15, 6, 6, 3 rows, none a multiple of the four waves of a block but for none at all; a step stride
    larger than a step where pad > 0; the last env's first agent has nothing finite"""
    rng = np.random.default_rng(Kk * 1000 + nh * 100 + E * 10 + n)
    us = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([0.25], f32)
    vs = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([-0.5], f32)
    P = 1 + grid * grid
    G = E * n * P
    mag = rng.uniform(0.5, 1.0, size=(Kk, G, n, nh))
    # per (env, agent) the share of unsafe words differs: some agents admit everything, some nothing
    share = rng.uniform(0.0, 0.25, size=(1, E, n, 1, 1, 1)) ** 2
    unsafe = rng.uniform(size=(Kk, E, n, P, n, nh)) < share
    cost = np.where(unsafe.reshape(Kk, G, n, nh), mag, -mag).astype(f32)
    cost[rng.uniform(size=cost.shape) < 0.01] = np.nan
    cost.reshape(Kk, E, n, P, n, nh)[:, E - 1, 0, :, 0] = np.nan
    a_pol = rng.uniform(-1.3, 1.3, size=(E, n, 2)).astype(f32)
    seen = set()
    for margin in (0.0, 0.75, -2.0):
        index, flag, s = _check_select(cuda, cost, pad, a_pol, us, vs, margin, f"random margin {margin}")
        assert flag[E - 1, 0] == 2 and index[E - 1, 0] == 0
        seen |= set(np.unique(flag).tolist())
    if E * n >= 6:
        assert seen == {0, 1, 2}


# ---- 3. the core on a hand-made scene ---------------------------------------------------------------------------------------------------
def _engine(kind, n, n_obs, T_, cuda, use_rnn=True, rnn_layers=1, algo="dgppo"):
    from dgppo_amd import engine as EN, init
    cfg = _cfg(kind, n, n_obs)
    nc = rnn_layers if use_rnn else 0
    hp = EN.Hyper(batch_size=1024, rnn_step=2, train_steps=100, use_rnn=use_rnn, rnn_layers=rnn_layers, use_lstm=False)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo=algo)
    trees = {"policy": init.init_policy(0, cfg.node_dim, 2, 2, nc, False),
             "Vl": init.init_value(0, cfg.node_dim, 1, 2, 2, rnn_layers=nc, lstm=False),
             "Vh": init.init_value(0, cfg.node_dim, cfg.n_cost, 1, 3, rnn_layers=min(nc, 1))}
    rng = np.random.default_rng(11)
    jitter = lambda tr: T.tree_map(lambda a: torch.from_numpy(a + 0.05 * rng.standard_normal(a.shape).astype(f32)), tr)
    for k_, net in eng.nets.items():
        net.load_tree(jitter(trees[k_]))
    eng.set_entropy_noise(77)
    return cfg, eng


@pytest.mark.parametrize("mover", [0, 1])
def test_core_on_a_hand_made_scene(cuda, mover):
    """LidarSpread n = 2, obs = 1 (lookahead_np.scene): one agent flies at the obstacle, the other rests far away; the policy's
    parameters are zero, so its action is exactly 0.  The oracle alone first shows that the scene is not trivial: left alone the
    mover's worst own-row cost within H is >= 0.5, and some grid action keeps it <= -0.5.  Then Engine.lookahead_select: s within
    1e-5 of the oracle's, index / flag the NumPy rule on the oracle's s.  Every finite cost is <= -0.5 or >= 0.5
    (lidar_env/base.py:203-205), so at margin 0 no value can sit at the threshold and no flip is excusable."""
    from dgppo_amd import ops_env as OE, ops_nn as K_
    H, us, vs = L.SCENE_H, L.SCENE_US, L.SCENE_VS
    ocfg, agent, goal, obst = L.scene(mover)
    want_s = L.scene_oracle(mover)
    P = want_s.shape[-1]
    assert want_s[0, mover, 0] >= 0.5, "the scene became trivial: the policy's own action is safe"
    assert (want_s[0, mover, 1:] <= -0.5).any(), "the scene became hopeless: no grid action is safe"
    assert ((want_s <= -0.5) | (want_s >= 0.5)).all()
    cfg, eng = _engine("LidarSpread", 2, 1, 4, cuda)
    eng.policy.params.zero_()
    eng.policy.prepare()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, f32)).to(cuda)
    st = OE.State({"agent": d(agent)}, {"goal": d(goal), "obst": d(obst)})
    OE.sense(cfg, st)
    n, HC = 2, eng.HC
    # the policy's action on this state, through the path rollout_lookahead_shielded takes
    carry_next = torch.full((n, HC), float("nan"), device=cuda)
    act = eng.policy.forward(eng._feats("la", st, 1), n_seq=n, T=1, h0=torch.zeros(n, HC, device=cuda), tag="la",
                             hs_out=carry_next, train=False)
    a_pol = torch.full((1, n, 2), float("nan"), device=cuda)
    K_.policy_head(act["ms"], None, None, a_pol.view(n, 2), None, None, n, 1)
    torch.cuda.synchronize()
    assert bool((a_pol == 0).all()), "zero parameters give the zero action"
    action = torch.full((1, n, 2), float("nan"), device=cuda)
    index = torch.full((1, n), -7, dtype=torch.int32, device=cuda)
    flag = torch.full((1, n), -7, dtype=torch.int32, device=cuda)
    s = torch.full((1, n, P), float("nan"), device=cuda)
    records = []
    eng.lookahead_select(st, carry_next, a_pol, K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda), H, 0.0, action, index,
                         flag, s, records=records)
    torch.cuda.synchronize()
    assert len(records) == 1 and records[0][:3] == (0, 0, 1) and records[0][3].T == H + 1
    assert bool((records[0][3].action_tm[1:] == 0).all()), "the rolled policy plays the zero action"
    got = s.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want_s).max())
    print(f"mover {mover}: s max abs err against the oracle {err:.3e}; bit-equal: {np.array_equal(got, want_s)}")
    assert err <= 1e-5
    wi, wf, wa = L.rule_np(want_s, np.zeros((1, n, 2), f32), us, vs, 0.0)
    np.testing.assert_array_equal(index.cpu().numpy(), wi)
    np.testing.assert_array_equal(flag.cpu().numpy(), wf)
    np.testing.assert_array_equal(action.cpu().numpy(), wa)
    assert wf[0, mover] == 1 and wf[0, 1 - mover] == 0


# ---- 4. the engine ------------------------------------------------------------------------------------------------------------------------
def _record_words(ro):
    """every word of a time-major record"""
    out = {f"step.{k}": v for k, v in ro.step_tm.items()}
    out.update(action=ro.action_tm, rnn=ro.rnn_tm, reward=ro.reward_tm, cost=ro.cost_tm)
    return out


def _step_check(cfg, st, action, nst, name):
    """nst's per-step fields are ops_env.step(st, action) bit for bit"""
    from dgppo_amd import ops_env as OE
    B = int(action.shape[0])
    got = st.like()
    OE.step(cfg, st, action, got, torch.empty(B, device=action.device), torch.empty(B, cfg.n_agents, cfg.n_cost, device=action.device))
    for key, v in got.step.items():
        _same_words(v, nst.step[key], f"{name}: {key}")


ENGINE_CASES = [("dgppo", "LidarSpread", 3, 2, "dgppo", True, 1), ("dgppo-no-rnn", "LidarSpread", 3, 2, "dgppo", False, 1),
                ("dgppo-rnn-layers-2", "LidarSpread", 3, 2, "dgppo", True, 2), ("informarl-mpe", "MPESpread", 3, 3, "informarl", True, 1),
                ("hcbfcrpo", "LidarSpread", 3, 2, "hcbfcrpo", True, 1)]


@pytest.mark.parametrize("grid", [2, 3])
@pytest.mark.parametrize("name,kind,n,n_obs,algo,use_rnn,rnn_layers", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_rollout_lookahead_shielded(cuda, name, kind, n, n_obs, algo, use_rnn, rnn_layers, grid):
    """T = 3, H = 3, B = 2.  From the block records, for every block and every k: states[k + 1] is ops_env.step(states[k],
    action[k]) bit for bit, action[0] the restated joint action, rnn[1] the broadcast of h_{t+1}, log.s the restated fold of that
    record's cost_tm[1 : H + 1] bit for bit; index / flag / executed action are the NumPy rule on log.s.  Step 0 sees the state of
    rollout(seeds, False): policy_action[0] is that record's action in every word and s[0, e, i, 0] the own-row maximum of its
    cost_tm[1 : H + 1] within 1e-5 (the what-if env of candidate 0 replays the unshielded episode in another batch size).  Every
    step: state t + 1 is ops_env.step(state t, action t) bit for bit.  margin -10 admits everything (costs lie in [-1, 1]): the
    record equals rollout(seeds, False) in every word; margin +10 admits nothing: flag 2, the lowest-index argmin of s.  One env
    per block and prepass_graphs = 1 give every word again."""
    T_, H, B = 3, 3, 2
    cfg, eng = _engine(kind, n, n_obs, T_, cuda, use_rnn, rnn_layers, algo)
    nh, HC = cfg.n_cost, eng.HC
    seeds = torch.tensor([9, 10], dtype=torch.int64, device=cuda)
    us = vs = np.linspace(-1.0, 1.0, grid).astype(f32)
    P = 1 + grid * grid
    records = []
    ro, log = eng.rollout_lookahead_shielded(seeds, us, vs, H, records=records)
    torch.cuda.synchronize()
    assert tuple(log["policy_action"].shape) == (T_, B, n, 2) and tuple(log["s"].shape) == (T_, B, n, P)
    assert tuple(log["index"].shape) == tuple(log["flag"].shape) == (T_, B, n) and sorted(log) == ["flag", "index", "policy_action", "s"]
    assert log["index"].dtype == log["flag"].dtype == torch.int32 and not ro.stochastic and ro.log_pi_tm is None
    assert [r[:3] for r in records] == [(t, 0, B) for t in range(T_)], "the default prepass_graphs holds both envs in one block"
    s_all, pol = log["s"].cpu().numpy(), log["policy_action"].cpu().numpy()
    assert np.isfinite(s_all).all()

    # ---- every block record ----
    for t, e0, Eb, rec in records:
        assert rec.B == Eb * n * P and rec.T == H + 1
        st = ro.states_tm[t]
        fields = {k: v[e0:e0 + Eb].cpu().numpy() for k, v in {**st.step, **st.env}.items()}
        carry = ro.rnn_tm[t + 1][e0:e0 + Eb].reshape(Eb * n, HC).cpu().numpy() if use_rnn else None
        want, want_action, want_carry = L.fork_np(fields, pol[t, e0:e0 + Eb], us, vs, carry)
        tag = f"{name} grid {grid} t={t} block {e0}"
        for k, v in {**rec.states_tm[0].step, **rec.states_tm[0].env}.items():
            np.testing.assert_array_equal(_words(v), want[k], err_msg=f"{tag}: slot 0 {k}")
        np.testing.assert_array_equal(_words(rec.action_tm[0]), want_action, err_msg=f"{tag}: the forced joint action")
        if use_rnn:
            np.testing.assert_array_equal(_words(rec.rnn_tm[1]).reshape(-1, HC), want_carry, err_msg=f"{tag}: rnn[1]")
        for k in range(H + 1):
            _step_check(cfg, rec.states_tm[k], rec.action_tm[k], rec.states_tm[k + 1], f"{tag}: block states[{k + 1}]")
        L.assert_same_words(s_all[t, e0:e0 + Eb], L.fold_np(rec.cost_tm[1:H + 1].cpu().numpy(), Eb, n, P), f"{tag}: log.s")

    # ---- every step ----
    for t in range(T_):
        _step_check(cfg, ro.states_tm[t], ro.action_tm[t], ro.states_tm[t + 1], f"{name}: states[{t + 1}]")
        wi, wf, wa = L.rule_np(s_all[t], pol[t], us, vs, 0.0)
        np.testing.assert_array_equal(log["index"][t].cpu().numpy(), wi, err_msg=f"{name}: index[{t}]")
        np.testing.assert_array_equal(log["flag"][t].cpu().numpy(), wf, err_msg=f"{name}: flag[{t}]")
        np.testing.assert_array_equal(_words(ro.action_tm[t]), wa.view(np.uint32), err_msg=f"{name}: action[{t}]")

    # ---- step 0 against the unshielded record of H + 1 steps ----
    _, eng_u = _engine(kind, n, n_obs, H + 1, cuda, use_rnn, rnn_layers, algo)
    ro_u = eng_u.rollout(seeds, False)
    _same_words(log["policy_action"][0], ro_u.action_tm[0], f"{name}: policy_action[0] vs rollout(seeds, False)")
    want0 = ro_u.cost_tm[1:H + 1].cpu().numpy().max(axis=(0, 3))              # [B, n]: row i of the record is agent i's own
    err = float(np.abs(s_all[0, :, :, 0].astype(np.float64) - want0).max())
    print(f"{name} grid {grid}: s[0, :, :, 0] vs the unshielded record: max abs err {err:.3e}; bit-equal: "
          f"{np.array_equal(s_all[0, :, :, 0], want0)}")
    assert err <= 1e-5

    # ---- everything admissible / nothing admissible ----
    mine = {k: v.clone() for k, v in _record_words(ro).items()}
    ro_a, log_a = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=-10.0)
    assert int(log_a["flag"].abs().sum()) == 0 and int(log_a["index"].abs().sum()) == 0
    ro_3 = eng.rollout(seeds, False)
    for (key, a), b in zip(_record_words(ro_a).items(), _record_words(ro_3).values()):
        if key == "rnn" and not use_rnn:
            continue                                   # without a cell nothing writes the carries
        _same_words(a, b, f"{name}: everything admissible: {key} vs rollout(seeds, False)")
    ro_n, log_n = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=10.0)
    assert bool((log_n["flag"] == 2).all())
    sn = log_n["s"].cpu().numpy()
    assert np.isfinite(sn).all()
    np.testing.assert_array_equal(log_n["index"].cpu().numpy(), sn.argmin(axis=-1))

    # ---- several blocks of environments ----
    cap = eng.prepass_graphs
    try:
        eng.prepass_graphs = n * P * (H + 2)                         # one env per block
        recs_b = []
        ro_b, log_b = eng.rollout_lookahead_shielded(seeds, us, vs, H, records=recs_b)
        eng.prepass_graphs = 1                                       # less than one env: still one env per block
        ro_c, log_c = eng.rollout_lookahead_shielded(seeds, us, vs, H)
    finally:
        eng.prepass_graphs = cap
    assert [r[:3] for r in recs_b] == [(t, e, 1) for t in range(T_) for e in range(B)]
    for other_ro, other_log, what in ((ro_b, log_b, "blocks of one env"), (ro_c, log_c, "prepass_graphs = 1")):
        for key, b in _record_words(other_ro).items():
            if key == "rnn" and not use_rnn:
                continue
            _same_words(b, mine[key], f"{name}: {what}: {key}")
        for key in log:
            _same_words(other_log[key], log[key], f"{name}: {what}: log.{key}")


def test_engine_refusals(cuda):
    from dgppo_amd import _native as N, engine as EN
    seeds = torch.tensor([1], dtype=torch.int64, device=cuda)
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="rollout_lookahead_shielded.*VMASReverseTransport"):
        vmas.rollout_lookahead_shielded(seeds, [0.5], [0.5], 2)
    cfg, eng = _engine("LidarSpread", 3, 2, 3, cuda)
    for kw, match in ((dict(us=[]), "us"), (dict(vs=[0.5, float("inf")]), "vs"), (dict(margin=float("nan")), "margin"),
                      (dict(horizon=0), "horizon"), (dict(horizon=-3), "horizon")):
        args = dict(us=[0.5], vs=[0.5], horizon=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            eng.rollout_lookahead_shielded(seeds, **args)


# ---- 5. test.py --shield --shield-horizon, in-process -----------------------------------------------------------------------------------
def _load_test_py():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))   # `test` is a stdlib package
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_dir(tmp_path, algo_name, n, Tn):
    """a run directory as train.py leaves it before the first update: config.yaml and models/0"""
    import yaml
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    conf = dict(env="LidarSpread", num_agents=n, obs=1, algo=algo_name, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, seed=3, use_rnn=True, rnn_layers=1, use_lstm=False, alpha=10.0)
    env = make_env(env_id=conf["env"], num_agents=n, num_obs=conf["obs"], max_step=Tn)
    algo = make_algo(algo=algo_name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=n, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2,
                     Vh_gnn_layers=1, lr_actor=3e-4, lr_Vl=1e-3, max_grad_norm=2.0, seed=3, use_rnn=True, rnn_layers=1,
                     use_lstm=False, alpha=10.0, batch_size=4 * Tn, rnn_step=Tn, train_steps=1)
    run = tmp_path / f"run_{algo_name}"
    algo.save(str(run / "models"), 0)
    with open(run / "config.yaml", "w") as f:
        yaml.safe_dump(conf, f)
    return run


def test_cli_runs_the_lookahead_shield_for_informarl(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import LookaheadShieldLog
    n, grid, Tn, H = 2, 2, 3, 2
    run = _run_dir(tmp_path, "informarl", n, Tn)
    mod = _load_test_py()
    common = ["--path", str(run), "--epi", "2", "--no-video", "--max-step", str(Tn)]
    with pytest.raises(ValueError, match="informarl"):                      # the one-step shield still needs DGPPO's Vh
        mod.main(common + ["--shield"])
    capsys.readouterr()
    mod.main(common + ["--shield", "--shield-horizon", str(H), "--shield-grid", str(grid)])
    printed = capsys.readouterr().out
    for word in ("intervention_frac", "infeasible_frac", "mean_deviation"):
        assert printed.count(word) == 2, word
    assert printed.count("safe rate") == 2
    files = sorted(glob.glob(str(run / "videos" / "0" / "*_shield.npz")))
    assert len(files) == 2
    lin = np.linspace(-1.0, 1.0, grid).astype(f32)
    P = 1 + grid * grid
    stats = ("intervention_frac", "infeasible_frac", "mean_deviation")
    per_epi = ("policy_action", "action", "index", "flag", "s")
    for path in files:
        z = np.load(path)
        assert sorted(z.files) == sorted([*LookaheadShieldLog._fields, *stats])
        np.testing.assert_array_equal(z["us"], lin)
        np.testing.assert_array_equal(z["vs"], lin)
        assert z["policy_action"].shape == z["action"].shape == (Tn, n, 2) and z["s"].shape == (Tn, n, P)
        assert z["index"].shape == z["flag"].shape == (Tn, n) and float(z["margin"]) == 0.0 and int(z["horizon"]) == H
        wi, wf, wa = L.rule_np(z["s"], z["policy_action"], lin, lin, 0.0)
        np.testing.assert_array_equal(z["index"], wi)
        np.testing.assert_array_equal(z["flag"], wf)
        np.testing.assert_array_equal(z["action"], wa)
        one = LookaheadShieldLog(*(z[k][None] if k in per_epi else z[k] for k in LookaheadShieldLog._fields))
        for key, v in EV.shield_stats(one).items():
            np.testing.assert_array_equal(z[key], v[0])
