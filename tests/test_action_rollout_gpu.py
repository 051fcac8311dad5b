"""Action rollout landscape on the device: dgppo_env_action_sweep_fork bit for bit against the NumPy restatement
(tests/action_rollout_np.py), Engine.action_rollout_landscape on the lookahead shield's hand-made scene against oracle/env_np.py,
re-derived step by step from its block records, against Engine.lookahead_select and against the record it forks from, its walks
over the grid, and the public surface up to test.py --action-rollout-landscape in-process."""
import glob
import inspect
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import action_rollout_np as AR  # noqa: E402
import lookahead_np as L  # noqa: E402
from test_lookahead_shield_gpu import (ENGINE_CASES, _cfg, _engine, _load_test_py, _run_dir, _same_words, _step_check,  # noqa: E402
                                       _words)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
SENTINEL = 0x7FC0BEEF                                      # a NaN no input holds
GUARD = 8                                                  # rows behind every output that must come back untouched


def _random_words(rng, shape, device):
    """every bit pattern: finite values, infinities, NaNs with payloads"""
    w = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(w.view(f32).copy()).to(device)


def _guarded(shape, device):
    """-> (the [G, ...] output, its whole buffer with GUARD rows behind it), every word the sentinel"""
    buf = torch.empty((shape[0] + GUARD,) + tuple(shape[1:]), device=device)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf[:shape[0]], buf


def _offset_view(t):
    """the same values one word into a larger buffer: no 8- or 16-byte alignment is left"""
    buf = torch.empty(t.numel() + 5, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---- 1. the fork against the restatement --------------------------------------------------------------------------------------------
# rows of 12 / 48 / 32 words (16-byte vectors), of 15 (single words: the bicycle's five columns, three agents), of 8 and of 16
FORK_KINDS = [("LidarSpread", 3, 2), ("LidarSpread", 3, 0), ("MPESpread", 3, 3), ("LidarBicycleTarget", 3, 1),
              ("MPEConnectSpread", 2, 0), ("LidarSpread", 4, 2)]
# frame_ids, n_frames, nu, nv, HC (None: no carry), agent (0: first, -1: last), source.  5 x 5 with 3 frames: G = 75 crosses the
# 64-env tile with a frame boundary inside a tile
FORK_SHAPES = [(None, 2, 1, 1, 64, 0, "offset"), ([3, 0, 2], 3, 3, 2, 128, -1, "record"), ([3, 0, 2], 3, 5, 5, None, -1, "offset"),
               (None, 2, 3, 2, 64, 0, "record"), ([3, 0, 2], 3, 5, 5, 64, 0, "record"), ([3, 0, 2], 3, 3, 2, 128, 0, "offset")]
T_REC = 4                                                  # a record of 5 frames


@pytest.mark.parametrize("kind,n,n_obs", FORK_KINDS, ids=["-".join(map(str, c)) for c in FORK_KINDS])
def test_fork_equals_the_restatement(cuda, kind, n, n_obs):
    """every word of every output and of the guard band behind it; the inputs are random words (NaNs with payloads, values far
    outside [-1, 1]) and the grid lies outside the box: the fork moves words, it does not clip"""
    from dgppo_amd import engine as EN, ops_env as OE
    cfg = _cfg(kind, n, n_obs)
    step_f, env_f = OE.record_fields(cfg)
    assert ("hits" in step_f) == (cfg.is_lidar and cfg.n_obs > 0) and ("obst" in env_f) == (cfg.n_obs > 0)
    for case, (ids, F, nu, nv, HC, aid, source) in enumerate(FORK_SHAPES):
        rng = np.random.default_rng(1000 * case + 10 * n + n_obs)
        agent_id = aid % n
        us = torch.from_numpy(np.linspace(-1.75, 2.5, nu).astype(f32)).to(cuda)
        vs = torch.from_numpy((np.linspace(-3.0, 1.25, nv) if nv > 1 else np.array([-3.0])).astype(f32)).to(cuda)
        if source == "record":
            # the env-major views of a finalized record: env 1 of 2, frames at the record's own strides, the carry of frame t in
            # slot t + 1 of the [T + 2, n, HC] slab
            ro = EN.RolloutData(cfg, 2, T_REC, cuda, False, HC or 64)
            for t_ in list(ro.step_tm.values()) + list(ro.env.values()) + [ro.action_tm, ro.rnn_tm]:
                t_.copy_(_random_words(rng, tuple(t_.shape), cuda))
            ro.finalize()
            step = {k: v[1] for k, v in ro.step.items()}
            env = {k: v[1] for k, v in ro.env.items()}
            actions, carry = ro.actions[1], (ro._rnn_em[1, 1:] if HC else None)
            assert not HC or (carry.stride(0) == n * HC and carry.storage_offset() == (T_REC + 2) * n * HC + n * HC)
        else:
            step = {k: _offset_view(_random_words(rng, (T_REC + 1,) + s, cuda)) for k, s in step_f.items()}
            env = {k: _random_words(rng, s, cuda) for k, s in env_f.items()}
            actions = _offset_view(_random_words(rng, (T_REC, n, 2), cuda))
            carry = _offset_view(_random_words(rng, (T_REC + 1, n, HC), cuda)) if HC else None
            assert all(v.data_ptr() % 8 == 4 for v in list(step.values()) + [actions] + ([carry] if HC else []))
        G = F * nv * nu
        outs, bufs = {}, {}
        for k, s in {**step_f, **env_f}.items():
            outs[k], bufs[k] = _guarded((G,) + s, cuda)
        out = OE.State({k: outs[k] for k in step_f}, {k: outs[k] for k in env_f})
        action_out, bufs["action"] = _guarded((G, n, 2), cuda)
        carry_out = None
        if HC:
            carry_out, bufs["carry"] = _guarded((G * n, HC), cuda)
        OE.action_sweep_fork(cfg, step, env, actions, ids, F, agent_id, us, vs, out, action_out, carry, n * HC if HC else 0,
                             carry_out, frame_max=None)
        torch.cuda.synchronize()
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        want, want_action, want_carry = AR.fork_np(host(step), host(env), actions.cpu().numpy(), ids, F, agent_id,
                                                   us.cpu().numpy(), vs.cpu().numpy(), carry.cpu().numpy() if HC else None)
        tag = f"{kind} case {case}: frames {ids} grid {nu}x{nv} HC={HC} agent {agent_id} {source}"
        for k in outs:
            np.testing.assert_array_equal(_words(outs[k]), want[k], err_msg=f"{k} {tag}")
        np.testing.assert_array_equal(_words(action_out), want_action, err_msg=f"action {tag}")
        if HC:
            np.testing.assert_array_equal(_words(carry_out), want_carry, err_msg=f"carry {tag}")
        for k, b in bufs.items():
            guard = _words(b)[-GUARD:]
            assert (guard == SENTINEL).all(), f"{k}: the guard band was written ({tag})"
        # the grid action stands in row agent_id of every env as it was given
        got = action_out.view(F, nv, nu, n, 2)[:, :, :, agent_id]
        assert bool((got[..., 0] == us.view(1, 1, nu)).all()) and bool((got[..., 1] == vs.view(1, nv, 1)).all())


# ---- 2. the hand-made scene ---------------------------------------------------------------------------------------------------------
def _scene_record(cuda, mover):
    """the lookahead shield's scene as a one-frame record, filled by hand and finalized: frame 0 is the scene, the recorded action
    the zero action, slot 1 of the carries what the (zeroed) policy leaves after its forward on frame 0"""
    from dgppo_amd import engine as EN, ops_env as OE
    ocfg, agent, goal, obst = L.scene(mover)
    cfg, eng = _engine("LidarSpread", 2, 1, 1, cuda)
    eng.policy.params.zero_()
    eng.policy.prepare()
    n, HC = 2, eng.HC
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, f32)).to(cuda)
    ro = EN.RolloutData(cfg, 1, 1, cuda, False, HC)
    st = ro.states_tm[0]
    st.agent.copy_(d(agent))
    st.goal.copy_(d(goal))
    st.obst.copy_(d(obst))
    OE.sense(cfg, st)
    ro.action_tm.zero_()
    ro.rnn_tm[0].zero_()
    eng.policy.forward(eng._feats("la", st, 1), n_seq=n, T=1, h0=ro.rnn_tm[0].view(n, HC), tag="la", hs_out=ro.rnn_tm[1].view(n, HC),
                       train=False)
    OE.step(cfg, st, ro.action_tm[0], ro.states_tm[1], ro.reward_tm[0], ro.cost_tm[0])
    return eng, ro.finalize()


@pytest.mark.parametrize("mover", [0, 1])
def test_hand_made_scene(cuda, mover):
    """LidarSpread n = 2, obs = 1 (lookahead_np.scene) with a zeroed policy.  Sweeping the mover over SCENE_US x SCENE_VS at
    SCENE_H: its own row is the oracle's s of the grid candidates within 1e-5 (the bound test_core_on_a_hand_made_scene holds the
    same scene to) and the resting agent's row is -1 everywhere; sweeping the resting agent: its own row is -1 and h_others() the
    mover's doomed value everywhere.  The oracle gives the mover 0.53 / 0.55 for six grid actions and -0.524 for the three with
    u = -1: nothing sits near the threshold, the frame is decisive and 6 of 9 actions are doomed."""
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import ActionRolloutLandscape
    H, us, vs = L.SCENE_H, L.SCENE_US, L.SCENE_VS
    nu, nv = us.size, vs.size
    oracle = L.scene_oracle(mover)                                           # [1, 2, 1 + nv * nu]
    want = oracle[0, mover, 1:].reshape(nv, nu)
    assert ((np.abs(want) >= 0.5)).all() and int((want >= 0).sum()) == 6 and (want[:, 0] < 0).all()
    eng, ro = _scene_record(cuda, mover)
    rest = 1 - mover

    def sweep(agent):
        records = []
        value, worst = eng.action_rollout_landscape(ro, 0, agent, [0], us, vs, H, records=records)
        torch.cuda.synchronize()
        assert len(records) == 1 and records[0][:6] == (0, 1, 0, nv, 0, nu) and records[0][6].T == H + 1
        assert bool((records[0][6].action_tm[1:] == 0).all()), "the rolled policy plays the zero action"
        return ActionRolloutLandscape(us, vs, value.cpu().numpy(), worst.cpu().numpy(), np.zeros((1, 2), f32), agent,
                                      np.array([0]), H, float(eng.hp.gamma))
    R = sweep(mover)
    assert R.worst.shape == R.value.shape == (1, nv, nu, 2, 2)
    err = float(np.abs(R.h()[0].astype(np.float64) - want).max())
    print(f"mover {mover}: own-row h() max abs err against the oracle {err:.3e}; bit-equal: {np.array_equal(R.h()[0], want)}")
    assert err <= 1e-5
    np.testing.assert_array_equal(R.worst[0, :, :, rest, :].max(axis=-1), np.full((nv, nu), -1.0, f32))
    np.testing.assert_array_equal(R.h_others()[0], np.full((nv, nu), -1.0, f32))
    got = EV.action_rollout_agreement(R)
    assert got["points"].tolist() == [9] and got["doomed"].tolist() == [6] and got["decisive_frac"] == 1.0
    assert got["empty_frac"] == 0.0 and got["others_doomed_frac"] == 0.0 and got["others_decisive_frac"] == 0.0
    Q = sweep(rest)
    np.testing.assert_array_equal(Q.h()[0], np.full((nv, nu), -1.0, f32))
    err = float(np.abs(Q.h_others()[0].astype(np.float64) - float(oracle[0, mover, 0])).max())
    print(f"mover {mover}: h_others() of the resting agent's sweep: max abs err against the mover's doomed value {err:.3e}")
    assert err <= 1e-5 and oracle[0, mover, 0] >= 0.5
    got = EV.action_rollout_agreement(Q)
    assert got["doomed"].tolist() == [0] and got["decisive_frac"] == 0.0 and got["others_doomed_frac"] == 1.0


# ---- 3. the engine, every block record ------------------------------------------------------------------------------------------------
CASES = ENGINE_CASES + [("dgppo-n4-one-launch", "LidarSpread", 4, 2, "dgppo", True, 1)]


def _record_fields(ro, e):
    host = lambda d: {k: v[e].cpu().numpy() for k, v in d.items()}
    return host(ro.step), host(ro.env)


@pytest.mark.parametrize("name,kind,n,n_obs,algo,use_rnn,rnn_layers", CASES, ids=[c[0] for c in CASES])
def test_engine_block_records(cuda, name, kind, n, n_obs, algo, use_rnn, rnn_layers):
    """T = 4, B = 2, horizon 3, frames [2, 0], a 2 x 3 grid, env 1.  From the block record: slot 0, action[0] and rnn[1] are the
    restated fork of the record bit for bit, states[k + 1] is ops_env.step(states[k], action[k]) bit for bit for every k, and
    value / worst the restated fold of its cost_tm[1:4] bit for bit"""
    T_, B, H, frames, e = 4, 2, 3, [2, 0], 1
    cfg, eng = _engine(kind, n, n_obs, T_, cuda, use_rnn, rnn_layers, algo)
    if name.endswith("one-launch"):
        assert eng.fused_step, "this case is here for the one-launch step"
    HC = eng.HC
    us, vs = np.array([-0.5, 1.0], f32), np.array([-1.0, 0.25, 0.75], f32)
    nu, nv = 2, 3
    for stochastic in (False, True):
        ro = eng.rollout(torch.tensor([9, 10], dtype=torch.int64, device=cuda), stochastic, 5)
        records = []
        agent_id = n - 1 if stochastic else 0
        value, worst = eng.action_rollout_landscape(ro, e, agent_id, frames, us, vs, H, records=records)
        torch.cuda.synchronize()
        assert tuple(value.shape) == tuple(worst.shape) == (2, nv, nu, n, cfg.n_cost)
        assert len(records) == 1 and records[0][:6] == (0, 2, 0, nv, 0, nu)
        rec = records[0][6]
        G = 2 * nv * nu
        assert rec.B == G and rec.T == H + 1
        step, env = _record_fields(ro, e)
        carry = ro.rnn_tm[1:, e].cpu().numpy() if use_rnn else None          # slot t: after frame t's forward
        want, want_action, want_carry = AR.fork_np(step, env, ro.action_tm[:, e].cpu().numpy(), frames, 2, agent_id, us, vs, carry)
        tag = f"{name} {'stochastic' if stochastic else 'deterministic'}"
        for k, v in {**rec.states_tm[0].step, **rec.states_tm[0].env}.items():
            np.testing.assert_array_equal(_words(v), want[k], err_msg=f"{tag}: slot 0 {k}")
        np.testing.assert_array_equal(_words(rec.action_tm[0]), want_action, err_msg=f"{tag}: the forced joint action")
        if use_rnn:
            np.testing.assert_array_equal(_words(rec.rnn_tm[1]).reshape(-1, HC), want_carry, err_msg=f"{tag}: rnn[1]")
        for k in range(H + 1):
            _step_check(cfg, rec.states_tm[k], rec.action_tm[k], rec.states_tm[k + 1], f"{tag}: block states[{k + 1}]")
        wv, ww = AR.fold_np(rec.cost_tm[1:H + 1].cpu().numpy(), eng.hp.gamma)
        L.assert_same_words(value.cpu().numpy().reshape(G, n, -1), wv, f"{tag}: value")
        L.assert_same_words(worst.cpu().numpy().reshape(G, n, -1), ww, f"{tag}: worst")
        assert np.isfinite(ww).all()


# ---- 4. against the lookahead shield's core -----------------------------------------------------------------------------------------
def test_own_row_is_the_lookahead_shields_s(cuda):
    """a deterministic record: for every frame t and agent i, Engine.lookahead_select on (state t, the carry after its forward,
    the recorded actions) judges the same (state, action) pairs.  Its s[e, i, 1 + iv * nu + iu] and the own-row maximum of
    worst[f, iv, iu, i, :] agree within 1e-5, the bound the suite holds the same envs replayed in another batch size to at
    horizon 3 (test_engine_rollout_lookahead_shielded)."""
    from dgppo_amd import ops_nn as K_
    T_, B, H, n = 4, 2, 3, 3
    cfg, eng = _engine("LidarSpread", n, 2, T_, cuda)
    HC = eng.HC
    us, vs = np.array([-1.0, 0.0, 1.0], f32), np.array([-0.5, 0.5], f32)
    nu, nv = 3, 2
    P = 1 + nu * nv
    ro = eng.rollout(torch.tensor([3, 4], dtype=torch.int64, device=cuda), False)
    d_us, d_vs = K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda)
    s_all = torch.full((T_, B, n, P), float("nan"), device=cuda)
    for t in range(T_):
        action = torch.empty(B, n, 2, device=cuda)
        index = torch.empty(B, n, dtype=torch.int32, device=cuda)
        flag = torch.empty(B, n, dtype=torch.int32, device=cuda)
        eng.lookahead_select(ro.states_tm[t], ro.rnn_tm[t + 1].view(B * n, HC), ro.action_tm[t], d_us, d_vs, H, 0.0, action, index,
                             flag, s_all[t])
    s_all = s_all.cpu().numpy()
    worst_err, equal = 0.0, True
    for e in range(B):
        for i in range(n):
            _, worst = eng.action_rollout_landscape(ro, e, i, np.arange(T_), us, vs, H)
            own = worst[:, :, :, i, :].cpu().numpy().max(axis=-1)            # [T, nv, nu]
            want = s_all[:, e, i, 1:].reshape(T_, nv, nu)
            assert np.isfinite(own).all() and np.isfinite(want).all()
            worst_err = max(worst_err, float(np.abs(own.astype(np.float64) - want).max()))
            equal = equal and np.array_equal(own, want)
    print(f"own row vs lookahead_select's s: max abs err {worst_err:.3e}; bit-equal: {equal}")
    assert worst_err <= 1e-5


# ---- 5. replay --------------------------------------------------------------------------------------------------------------------------
def test_the_recorded_action_replays_the_record(cuda):
    """us = [a_u], vs = [a_v], the deterministic record's own action of (t, i): the what-if env is the episode itself, so the
    block record's cost_tm[1:4] is the record's cost_tm[t + 1 : t + 4] of that env within 1e-5 (the same envs in another batch
    size), for every t with t + 3 <= T - 1"""
    T_, B, H, n = 5, 2, 3, 3
    cfg, eng = _engine("LidarSpread", n, 2, T_, cuda)
    ro = eng.rollout(torch.tensor([5, 6], dtype=torch.int64, device=cuda), False)
    acts = ro.action_tm.cpu().numpy()
    cost = ro.cost_tm.cpu().numpy()
    worst_err = 0.0
    for t in range(T_ - H):
        for e in range(B):
            for i in range(n):
                records = []
                eng.action_rollout_landscape(ro, e, i, [t], acts[t, e, i, :1], acts[t, e, i, 1:], H, records=records)
                rec = records[0][6]
                assert rec.B == 1
                got = rec.cost_tm[1:H + 1, 0].cpu().numpy()
                worst_err = max(worst_err, float(np.abs(got.astype(np.float64) - cost[t + 1:t + 1 + H, e]).max()))
                np.testing.assert_array_equal(_words(rec.action_tm[0, 0]), acts[t, e].view(np.uint32))
    print(f"replay: max abs err of the block record's costs against the record's {worst_err:.3e}")
    assert worst_err <= 1e-5


# ---- 6. walks ---------------------------------------------------------------------------------------------------------------------------
def test_walks_give_every_word_again(cuda):
    """prepass_graphs shrunk so that a block holds one frame, one row of a frame, less than a row, and set to 1 (one env per
    block): every word of value / worst is the same"""
    T_, H, n = 4, 3, 3
    cfg, eng = _engine("LidarSpread", n, 2, T_, cuda)
    ro = eng.rollout(torch.tensor([7, 8], dtype=torch.int64, device=cuda), True, 3)
    us, vs = np.array([-1.0, 0.0, 1.0], f32), np.array([-0.5, 0.5], f32)       # 6 envs a frame, rows of 3
    frames = [3, 1, 2]
    base = eng.action_rollout_landscape(ro, 0, 1, frames, us, vs, H)
    cap = eng.prepass_graphs
    walks = {"one frame": (6 * (H + 2), [(f, f + 1, 0, 2, 0, 3) for f in range(3)]),
             "one row": (3 * (H + 2), [(f, f + 1, v, v + 1, 0, 3) for f in range(3) for v in range(2)]),
             "less than a row": (2 * (H + 2), [(f, f + 1, v, v + 1, u, min(u + 2, 3)) for f in range(3) for v in range(2)
                                               for u in (0, 2)]),
             "prepass_graphs = 1": (1, [(f, f + 1, v, v + 1, u, u + 1) for f in range(3) for v in range(2) for u in range(3)])}
    try:
        for what, (graphs, blocks) in walks.items():
            eng.prepass_graphs = graphs
            records = []
            got = eng.action_rollout_landscape(ro, 0, 1, frames, us, vs, H, records=records)
            assert [r[:6] for r in records] == blocks, what
            _same_words(got[0], base[0], f"{what}: value")
            _same_words(got[1], base[1], f"{what}: worst")
    finally:
        eng.prepass_graphs = cap


# ---- 7. the surface -----------------------------------------------------------------------------------------------------------------------
def _algo(name, n, Tn):
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    env = make_env(env_id="LidarSpread", num_agents=n, num_obs=1, max_step=Tn)
    algo = make_algo(algo=name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=n, cost_weight=0.0, actor_gnn_layers=2, Vl_gnn_layers=2, Vh_gnn_layers=1,
                     lr_actor=3e-4, lr_Vl=1e-3, max_grad_norm=2.0, seed=3, use_rnn=True, rnn_layers=1, use_lstm=False, alpha=10.0,
                     batch_size=4 * Tn, rnn_step=Tn, train_steps=1)
    return env, algo


def test_algo_action_rollout_landscape(cuda):
    from dgppo_amd.trainer.data import ActionRolloutLandscape, Rollout
    n, Tn = 2, 4
    env, algo = _algo("informarl", n, Tn)
    sig = inspect.signature(algo.action_rollout_landscape).parameters
    assert [(k, sig[k].default) for k in ("frames", "nu", "nv", "us", "vs", "horizon")] == \
        [("frames", None), ("nu", 32), ("nv", 32), ("us", None), ("vs", None), ("horizon", 32)]
    keys = np.random.default_rng(3).integers(1, 2 ** 62, size=2)
    ro = algo.collect_deterministic(keys, env=env)
    R = algo.action_rollout_landscape(ro, 1, 1, frames=[0, 3], nu=3, nv=2, horizon=2)
    assert isinstance(R, ActionRolloutLandscape) and R.agent == 1 and R.horizon == 2 and R.gamma == float(algo.engine.hp.gamma)
    assert R.value.shape == R.worst.shape == (2, 2, 3, n, 2) and R.value.dtype == R.worst.dtype == f32
    np.testing.assert_array_equal(R.us, np.linspace(-1.0, 1.0, 3).astype(f32))
    np.testing.assert_array_equal(R.vs, np.linspace(-1.0, 1.0, 2).astype(f32))
    assert R.frames.tolist() == [0, 3] and R.frames.dtype == np.int64 and R.h().shape == R.h_others().shape == (2, 2, 3)
    np.testing.assert_array_equal(R.actions, np.clip(ro.actions[1, [0, 3], 1].cpu().numpy(), -1.0, 1.0))
    full = algo.action_rollout_landscape(ro, 0, 0, nu=2, nv=2, horizon=1)              # frames default to all of them
    assert full.frames.tolist() == list(range(Tn)) and full.worst.shape == (Tn, 2, 2, n, 2)
    st = algo.collect_stochastic(keys, env=env)                                       # a stochastic record serves as well
    assert algo.action_rollout_landscape(st, 0, 1, frames=[Tn - 1], nu=2, nv=2, horizon=2).value.shape == (1, 2, 2, n, 2)
    with pytest.raises(ValueError, match="needs a Rollout produced by this algo"):
        algo.action_rollout_landscape(Rollout(*ro)._replace(actions=ro.actions.clone()), 0, 0, nu=2, nv=2, horizon=1)
    for kw, match in ((dict(horizon=0), "horizon"), (dict(nu=0), "us"), (dict(vs=[]), "vs"), (dict(frames=[Tn]), "frame_ids"),
                      (dict(frames=[-1]), "frame_ids"), (dict(index=2), "env_index"), (dict(agent=n), "agent_id")):
        args = dict(index=0, agent=0, frames=[0], nu=2, nv=2, horizon=1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            algo.action_rollout_landscape(ro, **args)


def test_vmas_engine_refuses(cuda):
    from dgppo_amd import _native as N, engine as EN
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="action_rollout_landscape: VMASReverseTransport is not supported"):
        vmas.action_rollout_landscape(None, 0, 0, [0], [0.5], [0.5], 1)


BASE_KEYS = ["points", "doomed", "doomed_frac", "empty_frames", "empty_frac", "decisive_frac", "others_doomed_frac",
             "others_decisive_frac"]
BARRIER_KEYS = ["missed", "conservative", "missed_frac", "conservative_frac"]


@pytest.mark.parametrize("algo_name", ["informarl", "dgppo"])
def test_cli_writes_the_action_rollout_landscape(cuda, tmp_path, capsys, algo_name):
    """a saved two-episode run: the flag alone creates the videos directory, writes the .npz with every field of the record and
    every statistic and prints the line; with a dgppo run and --action-landscape for the same agent the line and the file carry
    the learned barrier's missed_frac / conservative_frac"""
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import ActionRolloutLandscape
    n, grid, Tn, H = 2, 3, 3, 2
    run = _run_dir(tmp_path, algo_name, n, Tn)
    mod = _load_test_py()
    common = ["--path", str(run), "--epi", "2", "--no-video", "--max-step", str(Tn), "--action-rollout-landscape", "1",
              "--landscape-grid", str(grid), "--rollout-horizon", str(H)]
    barrier = algo_name == "dgppo"
    mod.main(common + (["--action-landscape", "1"] if barrier else ["--stochastic"]))
    printed = capsys.readouterr().out
    for word in ("(doomed_frac)", "(decisive_frac)", "(others_doomed_frac", "others_decisive_frac)", "action rollout landscape: "):
        assert printed.count(word) == 2, word
    assert printed.count("(missed_frac)") == (2 if barrier else 0) and printed.count("(conservative_frac)") == (2 if barrier else 0)
    files = sorted(glob.glob(str(run / "videos" / "0" / "*_action_rollout.npz")))
    assert len(files) == 2
    lin = np.linspace(-1.0, 1.0, grid).astype(f32)
    for path in files:
        z = np.load(path)
        assert sorted(z.files) == sorted([*ActionRolloutLandscape._fields, *BASE_KEYS, *(BARRIER_KEYS if barrier else [])])
        R = ActionRolloutLandscape(*(z[k] for k in ActionRolloutLandscape._fields))
        np.testing.assert_array_equal(R.us, lin)
        np.testing.assert_array_equal(R.vs, lin)
        assert R.value.shape == R.worst.shape == (Tn, grid, grid, n, 2) and R.actions.shape == (Tn, 2)
        assert int(R.agent) == 1 and int(R.horizon) == H and R.frames.tolist() == list(range(Tn))
        for key, v in EV.action_rollout_agreement(R).items():
            np.testing.assert_array_equal(z[key], v)
    if not barrier:                                                       # with either shield, too
        mod.main(common + ["--shield", "--shield-horizon", "2", "--shield-grid", "2"])
        assert capsys.readouterr().out.count("action rollout landscape: ") == 2
