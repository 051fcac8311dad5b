"""Lookahead shield rounds on the device: dgppo_env_team_action_fork_ids and dgppo_lookahead_reselect against the NumPy restatement
(tests/lookahead_rounds_np.py) and against the one-shot entry points, Engine.lookahead_select_rounds on scene A against
oracle/env_np.py, Engine.rollout_lookahead_shielded(rounds=3) re-derived round by round from its block records, and
test.py --shield-rounds in-process."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lookahead_np as L  # noqa: E402
import lookahead_rounds_np as R  # noqa: E402
from test_lookahead_shield_gpu import (_cfg, _engine, _load_test_py, _record_words, _run_dir, _same_words, _step_check,  # noqa: E402
                                       _words)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32


def _d(x, cuda, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(cuda)


# ---- 1. the fork from a list of envs ------------------------------------------------------------------------------------------------
# rows of 12 / 48 / 32 words (16-byte vectors, hits), of 8 and 12 without hits, and of 10 (the bicycle's five columns: 8-byte)
FORK_KINDS = [("LidarSpread", 3, 2), ("MPESpread", 2, 3), ("LidarBicycleTarget", 2, 1)]


@pytest.mark.parametrize("kind,n,n_obs", FORK_KINDS, ids=["-".join(map(str, c)) for c in FORK_KINDS])
def test_fork_ids_equals_the_restatement(cuda, kind, n, n_obs):
    """B = 5; the lists [3], [0, 2, 4] and every env; grids 1 x 1 and 3 x 3 (G from 4 to 150: below one tile of 64 envs, and
    several with a ragged last one); with a carry of 64 and without (the action buffer then starts at an odd word).  Every word of
    every output; a_base holds a value outside [-1, 1] and a NaN with a payload in listed envs: words move, nothing is clipped.
    Without a list the outputs are dgppo_env_team_action_fork's, word for word"""
    from dgppo_amd import ops_env as OE, ops_nn as K_
    cfg = _cfg(kind, n, n_obs)
    B = 5
    st = OE.State.empty(cfg, B, cuda)
    OE.reset(cfg, torch.arange(B, dtype=torch.int64, device=cuda) + 31, st)
    fields = {k: v.cpu().numpy() for k, v in {**st.step, **st.env}.items()}
    assert ("hits" in fields) == (cfg.is_lidar and n_obs > 0)
    for ids in ([3], [0, 2, 4], None):
        for nu, nv in ((1, 1), (3, 3)):
            for HC in (64, None):
                rng = np.random.default_rng(nu * 10 + (HC or 0))
                a_base = rng.uniform(-1.0, 1.0, size=(B, n, 2)).astype(f32)
                a_base[3, 0, 0] = 3.5
                a_base.view(np.uint32)[3, n - 1, 1] = 0x7FC12345                 # a NaN with a payload
                us = np.linspace(-1.0, 1.0, nu).astype(f32) if nu > 1 else np.array([1.75], f32)
                vs = np.linspace(-1.0, 1.0, nv).astype(f32) if nv > 1 else np.array([-0.3], f32)
                carry = rng.standard_normal((B * n, HC)).astype(f32) if HC else None
                M = B if ids is None else len(ids)
                P = 1 + nu * nv
                G = M * n * P

                def run(fork, *lead):
                    out = OE.State.empty(cfg, G, cuda)
                    for v in list(out.step.values()) + list(out.env.values()):
                        v.fill_(float("nan"))
                    action = torch.full((G * n * 2 + 1,), float("nan"), device=cuda)[0 if HC else 1:][:G * n * 2].view(G, n, 2)
                    carry_out = torch.full((G * n, HC), float("nan"), device=cuda) if HC else None
                    fork(cfg, st, _d(a_base, cuda), *lead, K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda), out, action,
                         _d(carry, cuda) if HC else None, carry_out)
                    torch.cuda.synchronize()
                    return out, action, carry_out
                out, action, carry_out = run(OE.team_action_fork_ids, None if ids is None else np.array(ids))
                want, want_action, want_carry = R.fork_ids_np(fields, a_base, ids, us, vs, carry)
                tag = f"{kind} ids={ids} grid {nu}x{nv} HC={HC}"
                for k, v in {**out.step, **out.env}.items():
                    np.testing.assert_array_equal(_words(v), want[k], err_msg=f"{k} {tag}")
                np.testing.assert_array_equal(_words(action), want_action, err_msg=f"action {tag}")
                if HC:
                    np.testing.assert_array_equal(_words(carry_out), want_carry, err_msg=f"carry {tag}")
                m3 = 3 if ids is None else ids.index(3) if 3 in ids else None
                if m3 is not None:
                    g = (m3 * n + 1) * P                                         # agent 1's candidate 0: rows 0 and n - 1 are a_base's
                    assert float(action[g, 0, 0]) == 3.5 and int(_words(action)[m3 * n * P, n - 1, 1]) == 0x7FC12345
                if ids is None:
                    out1, action1, carry1 = run(OE.team_action_fork)
                    for k, v in {**out.step, **out.env}.items():
                        _same_words(v, {**out1.step, **out1.env}[k], f"{k} {tag} vs team_action_fork")
                    _same_words(action, action1, f"action {tag} vs team_action_fork")
                    if HC:
                        _same_words(carry_out, carry1, f"carry {tag} vs team_action_fork")


# ---- 2. the reselect kernel ---------------------------------------------------------------------------------------------------------
SENT = -7


def _reselect(cuda, cost, stride_pad, ids, a_ref, us, vs, margin, mode, action, index, want_s=True):
    """cost [K, G, n, nh] handed over as slots 1 .. K of a [K + 1, G * n * nh + stride_pad] buffer; flag / joint / changed / s start
    as sentinels -> numpy (action, index, flag, joint, changed, s)"""
    from dgppo_amd import ops_nn as K_
    Kk, G, n, nh = cost.shape
    E = a_ref.shape[0]
    P = 1 + len(us) * len(vs)
    buf = torch.full((Kk + 1, G * n * nh + stride_pad), float("nan"), device=cuda)
    cost_tm = buf[1:, :G * n * nh].view(Kk, G, n, nh)
    cost_tm.copy_(_d(cost, cuda))
    act, idx = _d(action, cuda), _d(index, cuda, np.int32)
    flag = torch.full((E, n), SENT, dtype=torch.int32, device=cuda)
    joint = torch.full((E,), SENT, dtype=torch.int32, device=cuda)
    changed = torch.full((E,), SENT, dtype=torch.int32, device=cuda)
    s = torch.full((E, n, P), float(SENT), device=cuda) if want_s else None
    K_.lookahead_reselect(cost_tm, None if ids is None else np.array(ids), _d(a_ref, cuda), K_.sweep_axis(us, "us", cuda),
                          K_.sweep_axis(vs, "vs", cuda), margin, mode, act, idx, flag, joint, changed, s)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (act, idx, flag, joint, changed, s))


def _random_costs(rng, Kk, M, n, P, nh):
    """costs of the environment's kind (-1 .. -0.5 and 0.5 .. 1), the share of unsafe words differing per (env, agent), a sprinkle
    of NaN; the last listed env's first agent has nothing finite"""
    G = M * n * P
    mag = rng.uniform(0.5, 1.0, size=(Kk, G, n, nh))
    share = rng.uniform(0.0, 0.25, size=(1, M, n, 1, 1, 1)) ** 2
    unsafe = rng.uniform(size=(Kk, M, n, P, n, nh)) < share
    cost = np.where(unsafe.reshape(Kk, G, n, nh), mag, -mag).astype(f32)
    cost[rng.uniform(size=cost.shape) < 0.01] = np.nan
    cost.reshape(Kk, M, n, P, n, nh)[:, M - 1, 0, :, 0] = np.nan
    return cost


EQ_CASES = [(1, 1, 1, 1, 1, 0), (3, 2, 5, 3, 3, 24), (1, 3, 3, 2, 9, 0)]


@pytest.mark.parametrize("Kk,nh,E,n,grid,pad", EQ_CASES, ids=[f"K{c[0]}-nh{c[1]}-E{c[2]}-n{c[3]}-grid{c[4]}-pad{c[5]}" for c in EQ_CASES])
def test_reselect_round_zero_equals_lookahead_select(cuda, Kk, nh, E, n, grid, pad):
    """mode 0, no list, a_ref = action = a_pol, index = 0: action, index, flag and s are dgppo_lookahead_select's words"""
    from dgppo_amd import ops_nn as K_
    rng = np.random.default_rng(Kk * 1000 + nh * 100 + E * 10 + n)
    us = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([0.25], f32)
    vs = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([-0.5], f32)
    P = 1 + grid * grid
    cost = _random_costs(rng, Kk, E, n, P, nh)
    a_pol = rng.uniform(-1.3, 1.3, size=(E, n, 2)).astype(f32)
    for margin in (0.0, 0.75):
        act, idx, flag, joint, changed, s = _reselect(cuda, cost, pad, None, a_pol, us, vs, margin, 0, a_pol, np.zeros((E, n), np.int32))
        G = E * n * P
        buf = torch.full((Kk + 1, G * n * nh + pad), float("nan"), device=cuda)
        cost_tm = buf[1:, :G * n * nh].view(Kk, G, n, nh)
        cost_tm.copy_(_d(cost, cuda))
        a1 = torch.full((E, n, 2), float("nan"), device=cuda)
        i1 = torch.full((E, n), SENT, dtype=torch.int32, device=cuda)
        f1 = torch.full((E, n), SENT, dtype=torch.int32, device=cuda)
        s1 = torch.full((E, n, P), float("nan"), device=cuda)
        K_.lookahead_select(cost_tm, _d(a_pol, cuda), K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda), margin, a1, i1, f1, s1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(act.view(np.uint32), _words(a1), err_msg="action")
        np.testing.assert_array_equal(idx, i1.cpu().numpy(), err_msg="index")
        np.testing.assert_array_equal(flag, f1.cpu().numpy(), err_msg="flag")
        L.assert_same_words(s, s1.cpu().numpy(), "s")
        np.testing.assert_array_equal(changed, (idx != 0).any(axis=1))
        np.testing.assert_array_equal(joint, np.where(changed == 1, 0, np.where((flag == 2).any(axis=1), 1, 2)))


RS_CASES = [(1, 1, 1, 1, 0), (3, 2, 2, 3, 8), (3, 3, 3, 3, 0), (1, 2, 3, 9, 4), (3, 3, 2, 9, 0), (1, 3, 1, 3, 4)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Kk,nh,n,grid,pad", RS_CASES, ids=[f"K{c[0]}-nh{c[1]}-n{c[2]}-grid{c[3]}-pad{c[4]}" for c in RS_CASES])
def test_reselect_random(cuda, Kk, nh, n, grid, pad, mode):
    """E = 5 with the list [1, 4]: the rows of envs 0, 2 and 3 keep their sentinels in every output.  The action held differs from
    the policy's (some rows hold a grid action with its index, one lies outside the box), P = 2, 10 and 82 (a second pass over the
    64 lanes), margins 0, 0.75 and -2, NaN costs; with and without the s output"""
    rng = np.random.default_rng(Kk * 1000 + nh * 100 + n * 10 + grid + mode)
    E, ids = 5, [1, 4]
    us = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([0.25], f32)
    vs = np.linspace(-1.0, 1.0, grid).astype(f32) if grid > 1 else np.array([-0.5], f32)
    P = 1 + grid * grid
    cost = _random_costs(rng, Kk, len(ids), n, P, nh)
    a_ref = rng.uniform(-1.3, 1.3, size=(E, n, 2)).astype(f32)
    index = np.where(rng.uniform(size=(E, n)) < 0.5, rng.integers(1, P, size=(E, n)), 0).astype(np.int32)
    held = np.where((index > 0)[..., None], L.grid_actions(us, vs)[np.maximum(index - 1, 0)], a_ref).astype(f32)
    held[2] = SENT                                                                # an env that is not listed
    seen = set()
    for margin in (0.0, 0.75, -2.0):
        act, idx, flag, joint, changed, s = _reselect(cuda, cost, pad, ids, a_ref, us, vs, margin, mode, held, index)
        want_s = L.fold_np(cost, len(ids), n, P)
        L.assert_same_words(s[ids], want_s, f"margin {margin}: s")
        wa, wi, wf, wj, wc = R.reselect_np(want_s, ids, a_ref, us, vs, margin, mode, held, index, flag=np.full((E, n), SENT),
                                           joint=np.full(E, SENT), changed=np.full(E, SENT))
        np.testing.assert_array_equal(act.view(np.uint32), wa.view(np.uint32), err_msg=f"margin {margin}: action")
        np.testing.assert_array_equal(idx, wi, err_msg=f"margin {margin}: index")
        np.testing.assert_array_equal(flag, wf, err_msg=f"margin {margin}: flag")
        np.testing.assert_array_equal(joint, wj, err_msg=f"margin {margin}: joint")
        np.testing.assert_array_equal(changed, wc, err_msg=f"margin {margin}: changed")
        rest = [0, 2, 3]
        assert (flag[rest] == SENT).all() and (joint[rest] == SENT).all() and (changed[rest] == SENT).all() and (s[rest] == SENT).all()
        assert np.array_equal(act[rest].view(np.uint32), held[rest].view(np.uint32)) and np.array_equal(idx[rest], index[rest])
        if mode == 1:
            assert ((idx[ids] != index[ids]).sum(axis=1) <= 1).all(), "one mover"
        a2, i2, f2, j2, c2, none = _reselect(cuda, cost, pad, ids, a_ref, us, vs, margin, mode, held, index, want_s=False)
        assert none is None and np.array_equal(i2, idx) and np.array_equal(f2, flag) and np.array_equal(j2, joint), "without s"
        seen |= set(joint[ids].tolist())
    if n > 1:
        assert 0 in seen


# ---- 3. scene A through the engine ----------------------------------------------------------------------------------------------------
def test_rounds_on_scene_a(cuda):
    """LidarSpread n = 2, obs = 1 (lookahead_rounds_np.scene_a), the policy's parameters zeroed: its action is exactly 0.
    rounds = 1 is today's shield: index (2, 2), both dodge down — a joint action that collides.  rounds = 4 reaches (0, 0) /
    (0, -1) in three rounds: the CPU test's values, word for word"""
    from dgppo_amd import ops_env as OE, ops_nn as K_
    H, us, vs = R.SCENE_A_H, R.SCENE_A_US, R.SCENE_A_VS
    ocfg, agent, goal, obst = R.scene_a()
    zero = np.zeros((1, 2, 2), f32)
    want1 = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 1)
    want4 = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 4)
    assert want1["index"].tolist() == [[2, 2]] and want4["rounds_used"].tolist() == [3] and want4["joint"].tolist() == [2]
    cfg, eng = _engine("LidarSpread", 2, 1, 4, cuda)
    eng.policy.params.zero_()
    eng.policy.prepare()
    st = OE.State({"agent": _d(agent, cuda)}, {"goal": _d(goal, cuda), "obst": _d(obst, cuda)})
    OE.sense(cfg, st)
    n, HC, P = 2, eng.HC, 10
    carry_next = torch.full((n, HC), float("nan"), device=cuda)
    act = eng.policy.forward(eng._feats("la", st, 1), n_seq=n, T=1, h0=torch.zeros(n, HC, device=cuda), tag="la",
                             hs_out=carry_next, train=False)
    a_pol = torch.full((1, n, 2), float("nan"), device=cuda)
    K_.policy_head(act["ms"], None, None, a_pol.view(n, 2), None, None, n, 1)
    torch.cuda.synchronize()
    assert bool((a_pol == 0).all()), "zero parameters give the zero action"
    dus, dvs = K_.sweep_axis(us, "us", cuda), K_.sweep_axis(vs, "vs", cuda)
    for rounds, want in ((1, want1), (4, want4)):
        action = torch.full((1, n, 2), float("nan"), device=cuda)
        index = torch.full((1, n), SENT, dtype=torch.int32, device=cuda)
        flag = torch.full((1, n), SENT, dtype=torch.int32, device=cuda)
        s = torch.full((1, n, P), float("nan"), device=cuda)
        joint = torch.full((1,), SENT, dtype=torch.int32, device=cuda)
        used = torch.full((1,), SENT, dtype=torch.int32, device=cuda)
        records = []
        eng.lookahead_select_rounds(st, carry_next, a_pol, dus, dvs, H, 0.0, rounds, action, index, flag, s, joint, used,
                                    records=records, t=5)
        torch.cuda.synchronize()
        got_s = s.cpu().numpy()
        print(f"rounds {rounds}: s bit-equal to the oracle's: {np.array_equal(got_s, want['s'])}; index {index.tolist()}, "
              f"joint {joint.tolist()}, rounds_used {used.tolist()}, s[.., 0] {got_s[0, :, 0].tolist()}")
        assert index.tolist() == want["index"].tolist() and flag.tolist() == want["flag"].tolist()
        assert joint.tolist() == want["joint"].tolist() and used.tolist() == want["rounds_used"].tolist()
        np.testing.assert_array_equal(_words(action), want["action"].view(np.uint32))
        err = float(np.abs(got_s.astype(np.float64) - want["s"]).max())
        assert err <= 1e-5, f"rounds {rounds}: s is {err:.3e} off the oracle's"
        assert [(r[0], r[1], r[2].tolist()) for r in records] == [(5, r, [0]) for r in range(len(want["trace"]))]
        for (_, r, _, rec), tr in zip(records, want["trace"]):
            assert rec.T == H + 1 and rec.B == n * P
            assert bool((rec.action_tm[1:] == 0).all()), "the rolled policy plays the zero action"
            fold = L.fold_np(rec.cost_tm[1:H + 1].cpu().numpy(), 1, n, P)
            assert float(np.abs(fold.astype(np.float64) - tr[1]).max()) <= 1e-5, f"rounds {rounds}: round {r} fold"
    assert index.tolist() == [[5, 2]] and used.tolist() == [3] and joint.tolist() == [2]
    assert got_s[0, :, 0].tolist() == [R.SCENE_A_SAFE, R.SCENE_A_SAFE]
    np.testing.assert_array_equal(action.cpu().numpy(), [[[0.0, 0.0], [0.0, -1.0]]])


# ---- 4. the engine ------------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = [("dgppo", "LidarSpread", 3, 2, "dgppo", True), ("informarl-no-rnn", "LidarSpread", 3, 2, "informarl", False)]


def _derive(cfg, eng, ro, log, records, us, vs, H, margin, rounds, use_rnn, name):
    """every block record, round by round: the fork is the restated one from the joint action held, every step of the record is
    ops_env.step's, the selection the restated rule on the restated fold, the next list the envs that changed; what is left after
    the last round is the log.  -> the rounds used, summed over the steps"""
    n, HC = cfg.n_agents, eng.HC
    T_, B = log["index"].shape[:2]
    P = 1 + len(us) * len(vs)
    pol = log["policy_action"].cpu().numpy()
    total = 0
    for t in range(T_):
        st = ro.states_tm[t]
        fields = {k: v.cpu().numpy() for k, v in {**st.step, **st.env}.items()}
        carry = ro.rnn_tm[t + 1].reshape(B * n, HC).cpu().numpy() if use_rnn else None
        A, index = pol[t].copy(), np.zeros((B, n), np.int32)
        flag, joint = np.zeros((B, n), np.int32), np.zeros(B, np.int32)
        s_all, used = np.zeros((B, n, P), f32), np.zeros(B, np.int32)
        ids = np.arange(B)
        mine = [r for r in records if r[0] == t]
        for r in range(rounds):
            blocks = [b for b in mine if b[1] == r]
            assert np.concatenate([b[2] for b in blocks]).tolist() == ids.tolist(), f"{name} t={t} round {r}: the active list"
            changed = np.zeros(B, np.int32)
            A_next, index_next = A, index
            for _, _, blk, rec in blocks:
                tag = f"{name} t={t} round {r} block {blk.tolist()}"
                G = blk.size * n * P
                assert rec.B == G and rec.T == H + 1
                want, want_action, want_carry = R.fork_ids_np(fields, A, blk, us, vs, carry)
                for k, v in {**rec.states_tm[0].step, **rec.states_tm[0].env}.items():
                    np.testing.assert_array_equal(_words(v), want[k], err_msg=f"{tag}: slot 0 {k}")
                np.testing.assert_array_equal(_words(rec.action_tm[0]), want_action, err_msg=f"{tag}: the forced joint action")
                if use_rnn:
                    np.testing.assert_array_equal(_words(rec.rnn_tm[1]).reshape(-1, HC), want_carry, err_msg=f"{tag}: rnn[1]")
                for k in range(H + 1):
                    _step_check(cfg, rec.states_tm[k], rec.action_tm[k], rec.states_tm[k + 1], f"{tag}: block states[{k + 1}]")
                s = L.fold_np(rec.cost_tm[1:H + 1].cpu().numpy(), blk.size, n, P)
                s_all[blk] = s
                A_next, index_next, flag, joint, changed = R.reselect_np(s, blk, pol[t], us, vs, margin, 0 if r == 0 else 1, A_next,
                                                                         index_next, flag, joint, changed)
            used[ids] += 1
            A, index = A_next, index_next
            ids = np.flatnonzero(changed)
            if ids.size == 0:
                break
        assert len(mine) == sum(1 for b in mine if b[1] <= r), f"{name} t={t}: rounds after the last one"
        np.testing.assert_array_equal(_words(ro.action_tm[t]), A.view(np.uint32), err_msg=f"{name}: action[{t}]")
        np.testing.assert_array_equal(log["index"][t].cpu().numpy(), index, err_msg=f"{name}: index[{t}]")
        np.testing.assert_array_equal(log["flag"][t].cpu().numpy(), flag, err_msg=f"{name}: flag[{t}]")
        np.testing.assert_array_equal(log["joint"][t].cpu().numpy(), joint, err_msg=f"{name}: joint[{t}]")
        np.testing.assert_array_equal(log["rounds_used"][t].cpu().numpy(), used, err_msg=f"{name}: rounds_used[{t}]")
        L.assert_same_words(log["s"][t].cpu().numpy(), s_all, f"{name}: s[{t}]")
        _step_check(cfg, ro.states_tm[t], ro.action_tm[t], ro.states_tm[t + 1], f"{name}: states[{t + 1}]")
        total += int(used.sum())
    return total


@pytest.mark.parametrize("name,kind,n,n_obs,algo,use_rnn", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_rollout_lookahead_shielded_rounds(cuda, name, kind, n, n_obs, algo, use_rnn):
    """T = 3, B = 3, H = 3, rounds = 3, a 3 x 3 grid, at margin 0 and at a margin that makes later rounds run.  A cost is
    (2 * car_radius - distance) - 0.5 clipped at -1 (lidar_env/base.py:203-205) and three steps move nobody far, so at margin 0
    a fresh policy is rarely replaced.  The second margin is put between the policy's own s and the best candidate's of the
    (env, agent) of step 0 whose candidates differ most: that agent is replaced in round 0, so round 1 judges its env.  Every
    block record and every round re-derived (_derive).  One env per block gives every word again.
    rounds = 1 is the call without the argument: records and log word for word, and no new key"""
    T_, H, B, rounds = 3, 3, 3, 3
    cfg, eng = _engine(kind, n, n_obs, T_, cuda, use_rnn, 1, algo)
    seeds = torch.tensor([9, 10, 11], dtype=torch.int64, device=cuda)
    us = vs = np.linspace(-1.0, 1.0, 3).astype(f32)
    P = 10
    margins = [0.0]
    for margin in margins:
        records = []
        ro, log = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=margin, records=records, rounds=rounds)
        torch.cuda.synchronize()
        assert sorted(log) == ["flag", "index", "joint", "policy_action", "rounds_used", "s"]
        assert tuple(log["joint"].shape) == tuple(log["rounds_used"].shape) == (T_, B)
        assert log["joint"].dtype == log["rounds_used"].dtype == torch.int32 and tuple(log["s"].shape) == (T_, B, n, P)
        total = _derive(cfg, eng, ro, log, records, us, vs, H, margin, rounds, use_rnn, f"{name} margin {margin}")
        print(f"{name} margin {margin}: {total} (env, round) pairs over {T_ * B} (env, step) pairs; joint "
              f"{np.bincount(log['joint'].cpu().numpy().ravel(), minlength=3).tolist()}")
        used = log["rounds_used"].cpu().numpy()
        assert used.min() >= 1 and used.max() <= rounds
        if len(margins) == 1:
            # round 0's fold of step 0 [B, n, P], from the shield without rounds: the same state at any margin
            s0 = eng.rollout_lookahead_shielded(seeds, us, vs, H)[1]["s"][0].cpu().numpy().astype(np.float64)
            gap = s0[..., 0] - s0.min(axis=-1)
            e, i = np.unravel_index(gap.argmax(), gap.shape)
            assert gap[e, i] > 1e-4, "the case became trivial: no candidate of step 0 is better than the policy's action"
            BUSY = float(f32(-(s0[e, i, 0] - gap[e, i] / 2)))
            margins.append(BUSY)
        else:
            assert total > T_ * B and int(log["index"][0, e, i]) != 0, "no env needed a second round"
    # ---- one env per block: every round walks its list in blocks; the record without `records` reuses one block record ----
    cap = eng.prepass_graphs
    try:
        eng.prepass_graphs = n * P * (H + 2)
        recs_b = []
        ro_b, log_b = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=BUSY, records=recs_b, rounds=rounds)
        ro_c, log_c = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=BUSY, rounds=rounds)
    finally:
        eng.prepass_graphs = cap
    assert all(r[2].size == 1 for r in recs_b)
    _derive(cfg, eng, ro_b, log_b, recs_b, us, vs, H, BUSY, rounds, use_rnn, f"{name} blocks of one env")
    for other_ro, other_log, what in ((ro_b, log_b, "blocks of one env"), (ro_c, log_c, "one block record reused")):
        for key, b in _record_words(other_ro).items():
            if key == "rnn" and not use_rnn:
                continue
            _same_words(b, _record_words(ro)[key], f"{name}: {what}: {key}")
        for key in log:
            _same_words(other_log[key], log[key], f"{name}: {what}: log.{key}")
    # ---- rounds = 1 ----
    r0, r1 = [], []
    ro_0, log_0 = eng.rollout_lookahead_shielded(seeds, us, vs, H, records=r0)
    ro_1, log_1 = eng.rollout_lookahead_shielded(seeds, us, vs, H, records=r1, rounds=1)
    assert sorted(log_1) == sorted(log_0) == ["flag", "index", "policy_action", "s"]
    for key in log_0:
        _same_words(log_1[key], log_0[key], f"{name}: rounds=1: log.{key}")
    for key, b in _record_words(ro_1).items():
        if key == "rnn" and not use_rnn:
            continue
        _same_words(b, _record_words(ro_0)[key], f"{name}: rounds=1: {key}")
    assert [r[:3] for r in r1] == [r[:3] for r in r0]
    for a, b in zip(r0, r1):
        for key, w in _record_words(a[3]).items():
            if key == "rnn":
                w, other = w[1:], _record_words(b[3])[key][1:]                 # slot 0 of a block record's carries is never written
                if not use_rnn:
                    continue
            else:
                other = _record_words(b[3])[key]
            _same_words(other, w, f"{name}: rounds=1: block record {key}")
    # rounds = 3 at a margin that admits everything: nothing moves, one round, the unshielded record
    ro_a, log_a = eng.rollout_lookahead_shielded(seeds, us, vs, H, margin=-10.0, rounds=rounds)
    assert int(log_a["index"].abs().sum()) == 0 and bool((log_a["joint"] == 2).all()) and bool((log_a["rounds_used"] == 1).all())
    _same_words(ro_a.action_tm, eng.rollout(seeds, False).action_tm, f"{name}: everything admissible")


def test_engine_refusals(cuda):
    from dgppo_amd import _native as N, engine as EN
    seeds = torch.tensor([1], dtype=torch.int64, device=cuda)
    vmas = EN.Engine(N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 4, 0), EN.Hyper(batch_size=256), cuda, T=4)
    with pytest.raises(ValueError, match="rollout_lookahead_shielded.*VMASReverseTransport"):
        vmas.rollout_lookahead_shielded(seeds, [0.5], [0.5], 2, rounds=3)
    with pytest.raises(ValueError, match="lookahead_select_rounds.*VMASReverseTransport"):
        vmas.lookahead_select_rounds(None, None, None, None, None, 2, 0.0, 2, None, None, None, None, None, None)
    cfg, eng = _engine("LidarSpread", 3, 2, 3, cuda)
    for rounds in (0, -1):
        with pytest.raises(ValueError, match="rounds"):
            eng.rollout_lookahead_shielded(seeds, [0.5], [0.5], 2, rounds=rounds)


# ---- 5. test.py --shield-rounds, in-process -------------------------------------------------------------------------------------------
def test_cli_runs_the_rounds(cuda, tmp_path, capsys):
    from dgppo_amd.trainer import evaluate as EV
    from dgppo_amd.trainer.data import JointLookaheadShieldLog
    n, grid, Tn, H, rounds = 2, 2, 3, 2, 2
    run = _run_dir(tmp_path, "informarl", n, Tn)
    mod = _load_test_py()
    mod.main(["--path", str(run), "--epi", "2", "--no-video", "--max-step", str(Tn), "--shield", "--shield-horizon", str(H),
              "--shield-grid", str(grid), "--shield-rounds", str(rounds)])
    printed = capsys.readouterr().out
    stats = ("intervention_frac", "infeasible_frac", "mean_deviation")
    more = ("joint_verified_frac", "joint_unrolled_frac", "mean_rounds")
    for word in stats + more:
        assert printed.count(word) == 2, word
    assert printed.count("shield rounds:") == 2
    files = sorted(glob.glob(str(run / "videos" / "0" / "*_shield.npz")))
    assert len(files) == 2
    per_epi = ("policy_action", "action", "index", "flag", "s", "joint", "rounds_used")
    for path in files:
        z = np.load(path)
        assert sorted(z.files) == sorted([*JointLookaheadShieldLog._fields, *stats, *more])
        assert z["joint"].shape == z["rounds_used"].shape == (Tn,) and int(z["rounds"]) == rounds and int(z["horizon"]) == H
        assert set(z["joint"].tolist()) <= {0, 1, 2} and 1 <= z["rounds_used"].min() and z["rounds_used"].max() <= rounds
        one = JointLookaheadShieldLog(*(z[k][None] if k in per_epi else z[k] for k in JointLookaheadShieldLog._fields))
        for key, v in {**EV.shield_stats(one), **EV.joint_shield_stats(one)}.items():
            np.testing.assert_array_equal(z[key], v[0])
