"""The rounds of the lookahead shield restated in NumPy, on tests/lookahead_np.py: the fork from a list of envs
(dgppo_env_team_action_fork_ids) as fork_np on the gathered envs, the rule of dgppo_lookahead_reselect (include/dgppo_hip.h), the
rounds of Engine.lookahead_select_rounds over oracle/env_np.py with a policy that plays the zero action, and scene A: two agents
flying at each other, whose individually admissible dodges collide.  Shared by tests/test_lookahead_rounds_cpu.py and
tests/test_lookahead_rounds_gpu.py."""
import numpy as np

import lookahead_np as L
from oracle import env_np as EN

f32 = np.float32


# ---- the fork from a list of envs ---------------------------------------------------------------------------------------------------
def fork_ids_np(fields, a_base, ids, us, vs, carry=None):
    """fork_np on the envs ids[0 .. M) of B dense envs: output env (m * n + i) * P + p is a copy of env ids[m], its joint action
    a_base[ids[m]] with row i replaced by candidate p for p > 0; carry [B * n, HC] rows of env ids[m].  ids None: every env"""
    a_base = np.ascontiguousarray(a_base, f32)
    B, n = a_base.shape[:2]
    ids = np.arange(B) if ids is None else np.asarray(ids, np.int64)
    c = None
    if carry is not None:
        c = np.ascontiguousarray(carry, f32).reshape(B, n, -1)[ids].reshape(ids.size * n, -1)
    return L.fork_np({k: np.ascontiguousarray(v)[ids] for k, v in fields.items()}, a_base[ids], us, vs, c)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def pick_np(s, held, ref, us, vs, margin):
    """one agent: s [P], held / ref [2] -> (pick, flag of the pick: 0 candidate 0 admissible, 1 an admissible candidate, 2 the
    least bad of none).  Candidate 0 is clip(held); the distance is taken from clip(ref)"""
    s = np.asarray(s, f32)
    cand = L.clip(L.candidates(np.asarray(held, f32), us, vs))                  # [P, 2]
    r = L.clip(ref)
    thr = f32(-f32(margin))
    with np.errstate(invalid="ignore", over="ignore"):
        adm = s <= thr
        if adm[0]:
            return 0, 0
        if adm.any():
            du, dv = (cand[:, 0] - r[0]).astype(f32), (cand[:, 1] - r[1]).astype(f32)
            d = ((du * du).astype(f32) + (dv * dv).astype(f32)).astype(f32)
            d = np.where(np.isnan(d), f32(np.inf), d)
            d = np.where(adm, d, f32(np.inf))
            return int(np.flatnonzero(adm & (d == d.min()))[0]), 1
        ok = ~np.isnan(s)
        return (int(np.flatnonzero(ok & (s == s[ok].min()))[0]) if ok.any() else 0), 2


def reselect_np(s, ids, a_ref, us, vs, margin, mode, action, index, flag=None, joint=None, changed=None):
    """dgppo_lookahead_reselect on the fold s [M, n, P] of the listed envs ids (None: all E).  action [E, n, 2] / index [E, n]:
    what is held; flag [E, n], joint / changed [E]: given arrays keep the rows of the envs that are not listed (zeros otherwise)
    -> new (action, index, flag, joint, changed); nothing is modified in place"""
    action, index = np.array(action, f32), np.array(index, np.int32)
    E, n = index.shape
    ids = np.arange(E) if ids is None else np.asarray(ids, np.int64)
    flag = np.zeros((E, n), np.int32) if flag is None else np.array(flag, np.int32)
    joint = np.zeros(E, np.int32) if joint is None else np.array(joint, np.int32)
    changed = np.zeros(E, np.int32) if changed is None else np.array(changed, np.int32)
    assert mode in (0, 1) and s.shape[:2] == (ids.size, n)
    thr = f32(-f32(margin))
    for m, e in enumerate(ids):
        picks = [pick_np(s[m, i], action[e, i], a_ref[e, i], us, vs, margin) for i in range(n)]
        movers = [i for i in range(n) if picks[i][0] != 0]
        if mode == 1:
            movers = movers[:1]
        for i in range(n):
            pick, fl = picks[i]
            cand = L.clip(L.candidates(action[e, i], us, vs))
            if i in movers:
                action[e, i], index[e, i], flag[e, i] = cand[pick], pick, fl
            else:
                with np.errstate(invalid="ignore"):
                    adm0 = bool(s[m, i, 0] <= thr)
                action[e, i] = cand[0]
                flag[e, i] = 2 if not adm0 else (0 if index[e, i] == 0 else 1)
        changed[e] = int(bool(movers))
        joint[e] = 0 if movers else (1 if any(fl != 0 for _, fl in picks) else 2)
    return action, index, flag, joint, changed


def rounds_np(fold, a_pol, us, vs, margin, rounds):
    """the rounds of Engine.lookahead_select_rounds: fold(ids, A) -> s [M, n, P], the worst own-row costs of the what-if envs forked
    from the joint action A [E, n, 2] for the envs ids.  -> dict(action, index, flag, s, joint, rounds_used, trace): s [E, n, P] is
    the fold of every env's last round, trace one (ids, s of the round, action, index, flag, joint, changed after it) per round"""
    a_pol = np.asarray(a_pol, f32)
    E, n = a_pol.shape[:2]
    P = 1 + len(us) * len(vs)
    action, index = a_pol.copy(), np.zeros((E, n), np.int32)
    flag, joint = np.zeros((E, n), np.int32), np.zeros(E, np.int32)
    s_all, used = np.zeros((E, n, P), f32), np.zeros(E, np.int32)
    ids, trace = np.arange(E), []
    for r in range(int(rounds)):
        s = np.asarray(fold(ids, action), f32)
        s_all[ids] = s
        used[ids] += 1
        action, index, flag, joint, changed = reselect_np(s, ids, a_pol, us, vs, margin, 0 if r == 0 else 1, action, index, flag,
                                                          joint, np.zeros(E, np.int32))
        trace.append((ids.copy(), s, action.copy(), index.copy(), flag.copy(), joint.copy(), changed.copy()))
        ids = np.flatnonzero(changed)
        if ids.size == 0:
            break
    return dict(action=action, index=index, flag=flag, s=s_all, joint=joint, rounds_used=used, trace=trace)


# ---- scene A: two agents head on, the obstacle far away ---------------------------------------------------------------------------------
SCENE_A_H = 12
SCENE_A_US = np.array([-1.0, 0.0, 1.0], f32)
SCENE_A_VS = np.array([-1.0, 0.0, 1.0], f32)
SCENE_A_UNSAFE = f32(0.5660001)          # the worst own-row cost of both agents when both hold on, and when both dodge down
SCENE_A_SAFE = f32(-0.50394225)          # ... when agent 0 holds on and agent 1 dodges down


def scene_a():
    """LidarSpread, n = 2, one 0.1 x 0.1 obstacle centred at (1.3, 0.1), far from everything.  Agent 0 at (0.5, 0.75) flies right at
    0.3, agent 1 at (0.75, 0.75) flies left at 0.3; the goals lie behind the other agent.  -> (oracle cfg, agent [1, 2, 4],
    goal [1, 2, 4], obst [1, 1, 16])"""
    cfg = EN.EnvCfg(kind=0, n_agents=2, n_obs=1)
    agent = np.array([[[0.5, 0.75, 0.3, 0.0], [0.75, 0.75, -0.3, 0.0]]], f32)
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[1.3, 0.75], [0.1, 0.75]]
    obst = EN.make_rect(np.array([[[1.3, 0.1]]], f32), np.full((1, 1), 0.1, f32), np.full((1, 1), 0.1, f32), np.zeros((1, 1), f32))
    return cfg, agent, goal, obst


def roll_joint(cfg, agent, goal, obst, joint_action, H):
    """one env: the joint action [n, 2] in the coming step, then H zero-action steps (the policy being the zero action) by
    oracle/env_np.py alone -> [n]: every agent's worst own-row cost over the H states after the forced step"""
    tab = EN.ray_table(cfg.n_rays)
    hits, _ = EN.lidar_sense(cfg, agent[..., :2], obst, *tab)
    a, h = agent, hits
    action = np.asarray(joint_action, f32).reshape(1, cfg.n_agents, 2)
    costs = []
    for k in range(H + 1):
        out = EN.env_step(cfg, a, goal, obst, h, action, ray_tab=tab, want_graph=False)
        costs.append(out["cost"])
        a, h = out["next_agent"], out["next_hits"]
        action = np.zeros((1, cfg.n_agents, 2), f32)
    return np.stack(costs[1:])[:, 0].max(axis=(0, 2)).astype(f32)


def scene_a_fold(H=SCENE_A_H, us=SCENE_A_US, vs=SCENE_A_VS):
    """the fold of scene A for rounds_np, by the oracle alone: s[0, i, p] is agent i's worst own-row cost with row i of the joint
    action A[0] replaced by candidate p (p > 0)"""
    cfg, agent, goal, obst = scene_a()
    n = cfg.n_agents

    def fold(ids, A):
        assert list(ids) == [0]
        cand = L.candidates(np.asarray(A, f32), us, vs)                          # [1, n, P, 2], candidate 0 the action held
        P = cand.shape[2]
        s = np.zeros((1, n, P), f32)
        for i in range(n):
            for p in range(P):
                ja = np.array(A[0], f32)
                ja[i] = cand[0, i, p]
                s[0, i, p] = roll_joint(cfg, agent, goal, obst, ja, H)[i]
        return s
    return fold
