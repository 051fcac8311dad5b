"""The lookahead shield restated in NumPy: the layout of dgppo_env_team_action_fork, the fold and the selection rule of
dgppo_lookahead_select (include/dgppo_hip.h), and a hand-made LidarSpread scene rolled with oracle/env_np.py alone.  Shared by
tests/test_lookahead_shield_cpu.py and tests/test_lookahead_shield_gpu.py."""
import numpy as np

from oracle import env_np as EN

f32 = np.float32


# ---- candidates and the fork ------------------------------------------------------------------------------------------------------
def grid_actions(us, vs):
    """[nv * nu, 2]: candidate 1 + iv * nu + iu is (us[iu], vs[iv])"""
    return np.stack(np.meshgrid(np.asarray(us, f32), np.asarray(vs, f32)), axis=-1).reshape(-1, 2).astype(f32)


def candidates(a_pol, us, vs):
    """[..., P, 2], unclipped: the policy's action, then the grid"""
    a_pol = np.asarray(a_pol, f32)
    grid = grid_actions(us, vs)
    return np.concatenate([a_pol[..., None, :], np.broadcast_to(grid, a_pol.shape[:-1] + grid.shape)], axis=-2)


def clip(a):
    a = np.asarray(a, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), a, np.minimum(np.maximum(a, f32(-1)), f32(1))).astype(f32)


def fork_np(fields, a_pol, us, vs, carry=None):
    """fields: name -> [B, ...] array of a dense env state; a_pol [B, n, 2]; carry [B * n, HC] or None -> (the same fields for the
    G = B * n * P envs, action [G, n, 2], carry [G * n, HC] or None).  Env (e * n + i) * P + p is a copy of env e; row i of its
    joint action is candidate p, every other row a_pol[e]'s.  Words only: the arrays are handled as uint32."""
    a_pol = np.ascontiguousarray(a_pol, f32)
    B, n = a_pol.shape[:2]
    grid = grid_actions(us, vs)
    P = 1 + grid.shape[0]
    rep = lambda x: np.repeat(np.ascontiguousarray(x, f32).view(np.uint32), n * P, axis=0)
    out = {k: rep(v) for k, v in fields.items()}
    action = rep(a_pol).reshape(B, n, P, n, 2)
    for i in range(n):
        action[:, i, 1:, i, :] = grid.view(np.uint32)[None]
    c = None
    if carry is not None:
        HC = carry.shape[1]
        c = rep(np.ascontiguousarray(carry, f32).reshape(B, n, HC)).reshape(B * n * P * n, HC)
    return out, action.reshape(B * n * P, n, 2), c


# ---- the fold and the rule --------------------------------------------------------------------------------------------------------
def fold_np(cost, E, n, P):
    """cost [K, G, n, nh] (the K states after the forced step), G = E * n * P -> s [E, n, P]: the maximum over the steps and the
    components of the agent's OWN row of its own what-if env; np.max propagates NaN"""
    cost = np.asarray(cost, f32)
    K, G, n_, nh = cost.shape
    assert G == E * n * P and n_ == n
    c = cost.reshape(K, E, n, P, n, nh)
    own = np.stack([c[:, :, i, :, i, :] for i in range(n)], axis=2)          # [K, E, n, P, nh]
    return own.max(axis=(0, 4)).astype(f32)


def rule_np(s, a_pol, us, vs, margin):
    """s [..., P] -> index, flag, action: candidate 0 if admissible (s <= -margin; never a NaN), else the admissible candidate
    nearest to it (du * du + dv * dv in fp32 on clipped actions, a NaN distance counts as +inf, lowest index on ties), else the
    smallest s (lowest index on ties, NaN skipped, candidate 0 when every s is NaN)"""
    s = np.asarray(s, f32)
    cand = clip(candidates(a_pol, us, vs))
    lead = s.shape[:-1]
    index, flag = np.zeros(lead, np.int32), np.zeros(lead, np.int32)
    thr = f32(-f32(margin))
    with np.errstate(invalid="ignore"):
        for ix in np.ndindex(*lead):
            ss, cc = s[ix], cand[ix]
            adm = ss <= thr
            if adm[0]:
                continue
            if adm.any():
                du, dv = (cc[:, 0] - cc[0, 0]).astype(f32), (cc[:, 1] - cc[0, 1]).astype(f32)
                d = ((du * du).astype(f32) + (dv * dv).astype(f32)).astype(f32)
                d = np.where(np.isnan(d), f32(np.inf), d)
                d = np.where(adm, d, f32(np.inf))
                index[ix], flag[ix] = int(np.flatnonzero(adm & (d == d.min()))[0]), 1
            else:
                ok = ~np.isnan(ss)
                index[ix], flag[ix] = (int(np.flatnonzero(ok & (ss == ss[ok].min()))[0]) if ok.any() else 0), 2
    action = np.take_along_axis(cand, index[..., None, None].astype(np.int64).repeat(2, -1), axis=-2)[..., 0, :]
    return index, flag, action


def assert_same_words(got, want, name):
    """bit-equal, a NaN matching any NaN (the kernels' NaN-propagating max returns the canonical one)"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{name}: NaN positions differ"
    bad = int((got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]).sum())
    assert bad == 0, f"{name}: {bad} of {got.size} words differ"


# ---- a hand-made scene: one agent heading for an obstacle, the other far away at rest ---------------------------------------------
SCENE_H = 8
SCENE_US = np.array([-1.0, 0.0, 1.0], f32)
SCENE_VS = np.array([-1.0, 0.0, 1.0], f32)


def scene(mover=0):
    """LidarSpread, n = 2, one obstacle: a 0.2 x 0.2 square whose left face is 0.08 in front of the mover, which flies at it at
    0.25 (0.0075 per step, dt = 0.03).  Left alone the mover is within car_radius = 0.05 of the face after 5 steps: the cost turns
    >= 0.5 within SCENE_H = 8.  A full brake (u = -1 changes the velocity by 0.3) reverses it after one more step.  The ray at
    angle 0 meets the face at a right angle, so the LiDAR distance is the true one.  The other agent rests 0.6 from the square,
    outside the sensing radius.  -> (oracle cfg, agent [1, 2, 4], goal [1, 2, 4], obst [1, 1, 16])"""
    cfg = EN.EnvCfg(kind=0, n_agents=2, n_obs=1)
    agent = np.zeros((1, 2, 4), f32)
    agent[0, mover] = [0.5, 0.75, 0.25, 0.0]
    agent[0, 1 - mover] = [1.2, 0.2, 0.0, 0.0]
    goal = np.zeros((1, 2, 4), f32)
    goal[0, :, :2] = [[0.2, 1.3], [1.3, 1.3]]
    obst = EN.make_rect(np.array([[[0.68, 0.75]]], f32), np.full((1, 1), 0.2, f32), np.full((1, 1), 0.2, f32), np.zeros((1, 1), f32))
    return cfg, agent, goal, obst


def scene_oracle(mover=0, H=SCENE_H, us=SCENE_US, vs=SCENE_VS):
    """s [1, 2, P] of the scene by oracle/env_np.py alone, the policy being the zero action: per (agent i, candidate p) the forced
    joint action (zeros but row i), then H zero-action steps; the worst own-row cost of the H states after the forced step"""
    cfg, agent, goal, obst = scene(mover)
    tab = EN.ray_table(cfg.n_rays)
    hits0, _ = EN.lidar_sense(cfg, agent[..., :2], obst, *tab)
    cand = candidates(np.zeros((1, 2, 2), f32), us, vs)                      # [1, 2, P, 2]
    P = cand.shape[2]
    s = np.zeros((1, 2, P), f32)
    for i in range(2):
        for p in range(P):
            a, h = agent, hits0
            action = np.zeros((1, 2, 2), f32)
            action[0, i] = cand[0, i, p]
            costs = []
            for k in range(H + 1):
                out = EN.env_step(cfg, a, goal, obst, h, action, ray_tab=tab, want_graph=False)
                costs.append(out["cost"])
                a, h = out["next_agent"], out["next_hits"]
                action = np.zeros((1, 2, 2), f32)
            s[0, i, p] = np.stack(costs[1:])[:, 0, i, :].max()
    return s
