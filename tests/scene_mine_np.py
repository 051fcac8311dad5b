"""NumPy restatement of dgppo_env_scene_mine and dgppo_env_scene_pool_push (csrc/env_scene.hip) for the scene-mining tests: the
first unsafe step and word, the template rows, the take rule, the ranks and the ring arithmetic; the validity bits come from
the restatement of dgppo_env_scene_load (tests/scenes_np.py) applied to the mined rows, which is the claim the kernel makes.
Everything here is integers or copied words."""
import functools

import numpy as np

import scenes_np as SN

f32 = np.float32
THRESH = f32(1e-6)


def first_unsafe(cost_tm, thresh):
    """cost_tm [T, B, n, n_cost] -> (first [B], who [B]) int32: the smallest t with a word >= thresh (NaN compares false) and
    the lowest such word index at that step, -1 / -1 without one"""
    T, B = cost_tm.shape[:2]
    with np.errstate(invalid="ignore"):
        unsafe = (np.asarray(cost_tm, f32) >= f32(thresh)).reshape(T, B, -1)
    first, who = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    for b in range(B):
        ts = np.flatnonzero(unsafe[:, b].any(axis=-1))
        if len(ts):
            first[b] = ts[0]
            who[b] = np.flatnonzero(unsafe[ts[0], b])[0]
    return first, who


def obstacle_template(cfg, obst):
    """[B, no, stride] records -> [B, no, 5] (LiDAR: cx, cy, w, h, theta) or [B, no, 2] (MPE: ox, oy); None without obstacles"""
    if obst is None:
        return None
    return np.ascontiguousarray(obst[..., :5 if cfg.is_lidar else 2])


def mine_np(cfg, agent_tm, cost_tm, goal, obst, back, thresh, sentinel):
    """-> dict(first, who, t0, flags int32 [B]; agent [B, n, sd], goal, obst ([B, no, 5 | 2] or None) float32, pre-filled with the
    word `sentinel` (uint32) and written only where first >= 0)"""
    T, B = cost_tm.shape[:2]
    first, who = first_unsafe(cost_tm, thresh)
    t0 = np.where(first >= 0, np.maximum(first - int(back), 0), -1).astype(np.int32)
    tmpl = obstacle_template(cfg, obst)
    rows = {"agent": np.full((B,) + agent_tm.shape[2:], sentinel, np.uint32), "goal": np.full(goal.shape, sentinel, np.uint32),
            "obst": None if tmpl is None else np.full(tmpl.shape, sentinel, np.uint32)}
    flags = np.zeros(B, np.int32)
    for b in range(B):
        if first[b] < 0:
            continue
        rows["agent"][b] = agent_tm[t0[b], b].view(np.uint32)
        rows["goal"][b] = goal[b].view(np.uint32)
        if tmpl is not None:
            rows["obst"][b] = tmpl[b].view(np.uint32)
        one = lambda k: None if rows[k] is None else rows[k][b:b + 1].view(f32)
        flags[b] = SN.scene_load_np(cfg, one("agent"), one("goal"), one("obst"), None, None, 0.0, 1)["flags"][0]
    return dict(first=first, who=who, t0=t0, flags=flags, **{k: None if v is None else v.view(f32) for k, v in rows.items()})


def taken(first, flags):
    """the take rule: unsafe at some step >= 1, and the mined row is a valid scene"""
    return (np.asarray(first) >= 1) & (np.asarray(flags) == 0)


def push_np(first, flags, rows, pool, fixed, state):
    """rows / pool: dict name -> float32 [B, ...] / [M, ...] (None entries skipped); state: 4 ints (head, filled, pushed_total,
    taken_last).  -> (pool after the push (copies), state after it, slot_of [B] int32)"""
    M = next(v for v in pool.values() if v is not None).shape[0]
    R = M - fixed
    head, filled, pushed, _ = (int(v) for v in state)
    out = {k: None if v is None else v.copy() for k, v in pool.items()}
    slot_of = np.full(len(first), -1, np.int32)
    r = 0
    for b in np.flatnonzero(taken(first, flags)):
        if r < R:
            slot_of[b] = fixed + (head + r) % R
            for k, v in out.items():
                if v is not None:
                    v.view(np.uint32)[slot_of[b]] = rows[k].view(np.uint32)[b]
        r += 1
    m = min(r, R)
    return out, [(head + m) % R, min(R, filled + m), pushed + m, r], slot_of


# ---- the head-on record: tests/golden/scenes/lidarspread_n2_headon.npz under constant full actions towards each other -----------
HEADON_T = 32
HEADON_ACTION = np.array([[1.0, 0.0], [-1.0, 0.0]], f32)        # agent 0 flies right, agent 1 left: full acceleration at each other


@functools.lru_cache(maxsize=None)
def headon_oracle():
    """the head-on scene stepped HEADON_T times with HEADON_ACTION by oracle/env_np.py alone -> (cost [T, n, n_cost], t*: the first
    step with a cost >= 1e-6, or -1)"""
    import lookahead_rounds_np as R
    from oracle import env_np as EN
    cfg, agent, goal, obst = R.scene_a()
    tab = EN.ray_table(cfg.n_rays)
    hits, _ = EN.lidar_sense(cfg, agent[..., :2], obst, *tab)
    action = HEADON_ACTION.reshape(1, 2, 2)
    costs = []
    for _ in range(HEADON_T):
        out = EN.env_step(cfg, agent, goal, obst, hits, action, ray_tab=tab, want_graph=False)
        costs.append(out["cost"][0])
        agent, hits = out["next_agent"], out["next_hits"]
    cost = np.stack(costs).astype(f32)
    first, _ = first_unsafe(cost[:, None], THRESH)
    return cost, int(first[0])


# ---- the hand-written cost cases (T = 6, n = 2, n_cost = 2, thresh 1e-6): name -> (cost [T, n, n_cost], first, who) ----------------
T_HAND = 6


def hand_cases():
    safe = np.full((T_HAND, 2, 2), -0.5, f32)

    def planted(*cells):
        c = safe.copy()
        for t, i, k, v in cells:
            c[t, i, k] = v
        return c
    below = np.nextafter(THRESH, f32(-1), dtype=f32)
    nan, inf = f32(np.nan), f32(np.inf)
    return {
        "never": (safe.copy(), -1, -1),
        "at_start": (planted((0, 1, 0, 0.2)), 0, 2),
        "at_end": (planted((T_HAND - 1, 0, 1, 0.3)), T_HAND - 1, 1),
        "equal_to_thresh": (planted((2, 1, 1, THRESH)), 2, 3),
        "one_ulp_below": (planted((2, 1, 1, below)), -1, -1),
        "nan_and_minus_inf": (planted((1, 0, 0, nan), (2, 1, 0, -inf), (3, 0, 1, nan)), -1, -1),
        "plus_inf": (planted((3, 1, 0, inf)), 3, 2),
        "two_agents": (planted((4, 1, 1, 0.1), (4, 0, 1, 0.1), (5, 0, 0, 0.5)), 4, 1),
        "nan_then_unsafe": (planted((1, 0, 0, nan), (3, 0, 0, 0.7)), 3, 0),
    }
