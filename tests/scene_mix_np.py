"""NumPy side of the scene-mix tests: what dgppo_env_scene_mix must leave in a record that held a reset, stated through the
restatement of dgppo_env_scene_load (tests/scenes_np.py), and the inputs of the kernel cases — three template scenes per case, the
assignments of B = 5 and B = 9 — with the conditions the cases must meet."""
import numpy as np

import scenes_np as SN

f32 = np.float32
# (kind, n, n_obs): n = 33 and 64 fill more than half a wave; two goals (LidarLine), one goal (MPEFormation), state_dim 5 (bicycle)
CASES = [("LidarSpread", 1, 0), ("LidarSpread", 2, 1), ("LidarSpread", 3, 3), ("LidarSpread", 33, 2), ("LidarSpread", 64, 2),
         ("LidarBicycleTarget", 2, 1), ("MPESpread", 3, 2), ("LidarLine", 2, 1), ("MPEFormation", 3, 1)]
LARGE_AREA = 4.0            # n >= 33: the reset refuses 1.5 x 1.5 at that density (tests/test_large_team_kernels_gpu.py)
S = 3
JITTERS = (0.0, 0.02)
# kept envs (any negative number) next to repeated ids; four waves per 256-thread block: one block with a tail, three with one
SCENE_OF = {5: np.array([1, -1, 0, 2, 1], np.int32), 9: np.array([0, -1, 2, 2, -3, 1, 0, -1, 1], np.int32)}


def make_cfg(kind, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind], n, n_obs, **({"area_size": LARGE_AREA} if n >= 33 else {}))


def seeds_of(B, salt):
    return (np.arange(1, B + 1, dtype=np.int64) * 104729) + salt


def high_pair(n):
    """the two agents of the large cases' overlap scene: both of index >= 32 where the team has two such agents (n = 64), else
    the one it has (index 32 of n = 33) and an agent of the lower half"""
    return (40, 63) if n == 64 else (5, 32)


def templates(cfg, random_templates, seed):
    """-> (agent_t, goal_t, obst_t) of S = 3 scenes.  Small teams: random_templates (test_scenes_gpu._templates) as it is.  n >= 33:
    random positions in [0.1, 1.4] always overlap, so scenes 0 and 1 put the agents on a grid of pitch 0.3 in [1.8, 3.9]^2, clear of
    the random obstacles; scene 1 then moves one agent of high_pair to 0.01 beside the other: the only invalid pair of that scene,
    at any jitter <= 0.02; scene 2 stays random (every kind of bit)."""
    agent, goal, obst = random_templates(cfg, S, seed)
    n = cfg.n_agents
    if n >= 33:
        gx, gy = np.meshgrid(np.arange(8), np.arange(8))
        grid = (1.8 + 0.3 * np.stack([gx.ravel(), gy.ravel()], axis=-1)).astype(f32)[:n]
        agent[0, :, :2] = grid
        agent[1, :, :2] = grid
        i, j = high_pair(n)
        agent[1, j, :2] = grid[i] + f32(0.01)
    return agent, goal, obst


def mix_np(cfg, agent_t, goal_t, obst_t, scene_of, seeds, jitter, record):
    """record: dict(agent, goal, obst | None) of the reset, float32 [B, ...] -> dict(agent, goal, obst, flags [B] (kept envs: None
    is not representable, so -1 there), n_fallback, attempt, load: scene_load_np's own output for ids = max(scene_of, 0))"""
    B = len(scene_of)
    ids = np.maximum(scene_of, 0)
    load = SN.scene_load_np(cfg, agent_t, goal_t, obst_t, ids, seeds, jitter, B)
    out = {k: (None if record[k] is None else record[k].copy()) for k in ("agent", "goal", "obst")}
    flags = np.full(B, -1, np.int64)
    for b in range(B):
        if scene_of[b] < 0:
            continue
        flags[b] = load["flags"][b]
        if load["flags"][b] == 0:
            for k in ("agent", "goal", "obst"):
                if out[k] is not None:
                    out[k].view(np.uint32)[b] = load[k].view(np.uint32)[b]
    assigned = scene_of >= 0
    return dict(out, flags=flags, n_fallback=int((load["flags"][assigned] != 0).sum()), attempt=load["attempt"], load=load)


def overlap_only_between(cfg, agent_rows, i, j):
    """is (i, j) the one pair of agent_rows [n, sd] closer than two_car_radius?"""
    xy = agent_rows[:, :2].astype(np.float64)
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    close = {(a, b) for a in range(len(xy)) for b in range(a + 1, len(xy)) if d[a, b] < float(cfg.two_car_radius)}
    return close == {(min(i, j), max(i, j))}
