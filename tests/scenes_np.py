"""NumPy restatement of dgppo_env_scene_load (csrc/env_scene.hip) in float32 with the kernel's expression order, for the scene
tests.  The Philox stream is the one oracle/env_np.py uses for the reset; the thresholds are read from the ctypes cfg the kernel
gets (dgppo_amd._native.make_env_cfg), so both sides compare against the same float32 numbers."""
import numpy as np

from oracle import env_np as EN

f32 = np.float32
NONFINITE, OUT_OF_AREA, AGENTS_OVERLAP, AGENT_IN_OBSTACLE = 1, 2, 4, 8
ATTEMPTS = 16


def draw_index(attempt: int, agent: int, n: int) -> int:
    """the Philox counter of agent `agent` in attempt `attempt`"""
    return attempt * n + agent


def uniforms(seed: int, d: int):
    """draw d of the stream keyed by seed: words 0, 1 of Philox(counter=(d, 0, 0, 0), key=(lo32 seed, hi32 seed))"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = EN.philox4x32((d, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return EN.u01(w[0]), EN.u01(w[1])


def jittered(xy_t, u0, u1, J):
    """x_t + (2 u0 - 1) J, y_t + (2 u1 - 1) J: one IEEE operation each, measured from the template"""
    J = f32(J)
    return f32(xy_t[0] + f32(f32(f32(2) * u0 - f32(1)) * J)), f32(xy_t[1] + f32(f32(f32(2) * u1 - f32(1)) * J))


def obstacle_rows(cfg, obst_t):
    """[no, 5] rectangles -> [no, 16] records (numpy cos / sin: the device's may differ in the last bits); [no, 2] discs ->
    [no, sd] rows [ox, oy, 0, 0]"""
    obst_t = np.asarray(obst_t, f32)
    if cfg.is_lidar:
        return EN.make_rect(obst_t[:, 0:2], obst_t[:, 2], obst_t[:, 3], obst_t[:, 4])
    rows = np.zeros((obst_t.shape[0], cfg.state_dim), f32)
    rows[:, :2] = obst_t
    return rows


def geometry_bits(cfg, agent, obst) -> int:
    """bits 2, 4, 8 of one scene: agent [n, sd] as it stands, obst the rows of obstacle_rows (None without obstacles).  Every
    comparison is false for a NaN, as in the kernel"""
    n = agent.shape[0]
    A, Y = f32(cfg.area_size), f32(cfg.y_limit)
    bits = 0
    for i in range(n):
        x, y = agent[i, 0], agent[i, 1]
        if x < 0 or x > A or y < 0 or y > Y:
            bits |= OUT_OF_AREA
        for j in range(i + 1, n):
            if EN.norm2(f32(x - agent[j, 0]), f32(y - agent[j, 1])) < f32(cfg.two_car_radius):
                bits |= AGENTS_OVERLAP
        for o in range(0 if obst is None else obst.shape[0]):
            if cfg.is_lidar:
                inside = bool(EN.rect_inside(x, y, obst[o], f32(cfg.car_radius)))
            else:
                inside = bool(EN.norm2(f32(x - obst[o, 0]), f32(y - obst[o, 1])) < f32(cfg.car_plus_obs))
            if inside:
                bits |= AGENT_IN_OBSTACLE
    return bits


def scene_load_np(cfg, agent_t, goal_t, obst_t, scene_ids, seeds, jitter, B):
    """-> dict(agent [B, n, sd], goal [B, ng, sd], obst [B, no, stride] or None, flags [B] int32, n_failed int, attempt [B]: the
    attempt that was kept, ATTEMPTS - 1 where none was valid, -1 without jitter)"""
    agent_t, goal_t = np.asarray(agent_t, f32), np.asarray(goal_t, f32)
    S, n = agent_t.shape[0], agent_t.shape[1]
    with np.errstate(invalid="ignore"):
        rows = None if obst_t is None else [obstacle_rows(cfg, obst_t[s]) for s in range(S)]
    agent = np.zeros((B,) + agent_t.shape[1:], f32)
    goal = np.zeros((B,) + goal_t.shape[1:], f32)
    obst = None if rows is None else np.zeros((B,) + rows[0].shape, f32)
    flags, attempt, n_failed = np.zeros(B, np.int32), np.full(B, -1, np.int32), 0
    for b in range(B):
        s = int(scene_ids[b]) if scene_ids is not None else b % S
        finite = np.isfinite(agent_t[s]).all() and np.isfinite(goal_t[s]).all() and (obst_t is None or np.isfinite(obst_t[s]).all())
        nonfinite = 0 if finite else NONFINITE
        goal.view(np.uint32)[b] = goal_t.view(np.uint32)[s]                       # words: a NaN keeps its payload
        agent.view(np.uint32)[b] = agent_t.view(np.uint32)[s]
        if obst is not None:
            obst[b] = rows[s]
        ob = None if obst is None else obst[b]
        with np.errstate(invalid="ignore"):
            bits = nonfinite | geometry_bits(cfg, agent[b], ob)
            if jitter > 0:
                for a in range(ATTEMPTS):
                    for i in range(n):
                        u0, u1 = uniforms(seeds[b], draw_index(a, i, n))
                        agent[b, i, 0], agent[b, i, 1] = jittered(agent_t[s, i], u0, u1, jitter)
                    bits = nonfinite | geometry_bits(cfg, agent[b], ob)
                    attempt[b] = a
                    if bits == 0:
                        break
                n_failed += int(bits != 0)
        flags[b] = bits
    return dict(agent=agent, goal=goal, obst=obst, flags=flags, n_failed=n_failed, attempt=attempt)
