"""Hand-built LiDAR scenes for the paths of the env step kernels that a scene drawn at random never takes: rays exactly parallel
to a rectangle edge (det == 0 -> NaN alpha), clipped determinants, bit-identical alphas among the hitting
rays, obstacles either side of the wave kernel's robustness / reach / ray-cull thresholds, distances one ulp either side of the
mask radii, and non-finite actions and states.  A plain helper module (like vmas_np.py): numpy and the oracle only.

build(ocfg, seed) -> (agent [B, n, sd], goal [B, n_goals, sd], obst [B, n_obs, 16], action [B, n, 2], tags [B]); one env per
scene, tags[b] names the scene of env b.  Velocities are zero wherever a scene depends on an exact position, so that a step
leaves the agent on it.  tests/test_env_edges_cpu.py proves on the oracle alone that each scene reaches its path."""
import numpy as np

from oracle import env_np as E

f32 = np.float32
FAR = (-3.0, -3.0)                    # centre of an obstacle nobody reaches (obstacles are not confined to the area)
ROBUST = 0.3                          # an angle at which no edge is near parallel to a ray of the 32-fan
AXIS_ANGLES = (f32(0.0), f32(np.pi / 2), f32(np.pi))
PARALLEL_K = (1, 3, 6)                # obstacle angles fp32(k * 2 pi / 32)
WEAK_ANGLES = (f32(1e-7), f32(3e-4), f32(5e-4))
CULL_DELTAS = (-1e-3, -1e-6, 0.0, 1e-6, 1e-3)
SCENES = ("axis-aligned", "parallel-to-ray", "weak-threshold", "on-vertex", "ties-beside-nan-agent", "symmetric-ties", "graze",
          "cull-boundary", "mask-radius", "non-finite", "clean")


def three(r):
    """nextafter(r, 0), r, nextafter(r, 1) in fp32"""
    r = f32(r)
    return np.nextafter(r, f32(0)), r, np.nextafter(r, f32(1))


def lidar_radius(ocfg):
    """the agent-hit mask radius of get_graph"""
    return f32(ocfg.comm_radius - 1e-1)


def cull_circle(rec):
    """vertex mean c_o and h_o + 0.05 of one rectangle record, in the wave kernel's fp32 order (csrc/env_wave.hip, P1a)"""
    P = rec[8:16].astype(f32)
    cx = f32(f32(f32(P[0] + P[2]) + f32(P[4] + P[6])) * f32(0.25))
    cy = f32(f32(f32(P[1] + P[3]) + f32(P[5] + P[7])) * f32(0.25))
    h2 = f32(0)
    for m in range(4):
        dx, dy = f32(P[2 * m] - cx), f32(P[2 * m + 1] - cy)
        h2 = max(h2, f32(f32(dx * dx) + f32(dy * dy)))
    return cx, cy, f32(np.sqrt(h2) + f32(0.05))


def is_weak(rec, ray_cos, ray_sin):
    """the wave kernel's robustness test: some ray of the fan is within 4e-4 of parallel to one of the two edge directions"""
    P = rec[8:16].astype(f32)
    for m in (0, 1):
        mm = (m + 3) & 3
        ex, ey = f32(P[2 * mm] - P[2 * m]), f32(P[2 * mm + 1] - P[2 * m + 1])
        cc = ((ray_cos * ey).astype(f32) - (ray_sin * ex).astype(f32)).astype(f32)
        if not bool(np.all(np.abs(cc) >= f32(4e-4))):
            return True
    return False


class _Scene:
    """one env under construction: agents parked apart at rest, goals at random, every obstacle out of reach"""
    PARK = [(1.4, 1.4), (1.4, 0.1), (0.1, 1.4), (0.1, 0.1), (1.4, 0.75), (0.75, 1.4), (0.1, 0.75), (0.75, 0.1)]

    def __init__(self, ocfg, rng, tag):
        n, sd = ocfg.n_agents, ocfg.state_dim
        self.ocfg, self.tag = ocfg, tag
        self.agent = np.zeros((n, sd), f32)
        self.agent[:, :2] = np.asarray(self.PARK[:n], f32)
        if ocfg.is_bicycle:
            self.agent[:, 2] = 1.0                                        # heading (1, 0), speed 0
        self.goal = np.zeros((ocfg.n_goals, sd), f32)
        self.goal[:, :2] = rng.uniform(0.1, 1.4, size=(ocfg.n_goals, 2))
        self.obst = np.stack([E.make_rect(np.asarray(FAR, f32) - f32(o), f32(0.2), f32(0.15), f32(ROBUST))
                              for o in range(ocfg.n_obs)])
        self.action = rng.uniform(-1.5, 1.5, size=(n, 2)).astype(f32)

    def rect(self, o, centre, w, h, theta):
        self.obst[o] = E.make_rect(np.asarray(centre, f32), f32(w), f32(h), f32(theta))
        return self.obst[o]

    def at(self, i, x, y):
        self.agent[i, 0], self.agent[i, 1] = f32(x), f32(y)


def _rotated(vals, n_obs, shift):
    return [vals[(o + shift) % len(vals)] for o in range(n_obs)]


def _cluster(s, angles, size=(0.3, 0.2)):
    """obstacles with the given angles around (0.45, 0.45); agent 0 at the centre of obstacle 0 (inside), agents 1, 2 within
    reach at heights that put whole-number rays onto edges, the last agent out of everybody's reach at y >= 1 (where
    y + sin * R rounds back onto y for the rays along x)"""
    centres = [(0.45, 0.45), (0.8, 0.3), (0.3, 0.85)]
    for o, th in enumerate(angles):
        s.rect(o, centres[o], size[0], size[1], th)
    n = s.ocfg.n_agents
    s.at(0, *centres[0])
    s.at(1, 0.125, 0.5)
    s.at(2, 0.75, 0.625)
    for i in range(3, n - 1):
        s.at(i, 0.25 + 0.125 * i, 1.0)
    s.at(n - 1, 1.4375, 1.4375)


def _axis_aligned(ocfg, rng):
    out = []
    for shift in (0, 2):
        s = _Scene(ocfg, rng, "axis-aligned")
        _cluster(s, _rotated(AXIS_ANGLES, ocfg.n_obs, shift))
        out.append(s)
    return out


def _parallel(ocfg, rng):
    out = []
    for shift in (0, 2):
        s = _Scene(ocfg, rng, "parallel-to-ray")
        ks = _rotated(PARALLEL_K, ocfg.n_obs, shift)
        _cluster(s, [f32(k * 2 * np.pi / 32) for k in ks])
        out.append(s)
    return out


def _weak(ocfg, rng):
    """unit squares (an edge of length 1 turned by theta gives |cos * ey - sin * ex| = theta for the ray along it): 1e-7 and
    3e-4 fail the 4e-4 test, 5e-4 passes it and is culled like any robust obstacle"""
    out = []
    centres = [(-0.25, 0.5), (0.75, -0.3), (1.75, 1.0)]
    for shift in (0, 2):
        s = _Scene(ocfg, rng, "weak-threshold")
        for o, th in enumerate(_rotated(WEAK_ANGLES, ocfg.n_obs, shift)):
            s.rect(o, centres[o], 1.0, 1.0, th)
        n = s.ocfg.n_agents
        s.at(0, 0.5, 0.5)
        s.at(1, 0.75, 0.375)
        s.at(2, 1.0, 1.0)
        for i in range(3, n):
            s.at(i, 0.125 * i, 1.25)
        out.append(s)
    return out


def _on_vertex(ocfg, rng):
    s = _Scene(ocfg, rng, "on-vertex")
    rec = s.rect(0, (0.7, 0.6), 0.25, 0.15, ROBUST)
    s.at(0, rec[8 + 2 * 1], rec[9 + 2 * 1])                              # stored vertex m = 1
    s.at(1, rec[8 + 2 * 3], rec[9 + 2 * 3])                              # and m = 3
    s.at(2, 0.3, 0.55)
    return [s]


def _ties_beside_nan_agent(ocfg, rng):
    """the on-vertex scene with its tied agents 2 and 3 and a NaN x for agent 0: an env with NaN alphas in which the pair
    (2, 3) has none — in the wave kernel the two-class ranking of its NaN branch, with ties"""
    s = _Scene(ocfg, rng, "ties-beside-nan-agent")
    rec = s.rect(0, (0.7, 0.6), 0.25, 0.15, ROBUST)
    s.at(2, rec[8 + 2 * 1], rec[9 + 2 * 1])
    s.at(3, rec[8 + 2 * 3], rec[9 + 2 * 3])
    s.at(1, 0.3, 0.55)
    s.agent[0, 0] = np.nan
    return [s]


def _symmetric_ties(ocfg, rng):
    s = _Scene(ocfg, rng, "symmetric-ties")
    cx, cy = 0.75, 0.5
    s.rect(0, (cx, cy), 0.3, 0.3, 0.0)
    s.at(0, cx - 0.45, cy)
    s.at(1, cx, cy - 0.45)                                               # the same from below: ties around the ray along +y
    s.at(2, cx + 0.45, cy)
    return [s]


def _graze(ocfg, rng):
    """ray 16 (direction (1, 0)) at the leftmost stored vertex of a turned rectangle, from R - ulp, R and R + ulp away"""
    s = _Scene(ocfg, rng, "graze")
    rec = s.rect(0, (1.0, 0.75), 0.25, 0.15, 0.7)
    xs, ys = rec[8:16:2], rec[9:16:2]
    m = int(np.argmin(xs))
    for i, d in enumerate(three(ocfg.comm_radius)):
        s.at(i, f32(xs[m] - d), ys[m])
    return [s]


def _chunks(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def _cull_boundary(ocfg, rng):
    """robust obstacle at (0.75, 0.75); agents on the radial line at 0.9 rad through c_o at R + h_o + 0.05 + d (pair cull), and
    agents within reach, below c_o by h_o + 0.05 + d (ray 16's line either side of the cull circle); every env also holds one
    agent next to the obstacle"""
    probe = _Scene(ocfg, rng, "cull-boundary")
    rec = probe.rect(0, (0.75, 0.75), 0.2, 0.25, ROBUST)
    cx, cy, hm = cull_circle(rec)
    thr = f32(f32(ocfg.comm_radius) + hm)
    spots = [(float(cx) + (float(thr) + d) * np.cos(0.9), float(cy) + (float(thr) + d) * np.sin(0.9)) for d in CULL_DELTAS]
    spots += [(float(cx) - 0.4, float(cy) - (float(hm) + d)) for d in CULL_DELTAS]
    out = []
    for part in _chunks(spots, ocfg.n_agents - 1):
        s = _Scene(ocfg, rng, "cull-boundary")
        s.rect(0, (0.75, 0.75), 0.2, 0.25, ROBUST)
        for i, (x, y) in enumerate(part):
            s.at(i, x, y)
        s.at(ocfg.n_agents - 1, 0.75, 0.45)
        out.append(s)
    return out


def _mask_radius(ocfg, rng):
    """one env per distance.  agents 0 - 1 (along x) and agent 0 - goal 0 (along y) that far apart (comm_radius); agent 2 that far (the
    LiDAR mask radius) from the leftmost vertex of a turned rectangle, which its ray 16 points at"""
    out = []
    for d_comm, d_lidar in zip(three(ocfg.comm_radius), three(lidar_radius(ocfg))):
        s = _Scene(ocfg, rng, "mask-radius")
        s.at(0, 0.0, 0.0)                                                # from the origin the coordinate is the distance, exactly
        s.at(1, d_comm, 0.0)
        s.goal[0, 0], s.goal[0, 1] = f32(0.0), d_comm
        rec = s.rect(0, (1.0, 0.4), 0.25, 0.15, 0.7)
        xs, ys = rec[8:16:2], rec[9:16:2]
        m = int(np.argmin(xs))
        s.at(2, f32(xs[m] - d_lidar), ys[m])
        out.append(s)
    return out


def _clean(ocfg, rng, tag="clean"):
    """a scene as the suite draws them: oracle reset, agents pulled together, random velocities and actions"""
    s = _Scene(ocfg, rng, tag)
    agent, goal, obst = E.env_reset(ocfg, rng.integers(1, 2 ** 62, size=1))
    n, v = ocfg.n_agents, ocfg.vel_limit
    agent = agent[0].copy()
    agent[:, :2] = (agent[:, :2] * 0.5 + 0.4).astype(f32)
    if ocfg.is_bicycle:
        th = rng.uniform(0, 2 * np.pi, size=n)
        agent[:, 2], agent[:, 3], agent[:, 4] = np.cos(th), np.sin(th), rng.uniform(-0.5, 0.5, size=n)
    else:
        agent[:, 2:4] = rng.uniform(-v, v, size=(n, 2))
    s.agent, s.goal, s.obst = agent.astype(f32), goal[0], obst[0]
    return s


NON_FINITE = ("action-nan", "action-inf", "position-nan", "velocity-nan", "velocity-inf")
NF_AGENT = 1                          # the agent the non-finite value is given to


def _non_finite(ocfg, rng):
    """each in an otherwise clean env.  `velocity`: the x velocity of the double integrator, the speed of the bicycle"""
    out = []
    vcol = 4 if ocfg.is_bicycle else 2
    for name in NON_FINITE:
        s = _clean(ocfg, rng, "non-finite/" + name)
        if name == "action-nan":
            s.action[NF_AGENT, 0] = np.nan
        elif name == "action-inf":
            s.action[NF_AGENT] = (np.inf, -np.inf)
            s.action[0] = (-np.inf, np.inf)
        elif name == "position-nan":
            s.agent[NF_AGENT, 0] = np.nan
        elif name == "velocity-nan":
            s.agent[NF_AGENT, vcol] = np.nan
        else:
            s.agent[NF_AGENT, vcol] = np.inf
        out.append(s)
    return out


_BUILDERS = {"axis-aligned": _axis_aligned, "parallel-to-ray": _parallel, "weak-threshold": _weak, "on-vertex": _on_vertex,
             "ties-beside-nan-agent": _ties_beside_nan_agent,
             "symmetric-ties": _symmetric_ties, "graze": _graze, "cull-boundary": _cull_boundary, "mask-radius": _mask_radius,
             "non-finite": _non_finite}


def build(ocfg, seed, only=None):
    """the catalogue for one LiDAR config (n_agents >= 4, n_obs >= 1); `only`: the scene names to keep, in catalogue order"""
    assert ocfg.is_lidar and ocfg.n_agents >= 4 and ocfg.n_obs >= 1
    rng = np.random.default_rng(seed)
    envs = []
    for name in SCENES:
        if only is not None and name not in only:
            continue
        if name == "clean":
            continue
        envs += _BUILDERS[name](ocfg, rng)
    if only is None or "clean" in only:                                   # two clean envs between the others
        for pos in (len(envs) // 3, 2 * len(envs) // 3 + 1):
            envs.insert(pos, _clean(ocfg, rng))
    stack = lambda key: np.stack([getattr(s, key) for s in envs]).astype(f32)
    return stack("agent"), stack("goal"), stack("obst"), stack("action"), [s.tag for s in envs]


def env_ids(tags, name):
    """indices of the envs whose tag is `name` or starts with `name/`"""
    return [b for b, t in enumerate(tags) if t == name or t.startswith(name + "/")]
