"""Hand-built scenes for the paths of the MPE env step (env_step_kernel, csrc/env_step.hip) that a scene drawn at random never
takes: distances one ulp either side of the mask radii, cost margins on the zero where cost_value jumps by 1.0 and on the -1
clip, coincident bodies, the connectivity cost at its radius, goals one ulp around dist2goal, positions and velocities on
their limits, actions on the clip, and non-finite states, actions, obstacles and goals.  A plain helper module (like
env_edge_scenes.py): numpy and the oracle only.

build(ocfg, seed) -> (agent [B, n, 4], goal [B, n_goals, 4], obst [B, n_obs, 4] or None, action [B, n, 2], tags [B]); one env
per scene instance, tags[b] names the scene of env b ("scene" or "scene/instance").  Velocities are zero wherever a scene
depends on an exact position of the t+1 graph (x' = vx * dt + x leaves x where it is), and the agents a scene does not use
are parked on a grid wider than comm_radius.  tests/test_mpe_edges_cpu.py proves on the oracle alone that each scene reaches
its path."""
import numpy as np

from oracle import env_np as E
from env_edge_scenes import env_ids, three  # noqa: F401  (three: nextafter(r, 0), r, nextafter(r, 1); env_ids: re-exported)

f32 = np.float32
FAR = (-3.0, -3.0)                    # an obstacle nobody is near (obstacle discs are not confined to the area)
LO = 0.05                             # the parking grid starts here; its spacing follows from the area (see _spacing)
GRID = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2), (2, 2)]      # agent i parks on cell GRID[i]
ALONG_X, ALONG_Y = 0.05, np.pi / 2 - 0.05      # directions (rad) in which agents 1 and 2 approach agent 0: off the axes, so
                                               # that both squares of the distance vary in the search of at_distance
SCENES = ("comm-radius", "obs-mask-radius", "agent-cost-zero", "obs-cost-zero", "cost-floor", "coincident", "connectivity",
          "goal-reached", "walls", "action-clip", "non-finite", "clean")
ACTION_VALUES = (f32(1), f32(-1), np.nextafter(f32(1), f32(np.inf)), np.nextafter(f32(-1), f32(-np.inf)), f32(np.inf),
                 f32(-np.inf), f32(-0.0), f32(1e-30))
NON_FINITE = ("position-nan", "position-inf", "position-neg-inf", "velocity-nan", "action-nan", "obstacle-nan", "goal-nan")
NF_AGENT = 1                          # the agent (obstacle 0, goal 0) the non-finite value is given to
N_CLEAN = 4

# Which configs legitimately lack which scene (or instance of a scene); everything else is present for every MPE config:
#   connectivity               the third cost exists in MPEConnectSpread only (n_cost == 3)
#   obs-mask-radius            needs an obstacle
#   coincident/on-obstacle     needs an obstacle
#   non-finite/obstacle-nan    needs an obstacle
#   goal-reached/tie           two agents equally near one goal: the kinds whose reward takes a minimum over the agents and
#                              whose reward goals are the goal nodes themselves (MPESpread, MPECorridor, MPEConnectSpread)
# obs-cost-zero stays for n_obs == 0: one env, whose obstacle cost must be -0.5 exactly.
def supports(ocfg, name):
    """whether the config has the scene or instance `name`"""
    if name == "connectivity":
        return ocfg.n_cost == 3
    if name in ("obs-mask-radius", "coincident/on-obstacle", "non-finite/obstacle-nan"):
        return ocfg.n_obs > 0
    if name == "goal-reached/tie":
        return ocfg.is_spread and ocfg.reward_goals == E.GOALS_NODES
    return True


def always_connected(ocfg):
    """MPECorridor / MPEConnectSpread: the obstacle mask radius is 100 x comm_radius"""
    return ocfg.kind in (E.MPE_CORRIDOR, E.MPE_CONNECT_SPREAD)


def car_plus_obs(ocfg):
    """the obstacle cost's radius, formed in double and rounded once as the oracle and make_env_cfg form it"""
    return f32(ocfg.car_radius + ocfg.obs_radius)


def floor_radius(ocfg):
    """the nearest-neighbour distance at which the agent cost meets its lower clip"""
    return f32(ocfg.car_radius * 2 + 0.5)


def _bits_around(v, span):
    """the 2 * span + 1 floats around v > 0, in order"""
    v = np.asarray(v, f32)
    assert v > 0
    return (v.view(np.int32) + np.arange(-span, span + 1, dtype=np.int32)).view(f32)


def at_distance(x0, y0, r, angle, span=64):
    """a point (x, y) near (x0, y0) + r * (cos, sin)(angle) whose fp32 distance from (x0, y0) — sqrt(dx * dx + dy * dy) in
    the oracle's operation order (E.norm2) — equals r exactly; found by searching the floats around the ideal point"""
    x0, y0, r = f32(x0), f32(y0), f32(r)
    if r == 0:
        return x0, y0
    xs = _bits_around(f32(float(x0) + float(r) * np.cos(angle)), span)
    ys = _bits_around(f32(float(y0) + float(r) * np.sin(angle)), span)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    hit = np.argwhere(E.norm2((x0 - X).astype(f32), (y0 - Y).astype(f32)) == r)
    assert len(hit), f"no point at distance {r!r} from ({x0!r}, {y0!r})"
    i, j = hit[np.argmin(np.abs(hit - span).sum(axis=1))]
    return xs[i], ys[j]


def _spacing(ocfg):
    """the parking grid: three columns 0.7 apart in the 1.5 area, two 0.9 apart in the 1.0 area — both above comm_radius and
    above floor_radius, so that a parked agent is nobody's nearest neighbour in a cost scene"""
    return 0.7 if ocfg.area_size >= 1.5 else 0.9


def park(ocfg, i):
    sp = _spacing(ocfg)
    cx, cy = GRID[i]
    assert LO + sp * max(cx, cy) <= ocfg.area_size, "no parking cell for this agent"
    return f32(LO + sp * cx), f32(LO + sp * cy)


class _Scene:
    """one env under construction: agents parked apart at rest, goals at random, every obstacle out of reach"""

    def __init__(self, ocfg, rng, tag):
        n, A = ocfg.n_agents, ocfg.area_size
        self.ocfg, self.tag = ocfg, tag
        self.agent = np.zeros((n, 4), f32)
        self.agent[:, :2] = np.asarray([park(ocfg, i) for i in range(n)], f32)
        self.goal = np.zeros((ocfg.n_goals, 4), f32)
        self.goal[:, :2] = rng.uniform(0.3, A - 0.3, size=(ocfg.n_goals, 2))
        self.obst = np.zeros((ocfg.n_obs, 4), f32)
        for o in range(ocfg.n_obs):
            self.obst[o, :2] = (FAR[0] - o, FAR[1])
        self.action = rng.uniform(-1.5, 1.5, size=(n, 2)).astype(f32)

    def at(self, i, x, y):
        self.agent[i, 0], self.agent[i, 1] = f32(x), f32(y)

    def near0(self, i, r, angle):
        """agent i at fp32 distance r from agent 0"""
        self.at(i, *at_distance(self.agent[0, 0], self.agent[0, 1], r, angle))

    def obst_near0(self, o, r, angle):
        """obstacle o at fp32 distance r from agent 0"""
        self.obst[o, 0], self.obst[o, 1] = at_distance(self.agent[0, 0], self.agent[0, 1], r, angle)


def _pair_at(ocfg, rng, name, radius):
    """one env per distance of three(radius): agent 1 that far from agent 0"""
    out = []
    for k, d in enumerate(three(radius)):
        s = _Scene(ocfg, rng, f"{name}/{('below', 'on', 'above')[k]}")
        s.near0(1, d, ALONG_X)
        out.append(s)
    return out


def _comm_radius(ocfg, rng):
    return _pair_at(ocfg, rng, "comm-radius", ocfg.comm_radius)


def _obs_mask_radius(ocfg, rng):
    """obstacle 0 at three(comm_radius) from agent 0; where the obstacle edges are always connected, the obstacles stay where
    _Scene parks them, farther than comm_radius from everybody"""
    if always_connected(ocfg):
        return [_Scene(ocfg, rng, "obs-mask-radius/far")]
    out = []
    for k, d in enumerate(three(ocfg.obs_mask_radius)):
        s = _Scene(ocfg, rng, f"obs-mask-radius/{('below', 'on', 'above')[k]}")
        s.obst_near0(0, d, ALONG_Y)
        out.append(s)
    return out


def _agent_cost_zero(ocfg, rng):
    return _pair_at(ocfg, rng, "agent-cost-zero", f32(ocfg.car_radius * 2))


def _obs_cost_zero(ocfg, rng):
    if ocfg.n_obs == 0:
        return [_Scene(ocfg, rng, "obs-cost-zero/no-obstacle")]
    out = []
    for k, d in enumerate(three(car_plus_obs(ocfg))):
        s = _Scene(ocfg, rng, f"obs-cost-zero/{('below', 'on', 'above')[k]}")
        s.obst_near0(ocfg.n_obs - 1, d, ALONG_Y)                          # the last obstacle: the minimum is not its first term
        out.append(s)
    return out


def agent_cost_before_clip(ocfg, d):
    """cost_value(two_car_radius - d) for a nearest-neighbour distance d, in the oracle's fp32 order (E.get_cost)"""
    m = f32(f32(ocfg.car_radius * 2) - f32(d))
    return f32(m - f32(0.5)) if m <= 0 else f32(m + f32(0.5))


def _cost_floor(ocfg, rng):
    """three(floor_radius) — the cost before its clip rounds onto -1 around there — and the nearest distances either side at
    which it is above -1 (kept) and below -1 (clipped)"""
    out = _pair_at(ocfg, rng, "cost-floor", floor_radius(ocfg))
    for tag, toward, past in (("kept", f32(0), lambda v: v > -1), ("clipped", f32(1), lambda v: v < -1)):
        d = floor_radius(ocfg)
        while not past(agent_cost_before_clip(ocfg, d)):
            d = np.nextafter(d, toward)
        s = _Scene(ocfg, rng, f"cost-floor/{tag}")
        s.near0(1, d, ALONG_X)
        out.append(s)
    return out


def _coincident(ocfg, rng):
    s = _Scene(ocfg, rng, "coincident/agents")
    s.at(1, s.agent[0, 0], s.agent[0, 1])
    s.action[1] = s.action[0]                                             # the same velocity at t+1: all four edge features zero
    out = [s]
    if supports(ocfg, "coincident/on-obstacle"):
        s = _Scene(ocfg, rng, "coincident/on-obstacle")
        s.obst[0, :2] = s.agent[0, :2]
        out.append(s)
    return out


def _connectivity(ocfg, rng):
    """agents 0, 1 a close pair; agents 2, 3 each other's nearest neighbour at three(connect_radius): the largest
    nearest-neighbour distance of the team.  Then one straggler beyond the +1 clip, and a tight cluster"""
    assert ocfg.n_agents == 4
    out = []
    for k, d in enumerate(three(ocfg.connect_radius)):
        s = _Scene(ocfg, rng, f"connectivity/{('below', 'on', 'above')[k]}")
        s.near0(1, f32(0.2), ALONG_X)
        s.at(3, *at_distance(s.agent[2, 0], s.agent[2, 1], d, ALONG_X))
        out.append(s)
    for tag, last in (("straggler", (0.95, 1.9)), ("cluster", (0.17, 0.17))):
        s = _Scene(ocfg, rng, f"connectivity/{tag}")
        s.at(1, 0.17, 0.05)
        s.at(2, 0.05, 0.17)
        s.at(3, *last)
        out.append(s)
    return out


def goal_index(ocfg):
    """the reward goal of the goal-reached scene: an interior one where the goals are derived from landmarks"""
    return 0 if ocfg.reward_goals == E.GOALS_NODES else 1


def _goal_reached(ocfg, rng):
    """agent 0 at distance 0 and three(dist2goal) from reward goal goal_index (its own goal in MPETarget); MPEFormation, whose
    goals come from device cosf / sinf, only at half and at twice dist2goal.  Then two agents bit-equally far from goal 0"""
    g = goal_index(ocfg)
    if ocfg.kind == E.MPE_FORMATION:
        dists = [("inside", f32(ocfg.dist2goal * 0.5)), ("outside", f32(ocfg.dist2goal * 2))]
    else:
        dists = [("zero", f32(0))] + list(zip(("below", "on", "above"), three(ocfg.dist2goal)))
    out = []
    for tag, d in dists:
        s = _Scene(ocfg, rng, f"goal-reached/{tag}")
        if out:
            s.goal[:] = out[0].goal                                       # the same goals throughout: only agent 0's distance differs
        if ocfg.reward_goals == E.GOALS_NODES:
            s.goal[0, :2] = (0.4, 0.3)
        elif ocfg.kind == E.MPE_FORMATION:
            s.goal[0, :2] = (0.75, 0.75)
        else:
            s.goal[0, :2], s.goal[1, :2] = (0.3, 0.35), (1.2, 0.95)
        rg = E.reward_goal_positions(ocfg, s.goal[None])[0, g]            # the oracle's own goal position
        s.at(0, *at_distance(rg[0], rg[1], d, 0.7))
        out.append(s)
    if supports(ocfg, "goal-reached/tie"):
        s = _Scene(ocfg, rng, "goal-reached/tie")
        s.at(0, 0.25, 0.25)
        s.at(1, 0.5, 0.25)
        s.goal[0, :2] = (0.375, 0.25)
        out.append(s)
    return out


def _walls(ocfg, rng):
    """positions on the limits with the velocity pointing outward and inward; then velocities on the limits with the action
    pushing outward, and a -0.0 velocity"""
    A, Y, v, n = f32(ocfg.area_size), f32(ocfg.y_limit), f32(ocfg.vel_limit), ocfg.n_agents
    s = _Scene(ocfg, rng, "walls/position")
    s.agent[0] = (0, 0, -0.5, -0.5)                                       # outward at both lower walls
    s.agent[1] = (A, Y, 0.5, 0.5)                                         # outward at both upper walls
    s.agent[2] = (0, A, 0.5, 0.5 if Y > A else -0.5)                      # inward in x; in y inward, or on past A where y may go to 2 A
    if n >= 4:
        s.agent[3] = (0.5, 1.5 * A, 0.0, 0.25) if Y > A else (A, 0, -0.5, 0.5)
    t = _Scene(ocfg, rng, "walls/velocity")
    t.agent[0, 2:], t.action[0] = (v, -v), (1.5, -1.5)
    t.agent[1, 2:], t.action[1] = (-v, v), (-1.0, 1.0)
    t.agent[2, 2:], t.action[2] = (-0.0, -0.0), (-0.0, 0.0)
    return [s, t]


def _action_clip(ocfg, rng):
    """every value of ACTION_VALUES in some action component, in as many envs as that takes"""
    per = 2 * ocfg.n_agents
    out = []
    for start in range(0, len(ACTION_VALUES), per):
        s = _Scene(ocfg, rng, "action-clip")
        vals = ACTION_VALUES[start:start + per]
        s.action.reshape(-1)[:len(vals)] = vals
        out.append(s)
    return out


def _clean(ocfg, rng, tag="clean"):
    """a scene as the suite draws them: oracle reset, agents pulled together, random velocities and actions"""
    s = _Scene(ocfg, rng, tag)
    agent, goal, obst = E.env_reset(ocfg, rng.integers(1, 2 ** 62, size=1))
    agent = agent[0].copy()
    agent[:, :2] = (agent[:, :2] * 0.5 + 0.4).astype(f32)
    agent[:, 2:4] = rng.uniform(-ocfg.vel_limit, ocfg.vel_limit, size=(ocfg.n_agents, 2))
    s.agent, s.goal = agent.astype(f32), goal[0]
    if ocfg.n_obs > 0:
        s.obst = obst[0]
    return s


def _non_finite(ocfg, rng):
    """each in an otherwise clean env of its own"""
    out = []
    for name in NON_FINITE:
        if not supports(ocfg, "non-finite/" + name):
            continue
        s = _clean(ocfg, rng, "non-finite/" + name)
        if name == "position-nan":
            s.agent[NF_AGENT, 0] = np.nan
        elif name == "position-inf":
            s.agent[NF_AGENT, 0] = np.inf
        elif name == "position-neg-inf":
            s.agent[NF_AGENT, 1] = -np.inf
        elif name == "velocity-nan":
            s.agent[NF_AGENT, 2] = np.nan
        elif name == "action-nan":
            s.action[NF_AGENT, 0] = np.nan
        elif name == "obstacle-nan":
            s.obst[0, 0] = np.nan
        else:
            s.goal[0, 0] = np.nan
        out.append(s)
    return out


_BUILDERS = {"comm-radius": _comm_radius, "obs-mask-radius": _obs_mask_radius, "agent-cost-zero": _agent_cost_zero,
             "obs-cost-zero": _obs_cost_zero, "cost-floor": _cost_floor, "coincident": _coincident,
             "connectivity": _connectivity, "goal-reached": _goal_reached, "walls": _walls, "action-clip": _action_clip,
             "non-finite": _non_finite}


def build(ocfg, seed, only=None):
    """the catalogue for one MPE config (n_agents >= 3); `only`: the scene names to keep, in catalogue order.  The clean envs
    sit among the others: one a third of the way in, one before, one inside and one after the non-finite block"""
    assert not ocfg.is_lidar and ocfg.state_dim == 4 and ocfg.n_agents >= 3
    rng = np.random.default_rng(seed)
    envs = []
    for name in SCENES:
        if name == "clean" or (only is not None and name not in only) or not supports(ocfg, name):
            continue
        envs += _BUILDERS[name](ocfg, rng)
    if only is None or "clean" in only:
        nf = [b for b, s in enumerate(envs) if s.tag.startswith("non-finite")]
        first, last = (nf[0], nf[-1]) if nf else (len(envs), len(envs) - 1)
        spots = sorted({len(envs) // 3, first, (first + last + 1) // 2, last + 1})
        for k, pos in enumerate(spots):                                   # earlier insertions shift the later spots by one each
            envs.insert(pos + k, _clean(ocfg, rng))
    stack = lambda key: np.stack([getattr(s, key) for s in envs]).astype(f32)
    obst = stack("obst") if ocfg.n_obs > 0 else None
    return stack("agent"), stack("goal"), obst, stack("action"), [s.tag for s in envs]
