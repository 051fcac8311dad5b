"""Hand-built VMASReverseTransport states for the branches of csrc/env_vmas.hip that a state drawn at random never takes: the
contact force exactly at, one float above and one float below its two distance thresholds, a corner equidistant from two sides,
an agent abeam of a side's centre (dot == 0), beyond a side's end and outside the box, contact that changes sides within a step,
the world clamp, cost margins and the reward term exactly at their thresholds, the in-contact flag at 0.59, actions at and beyond
the clip, and non-finite actions and states.  A plain helper module (like vmas_np.py and env_edge_scenes.py): numpy and the
restatement only, not collected by pytest.

scenes(n) -> dict(agent [B, n, 4], body [B, 4], scene [B, 8], action [B, n, 2], tags [B]); one env per scene, tags[b] names it as
"family/case".  Agent 0 (and agent 1 where a scene needs a pair) carries the case; every other agent is parked deep inside the
box with a small random velocity and action, where it meets no side.  The exact cases put the side (or the other agent, the
obstacle, the goal) at coordinate 0, so that the distance IS the agent's coordinate: sqrt(x * x) == |x| in binary floating
point.  tests/test_vmas_edges_cpu.py proves on the restatement alone that each scene takes the branch its tag names.

The upper clip of the cost (+1) cannot be reached: the margins are at most 4 * 0.06 + 0.5 = 0.74 (coincident agents) and
2 * 0.15 + 0.5 = 0.8 (the box on an obstacle); those two largest values are in the catalogue instead."""
import numpy as np

import vmas_np as V

f32 = np.float32
H = V.HALF_SIDE
H2X = f32(V.C90 * V.HALF_SIDE)         # x offset of the centres of sides 3 and 4: cos(fp32(pi / 2)) * 0.3 = -1.3e-8
NF_AGENT = -1                          # the agent a non-finite value is given to: the last one, next to the dead lanes of its group
NON_FINITE = ("action-nan", "position-nan", "velocity-nan", "box-nan", "obstacle-nan", "goal-nan", "velocity-inf", "position-inf")
PAIR_FAMILIES = ("cost-margins/agent-below", "cost-margins/agent-at", "cost-margins/agent-above", "cost-margins/coincident")
SLOTS = [(f32(0.09 * i), f32(0.09 * j)) for j in (0, -1, 1, -2, 2) for i in (0, -1, 1, -2, 2)]     # parking places, box-relative


def three(r):
    """nextafter(r, 0), r, nextafter(r, 1) in fp32, named below / at / above"""
    r = f32(r)
    return (("below", np.nextafter(r, f32(0))), ("at", r), ("above", np.nextafter(r, f32(1))))


def side_distances(px, py, bx, by):
    """distance from (px, py) to the closest point of each of the four sides, in get_all_lines_box order, and those points"""
    px, py, bx, by = (np.asarray(v, f32) for v in (px, py, bx, by))
    h2y = f32(V.S90 * H)
    lines = ((bx + H, by + f32(0) * H, V.C90, V.S90), (bx - H, by - f32(0) * H, V.C90, V.S90),
             (bx + H2X, by + h2y, f32(1), f32(0)), (bx - H2X, by - h2y, f32(1), f32(0)))
    d, q = [], []
    for lx, ly, rx, ry in lines:
        qx, qy = V._closest_on_line(np.asarray(lx, f32), np.asarray(ly, f32), rx, ry, px, py)
        d.append(f32(V.norm2((px - qx).astype(f32), (py - qy).astype(f32))))
        q.append((f32(qx), f32(qy)))
    return d, q


def corner_tie_inside(a=0.03):
    """box centre and agent position for an agent inside the box, `a` from side 1 and exactly as far from side 3.  The corner
    of sides 1 and 3 is put at (0, 0); the distance to side 1 is not quite a (its closest point is off by cos(fp32(pi / 2))
    times the offset along the side), so y is set to that distance, which is then the distance to side 3 exactly."""
    bx = by = -H
    px, py = f32(-a), f32(-a)
    for _ in range(4):
        d, _ = side_distances(px, py, bx, by)
        py = f32(-d[0])
    return (bx, by), (px, py)


class _Env:
    def __init__(self, n, seed, tag, box, box_vel=(0.0, 0.0)):
        self.n, self.tag = n, tag
        self.rng = np.random.default_rng(seed)
        bx, by = f32(box[0]), f32(box[1])
        self.body = np.array([bx, by, box_vel[0], box_vel[1]], f32)
        # goal and obstacles out of everybody's way, at distances that differ
        self.scene = np.array([bx + f32(0.4), by + f32(0.1), bx - f32(0.6), by + f32(0.6), bx + f32(0.7), by + f32(0.6),
                               bx - f32(0.6), by - f32(0.8)], f32)
        self.special = {}

    def put(self, i, pos, vel=(0.0, 0.0), act=(0.0, 0.0)):
        self.special[i] = (np.array([pos[0], pos[1], vel[0], vel[1]], f32), np.array(act, f32))
        return self

    def finish(self):
        """park the agents that carry no case on the slots at least 0.075 from every agent that does"""
        n, bx, by = self.n, self.body[0], self.body[1]
        self.agent, self.action = np.zeros((n, 4), f32), np.zeros((n, 2), f32)
        taken = [s[0][:2] for i, s in self.special.items() if i < n]
        free = [(bx + sx, by + sy) for sx, sy in SLOTS
                if all(np.hypot(float(bx + sx) - float(t[0]), float(by + sy) - float(t[1])) > 0.075 for t in taken)]
        vel = self.rng.uniform(-0.05, 0.05, (n, 2)).astype(f32)
        act = self.rng.uniform(-1.5, 1.5, (n, 2)).astype(f32)
        k = 0
        for i in range(n):
            if i in self.special:
                self.agent[i], self.action[i] = self.special[i]
            else:
                self.agent[i, :2], self.agent[i, 2:], self.action[i] = free[k], vel[i], act[i]
                k += 1
        return self


def _catalogue(n):
    """the finite scenes and the bases of the action and non-finite families"""
    out = []
    seed = [n * 1000]

    def env(tag, box, **kw):
        seed[0] += 1
        e = _Env(n, seed[0], tag, box, **kw)
        out.append(e)
        return e

    Y = f32(0.125)
    # side 1 on the line x = 0: an agent at (-d, Y) is d from it
    for name, d in three(V.DIST_MIN):
        env("contact-threshold/" + name, (-H, Y)).put(0, (-d, Y))
    env("on-the-side/centre", (-H, Y)).put(0, (0.0, Y))
    for name, d in three(V.MIN_DIST):
        env("on-the-side/min-dist-" + name, (-H, Y)).put(0, (-d, Y))
    box, pos = corner_tie_inside()
    env("corner-tie/inside", box).put(0, pos)
    env("corner-tie/outside", (0.0, 0.0)).put(0, (H + f32(0.02), H + f32(0.02)))
    env("abeam-centre", (0.0, -H)).put(0, (H2X, -0.03))                     # side 3 on y = 0, its centre at x = H2X
    B0 = (f32(0.1), f32(-0.2))
    env("past-the-end", B0).put(0, (B0[0] + H + f32(0.01), B0[1] + H + f32(0.02)), act=(-0.3, 0.2))
    env("outside-the-box", B0).put(0, (B0[0] + H + f32(0.02), B0[1] + f32(0.05)), act=(0.2, -0.4))
    env("deep-inside", B0)
    env("two-sides", B0).put(0, (B0[0] + H - f32(0.02), B0[1] + H - f32(0.03)))
    env("world-clamp/plus", (0.2, 1.195), box_vel=(0.0, 0.5)).put(0, (1.195, 0.5), vel=(0.5, 0.1), act=(1.0, 0.0))
    env("world-clamp/minus", (-0.2, -1.195), box_vel=(0.0, -0.5)).put(0, (-1.195, -0.5), vel=(-0.5, 0.1), act=(-1.0, 0.0))
    if n > 1:
        for name, d in three(V.TWO_AGENT_R):
            env("cost-margins/agent-" + name, (-0.015, -0.045)).put(0, (0.0, 0.0), (0.01, 0.02), (0.5, -0.5)).put(
                1, (d, 0.0), (-0.02, 0.01), (-0.5, 0.25))
        env("cost-margins/coincident", (0.0, 0.0)).put(0, (0.01, 0.02), (0.01, 0.0), (0.5, 0.5)).put(
            1, (0.01, 0.02), (0.0, -0.01), (0.25, -0.5))
    for name, d in three(V.OBS_R):
        e = env("cost-margins/obstacle-" + name, (0.0, 0.0))
        e.scene[2:4] = (d, 0.0)
    e = env("cost-margins/obstacle-tie", (0.0, 0.0))
    e.scene[2:8] = (0.0, 0.25, 0.5, 0.0, 0.25, 0.0)                          # obstacles 0 and 2 tie, nearer than obstacle 1
    e = env("cost-margins/on-obstacle", B0)
    e.scene[2:4] = B0                                                        # the largest obstacle cost: 0.8
    env("cost-margins/far", B0)                                              # the obstacle cost clipped to -1
    for name, d in three(V.DIST2GOAL):
        e = env("reward-threshold/" + name, (0.0, 0.0))
        e.scene[0:2] = (d, 0.0)
    (_, _), (_, t), (_, t1) = three(V.CONTACT_THR)
    for name, pos in (("x-at", (t, 0.0)), ("x-above", (t1, 0.0)), ("x-neg-above", (-t1, 0.0)), ("y-at", (0.0, t)),
                      ("y-above", (0.0, t1))):
        env("flag-threshold/" + name, (0.0, 0.0)).put(0, pos)               # outside the box, at rest: it stays there
    return out


ACTIONS = {"zero": (0.0, 0.0), "negzero": (-0.0, -0.0), "one": (1.0, -1.0), "beyond": (1.5, -2.5), "inf": (np.inf, -np.inf)}


def scenes(n):
    assert 1 <= n <= 16
    envs = [e.finish() for e in _catalogue(n)]
    B0 = (f32(0.1), f32(-0.2))
    for name, a in ACTIONS.items():                                          # one state, every agent given the action
        e = _Env(n, n * 1000 + 500, "actions/" + name, B0).finish()
        e.action[:] = np.array(a, f32)
        envs.append(e)
    for name in NON_FINITE:                                                  # one state, one non-finite value
        e = _Env(n, n * 1000 + 600, "non-finite/" + name, B0).finish()
        if name == "action-nan":
            e.action[NF_AGENT, 0] = np.nan
        elif name == "position-nan":
            e.agent[NF_AGENT, 0] = np.nan
        elif name == "velocity-nan":
            e.agent[NF_AGENT, 2] = np.nan
        elif name == "box-nan":
            e.body[0] = np.nan
        elif name == "obstacle-nan":
            e.scene[2] = np.nan
        elif name == "goal-nan":
            e.scene[0] = np.nan
        elif name == "velocity-inf":
            e.agent[NF_AGENT, 2] = np.inf
        else:
            e.agent[NF_AGENT, 0] = np.inf
        envs.append(e)
    stack = lambda key: np.stack([getattr(e, key) for e in envs]).astype(f32)
    return dict(agent=stack("agent"), body=stack("body"), scene=stack("scene"), action=stack("action"),
                tags=tuple(e.tag for e in envs))


def free_flight(agent, action):
    """agent [.., 4] after one step on which no contact force acts, in the restatement's fp32 order (vmas_np.physics with
    f = 0): what an agent whose force is off at every substep must give bit for bit"""
    u = (np.clip(action.astype(f32), f32(-1), f32(1)) * V.U_MULT).astype(f32)
    p, v = agent[..., :2].astype(f32).copy(), agent[..., 2:].astype(f32).copy()
    F = (u + f32(0)).astype(f32)
    for _ in range(V.FRAME_SKIP):
        for s in range(V.SUBSTEPS):
            if s == 0:
                v = (v * V.DRAG_KEEP).astype(f32)
            v = (v + (F / f32(1)) * V.SUB_DT).astype(f32)
            p = np.clip((p + v * V.SUB_DT).astype(f32), -V.SEMIDIM, V.SEMIDIM)
    return np.concatenate([p, v], -1).astype(f32)


def env_ids(tags, name):
    """indices of the envs whose tag is `name` or starts with `name/`"""
    return [b for b, t in enumerate(tags) if t == name or t.startswith(name + "/")]


def finite_ids(tags):
    """the envs whose outputs are finite: all but the non-finite family (actions/inf clips to actions/one)"""
    return [b for b, t in enumerate(tags) if not t.startswith("non-finite/")]
