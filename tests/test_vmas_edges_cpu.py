"""The hand-built VMASReverseTransport states of tests/vmas_edge_scenes.py on the restatement alone (tests/vmas_np.py): every
scene takes the branch its tag names, no contact scene comes near a force threshold after its first substep (where the device
is a few ulps off the restatement and the force jumps by 2.08), the non-finite scenes put NaN where the GPU test then looks for
it, the restatement's contact force agrees with a float64 closed form, and the reset seeds of the GPU test do restart."""
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vmas_edge_scenes as S  # noqa: E402
import vmas_np as V  # noqa: E402

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")
f32 = np.float32
TEAMS = (1, 2, 3, 5, 8, 9, 15, 16)


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(n):
    s = S.scenes(n)
    a, b, sc, u = s["agent"], s["body"], s["scene"], s["action"]
    out = V.env_step(a, b, sc, u)
    _, _, _, near = V.physics(a, b, u, trace=True)
    fx, fy, on, dist = V.contact_force(a[..., 0], a[..., 1], b[:, 0:1], b[:, 1:2], with_dist=True)
    by = {t: i for i, t in enumerate(s["tags"])}
    return dict(s, out=out, near=near, fx=fx, fy=fy, on=on, dist=dist, by=by, free=S.free_flight(a, u),
                margins=V.cost_margins(a, b, sc))


def test_sqrt_of_a_square_is_exact_for_the_threshold_values():
    for x in (V.TWO_AGENT_R, V.DIST_MIN, V.MIN_DIST, V.OBS_R, V.DIST2GOAL):
        for _, v in S.three(x):
            assert np.sqrt(f32(v * v)) == v


@pytest.mark.parametrize("n", TEAMS)
def test_every_tag_takes_its_branch(n):
    r = _ref(n)
    by, a, b, out, on, dist = r["by"], r["agent"], r["body"], r["out"], r["on"], r["dist"]
    nx, free = out["next_agent"], r["free"]
    kicked = lambda e: np.abs(nx[e, 0, 2:].astype(np.float64) - free[e, 0, 2:]) > 1e-3
    same = lambda e: np.array_equal(_bits(nx[e, 0]), _bits(free[e, 0]))
    # only agent 0 of a scene ever touches the box
    assert not on[S.finite_ids(r["tags"]), 1:].any()

    # ---- the force thresholds, decided at substep 0 from exact inputs ----
    for (name, d), want_on in zip(S.three(V.DIST_MIN), (True, True, False)):
        e = by["contact-threshold/" + name]
        assert dist[e, 0] == d and on[e, 0] == want_on
        assert kicked(e)[0] if want_on else (same(e) and not out["contact"][e])
    assert dist[by["contact-threshold/at"], 0] == V.DIST_MIN
    e = by["on-the-side/centre"]
    assert dist[e, 0] == 0 and not on[e, 0] and same(e) and not out["contact"][e]
    for (name, d), want_on in zip(S.three(V.MIN_DIST), (False, True, True)):
        e = by["on-the-side/min-dist-" + name]
        assert dist[e, 0] == d and on[e, 0] == want_on
        assert kicked(e)[0] if want_on else (same(e) and not out["contact"][e])
    assert abs(float(r["fx"][by["on-the-side/min-dist-above"], 0])) > 18.0        # the deepest penetration: 500 * 0.0367

    # ---- ties and geometry ----
    e = by["corner-tie/inside"]
    d, q = S.side_distances(a[e, 0, 0], a[e, 0, 1], b[e, 0], b[e, 1])
    assert d[0] == d[2] == min(d) and q[0] != q[2] and on[e, 0]
    assert r["fx"][e, 0] < -1.0 and abs(r["fy"][e, 0]) < 1e-3                       # side 1 wins: pushed along -x, not along -y
    e = by["corner-tie/outside"]
    d, q = S.side_distances(a[e, 0, 0], a[e, 0, 1], b[e, 0], b[e, 1])
    assert d[0] == d[2] == min(d) and on[e, 0] and r["fx"][e, 0] > 1.0 and r["fy"][e, 0] > 1.0
    e = by["abeam-centre"]
    assert f32(f32(b[e, 0] + S.H2X) - a[e, 0, 0]) == 0 and on[e, 0]                 # dot == 0 on side 3
    assert r["fy"][e, 0] < -1.0 and r["fx"][e, 0] == 0
    e = by["past-the-end"]
    d, q = S.side_distances(a[e, 0, 0], a[e, 0, 1], b[e, 0], b[e, 1])
    assert on[e, 0] and q[0][1] == f32(b[e, 1] + S.H) and a[e, 0, 1] > q[0][1]      # clipped to the end of side 1
    e = by["outside-the-box"]
    assert on[e, 0] and a[e, 0, 0] - b[e, 0] > S.H and r["fx"][e, 0] > 1.0 and nx[e, 0, 2] > free[e, 0, 2] + 1e-3
    assert out["next_body"][e, 2] < 0                                               # the box is pulled the other way
    e = by["deep-inside"]
    assert not out["contact"][e] and np.array_equal(_bits(nx[e]), _bits(free[e]))
    e = by["two-sides"]
    d, _ = S.side_distances(a[e, 0, 0], a[e, 0, 1], b[e, 0], b[e, 1])
    assert int(np.argmin(d)) == 0 and r["fx"][e, 0] < -1.0 and abs(r["fy"][e, 0]) < 1e-6
    assert kicked(e).all()                                                          # first side 1 (x), then side 3 (y)
    for name, sgn in (("plus", 1), ("minus", -1)):
        e = by["world-clamp/" + name]
        assert nx[e, 0, 0] == sgn * V.SEMIDIM and out["next_body"][e, 1] == sgn * V.SEMIDIM
        assert nx[e, 0, 2] == free[e, 0, 2] and abs(nx[e, 0, 2]) > 0.2 and abs(out["next_body"][e, 3]) > 0.1
        assert not out["contact"][e]

    # ---- cost margins, reward term, flag ----
    cost, m = out["cost"], r["margins"]
    if n > 1:
        for (name, d), sign in zip(S.three(V.TWO_AGENT_R), (1, 0, -1)):
            e = by["cost-margins/agent-" + name]
            assert (np.sign(m[e, :2, 0]) == sign).all()
            assert (cost[e, :2, 0] == -0.5).all() if sign == 0 else (np.sign(cost[e, :2, 0]) == sign).all()
            assert (np.abs(np.abs(cost[e, :2, 0]) - 0.5) < 1e-6).all()
        e = by["cost-margins/coincident"]
        assert (cost[e, :2, 0] == f32(f32(4) * V.TWO_AGENT_R) + f32(0.5)).all()
        assert (V.edge_feats(a[e:e + 1])[0][0, 0, 1, :2] == 0).all()               # and a zero edge between the two
    else:
        assert not any(t.startswith(S.PAIR_FAMILIES) for t in r["tags"])
    for (name, d), sign in zip(S.three(V.OBS_R), (1, 0, -1)):
        e = by["cost-margins/obstacle-" + name]
        assert (np.sign(m[e, :, 1]) == sign).all()
        assert (cost[e, :, 1] == -0.5).all() if sign == 0 else (np.sign(cost[e, :, 1]) == sign).all()
    e = by["cost-margins/obstacle-tie"]
    _, _, od, idx = V.obstacle_order(b[e:e + 1], r["scene"][e:e + 1])
    assert od[0, 0] == od[0, 2] < od[0, 1] and idx[0].tolist() == [0, 2, 1]
    assert (cost[by["cost-margins/on-obstacle"], :, 1] == f32(f32(2) * V.OBS_R) + f32(0.5)).all()
    assert (cost[by["cost-margins/far"], :, 1] == -1).all()
    assert (cost <= 0.8).all() or np.isnan(cost).any()                              # the upper clip is out of reach
    for (name, d), term in zip(S.three(V.DIST2GOAL), (0, 0, 1)):
        e = by["reward-threshold/" + name]
        assert out["reward"][e] == f32(f32(-d * f32(0.01)) - f32(term) * f32(0.001))
    flag = out["graph"]["nodes"][:, 0, 10]
    for name, want in (("x-at", 0), ("x-above", 1), ("x-neg-above", 1), ("y-at", 0), ("y-above", 1)):
        e = by["flag-threshold/" + name]
        assert flag[e] == want and np.array_equal(_bits(nx[e, 0]), _bits(a[e, 0])) and not out["contact"][e]
    rel = np.abs(nx[by["flag-threshold/x-at"], 0, 0] - out["next_body"][by["flag-threshold/x-at"], 0])
    assert rel == V.CONTACT_THR

    # ---- actions ----
    one = by["actions/one"]
    for name in ("beyond", "inf"):
        e = by["actions/" + name]
        for k in ("next_agent", "next_body", "cost"):
            assert np.array_equal(_bits(out[k][e]), _bits(out[k][one])), (name, k)
        assert np.isfinite(nx[e]).all()
    assert np.array_equal(_bits(nx[by["actions/zero"]]), _bits(nx[by["actions/negzero"]]))
    assert not np.array_equal(_bits(nx[by["actions/zero"]]), _bits(nx[one]))


@pytest.mark.parametrize("n", TEAMS)
def test_contact_scenes_stay_clear_of_the_force_thresholds_after_the_first_substep(n):
    """a condition on the inputs: after its first contact the device is a few ulps off the restatement (expf, log1pf), and the
    force is discontinuous at DIST_MIN and at MIN_DIST, so no later substep of a contact scene may come within 1e-5 of either"""
    r = _ref(n)
    for e in S.finite_ids(r["tags"]):
        if r["out"]["contact"][e]:
            assert r["near"][e].min() >= 1e-5, (r["tags"][e], r["near"][e])
    assert sum(bool(r["out"]["contact"][e]) for e in S.finite_ids(r["tags"])) >= 10


@pytest.mark.parametrize("n", TEAMS)
def test_nan_map_of_the_non_finite_scenes(n):
    """where the restatement (np.clip, np.min, a stable argsort: NaN kept, NaN kept, NaN last) puts NaN"""
    r = _ref(n)
    by, out = r["by"], r["out"]
    nf = n - 1
    others = [i for i in range(n) if i != nf]
    nodes = out["graph"]["nodes"]
    for name in ("action-nan", "position-nan", "velocity-nan", "position-inf"):
        e = by["non-finite/" + name]
        assert np.isnan(out["next_agent"][e, nf]).all() and np.isnan(out["next_body"][e]).all(), name
        assert np.isfinite(out["next_agent"][e, others]).all(), name       # a NaN box: dist = inf, no force
        assert np.isnan(nodes[e, :n, 4:10]).all() and np.isnan(nodes[e, :n, 11:20]).all(), name   # box and obstacle columns
    e = by["non-finite/position-nan"]
    assert np.isnan(out["cost"][e, :, 0]).all()
    assert np.isfinite(out["cost"][e, :, 1]).all()
    e = by["non-finite/box-nan"]
    assert np.isnan(out["reward"][e]) and np.isnan(out["cost"][e, :, 1]).all() and np.isfinite(out["cost"][e, :, 0]).all()
    assert np.isfinite(out["next_agent"][e]).all() and np.isnan(out["next_body"][e, 0])
    e = by["non-finite/obstacle-nan"]
    assert np.isnan(out["cost"][e, :, 1]).all() and np.isfinite(out["reward"][e])
    assert np.isnan(nodes[e, :n, 15]).all() and np.isnan(nodes[e, :n, 19]).all()    # the NaN obstacle sorts last
    assert np.isfinite(nodes[e, :n, 11:15]).all() and np.isfinite(nodes[e, :n, 17:19]).all()
    e = by["non-finite/goal-nan"]
    assert np.isnan(out["reward"][e]) and np.isnan(nodes[e, :n, 8]).all() and np.isfinite(out["cost"][e]).all()
    e = by["non-finite/velocity-inf"]
    assert out["next_agent"][e, nf, 0] == V.SEMIDIM and np.isposinf(out["next_agent"][e, nf, 2])
    assert np.isfinite(out["next_body"][e]).all()
    one, inf = by["actions/one"], by["actions/inf"]
    assert np.isfinite(out["next_agent"][inf]).all() and np.array_equal(_bits(out["next_agent"][inf]), _bits(out["next_agent"][one]))


def _force64(rx, ry):
    """float64 closed form for an agent INSIDE the axis-aligned hollow box, offset (rx, ry) from its centre: the nearest side
    is 0.3 - max(|rx|, |ry|) away, the force 500 * k * log(1 + exp((dist_min - dist) / k)) points back along that axis"""
    k, dmin = 6e-3, 0.03 + 4 / 6e2
    dist = 0.3 - max(abs(rx), abs(ry))
    mag = 500.0 * k * math.log1p(math.exp((dmin - dist) / k)) if 1e-6 <= dist <= dmin else 0.0
    if abs(rx) >= abs(ry):
        return -math.copysign(mag, rx), 0.0
    return 0.0, -math.copysign(mag, ry)


MEASURED_MARGIN = 8.84e-6          # see the docstring below


def test_contact_force_against_a_float64_closed_form():
    """The restatement's contact force (four segments, closest points, fp32) against the closed form above, written from the
    geometry and not from the code, at 4 sides x 60 depths x 9 places along the side.  Measured on this grid: the largest
    difference is 8.84e-6, at the deepest penetration (force 18.3, stiffness 500 per unit of distance): fp32(0.3) is 1.2e-8
    above 0.3, which alone moves the force by 6e-6, and the rest is the rounding of (dist_min - dist) / 0.006.  Twice the
    measured figure is allowed; the jump at the threshold is 2.08."""
    worst = 0.0
    depths = np.concatenate([np.linspace(2e-6, 1e-3, 10), np.linspace(1e-3, float(V.DIST_MIN) - 2e-6, 40),
                             np.linspace(float(V.DIST_MIN) + 2e-6, 0.06, 10)])
    for side in range(4):
        for dist in depths:
            for along in np.linspace(-0.2, 0.2, 9):
                near = (0.3 - dist) * (1 if side % 2 == 0 else -1)
                rx, ry = (f32(near), f32(along)) if side < 2 else (f32(along), f32(near))
                fx, fy, on = V.contact_force(np.array([rx]), np.array([ry]), np.zeros(1, f32), np.zeros(1, f32))
                wx, wy = _force64(float(rx), float(ry))
                assert bool(on[0]) == (wx != 0 or wy != 0), (side, dist, along)
                worst = max(worst, abs(float(fx[0]) - wx), abs(float(fy[0]) - wy))
    print(f"largest |fp32 restatement - float64 closed form| = {worst:.3e}")
    assert worst <= 2 * MEASURED_MARGIN, worst


def _seeds(n, count=32):
    return (np.arange(count, dtype=np.int64) + 1) * 104729 + n


@functools.lru_cache(maxsize=None)
def reset_stats(n, count=32):
    """(agent, body, scene, placed, restarts, draws) of each seed"""
    out = []
    for s in _seeds(n, count):
        st = {}
        a, b, sc, placed = V.reset_single(int(s), n, stats=st)
        out.append((a, b, sc, placed, st["restarts"], st["draws"]))
    return out


def test_reset_seeds_restart_near_jamming():
    """n = 14 and 15 in the 0.24 square: the 1024-iteration cut and the restart with a continuing counter are reached"""
    r14, r15 = reset_stats(14), reset_stats(15)
    assert all(o[3] for o in r14) and all(o[3] for o in r15)
    assert sum(o[4] > 0 for o in r14) >= 8
    assert sum(o[4] > 0 for o in r15) >= 16 and max(o[4] for o in r15) >= 10
    for o in r14 + r15:
        assert o[5] >= 3 + len(o[0]) + len(o[0]) + 1024 * o[4]                  # every restart follows 1025 rejected draws
    for n in (2, 5):
        assert all(o[3] and o[4] == 0 for o in reset_stats(n, 8))
