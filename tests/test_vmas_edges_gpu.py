"""The dgppo_vmas_* kernels on the hand-built states of tests/vmas_edge_scenes.py against the restatement (tests/vmas_np.py):
the contact force at its thresholds, ties, the world clamp, the cost / reward / flag thresholds and non-finite inputs, at every
lane layout of the step kernel (n = 1 .. 16, with and without dead lanes), in batches that leave the last wave and the last
workgroup partly empty, through dgppo_vmas_graph_materialize and dgppo_vmas_graph_feats, and the reset near jamming (n = 14,
15).  tests/test_vmas_edges_cpu.py shows on the restatement that every scene takes the branch its tag names and that no
contact scene comes near a force threshold after its first substep.  Every output is allocated with a guard row each side."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vmas_edge_scenes as S  # noqa: E402
import vmas_np as V  # noqa: E402
from test_vmas_gpu import _cfg, _check_step, _close, _dev  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable"),
              pytest.mark.filterwarnings("ignore:invalid value encountered")]      # the restatement computing with NaN
f32 = np.float32
SENT = -777.0
OUT = ("next_agent", "next_body", "reward", "cost")
INT_KEYS, FLOAT_KEYS = ("receivers", "senders", "node_type", "n_node", "n_edge"), ("nodes", "edges")
FORCE_OFF = ("contact-threshold/above", "on-the-side/centre", "on-the-side/min-dist-below")
FORCE_ON = {"contact-threshold/below": 0, "contact-threshold/at": 0, "on-the-side/min-dist-at": 0,
            "on-the-side/min-dist-above": 0, "corner-tie/inside": 0, "abeam-centre": 1}      # tag: the velocity column kicked
NAN_BOX = ("action-nan", "position-nan", "velocity-nan", "position-inf", "box-nan")           # every other agent flies free


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same_bits(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}"


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


def _sub(d, ids):
    return {k: (_sub(v, ids) if isinstance(v, dict) else v[ids]) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _ref(n):
    """the catalogue of one team size and the restatement's answers for it, computed once and shared read-only"""
    s = S.scenes(n)
    want = V.env_step(s["agent"], s["body"], s["scene"], s["action"])
    return _freeze(dict(s, want=want, free=S.free_flight(s["agent"], s["action"]), by={t: i for i, t in enumerate(s["tags"])}))


def _guarded(like):
    """tensors like `like` [B, ...] with one more row each side, filled with a sentinel, and the views of the B rows between"""
    full = {k: torch.full((v.shape[0] + 2,) + tuple(v.shape[1:]), SENT if v.is_floating_point() else int(SENT), dtype=v.dtype,
                          device=v.device) for k, v in like.items()}
    return full, {k: v[1:-1] for k, v in full.items()}


def _guards_untouched(full, name):
    for k, v in full.items():
        assert bool((v[0] == SENT).all()) and bool((v[-1] == SENT).all()), f"{name}: {k} written outside its rows"


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _run_step(cfg, agent, body, scene, action, dev):
    from dgppo_amd import ops_env as OE
    B, n = agent.shape[:2]
    ad, bd, sd, ud = (_dev(x, dev) for x in (agent, body, scene, action))
    e = lambda *s: torch.empty(*s, device=dev)
    full, out = _guarded(dict(next_agent=e(B, n, 4), next_body=e(B, 4), reward=e(B), cost=e(B, n, 2)))
    gfull, g = _guarded(OE.alloc_graph(cfg, B, dev))
    OE.vmas_step(cfg, ad, bd, sd, ud, out["next_agent"], out["next_body"], out["reward"], out["cost"], g)
    torch.cuda.synchronize()
    _guards_untouched(full, "step")
    _guards_untouched(gfull, "step graph")
    return dict(_np(out), graph=_np(g))


def _materialize(cfg, agent, body, scene, dev):
    from dgppo_amd import ops_env as OE
    gfull, g = _guarded(OE.alloc_graph(cfg, agent.shape[0], dev))
    OE.vmas_graph_materialize(cfg, _dev(agent, dev), _dev(body, dev), _dev(scene, dev), g)
    torch.cuda.synchronize()
    _guards_untouched(gfull, "materialise")
    return _np(g)


def _feats(cfg, agent, agent_se, agent_st, body, body_se, body_st, scene, env_ids, n_env, n_time, Fp, dev):
    from dgppo_amd import ops_nn as K
    n, G = cfg.n_agents, n_env * n_time
    e = lambda *s: torch.empty(*s, device=dev)
    full, o = _guarded(dict(Xa=e(G, n, Fp), efeat=e(G, n, n, 4), emask=e(G, n, n)))
    K.vmas_graph_feats(cfg, agent, agent_se, agent_st, body, body_se, body_st, scene, env_ids, n_env, n_time,
                       o["Xa"].view(G * n, Fp), o["efeat"].view(G * n, n, 4), o["emask"].view(G * n, n), Fp)
    torch.cuda.synchronize()
    _guards_untouched(full, "feats")
    return _np(o)


def _check_feats(got, agent, body, scene, name):
    """Xa[:, :20], efeat, emask against the restatement's node and edge features of the same arrays, NaN where it has NaN and
    equal bits elsewhere; the padding columns +0.0"""
    n = agent.shape[1]
    Xw = V.node_feats(agent, body, scene)
    ew, mw = V.edge_feats(agent)
    for key, g, w in (("Xa", got["Xa"][..., :20], Xw), ("efeat", got["efeat"], ew)):
        nan = np.isnan(w)
        np.testing.assert_array_equal(np.isnan(g), nan, err_msg=f"{name} {key}: NaN positions")
        _same_bits(np.where(nan, f32(0), g), np.where(nan, f32(0), w), f"{name} {key}")
    assert not _bits(got["Xa"][..., 20:]).any(), f"{name}: padding columns"
    _same_bits(got["emask"], np.broadcast_to(mw.astype(f32), got["emask"].shape), f"{name} emask")
    assert n == got["emask"].shape[-1]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 15, 16])
def test_edge_scenes_match_restatement(cuda, n):
    """every lane layout (P = 1, 2, 4, 8, 16; dead lanes at n = 3, 5, 9, 15): the finite scenes by the rule of _check_step, and
    the cases decided at substep 0 from exact inputs by their outcome itself"""
    r = _ref(n)
    got = _run_step(_cfg(n), r["agent"], r["body"], r["scene"], r["action"], cuda)
    fin = S.finite_ids(r["tags"])
    want, by, free, nx = r["want"], r["by"], r["free"], got["next_agent"]
    assert want["contact"][fin].sum() >= 10 and (~want["contact"][fin]).sum() >= 20
    _check_step(_sub(got, fin), _sub(want, fin), f"n={n}")
    for tag in FORCE_OFF:
        _same_bits(nx[by[tag], 0], free[by[tag], 0], f"n={n} {tag}: the force is off, free flight")
    for tag, col in FORCE_ON.items():
        e = by[tag]
        assert abs(float(nx[e, 0, 2 + col]) - float(free[e, 0, 2 + col])) > 1e-3, f"n={n} {tag}: the force is on"
    for e in S.env_ids(r["tags"], "flag-threshold"):
        _same_bits(got["graph"]["nodes"][e, :n, 10], want["graph"]["nodes"][e, :n, 10], f"n={n} {r['tags'][e]}: flag")
        _same_bits(nx[e, 0], r["agent"][e, 0], f"n={n} {r['tags'][e]}: the agent stays")
    for k in OUT + ("nodes", "edges"):                                   # +-inf clips to +-1
        g = got["graph"] if k in FLOAT_KEYS else got
        for name in ("beyond", "inf"):
            _same_bits(g[k][by["actions/" + name]], g[k][by["actions/one"]], f"n={n} actions/{name} vs actions/one: {k}")


@pytest.mark.parametrize("B", [1, 37, 261])
@pytest.mark.parametrize("n", [2, 5, 16])
def test_ragged_batches_and_lane_independence(cuda, n, B):
    """the finite scenes tiled to batches that are no multiple of the envs of a wave (64 / P) or of a workgroup: every copy
    of a scene gives the bits of its first copy, the restatement's rule holds, and nothing is written outside the B rows"""
    r = _ref(n)
    fin = np.array(S.finite_ids(r["tags"]))
    first = np.arange(B) % len(fin)
    idx = fin[first]
    got = _run_step(_cfg(n), r["agent"][idx], r["body"][idx], r["scene"][idx], r["action"][idx], cuda)
    _check_step(got, _sub(r["want"], idx), f"n={n} B={B}")
    for k in OUT:
        _same_bits(got[k], got[k][first], f"n={n} B={B} {k}: copies differ")
    for k in INT_KEYS + FLOAT_KEYS:
        _same_bits(got["graph"][k], got["graph"][k][first], f"n={n} B={B} graph {k}: copies differ")


@pytest.mark.parametrize("n", [2, 16])
def test_materialize_and_feats_of_the_post_step_state(cuda, n):
    """dgppo_vmas_graph_materialize and dgppo_vmas_graph_feats of the step's own outputs: the graph the step wrote and the
    restatement's graph of the same arrays, bit for bit (no transcendental is involved)"""
    r = _ref(n)
    cfg = _cfg(n)
    fin = S.finite_ids(r["tags"])
    a, b, sc, u = (np.ascontiguousarray(r[k][fin]) for k in ("agent", "body", "scene", "action"))
    Bf = len(fin)
    got = _run_step(cfg, a, b, sc, u, cuda)
    nx, nb = got["next_agent"], got["next_body"]
    mat = _materialize(cfg, nx, nb, sc, cuda)
    wg = V.get_graph(nx, nb, sc)
    for k in INT_KEYS + FLOAT_KEYS:
        _same_bits(mat[k], got["graph"][k], f"n={n} materialise vs step: {k}")
        _same_bits(mat[k], wg[k], f"n={n} materialise vs restatement: {k}")
    # a record of three time slots (pre, post, pre) read from its second slot, and the dense post-step state
    T1 = 3
    rec_a, rec_b = np.stack([a, nx, a], 1), np.stack([b, nb, b], 1)
    rad, rbd, nxd, nbd, scd = (_dev(x, cuda) for x in (rec_a, rec_b, nx, nb, sc))
    ids = np.array(list(range(Bf))[::-2] + [0, 0], np.int32)
    sel = lambda x, e: x[e][:, 1:3].reshape((-1,) + x.shape[2:])
    everyone = np.arange(Bf)
    for Fp in (20, 24, 32):
        f = _feats(cfg, nxd, n * 4, 0, nbd, 4, 0, scd, None, Bf, 1, Fp, cuda)
        _check_feats(f, nx, nb, sc, f"n={n} Fp={Fp} dense")
        f = _feats(cfg, nxd, n * 4, 0, nbd, 4, 0, scd, None, Bf, 2, Fp, cuda)               # time stride 0: each state twice
        _check_feats(f, np.repeat(nx, 2, 0), np.repeat(nb, 2, 0), np.repeat(sc, 2, 0), f"n={n} Fp={Fp} time stride 0")
        f = _feats(cfg, rad[:, 1], T1 * n * 4, n * 4, rbd[:, 1], T1 * 4, 4, scd, None, Bf, 2, Fp, cuda)
        _check_feats(f, sel(rec_a, everyone), sel(rec_b, everyone), np.repeat(sc, 2, 0), f"n={n} Fp={Fp} strided record")
        f = _feats(cfg, rad[:, 1], T1 * n * 4, n * 4, rbd[:, 1], T1 * 4, 4, scd, _dev(ids, cuda), len(ids), 2, Fp, cuda)
        _check_feats(f, sel(rec_a, ids), sel(rec_b, ids), np.repeat(sc[ids], 2, 0), f"n={n} Fp={Fp} strided record, env ids")


def _nan_positions(got, want, tags, name, problems):
    """NaN exactly where the restatement has NaN, the other non-finite values equal; mismatches are collected per scene"""
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        bad = (gn != wn).reshape(len(tags), -1)
        for e in np.nonzero(bad.any(1))[0]:
            problems.append(f"{name}: {tags[e]}: NaN positions differ in {int(bad[e].sum())} of {bad.shape[1]} words "
                            f"(device {int(gn.reshape(len(tags), -1)[e].sum())} NaN, restatement "
                            f"{int(wn.reshape(len(tags), -1)[e].sum())})")
    inf = np.isinf(want)
    if not np.array_equal(np.where(inf, got, f32(0)), np.where(inf, want, f32(0))):
        problems.append(f"{name}: infinite values differ")
    finite = np.isfinite(want) & np.isfinite(got)
    return np.where(finite, got, f32(0)), np.where(finite, want, f32(0))


@pytest.mark.parametrize("n", [3, 5, 16])
def test_non_finite_inputs_follow_the_restatement(cuda, n):
    """NaN through every clip (jnp.clip keeps it), through both cost minima (jnp.min keeps it) and sorted last among the
    obstacle distances (jnp.argsort): NaN in the step outputs, the graph and the feature rows exactly where the restatement
    has it, the finite rest by the rule of _check_step, and the finite envs untouched by the NaN envs of their wave"""
    r = _ref(n)
    cfg = _cfg(n)
    tags, by, want = r["tags"], r["by"], r["want"]
    B = len(tags)
    nf = n - 1
    others = [i for i in range(n) if i != nf]
    got = _run_step(cfg, r["agent"], r["body"], r["scene"], r["action"], cuda)
    assert np.isnan(want["next_agent"]).any() and np.isnan(want["cost"]).any() and np.isnan(want["reward"]).any()
    assert np.isnan(want["graph"]["nodes"][..., 11:]).any()
    problems, g0, w0 = [], dict(graph={}), dict(graph={}, contact=want["contact"])
    for k in OUT:
        g0[k], w0[k] = _nan_positions(got[k], want[k], tags, k, problems)
    for k in FLOAT_KEYS:
        g0["graph"][k], w0["graph"][k] = _nan_positions(got["graph"][k], want["graph"][k], tags, "graph " + k, problems)
    for k in INT_KEYS:
        g0["graph"][k], w0["graph"][k] = got["graph"][k], want["graph"][k]
    # the features and the graph of the restatement's own post-step state, NaN box and all
    wnx, wnb, sc = want["next_agent"], want["next_body"], r["scene"]
    f = _feats(cfg, _dev(wnx, cuda), n * 4, 0, _dev(wnb, cuda), 4, 0, _dev(sc, cuda), None, B, 1, 20, cuda)
    Xw = V.node_feats(wnx, wnb, sc)
    _nan_positions(f["Xa"], Xw, tags, "Xa of the restatement's state", problems)
    mat = _materialize(cfg, wnx, wnb, sc, cuda)
    _nan_positions(mat["nodes"], want["graph"]["nodes"], tags, "materialised nodes of the restatement's state", problems)
    assert not problems, "\n".join(problems)
    _check_feats(f, wnx, wnb, sc, f"n={n} non-finite")
    for k in FLOAT_KEYS:
        nan = np.isnan(want["graph"][k])
        _same_bits(np.where(nan, f32(0), mat[k]), np.where(nan, f32(0), want["graph"][k]), f"n={n} materialise {k}")
    _check_step(g0, w0, f"n={n} with the non-finite scenes")
    for name in NAN_BOX:                                                 # a NaN box: dist = inf, no force on anybody else
        e = by["non-finite/" + name]
        _same_bits(got["next_agent"][e, others], want["next_agent"][e, others], f"n={n} {name}: the other agents")
    for k in OUT:
        _same_bits(got[k][by["actions/inf"]], got[k][by["actions/one"]], f"n={n} +-inf against +-1: {k}")
    # isolation: the same batch with every non-finite env replaced by a finite one
    fin = S.finite_ids(tags)
    sick = [e for e in range(B) if e not in fin]
    a2, b2, s2, u2 = (r[k].copy() for k in ("agent", "body", "scene", "action"))
    for x in (a2, b2, s2, u2):
        x[sick] = x[by["deep-inside"]]
    clean = _run_step(cfg, a2, b2, s2, u2, cuda)
    for k in OUT:
        _same_bits(got[k][fin], clean[k][fin], f"n={n} {k}: a finite env depends on the NaN envs of its wave")
    for k in INT_KEYS + FLOAT_KEYS:
        _same_bits(got["graph"][k][fin], clean["graph"][k][fin], f"n={n} graph {k}: a finite env depends on the NaN envs")


RESET_B = 33


@functools.lru_cache(maxsize=None)
def _reset_ref(n):
    seeds = (np.arange(RESET_B, dtype=np.int64) + 1) * 104729 + n
    out = []
    for s in seeds:
        st = {}
        out.append(V.reset_single(int(s), n, stats=st) + (st["pos"], st["restarts"]))
    stack = lambda k: np.stack([o[k] for o in out])
    return seeds, stack(0), stack(1), stack(2), [o[3] for o in out], stack(4), [o[5] for o in out]


@pytest.mark.parametrize("n", [2, 5, 14, 15])
def test_reset_near_jamming(cuda, n):
    """n = 14 and 15 restart (test_vmas_edges_cpu.py counts them): the 1024-iteration cut and the restart that goes on with
    the same counter.  The uniform draws are bit-exact: the velocities, and the placement, which is read off as the device's
    positions being the restatement's placement shifted onto the device's own box position, bit for bit."""
    from dgppo_amd import ops_env as OE
    B = RESET_B
    seeds, wa, wb, ws, placed, pos, restarts = _reset_ref(n)
    assert all(placed) and (n < 14 or sum(k > 0 for k in restarts) >= 8)
    e = lambda *s: torch.full(s, SENT, device=cuda)
    agent, body, scene = e(B + 1, n, 4), e(B + 1, 4), e(B + 1, 8)
    failed = torch.zeros(1, dtype=torch.int32, device=cuda)
    OE.vmas_reset(_cfg(n), _dev(seeds, cuda), agent[:B], body[:B], scene[:B], failed)
    torch.cuda.synchronize()
    for k, v in (("agent", agent), ("body", body), ("scene", scene)):
        assert bool((v[B] == SENT).all()), f"{k}: the row after the last env was written"
    a, b, s = agent[:B].cpu().numpy(), body[:B].cpu().numpy(), scene[:B].cpu().numpy()
    assert int(failed.item()) == 0
    _same_bits(a[..., 2:], wa[..., 2:], "velocities")
    shifted = ((pos - V.SHIFT).astype(f32) + b[:, None, :2]).astype(f32)
    _same_bits(a[..., :2], shifted, "placement, shifted onto the device's box position")
    _close(a[..., :2], wa[..., :2], 1e-6, "agent positions", 1.0)
    _close(b, wb, 1e-6, "body", 1.0)
    _close(s, ws, 1e-6, "scene", 1.0)
    d = np.linalg.norm(a[:, :, None, :2].astype(np.float64) - a[:, None, :, :2], axis=-1) + np.eye(n) * 9
    assert (d > 0.06).all(), d.min()
