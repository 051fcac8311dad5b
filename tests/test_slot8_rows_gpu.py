"""The first-layer attention without its redundant operands (dgppo_attn_fwd_rows / dgppo_attn_bwd_rows, attn_slot8.hip): edge
features subtracted from the node rows the lane holds, and the backward's weights formed again from qt and emask.  Nothing is
recomputed differently, so every comparison is BIT FOR BIT against the general entry points (dgppo_attn_fwd / _bwd) on the
features dgppo_graph_feats writes for the same states; those entry points are held to float64 by test_nn_gpu.py and
test_attn_edges_gpu.py.

Shapes (each from a kind dgppo_attn_rows_supported accepts): LidarSpread 8 / 3 (S = 24: three full slot passes, the benchmark's
shape), LidarSpread 5 / 2 (S = 18: partial last slot pass, dead agent groups), LidarTarget 6 / 2 (own-goal slot, S = 15),
LidarSpread 16 / 3 (two agent passes, S = 40), MPESpread 4 / 3 (four-column obstacle slots, S = 11); G in {1, 5, 261}: one
wave, a workgroup with idle waves, and 66 workgroups of which the last holds one graph."""
import numpy as np
import pytest
import torch

from oracle import nn_torch as T

pytestmark = pytest.mark.gpu
F, H, KP = 8, 3, 48
GUARD = 64                       # floats behind an output that must keep their sentinel
SENT = -12345.5
CASES = [("LidarSpread", 8, 3), ("LidarSpread", 5, 2), ("LidarTarget", 6, 2), ("LidarSpread", 16, 3), ("MPESpread", 4, 3)]


def _cfg(name, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[name], n, n_obs)


def _states(cfg, G, seed, poison=True):
    """random records of G graphs (non-zero velocities on agents, goals and obstacles) with, in every graph: agent 1 a copy of
    agent 0 (tied logits at every receiver that sees both), one obstacle / hit row NaN and one at the 5e5 sentinel (their
    distance tests fail, so graph_feats masks them; poison=False leaves them out)"""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *shp: (torch.rand(*shp, generator=gen) * 1.4 - 0.7)
    n, k = cfg.n_agents, cfg.top_k
    agent, goal = u(G, n, 4), u(G, cfg.n_goals, 4)
    agent[:, 1] = agent[:, 0]
    hits = obst = None
    if cfg.is_lidar:
        hits = agent[:, :, None, :2] + 0.6 * u(G, n, k, 2)
        if poison:
            hits[:, 0, 2] = float("nan")
            hits[:, n - 1, 5] = 5e5
    else:
        obst = u(G, cfg.n_obs, 4)
        if poison:
            obst[:, 0] = float("nan")
            obst[:, 1] = 5e5
    return agent, goal, obst, hits


def _feats(cfg, G, st, dev):
    from dgppo_amd import nets
    agent, goal, obst, hits = (t.to(dev) if t is not None else None for t in st)
    n, k = cfg.n_agents, cfg.top_k
    f = nets.GraphFeats(cfg, G, nets.Arena(dev), "t")
    f.compute(agent, n * 4, 0, goal, obst, hits, n * k * 2, 0, None, G, 1)
    f._keep = (agent, goal, obst, hits)
    return f


def _guarded(rows, cols, dev):
    buf = torch.full((rows * cols + GUARD,), SENT, device=dev)
    return buf, buf[:rows * cols].view(rows, cols)


def _same_bits(a, b, what, nan_ok=False):
    """bit-equal; with nan_ok the NaN positions must agree and everything else is bit-equal"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if nan_ok:
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN positions differ"
        keep = ~torch.isnan(a)
        a, b = a[keep], b[keep]
    else:
        assert not torch.isnan(a).any() and not torch.isnan(b).any(), f"{what}: NaN reached the output"
    diff = a.view(torch.int32) != b.view(torch.int32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} words differ"


def _operands(cfg, G, seed, dev, live_nan):
    """features of _states through dgppo_graph_feats, queries and output gradients, and the edge rows: a receiver with every slot
    masked, one with exactly one live slot, one whose queries put the logits beyond +-100.  live_nan: one receiver has the slot of
    a NaN sender row forced live."""
    n, S = cfg.n_agents, cfg.fan_in
    R = G * n
    f = _feats(cfg, G, _states(cfg, G, seed), dev)
    gen = torch.Generator().manual_seed(seed + 1)
    qt = torch.randn(R, H * F, generator=gen)
    dz = torch.randn(R, KP, generator=gen)
    em = f.emask.clone()
    obs0 = n + cfg.goal_slots
    nan_slot = obs0 + 2 if cfg.is_lidar else obs0         # receiver 0's third hit / obstacle 0 at every receiver
    assert float(em.view(G, n, S)[:, 0, nan_slot].max()) == 0.0, "graph_feats must mask the NaN sender row"
    assert bool(torch.isnan(f.efeat.view(G, n, S, 4)[:, 0, nan_slot, :2]).all())
    rows = {"dead": (n - 1) % R, "single": (2 * n - 2) % R, "sharp": (3 * n - 3) % R}
    if R >= 3:
        assert len(set(rows.values())) == 3
    em[rows["dead"]] = 0.0
    em[rows["single"]] = 0.0
    em[rows["single"], n] = 1.0                           # its (first) goal slot
    if rows["sharp"] != rows["dead"] and rows["sharp"] != rows["single"]:
        qt[rows["sharp"]] *= 2000.0
        em[rows["sharp"], 1] = 0.0                        # (of the tied pair it sees one: its largest logit stands alone)
    em[0, 0] = em[0, 1] = 1.0                             # receiver 0 sees both agents of the tied pair, whatever the distances
    if live_nan:
        em.view(G, n, S)[0, 0, nan_slot] = 1.0
    return dict(f=f, qt=qt.to(dev), dz=dz.to(dev), em=em, rows=rows, R=R, S=S)


def _largest_logit(cfg, op, r):
    """largest |logit| over the live slots of receiver row r, in float64 from the operands"""
    n = cfg.n_agents
    f, g, i = op["f"], r // n, r % n
    snd = T.attn_sender_nodes(n, cfg.n_goals, cfg.goal_slots, cfg.obs_slots, cfg.is_lidar, cfg.is_spread)
    X = torch.cat([f.Xa.view(-1, n, F)[g], f.Xo.view(-1, f.n_other, F)[g]]).double().cpu()
    lg = op["qt"][r].double().cpu().view(H, F) @ X[torch.as_tensor(snd)[i]].t()            # [H, S]
    return float(lg[:, op["em"][r].cpu() != 0].abs().max())


def _run_both(cfg, G, op, dev):
    from dgppo_amd import ops_nn as K
    f, R, S = op["f"], op["R"], op["S"]
    Xo = f.Xo if f.n_other > 0 else None
    out = {}
    # the general entry points on the stored edge features, weights saved
    zb, z = _guarded(R, KP, dev)
    at = torch.full((R, S, H), SENT, device=dev)
    K.attn_fwd(cfg, F, H, KP, op["qt"], f.Xa, Xo, f.efeat, op["em"], z, at, G)
    db, dq = _guarded(R, H * F, dev)
    K.attn_bwd(cfg, F, H, KP, op["dz"], at, op["qt"], f.Xa, Xo, f.efeat, dq, None, None, G)
    out["old"] = (zb, z, at, db, dq)
    # edge features from the rows: inference form (no weights) and with the weights written
    zb2, z2 = _guarded(R, KP, dev)
    untouched = torch.full((R, S, H), SENT, device=dev)
    K.attn_fwd_rows(cfg, F, H, KP, op["qt"], f.Xa, Xo, op["em"], z2, None, G)
    zb3, z3 = _guarded(R, KP, dev)
    at3 = torch.full((R, S, H), SENT, device=dev)
    K.attn_fwd_rows(cfg, F, H, KP, op["qt"], f.Xa, Xo, op["em"], z3, at3, G)
    # backward: weights formed again, and saved weights with the edge features from the rows
    db2, dq2 = _guarded(R, H * F, dev)
    K.attn_bwd_rows(cfg, F, H, KP, op["dz"], None, op["qt"], op["em"], f.Xa, Xo, dq2, G)
    db3, dq3 = _guarded(R, H * F, dev)
    K.attn_bwd_rows(cfg, F, H, KP, op["dz"], at, None, None, f.Xa, Xo, dq3, G)
    torch.cuda.synchronize()
    assert bool((untouched == SENT).all())
    out["lean"] = (zb2, z2, None, db2, dq2)
    out["rows+attn"] = (zb3, z3, at3, db3, dq3)
    return out


@pytest.mark.parametrize("G", [1, 5, 261])
@pytest.mark.parametrize("name,n,n_obs", CASES)
def test_lean_modes_match_the_general_entry_points_bit_for_bit(cuda, name, n, n_obs, G):
    from dgppo_amd import ops_nn as K
    cfg = _cfg(name, n, n_obs)
    assert K.attn_rows_supported(cfg, F, H)
    op = _operands(cfg, G, seed=1000 * n + G, dev=cuda, live_nan=False)
    out = _run_both(cfg, G, op, cuda)
    zb, z, at, db, dq = out["old"]
    for mode in ("lean", "rows+attn"):
        zb_m, z_m, at_m, db_m, dq_m = out[mode]
        _same_bits(z_m, z, f"{mode} zcat")
        _same_bits(dq_m, dq, f"{mode} dqt")
        if at_m is not None:
            _same_bits(at_m, at, f"{mode} attn")
        assert bool((zb_m[-GUARD:] == SENT).all()), f"{mode}: guard words behind zcat were written"
        assert bool((db_m[-GUARD:] == SENT).all()), f"{mode}: guard words behind dqt were written"
    assert bool((zb[-GUARD:] == SENT).all()) and bool((db[-GUARD:] == SENT).all())
    # the edge rows did what they are there for (read off the general entry points' outputs)
    rows, S = op["rows"], op["S"]
    kc = F + H * (F + 4)
    assert float(at[rows["dead"]].abs().max()) == 0.0 and float(dq[rows["dead"]].abs().max()) == 0.0
    assert float(z[rows["dead"], F:kc].abs().max()) == 0.0
    if op["R"] >= 3:
        a1 = at[rows["single"]]
        assert bool((a1[n] == 1.0).all()) and float(a1.sum()) == float(H)
        assert _largest_logit(cfg, op, rows["sharp"]) >= 100.0, "queries x 2000 must put a live logit beyond +-100"
        assert float(at[rows["sharp"]].max(0).values.max()) >= 1.0 - 1e-6, "... and make a head's row one-hot"
    live01 = (op["em"][:, 0] != 0) & (op["em"][:, 1] != 0)
    assert bool(live01.any()), "no receiver sees the two tied agents"
    _same_bits(at[live01][:, 0], at[live01][:, 1], "weights of the tied pair")
    assert float(at[live01][:, 0].max()) > 1e-3


@pytest.mark.parametrize("name,n,n_obs", CASES)
def test_a_live_nan_row_poisons_the_same_outputs_in_both_modes(cuda, name, n, n_obs):
    cfg = _cfg(name, n, n_obs)
    G = 5
    op = _operands(cfg, G, seed=77 + n, dev=cuda, live_nan=True)
    out = _run_both(cfg, G, op, cuda)
    zb, z, at, db, dq = out["old"]
    assert bool(torch.isnan(z[0]).any()) and bool(torch.isnan(dq[0]).any()), "the live NaN row must reach receiver 0"
    assert not bool(torch.isnan(z[1:]).any()) and not bool(torch.isnan(dq[1:]).any()), "... and nobody else"
    for mode in ("lean", "rows+attn"):
        zb_m, z_m, at_m, db_m, dq_m = out[mode]
        _same_bits(z_m, z, f"{mode} zcat", nan_ok=True)
        _same_bits(dq_m, dq, f"{mode} dqt", nan_ok=True)
        if at_m is not None:
            _same_bits(at_m, at, f"{mode} attn", nan_ok=True)


def test_other_shapes_and_kinds_are_refused_and_nothing_is_written(cuda):
    from dgppo_amd import ops_nn as K
    G = 3

    def refused(cfg, Fx, Kp):
        n, S = cfg.n_agents, cfg.fan_in
        R, n_other = G * n, cfg.num_nodes - 1 - n
        assert not K.attn_rows_supported(cfg, Fx, H)
        ins = lambda *shp: torch.randn(*shp, device=cuda)
        qt, Xa, Xo, em, dz = ins(R, H * Fx), ins(R, Fx), ins(G * n_other, Fx), torch.ones(R, S, device=cuda), ins(R, Kp)
        z, at, dq = (torch.full(shp, SENT, device=cuda) for shp in ((R, Kp), (R, S, H), (R, H * Fx)))
        with pytest.raises(ValueError, match="dgppo_attn_rows_supported"):
            K.attn_fwd_rows(cfg, Fx, H, Kp, qt, Xa, Xo, em, z, at, G)
        with pytest.raises(ValueError, match="dgppo_attn_rows_supported"):
            K.attn_bwd_rows(cfg, Fx, H, Kp, dz, None, qt, em, Xa, Xo, dq, G)
        with pytest.raises(ValueError, match="dgppo_attn_rows_supported"):
            K.attn_bwd_rows(cfg, Fx, H, Kp, dz, torch.rand(R, S, H, device=cuda), None, None, Xa, Xo, dq, G)
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in (z, at, dq))

    refused(_cfg("LidarSpread", 8, 3), 32, 144)              # second-layer width: the block-diagonal family
    refused(_cfg("LidarBicycleTarget", 4, 2), 8, KP)         # slot-sparse shape, but a 5-float state
    # a zcat width that is no multiple of 4 takes the workgroup kernels: refused as well
    cfg = _cfg("LidarSpread", 8, 3)
    R, S = G * 8, cfg.fan_in
    z = torch.full((R, 46), SENT, device=cuda)
    with pytest.raises(ValueError, match="dgppo_attn_rows_supported"):
        K.attn_fwd_rows(cfg, F, H, 46, torch.randn(R, H * F, device=cuda), torch.randn(R, F, device=cuda),
                        torch.randn(G * (cfg.num_nodes - 1 - 8), F, device=cuda), torch.ones(R, S, device=cuda), z, None, G)
    torch.cuda.synchronize()
    assert bool((z == SENT).all())


# ---- Net level: the constructor switch ---------------------------------------------------------------------------------------
def _net_pair(kindname, cfg, layers, n_out, tree, dev):
    from dgppo_amd import nets
    pair = []
    for lean in (True, False):
        net = nets.Net(kindname, cfg, layers, n_out, dev, lean_attn0=lean)
        net.load_tree(tree)
        pair.append(net)
    assert pair[0].lean_attn0 and not pair[1].lean_attn0
    return pair


@pytest.mark.parametrize("name,n,n_obs", [("LidarSpread", 8, 3), ("LidarSpread", 4, 2)])
@pytest.mark.parametrize("net_kind", ["policy", "Vl", "Vh"])
def test_net_switch_changes_no_bit_of_zcat0_and_dqt0(cuda, net_kind, name, n, n_obs):
    """policy, Vl and Vh at 16 graphs with the lean first layer on and off: no attn0 in the arena with it on, zcat0 and dqt0
    bit-equal, every gradient leaf within the 3e-5 of the largest gradient that the Net tests of test_nn_gpu.py allow against the
    oracle (the leaves differ only through the atomics of the weight-gradient reduce)."""
    cfg = _cfg(name, n, n_obs)
    n_env, T_ = 4, 4
    G = n_env * T_
    gen = torch.Generator().manual_seed(11)
    layers, n_out, tree = {"policy": (2, 2, T.init_policy(1, cfg.node_dim)), "Vl": (2, 1, T.init_value(2, cfg.node_dim, 1, 2)),
                           "Vh": (1, 2, T.init_value(3, cfg.node_dim, 2, 1))}[net_kind]
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), tree)
    on, off = _net_pair(net_kind, cfg, layers, n_out, tree, cuda)
    feats = _feats(cfg, G, _states(cfg, G, seed=5, poison=False), cuda)
    assert feats.edges_from_rows
    R = G * n
    if net_kind == "policy":
        kw, dout = dict(n_seq=n_env * n, T=T_, h0=None), torch.randn(R, 4, generator=gen)
    elif net_kind == "Vl":
        kw, dout = dict(n_seq=n_env, T=T_, h0=None), torch.randn(G, 1, generator=gen)
    else:
        kw = dict(n_seq=R, T=1, h0=(0.5 * torch.randn(R, 64, generator=gen)).to(cuda))
        dout = torch.randn(R, 2, generator=gen)
    dout = dout.to(cuda)
    got = {}
    for key, net in (("on", on), ("off", off)):
        act = net.forward(feats, **kw)
        net.zero_grads()
        net.backward(act, dout)
        torch.cuda.synchronize()
        got[key] = (act["zcat0"].clone(), net.arena.bufs["b.dqt0"][:R * H * F].clone(), net.grads.clone(), act)
    assert "f.attn0" not in on.arena.bufs and got["on"][3]["attn0"] is None
    assert "f.attn0" in off.arena.bufs and got["off"][3]["attn0"] is not None
    _same_bits(got["on"][0], got["off"][0], "zcat0")
    _same_bits(got["on"][1], got["off"][1], "dqt0")
    g_on, g_off = on.to_tree(got["on"][2]), off.to_tree(got["off"][2])
    leaves_on = dict(T.tree_leaves(T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), g_on)))
    leaves_off = dict(T.tree_leaves(T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), g_off)))
    gscale = max(float(v.abs().max()) for v in leaves_off.values())
    assert gscale > 0.0
    for k, v in leaves_off.items():
        err = float((leaves_on[k].double() - v.double()).abs().max())
        assert err <= 3e-5 * max(gscale, 1e-3), f"{k}: {err:.3e} (scale {gscale:.3e})"
