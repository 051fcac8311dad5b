"""The value nets' one-step tail in two launches (dgppo_mlp_gi_fwd with gi == NULL, dgppo_gi_gru1_head_fwd) against the three it
replaces (dgppo_mlp_gi_fwd with gi, dgppo_gru_fwd / _h0_blocks / _h0_map at T = 1, dgppo_dense_fwd) on the same inputs, and both
against a float64 restatement written here.

What is asserted, and where the bounds come from:
  * y2 of the gi == NULL call, hs and gates: bit-equal to the present launches.  The new step kernel sums gi and gh in the k
    orders of the kernels it replaces and shares their gate function (nn_gru.h: gru_gate_fwd), so no tolerance is needed.
  * out: the head sums its 64 products in another order than dgppo_dense_fwd.  Per row count, |new - present| is held to the
    forward error bound of two fp32 dot products of 64 terms, 2 * 64 * 2^-24 * (|h'| |W| + |b|) (Higham, Accuracy and
    Stability, (3.5), gamma_64 ~ 64 u; each path is within one such bound of the exact sum).  Over all row counts of a
    (h0 form, n_out) combination, the largest error against float64 is held to 2 x the present path's largest error on the same
    inputs, and so is the largest error of every single row count from 191 rows on.  Below that the rule is applied to the
    sweep's maxima only: the largest of N rounding errors is an estimate of a path's error once N is large (N >= 191 here: the
    maxima of two samples of that size from one distribution differ by a few tens of per cent), while the one or two numbers
    of M = 1 estimate neither path's error and their ratio can be anything.  The float64 restatement starts from the fp32 y2 and h' both paths share, so the errors are those of the
    step and of the head alone.
  * hs, gates against float64: the same 2 x rule (trivially met while they are bit-equal; it stays asserted).
Row counts: 1, 15, 16, 17, 31, 33, 191, 193, 16 352, 16 353 (the two sides of dgppo_gru_fwd's tile-size threshold) and
16 (12 CUs + 3) + 5 (some waves walk two tiles, the last tile is ragged).
Every row operand is the head of a buffer with 16 more rows: NaN in inputs, a sentinel in outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
H = 64
SENT = 12345.0
U = 2.0 ** -24


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _row_counts(dev):
    # (16 352 / 16 353: where dgppo_gru_fwd goes from 16- to 32-sequence tiles, whose h' is rounded the other way round)
    return [1, 15, 16, 17, 31, 33, 191, 193, 16352, 16353, 16 * (12 * _cus(dev) + 3) + 5]


def _params(dev, n_out, seed=3):
    g = torch.Generator().manual_seed(seed + n_out)
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g)).to(dev)
    trunk = [r(H, H, k=0.2), r(H, k=0.1), 1.0 + r(H, k=0.1), r(H, k=0.1), r(H, H, k=0.2), r(H, k=0.1), 1.0 + r(H, k=0.1), r(H, k=0.1)]
    return dict(trunk=trunk, Wi=r(H, 192, k=0.2), bi=r(192, k=0.1), Wh=r(H, 192, k=0.2), bhn=r(H, k=0.1), Wo=r(H, n_out, k=0.3),
                bo=r(n_out, k=0.1))


def _padded(dev, M, w, gen=None, fill=float("nan")):
    """[M + 16, w] buffer and its [M, w] head: random head when gen is given, `fill` everywhere else"""
    buf = torch.full((M + 16, w), fill, device=dev)
    if gen is not None:
        buf[:M] = torch.randn(M, w, generator=gen).to(dev)
    return buf, buf[:M]


def _h0_forms(K, dev, form, M, seed):
    """-> (h0 operand of the new call, the dense [M, 64] copy, how the present path reads it: (name, operand, n_inner))"""
    g = torch.Generator().manual_seed(100 + seed)
    if form == "zero":
        return None, None, ("dense", None, 1)
    if form == "dense":
        buf, h0 = _padded(dev, M, H, g)
        h0.mul_(0.5)
        return h0, h0, ("dense", h0, 1)
    if form == "blocks":                       # blocks of 5 rows, 2 NaN rows between them
        rpb, nb = 5, (M + 4) // 5
        rec = torch.full((nb + 1, rpb + 2, H), float("nan"), device=dev)
        rec[:nb, :rpb] = (0.5 * torch.randn(nb, rpb, H, generator=g)).to(dev)
        blocks = K.H0Blocks(rec, rpb, (rpb + 2) * H, nb)
        dense = rec[:nb, :rpb].reshape(-1, H)[:M].contiguous()
        return blocks, dense, ("blocks", blocks, 1)
    # mapped: time-major record [4 slots, n_src envs, n_inner, 64], slot 0 NaN, 3 usable slots (tests/test_gru_h0_map_gpu.py)
    n_inner = 8 if form.endswith("8") else 1
    with_ids = form.startswith("map-ids")
    n_time = 3
    n_env = (M + n_time * n_inner - 1) // (n_time * n_inner)
    n_src = n_env + 2
    rec = (0.5 * torch.randn(4, n_src, n_inner, H, generator=g))
    rec[0] = float("nan")
    rec = rec.to(dev)
    view = rec[1:].transpose(0, 1)              # [env, time, n, 64]
    ids = None
    if with_ids:                                # out of order, with a repeat where there is room for one
        ids = torch.randint(0, n_src, (n_env,), generator=g)
        if n_env > 1:
            ids[1] = ids[0]
        ids = ids.to(torch.int32).to(dev)
    m = K.H0Map(view, view.stride(0), view.stride(1), n_time, n_inner, n_env, ids=ids, n_env_src=n_src)
    dense = m.dense()[:M].contiguous()
    assert not torch.isnan(dense).any()
    return m, dense, ("map", m, n_inner)


def _present(K, X, P, present_h0, dense_h0, M, n_out, dev):
    """the three launches of the present path -> y2, hs, gates, out"""
    sv = [torch.empty(M, w, device=dev) for w in (H, H, 2, H, H, 2)]
    gi = torch.empty(M, 192, device=dev)
    K.mlp_gi_fwd(X, *P["trunk"], P["Wi"], P["bi"], gi, tuple(sv))
    hs, gates = torch.empty(M, H, device=dev), torch.empty(M, 256, device=dev)
    kind, op, n_inner = present_h0
    if kind == "blocks":
        K.gru_fwd_h0_blocks(gi, P["Wh"], P["bhn"], op, hs, None, gates, M, 1, 1)
    elif kind == "map" and M % n_inner == 0:
        K.gru_fwd_h0_map(gi, P["Wh"], P["bhn"], op, hs, None, gates, M, 1, n_inner)
    else:                                       # (the library takes whole graphs only: the gathered copy, same kernel)
        K.gru_fwd(gi, P["Wh"], P["bhn"], dense_h0, hs, None, gates, M, 1, 1)
    out = torch.empty(M, n_out, device=dev)
    K.dense_fwd(hs, P["Wo"], P["bo"], out)
    return sv, gi, hs, gates, out


def _f64(P, y2, h0, hs):
    """float64 restatement of the step from the fp32 y2 (flax GRUCell, r | z | n) and of the head from the fp32 h'"""
    d = lambda t: t.double()
    gi = d(y2) @ d(P["Wi"]) + d(P["bi"])
    h = d(h0) if h0 is not None else torch.zeros_like(d(y2))
    gh = h @ d(P["Wh"])
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:] + d(P["bhn"])
    n = torch.tanh(gi[:, 2 * H:] + r * hn)
    hnew = (1.0 - z) * n + z * h
    out = d(hs) @ d(P["Wo"]) + d(P["bo"])
    bound = 2 * 64 * U * (d(hs).abs() @ d(P["Wo"]).abs() + d(P["bo"]).abs())
    return hnew, torch.cat([r, z, n, hn], 1), out, bound


def _bits(a, b, what):
    assert not torch.isnan(b).any(), f"{what}: the present path holds NaN"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what} differs from the present path"


def _err(a, want):
    return float((a.double() - want).abs().max())


FORMS = [("dense", 1), ("dense", 2), ("dense", 3), ("dense", 16), ("zero", 2), ("blocks", 2), ("map-1", 2), ("map-8", 2),
         ("map-ids-1", 2), ("map-ids-8", 3)]


@pytest.mark.parametrize("form,n_out", FORMS, ids=[f"{f}-nout{n}" for f, n in FORMS])
def test_pair_equals_the_three_launches(cuda, form, n_out):
    from dgppo_amd import ops_nn as K
    P = _params(cuda, n_out)
    worst = {k: [0.0, 0.0] for k in ("hs", "gates", "out")}          # largest error against float64: [new, present]
    for M in _row_counts(cuda):
        g = torch.Generator().manual_seed(M)
        xbuf, X = _padded(cuda, M, H, g)
        h0, dense_h0, present_h0 = _h0_forms(K, cuda, form, M, M)
        sv, gi, hs_p, gates_p, out_p = _present(K, X, P, present_h0, dense_h0, M, n_out, cuda)
        # Part A: the trunk without the gate projection, y2 alone
        y2buf, y2 = _padded(cuda, M, H, fill=SENT)
        K.mlp_gi_fwd(X, *P["trunk"], P["Wi"], P["bi"], None, (None, None, None, None, y2, None))
        _bits(y2, sv[4], f"M={M}: y2 without gi")
        assert bool((y2buf[M:] == SENT).all()), f"M={M}: y2 written past M"
        y2buf[M:] = float("nan")                 # (an input from here on)
        # Part B
        hsbuf, hs = _padded(cuda, M, H, fill=SENT)
        gtbuf, gates = _padded(cuda, M, 256, fill=SENT)
        obuf = torch.full((M + 16, n_out + 1), SENT, device=cuda)
        out = obuf[:M, :n_out]                   # row stride n_out + 1
        K.gi_gru1_head_fwd(y2, P["Wi"], P["bi"], P["Wh"], P["bhn"], h0, P["Wo"], P["bo"], out, hs, gates)
        torch.cuda.synchronize()
        for nm, buf in (("hs", hsbuf), ("gates", gtbuf), ("out", obuf)):
            assert bool((buf[M:] == SENT).all()), f"M={M}: {nm} written past M"
        assert bool((obuf[:M, n_out:] == SENT).all()), f"M={M}: out written past n_out"
        _bits(hs, hs_p, f"M={M}: hs")
        _bits(gates, gates_p, f"M={M}: gates")
        hs64, gates64, out64, bound = _f64(P, y2, dense_h0, hs_p)
        assert bool(torch.isfinite(out).all())
        gap = (out.double() - out_p.double()).abs()
        assert bool((gap <= bound).all()), f"M={M}: out is {float((gap / bound).max()):.2f} x the reordered-sum bound from dense_fwd"
        for nm, new, old, want in (("hs", hs, hs_p, hs64), ("gates", gates, gates_p, gates64), ("out", out, out_p, out64)):
            e_new, e_old = _err(new, want), _err(old, want)
            worst[nm][0] = max(worst[nm][0], e_new)
            worst[nm][1] = max(worst[nm][1], e_old)
            if M >= 191:                         # the 2 x rule per row count, where a maximum is an estimate (module docstring)
                print(f"{form} n_out={n_out} M={M} {nm}: error against float64 new {e_new:.3e} present {e_old:.3e}")
                assert e_new <= 2.0 * e_old, f"M={M} {nm}: {e_new:.3e} > 2 x {e_old:.3e}"
        assert worst["out"][1] <= 1e-5 and worst["hs"][1] <= 1e-5, f"M={M}: the restatement disagrees with the present path: {worst}"
    for nm, (new, old) in worst.items():
        print(f"{form} n_out={n_out} {nm}: largest error against float64 new {new:.3e} present {old:.3e}")
        assert new <= 2.0 * old, f"{nm}: {new:.3e} > 2 x {old:.3e}"


@pytest.mark.parametrize("M", [17, 193])
def test_trunk_without_gi_keeps_the_saves(cuda, M):
    """gi == NULL with all six saves: every save is bit-equal to the call with gi; a save other than y2 alone is refused"""
    from dgppo_amd import ops_nn as K
    P = _params(cuda, 2)
    X = torch.randn(M, H, generator=torch.Generator().manual_seed(M)).to(cuda)
    sv, _, _, _, _ = _present(K, X, P, ("dense", None, 1), None, M, 2, cuda)
    sv2 = [torch.full((M, w), SENT, device=cuda) for w in (H, H, 2, H, H, 2)]
    K.mlp_gi_fwd(X, *P["trunk"], P["Wi"], P["bi"], None, tuple(sv2))
    torch.cuda.synchronize()
    for nm, a, b in zip(("p1", "y1", "st1", "p2", "y2", "st2"), sv2, sv):
        _bits(a, b, f"M={M}: {nm} without gi")
    with pytest.raises(ValueError, match="all-or-none"):
        K.mlp_gi_fwd(X, *P["trunk"], P["Wi"], P["bi"], None, (sv2[0], None, None, None, sv2[4], None))
    with pytest.raises(ValueError, match="neither"):
        K.mlp_gi_fwd(X, *P["trunk"], P["Wi"], P["bi"], None, None)
    with pytest.raises(ValueError, match="aligned"):   # the tiled kernel of unaligned rows keeps its gate projection
        K.mlp_gi_fwd(torch.zeros(M, H + 1, device=cuda)[:, 1:], *P["trunk"], P["Wi"], P["bi"], None, (None, None, None, None, sv2[4], None))


def test_optional_outputs_nan_rows_and_repeats(cuda):
    from dgppo_amd import ops_nn as K
    M, n_out = 33, 2
    P = _params(cuda, n_out)
    g = torch.Generator().manual_seed(1)
    y2 = torch.randn(M, H, generator=g).abs().to(cuda)
    h0 = (0.5 * torch.randn(M, H, generator=g)).to(cuda)

    def run(y, h, want_hs=True, want_gates=True):
        hs = torch.full((M, H), SENT, device=cuda) if want_hs else None
        gates = torch.full((M, 256), SENT, device=cuda) if want_gates else None
        out = torch.full((M, n_out), SENT, device=cuda)
        K.gi_gru1_head_fwd(y, P["Wi"], P["bi"], P["Wh"], P["bhn"], h, P["Wo"], P["bo"], out, hs, gates)
        torch.cuda.synchronize()
        return hs, gates, out
    hs, gates, out = run(y2, h0)
    again = run(y2, h0)
    for a, b, nm in zip((hs, gates, out), again, ("hs", "gates", "out")):
        _bits(b, a, f"second launch: {nm}")
    hs1, _, out1 = run(y2, h0, want_gates=False)
    _, gates2, out2 = run(y2, h0, want_hs=False)
    _, _, out3 = run(y2, h0, want_hs=False, want_gates=False)
    _bits(hs1, hs, "hs without gates"); _bits(gates2, gates, "gates without hs")
    for o in (out1, out2, out3):
        _bits(o, out, "out without the optional outputs")
    # a NaN row of y2, another of h0: each stays in its own row
    yn, hn = y2.clone(), h0.clone()
    yn[16] = float("nan"); hn[5, 3] = float("nan")
    hs_n, gates_n, out_n = run(yn, hn)
    bad = torch.zeros(M, dtype=torch.bool, device=cuda)
    bad[16] = bad[5] = True
    for a, b, nm in ((hs_n, hs, "hs"), (gates_n, gates, "gates"), (out_n, out, "out")):
        _bits(a[~bad], b[~bad], f"NaN rows: clean rows of {nm}")
        assert bool(torch.isnan(a[bad]).any(1).all()), f"NaN rows: {nm} lost a NaN"
    assert bool(torch.isnan(hs_n[16]).all()) and bool(torch.isnan(out_n[bad]).all())


def test_misaligned_operands_are_refused_not_launched(cuda):
    from dgppo_amd import _native as N, ops_nn as K
    lib = N.lib()
    M, n, n_out = 18, 3, 2
    P = _params(cuda, n_out)
    z = lambda *s: torch.zeros(*s, device=cuda)
    y2, hs, out, rec, ids = z(M + 1, H), z(M + 1, H), z(M, n_out), z(4, 4, n, H), torch.zeros(2, dtype=torch.int32, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    i64 = C.c_int64

    def call(y, base, es, ts, form=2, hs_=None, rpb=0, bs=0):
        return lib.dgppo_gi_gru1_head_fwd(y, p(P["Wi"]), p(P["bi"]), p(P["Wh"]), p(P["bhn"]), p(P["Wo"]), p(P["bo"]), base, form, rpb,
                                          i64(bs), p(ids), 2, 3, n, i64(es), i64(ts), p(out), n_out, hs_, None, M, n_out, N.stream_ptr())
    es, ts = 4 * n * H, n * H
    off = lambda t: C.c_void_p(t.data_ptr() + 4)
    assert call(p(y2), p(rec), es, ts) == 0, lib.dgppo_last_error()
    assert call(p(y2), off(rec), es, ts) == -1 and b"aligned" in lib.dgppo_last_error()
    assert call(off(y2), p(rec), es, ts) == -1 and b"aligned" in lib.dgppo_last_error()
    assert call(p(y2), p(rec), es, ts, hs_=off(hs)) == -1 and b"aligned" in lib.dgppo_last_error()
    assert call(p(y2), p(rec), es + 2, ts) == -1 and b"multiples of 4" in lib.dgppo_last_error()
    assert call(p(y2), p(rec), es, ts + 1) == -1 and b"multiples of 4" in lib.dgppo_last_error()
    assert call(p(y2), None, es, ts) == -1
    assert call(p(y2), p(rec), es, ts, form=1, rpb=3, bs=3 * H + 2) == -1 and b"block_stride" in lib.dgppo_last_error()
    assert call(p(y2), p(rec), es, ts, form=7) == -1
    assert lib.dgppo_gi_gru1_head_fwd(p(y2), p(P["Wi"]), p(P["bi"]), p(P["Wh"]), p(P["bhn"]), p(P["Wo"]), p(P["bo"]), p(rec), 2, 0,
                                      i64(0), p(ids), 1, 3, n, i64(es), i64(ts), p(out), n_out, None, None, M, n_out,
                                      N.stream_ptr()) == -1 and b"fewer" in lib.dgppo_last_error()
    assert K.gi_gru1_head_ok(y2[:M], None) and not K.gi_gru1_head_ok(y2.view(-1)[1:1 + M * H].view(M, H), None)
    torch.cuda.synchronize()


# ---- Net level -------------------------------------------------------------------------------------------------------------------
def _scene(n, n_obs, n_env, T_steps, seed):
    from dgppo_amd import _native as N
    from oracle import env_np as E
    ocfg = E.EnvCfg(E.LIDAR_SPREAD, n_agents=n, n_obs=n_obs)
    cfg = N.make_env_cfg(E.LIDAR_SPREAD, n, n_obs)
    rng = np.random.default_rng(seed)
    agent, goal, obst = E.env_reset(ocfg, rng.integers(1, 2 ** 60, size=n_env))
    agent[:, :, :2] = (agent[:, :, :2] * 0.5 + 0.4).astype(np.float32)
    tab = E.ray_table(32)
    hits, _ = E.lidar_sense(ocfg, agent[..., :2], obst, *tab)
    agents, hitss = [agent], [hits]
    for t in range(T_steps - 1):
        a = rng.uniform(-1, 1, size=(n_env, n, 2)).astype(np.float32)
        o = E.env_step(ocfg, agent, goal, obst, hits, a, tab)
        agent, hits = o["next_agent"], o["next_hits"]
        agents.append(agent); hitss.append(hits)
    return cfg, np.stack(agents, 1), goal, obst, np.stack(hitss, 1)


def _feats(cfg, ag, goal, obst, hi, dev):
    from dgppo_amd import nets
    n_env, T_steps = ag.shape[:2]
    arena = nets.Arena(dev)
    f = nets.GraphFeats(cfg, n_env * T_steps, arena, "t")
    agd, hid = torch.from_numpy(ag).to(dev), torch.from_numpy(hi).to(dev)
    n, sd = cfg.n_agents, cfg.state_dim
    f.compute(agd, T_steps * n * sd, n * sd, torch.from_numpy(goal).to(dev), torch.from_numpy(obst).to(dev),
              hid, T_steps * n * cfg.top_k * 2, n * cfg.top_k * 2, None, n_env, T_steps)
    f._keep = (agd, hid, arena)
    return f


def _vh_nets(dev, cfg):
    from dgppo_amd import nets
    from oracle import nn_torch as T
    gen = torch.Generator().manual_seed(8)
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), T.init_value(3, cfg.node_dim, 2, 1))
    pair = []
    for flag in (True, False):
        net = nets.Net("Vh", cfg, 1, 2, dev, gi_in_step=flag)
        net.load_tree(tree)
        pair.append(net)
    return pair


def test_net_forward_and_backward_with_and_without_the_pair(cuda, monkeypatch):
    """LidarSpread n = 3, 48 graphs, Vh at T = 1 from a random carry.  Inference: v under the rules of the module docstring (the
    float64 head restated from the old path's h'), and the carry a caller asks for (hs_out) bit-equal.  Training: Net.forward
    keeps the three launches for both nets (the pair's training form is held to them at kernel level above), so the saved
    activations are bit-equal; the backward adds per-workgroup sums with atomics in arrival order (LayerNorm gradients; with
    144 rows the GRU pass has three workgroups, one addend more than the two whose order cannot matter), which no path repeats
    bit for bit, so the flat gradient is held to 3e-5 of the gradient scale, the tolerance of tests/test_bwd_w_paths_gpu.py for
    two backward passes of one network.  A mapped carry at a misaligned base goes to the present launches, whose own check
    refuses it."""
    from dgppo_amd import ops_nn as K
    n, n_env, T_ = 3, 3, 16
    cfg, ag, goal, obst, hi = _scene(n, 2, n_env, T_, seed=11)
    R = n_env * T_ * n
    new, old = _vh_nets(cuda, cfg)
    feats = _feats(cfg, ag, goal, obst, hi, cuda)
    gen = torch.Generator().manual_seed(9)
    h0 = (torch.randn(R, 64, generator=gen) * 0.5).to(cuda)
    calls = []
    monkeypatch.setattr(K, "gi_gru1_head_fwd", (lambda f: lambda *a, **k: (calls.append("pair"), f(*a, **k))[1])(K.gi_gru1_head_fwd))
    monkeypatch.setattr(K, "gru_fwd", (lambda f: lambda *a, **k: (calls.append("gru_fwd"), f(*a, **k))[1])(K.gru_fwd))
    # inference, the head writing into a caller's buffer
    vbuf = torch.full((R, 2), SENT, device=cuda)
    a_new = new.forward(feats, n_seq=R, T=1, h0=h0, train=False, v_out=vbuf)
    a_old = old.forward(feats, n_seq=R, T=1, h0=h0, train=False)
    torch.cuda.synchronize()
    assert calls == ["pair", "gru_fwd"], calls
    assert a_new["v"] is vbuf and a_new["gi"] is None and a_new["hs"] is None and "f.gi" not in new.arena.bufs
    hs_old = a_old["hs"]
    want = hs_old.double() @ old.p("head.Wo").double() + old.p("head.bo").double()
    bound = 2 * 64 * U * (hs_old.double().abs() @ old.p("head.Wo").double().abs() + old.p("head.bo").double().abs())
    assert bool(((vbuf.double() - a_old["v"].double()).abs() <= bound).all())
    e_new, e_old = _err(vbuf, want), _err(a_old["v"], want)
    print(f"net v: error against float64 new {e_new:.3e} present {e_old:.3e}")
    assert e_new <= 2.0 * e_old
    hs_buf = torch.full((R, 64), SENT, device=cuda)
    a_hs = new.forward(feats, n_seq=R, T=1, h0=h0, train=False, hs_out=hs_buf)
    torch.cuda.synchronize()
    _bits(hs_buf, hs_old, "hs_out of the pair")
    _bits(a_hs["v"], vbuf, "v with hs_out")
    assert calls == ["pair", "gru_fwd", "pair"] and "f.gi" not in new.arena.bufs and "f.gi" in old.arena.bufs
    # training forward + backward: the three launches in both nets
    del calls[:]
    dout = (torch.randn(R, 2, generator=gen) / R).to(cuda)
    grads = []
    for net in (new, old):
        act = net.forward(feats, n_seq=R, T=1, h0=h0)
        assert act["hprev"] is h0
        net.zero_grads()
        net.backward(act, dout)
        torch.cuda.synchronize()
        grads.append((act, net.grads.clone()))
    assert calls == ["gru_fwd", "gru_fwd"], calls
    (act_n, g_n), (act_o, g_o) = grads
    for nm in ("y2", "p1", "y1", "st1", "p2", "st2", "hs", "gates"):
        _bits(act_n[nm], act_o[nm], f"training forward: {nm}")
    gscale = max(float(g_o.abs().max()), 1e-3)
    err = float((g_n.double() - g_o.double()).abs().max())
    print(f"net flat gradient: err {err:.3e} bound {3e-5 * gscale:.3e}")
    assert float(g_o.abs().max()) > 0 and err <= 3e-5 * gscale
    # a mapped carry at a misaligned base: not the pair's (the present launch answers, with its refusal)
    del calls[:]
    rec = torch.zeros(n_env * T_ * n * 64 + 1, device=cuda)[1:].view(n_env, T_, n, 64)
    m = K.H0Map(rec, rec.stride(0), rec.stride(1), T_, n, n_env)
    assert not K.gi_gru1_head_ok(act_n["y2"], m)
    with pytest.raises(ValueError, match="gru_fwd_h0_map.*aligned"):
        new.forward(feats, n_seq=R, T=1, h0=m, train=False)
    assert calls == [], calls
