"""The backward glue on the GPU: the one-step GRU backward inside the weight-gradient pass (gru_bwd_w_t1) against the scan
(gru_bwd_dhn, bit for bit in dgi) and float64 (weight gradients), and Net.backward on these paths against the separate
kernels.  Tolerances are those of tests/test_bwd_w_paths_gpu.py: 3e-6 sqrt(M) + 1e-6 for weight gradients (relative to
max(1, |want|)), 3e-5 of the gradient scale for a network's gradients."""
import math
import os
import sys

import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_bwd_w_paths_gpu import _close, _cus, _feats, _scene  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- 1. gru_bwd_w_t1: dgi against the scan, the weight gradients against float64 ----------------------------------------
def _batch(K_, cuda, batched, fn):
    if not batched:
        return fn()
    ws = {}

    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        fn()


def _t1_inputs(cuda, M, seed):
    """(x, h0, dhs, Wh, gates) with gates as the forward saves them for one step from h0"""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(seed)
    Wh = (torch.randn(64, 192, generator=g) * 0.125).to(cuda)
    bhn = (torch.randn(64, generator=g) * 0.1).to(cuda)
    gi = torch.randn(M, 192, generator=g).to(cuda)
    x = torch.randn(M, 64, generator=g).to(cuda)
    h0 = (torch.randn(M, 64, generator=g) * 0.5).to(cuda)
    dhs = torch.randn(M, 64, generator=g).to(cuda)
    hs, gates = torch.empty(M, 64, device=cuda), torch.empty(M, 256, device=cuda)
    K_.gru_fwd(gi, Wh, bhn, h0, hs, None, gates, M, 1, 1)
    return x, h0, dhs, Wh, gates


def _t1_case(cuda, M, batched, x, h0, dhs, Wh, gates, check_w=True):
    from dgppo_amd import ops_nn as K_
    dgi_s = torch.full((M, 192), float("nan"), device=cuda)
    dhn_s = torch.full((M, 64), float("nan"), device=cuda)
    K_.gru_bwd_dhn(dhs, Wh, h0, gates, dgi_s, dhn_s, M, 1, 1)
    # outputs as slices of a flat gradient buffer seen through wider rows (ldw > N), pre-filled: the kernel accumulates
    g = torch.Generator().manual_seed(M + 1)
    flat0 = torch.randn(2 * 64 * 200 + 192 + 64, generator=g)
    flat = flat0.to(cuda)
    dWi, dWh = flat[:64 * 200].view(64, 200)[:, 4:196], flat[64 * 200:2 * 64 * 200].view(64, 200)[:, 8:200]
    dbi, dbhn = flat[2 * 64 * 200:2 * 64 * 200 + 192], flat[2 * 64 * 200 + 192:]
    dgi = torch.full((M, 192), float("nan"), device=cuda)
    _batch(K_, cuda, batched, lambda: K_.gru_bwd_w_t1(x, h0, dhs, gates, dgi, dWi, dbi, dWh, dbhn))
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(dgi), torch.isnan(dgi_s)), "NaNs of dgi differ from the scan's"
    a, b = dgi.cpu().view(torch.int32), dgi_s.cpu().view(torch.int32)
    same = (a == b) | torch.isnan(dgi_s.cpu())
    assert bool(same.all()), f"dgi differs from gru_bwd_dhn in {int((~same).sum())} elements"
    pad = torch.ones(2 * 64 * 200, dtype=torch.bool)
    pad[:64 * 200].view(64, 200)[:, 4:196] = False
    pad[64 * 200:].view(64, 200)[:, 8:200] = False
    assert torch.equal(flat.cpu()[:2 * 64 * 200][pad], flat0[:2 * 64 * 200][pad]), "columns outside the views were written"
    if not check_w:
        return dgi, dgi_s
    ref = flat0.double().clone()
    rWi, rWh = ref[:64 * 200].view(64, 200)[:, 4:196], ref[64 * 200:2 * 64 * 200].view(64, 200)[:, 8:200]
    rbi, rbhn = ref[2 * 64 * 200:2 * 64 * 200 + 192], ref[2 * 64 * 200 + 192:]
    d64, n64 = dgi_s.cpu().double(), dhn_s.cpu().double()
    rWi += x.cpu().double().T @ d64
    rbi += d64.sum(0)
    rWh += h0.cpu().double().T @ torch.cat([d64[:, :128], n64], 1)
    rbhn += n64.sum(0)
    tol = 3e-6 * math.sqrt(M) + 1e-6
    _close(dWi, rWi, tol, f"gru_bwd_w_t1 dWi M={M}")
    _close(dWh, rWh, tol, f"gru_bwd_w_t1 dWh M={M}")
    _close(dbi, rbi, tol, f"gru_bwd_w_t1 dbi M={M}")
    _close(dbhn, rbhn, tol, f"gru_bwd_w_t1 dbhn M={M}")
    return dgi, dgi_s


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("M", [37, 210, 16408, -1])
def test_gru_bwd_w_t1_against_the_scan_and_float64(cuda, M, batched):
    """M = 37: one workgroup, atomicAdd; 210: four ragged workgroups, atomicAdd; 16 408: slabs, ragged; -1: more than two tiles
    on every CU (2 * 64 * CUs + 37)"""
    M = M if M > 0 else 2 * 64 * _cus(cuda) + 37
    _t1_case(cuda, M, batched, *_t1_inputs(cuda, M, seed=M))


def test_gru_bwd_w_t1_negative_zero_and_nan_rows(cuda):
    """Rows of dhs at -0.0 (the scan adds them to its +0.0 carry: every gradient of the row is +-0 with the scan's sign), then one
    NaN row: it stays in its row of dgi, bit for bit where the scan is finite and NaN where the scan is NaN"""
    M = 16408
    x, h0, dhs, Wh, gates = _t1_inputs(cuda, M, seed=5)
    dhs[3] = -0.0
    dhs[M - 1] = -0.0
    dhs[4100, ::2] = -0.0
    dgi, dgi_s = _t1_case(cuda, M, False, x, h0, dhs, Wh, gates)
    assert bool((dgi[3] == 0).all()) and bool((dgi[M - 1] == 0).all())
    dhs[777] = float("nan")
    dgi, dgi_s = _t1_case(cuda, M, True, x, h0, dhs, Wh, gates, check_w=False)
    assert bool(torch.isnan(dgi[777]).all()), "the NaN row lost its NaN"
    keep = torch.ones(M, dtype=torch.bool, device=cuda)
    keep[777] = False
    assert bool(torch.isfinite(dgi[keep]).all()), "the NaN left its row"


def test_gru_bwd_w_t1_refuses_misaligned_rows(cuda):
    from dgppo_amd import ops_nn as K_
    M = 64
    x, h0, dhs, Wh, gates = _t1_inputs(cuda, M, seed=9)
    dW = [torch.zeros(64, 192, device=cuda), torch.zeros(192, device=cuda), torch.zeros(64, 192, device=cuda), torch.zeros(64, device=cuda)]
    off = torch.empty(M * 64 + 1, device=cuda)[1:].view(M, 64)
    off.copy_(dhs)
    with pytest.raises(ValueError, match="16-byte aligned"):
        K_.gru_bwd_w_t1(x, h0, off, gates, torch.empty(M, 192, device=cuda), *dW)


# ---- 2. dense_bwd_xw: dX and dW / db of a Dense from one call, against float64 -------------------------------------------
def _wide(t, pad, cuda, gen):
    """t as a view of a wider pre-filled buffer (leading dimension + pad): (view, whole buffer, its initial copy)"""
    buf0 = torch.randn(t.shape[0], t.shape[1] + pad, generator=gen)
    buf0[:, :t.shape[1]] = t
    buf = buf0.to(cuda)
    return buf[:, :t.shape[1]], buf, buf0


def _xw_case(cuda, M, K, N, misalign=False):
    from dgppo_amd import ops_nn as K_
    gen = torch.Generator().manual_seed(M + 7 * K + N)
    X = torch.relu(torch.randn(M, K, generator=gen))               # a ReLU output: its own mask
    dY = torch.randn(M, N, generator=gen)
    W = torch.randn(K, N, generator=gen) * 0.25
    dX0, dW0, db0 = torch.randn(M, K, generator=gen), torch.randn(K, N, generator=gen), torch.randn(N, generator=gen)
    prod = dY.double() @ W.double().T
    want_W = dW0.double() + X.double().T @ dY.double()
    want_b = db0.double() + dY.double().sum(0)
    tol_x, tol_w = 3e-6 * math.sqrt(N) + 1e-6, 3e-6 * math.sqrt(M) + 1e-6
    if misalign:                                                   # X one float off a 16-byte boundary: the pair must run
        Xd = torch.empty(M * K + 1, device=cuda)[1:].view(M, K)
        Xd.copy_(X)
    else:
        Xd = X.to(cuda)
    dYd, Wd = dY.to(cuda), W.to(cuda)
    # "=": dense operands, with db; dX pre-filled with NaN, which must not survive
    dXd, dWd, dbd = torch.full((M, K), float("nan"), device=cuda), dW0.to(cuda), db0.to(cuda)
    K_.dense_bwd_xw(Xd, dYd, Wd, dXd, dWd, dbd)
    torch.cuda.synchronize()
    _close(dXd, prod, tol_x, f"dense_bwd_xw dX M={M} K={K} N={N}")
    _close(dWd, want_W, tol_w, f"dense_bwd_xw dW M={M} K={K} N={N}")
    _close(dbd, want_b, tol_w, f"dense_bwd_xw db M={M} N={N}")
    # "+=" through the ReLU mask X on a pre-filled dX, db NULL, every leading dimension wider than the width, deferred
    pad = 4 if (K % 4 == 0 and not misalign) else 3
    Xv, _, _ = _wide(X, pad, cuda, gen)
    dYv, _, _ = _wide(dY, 8, cuda, gen)
    Wv, _, _ = _wide(W, 4, cuda, gen)
    dXv, dXbuf, dXbuf0 = _wide(dX0, 12, cuda, gen)
    dWv, dWbuf, dWbuf0 = _wide(dW0, 4, cuda, gen)
    ws = {}

    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        K_.dense_bwd_xw(Xv, dYv, Wv, dXv, dWv, None, accumulate_mask=True)
    torch.cuda.synchronize()
    want_X = torch.where(X.double() > 0, dX0.double() + prod, torch.zeros((), dtype=torch.float64))
    _close(dXv, want_X, tol_x, f"dense_bwd_xw dX += masked M={M} K={K} N={N}")
    _close(dWv, want_W, tol_w, f"dense_bwd_xw dW (wide) M={M} K={K} N={N}")
    assert torch.equal(dXbuf.cpu()[:, K:], dXbuf0[:, K:]), "columns beside dX were written"
    assert torch.equal(dWbuf.cpu()[:, N:], dWbuf0[:, N:]), "columns beside dW were written"
    assert bool(((dXv == 0) | (Xv > 0)).all()), "an entry with X <= 0 is not zero"


@pytest.mark.parametrize("M", [37, 210, 16408, -1])
@pytest.mark.parametrize("K,N", [(144, 64), (32, 96), (48, 32), (48, 64)])
def test_dense_bwd_xw_against_float64(cuda, K, N, M):
    """the four glue shapes ((32, 96) is served by the pair: the library's selector keeps it there, the contract is the same);
    M as for gru_bwd_w_t1: one workgroup, ragged atomicAdd, slabs, more than two tiles on every CU"""
    _xw_case(cuda, M if M > 0 else 2 * 64 * _cus(cuda) + 37, K, N)


@pytest.mark.parametrize("K,N,misalign", [(48, 32, True), (144, 64, True), (46, 32, False), (30, 96, False)])
def test_dense_bwd_xw_takes_the_pair_when_it_must(cuda, K, N, misalign):
    """a misaligned X or a K that is no multiple of 4: the call runs dense_bwd_w + dense_fwd and meets the same bars"""
    _xw_case(cuda, 16408, K, N, misalign=misalign)


# ---- 3. Net backward on the new paths against the separate kernels ------------------------------------------------------
@pytest.mark.parametrize("kind", ["Vh", "policy", "Vl"])
def test_net_backward_new_paths_equal_the_separate_kernels(cuda, kind, monkeypatch):
    """LidarSpread n = 3, 40 graphs.  Vh: T = 1 from a random carry (gru_bwd_w_t1, no scan launch); policy and Vl: T = 4 chunks
    (the scan without its first-step product); the Wout / Mcat glue of every net through dense_bwd_xw as nets.py wires it.
    Against (a) the per-layer loop (gru_bwd + three dense_bwd_w) and, for Vh, (b) the same backward with the one-step path
    switched off (gru_bwd_dhn + gru_bwd_w), both with dense_bwd_xw replaced by the pair dense_bwd_w + dense_fwd(W^T): every
    parameter gradient, every dz = dXa Wout^T and the gradient entering the first GNN layer's output within 3e-5 of the
    gradient scale."""
    from dgppo_amd import nets, ops_nn as K_
    n, n_env, T_ = 3, 10, 4
    cfg, ag, goal, obst, hi = _scene(E.LIDAR_SPREAD, n, 2, n_env, T_, seed=13)
    G, R = n_env * T_, n_env * T_ * n
    gen = torch.Generator().manual_seed(21)
    if kind == "policy":
        tree, net = T.init_policy(1, cfg.node_dim), nets.Net("policy", cfg, 2, 2, cuda)
        n_seq, Tn, h0, rows, n_out = n_env * n, T_, None, R, 4
    elif kind == "Vl":
        tree, net = T.init_value(2, cfg.node_dim, 1, 2), nets.Net("Vl", cfg, 2, 1, cuda)
        n_seq, Tn, h0, rows, n_out = n_env, T_, None, G, 1
    else:
        tree, net = T.init_value(3, cfg.node_dim, 2, 1), nets.Net("Vh", cfg, 1, 2, cuda)
        n_seq, Tn, h0, rows, n_out = R, 1, (torch.randn(R, 64, generator=gen) * 0.5).to(cuda), R, 2
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), tree)
    net.load_tree(tree)
    feats = _feats(cfg, ag, goal, obst, hi, cuda)
    act = net.forward(feats, n_seq=n_seq, T=Tn, h0=h0)
    dout = (torch.randn(rows, n_out, generator=gen) / rows).to(cuda)
    calls = []
    for nm in ("gru_bwd_w_t1", "gru_bwd_dhn", "gru_bwd_w", "gru_bwd"):
        monkeypatch.setattr(K_, nm, (lambda f, nm_: lambda *a, **k: (calls.append(nm_), f(*a, **k))[1])(getattr(K_, nm), nm))
    xw = K_.dense_bwd_xw

    def xw_new(*a, **k):                 # the call under test, recorded
        calls.append("dense_bwd_xw")
        return xw(*a, **k)

    def xw_pair(X, dY, W, dX, dW, db=None, accumulate_mask=False):     # the two launches it stands for at every site
        calls.append("pair")
        K_.dense_bwd_w(X, dY, dW, db)
        K_.dense_fwd(dY, W, None, dX, accumulate=accumulate_mask, trans_w=True, relu_mask=X if accumulate_mask else None)

    def run(a, separate):
        monkeypatch.setattr(K_, "dense_bwd_xw", xw_pair if separate else xw_new)
        del calls[:]
        net.zero_grads()
        net.backward(a, dout)
        torch.cuda.synchronize()
        dx = {f"dz{l}": net.arena.get(f"b.dz{l}", R, net.dims[l][3]).clone() for l in range(net.gnn_layers)}
        if net.gnn_layers > 1:
            dx["dXa1"] = net.arena.get("b.dXa1", R, net.dims[1][1]).clone()
        return net.grads.clone(), dx, list(calls)

    # Wout of every layer, and Mcat of every layer above the first, go through dense_bwd_xw
    n_xw = 2 * net.gnn_layers - 1
    new, new_dx, new_calls = run(act, separate=False)
    assert new_calls.count("dense_bwd_xw") == n_xw and "pair" not in new_calls, new_calls
    gru_calls = [c for c in new_calls if c != "dense_bwd_xw"]
    if kind == "Vh":
        assert act["hprev"] is h0
        assert gru_calls == ["gru_bwd_w_t1"], new_calls
    else:
        assert gru_calls == ["gru_bwd_dhn", "gru_bwd_w"], new_calls
    others = []
    act_loop = dict(act)
    act_loop["stack"] = [dict(x=None, gi=act["gi"], hs=act["hs"], hprev=act["hprev"], gates=act["gates"])]
    others.append(("per-layer loop, Dense pairs",) + run(act_loop, separate=True))
    assert others[0][3][0] == "gru_bwd" and others[0][3].count("pair") == n_xw and "dense_bwd_xw" not in others[0][3], others[0][3]
    if kind == "Vh":
        monkeypatch.setattr(nets.Net, "_gru_t1_in_pass", staticmethod(lambda *a: False))
        others.append(("scan + gru_bwd_w, Dense pairs",) + run(act, separate=True))
        assert [c for c in others[1][3] if c != "pair"] == ["gru_bwd_dhn", "gru_bwd_w"], others[1][3]
    for name, old, old_dx, _ in others:
        gscale = max(float(old.abs().max()), 1e-3)
        err = float((new.double() - old.double()).abs().max())
        print(f"{kind} vs {name}: flat gradient err {err:.3e} bound {3e-5 * gscale:.3e} (scale {gscale:.3e})")
        assert float(old.abs().max()) > 0
        assert err <= 3e-5 * gscale
        for nm, o in old_dx.items():
            xscale = max(float(o.abs().max()), 1e-3)
            xerr = float((new_dx[nm].double() - o.double()).abs().max())
            print(f"{kind} vs {name}: {nm} err {xerr:.3e} bound {3e-5 * xscale:.3e}")
            assert float(o.abs().max()) > 0
            assert xerr <= 3e-5 * xscale
