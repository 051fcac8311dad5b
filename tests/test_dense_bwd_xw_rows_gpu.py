"""dense_bwd_xw where the one-pass kernel can go wrong: its dX tile leaves LDS as whole rows one round behind the products
(the last tile after the loop), the products are dealt over a group's four waves, and the `+=` form requests the old dX ahead.
All four glue shapes, `=` and `+=`, against float64 with the bars of tests/test_bwd_glue_gpu.py for this call:
tol_x = 3e-6 sqrt(N) + 1e-6 for dX, tol_w = 3e-6 sqrt(M) + 1e-6 for dW / db (relative to max(1, |want|))."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_bwd_w_paths_gpu import _close, _cus  # noqa: E402

pytestmark = pytest.mark.gpu

SITES = [(144, 64), (32, 96), (48, 32), (48, 64)]
# one ragged tile; exactly one tile (the store after the loop is the only store); the store of tile t issued in round t + 1; a
# last tile of one row.  -1: 64 CUs + 5 rows, the last workgroup's second group has no rows (and its first a chunk of 5);
# -2: above 2 * 64 * CUs + 37, every CU walks more than two tiles and writes a slab
ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, -1, -2]


def _rows(M, cuda):
    if M == -1:
        return 64 * _cus(cuda) + 5
    if M == -2:
        return 2 * 64 * _cus(cuda) + 101
    return M


def _wide(t, pad, rows_more, gen, cuda):
    """t as the top-left view of a larger pre-filled buffer: (view, whole buffer on the device, its initial host copy)"""
    buf0 = torch.randn(t.shape[0] + rows_more, t.shape[1] + pad, generator=gen)
    buf0[:t.shape[0], :t.shape[1]] = t
    buf = buf0.to(cuda)
    return buf[:t.shape[0], :t.shape[1]], buf, buf0


def _guards_unchanged(buf, buf0, M, W, name):
    got = buf.cpu()
    assert torch.equal(got[:M, W:].view(torch.int32), buf0[:M, W:].view(torch.int32)), f"columns beside {name} were written"
    assert torch.equal(got[M:].view(torch.int32), buf0[M:].view(torch.int32)), f"rows at and above M of {name} were written"


def _run(K_, cuda, deferred, fn):
    if not deferred:
        return fn()
    ws = {}

    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        fn()


_INPUTS = {}


def _inputs(M, K, N):
    """host operands and float64 references of a case, computed once and shared by the tests that need them"""
    key = (M, K, N)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 * M + 7 * K + N)
        X = torch.relu(torch.randn(M, K, generator=gen))           # a ReLU output: its own mask
        dY = torch.randn(M, N, generator=gen)
        W = torch.randn(K, N, generator=gen) * 0.25
        dW0, db0 = torch.randn(K, N, generator=gen), torch.randn(N, generator=gen)
        old = torch.randn(M, K, generator=gen)
        _INPUTS.clear()                                            # one case at a time: the large ones are tens of MB
        _INPUTS[key] = dict(gen=gen, X=X, dY=dY, W=W, dW0=dW0, db0=db0, old=old, prod=dY.double() @ W.double().T,
                            want_W=dW0.double() + X.double().T @ dY.double(), want_b=db0.double() + dY.double().sum(0))
    return _INPUTS[key]


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", SITES)
def test_dense_bwd_xw_assign_form(cuda, K, N, M, deferred):
    """`=`: dX pre-filled with NaN inside a larger buffer (wider rows, more rows): no NaN survives below M, nothing beside or
    above is touched; every operand through a leading dimension wider than its width; db given; two calls agree bit for bit"""
    from dgppo_amd import ops_nn as K_
    M = _rows(M, cuda)
    c = _inputs(M, K, N)
    gen = c["gen"]
    tol_x, tol_w = 3e-6 * math.sqrt(N) + 1e-6, 3e-6 * math.sqrt(M) + 1e-6
    Xv, _, _ = _wide(c["X"], 4, 0, gen, cuda)
    dYv, _, _ = _wide(c["dY"], 8, 0, gen, cuda)
    Wv, _, _ = _wide(c["W"], 4, 0, gen, cuda)
    dWv, dWbuf, dWbuf0 = _wide(c["dW0"], 4, 2, gen, cuda)
    dXv, dXbuf, dXbuf0 = _wide(torch.full((M, K), float("nan")), 12, 3, gen, cuda)
    dbd = c["db0"].to(cuda)
    _run(K_, cuda, deferred, lambda: K_.dense_bwd_xw(Xv, dYv, Wv, dXv, dWv, dbd))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dXv).any()), "a NaN of the pre-filled dX survived below M"
    _close(dXv, c["prod"], tol_x, f"dX = M={M} K={K} N={N}")
    _close(dWv, c["want_W"], tol_w, f"dW M={M} K={K} N={N}")
    _close(dbd, c["want_b"], tol_w, f"db M={M} N={N}")
    _guards_unchanged(dXbuf, dXbuf0, M, K, "dX")
    _guards_unchanged(dWbuf, dWbuf0, K, N, "dW")
    first = dXv.clone()
    dXv.fill_(float("nan"))
    _run(K_, cuda, deferred, lambda: K_.dense_bwd_xw(Xv, dYv, Wv, dXv, dWv, dbd))
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), dXv.view(torch.int32)), "two calls on the same inputs differ in dX"


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", SITES)
def test_dense_bwd_xw_accumulate_form(cuda, K, N, M, deferred):
    """`+=` through the ReLU mask X: the old dX holds NaN, +Inf and -Inf exactly where X <= 0 (those entries come out as exact
    zeros) and finite values elsewhere (added once); db is None; wide leading dimensions; two calls agree bit for bit"""
    from dgppo_amd import ops_nn as K_
    M = _rows(M, cuda)
    c = _inputs(M, K, N)
    gen = c["gen"]
    tol_x, tol_w = 3e-6 * math.sqrt(N) + 1e-6, 3e-6 * math.sqrt(M) + 1e-6
    X = c["X"]
    old = c["old"].clone()
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(M * K).view(M, K) % 3]
    old[X <= 0] = bad[X <= 0]
    Xv, _, _ = _wide(X, 4, 0, gen, cuda)
    dYv, _, _ = _wide(c["dY"], 8, 0, gen, cuda)
    Wv, _, _ = _wide(c["W"], 4, 0, gen, cuda)
    dWv, dWbuf, dWbuf0 = _wide(c["dW0"], 4, 2, gen, cuda)
    dXv, dXbuf, dXbuf0 = _wide(old, 12, 3, gen, cuda)
    _run(K_, cuda, deferred, lambda: K_.dense_bwd_xw(Xv, dYv, Wv, dXv, dWv, None, accumulate_mask=True))
    torch.cuda.synchronize()
    got = dXv.cpu()
    dead = X <= 0
    assert bool((got[dead] == 0).all()), "an entry with X <= 0 is not zero"
    assert bool(torch.isfinite(got).all()), "a non-finite old value left its masked entry"
    want = torch.where(dead, torch.zeros((), dtype=torch.float64), c["old"].double() + c["prod"])
    _close(dXv, want, tol_x, f"dX += M={M} K={K} N={N}")
    _close(dWv, c["want_W"], tol_w, f"dW (+= call) M={M} K={K} N={N}")
    _guards_unchanged(dXbuf, dXbuf0, M, K, "dX")
    _guards_unchanged(dWbuf, dWbuf0, K, N, "dW")
    dXv.copy_(old.to(cuda))
    _run(K_, cuda, deferred, lambda: K_.dense_bwd_xw(Xv, dYv, Wv, dXv, dWv, None, accumulate_mask=True))
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), dXv.cpu().view(torch.int32)), "two calls on the same inputs differ in dX"
