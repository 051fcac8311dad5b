"""dgppo_head_bwd on the GPU: the backward of the output head in one pass over the rows, in its two-layer (policy) and
one-layer (value) forms, against float64 and against the launches it replaces (dense_bwd_w, dense_fwd transposed, dense_bwd_w,
dense_fwd transposed; or the first two alone).  Bounds: 3e-6 sqrt(M) + 1e-6 for the weight gradients (test_dense_bwd_w's, on
unit-normal rows), 2e-5 for dhs, both relative to max(1, |want|)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

_CASES = {}


def _close(got, want, tol, name):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})"


def _case(M, n_out, two):
    """fp32 inputs on the CPU and the float64 results; computed once per shape and left unchanged"""
    key = (M, n_out, two)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(M * 7 + n_out * 3 + int(two))
    c = dict(M=M, n_out=n_out, two=two, feat=torch.randn(M, 64, generator=g), dout=torch.randn(M, n_out, generator=g))
    f, d = c["feat"].double(), c["dout"].double()
    if two:
        c["u"] = torch.randn(M, 64, generator=g)
        c["W1"], c["W2"] = torch.randn(64, 64, generator=g) * 0.2, torch.randn(64, n_out, generator=g) * 0.2
        du = d @ c["W2"].double().T
        c["want"] = dict(dW2=c["u"].double().T @ d, db2=d.sum(0), dW1=f.T @ du, db1=du.sum(0), dhs=du @ c["W1"].double().T)
    else:
        c["W1"] = torch.randn(64, n_out, generator=g) * 0.2
        c["want"] = dict(dW1=f.T @ d, db1=d.sum(0), dhs=d @ c["W1"].double().T)
    _CASES[key] = c
    return c


def _names(two):
    return ("dW1", "db1", "dW2", "db2") if two else ("dW1", "db1")


def _run(K_, c, dev, ldf=64, init=None):
    """one head_bwd call; feat is a view at column 32 of an [M, ldf] buffer when ldf > 64 (the packed carry of two GRU layers)"""
    M, n_out, two = c["M"], c["n_out"], c["two"]
    if ldf > 64:
        wide = torch.zeros(M, ldf, device=dev)
        off = ldf - 64
        wide[:, off:] = c["feat"].to(dev)
        feat = wide[:, off:]
    else:
        feat = c["feat"].to(dev)
    o = dict(dhs=torch.full((M, 64), float("nan"), device=dev))
    shapes = dict(dW1=(64, 64) if two else (64, n_out), db1=(64,) if two else (n_out,), dW2=(64, n_out), db2=(n_out,))
    for k in _names(two):
        o[k] = init[k].to(dev).clone() if init is not None else torch.zeros(*shapes[k], device=dev)
    K_.head_bwd(feat, c["u"].to(dev) if two else None, c["dout"].to(dev), c["W1"].to(dev), c["W2"].to(dev) if two else None,
                o["dhs"], o["dW1"], o["db1"], o.get("dW2"), o.get("db2"))
    return o


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("n_out", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("M", [1, 17, 45, 33000])
def test_head_bwd(cuda, M, n_out, two):
    from dgppo_amd import ops_nn as K_
    c = _case(M, n_out, two)
    tol = 3e-6 * math.sqrt(M) + 1e-6
    o = _run(K_, c, cuda, ldf=128)
    torch.cuda.synchronize()
    for k in _names(two):
        _close(o[k], c["want"][k], tol, f"{k} M={M} n_out={n_out} two={two}")
    _close(o["dhs"], c["want"]["dhs"], 2e-5, f"dhs M={M} n_out={n_out} two={two}")
    # the launches it replaces
    d = lambda t: t.to(cuda)
    feat, dout = d(c["feat"]), d(c["dout"])
    sep = {k: torch.zeros_like(o[k]) for k in _names(two)}
    dhs = torch.empty(M, 64, device=cuda)
    if two:
        du = torch.empty(M, 64, device=cuda)
        K_.dense_bwd_w(d(c["u"]), dout, sep["dW2"], sep["db2"])
        K_.dense_fwd(dout, d(c["W2"]), None, du, trans_w=True)
        K_.dense_bwd_w(feat, du, sep["dW1"], sep["db1"])
        K_.dense_fwd(du, d(c["W1"]), None, dhs, trans_w=True)
    else:
        K_.dense_bwd_w(feat, dout, sep["dW1"], sep["db1"])
        K_.dense_fwd(dout, d(c["W1"]), None, dhs, trans_w=True)
    torch.cuda.synchronize()
    for k in _names(two):
        _close(o[k], sep[k], tol, f"{k} vs separate launches M={M} n_out={n_out}")
    _close(o["dhs"], dhs, 2e-5, f"dhs vs separate launches M={M} n_out={n_out}")


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("M", [17, 45, 33000])
def test_head_bwd_accumulates_and_defers(cuda, M, two):
    """the weight gradients accumulate onto what they hold; inside a BwdWBatch, next to an unrelated dense_bwd_w, the deferred
    reduction gives what the immediate one gives, to the same tolerance"""
    from dgppo_amd import ops_nn as K_
    n_out = 4 if two else 2
    c = _case(M, n_out, two)
    g = torch.Generator().manual_seed(6)
    init = {k: torch.randn(*c["want"][k].shape, generator=g) for k in _names(two)}
    tol = 3e-6 * math.sqrt(M) + 1e-6
    now = _run(K_, c, cuda, init=init)
    torch.cuda.synchronize()
    Xo = torch.randn(100, 64, generator=g).to(cuda); dYo = torch.randn(100, 64, generator=g).to(cuda)
    other = torch.zeros(64, 64, device=cuda)
    ws = {}

    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        later = _run(K_, c, cuda, init=init)
        K_.dense_bwd_w(Xo, dYo, other)
    torch.cuda.synchronize()
    for k in _names(two):
        _close(now[k], init[k].double() + c["want"][k], tol, f"immediate {k} M={M}")
        _close(later[k], init[k].double() + c["want"][k], tol, f"deferred {k} M={M}")
        _close(later[k], now[k], tol, f"deferred vs immediate {k} M={M}")
    assert torch.equal(later["dhs"], now["dhs"])
    _close(other, Xo.double().T @ dYo.double(), 3e-6 * 10 + 1e-6, "deferred neighbour")


@pytest.mark.parametrize("two", [True, False])
def test_head_bwd_zero_rows_touch_nothing(cuda, two):
    from dgppo_amd import ops_nn as K_
    n_out = 4 if two else 2
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    z = lambda *s: torch.zeros(*s, device=cuda)
    outs = [nan(64, 64), nan(64), nan(64, n_out), nan(n_out)] if two else [nan(64, n_out), nan(n_out)]
    args = (z(0, 64), z(0, 64) if two else None, z(0, n_out), z(64, 64) if two else z(64, n_out), z(64, n_out) if two else None,
            nan(0, 64), *outs)
    K_.head_bwd(*args)
    with K_.BwdWBatch(cuda, lambda n: torch.empty(n, device=cuda)) as b:
        K_.head_bwd(*args)
        assert b.descs == []                                    # nothing is owed
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs)


def test_head_bwd_refuses_misaligned_operands(cuda):
    """feat starting 4 bytes into a row, and a leading dimension that is no multiple of 4: refused with a message, no launch
    (the NaN-filled outputs stay as they are)"""
    from dgppo_amd import _native as N, ops_nn as K_
    M, n_out = 40, 2
    z = lambda *s: torch.zeros(*s, device=cuda)
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    outs = dict(dhs=nan(M, 64), dW1=nan(64, n_out), db1=nan(n_out))
    for feat in (z(M, 72)[:, 1:65], z(M, 66)[:, :64]):
        with pytest.raises(ValueError, match="16-byte aligned"):
            K_.head_bwd(feat, None, z(M, n_out), z(64, n_out), None, outs["dhs"], outs["dW1"], outs["db1"])
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values())
    assert b"head_bwd" in N.lib().dgppo_last_error()
