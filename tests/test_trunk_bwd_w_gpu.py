"""dgppo_mlp_gi_bwd_w on the GPU: the backward chain of the MLP trunk that also forms the trunk's weight gradients
(dW2 = y1^T dpre2, dW1 = x^T dpre1 and the two bias sums) from the tiles it holds.

Reference: float64 torch autograd of the plain composition Dense -> LayerNorm -> ReLU -> Dense -> LayerNorm -> ReLU -> Dense(192),
the construction of test_mlp_gi_bwd_fused in tests/test_nn_gpu.py.  Bounds: 3e-6 sqrt(M) + 1e-6 for dW* / dbias* (that of
test_dense_bwd_w for the same (M, 64, 64) products), 3e-5 for the LayerNorm gradients, both relative to max(1, |want|).

Against ops_nn.mlp_gi_bwd on the same inputs dx and dpre* are bit-equal at every M.  The LayerNorm gradients dg* / db* are
bit-equal wherever their sum has a defined order, which is up to two workgroups (M <= 32: fp32 addition commutes).  From three
workgroups on, both kernels add the SAME per-workgroup partial sums (same tiles per workgroup) with atomicAdd in whatever order
the workgroups finish, so two launches of either kernel may differ in the last bits.  There the two are held to the bound of a
reordered fp32 sum of n terms, 2 (n - 1) 2^-24 sum|terms|, with n the number of workgroups and sum|terms| taken from the
float64 reference."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [1, 15, 16, 17, 45, 33000]
_CASES = {}


def _close(got, want, tol, name):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})"


def _case(M):
    """inputs (fp32, CPU) and the float64 reference gradients of one M; computed once and left unchanged"""
    if M in _CASES:
        return _CASES[M]
    g = torch.Generator().manual_seed(M + 11)
    X = torch.randn(M, 64, generator=g)
    P = {k: (torch.randn(*shp, generator=g) * sc) for k, shp, sc in (
        ("W1", (64, 64), 0.2), ("b1", (64,), 0.1), ("g1", (64,), 1.0), ("be1", (64,), 0.1), ("W2", (64, 64), 0.2),
        ("b2", (64,), 0.1), ("g2", (64,), 1.0), ("be2", (64,), 0.1), ("Wi", (64, 192), 0.2), ("bi", (192,), 0.1))}
    dgi = torch.randn(M, 192, generator=g)
    mask = torch.randn(M, 64, generator=g)
    D = {k: v.double().requires_grad_() for k, v in P.items()}
    Xd = X.double().requires_grad_()

    def ln(v, gam, bet):   # flax LayerNorm: fast variance, eps 1e-6
        mean = v.mean(-1, keepdim=True)
        var = ((v * v).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        rstd = torch.rsqrt(var + 1e-6)
        return (v - mean) * rstd * gam + bet, mean, rstd
    p1 = Xd @ D["W1"] + D["b1"]; p1.retain_grad()
    o1, m1, r1 = ln(p1, D["g1"], D["be1"]); o1.retain_grad(); y1 = torch.relu(o1)
    p2 = y1 @ D["W2"] + D["b2"]; p2.retain_grad()
    o2, m2, r2 = ln(p2, D["g2"], D["be2"]); o2.retain_grad(); y2 = torch.relu(o2)
    gi = y2 @ D["Wi"] + D["bi"]
    gi.backward(dgi.double())
    f = lambda t: t.detach().float().contiguous()
    c = dict(M=M, P=P, dgi=dgi, mask=mask, X=X,
             saves=dict(p2=f(p2), y2=f(y2), st2=f(torch.cat([m2, r2], 1)), p1=f(p1), y1=f(y1), st1=f(torch.cat([m1, r1], 1))),
             want=dict(dx=Xd.grad, dpre2=p2.grad, dpre1=p1.grad, dg2=D["g2"].grad, db2=D["be2"].grad, dg1=D["g1"].grad,
                       db1=D["be1"].grad, dW2=D["W2"].grad, dbias2=D["b2"].grad, dW1=D["W1"].grad, dbias1=D["b1"].grad),
             # sum over the rows of |term| of each LayerNorm gradient, for the reordering bound
             sabs=dict(dg2=float((o2.grad * ((p2 - m2) * r2).detach()).abs().sum(0).max()), db2=float(o2.grad.abs().sum(0).max()),
                       dg1=float((o1.grad * ((p1 - m1) * r1).detach()).abs().sum(0).max()), db1=float(o1.grad.abs().sum(0).max())))
    _CASES[M] = c
    return c


def _run_w(K_, c, dev, masked, x_is_mask, with_dpre, dW0=None):
    """one mlp_gi_bwd_w call; returns its outputs.  x_is_mask: the chain's input is the mask tensor (policy / Vh form); else a
    separate x, passed as a strided view (the Vl form when masked is False)."""
    M = c["M"]
    d = lambda t: t.to(dev).contiguous()
    sv = {k: d(v) for k, v in c["saves"].items()}
    P = {k: d(v) for k, v in c["P"].items()}
    if x_is_mask:
        x = mask = d(c["X"])                      # the trunk input masks its own gradient
    else:
        xw = torch.zeros(M, 80, device=dev)
        xw[:, 8:72] = d(c["X"])
        x, mask = xw[:, 8:72], (d(c["mask"]) if masked else None)
    o = {k: torch.full((M, 64), float("nan"), device=dev) for k in ("dx",) + (("dpre2", "dpre1") if with_dpre else ())}
    o.update({k: torch.zeros(64, device=dev) for k in ("dg2", "db2", "dg1", "db1")})
    for k, shp in (("dW2", (64, 64)), ("dbias2", (64,)), ("dW1", (64, 64)), ("dbias1", (64,))):
        o[k] = d(dW0[k]) if dW0 is not None else torch.zeros(*shp, device=dev)
    K_.mlp_gi_bwd_w(d(c["dgi"]), P["Wi"], P["W2"], P["W1"], P["g2"], P["g1"], sv["p2"], sv["y2"], sv["st2"], sv["p1"], sv["y1"],
                    sv["st1"], x, mask, o["dx"], o["dg2"], o["db2"], o["dg1"], o["db1"], o["dW2"], o["dbias2"], o["dW1"],
                    o["dbias1"], o.get("dpre2"), o.get("dpre1"))
    return o, mask, (sv, P)


def _workgroups(M, dev):
    return min((M + 15) // 16, 2 * torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.mark.parametrize("variant", ["masked_x_is_mask", "masked_separate_x", "unmasked_separate_x"])
@pytest.mark.parametrize("with_dpre", [False, True])
@pytest.mark.parametrize("M", MS)
def test_mlp_gi_bwd_w(cuda, M, with_dpre, variant):
    from dgppo_amd import ops_nn as K_
    c = _case(M)
    masked, x_is_mask = variant != "unmasked_separate_x", variant == "masked_x_is_mask"
    o, mask, (sv, P) = _run_w(K_, c, cuda, masked, x_is_mask, with_dpre)
    torch.cuda.synchronize()
    # the chain without the weight gradients, on the same inputs
    ref = {k: torch.full((M, 64), float("nan"), device=cuda) for k in ("dpre2", "dpre1", "dx")}
    ref.update({k: torch.zeros(64, device=cuda) for k in ("dg2", "db2", "dg1", "db1")})
    K_.mlp_gi_bwd(c["dgi"].to(cuda), P["Wi"], P["W2"], P["W1"], P["g2"], P["g1"], sv["p2"], sv["y2"], sv["st2"], sv["p1"], sv["y1"],
                  sv["st1"], mask, ref["dpre2"], ref["dpre1"], ref["dx"], ref["dg2"], ref["db2"], ref["dg1"], ref["db1"])
    torch.cuda.synchronize()
    assert torch.equal(o["dx"], ref["dx"]), "dx differs from mlp_gi_bwd"
    if with_dpre:
        assert torch.equal(o["dpre2"], ref["dpre2"]) and torch.equal(o["dpre1"], ref["dpre1"]), "dpre differs from mlp_gi_bwd"
    n_wg = _workgroups(M, cuda)
    for k in ("dg2", "db2", "dg1", "db1"):
        if n_wg <= 2:
            assert torch.equal(o[k], ref[k]), f"{k} differs from mlp_gi_bwd"
        else:
            err = float((o[k].double() - ref[k].double()).abs().max())
            bound = 2.0 * (n_wg - 1) * 2.0 ** -24 * c["sabs"][k]
            print(f"{k} vs mlp_gi_bwd ({n_wg} workgroups): {err:.3e} bound {bound:.3e}")
            assert err <= bound, f"{k} vs mlp_gi_bwd: {err:.3e} > {bound:.3e}"
    # float64 reference
    w = c["want"]
    mk = mask.cpu() if mask is not None else None
    want_dx = w["dx"] * (mk > 0) if mk is not None else w["dx"]
    _close(o["dx"], want_dx, 2e-5, "dx")
    tol = 3e-6 * math.sqrt(M) + 1e-6
    for k in ("dW2", "dbias2", "dW1", "dbias1"):
        _close(o[k], w[k], tol, f"{k} M={M}")
    for k in ("dg2", "db2", "dg1", "db1"):
        _close(o[k], w[k], 3e-5, f"{k} M={M}")


@pytest.mark.parametrize("M", [17, 45, 33000])
def test_mlp_gi_bwd_w_accumulates_and_defers(cuda, M):
    """dW / dbias accumulate onto what they hold; inside a BwdWBatch, next to an unrelated dense_bwd_w, the deferred reduction
    gives what the immediate one gives, to the same tolerance"""
    from dgppo_amd import ops_nn as K_
    c = _case(M)
    g = torch.Generator().manual_seed(5)
    dW0 = {k: torch.randn(*shp, generator=g) for k, shp in (("dW2", (64, 64)), ("dbias2", (64,)), ("dW1", (64, 64)), ("dbias1", (64,)))}
    tol = 3e-6 * math.sqrt(M) + 1e-6
    now, _, _ = _run_w(K_, c, cuda, True, True, False, dW0)
    torch.cuda.synchronize()
    Xo = torch.randn(100, 64, generator=g).to(cuda); dYo = torch.randn(100, 64, generator=g).to(cuda)
    other = torch.zeros(64, 64, device=cuda)
    ws = {}

    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        later, _, _ = _run_w(K_, c, cuda, True, True, False, dW0)
        K_.dense_bwd_w(Xo, dYo, other)
    torch.cuda.synchronize()
    for k in ("dW2", "dbias2", "dW1", "dbias1"):
        _close(now[k], dW0[k].double() + c["want"][k], tol, f"immediate {k} M={M}")
        _close(later[k], dW0[k].double() + c["want"][k], tol, f"deferred {k} M={M}")
        _close(later[k], now[k], tol, f"deferred vs immediate {k} M={M}")
    assert torch.equal(later["dx"], now["dx"])
    _close(other, Xo.double().T @ dYo.double(), 3e-6 * 10 + 1e-6, "deferred neighbour")


def test_mlp_gi_bwd_w_zero_rows_touch_nothing(cuda):
    from dgppo_amd import ops_nn as K_
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    z = lambda *s: torch.zeros(*s, device=cuda)
    outs = [nan(0, 64)] + [nan(64) for _ in range(4)] + [nan(64, 64), nan(64), nan(64, 64), nan(64)]
    for batched in (False, True):
        args = (z(0, 192), z(64, 192), z(64, 64), z(64, 64), z(64), z(64), z(0, 64), z(0, 64), z(0, 2), z(0, 64), z(0, 64), z(0, 2),
                z(0, 64), None, *outs)
        if batched:
            with K_.BwdWBatch(cuda, lambda n: torch.empty(n, device=cuda)) as b:
                K_.mlp_gi_bwd_w(*args)
                assert b.descs == []                                # nothing is owed
        else:
            K_.mlp_gi_bwd_w(*args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs[1:])
