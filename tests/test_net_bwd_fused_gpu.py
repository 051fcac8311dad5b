"""Net.backward with the trunk's weight gradients formed inside the backward chain kernel (dgppo_mlp_gi_bwd_w) and the head's
backward in one pass (dgppo_head_bwd), against the same backward with both calls replaced, by a local monkeypatch, with the
launches they stand for: dgppo_mlp_gi_bwd writing dpre2 / dpre1 and two dense_bwd_w; dense_bwd_w and dense_fwd^T per head layer.
Vl and a policy without a recurrent cell are the forms the other network tests do not reach: Vl's chain input is the pooled
rows, a tensor of its own, and nothing masks dx; without a cell the head reads the MLP output and the trunk keeps its separate
kernels.  LidarSpread n = 3, 48 graphs; every leaf at 3e-5 of the gradient scale, the bound of
test_net_backward_equals_the_separate_kernels."""
import os
import sys

import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_bwd_w_paths_gpu import _feats, _scene  # noqa: E402

pytestmark = pytest.mark.gpu


def _separate(K_):
    """mlp_gi_bwd_w as the three launches it replaces"""
    def fn(dgi, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, x, relu_mask, dx, dg2, db2, dg1, db1, dW2, dbias2, dW1, dbias1,
           dpre2=None, dpre1=None):
        dpre2, dpre1 = torch.empty_like(dx), torch.empty_like(dx)
        K_.mlp_gi_bwd(dgi, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, relu_mask, dpre2, dpre1, dx, dg2, db2, dg1, db1)
        K_.dense_bwd_w(y1, dpre2, dW2, dbias2)
        K_.dense_bwd_w(x, dpre1, dW1, dbias1)
    return fn


def _separate_head(K_):
    """head_bwd as the four (two) launches it replaces"""
    def fn(feat, u, dout, W1, W2, dhs, dW1, db1, dW2=None, db2=None):
        if W2 is not None:
            K_.dense_bwd_w(u, dout, dW2, db2)
            du = torch.empty_like(dhs)
            K_.dense_fwd(dout, W2, None, du, trans_w=True)
            K_.dense_bwd_w(feat, du, dW1, db1)
            K_.dense_fwd(du, W1, None, dhs, trans_w=True)
        else:
            K_.dense_bwd_w(feat, dout, dW1, db1)
            K_.dense_fwd(dout, W1, None, dhs, trans_w=True)
    return fn


@pytest.mark.parametrize("kind", ["Vl", "policy_no_rnn"])
def test_net_backward_trunk_and_head(cuda, kind, monkeypatch):
    from dgppo_amd import nets, ops_nn as K_
    n, n_env, T_ = 3, 3, 16
    cfg, ag, goal, obst, hi = _scene(E.LIDAR_SPREAD, n, 2, n_env, T_, seed=12)
    G, R = n_env * T_, n_env * T_ * n
    gen = torch.Generator().manual_seed(9)
    if kind == "Vl":
        tree = T.init_value(5, cfg.node_dim, 1, 2)
        net = nets.Net("Vl", cfg, 2, 1, cuda)
        n_seq, Tn, h0, rows, n_out = n_env, T_, None, G, 1
    else:
        tree = T.init_policy(1, cfg.node_dim, rnn_layers=0)
        net = nets.Net("policy", cfg, 2, 2, cuda, rnn="none")
        n_seq, Tn, h0, rows, n_out = n_env * n, T_, None, R, 4
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), tree)
    net.load_tree(tree)
    feats = _feats(cfg, ag, goal, obst, hi, cuda)
    act = net.forward(feats, n_seq=n_seq, T=Tn, h0=h0)
    dout = (torch.randn(rows, n_out, generator=gen) / rows).to(cuda)
    calls = []
    real_t, real_h = K_.mlp_gi_bwd_w, K_.head_bwd
    monkeypatch.setattr(K_, "mlp_gi_bwd_w", lambda *a, **k: (calls.append("trunk"), real_t(*a, **k))[1])
    monkeypatch.setattr(K_, "head_bwd", lambda *a, **k: (calls.append("head"), real_h(*a, **k))[1])
    net.zero_grads()
    net.backward(act, dout)
    torch.cuda.synchronize()
    assert calls == (["head", "trunk"] if kind == "Vl" else ["head"]), f"the backward took {calls}"
    new = net.grads.clone()
    monkeypatch.setattr(K_, "mlp_gi_bwd_w", _separate(K_))
    monkeypatch.setattr(K_, "head_bwd", _separate_head(K_))
    net.zero_grads()
    net.backward(act, dout)
    torch.cuda.synchronize()
    old = net.grads.clone()
    gscale = max(float(old.abs().max()), 1e-3)
    net.grads.copy_(new)
    for nm in ("mlp.W2", "mlp.b2", "mlp.W1", "mlp.b1") + (("head.Wo", "head.bo") if kind == "Vl" else ("head.Ws", "head.Wms", "head.bms")):
        assert float(net.g(nm).abs().max()) > 0, nm
    err = float((new.double() - old.double()).abs().max())
    print(f"{kind} flat gradient: err {err:.3e} bound {3e-5 * gscale:.3e} (scale {gscale:.3e})")
    assert err <= 3e-5 * gscale
