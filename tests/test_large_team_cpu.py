"""The yardstick of tests/test_large_team_gpu.py pinned at large team sizes: the oracle's per-agent fixed-fan-in attention
(oracle/nn_torch.py attn_fixed_fan_in, the contract of dgppo_attn_fwd / _bwd) composed into a whole GraphTransformer layer
equals the per-edge segment-softmax form (gnn_layer) at team sizes the small-n oracle tests do not reach."""
import math

import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T


@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 24, 3), ("MPESpread", 40, 3)])
def test_attn_fixed_fan_in_matches_gnn_layer_at_large_n(kind, n, n_obs):
    """random node rows, random masks (first slot kept), NaN edge features behind the mask.  Per-edge form: the unmasked
    (agent, slot) pairs as an edge list into gnn_layer.  Fixed-fan-in form with the algebra of DESIGN.md "GNN layer":
    qt = q_h(x_i) W_k,h^T / sqrt(D) (the key bias cancels in the softmax), aggregate raw rows and edge features, project
    after: out_i = relu(u(x_i) + mean_h([sum a x_s | sum a e] [W_v,h ; W_e,h] + b_v,h))."""
    cfg = E.EnvCfg(E.KIND_NAMES[kind], n_agents=n, n_obs=n_obs)
    F, H, D, G = 7, 3, 32, 2
    lidar, spread = cfg.is_lidar, cfg.is_spread
    gs = cfg.n_goals if spread else 1
    os_ = (cfg.top_k if n_obs > 0 else 0) if lidar else n_obs
    snd = T.attn_sender_nodes(n, cfg.n_goals, gs, os_, lidar, spread)
    S, N = snd.shape[1], cfg.num_nodes
    assert S == cfg.num_edges // n and int(snd.max()) == N - 2          # every non-pad node id is reached
    gen = torch.Generator().manual_seed(n)
    p = T.tree_map(lambda t: t.double(), T.init_gnn_layer(gen, F, D, H))
    for k in ("Dense_0", "Dense_1", "Dense_2", "Dense_4"):
        p[k]["bias"] = 0.1 * torch.randn(p[k]["bias"].shape, generator=gen, dtype=torch.float64)
    X = torch.randn(G, N - 1, F, generator=gen, dtype=torch.float64)
    em = (torch.rand(G, n, S, generator=gen) > 0.3).double()
    em[:, :, 0] = 1.0
    ef = torch.randn(G, n, S, 4, generator=gen, dtype=torch.float64)
    # fixed-fan-in form
    Xa, Xo = X[:, :n], X[:, n:]
    Wq, Wk = p["Dense_0"]["kernel"].reshape(F, H, D), p["Dense_1"]["kernel"].reshape(F, H, D)
    q = torch.einsum("gif,fhd->gihd", Xa, Wq) + p["Dense_0"]["bias"].reshape(H, D)
    qt = torch.einsum("gihd,fhd->gihf", q, Wk) / math.sqrt(D)
    Kp = F + H * (F + 4) + 1
    ef_nan = torch.where(em[..., None] != 0, ef, torch.full_like(ef, float("nan")))
    z, a = T.attn_fixed_fan_in(snd, qt, Xa, Xo, ef_nan, em, Kp)
    agg = z[..., F:F + H * (F + 4)].reshape(G, n, H, F + 4)
    Wve = torch.cat([p["Dense_2"]["kernel"].reshape(F, H, D), p["Dense_3"]["kernel"].reshape(4, H, D)], 0)   # [F + 4, H, D]
    msg = torch.einsum("gihw,whd->gihd", agg, Wve) + z[..., -1, None, None] * p["Dense_2"]["bias"].reshape(H, D)
    got = torch.relu(T.dense(p["Dense_4"], Xa) + msg.mean(2))
    assert torch.isfinite(got).all()
    # per-edge form, graph by graph: masked slots become pad -> pad edges (they never reach an agent)
    for g in range(G):
        nodes = torch.cat([X[g], torch.zeros(1, F, dtype=torch.float64)], 0)
        keep = em[g] != 0
        recv = torch.where(keep, torch.arange(n)[:, None].expand(n, S), torch.full((n, S), N - 1)).reshape(-1)
        send = torch.where(keep, snd, torch.full((n, S), N - 1)).reshape(-1)
        edges = torch.where(keep[..., None], ef[g], torch.zeros_like(ef[g])).reshape(-1, 4)
        want = T.gnn_layer(p, nodes, edges, send, recv, H, D)[:n]
        torch.testing.assert_close(got[g], want, rtol=0, atol=1e-12)
    assert torch.allclose(a.sum(2), torch.ones(G, n, H, dtype=torch.float64))
