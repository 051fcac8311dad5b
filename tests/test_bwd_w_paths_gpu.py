"""The weight-gradient paths of the backward pass on the GPU: the GRU backward that leaves (dgi, dhn), the one-pass GRU
weight-gradient kernel, the one-slab-per-CU dense_bwd_w launches, and a Net backward against the separate kernels in their
earlier order.  References are float64 on the CPU; tolerances are those of tests/test_nn_gpu.py: 3e-6 sqrt(M) + 1e-6 for weight
gradients (relative to max(1, |want|)), 3e-5 of the gradient scale for the GRU parameter gradients of a network."""
import math

import numpy as np
import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

pytestmark = pytest.mark.gpu


def _close(got, want, tol, name):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max abs err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})"


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- 1. gru_bwd_dhn against gru_bwd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grp,T_,n_inner,use_h0", [(5, 16, 8, False), (70, 1, 3, True), (9, 7, 1, True),
                                                     (2051, 2, 8, True),       # 16 408 sequences: the 32-sequence-tile kernels
                                                     (16390, 1, 1, True)])     # same kernels, T = 1, ragged last tile
def test_gru_bwd_dhn_is_bit_equal_to_gru_bwd(cuda, n_grp, T_, n_inner, use_h0):
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(n_grp + T_)
    n_seq = n_grp * n_inner
    rows = n_seq * T_
    Wh = (torch.randn(64, 192, generator=g) * 0.125).to(cuda)
    bhn = (torch.randn(64, generator=g) * 0.1).to(cuda)
    gi = torch.randn(rows, 192, generator=g).to(cuda)
    h0 = (torch.randn(n_seq, 64, generator=g) * 0.5).to(cuda) if use_h0 else None
    dhs = torch.randn(rows, 64, generator=g).to(cuda)
    hs = torch.empty(rows, 64, device=cuda)
    hprev = torch.empty(rows, 64, device=cuda)
    gates = torch.empty(rows, 256, device=cuda)
    K_.gru_fwd(gi, Wh, bhn, h0, hs, hprev, gates, n_seq, T_, n_inner)
    dgi_a = torch.full((rows, 192), float("nan"), device=cuda)
    dgh_a = torch.full((rows, 192), float("nan"), device=cuda)
    K_.gru_bwd(dhs, Wh, hprev, gates, dgi_a, dgh_a, n_seq, T_, n_inner)
    dgi_b = torch.full((rows, 192), float("nan"), device=cuda)
    dhn_b = torch.full((rows, 64), float("nan"), device=cuda)
    K_.gru_bwd_dhn(dhs, Wh, hprev, gates, dgi_b, dhn_b, n_seq, T_, n_inner)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dgi_a).all()) and bool(torch.isfinite(dgh_a).all())
    assert torch.equal(dgi_a, dgi_b), "dgi differs between the two forms"
    assert torch.equal(dgh_a[:, 128:], dhn_b), "dhn differs from dgh[:, 128:]"
    assert torch.equal(dgh_a[:, :128], dgi_a[:, :128])          # what makes the duplicate a duplicate
    if T_ == 1 and use_h0:                                       # the T = 1 alias: h before the only step is h0
        assert torch.equal(hprev, h0)
        hs2 = torch.empty(rows, 64, device=cuda)
        K_.gru_fwd(gi, Wh, bhn, h0, hs2, None, gates, n_seq, T_, n_inner)
        assert torch.equal(hs2, hs)


# ---- 2. gru_bwd_w against float64 -------------------------------------------------------------------------------------
def _gru_w_case(cuda, M, batched):
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(M)
    x, hp = torch.randn(M, 64, generator=g), torch.randn(M, 64, generator=g)
    dgi, dhn = torch.randn(M, 192, generator=g), torch.randn(M, 64, generator=g)
    # outputs as slices of a flat gradient buffer seen through wider rows (ldw > N), pre-filled: the kernel accumulates
    flat0 = torch.randn(2 * 64 * 200 + 192 + 64, generator=g)
    flat = flat0.to(cuda)
    dWi, dWh = flat[:64 * 200].view(64, 200)[:, 3:195], flat[64 * 200:2 * 64 * 200].view(64, 200)[:, 8:200]
    dbi, dbhn = flat[2 * 64 * 200:2 * 64 * 200 + 192], flat[2 * 64 * 200 + 192:]
    ref = flat0.double().clone()
    rWi, rWh = ref[:64 * 200].view(64, 200)[:, 3:195], ref[64 * 200:2 * 64 * 200].view(64, 200)[:, 8:200]
    rbi, rbhn = ref[2 * 64 * 200:2 * 64 * 200 + 192], ref[2 * 64 * 200 + 192:]
    rWi += x.double().T @ dgi.double()
    rbi += dgi.double().sum(0)
    rWh += hp.double().T @ torch.cat([dgi[:, :128], dhn], 1).double()
    rbhn += dhn.double().sum(0)
    args = (x.to(cuda), hp.to(cuda), dgi.to(cuda), dhn.to(cuda), dWi, dbi, dWh, dbhn)
    if batched:
        ws = {}
        def alloc(n):
            ws["t"] = torch.empty(n, device=cuda)
            return ws["t"]
        with K_.BwdWBatch(cuda, alloc):
            K_.gru_bwd_w(*args)
    else:
        K_.gru_bwd_w(*args)
    torch.cuda.synchronize()
    tol = 3e-6 * math.sqrt(M) + 1e-6
    # the whole flat buffer: the gradients, and the padding columns between them untouched
    pad = torch.ones(2 * 64 * 200, dtype=torch.bool)
    pad[:64 * 200].view(64, 200)[:, 3:195] = False
    pad[64 * 200:].view(64, 200)[:, 8:200] = False
    assert torch.equal(flat.cpu()[:2 * 64 * 200][pad], flat0[:2 * 64 * 200][pad]), "columns outside the views were written"
    _close(dWi, rWi, tol, f"gru_bwd_w dWi M={M}")
    _close(dWh, rWh, tol, f"gru_bwd_w dWh M={M}")
    _close(dbi, rbi, tol, f"gru_bwd_w dbi M={M}")
    _close(dbhn, rbhn, tol, f"gru_bwd_w dbhn M={M}")


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("M", [37, 210, 16408, -1])
def test_gru_bwd_w_against_float64(cuda, M, batched):
    """M = 37: one workgroup, atomicAdd; 210: four ragged workgroups, atomicAdd; 16 408: slabs, ragged; -1: more than two tiles
    on every CU (2 * 64 * CUs + 37)"""
    _gru_w_case(cuda, M if M > 0 else 2 * 64 * _cus(cuda) + 37, batched)


# ---- 3. dense_bwd_w: every (K, N) of the networks through the atomic, per-group and per-CU slab launches ----------------
def _groups(K, N):
    """4-wave groups of a workgroup: what a CU's 160 KB of LDS holds of the double-buffered 32-row tiles, at most 4"""
    kt, nt = -(-K // 16), -(-N // 16)
    kt = next(v for v in (1, 2, 3, 4, 6, 8, 9, 12, 16) if v >= kt)
    nt = next(v for v in (1, 2, 4, 6, 12) if v >= nt)
    kl = kt * 16 + (0 if kt & 1 else 16)
    nl = nt * 16 + (0 if nt & 1 else 16)
    return max(1, min(4, (160 * 1024) // (2 * 4 * 32 * (kl + nl))))


@pytest.mark.parametrize("which", ["atomic", "ragged", "empty_groups", "two_tiles_per_group"])
@pytest.mark.parametrize("K,N", [(64, 192), (64, 128), (64, 64), (144, 64), (32, 96), (48, 32), (64, 4)])
def test_dense_bwd_w_slab_paths(cuda, K, N, which):
    from dgppo_amd import ops_nn as K_
    cus = _cus(cuda)
    M = {"atomic": 200, "ragged": 777, "empty_groups": 64 * cus + 32,
         "two_tiles_per_group": 2 * 64 * _groups(K, N) * cus + 19}[which]
    g = torch.Generator().manual_seed(M + K + N)
    X, dY = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    dW0, db0 = torch.randn(K, N + 5, generator=g), torch.randn(N, generator=g)
    want_W = dW0[:, 2:2 + N].double() + X.double().T @ dY.double()
    want_b = db0.double() + dY.double().sum(0)
    Xd, dYd = X.to(cuda), dY.to(cuda)
    tol = 3e-6 * math.sqrt(M) + 1e-6
    for with_db in (True, False):
        dWw, db = dW0.to(cuda), db0.to(cuda)
        K_.dense_bwd_w(Xd, dYd, dWw[:, 2:2 + N], db if with_db else None)
        torch.cuda.synchronize()
        _close(dWw[:, 2:2 + N], want_W, tol, f"dense_bwd_w dW M={M} K={K} N={N} db={with_db}")
        assert torch.equal(dWw[:, :2].cpu(), dW0[:, :2]) and torch.equal(dWw[:, 2 + N:].cpu(), dW0[:, 2 + N:])
        if with_db:
            _close(db, want_b, tol, f"dense_bwd_w db M={M} N={N}")
        else:
            assert torch.equal(db.cpu(), db0)
    # and deferred, next to a second gradient in the same batch
    dWw, db = dW0.to(cuda), db0.to(cuda)
    other = torch.zeros(K, N, device=cuda)
    ws = {}
    def alloc(n):
        ws["t"] = torch.empty(n, device=cuda)
        return ws["t"]
    with K_.BwdWBatch(cuda, alloc):
        K_.dense_bwd_w(Xd, dYd, dWw[:, 2:2 + N], db)
        K_.dense_bwd_w(Xd[:100], dYd[:100], other)
    torch.cuda.synchronize()
    _close(dWw[:, 2:2 + N], want_W, tol, f"deferred dW M={M} K={K} N={N}")
    _close(db, want_b, tol, f"deferred db M={M} N={N}")
    _close(other, X[:100].double().T @ dY[:100].double(), 3e-6 * 10 + 1e-6, "deferred neighbour")


# ---- 4. Net backward end to end -----------------------------------------------------------------------------------------
def _scene(kind, n, n_obs, n_env, T_steps, seed):
    from dgppo_amd import _native as N
    ocfg = E.EnvCfg(kind, n_agents=n, n_obs=n_obs)
    cfg = N.make_env_cfg(kind, n, n_obs)
    rng = np.random.default_rng(seed)
    agent, goal, obst = E.env_reset(ocfg, rng.integers(1, 2 ** 60, size=n_env))
    agent[:, :, :2] = (agent[:, :, :2] * 0.5 + 0.4).astype(np.float32)
    tab = E.ray_table(32)
    hits, _ = E.lidar_sense(ocfg, agent[..., :2], obst, *tab)
    agents, hitss = [agent], [hits]
    for t in range(T_steps - 1):
        a = rng.uniform(-1, 1, size=(n_env, n, 2)).astype(np.float32)
        out = E.env_step(ocfg, agent, goal, obst, hits, a, tab)
        agent, hits = out["next_agent"], out["next_hits"]
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


@pytest.mark.parametrize("kind", ["policy", "Vh"])
def test_net_backward_equals_the_separate_kernels(cuda, kind):
    """LidarSpread n = 3, 48 graphs.  policy: T = 16 chunks from a zero carry; Vh: T = 1 from a random carry (which the
    backward now reads as hprev).  The GRU parameter gradients are rebuilt from gru_bwd + three dense_bwd_w, the earlier
    sequence, on the same upstream gradient; every other leaf is compared with a backward that takes the per-layer loop."""
    from dgppo_amd import nets, ops_nn as K_
    n, n_env, T_ = 3, 3, 16
    cfg, ag, goal, obst, hi = _scene(E.LIDAR_SPREAD, n, 2, n_env, T_, seed=11)
    G, R = n_env * T_, n_env * T_ * n
    gen = torch.Generator().manual_seed(8)
    if kind == "policy":
        tree = T.init_policy(1, cfg.node_dim)
        net = nets.Net("policy", cfg, 2, 2, cuda)
        n_seq, Tn, h0, n_out = n_env * n, T_, None, 4
    else:
        tree = T.init_value(3, cfg.node_dim, 2, 1)
        net = nets.Net("Vh", cfg, 1, 2, cuda)
        n_seq, Tn, h0, n_out = R, 1, (torch.randn(R, 64, generator=gen) * 0.5).to(cuda), 2
    tree = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), tree)
    net.load_tree(tree)
    feats = _feats(cfg, ag, goal, obst, hi, cuda)
    act = net.forward(feats, n_seq=n_seq, T=Tn, h0=h0)
    if kind == "Vh":
        assert act["hprev"] is h0
    dout = (torch.randn(R, n_out, generator=gen) / R).to(cuda)
    net.zero_grads()
    net.backward(act, dout)
    torch.cuda.synchronize()
    new = net.grads.clone()
    # the earlier GRU sequence from the public kernels, on the dhs the backward left in the arena
    dhs = net.arena.get("b.dhs", R, 64)
    dgi, dgh = torch.empty(R, 192, device=cuda), torch.empty(R, 192, device=cuda)
    K_.gru_bwd(dhs, net.p("gru.Wh"), act["hprev"], act["gates"], dgi, dgh, n_seq, Tn, n)
    want = {nm: torch.zeros_like(net.g(nm)) for nm in ("gru.Wi", "gru.bi", "gru.Wh", "gru.bhn")}
    K_.dense_bwd_w(act["hprev"], dgh[:, :128], want["gru.Wh"][:, :128], None)
    K_.dense_bwd_w(act["hprev"], dgh[:, 128:], want["gru.Wh"][:, 128:], want["gru.bhn"])
    K_.dense_bwd_w(act["y2"], dgi, want["gru.Wi"], want["gru.bi"])
    torch.cuda.synchronize()
    # all leaves: the same backward through the per-layer loop (gru_bwd + three dense_bwd_w)
    act_old = dict(act)
    act_old["stack"] = [dict(x=None, gi=act["gi"], hs=act["hs"], hprev=act["hprev"], gates=act["gates"])]
    net.zero_grads()
    net.backward(act_old, dout)
    torch.cuda.synchronize()
    old = net.grads.clone()
    gscale = max(float(old.abs().max()), 1e-3)
    net.grads.copy_(new)                       # net.g(name) views the new gradients again
    for nm, w in want.items():
        err = float((net.g(nm).double() - w.double()).abs().max())
        print(f"{kind} {nm}: err {err:.3e} bound {3e-5 * gscale:.3e}")
        assert float(w.abs().max()) > 0
        assert err <= 3e-5 * gscale, f"{kind} {nm}: {err:.3e} > {3e-5 * gscale:.3e}"
    err = float((new.double() - old.double()).abs().max())
    print(f"{kind} flat gradient: err {err:.3e} bound {3e-5 * gscale:.3e} (scale {gscale:.3e})")
    assert err <= 3e-5 * gscale
