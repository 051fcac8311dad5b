"""Developer tool: GPU time of the network building blocks at training sizes (minibatch of 16384 LidarSpread n=8 graphs)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, ops_nn as K

dev = torch.device("cuda:0")
R = 131072          # agent rows of a minibatch (16384 graphs x 8)
Ro = 16384 * 72


HBM_TBS = 4.5      # the streaming rate DESIGN 4.2 holds the one-pass Dense backward to: `x HBM` = time over bytes at that rate


def timeit(name, fn, iters=20, flops=None, bytes_=None, hbm=False):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    extra = ""
    if flops:
        extra += f"  {flops / us / 1e6:7.1f} TFLOP/s"
    if bytes_:
        extra += f"  {bytes_ / us / 1e3:7.0f} GB/s"
        if hbm:
            extra += f"  {us / (bytes_ / (HBM_TBS * 1e6)):5.2f} x HBM"
    print(f"{name:44s} {us:9.1f} us{extra}", flush=True)


def dense_case(M, Kd, Nd, trans=False, act=0):
    X = torch.randn(M, Kd, device=dev)
    W = torch.randn(Nd, Kd, device=dev) if trans else torch.randn(Kd, Nd, device=dev)
    b = torch.randn(Nd, device=dev)
    Y = torch.empty(M, Nd, device=dev)
    timeit(f"dense_fwd M={M} K={Kd} N={Nd} trans={int(trans)}", lambda: K.dense_fwd(X, W, b, Y, act=act, trans_w=trans),
           flops=2.0 * M * Kd * Nd, bytes_=4.0 * M * (Kd + Nd))
    dW = torch.zeros(Kd, Nd, device=dev); db = torch.zeros(Nd, device=dev)
    if not trans:
        timeit(f"dense_bwd_w M={M} K={Kd} N={Nd}", lambda: K.dense_bwd_w(X, Y, dW, db), flops=2.0 * M * Kd * Nd,
               bytes_=4.0 * M * (Kd + Nd))


which = sys.argv[1] if len(sys.argv) > 1 else "all"
if which in ("all", "dense"):
    for (M, Kd, Nd, tr) in [(R, 144, 64, False), (R, 64, 64, False), (R, 64, 192, False), (R, 48, 32, False), (R, 32, 96, False),
                            (R, 8, 24, False), (Ro, 8, 32, False), (R, 64, 144, True), (R, 192, 64, True), (R, 64, 64, True),
                            (R, 64, 4, False), (R, 4, 64, True), (R, 1, 64, True), (32768, 8, 24, False), (32768, 144, 64, False), (32768, 64, 64, False), (32768, 64, 192, False)]:
        dense_case(M, Kd, Nd, tr)
if which in ("all", "dense", "densemask"):
    # the ReLU-masked input gradients of the update: dX = (mask > 0) ? dY @ W^T : 0
    for (M, Kd, Nd) in [(R, 64, 64), (R, 192, 64), (R, 64, 144), (Ro, 32, 32)]:
        X = torch.randn(M, Kd, device=dev); W = torch.randn(Nd, Kd, device=dev); Y = torch.empty(M, Nd, device=dev)
        mk = torch.randn(M, Nd, device=dev)
        timeit(f"dense_fwd masked M={M} K={Kd} N={Nd} trans=1", lambda: K.dense_fwd(X, W, None, Y, trans_w=True, relu_mask=mk),
               flops=2.0 * M * Kd * Nd, bytes_=4.0 * M * (Kd + 2 * Nd))
if which in ("all", "elem"):
    x = torch.randn(R, 64, device=dev); g = torch.ones(64, device=dev); b = torch.zeros(64, device=dev)
    y = torch.empty_like(x); st = torch.empty(R, 2, device=dev); dx = torch.empty_like(x)
    dg = torch.zeros(64, device=dev); dbb = torch.zeros(64, device=dev)
    timeit("ln_relu_fwd R x 64", lambda: K.ln_relu_fwd(x, g, b, y, st), bytes_=4.0 * R * 128)
    timeit("ln_relu_bwd R x 64", lambda: K.ln_relu_bwd(x, y, st, g, x, dx, dg, dbb), bytes_=4.0 * R * 256)
    timeit("relu_bwd R x 64", lambda: K.relu_bwd(dx, y), bytes_=4.0 * R * 128)
    gi = torch.randn(R, 192, device=dev); Wh = torch.randn(64, 192, device=dev) * 0.1; bh = torch.zeros(64, device=dev)
    hs = torch.empty(R, 64, device=dev); hp = torch.empty(R, 64, device=dev); gt = torch.empty(R, 256, device=dev)
    timeit("gru_fwd n_seq=8192 T=16", lambda: K.gru_fwd(gi, Wh, bh, None, hs, hp, gt, R // 16, 16, 8))
    dgi = torch.empty(R, 192, device=dev); dgh = torch.empty(R, 192, device=dev)
    timeit("gru_bwd n_seq=8192 T=16", lambda: K.gru_bwd(hs, Wh, hp, gt, dgi, dgh, R // 16, 16, 8))
    h0 = torch.randn(32768, 64, device=dev); gi1 = torch.randn(32768, 192, device=dev); hs1 = torch.empty(32768, 64, device=dev)
    timeit("gru_fwd rollout n_seq=32768 T=1", lambda: K.gru_fwd(gi1, Wh, bh, h0, hs1, None, None, 32768, 1, 8))
if which in ("all", "gruw"):
    # the GRU backward's two forms and its weight gradients: one pass against the three dense_bwd_w calls it replaces
    for M, T_ in ((R, 16), (R, 1), (16384, 16)):
        Wh = torch.randn(64, 192, device=dev) * 0.1
        x = torch.randn(M, 64, device=dev); hp = torch.randn(M, 64, device=dev); gt = torch.rand(M, 256, device=dev)
        dhs = torch.randn(M, 64, device=dev)
        dgi = torch.empty(M, 192, device=dev); dgh = torch.empty(M, 192, device=dev); dhn = torch.empty(M, 64, device=dev)
        dWi = torch.zeros(64, 192, device=dev); dbi = torch.zeros(192, device=dev)
        dWh = torch.zeros(64, 192, device=dev); dbhn = torch.zeros(64, device=dev)
        timeit(f"gru_bwd (dgi, dgh) M={M} T={T_}", lambda: K.gru_bwd(dhs, Wh, hp, gt, dgi, dgh, M // T_, T_, 8), bytes_=4.0 * M * 832)
        timeit(f"gru_bwd_dhn (dgi, dhn) M={M} T={T_}", lambda: K.gru_bwd_dhn(dhs, Wh, hp, gt, dgi, dhn, M // T_, T_, 8), bytes_=4.0 * M * 704)

        def three():
            K.dense_bwd_w(hp, dgh[:, :128], dWh[:, :128], None)
            K.dense_bwd_w(hp, dgh[:, 128:], dWh[:, 128:], dbhn)
            K.dense_bwd_w(x, dgi, dWi, dbi)
        timeit(f"GRU weight gradients: 3 x dense_bwd_w M={M}", three, flops=2.0 * M * 64 * 384, bytes_=4.0 * M * 576)
        timeit(f"GRU weight gradients: gru_bwd_w M={M}", lambda: K.gru_bwd_w(x, hp, dgi, dhn, dWi, dbi, dWh, dbhn),
               flops=2.0 * M * 64 * 384, bytes_=4.0 * M * 384)
if which in ("all", "gruw1"):
    # the one-step GRU backward (Vh: T = 1 from h0): scan + weight-gradient pass against the pass that forms the gate gradients
    # itself; inside a BwdWBatch, so each time includes one batched slab-reduce launch.  Three repeats, alternating
    M = R
    Wh = torch.randn(64, 192, device=dev) * 0.1
    x = torch.randn(M, 64, device=dev); h0 = torch.randn(M, 64, device=dev); gt = torch.rand(M, 256, device=dev)
    dhs = torch.randn(M, 64, device=dev)
    dgi = torch.empty(M, 192, device=dev); dhn = torch.empty(M, 64, device=dev)
    dW = [torch.zeros(64, 192, device=dev), torch.zeros(192, device=dev), torch.zeros(64, 192, device=dev), torch.zeros(64, device=dev)]
    wsbuf = torch.empty(16 << 20, device=dev)

    def pair():
        with K.BwdWBatch(dev, lambda n: wsbuf):
            K.gru_bwd_dhn(dhs, Wh, h0, gt, dgi, dhn, M, 1, 8)
            K.gru_bwd_w(x, h0, dgi, dhn, *dW)

    def one():
        with K.BwdWBatch(dev, lambda n: wsbuf):
            K.gru_bwd_w_t1(x, h0, dhs, gt, dgi, *dW)
    for rep in range(3):
        timeit(f"GRU T=1 bwd: gru_bwd_dhn + gru_bwd_w M={M}", pair, iters=50, bytes_=4.0 * M * (384 + 256 + 256 + 384))
        if hasattr(K, "gru_bwd_w_t1"):
            timeit(f"GRU T=1 bwd: gru_bwd_w_t1 M={M}", one, iters=50, bytes_=4.0 * M * (64 + 64 + 64 + 256 + 192))
if which in ("all", "h0map"):
    # Vh's minibatch pair (T = 1 forward + weight-gradient pass) at 131 072 rows from the carry record of 4096 envs x 128 steps x
    # 8 agents: the gathered copy (gather_rows of 128 env rows included) against the map over the env-major and over the
    # time-major record through the same ids.  Also the value pre-pass read (528 384 graphs, 129 slots per env): the env-major blocks against the time-major map.
    # Three repeats, alternating
    Bm, Tm, nm, Em = 4096, 128, 8, 128
    M = Em * Tm * nm
    tm = torch.randn(Tm + 2, Bm, nm, 64, device=dev)
    em = tm.transpose(0, 1).contiguous()                       # [B, T+2, n, 64], what finalize() used to make
    ids = torch.randperm(Bm, device=dev)[:Em].to(torch.int32)
    Wh = torch.randn(64, 192, device=dev) * 0.1; bh = torch.zeros(64, device=dev)
    gi = torch.randn(M, 192, device=dev); hs = torch.empty(M, 64, device=dev); gt = torch.empty(M, 256, device=dev)
    x = torch.randn(M, 64, device=dev); dhs = torch.randn(M, 64, device=dev); dgi = torch.empty(M, 192, device=dev)
    dW = [torch.zeros(64, 192, device=dev), torch.zeros(192, device=dev), torch.zeros(64, 192, device=dev), torch.zeros(64, device=dev)]
    wsbuf = torch.empty(16 << 20, device=dev)
    h0g = torch.empty(Em, Tm, nm, 64, device=dev)
    hmap = K.H0Map(tm[1], tm.stride(1), tm.stride(0), Tm, nm, Em, ids=ids, n_env_src=Bm)

    def gathered():
        K.gather_rows([(em[:, 1:Tm + 1], h0g)], ids)
        K.gru_fwd(gi, Wh, bh, h0g.view(M, 64), hs, None, gt, M, 1, nm)
        with K.BwdWBatch(dev, lambda n: wsbuf):
            K.gru_bwd_w_t1(x, h0g.view(M, 64), dhs, gt, dgi, *dW)

    rs = em[:, 1:Tm + 1]
    hmap_em = K.H0Map(rs, rs.stride(0), rs.stride(1), Tm, nm, Em, ids=ids, n_env_src=Bm)

    def mapped(m):
        K.gru_fwd_h0_map(gi, Wh, bh, m, hs, None, gt, M, 1, nm)
        with K.BwdWBatch(dev, lambda n: wsbuf):
            K.gru_bwd_w_t1(x, m, dhs, gt, dgi, *dW)
    for rep in range(3):
        timeit(f"Vh T=1 pair M={M}: gather + dense h0", gathered, iters=50)
        timeit(f"Vh T=1 pair M={M}: mapped h0 (env-major, ids)", lambda: mapped(hmap_em), iters=50)
        timeit(f"Vh T=1 pair M={M}: mapped h0 (time-major, ids)", lambda: mapped(hmap), iters=50)
    Ep = Bm
    Mp = Ep * (Tm + 1) * nm
    gip = torch.randn(Mp, 192, device=dev); hsp = torch.empty(Mp, 64, device=dev)
    blocks = K.H0Blocks(em[0, 0], (Tm + 1) * nm, (Tm + 2) * nm * 64, Ep)
    pmap = K.H0Map(tm[0], tm.stride(1), tm.stride(0), Tm + 1, nm, Ep, n_env_src=Bm)
    for rep in range(3):
        timeit(f"pre-pass gru_fwd M={Mp}: env-major blocks", lambda: K.gru_fwd_h0_blocks(gip, Wh, bh, blocks, hsp, None, None, Mp, 1, nm),
               iters=50, bytes_=4.0 * Mp * 320)
        timeit(f"pre-pass gru_fwd M={Mp}: time-major map", lambda: K.gru_fwd_h0_map(gip, Wh, bh, pmap, hsp, None, None, Mp, 1, nm),
               iters=50, bytes_=4.0 * Mp * 320)
if which in ("all", "gistep"):
    # Vh's one-step tail from the trunk's input rows to the values: the three launches (mlp_gi_fwd with gi, gru_fwd_h0_map,
    # dense_fwd) against the pair (mlp_gi_fwd without gi, gi_gru1_head_fwd; only where the library has it: the same script times
    # an older library).  Pre-pass form: 4 227 072 rows (4096 envs x 129 steps x 8 agents), mapped h0 without ids, nothing saved.
    # Training form: 131 072 rows (128 envs by ids x 128 steps x 8), the six saves, hs and gates written.  Step form: 32 768
    # rows (4096 envs x 8, one step: the shield's and the landscapes' size), dense h0, nothing saved.  The trunk of each form is
    # also timed alone, with and without its gate projection.  Three repeats, alternating
    Bm, Tm, nm, Em, nh = 4096, 128, 8, 128, 2
    tm = torch.randn(Tm + 2, Bm, nm, 64, device=dev) * 0.5
    g_ = torch.Generator(device="cpu").manual_seed(2)
    rnd = lambda *s, k=1.0: (k * torch.randn(*s, generator=g_)).to(dev)
    P = [rnd(64, 64, k=0.2), rnd(64, k=0.1), 1.0 + rnd(64, k=0.1), rnd(64, k=0.1), rnd(64, 64, k=0.2), rnd(64, k=0.1),
         1.0 + rnd(64, k=0.1), rnd(64, k=0.1), rnd(64, 192, k=0.2), rnd(192, k=0.1)]
    Wh, bh, Wo, bo = rnd(64, 192, k=0.2), rnd(64, k=0.1), rnd(64, nh, k=0.3), rnd(nh, k=0.1)
    has_pair = hasattr(N.lib(), "dgppo_gi_gru1_head_fwd")
    ids = torch.randperm(Bm, device=dev)[:Em].to(torch.int32)
    for label, M, hmap, train in (("pre-pass", Bm * (Tm + 1) * nm, K.H0Map(tm[0], tm.stride(1), tm.stride(0), Tm + 1, nm, Bm, n_env_src=Bm), False),
                                  ("minibatch", Em * Tm * nm, K.H0Map(tm[1], tm.stride(1), tm.stride(0), Tm, nm, Em, ids=ids, n_env_src=Bm), True),
                                  ("step", Bm * nm, tm[3].reshape(Bm * nm, 64), False)):
        X = torch.randn(M, 64, device=dev).relu_()
        gi = torch.empty(M, 192, device=dev); hs = torch.empty(M, 64, device=dev); v = torch.empty(M, nh, device=dev)
        y2 = torch.empty(M, 64, device=dev)
        sv = tuple(torch.empty(M, w, device=dev) for w in (64, 64, 2, 64, 64, 2)) if train else None
        gt = torch.empty(M, 256, device=dev) if train else None

        def three():
            K.mlp_gi_fwd(X, *P, gi, sv)
            if isinstance(hmap, K.H0Map):
                K.gru_fwd_h0_map(gi, Wh, bh, hmap, hs, None, gt, M, 1, nm)
            else:
                K.gru_fwd(gi, Wh, bh, hmap, hs, None, gt, M, 1, nm)
            K.dense_fwd(hs, Wo, bo, v)

        def pair():
            K.mlp_gi_fwd(X, *P, None, sv if train else (None, None, None, None, y2, None))
            K.gi_gru1_head_fwd(sv[4] if train else y2, P[8], P[9], Wh, bh, hmap, Wo, bo, v, hs if train else None, gt)
        for rep in range(3):
            timeit(f"Vh {label} tail M={M}: three launches", three, iters=20)
            if has_pair:
                timeit(f"Vh {label} tail M={M}: pair", pair, iters=20)
            timeit(f"Vh {label} trunk M={M}: with gi", lambda: K.mlp_gi_fwd(X, *P, gi, sv), iters=20)
            if has_pair:
                timeit(f"Vh {label} trunk M={M}: y2 only", lambda: K.mlp_gi_fwd(X, *P, None, sv if train else (None, None, None, None, y2, None)), iters=20)
if which in ("all", "featlayout"):
    # dgppo_graph_feats reading the env-major record [B, T+1, ...] against the time-major one [T+1, B, ...] (env and time stride
    # swapped): the minibatch form (128 envs by ids x 128 steps = 16 384 graphs) and the pre-pass form (4096 envs x 129 steps =
    # 528 384 graphs), LidarSpread n = 8 / 3 obstacles.  Three repeats each, alternating
    from dgppo_amd import nets
    cfg = N.make_env_cfg(0, 8, 3)
    Bm, Tm, nm = 4096, 128, 8
    ag_tm = torch.rand(Tm + 1, Bm, nm, cfg.state_dim, device=dev) * 2.0
    hi_tm = ag_tm[..., None, :2] + 0.3 * torch.rand(Tm + 1, Bm, nm, cfg.top_k, 2, device=dev)
    ag_em, hi_em = ag_tm.transpose(0, 1).contiguous(), hi_tm.transpose(0, 1).contiguous()
    goal = torch.rand(Bm, nm, cfg.state_dim, device=dev) * 2.0
    obst = torch.rand(Bm, 3, 16, device=dev)
    ids = torch.randperm(Bm, device=dev)[:128].to(torch.int32)
    ia, ih = nm * cfg.state_dim, nm * cfg.top_k * 2
    arena = nets.Arena(dev)
    for n_env, n_time, use_ids in ((128, Tm, True), (Bm, Tm + 1, False)):
        f = nets.GraphFeats(cfg, n_env * n_time, arena, "bench")
        e_ids = ids if use_ids else None
        em = lambda: f.compute(ag_em, (Tm + 1) * ia, ia, goal, obst, hi_em, (Tm + 1) * ih, ih, e_ids, n_env, n_time)
        tmj = lambda: f.compute(ag_tm, ia, Bm * ia, goal, obst, hi_tm, ih, Bm * ih, e_ids, n_env, n_time)
        for rep in range(3):
            timeit(f"graph_feats G={n_env * n_time}: env-major record", em, iters=20)
            timeit(f"graph_feats G={n_env * n_time}: time-major record", tmj, iters=20)
if which in ("all", "xw"):
    # both gradients of a GNN glue Dense: dense_bwd_w + dense_fwd(W^T) against the one dense_bwd_xw call, per site of
    # Net._backward_body; inside a BwdWBatch (kernel plus its share of the batched reduce).  Three repeats, alternating
    for Kd, Nd, accm in ((144, 64, False), (32, 96, True), (48, 32, False), (48, 64, False)):
        M = R
        X = torch.relu(torch.randn(M, Kd, device=dev)); dY = torch.randn(M, Nd, device=dev); W = torch.randn(Kd, Nd, device=dev) * 0.1
        dX = torch.zeros(M, Kd, device=dev); dW = torch.zeros(Kd, Nd, device=dev); db = torch.zeros(Nd, device=dev)
        wsbuf = torch.empty(16 << 20, device=dev)

        def pair():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                K.dense_bwd_w(X, dY, dW, db)
                K.dense_fwd(dY, W, None, dX, accumulate=accm, trans_w=True, relu_mask=X if accm else None)

        def one():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                K.dense_bwd_xw(X, dY, W, dX, dW, db, accumulate_mask=accm)
        nbytes = 4.0 * M * (Kd + Nd + Kd * (2 if accm else 1))
        for rep in range(3):
            timeit(f"dense bwd K={Kd} N={Nd}: dense_bwd_w + dense_fwd^T", pair, iters=50, bytes_=nbytes, hbm=True)
            if hasattr(K, "dense_bwd_xw"):
                timeit(f"dense bwd K={Kd} N={Nd}: dense_bwd_xw", one, iters=50, bytes_=nbytes, hbm=True)
if which in ("all", "attn"):
    cfg = N.make_env_cfg(0, 8, 3)
    for G in (16384, 4096):
        Rg = G * 8
        for (F, Kp) in ((8, 48), (32, 144)):
            qt = torch.randn(Rg, 3 * F, device=dev); Xa = torch.randn(Rg, F, device=dev); Xo = torch.randn(G * 72, F, device=dev)
            ef = torch.randn(Rg, 24, 4, device=dev); em = (torch.rand(Rg, 24, device=dev) > 0.3).float()
            em[:, 8:16] = 1.0
            z = torch.empty(Rg, Kp, device=dev); at = torch.empty(Rg, 24, 3, device=dev)
            timeit(f"attn_fwd G={G} F={F}", lambda: K.attn_fwd(cfg, F, 3, Kp, qt, Xa, Xo, ef, em, z, at, G))
            dq = torch.empty_like(qt); dXa = torch.empty_like(Xa); dXo = torch.empty_like(Xo)
            timeit(f"attn_bwd G={G} F={F}", lambda: K.attn_bwd(cfg, F, 3, Kp, z, at, qt, Xa, Xo, ef, dq, dXa, dXo, G))
            if F == 32:   # how much of the wide backward is the input gradient (dXs: 160 of its 320 MFMAs, 10 KB of stores per graph)
                timeit(f"attn_bwd G={G} F={F} (dqt only)", lambda: K.attn_bwd(cfg, F, 3, Kp, z, at, qt, Xa, Xo, ef, dq, None, None, G))
            if F == 32 and K.attn_xo_supported(cfg, F, 3, Kp):   # other-node rows recomputed from the raw features in the kernel
                raw = torch.randn(Xo.shape[0], 8, device=dev); Wo = torch.randn(8, 32, device=dev) * 0.5; bo = torch.randn(32, device=dev) * 0.3
                timeit(f"attn_fwd_xo G={G} F={F}", lambda: K.attn_fwd_xo(cfg, F, 3, Kp, qt, Xa, raw, Wo, bo, ef, em, z, at, G))
                timeit(f"attn_fwd_xo G={G} F={F} (inference)", lambda: K.attn_fwd_xo(cfg, F, 3, Kp, qt, Xa, raw, Wo, bo, ef, em, z, None, G))
                timeit(f"attn_bwd_xo G={G} F={F}", lambda: K.attn_bwd_xo(cfg, F, 3, Kp, z, at, qt, Xa, raw, Wo, bo, ef, dq, dXa, dXo, G, relu_xo=True))
                dWo = torch.zeros(8, 32, device=dev); dbo = torch.zeros(32, device=dev); ws = torch.empty(K.attn_xo_workspace_floats(G), device=dev)
                timeit(f"attn_bwd_xo_dw G={G} F={F} (+ slab reduce)", lambda: K.attn_bwd_xo_dw(cfg, F, 3, Kp, z, at, qt, Xa, raw, Wo, bo, ef, dq, dXa, dWo, dbo, ws, G))
            if F == 8:    # the first layer needs no input gradient
                timeit(f"attn_bwd G={G} F={F} (dqt only)", lambda: K.attn_bwd(cfg, F, 3, Kp, z, at, qt, Xa, Xo, ef, dq, None, None, G))
if which in ("all", "fused"):
    for M, train in ((32768, False), (131072, False), (131072, True)):
        X = torch.randn(M, 64, device=dev)
        P = [torch.randn(*s, device=dev) * 0.1 for s in ((64, 64), (64,), (64,), (64,), (64, 64), (64,), (64,), (64,), (64, 192), (192,))]
        gi = torch.empty(M, 192, device=dev)
        sv = tuple(torch.empty(M, w, device=dev) for w in (64, 64, 2, 64, 64, 2)) if train else None
        timeit(f"mlp_gi_fwd M={M} train={train}", lambda: K.mlp_gi_fwd(X, *P, gi, sv))
if which in ("all", "fusedbwd"):
    for M in (131072, 16384):
        P = [torch.randn(*s_, device=dev) * 0.1 for s_ in ((64, 192), (64, 64), (64, 64), (64,), (64,))]
        dgi = torch.randn(M, 192, device=dev)
        A = [torch.randn(M, w, device=dev) for w in (64, 64, 2, 64, 64, 2)]
        mask = torch.randn(M, 64, device=dev)
        o = [torch.empty(M, 64, device=dev) for _ in range(3)]
        pg = [torch.zeros(64, device=dev) for _ in range(4)]
        timeit(f"mlp_gi_bwd fused M={M}", lambda: K.mlp_gi_bwd(dgi, P[0], P[1], P[2], P[3], P[4], A[3], A[4], A[5], A[0], A[1], A[2], mask,
                                                               o[0], o[1], o[2], *pg))
        dy = torch.empty(M, 64, device=dev)

        def unfused():
            K.dense_fwd(dgi, P[0], None, dy, trans_w=True)
            K.ln_relu_bwd(A[3], A[4], A[5], P[3], dy, o[0], pg[0], pg[1])
            K.dense_fwd(o[0], P[1], None, dy, trans_w=True)
            K.ln_relu_bwd(A[0], A[1], A[2], P[4], dy, o[1], pg[2], pg[3])
            K.dense_fwd(o[1], P[2], None, o[2], trans_w=True, relu_mask=mask)
        timeit(f"mlp bwd chain unfused (5 launches) M={M}", unfused)
if which in ("all", "trunkw"):
    # the trunk backward with its two weight gradients: mlp_gi_bwd + 2 x dense_bwd_w (dpre2 / dpre1 through HBM) against the one
    # mlp_gi_bwd_w launch; either way inside a BwdWBatch, so the time includes one batched slab-reduce launch.  Three repeats,
    # alternating; `vl` is the pooled-rows form (separate x, no mask)
    for M, vl in ((131072, False), (16384, True), (16384, False)):
        P = [torch.randn(*s_, device=dev) * 0.1 for s_ in ((64, 192), (64, 64), (64, 64), (64,), (64,))]
        dgi = torch.randn(M, 192, device=dev)
        A = [torch.randn(M, w, device=dev) for w in (64, 64, 2, 64, 64, 2)]
        x = torch.randn(M, 64, device=dev)
        mask = None if vl else x
        o = [torch.empty(M, 64, device=dev) for _ in range(3)]
        pg = [torch.zeros(64, device=dev) for _ in range(4)]
        dW = [torch.zeros(64, 64, device=dev), torch.zeros(64, device=dev), torch.zeros(64, 64, device=dev), torch.zeros(64, device=dev)]
        wsbuf = torch.empty(16 << 20, device=dev)

        def parent():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                K.mlp_gi_bwd(dgi, P[0], P[1], P[2], P[3], P[4], A[3], A[4], A[5], A[0], A[1], A[2], mask, o[0], o[1], o[2], *pg)
                K.dense_bwd_w(A[1], o[0], dW[0], dW[1])
                K.dense_bwd_w(x, o[1], dW[2], dW[3])

        def fused():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                K.mlp_gi_bwd_w(dgi, P[0], P[1], P[2], P[3], P[4], A[3], A[4], A[5], A[0], A[1], A[2], x, mask, o[2], *pg, *dW)
        for rep in range(3):
            timeit(f"trunk bwd: mlp_gi_bwd + 2 dense_bwd_w M={M} vl={int(vl)}", parent, iters=50)
            timeit(f"trunk bwd: mlp_gi_bwd_w M={M} vl={int(vl)}", fused, iters=50)
if which in ("all", "headb"):
    # the head backward: dense_bwd_w, dense_fwd^T, dense_bwd_w, dense_fwd^T (policy, n_out = 4) or the first two (values,
    # n_out = 1 / 2) against the one head_bwd launch; inside a BwdWBatch as above.  Three repeats, alternating
    for M, n_out, two in ((131072, 4, True), (131072, 2, False), (16384, 4, True), (16384, 1, False)):
        feat = torch.randn(M, 64, device=dev); u = torch.randn(M, 64, device=dev); dout = torch.randn(M, n_out, device=dev)
        W1 = torch.randn(64, 64 if two else n_out, device=dev) * 0.1; W2 = torch.randn(64, n_out, device=dev) * 0.1
        dW1 = torch.zeros_like(W1); db1 = torch.zeros(W1.shape[1], device=dev)
        dW2 = torch.zeros_like(W2); db2 = torch.zeros(n_out, device=dev)
        du = torch.empty(M, 64, device=dev); dhs = torch.empty(M, 64, device=dev)
        wsbuf = torch.empty(16 << 20, device=dev)

        def parent():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                if two:
                    K.dense_bwd_w(u, dout, dW2, db2)
                    K.dense_fwd(dout, W2, None, du, trans_w=True)
                    K.dense_bwd_w(feat, du, dW1, db1)
                    K.dense_fwd(du, W1, None, dhs, trans_w=True)
                else:
                    K.dense_bwd_w(feat, dout, dW1, db1)
                    K.dense_fwd(dout, W1, None, dhs, trans_w=True)

        def fused():
            with K.BwdWBatch(dev, lambda n: wsbuf):
                if two:
                    K.head_bwd(feat, u, dout, W1, W2, dhs, dW1, db1, dW2, db2)
                else:
                    K.head_bwd(feat, None, dout, W1, None, dhs, dW1, db1)
        for rep in range(3):
            timeit(f"head bwd: {4 if two else 2} launches M={M} n_out={n_out}", parent, iters=50, bytes_=4.0 * M * (196 if two else 129))
            timeit(f"head bwd: head_bwd M={M} n_out={n_out}", fused, iters=50, bytes_=4.0 * M * (196 if two else 129))
if which in ("all", "tail"):
    for M, two, train in ((32768, True, False), (131072, False, True), (524288, False, False)):
        gi = torch.randn(M, 192, device=dev); h0 = torch.randn(M, 64, device=dev)
        Wh = torch.randn(64, 192, device=dev) * 0.1; bhn = torch.zeros(64, device=dev)
        n_out = 4 if two else 2
        W1 = torch.randn(64, 64 if two else n_out, device=dev) * 0.1; b1 = torch.zeros(64 if two else n_out, device=dev)
        W2 = torch.randn(64, n_out, device=dev) * 0.1 if two else None; b2 = torch.zeros(n_out, device=dev) if two else None
        hs = torch.empty(M, 64, device=dev); out = torch.empty(M, n_out, device=dev)
        hp = torch.empty(M, 64, device=dev) if train else None; gt = torch.empty(M, 256, device=dev) if train else None
        u = torch.empty(M, 64, device=dev)
        timeit(f"gru1_head_fwd fused M={M} two={two} train={train}",
               lambda: K.gru1_head_fwd(gi, Wh, bhn, h0, W1, b1, W2, b2, hs, hp, gt, u if (two and train) else None, out))

        def unfused():
            K.gru_fwd(gi, Wh, bhn, h0, hs, hp, gt, M, 1, 8)
            if two:
                K.dense_fwd(hs, W1, b1, u); K.dense_fwd(u, W2, b2, out)
            else:
                K.dense_fwd(hs, W1, b1, out)
        timeit(f"gru_fwd + dense unfused M={M} two={two} train={train}", unfused)
