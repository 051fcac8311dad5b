#!/usr/bin/env python
"""Times the cost landscape of one LidarSpread episode (n = 8, obs = 3, T = 128, 64 x 64 grid: 524 288 points), the workload of
tools/bench_landscape.py:

  (A) Engine.cost_landscape (one dgppo_cost_sweep launch writing the result in place);
  (B) the same costs from the entry points that existed before it: the record tiled per grid point in chunks of frames, the
      agent row overwritten, ops_env.sense of all agents, ops_env.step with zero actions, its cost output kept;
  (C) dgppo_graph_feats_sweep on the same grid (the features kernel of the Vh landscape), for scale.

Before timing, (A) is compared with (B) word for word.  A, B and C alternate within one process, timed with device events after a
warm-up.  Writes profiles/landscape_cost.json: the number of differing words, per-repeat times and their spread, the bytes (A)
writes (from the shapes), the resulting GB/s and the A/B and A/C ratios.

  python tools/bench_cost_landscape.py [--repeats 5] [--grid 64] [--out profiles/landscape_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--chunk-frames", type=int, default=16, help="frames per chunk of (B) and (C)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landscape_cost.json"))
    args = ap.parse_args()
    from dgppo_amd import _native as N, engine as EN, init, nets, ops_env as OE, ops_nn as K
    dev = torch.device("cuda:0")
    n, n_obs, T, g = 8, 3, args.steps, args.grid
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs)
    eng = EN.Engine(cfg, EN.Hyper(batch_size=1024), dev, T=T)
    eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
    eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
    eng.Vh.load_tree(init.init_value(0, cfg.node_dim, 2, 1, 3))
    ro = eng.rollout(torch.tensor([12345], dtype=torch.int64, device=dev), False).finalize()
    sd, k, nc = cfg.state_dim, cfg.top_k, cfg.n_cost
    aid, frames = 0, np.arange(T)
    xs = np.linspace(0.0, cfg.area_size, g).astype(np.float32)
    ys = np.linspace(0.0, cfg.area_size, g).astype(np.float32)
    dxs, dys = K.sweep_axis(xs, "xs", dev), K.sweep_axis(ys, "ys", dev)
    G = T * g * g
    timed = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def run_a():
        t0, t1 = timed()
        t0.record()
        out = eng.cost_landscape(ro, 0, aid, frames, dxs, dys)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    agent, goal, obst = ro.agent[0], ro.goal[0], ro.obst[0]
    cf = min(args.chunk_frames, T)
    Gc = cf * g * g
    ag = torch.empty(cf, g, g, n, sd, device=dev)
    goal_t = goal.unsqueeze(0).expand(Gc, -1, -1).contiguous()            # per-env constants: tiled once, outside the timing
    obst_t = obst.unsqueeze(0).expand(Gc, -1, -1).contiguous()
    hits_t = torch.empty(Gc, n, k, 2, device=dev)
    zero_act = torch.zeros(Gc, n, 2, device=dev)
    nxt = OE.State({"agent": torch.empty(Gc, n, sd, device=dev), "hits": torch.empty(Gc, n, k, 2, device=dev)},
                   {"goal": goal_t, "obst": obst_t})
    rew = torch.empty(Gc, device=dev)
    cost_b = torch.empty(T, g, g, n, nc, device=dev)

    def run_b():
        t0, t1 = timed()
        t0.record()
        for f0 in range(0, T, cf):
            f1 = min(T, f0 + cf)
            Fb = f1 - f0
            Gb = Fb * g * g
            a = ag[:Fb]
            a.copy_(agent[f0:f1].view(Fb, 1, 1, n, sd).expand(Fb, g, g, n, sd))
            a[:, :, :, aid, 0] = dxs.view(1, 1, g)
            a[:, :, :, aid, 1] = dys.view(1, g, 1)
            st = OE.State({"agent": a.view(Gb, n, sd), "hits": hits_t[:Gb]}, {"goal": goal_t[:Gb], "obst": obst_t[:Gb]})
            OE.sense(cfg, st)
            st1 = OE.State({"agent": nxt.agent[:Gb], "hits": nxt.hits[:Gb]}, {"goal": goal_t[:Gb], "obst": obst_t[:Gb]})
            OE.step(cfg, st, zero_act[:Gb], st1, rew[:Gb], cost_b[f0:f1].view(Gb, n, nc))
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    step = {k_: v[0] for k_, v in ro.step.items()}
    env = {k_: v[0] for k_, v in ro.env.items()}
    rc, rs = OE._rays(cfg, dev)
    feats = nets.GraphFeats(cfg, Gc, eng.arena, "bench")                # (C) runs whole chunks only: T % chunk-frames == 0
    ids_dev = torch.arange(T, dtype=torch.int32, device=dev)

    def run_c():
        t0, t1 = timed()
        t0.record()
        for f0 in range(0, T, cf):
            feats.compute_sweep(step, env, ids_dev[f0:f0 + cf], cf, aid, dxs, dys, rc, rs, frame_max=f0 + cf - 1)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    _, cost_a = run_a()                                                     # warm-up: scratch buffers, ray tables
    run_b()
    if T % cf == 0:
        run_c()
    wa, wb = cost_a.view(torch.int32), cost_b.view(torch.int32)
    differing = int(((wa != wb) & ~(torch.isnan(cost_a) & torch.isnan(cost_b))).sum())     # two NaNs count as equal
    nan_same = bool(torch.equal(torch.isnan(cost_a), torch.isnan(cost_b)))
    A, B, Cc = [], [], []
    for _ in range(args.repeats):
        A.append(run_a()[0])
        B.append(run_b())
        if T % cf == 0:
            Cc.append(run_c())
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)
    med = float(np.median(A))
    written = G * n * nc * 4
    res = dict(device=torch.cuda.get_device_name(0), workload=dict(env="LidarSpread", n=n, obs=n_obs, T=T, grid=[g, g], points=G),
               differing_words=differing, words=int(wa.numel()), nan_in_the_same_places=nan_same,
               nan_words=int(torch.isnan(cost_a).sum()),
               cost_sweep_ms=spread(A), composition_ms=spread(B), composition_chunk_frames=cf,
               cost_sweep_bytes_written=written, bytes_per_point=n * nc * 4, cost_sweep_GBps=written / (med * 1e-3) / 1e9,
               composition_over_cost_sweep=float(np.median(B)) / med, cost_sweep_max_below_composition_min=max(A) < min(B))
    if Cc:
        res.update(features_sweep_ms=spread(Cc), cost_sweep_over_features_sweep=med / float(np.median(Cc)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if differing or not nan_same:
        raise SystemExit(f"(A) and (B) differ in {differing} words (NaN in the same places: {nan_same})")


if __name__ == "__main__":
    main()
