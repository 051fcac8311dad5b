#!/usr/bin/env python
"""Times the Vh landscape of one LidarSpread episode (n = 8, obs = 3, T = 128, 64 x 64 grid: 524 288 graphs):

  (A) Engine.vh_landscape, split with device events into the sweep-features kernel and the Vh forward;
  (B) the same features from the entry points that existed before the sweep kernel: the record tiled per grid point, the
      agent row overwritten, ops_env.sense of all agents, ops_nn.graph_feats — in chunks of frames that fit memory.

A and B alternate within one process.  Writes profiles/landscape_sweep.json: per-repeat times, their spread, the bytes the
sweep kernel writes (from the shapes), the resulting GB/s and its share of the HBM peak.

  python tools/bench_landscape.py [--repeats 5] [--grid 64] [--out profiles/landscape_sweep.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12           # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--chunk-frames", type=int, default=16, help="frames per chunk of the composition (B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landscape_sweep.json"))
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
    sd, k, S = cfg.state_dim, cfg.top_k, cfg.fan_in
    n_other, Fp = cfg.num_nodes - 1 - n, nets.input_width(cfg)
    aid, frames = 0, np.arange(T)
    xs = np.linspace(0.0, cfg.area_size, g).astype(np.float32)
    ys = np.linspace(0.0, cfg.area_size, g).astype(np.float32)
    dxs, dys = K.sweep_axis(xs, "xs", dev), K.sweep_axis(ys, "ys", dev)
    G = T * g * g
    bytes_per_graph = 4 * (n * Fp + n_other * Fp + n * S * 4 + n * S)

    def run_a():
        ev = []
        eng.vh_landscape(ro, 0, aid, frames, dxs, dys, events=ev)
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b, _ in ev), sum(b.elapsed_time(c) for _, b, c in ev)

    agent, hits, goal, obst = ro.agent[0], ro.hits[0], ro.goal[0], ro.obst[0]
    cf = min(args.chunk_frames, T)
    Gc = cf * g * g
    buf = dict(Xa=torch.empty(Gc * n, Fp, device=dev), Xo=torch.empty(Gc * n_other, Fp, device=dev),
               ef=torch.empty(Gc * n, S, 4, device=dev), em=torch.empty(Gc * n, S, device=dev))
    ag = torch.empty(cf, g, g, n, sd, device=dev)
    goal_t = goal.unsqueeze(0).expand(Gc, -1, -1).contiguous()            # per-env constants: tiled once, outside the timing
    obst_t = obst.unsqueeze(0).expand(Gc, -1, -1).contiguous()
    hits_t = torch.empty(Gc, n, k, 2, device=dev)

    def run_b():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
            K.graph_feats(cfg, st.agent, n * sd, 0, st.goal, None, st.hits, n * k * 2, 0, None, Gb, 1, buf["Xa"][:Gb * n],
                          buf["Xo"][:Gb * n_other], buf["ef"][:Gb * n], buf["em"][:Gb * n], Fp)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    run_a(); run_b()                                                       # warm-up: scratch buffers, ray tables
    A_feat, A_vh, B_feat = [], [], []
    for _ in range(args.repeats):
        fa, va = run_a()
        A_feat.append(fa); A_vh.append(va)
        B_feat.append(run_b())
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)
    med = float(np.median(A_feat))
    res = dict(device=torch.cuda.get_device_name(0), workload=dict(env="LidarSpread", n=n, obs=n_obs, T=T, grid=[g, g], graphs=G),
               sweep_features_ms=spread(A_feat), vh_forward_ms=spread(A_vh), composition_features_ms=spread(B_feat),
               composition_chunk_frames=cf, sweep_bytes_written=G * bytes_per_graph, bytes_per_graph=bytes_per_graph,
               sweep_GBps=G * bytes_per_graph / (med * 1e-3) / 1e9,
               share_of_hbm_peak=G * bytes_per_graph / (med * 1e-3) / HBM_PEAK, hbm_peak_Bps=HBM_PEAK,
               composition_over_sweep=float(np.median(B_feat)) / med)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k_: res[k_] for k_ in ("sweep_features_ms", "vh_forward_ms", "composition_features_ms", "sweep_GBps",
                                             "share_of_hbm_peak", "composition_over_sweep")}))


if __name__ == "__main__":
    main()
