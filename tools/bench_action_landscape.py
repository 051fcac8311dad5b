#!/usr/bin/env python
"""Times the CBF action landscape of one LidarSpread episode (n = 8, obs = 3, T = 128, 32 x 32 actions: 131 072 graphs):

  (A) Engine.action_landscape, split with device events into the action-sweep features kernel
      (dgppo_graph_feats_action_sweep) and the Vh forward;
  (B) the same features from the entry points that existed before the kernel: frame t + 1 of the record (states and hits)
      tiled per grid point in chunks of frames, the agent's row overwritten with its stepped state, dgppo_graph_feats.  The
      stepped rows themselves are prepared outside the timing (ops_env.step on the tiled frame t with the grid actions), which
      favours (B).

Before timing, (A)'s four outputs are compared with (B)'s word for word, chunk by chunk.  A and B alternate within one process,
timed with device events after a warm-up.  Writes profiles/landscape_action.json: the number of differing words, per-repeat
times and their spread, the bytes the kernel writes (from the shapes), the resulting GB/s and the B/A ratio.

  python tools/bench_action_landscape.py [--repeats 5] [--grid 32] [--out profiles/landscape_action.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12            # B/s, MI355X datasheet


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--chunk-frames", type=int, default=16, help="frames per chunk of the composition (B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landscape_action.json"))
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
    sd, k, S, nc = cfg.state_dim, cfg.top_k, cfg.fan_in, cfg.n_cost
    n_other, Fp = cfg.num_nodes - 1 - n, nets.input_width(cfg)
    aid, frames = 0, np.arange(T)
    us = np.linspace(-1.0, 1.0, g).astype(np.float32)
    vs = np.linspace(-1.0, 1.0, g).astype(np.float32)
    dus, dvs = K.sweep_axis(us, "us", dev), K.sweep_axis(vs, "vs", dev)
    P = g * g
    G = T * P
    bytes_per_graph = 4 * (n * Fp + n_other * Fp + n * S * 4 + n * S)

    def run_a():
        ev = []
        eng.action_landscape(ro, 0, aid, frames, dus, dvs, events=ev)
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b, _ in ev), sum(b.elapsed_time(c) for _, b, c in ev), len(ev)

    agent, hits, goal, obst, actions = ro.agent[0], ro.hits[0], ro.goal[0], ro.obst[0], ro.actions[0]
    cf = min(args.chunk_frames, T)
    Gc = cf * P
    buf = dict(Xa=torch.empty(Gc * n, Fp, device=dev), Xo=torch.empty(Gc * n_other, Fp, device=dev),
               ef=torch.empty(Gc * n, S, 4, device=dev), em=torch.empty(Gc * n, S, device=dev))
    ag = torch.empty(cf, P, n, sd, device=dev)
    goal_t = goal.unsqueeze(0).expand(Gc, -1, -1).contiguous()            # per-env constants: tiled once, outside the timing
    obst_t = obst.unsqueeze(0).expand(Gc, -1, -1).contiguous()
    hits_t = torch.empty(cf, P, n, k, 2, device=dev)

    # the stepped rows (B) writes over the agent's: ops_env.step of frame t tiled per grid action, outside the timing
    rows = torch.empty(T, P, sd, device=dev)
    grid_act = torch.stack(torch.meshgrid(dvs, dus, indexing="ij"), dim=-1).flip(-1).reshape(P, 2)     # q = iv * g + iu -> (u, v)
    nxt = OE.State({"agent": torch.empty(Gc, n, sd, device=dev), "hits": torch.empty(Gc, n, k, 2, device=dev)},
                   {"goal": goal_t, "obst": obst_t})
    rew, cst = torch.empty(Gc, device=dev), torch.empty(Gc, n, nc, device=dev)
    for f0 in range(0, T, cf):
        f1 = min(T, f0 + cf)
        Fb = f1 - f0
        Gb = Fb * P
        a = agent[f0:f1].unsqueeze(1).expand(Fb, P, n, sd).reshape(Gb, n, sd).contiguous()
        h = hits[f0:f1].unsqueeze(1).expand(Fb, P, n, k, 2).reshape(Gb, n, k, 2).contiguous()
        act = actions[f0:f1].unsqueeze(1).expand(Fb, P, n, 2).clone()
        act[:, :, aid] = grid_act.unsqueeze(0)
        st = OE.State({"agent": a, "hits": h}, {"goal": goal_t[:Gb], "obst": obst_t[:Gb]})
        st1 = OE.State({"agent": nxt.agent[:Gb], "hits": nxt.hits[:Gb]}, {"goal": goal_t[:Gb], "obst": obst_t[:Gb]})
        OE.step(cfg, st, act.view(Gb, n, 2), st1, rew[:Gb], cst[:Gb])
        rows[f0:f1].copy_(nxt.agent[:Gb].view(Fb, P, n, sd)[:, :, aid])
    torch.cuda.synchronize()

    def compose(f0, f1):
        Fb = f1 - f0
        Gb = Fb * P
        a = ag[:Fb]
        a.copy_(agent[f0 + 1:f1 + 1].view(Fb, 1, n, sd).expand(Fb, P, n, sd))
        a[:, :, aid] = rows[f0:f1]
        ht = hits_t[:Fb]
        ht.copy_(hits[f0 + 1:f1 + 1].view(Fb, 1, n, k, 2).expand(Fb, P, n, k, 2))
        K.graph_feats(cfg, a.view(Gb, n, sd), n * sd, 0, goal_t[:Gb], None, ht.view(Gb, n, k, 2), n * k * 2, 0, None, Gb, 1,
                      buf["Xa"][:Gb * n], buf["Xo"][:Gb * n_other], buf["ef"][:Gb * n], buf["em"][:Gb * n], Fp)
        return Gb

    def run_b():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for f0 in range(0, T, cf):
            compose(f0, min(T, f0 + cf))
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    run_a(); run_b()                                                       # warm-up: scratch buffers
    # ---- (A) against (B), word for word ----
    step = {k_: v[0] for k_, v in ro.step.items()}
    env = {k_: v[0] for k_, v in ro.env.items()}
    feats = nets.GraphFeats(cfg, Gc, eng.arena, "bench")
    ids_dev = torch.arange(T, dtype=torch.int32, device=dev)
    differing = words = 0
    for f0 in range(0, T, cf):
        f1 = min(T, f0 + cf)
        Gb = compose(f0, f1)
        fa = nets.GraphFeats(cfg, Gb, eng.arena, "bench") if Gb != Gc else feats
        fa.compute_action_sweep(step, env, ids_dev[f0:f1], f1 - f0, aid, dus, dvs, frame_max=f1 - 1)
        for got, want in ((fa.Xa, buf["Xa"][:Gb * n]), (fa.Xo, buf["Xo"][:Gb * n_other]), (fa.efeat, buf["ef"][:Gb * n]),
                          (fa.emask, buf["em"][:Gb * n])):
            differing += int((got.view(torch.int32) != want.view(torch.int32)).sum())
            words += got.numel()
    if differing:
        raise SystemExit(f"(A) and (B) differ in {differing} of {words} words")

    A_feat, A_vh, B_feat, launches = [], [], [], 0
    for _ in range(args.repeats):
        fa, va, launches = run_a()
        A_feat.append(fa); A_vh.append(va)
        B_feat.append(run_b())
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)
    med = float(np.median(A_feat))
    res = dict(device=torch.cuda.get_device_name(0), workload=dict(env="LidarSpread", n=n, obs=n_obs, T=T, grid=[g, g], graphs=G),
               differing_words=differing, words=words,
               action_sweep_features_ms=spread(A_feat), action_sweep_launches=launches, vh_forward_ms=spread(A_vh),
               composition_features_ms=spread(B_feat), composition_chunk_frames=cf,
               sweep_bytes_written=G * bytes_per_graph, bytes_per_graph=bytes_per_graph,
               sweep_GBps=G * bytes_per_graph / (med * 1e-3) / 1e9,
               share_of_hbm_peak=G * bytes_per_graph / (med * 1e-3) / HBM_PEAK, hbm_peak_Bps=HBM_PEAK,
               composition_over_sweep=float(np.median(B_feat)) / med, sweep_max_below_composition_min=max(A_feat) < min(B_feat))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k_: res[k_] for k_ in ("differing_words", "action_sweep_features_ms", "vh_forward_ms",
                                             "composition_features_ms", "sweep_GBps", "share_of_hbm_peak",
                                             "composition_over_sweep", "sweep_max_below_composition_min")}))


if __name__ == "__main__":
    main()
