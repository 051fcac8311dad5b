#!/usr/bin/env python
"""Times the barrier shield at LidarSpread n = 8, obs = 3, B = 32, an 8 x 8 action grid (P = 65 candidates per agent,
B * n * P = 16 640 what-if graphs per step):

  1. the features of one step:
     (A) one dgppo_graph_feats_team_action_sweep launch;
     (B) the same features from the entry point that existed before it: per (env, agent) one dgppo_graph_feats_action_sweep
         launch on the two-frame record [state_t, next] for the grid and one 1 x 1 launch for the policy's own action, written
         into the same slices — 2 * B * n launches.  The two-frame records and the device frame numbers are prepared outside
         the timing, which favours (B).
     Before timing, (A)'s four outputs are compared with (B)'s word for word.  A and B alternate within one process.
  2. Engine.rollout_shielded against Engine.rollout(seeds, False) at the same shape, T = 128, alternating; the shielded
     rollout is split with device events into policy + Vh_t, provisional step + carry, features, Vh forward, select and the
     second step.

Device events, 5 repeats after a warm-up.  Writes profiles/shield.json.

  python tools/bench_shield.py [--repeats 5] [--grid 8] [--steps 128] [--out profiles/shield.json]"""
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
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shield.json"))
    args = ap.parse_args()
    from dgppo_amd import _native as N, engine as EN, init, nets, ops_env as OE, ops_nn as K
    dev = torch.device("cuda:0")
    n, n_obs, T, g, B = 8, 3, args.steps, args.grid, args.envs
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs)
    eng = EN.Engine(cfg, EN.Hyper(batch_size=1024), dev, T=T)
    eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
    eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
    eng.Vh.load_tree(init.init_value(0, cfg.node_dim, 2, 1, 3))
    sd, k, S = cfg.state_dim, cfg.top_k, cfg.fan_in
    n_other, Fp = cfg.num_nodes - 1 - n, nets.input_width(cfg)
    us = vs = np.linspace(-1.0, 1.0, g).astype(np.float32)
    dus, dvs = K.sweep_axis(us, "us", dev), K.sweep_axis(vs, "vs", dev)
    P = 1 + g * g
    G = B * n * P
    bytes_per_graph = 4 * (n * Fp + n_other * Fp + n * S * 4 + n * S)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)

    # ---- 1. the features of one step ----
    st0 = OE.State.empty(cfg, B, dev)
    OE.reset(cfg, seeds, st0)
    a_pol = (torch.rand(B, n, 2, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2).to(dev)     # some outside the box
    st1 = st0.like()
    OE.step(cfg, st0, a_pol, st1, torch.empty(B, device=dev), torch.empty(B, n, cfg.n_cost, device=dev))
    mk = lambda: dict(Xa=torch.empty(G * n, Fp, device=dev), Xo=torch.empty(G * n_other, Fp, device=dev),
                      ef=torch.empty(G * n, S, 4, device=dev), em=torch.empty(G * n, S, device=dev))
    out_a, out_b = mk(), mk()
    recs = [(torch.stack([st0.agent[e], st1.agent[e]]).contiguous(), torch.stack([st0.hits[e], st1.hits[e]]).contiguous(),
             st0.goal[e].contiguous(), st0.obst[e].contiguous()) for e in range(B)]
    pol_axes = [[(a_pol[e, i, 0:1].clone(), a_pol[e, i, 1:2].clone()) for i in range(n)] for e in range(B)]
    ids0 = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def feats_a():
        K.graph_feats_team_action_sweep(cfg, st0.agent, st1.agent, st0.goal, st0.obst, st1.hits, a_pol, dus, dvs, out_a["Xa"],
                                        out_a["Xo"], out_a["ef"], out_a["em"], Fp)

    def feats_b():
        o = out_b
        for e in range(B):
            agent, hits, goal, obst = recs[e]
            for i in range(n):
                g0 = (e * n + i) * P
                for lo, hi, u_, v_ in ((g0, g0 + 1) + pol_axes[e][i], (g0 + 1, g0 + P, dus, dvs)):
                    K.graph_feats_action_sweep(cfg, agent, n * sd, goal, obst, hits, n * k * 2, ids0, 1, i, u_, v_,
                                               o["Xa"][lo * n:hi * n], o["Xo"][lo * n_other:hi * n_other], o["ef"][lo * n:hi * n],
                                               o["em"][lo * n:hi * n], Fp, frame_max=0)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    timed(feats_a); timed(feats_b)                                          # warm-up
    differing = sum(int((out_a[key].view(torch.int32) != out_b[key].view(torch.int32)).sum()) for key in out_a)
    words = sum(v.numel() for v in out_a.values())
    if differing:
        raise SystemExit(f"(A) and (B) differ in {differing} of {words} words")
    A, Bt = [], []
    for _ in range(args.repeats):
        A.append(timed(feats_a))
        Bt.append(timed(feats_b))
    med = float(np.median(A))
    res = dict(device=torch.cuda.get_device_name(0),
               workload=dict(env="LidarSpread", n=n, obs=n_obs, B=B, T=T, grid=[g, g], candidates=P, graphs_per_step=G),
               features=dict(differing_words=differing, words=words, team_sweep_ms=spread(A), composition_ms=spread(Bt),
                             composition_launches=2 * B * n, bytes_written=G * bytes_per_graph,
                             team_sweep_GBps=G * bytes_per_graph / (med * 1e-3) / 1e9,
                             share_of_hbm_peak=G * bytes_per_graph / (med * 1e-3) / HBM_PEAK,
                             composition_over_team_sweep=float(np.median(Bt)) / med,
                             team_sweep_max_below_composition_min=max(A) < min(Bt)))

    # ---- 2. the shielded rollout against the plain deterministic one ----
    names = ("policy_and_Vh_t", "provisional_step_and_carry", "features", "Vh_forward", "select", "second_step")

    def shielded():
        ev = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.rollout_shielded(seeds, dus, dvs, events=ev)
        t1.record()
        torch.cuda.synchronize()
        assert all(len(e) == len(names) + 1 for e in ev), "one block of environments per step"
        parts = [sum(e[j].elapsed_time(e[j + 1]) for e in ev) for j in range(len(names))]
        return t0.elapsed_time(t1), parts

    plain = lambda: timed(lambda: eng.rollout(seeds, False))
    shielded(); plain()                                                      # warm-up: scratch buffers
    S_tot, S_parts, Pl = [], [], []
    for _ in range(args.repeats):
        tot, parts = shielded()
        S_tot.append(tot); S_parts.append(parts)
        Pl.append(plain())
    res["rollout"] = dict(shielded_ms=spread(S_tot), plain_deterministic_ms=spread(Pl),
                          shielded_over_plain=float(np.median(S_tot)) / float(np.median(Pl)),
                          split_ms={nm: spread([p[j] for p in S_parts]) for j, nm in enumerate(names)},
                          note="eager launches on both sides; the split is device time between events, the totals include the "
                               "host's launch gaps")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(features={k_: res["features"][k_] for k_ in ("differing_words", "team_sweep_ms", "composition_ms",
                                                                       "team_sweep_GBps", "composition_over_team_sweep",
                                                                       "team_sweep_max_below_composition_min")},
                          rollout=res["rollout"])))


if __name__ == "__main__":
    main()
