#!/usr/bin/env python
"""Times the rollout landscape of one LidarSpread episode (n = 8, obs = 3, T = 128; by default 16 of its frames on a 64 x 64 grid
rolled 32 steps forward: 65 536 what-if envs, 2 097 152 what-if env-steps), the workload of tools/bench_landscape.py with a
policy rollout behind every grid point:

  (A) Engine.rollout_landscape: per sub-grid the fork (dgppo_env_sweep_fork), the horizon's steps (Engine._rollout_steps, eager
      launches) and the fold (dgppo_constraint_return) with the copy into the result — their shares from the device events the
      call hands out, and the time per what-if env-step over the whole call;
  (B) Engine.rollout(seeds, False) of an engine with T = horizon at the batch of one sub-grid, eager launches as well: the same
      step kernels from reset instead of from a fork, so A's per-env-step time against B's shows what the fork, the fold and the
      walk over the sub-grids add.

A and B alternate within one process, timed with device events after a warm-up.  Writes profiles/landscape_rollout.json with the
per-repeat times and their spread.

  python tools/bench_rollout_landscape.py [--repeats 5] [--grid 64] [--frames 16] [--horizon 32] [--out profiles/landscape_rollout.json]"""
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
    ap.add_argument("--frames", type=int, default=16, help="frames of the episode that are swept, evenly spaced")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landscape_rollout.json"))
    args = ap.parse_args()
    from dgppo_amd import _native as N, engine as EN, init, ops_nn as K
    dev = torch.device("cuda:0")
    n, n_obs, T, g, H = 8, 3, args.steps, args.grid, args.horizon
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs)

    def engine(T_):
        eng = EN.Engine(cfg, EN.Hyper(batch_size=1024), dev, T=T_)
        eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
        eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
        eng.Vh.load_tree(init.init_value(0, cfg.node_dim, 2, 1, 3))
        return eng
    eng, ref = engine(T), engine(H)
    ro = eng.rollout(torch.tensor([12345], dtype=torch.int64, device=dev), False).finalize()
    frames = np.unique(np.linspace(0, T - 1, min(args.frames, T)).astype(np.int64))
    F = int(frames.size)
    dxs = K.sweep_axis(np.linspace(0.0, cfg.area_size, g).astype(np.float32), "xs", dev)
    dys = K.sweep_axis(np.linspace(0.0, cfg.area_size, g).astype(np.float32), "ys", dev)
    G = F * g * g
    cap = max(1, eng.prepass_graphs // (H + 1))
    Gb = min(G, max(1, cap // (g * g)) * g * g if cap >= g * g else cap)          # envs of the first (largest) sub-grid
    seeds = torch.arange(1, Gb + 1, dtype=torch.int64, device=dev) * 7919
    timed = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def run_a():
        events = []
        t0, t1 = timed()
        t0.record()
        value, worst = eng.rollout_landscape(ro, 0, 0, frames, dxs, dys, H, events=events)
        t1.record()
        torch.cuda.synchronize()
        part = [sum(ev[i].elapsed_time(ev[i + 1]) for ev in events) for i in range(3)]
        return t0.elapsed_time(t1), part, len(events), worst

    def run_b():
        t0, t1 = timed()
        t0.record()
        ref.rollout(seeds, False)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    _, _, n_sub, worst = run_a()                                        # warm-up: scratch buffers, ray tables, code objects
    run_b()
    A, B, parts = [], [], []
    for _ in range(args.repeats):
        ms, part, _, _ = run_a()
        A.append(ms)
        parts.append(part)
        B.append(run_b())
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)
    med_a, med_b = float(np.median(A)), float(np.median(B))
    fork, steps, fold = (float(np.median([p[i] for p in parts])) for i in range(3))
    inside = fork + steps + fold
    h = worst[:, :, :, 0, :].max(dim=-1).values
    res = dict(device=torch.cuda.get_device_name(0),
               workload=dict(env="LidarSpread", n=n, obs=n_obs, T=T, frames=F, grid=[g, g], horizon=H, what_if_envs=G,
                             what_if_env_steps=G * H, sub_grids=n_sub, envs_per_sub_grid=Gb, fused_step=bool(eng.fused_step),
                             launches="eager"),
               rollout_landscape_ms=spread(A), fork_ms=fork, steps_ms=steps, fold_ms=fold,
               fork_share=fork / inside, steps_share=steps / inside, fold_share=fold / inside,
               outside_the_events_ms=med_a - inside,
               ns_per_what_if_env_step=med_a * 1e6 / (G * H),
               plain_rollout=dict(batch=Gb, T=H, ms=spread(B), ns_per_env_step=med_b * 1e6 / (Gb * H)),
               landscape_over_plain_per_env_step=(med_a / (G * H)) / (med_b / (Gb * H)),
               doomed_frac=float((h >= 0).float().mean()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
