#!/usr/bin/env python
"""Times the action rollout landscape of one LidarSpread episode (n = 8, obs = 3, T = 128; by default 16 of its frames with one
agent's action swept over a 32 x 32 grid and the policy rolled until 32 further costs are known: 16 384 what-if envs, 33 env
steps each), the workload of tools/bench_rollout_landscape.py with the action swept instead of the position:

  (A) Engine.action_rollout_landscape: per sub-grid the fork (dgppo_env_action_sweep_fork) with the forced step, the policy
      steps (Engine._rollout_steps from slot 1, eager launches) and the fold (dgppo_constraint_return) with the copy into the
      result — their shares from the device events the call hands out, and the time per what-if env-step over the whole call;
  (B) Engine.rollout(seeds, False) of an engine with T = horizon + 1 at the batch of one sub-grid, eager launches as well: the
      same step kernels from reset instead of from a fork;
  (C) the fork alone against (D) its torch composition — per field index_select of the frames, expand over the grid and copy_
      into the output, plus the action write — on the same operands, alternating within the same loop.  The fork's figure is also
      given as bytes moved over time (what it writes plus the frames it reads once).

Timed with device events after a warm-up.  Writes profiles/action_rollout.json with the per-repeat times and their spread.

  python tools/bench_action_rollout.py [--repeats 5] [--grid 32] [--frames 16] [--horizon 32] [--out profiles/action_rollout.json]"""
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
    ap.add_argument("--fork-repeats", type=int, default=50)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--frames", type=int, default=16, help="frames of the episode whose actions are swept, evenly spaced")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--agent", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_rollout.json"))
    args = ap.parse_args()
    from dgppo_amd import _native as N, engine as EN, init, ops_env as OE, ops_nn as K
    dev = torch.device("cuda:0")
    n, n_obs, T, g, H, aid = 8, 3, args.steps, args.grid, args.horizon, args.agent
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs)

    def engine(T_):
        eng = EN.Engine(cfg, EN.Hyper(batch_size=1024), dev, T=T_)
        eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
        eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
        eng.Vh.load_tree(init.init_value(0, cfg.node_dim, 2, 1, 3))
        return eng
    eng, ref = engine(T), engine(H + 1)
    HC = eng.HC
    ro = eng.rollout(torch.tensor([12345], dtype=torch.int64, device=dev), False).finalize()
    frames = np.unique(np.linspace(0, T - 1, min(args.frames, T)).astype(np.int64))
    F = int(frames.size)
    lin = np.linspace(-1.0, 1.0, g).astype(np.float32)
    dus, dvs = K.sweep_axis(lin, "us", dev), K.sweep_axis(lin, "vs", dev)
    G = F * g * g
    cap = max(1, eng.prepass_graphs // (H + 2))
    Gb = min(G, max(1, cap // (g * g)) * g * g if cap >= g * g else cap)          # envs of the first (largest) sub-grid
    seeds = torch.arange(1, Gb + 1, dtype=torch.int64, device=dev) * 7919
    timed = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def run_a():
        events = []
        t0, t1 = timed()
        t0.record()
        value, worst = eng.action_rollout_landscape(ro, 0, aid, frames, dus, dvs, H, events=events)
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

    # ---- the fork alone and its torch composition, on the whole grid ----
    step = {k: v[0] for k, v in ro.step.items()}
    env = {k: v[0] for k, v in ro.env.items()}
    actions, carry = ro.actions[0], ro._rnn_em[0, 1:]
    ids_dev = torch.from_numpy(frames.astype(np.int32)).to(dev)
    ids_long = ids_dev.long()
    P = g * g
    out_c, out_d = OE.State.empty(cfg, G, dev), OE.State.empty(cfg, G, dev)
    act_c, act_d = torch.empty(G, n, 2, device=dev), torch.empty(G, n, 2, device=dev)
    car_c, car_d = torch.empty(G * n, HC, device=dev), torch.empty(G * n, HC, device=dev)
    grid_uv = torch.stack(torch.meshgrid(dvs, dus, indexing="ij")[::-1], dim=-1)        # [nv, nu, 2] = (us[iu], vs[iv])

    def fork():
        OE.action_sweep_fork(cfg, step, env, actions, ids_dev, F, aid, dus, dvs, out_c, act_c, carry, n * HC, car_c,
                             frame_max=int(frames.max()))

    def composition():
        tile = lambda src, dst: dst.view((F, P) + tuple(src.shape[1:])).copy_(
            src.index_select(0, ids_long).unsqueeze(1).expand((F, P) + tuple(src.shape[1:])))
        for k, v in step.items():
            tile(v, out_d.step[k])
        for k, v in env.items():
            out_d.env[k].copy_(v.unsqueeze(0).expand_as(out_d.env[k]))
        tile(actions, act_d)
        act_d.view(F, g, g, n, 2)[:, :, :, aid].copy_(grid_uv.unsqueeze(0).expand(F, g, g, 2))
        tile(carry, car_d.view(G, n, HC))

    def clock(fn):
        t0, t1 = timed()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    _, _, n_sub, worst = run_a()                                        # warm-up: scratch buffers, ray tables, code objects
    run_b()
    fork()
    composition()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in
               [(out_c.step[k], out_d.step[k]) for k in step] + [(out_c.env[k], out_d.env[k]) for k in env]
               + [(act_c, act_d), (car_c, car_d)])
    A, B, parts, Cf, Df = [], [], [], [], []
    for _ in range(args.repeats):
        ms, part, _, _ = run_a()
        A.append(ms)
        parts.append(part)
        B.append(run_b())
    for _ in range(args.fork_repeats):
        Cf.append(clock(fork))
        Df.append(clock(composition))
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)
    med_a, med_b = float(np.median(A)), float(np.median(B))
    fork_ms, steps_ms, fold_ms = (float(np.median([p[i] for p in parts])) for i in range(3))
    inside = fork_ms + steps_ms + fold_ms
    words = lambda d: sum(int(np.prod(v.shape[1:])) for v in d.values())
    per_env = words(out_c.step) + words(out_c.env) + n * 2 + n * HC
    per_frame = words(out_c.step) + n * 2 + n * HC
    moved = 4 * (G * per_env + F * per_frame + words(out_c.env))
    med_c, med_d = float(np.median(Cf)), float(np.median(Df))
    h = worst[:, :, :, aid, :].max(dim=-1).values
    res = dict(device=torch.cuda.get_device_name(0),
               workload=dict(env="LidarSpread", n=n, obs=n_obs, T=T, frames=F, grid=[g, g], horizon=H, agent=aid, what_if_envs=G,
                             what_if_env_steps=G * (H + 1), sub_grids=n_sub, envs_per_sub_grid=Gb,
                             fused_step=bool(eng.fused_step), launches="eager"),
               action_rollout_landscape_ms=spread(A), fork_and_forced_step_ms=fork_ms, policy_steps_ms=steps_ms, fold_ms=fold_ms,
               fork_and_forced_step_share=fork_ms / inside, policy_steps_share=steps_ms / inside, fold_share=fold_ms / inside,
               outside_the_events_ms=med_a - inside,
               ns_per_what_if_env_step=med_a * 1e6 / (G * (H + 1)),
               plain_rollout=dict(batch=Gb, T=H + 1, ms=spread(B), ns_per_env_step=med_b * 1e6 / (Gb * (H + 1))),
               landscape_over_plain_per_env_step=(med_a / (G * (H + 1))) / (med_b / (Gb * (H + 1))),
               fork=dict(ms=spread(Cf), torch_composition_ms=spread(Df), composition_over_fork=med_d / med_c,
                         same_words_as_the_composition=bool(same), bytes_moved=moved, GB_per_s=moved / (med_c * 1e-3) / 1e9,
                         hbm_peak_GB_per_s=dict(spec=8000.0, measured_float4_copy=6290.0)),
               doomed_frac=float((h >= 0).float().mean()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
