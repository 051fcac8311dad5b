#!/usr/bin/env python
"""Times the lookahead shield at LidarSpread n = 8, obs = 3, B = 32, an 8 x 8 action grid (P = 65 candidates per agent,
G = B * n * P = 16 640 what-if envs per step), horizons H = 8 and 16:

  1. the fork of one step:
     (A) one dgppo_env_team_action_fork launch;
     (B) the same outputs composed in torch: one expand / copy_ per field (agent, goal, obst, hits, carry, action) and one
         strided copy_ of the grid per agent for the candidate rows — 6 + n launches.
     Before timing, every output of (A) is compared with (B)'s word for word.  A and B alternate within one process.
  2. the selection on a rolled block record, per horizon:
     (A) one dgppo_lookahead_select launch;
     (B) dgppo_constraint_return over every row of the what-if envs, the own-row gather and the maximum over the components
         in torch (device time), then the copy to the host and the selection rule in NumPy (host time).
     Before timing, s / index / flag / action of (A) are compared with (B)'s.
  3. Engine.rollout_lookahead_shielded against Engine.rollout(seeds, False) at the same shape, alternating, per horizon; the
     shielded rollout is split with device events into policy forward, fork + forced step, policy steps, select and the step
     that counts, per step of the episode.

  4. with --rounds R >= 2 (Engine.lookahead_select_rounds): part 3's total again with rollout_lookahead_shielded(rounds=R) at
     --margin, alternating with the rollout without rounds at the same margin: ms per real step of both, the rounds a step
     used and what `joint` says.  The blocks of a round vary with the active list, so there is no split by events.

Device events, --repeats repeats after a warm-up; median and spread.  Writes profiles/lookahead_shield.json.

  python tools/bench_lookahead_shield.py [--repeats 5] [--grid 8] [--steps 16] [--horizons 8 16] [--rounds 1] [--margin 0]
                                         [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12            # B/s, MI355X datasheet
f32 = np.float32


def rule_np(s, a_pol, us, vs, margin):
    """the selection rule of dgppo_shield_select / dgppo_lookahead_select on s [R, P], a_pol [R, 2], vectorised over the rows"""
    clip = lambda a: np.minimum(np.maximum(a, f32(-1)), f32(1)).astype(f32)
    grid = np.stack(np.meshgrid(us, vs), axis=-1).reshape(-1, 2).astype(f32)
    cand = clip(np.concatenate([a_pol[:, None, :], np.broadcast_to(grid, (a_pol.shape[0],) + grid.shape)], axis=1))
    with np.errstate(invalid="ignore"):
        adm = s <= f32(-f32(margin))
    du, dv = cand[..., 0] - cand[:, :1, 0], cand[..., 1] - cand[:, :1, 1]
    d = ((du * du).astype(f32) + (dv * dv).astype(f32)).astype(f32)
    d = np.where(adm & ~np.isnan(d), d, f32(np.inf))
    nearest = d.argmin(axis=1)                                           # first occurrence: lowest index on ties
    fin = np.where(np.isnan(s), f32(np.inf), s)
    least = np.where(np.isnan(s).all(axis=1), 0, fin.argmin(axis=1))
    index = np.where(adm[:, 0], 0, np.where(adm.any(axis=1), nearest, least)).astype(np.int32)
    flag = np.where(adm[:, 0], 0, np.where(adm.any(axis=1), 1, 2)).astype(np.int32)
    return index, flag, cand[np.arange(s.shape[0]), index]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--horizons", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--margin", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead_shield.json"))
    args = ap.parse_args()
    from dgppo_amd import _native as N, engine as EN, init, ops_algo as OA, ops_env as OE, ops_nn as K
    dev = torch.device("cuda:0")
    n, n_obs, T, g, B = 8, 3, args.steps, args.grid, args.envs
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs)
    eng = EN.Engine(cfg, EN.Hyper(batch_size=1024), dev, T=T)
    eng.policy.load_tree(init.init_policy(0, cfg.node_dim, 2, 2))
    eng.Vl.load_tree(init.init_value(0, cfg.node_dim, 1, 2, 2))
    eng.Vh.load_tree(init.init_value(0, cfg.node_dim, 2, 1, 3))
    nh, HC = cfg.n_cost, eng.HC
    us = vs = np.linspace(-1.0, 1.0, g).astype(f32)
    dus, dvs = K.sweep_axis(us, "us", dev), K.sweep_axis(vs, "vs", dev)
    P = 1 + g * g
    G = B * n * P
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919
    spread = lambda v: dict(min=min(v), median=float(np.median(v)), max=max(v), all=v)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    # ---- 1. the fork of one step ----
    st = OE.State.empty(cfg, B, dev)
    OE.reset(cfg, seeds, st)
    a_pol = (torch.rand(B, n, 2, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2).to(dev)     # some outside the box
    carry = torch.randn(B * n, HC, generator=torch.Generator().manual_seed(4)).to(dev)
    mk = lambda: (OE.State.empty(cfg, G, dev), torch.empty(G, n, 2, device=dev), torch.empty(G * n, HC, device=dev))
    out_a, out_b = mk(), mk()
    grid_dev = torch.stack(torch.meshgrid(dvs, dus, indexing="ij"), dim=-1).flip(-1).reshape(g * g, 2).contiguous()   # (us[iu], vs[iv])

    def fork_a():
        OE.team_action_fork(cfg, st, a_pol, dus, dvs, out_a[0], out_a[1], carry, out_a[2])

    def fork_b():
        o, act, co = out_b
        for src, dst in ((st.step, o.step), (st.env, o.env)):
            for key, x in src.items():
                dst[key].view((B, n * P) + x.shape[1:]).copy_(x.unsqueeze(1).expand((B, n * P) + x.shape[1:]))
        co.view(B, n * P, n, HC).copy_(carry.view(B, 1, n, HC).expand(B, n * P, n, HC))
        a5 = act.view(B, n, P, n, 2)
        a5.copy_(a_pol.view(B, 1, 1, n, 2).expand(B, n, P, n, 2))
        for i in range(n):
            a5[:, i, 1:, i, :].copy_(grid_dev.unsqueeze(0).expand(B, g * g, 2))

    timed(fork_a); timed(fork_b)                                            # warm-up
    pairs = [(out_a[0].step[k_], out_b[0].step[k_]) for k_ in out_a[0].step] + \
            [(out_a[0].env[k_], out_b[0].env[k_]) for k_ in out_a[0].env] + [(out_a[1], out_b[1]), (out_a[2], out_b[2])]
    differing = sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in pairs)
    words = sum(x.numel() for x, _ in pairs)
    if differing:
        raise SystemExit(f"fork: (A) and (B) differ in {differing} of {words} words")
    A, Bt = [], []
    for _ in range(args.repeats):
        A.append(timed(fork_a))
        Bt.append(timed(fork_b))
    med = float(np.median(A))
    res = dict(device=torch.cuda.get_device_name(0),
               workload=dict(env="LidarSpread", n=n, obs=n_obs, B=B, T=T, grid=[g, g], candidates=P, envs_per_step=G, HC=HC,
                             horizons=args.horizons),
               fork=dict(differing_words=differing, words=words, kernel_ms=spread(A), composition_ms=spread(Bt),
                         composition_launches=len(pairs) + n, bytes_written=4 * words, kernel_GBps=4 * words / (med * 1e-3) / 1e9,
                         share_of_hbm_peak=4 * words / (med * 1e-3) / HBM_PEAK, composition_over_kernel=float(np.median(Bt)) / med,
                         kernel_max_below_composition_min=max(A) < min(Bt)))

    # ---- 2. and 3. per horizon ----
    names = ("policy_forward", "fork_and_forced_step", "policy_steps", "select", "final_step")
    plain = lambda: timed(lambda: eng.rollout(seeds, False))
    res["select"], res["rollout"], res["rounds"] = {}, {}, {}
    for H in args.horizons:
        # a block record as one real step leaves it
        recs = []
        act = dict(action=torch.empty(B, n, 2, device=dev), index=torch.empty(B, n, dtype=torch.int32, device=dev),
                   flag=torch.empty(B, n, dtype=torch.int32, device=dev), s=torch.empty(B, n, P, device=dev))
        eng.lookahead_select(st, carry, a_pol, dus, dvs, H, 0.0, act["action"], act["index"], act["flag"], act["s"], records=recs)
        cost_tm = recs[0][3].cost_tm[1:H + 1]
        val, wor = torch.empty(G, n, nh, device=dev), torch.empty(G, n, nh, device=dev)
        own = torch.arange(n, device=dev).view(1, n, 1, 1, 1).expand(B, n, P, 1, nh)
        s_b = torch.empty(B, n, P, device=dev)

        def sel_a():
            K.lookahead_select(cost_tm, a_pol, dus, dvs, 0.0, act["action"], act["index"], act["flag"], act["s"])

        def sel_b_device():
            OA.constraint_return(cost_tm, eng.hp.gamma, val, wor)
            s_b.copy_(wor.view(B, n, P, n, nh).gather(3, own).squeeze(3).amax(dim=-1))

        def sel_b_host():
            t0 = time.perf_counter()
            out = rule_np(s_b.cpu().numpy().reshape(B * n, P), a_pol.cpu().numpy().reshape(B * n, 2), us, vs, 0.0)
            return (time.perf_counter() - t0) * 1e3, out

        timed(sel_a); timed(sel_b_device)
        _, (bi, bf, ba) = sel_b_host()
        same = (torch.equal(act["s"], s_b) and np.array_equal(act["index"].cpu().numpy().reshape(-1), bi)
                and np.array_equal(act["flag"].cpu().numpy().reshape(-1), bf)
                and np.array_equal(act["action"].cpu().numpy().reshape(-1, 2), ba))
        if not same:
            raise SystemExit(f"select, H = {H}: (A) and (B) differ")
        A, Bd, Bh = [], [], []
        for _ in range(args.repeats):
            A.append(timed(sel_a))
            Bd.append(timed(sel_b_device))
            Bh.append(sel_b_host()[0])
        med = float(np.median(A))
        flags = np.bincount(bf, minlength=3).tolist()
        res["select"][f"H{H}"] = dict(
            agrees=same, flags_kept_replaced_infeasible=flags, kernel_ms=spread(A), composition_device_ms=spread(Bd),
            composition_host_ms=spread(Bh), words_needed=B * n * P * H * nh, words_of_the_full_fold=G * n * H * nh,
            composition_device_over_kernel=float(np.median(Bd)) / med,
            composition_over_kernel=(float(np.median(Bd)) + float(np.median(Bh))) / med,
            kernel_max_below_composition_device_min=max(A) < min(Bd))

        def shielded():
            ev = []
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            eng.rollout_lookahead_shielded(seeds, dus, dvs, H, events=ev)
            t1.record()
            torch.cuda.synchronize()
            assert all(len(e) == len(names) + 1 for e in ev), "one block of environments per step"
            return t0.elapsed_time(t1), [[e[j].elapsed_time(e[j + 1]) for e in ev] for j in range(len(names))]

        shielded(); plain()                                                  # warm-up: scratch buffers and block records
        S_tot, S_parts, Pl = [], [], []
        for _ in range(args.repeats):
            tot, parts = shielded()
            S_tot.append(tot); S_parts.append(parts)
            Pl.append(plain())
        # per step of the episode: the median over the steps of one rollout, then its spread over the repeats
        per_step = {nm: spread([float(np.median(p[j])) for p in S_parts]) for j, nm in enumerate(names)}
        res["rollout"][f"H{H}"] = dict(
            shielded_ms=spread(S_tot), plain_deterministic_ms=spread(Pl), shielded_ms_per_step=float(np.median(S_tot)) / T,
            shielded_over_plain=float(np.median(S_tot)) / float(np.median(Pl)), split_ms_per_step=per_step,
            env_steps_per_second=G * (H + 1) * T / (float(np.median(S_tot)) * 1e-3),
            note="eager launches on both sides; the split is device time between events, the totals include the host's launch "
                 "gaps")
        if args.rounds >= 2:
            def rolled(R):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                _, log = eng.rollout_lookahead_shielded(seeds, dus, dvs, H, margin=args.margin, rounds=R)
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1), log
            rolled(1); rolled(args.rounds)                                    # warm-up: the block record of the rounds
            one, many = [], []
            for _ in range(args.repeats):
                one.append(rolled(1)[0])
                ms, log = rolled(args.rounds)
                many.append(ms)
            used, joint = log["rounds_used"].cpu().numpy(), log["joint"].cpu().numpy()
            res["rounds"][f"H{H}"] = dict(
                rounds=args.rounds, margin=args.margin, without_rounds_ms=spread(one), with_rounds_ms=spread(many),
                without_rounds_ms_per_step=float(np.median(one)) / T, with_rounds_ms_per_step=float(np.median(many)) / T,
                with_over_without=float(np.median(many)) / float(np.median(one)), mean_rounds_per_env_step=float(used.mean()),
                env_rounds_per_step=float(used.sum()) / T, rounds_used_histogram=np.bincount(used.ravel(), minlength=args.rounds + 1).tolist(),
                joint_unrolled_rolled_unsafe_verified=np.bincount(joint.ravel(), minlength=3).tolist(),
                replaced_frac=float((log["index"] != 0).float().mean()),
                note="eager launches, one host sync per round but the last; totals include the host's launch gaps")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    short = lambda d_, keys: {k_: (d_[k_]["median"] if isinstance(d_[k_], dict) and "median" in d_[k_] else d_[k_]) for k_ in keys}
    print(json.dumps(dict(
        fork=short(res["fork"], ("differing_words", "kernel_ms", "composition_ms", "kernel_GBps", "composition_over_kernel")),
        select={h: short(v, ("kernel_ms", "composition_device_ms", "composition_host_ms", "composition_over_kernel"))
                for h, v in res["select"].items()},
        rollout={h: dict(short(v, ("shielded_ms", "plain_deterministic_ms", "shielded_ms_per_step")),
                         split={k_: x["median"] for k_, x in v["split_ms_per_step"].items()}) for h, v in res["rollout"].items()},
        rounds={h: {k_: x for k_, x in v.items() if not isinstance(x, (dict, str))} for h, v in res["rounds"].items()})))


if __name__ == "__main__":
    main()
