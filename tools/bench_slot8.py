"""Developer tool: per-call time of the first-layer (slot-sparse) attention kernels with and without their redundant operands:
the general entry points (dgppo_attn_fwd / _bwd: efeat read, weights saved and read back) against dgppo_attn_fwd_rows / _bwd_rows
(edge features subtracted from the node rows, weights formed again in the backward).  Each variant is captured into a HIP graph of
ITERS calls and replayed; the variants alternate, REPS repeats in one process.  The calls of a graph walk over SETS copies of the
operands (about 1 GB in all, at most 8), so that a call does not find its operands in the last-level cache because the call
before it left them there; --sets 1 is what a rollout does, which reuses one set of buffers step after step.
LidarSpread n = 8, 3 obstacles; the features come from dgppo_graph_feats on reset states.

    python3 tools/bench_slot8.py [--G 4096 16384 528384] [--sets N] [--out FILE]
    python3 tools/bench_slot8.py --G 16384 --eager      one eager call per variant, in the order printed (for rocprofv3 --pmc)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, nets, ops_env as OE, ops_nn as K  # noqa: E402

ITERS, REPS, F, H, KP = 100, 3, 8, 3, 48
BYTES_PER_GRAPH = 13400          # every operand and output of all variants, LidarSpread 8 / 3


def operand_set(cfg, G, dev, seed):
    n, S = cfg.n_agents, cfg.fan_in
    R = G * n
    st = OE.State.empty(cfg, G, dev)
    OE.reset(cfg, torch.arange(1, G + 1, dtype=torch.int64, device=dev) * 7919 + seed, st)
    f = nets.GraphFeats(cfg, G, nets.Arena(dev), "b").compute_record(st.step, 1, st.env, None, G, 1)
    g = torch.Generator(device=dev).manual_seed(seed)
    return dict(f=f, qt=torch.randn(R, H * F, device=dev, generator=g), dz=torch.randn(R, KP, device=dev, generator=g),
                z=torch.empty(R, KP, device=dev), at=torch.empty(R, S, H, device=dev), dq=torch.empty(R, H * F, device=dev))


def variants(cfg, G):
    def xo(o):
        return o["f"].Xo if o["f"].n_other > 0 else None

    def fwd(o, rows, train):
        f = o["f"]
        if rows:
            K.attn_fwd_rows(cfg, F, H, KP, o["qt"], f.Xa, xo(o), f.emask, o["z"], o["at"] if train else None, G)
        else:
            K.attn_fwd(cfg, F, H, KP, o["qt"], f.Xa, xo(o), f.efeat, f.emask, o["z"], o["at"] if train else None, G)

    def bwd(o, rows, recomp):
        f = o["f"]
        if rows:
            K.attn_bwd_rows(cfg, F, H, KP, o["dz"], None if recomp else o["at"], o["qt"], f.emask, f.Xa, xo(o), o["dq"], G)
        else:
            K.attn_bwd(cfg, F, H, KP, o["dz"], o["at"], o["qt"], f.Xa, xo(o), f.efeat, o["dq"], None, None, G)

    return {
        "inference forward, efeat read": lambda o: fwd(o, False, False),
        "training forward, efeat read, weights written": lambda o: fwd(o, False, True),
        "forward, edges from rows (both uses)": lambda o: fwd(o, True, False),
        "forward, edges from rows, weights written": lambda o: fwd(o, True, True),
        "backward, efeat and weights read": lambda o: bwd(o, False, False),
        "backward, edges from rows, weights read": lambda o: bwd(o, True, False),
        "backward, edges from rows, weights formed again": lambda o: bwd(o, True, True),
    }


def capture(fn, sets):
    for o in sets:
        fn(o)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for i in range(ITERS):
            fn(sets[i % len(sets)])
    graph.replay()
    torch.cuda.synchronize()
    return graph


def time_us(graph):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, nargs="+", default=[4096, 16384, 528384])
    ap.add_argument("--sets", type=int, default=0, help="operand sets a graph walks over (0: about 1 GB in all, 1..8)")
    ap.add_argument("--eager", action="store_true", help="one eager call per variant instead of the timed graphs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 8, 3)
    assert K.attn_rows_supported(cfg, F, H)
    lines = [f"{torch.cuda.get_device_name(0)}: us per call, HIP graph of {ITERS} calls, {REPS} alternating repeats"]
    for G in a.G:
        n_sets = a.sets if a.sets > 0 else max(1, min(8, (1 << 30) // (G * BYTES_PER_GRAPH)))
        sets = [operand_set(cfg, G, dev, s) for s in range(1 if a.eager else n_sets)]
        for o in sets:                      # saved weights for the backward variants that read them
            K.attn_fwd(cfg, F, H, KP, o["qt"], o["f"].Xa, o["f"].Xo, o["f"].efeat, o["f"].emask, o["z"], o["at"], G)
        torch.cuda.synchronize()
        vs = variants(cfg, G)
        if a.eager:
            lines.append(f"G = {G}: one eager call each, in this order (after one training forward that saves the weights)")
            for k, fn in vs.items():
                fn(sets[0])
                lines.append(f"  {k}")
            torch.cuda.synchronize()
            continue
        graphs = {k: capture(fn, sets) for k, fn in vs.items()}
        res = {k: [] for k in graphs}
        for _ in range(REPS):
            for k, g in graphs.items():
                res[k].append(time_us(g))
        lines.append(f"G = {G} graphs, {len(sets)} operand set(s)")
        for k, v in res.items():
            lines.append(f"  {k:52s} " + "  ".join(f"{x:8.2f}" for x in v) + f"   spread {max(v) - min(v):5.2f}")
        del graphs, sets
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
