"""Developer tool: per-call time of the one-launch rollout step (dgppo_env_act_step_feats) against the four launches it
replaces (policy_head -> env_step -> graph_feats -> dense_fwd), and of the launch with one fold left out next to the stand-alone
kernels that fold would have replaced.  Each variant is captured into a HIP graph of ITERS calls (no host time between the
launches) and replayed; the variants alternate, REPS repeats in one process.  LidarSpread n = 8, 3 obstacles.

    python3 tools/bench_act_step.py [--B 4096 16384] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, nets, ops_env as OE, ops_nn as K  # noqa: E402

ITERS, REPS, FP, H = 100, 3, 8, 3


def variants(cfg, B, dev, sample):
    n = cfg.n_agents
    st = OE.State.empty(cfg, B, dev)
    OE.reset(cfg, torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919, st)
    nst = st.like()
    g = torch.Generator(device=dev).manual_seed(1)
    ms = torch.randn(B * n, 4, device=dev, generator=g)
    eps = torch.randn(B * n, 2, device=dev, generator=g) if sample else None
    Mcat, cvec = torch.randn(FP, H * FP, device=dev, generator=g), torch.randn(H * FP, device=dev, generator=g)
    act, lp = torch.empty(B, n, 2, device=dev), torch.empty(B, n, device=dev)
    rew, cost, qt = torch.empty(B, device=dev), torch.empty(B, n, 2, device=dev), torch.empty(B * n, H * FP, device=dev)
    feats = nets.GraphFeats(cfg, B, nets.Arena(dev), "b")
    fk = dict(Xa=feats.Xa, Xo=feats.Xo, efeat=feats.efeat, emask=feats.emask, Fp=FP)
    qk = dict(Mcat=Mcat, cvec=cvec, qt0=qt, H=H)

    def head():
        if sample:
            K.policy_head(ms, eps, None, act.view(B * n, 2), lp.view(B * n), None, n, 0)
        else:
            K.policy_head(ms, None, None, act.view(B * n, 2), None, None, n, 1)

    def gfeats():
        feats.compute_record(nst.step, 1, nst.env, None, B, 1)

    def dense():
        K.dense_fwd(feats.Xa, Mcat, cvec, qt)

    def fused(**kw):
        OE.act_step_feats(cfg, st, ms, eps, act, lp if sample else None, nst, rew, cost, **kw)

    def four():
        head(); OE.step(cfg, st, act, nst, rew, cost); gfeats(); dense()

    return {
        "four launches": four,
        "one launch": lambda: fused(**fk, **qk),
        "one launch without qt0 + dense_fwd": lambda: (fused(**fk), dense()),
        "one launch without features + graph_feats + dense_fwd": lambda: (fused(), gfeats(), dense()),
    }


def capture(fn):
    fn()                                   # eager once: sizes buffers, builds the ray tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(ITERS):
            fn()
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
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 8, 3)
    assert OE.act_step_feats_supported(cfg, FP, H)
    lines = [f"{torch.cuda.get_device_name(0)}: us per rollout step (env part), HIP graph of {ITERS} calls, {REPS} alternating repeats"]
    for B in a.B:
        for sample in (True, False):
            graphs = {k: capture(fn) for k, fn in variants(cfg, B, dev, sample).items()}
            res = {k: [] for k in graphs}
            for _ in range(REPS):
                for k, g in graphs.items():
                    res[k].append(time_us(g))
            lines.append(f"B = {B}, {'sample' if sample else 'mode'}")
            for k, v in res.items():
                lines.append(f"  {k:56s} " + "  ".join(f"{x:7.2f}" for x in v) + f"   spread {max(v) - min(v):5.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
