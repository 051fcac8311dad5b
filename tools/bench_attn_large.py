"""Developer micro-benchmark of the attention kernels at large team sizes (the tiled family, attn_tiled.hip), for a
`rocprofv3 --kernel-trace --stats` run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/bench_attn_large.py [manifest.json]
Launches, in this order and each `WARM + REPS` times: forward and backward at LidarSpread n = 32 (obs 3) for F = 8 (backward:
dqt only, the first layer's form) and F = 32 (backward with dXa / dXo), then the F = 32 backward at n = 17 (whole-graph VALU
kernel, the last shape that fits) and n = 18 (first tiled shape).  Prints, per entry, the event-timed mean per launch, the
bytes the call must move and their time at 8 TB/s; the manifest (label, kernel launches, bytes) lets a trace be split per
entry."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, ops_nn as K  # noqa: E402

G, H, WARM, REPS = 16384, 3, 3, 10
HBM_TBS = 8.0


def operands(cfg, F, Kp, dev):
    n, S, no = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1 - cfg.n_agents
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    em = (torch.rand(G * n, S, device=dev, generator=g) > 0.3).float()
    em[:, 0] = 1.0
    return dict(qt=r(G * n, H * F), Xa=r(G * n, F), Xo=r(G * no, F), ef=r(G * n, S, 4), em=em, dz=r(G * n, Kp),
                z=torch.empty(G * n, Kp, device=dev), at=torch.empty(G * n, S, H, device=dev), dq=torch.empty(G * n, H * F, device=dev),
                dXa=torch.empty(G * n, F, device=dev), dXo=torch.empty(G * no, F, device=dev))


def timed(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


def main():
    dev = torch.device("cuda:0")
    out = []
    for n, F, Kp, passes in ((32, 8, 48, ("fwd", "bwd_dq")), (32, 32, 144, ("fwd", "bwd")), (17, 32, 144, ("bwd",)), (18, 32, 144, ("bwd",))):
        cfg = N.make_env_cfg(0, n, 3)
        o = operands(cfg, F, Kp, dev)
        nb = lambda *ks: sum(o[k].numel() * 4 for k in ks)
        K.attn_fwd(cfg, F, H, Kp, o["qt"], o["Xa"], o["Xo"], o["ef"], o["em"], o["z"], o["at"], G)      # real weights for the backward
        for p in passes:
            if p == "fwd":
                fn = lambda: K.attn_fwd(cfg, F, H, Kp, o["qt"], o["Xa"], o["Xo"], o["ef"], o["em"], o["z"], o["at"], G)
                byts = nb("qt", "Xa", "Xo", "ef", "em", "z", "at")
            elif p == "bwd":
                fn = lambda: K.attn_bwd(cfg, F, H, Kp, o["dz"], o["at"], o["qt"], o["Xa"], o["Xo"], o["ef"], o["dq"], o["dXa"], o["dXo"], G)
                byts = nb("dz", "at", "qt", "Xa", "Xo", "ef", "dq", "dXa", "dXo")
            else:
                fn = lambda: K.attn_bwd(cfg, F, H, Kp, o["dz"], o["at"], o["qt"], o["Xa"], o["Xo"], o["ef"], o["dq"], None, None, G)
                byts = nb("dz", "at", "qt", "Xa", "Xo", "ef", "dq")
            us = timed(fn)
            row = dict(label=f"LidarSpread n={n} F={F} {p}", launches=WARM + REPS, warm=WARM, graphs=G, us_event=round(us, 1),
                       ns_per_graph=round(us * 1e3 / G, 1), bytes=byts, us_hbm=round(byts / (HBM_TBS * 1e6), 1))
            print(json.dumps(row), flush=True)
            out.append(row)
        del o
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
