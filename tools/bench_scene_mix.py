"""Time of dgppo_env_scene_mix with every env assigned next to dgppo_env_scene_load of the same build on the same inputs
(developer tool).  Both entry points are called through ctypes on prepared device pointers, so neither pays a binding's host
checks or copies.  Per shape: a warm-up, then ITERS launches of each kernel are captured into a HIP graph of its own (a launch
issued from Python costs more host time than the shorter kernel runs) and ROUNDS rounds alternate the two graphs; a round
times one replay between two device events and reports the time per launch.  The outputs of the two are compared word for
word on the way.
Usage:  python tools/bench_scene_mix.py [B] [iters] [rounds]   (default 4096 envs, 500 launches per replay, 7 rounds)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, ops_env as OE  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 500
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
S, JITTER = 16, 0.01
dev = torch.device("cuda:0")
lib = N.lib()
p = lambda t: C.c_void_p(t.data_ptr())


def shape(n, n_obs, area):
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, n_obs, area_size=area)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    # the templates: S scenes the reset itself sampled (valid by construction), their rectangles as (cx, cy, w, h, theta)
    t0 = OE.State.empty(cfg, S, dev)
    OE.env_reset(cfg, seeds[:S], t0.agent, t0.goal, t0.obst, n_failed)
    agent_t, goal_t, obst_t = t0.agent.clone(), t0.goal.clone(), t0.obst[..., :5].contiguous()
    ids = (torch.arange(B, dtype=torch.int32, device=dev) % S).contiguous()
    st = {k: OE.State.empty(cfg, B, dev) for k in ("load", "mix")}
    for s in st.values():                                  # the mix runs over a record that holds a reset
        OE.env_reset(cfg, seeds, s.agent, s.goal, s.obst, n_failed)
    flags = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in st}
    count = {k: torch.zeros(1, dtype=torch.int32, device=dev) for k in st}

    def launch(which):
        fn = lib.dgppo_env_scene_load if which == "load" else lib.dgppo_env_scene_mix
        s = st[which]
        rc = fn(C.byref(cfg), p(agent_t), p(goal_t), p(obst_t), S, p(ids), p(seeds), JITTER, p(s.agent), p(s.goal), p(s.obst),
                p(flags[which]), p(count[which]), B, N.stream_ptr())
        assert rc == 0, lib.dgppo_last_error()

    for which in st:
        for _ in range(20):
            launch(which)
    torch.cuda.synchronize()
    graphs = {}
    for which in st:
        graphs[which] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[which]):
            for _ in range(ITERS):
                launch(which)
        graphs[which].replay()                             # the first replay uploads the graph
    torch.cuda.synchronize()
    us = {k: [] for k in st}
    for _ in range(ROUNDS):
        for which in st:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[which].replay()
            b.record()
            torch.cuda.synchronize()
            us[which].append(a.elapsed_time(b) * 1e3 / ITERS)
    taken = flags["mix"] == 0
    same = all(torch.equal(getattr(st["load"], f)[taken].view(torch.int32), getattr(st["mix"], f)[taken].view(torch.int32))
               for f in ("agent", "goal", "obst")) and torch.equal(flags["load"], flags["mix"])
    stat = lambda v: dict(median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2), max_us=round(float(np.max(v)), 2))
    return dict(n_agents=n, n_obs=n_obs, area_size=area, scene_load=stat(us["load"]), scene_mix=stat(us["mix"]),
                load_over_mix=round(float(np.median(us["load"]) / np.median(us["mix"])), 2), envs_fallen_back=int((~taken).sum()),
                outputs_equal=bool(same), reset_failed=int(n_failed.item()))


out = dict(B=B, iters=ITERS, rounds=ROUNDS, kind="LidarSpread", scenes=S, jitter=JITTER, device=torch.cuda.get_device_name(0),
           shapes=[shape(8, 3, 1.5), shape(64, 3, 4.0)])
print(json.dumps(out))
