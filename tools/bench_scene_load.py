"""Time of dgppo_env_scene_load next to dgppo_env_reset_checked at the same shape (developer tool; device events, one launch
each, after a warm-up).  Usage:  python tools/bench_scene_load.py [B] [iters]   (default 4096 envs, 200 launches each)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd import _native as N, ops_env as OE  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda:0")
cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], 8, 3)
seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 7919
st = OE.State.empty(cfg, B, dev)
n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
flags = torch.zeros(B, dtype=torch.int32, device=dev)
# the templates: 16 scenes the reset itself sampled (valid by construction), their rectangles as (cx, cy, w, h, theta)
S = 16
t0 = OE.State.empty(cfg, S, dev)
OE.env_reset(cfg, seeds[:S], t0.agent, t0.goal, t0.obst, n_failed)
rows = {"agent": t0.agent.clone(), "goal": t0.goal.clone(), "obst": t0.obst[..., :5].contiguous()}


def timed(fn):
    for _ in range(10):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=round(float(np.median(us)), 2), min_us=round(float(us.min()), 2), max_us=round(float(us.max()), 2))


out = dict(B=B, iters=ITERS, kind="LidarSpread", n_agents=8, n_obs=3, scenes=S,
           reset_checked=timed(lambda: OE.env_reset(cfg, seeds, st.agent, st.goal, st.obst, n_failed)),
           scene_load=timed(lambda: OE.scene_load(cfg, rows, None, None, 0.0, st, flags)),
           scene_load_jitter=timed(lambda: OE.scene_load(cfg, rows, None, seeds, 0.01, st, flags, n_failed)))
torch.cuda.synchronize()
out["failed"] = int(n_failed.item())
print(json.dumps(out))
