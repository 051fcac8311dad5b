"""Time of the two scene-mining launches (dgppo_env_scene_mine, dgppo_env_scene_pool_push) on a real training rollout, and of a
training iteration with and without the pool (developer tool).  The rollout is the stochastic one of an untrained dgppo policy:
LidarSpread, n = 8, obs = 3, B envs, T = 128.  The launches: ITERS pushes from that record are captured into a HIP graph per
kernel pair and ROUNDS replays are timed between device events.  The iterations: the trainer's loop body (mix_assignment, collect
with the pool as scenes, push_from, update) next to the plain one (collect, update), K iterations of each after a warm-up, each
timed on the host around a device sync; medians.
Usage:  python tools/bench_scene_mine.py [B] [iters] [rounds] [K]   (default 4096 envs, 200 launches per replay, 7 rounds, 12)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgppo_amd.algo import make_algo  # noqa: E402
from dgppo_amd.env import ScenePool, make_env  # noqa: E402
from dgppo_amd.env.scenes import mix_assignment  # noqa: E402
from dgppo_amd import ops_env as OE  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
K = int(sys.argv[4]) if len(sys.argv) > 4 else 12
M, FRAC, BACK, N_AGENTS, N_OBS = 256, 0.25, 8, 8, 3

env = make_env(env_id="LidarSpread", num_agents=N_AGENTS, num_obs=N_OBS)
algo = make_algo(algo="dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                 action_dim=env.action_dim, n_agents=env.num_agents, seed=0, train_steps=1000, batch_size=16384)
rng = np.random.default_rng(5)
keys = lambda: rng.integers(1, 2 ** 62, size=B)
stat = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))

# ---- the two launches on one record -------------------------------------------------------------------------------------------
ro = algo.collect(None, keys())
rec = algo.rollout_record(ro)
pool = ScenePool(env, M)
mined = OE.alloc_mined(env.cfg, B, rec.agent_tm.device)


def mine():
    OE.scene_mine(env.cfg, rec.agent_tm, rec.cost_tm, rec.goal, rec.obst, BACK, 1e-6, mined)


def push():
    OE.scene_pool_push(env.cfg, mined, pool.dev, 0, pool.state)


mine(), push()
torch.cuda.synchronize()
first = mined["first"].cpu().numpy()
counts = dict(unsafe_envs=int((first >= 0).sum()), unsafe_at_start=int((first == 0).sum()), taken=pool.fill()[2],
              mean_first=round(float(first[first >= 0].mean()), 2) if (first >= 0).any() else None)
us = {}
for name, fn in (("scene_mine", mine), ("scene_pool_push", push)):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / ITERS)
    us[name] = stat(ts)
algo.update(ro, 0)


# ---- the iteration ---------------------------------------------------------------------------------------------------------------
def iteration(step, mining):
    torch.cuda.synchronize()
    t = time.perf_counter()
    if mining:
        of = mix_assignment(B, int(np.floor(FRAC * B + 0.5)), M, step, 0, B)
        r = algo.collect(None, keys(), scenes=pool, jitter=0.0, scene_of=of)
        pool.push_from(algo.rollout_record(r), BACK, 1e-6)
    else:
        r = algo.collect(None, keys())
    info = algo.update(r, step)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), info


ms = {}
for mining in (False, True, False, True):
    for w in range(3):
        iteration(w, mining)
    ms.setdefault("mining" if mining else "plain", []).extend(iteration(3 + k, mining)[0] for k in range(K))
_, info = iteration(99, True)
print(json.dumps(dict(B=B, T=int(rec.T), n_agents=N_AGENTS, n_obs=N_OBS, pool=M, scene_frac=FRAC, back=BACK, iters=ITERS, rounds=ROUNDS,
                      device=torch.cuda.get_device_name(0), record=counts, launch_us=us,
                      iteration_ms={k: stat(v) for k, v in ms.items()},
                      pool_keys={k: v for k, v in info.items() if k.startswith("rollout/")})))
