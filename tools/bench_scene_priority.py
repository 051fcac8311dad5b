"""Time of a training iteration with the scene pool as a ring and as a pool by priority (developer tool).  LidarSpread, n = 8,
obs = 3, B envs, T = 128, an untrained dgppo policy, a pool of M scenes, a quarter of the batch started in it.  The iterations are
the trainer's loop bodies — ring: mix_assignment, collect with the pool as scenes, push_from, update; priority: draw, collect with the drawn
scene_of, score_from, push_from, update — in alternating blocks of K after a warm-up, each iteration timed on the host around a
device sync.  Reported: the median of every block, the median over a mode's iterations, and the spread of the ring's block medians,
which is what the difference between the two modes has to be read against.
Usage:  python tools/bench_scene_priority.py [M] [B] [K] [blocks]   (default 256 slots, 4096 envs, 12 iterations, 3 blocks per mode)."""
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

M = int(sys.argv[1]) if len(sys.argv) > 1 else 256
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
K = int(sys.argv[3]) if len(sys.argv) > 3 else 12
BLOCKS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
FRAC, BACK, N_AGENTS, N_OBS = 0.25, 8, 8, 3
N_SCENE = int(np.floor(FRAC * B + 0.5))

env = make_env(env_id="LidarSpread", num_agents=N_AGENTS, num_obs=N_OBS)
algo = make_algo(algo="dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                 action_dim=env.action_dim, n_agents=env.num_agents, seed=0, train_steps=1000, batch_size=16384)
rng = np.random.default_rng(5)
keys = lambda: rng.integers(1, 2 ** 62, size=B)
pools = {"ring": ScenePool(env, M), "priority": ScenePool(env, M, priority=True, draw_seed=5)}


def iteration(step, mode):
    pool = pools[mode]
    torch.cuda.synchronize()
    t = time.perf_counter()
    if mode == "ring":
        of = mix_assignment(B, N_SCENE, M, step, 0, B)
        r = algo.collect(None, keys(), scenes=pool, jitter=0.0, scene_of=of)
        pool.push_from(algo.rollout_record(r), BACK, 1e-6)
    else:
        drawn = pool.draw(B, N_SCENE, step, 0, B)
        r = algo.collect(None, keys(), scenes=pool, jitter=0.0, scene_of=pool.drawn(drawn))
        rec = algo.rollout_record(r)
        mined = pool.score_from(rec, drawn, pool.mix_flags(B), step, BACK, 1e-6)
        pool.push_from(rec, BACK, 1e-6, step=step, mined=mined)
    info = algo.update(r, step)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), info


step, blocks, last = 0, {"ring": [], "priority": []}, {}
for _ in range(BLOCKS):
    for mode in ("ring", "priority"):
        for _ in range(3):
            iteration(step, mode)
            step += 1
        ts = []
        for _ in range(K):
            ms, last[mode] = iteration(step, mode)
            ts.append(ms)
            step += 1
        blocks[mode].append(ts)
med = {m: [round(float(np.median(b)), 3) for b in v] for m, v in blocks.items()}
overall = {m: round(float(np.median(np.concatenate(v))), 3) for m, v in blocks.items()}
print(json.dumps(dict(pool=M, B=B, n_agents=N_AGENTS, n_obs=N_OBS, scene_frac=FRAC, back=BACK, K=K, blocks=BLOCKS,
                      device=torch.cuda.get_device_name(0), block_median_ms=med, median_ms=overall,
                      added_ms=round(overall["priority"] - overall["ring"], 3),
                      ring_block_median_spread_ms=round(max(med["ring"]) - min(med["ring"]), 3),
                      pool_keys={m: {k: v for k, v in last[m].items() if k.startswith("rollout/")} for m in last})))
