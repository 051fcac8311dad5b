"""Training driver with the reference's loop order and logged keys (dgppo/trainer/trainer.py:20-141):
eval -> save -> collect -> update, wandb when importable else JSONL + stdout.

Data-parallel runs (one process per GPU): `rank` / `world` are two optional constructor arguments after the
reference's.  `n_env_train` stays the GLOBAL number of training environments: every rank draws the same global key array
and rolls out its contiguous share of it, the algo (built with the same `allreduce` / `world` / `rank`) exchanges
gradients once per minibatch, and evaluation, checkpoints and logging happen on rank 0 only — the parameters are
bit-identical on every rank, so nothing is lost.

Stopped runs (not in the reference): with every weights save rank 0 also writes the whole training state to
`{log_dir}/resume/{step}.pkl`; `Trainer(..., resume=True)` loads the newest one on every rank and the loop goes on from that
step ("Resuming a stopped run").

Designed scenes (not in the reference): `Trainer(..., scenes=Scenes, scene_frac=P, scene_jitter=J)` starts
floor(P n_env_train + 0.5) envs of every training batch in the given scenes, jittered by up to J, and the rest at the sampled
reset (env.scenes.mix_assignment, a function of the global env index and the step: no new state to resume); every evaluation
also rolls each scene once.

Mined scenes (not in the reference): `Trainer(..., mine_scenes=M, mine_back=K, scene_frac=P)` keeps a device-resident pool of M
scenes (env.scenes.ScenePool; `scenes`, if given, pinned in its first slots), starts the share P of every batch in it, and after
every collect pushes the states K steps before the rollout's failures into its ring.  One rank only; the pool is part of the
state a stopped run resumes from, and every save also writes it as `{log_dir}/scenes/{step}.npz`.
`scene_priority=True` (needs mine_scenes) makes that a pool by priority (ScenePool(priority=True), csrc/env_scene_pool.hip): every
iteration draws the scene envs' slots on the device in proportion to 4 s (1 - s) of the slot's failure score s and to its
staleness, collects, mines, folds what the replays did into the scores, and pushes with eviction of solved and hopeless slots."""
from __future__ import annotations

import json
import os
from time import time

import numpy as np
import torch

from ..env.scenes import ScenePool, mix_assignment, write_npz
from ..utils import checkpoint as CK

KEEP_STATES = 2          # state files kept under {log_dir}/resume: the newest and the one before it


def no_state_error(run_dir: str) -> FileNotFoundError:
    return FileNotFoundError(f"{run_dir}: no training state to resume from (resume/flags.yaml and resume/{{step}}.pkl). Runs "
                             f"written before full-state checkpoints existed hold weights only (models/{{step}}/*.pkl): "
                             f"they can be tested, not continued.")


def scene_count(scene_frac: float, n_env_train: int) -> int:
    """envs of a training batch that start in scenes: floor(P n + 0.5)"""
    return int(np.floor(float(scene_frac) * int(n_env_train) + 0.5))


class _Logger:
    def __init__(self, log_dir, run_name, group, save_log):
        self.wandb = None
        self.path = os.path.join(log_dir, "metrics.jsonl") if save_log else None
        try:  # wandb is optional and must never touch the network here
            import wandb  # noqa: F401
            os.environ.setdefault("WANDB_MODE", "offline")
            wandb.init(name=run_name, project="dgppo", group=group, dir=log_dir)
            self.wandb = wandb
        except Exception:
            self.wandb = None

    def log(self, info: dict, step: int):
        if self.wandb is not None:
            self.wandb.log(info, step=step)
        if self.path is not None:
            with open(self.path, "a") as f:
                f.write(json.dumps({"step": step, **{k: float(v) for k, v in info.items()}}) + "\n")


class Trainer:
    def __init__(self, env, env_test, algo, gamma: float, n_env_train: int, n_env_test: int, log_dir: str, seed: int,
                 params: dict, save_log: bool = True, rank: int = 0, world: int = 1, resume: bool = False, scenes=None,
                 scene_frac: float = 0.0, scene_jitter: float = 0.0, mine_scenes: int = 0, mine_back: int = 8,
                 scene_priority: bool = False):
        self.env, self.env_test, self.algo, self.gamma = env, env_test, algo, gamma
        self.n_env_train, self.n_env_test, self.log_dir, self.seed = n_env_train, n_env_test, log_dir, seed
        self.rank, self.world = int(rank), int(world)
        assert 0 <= self.rank < self.world
        assert n_env_train % self.world == 0, f"n_env_train ({n_env_train}) must be a multiple of the number of ranks ({world})"
        assert getattr(algo, "world", 1) == self.world and getattr(algo, "rank", 0) == self.rank, \
            "the algo must be built with the same world / rank as the Trainer"
        save_log = save_log and self.rank == 0                   # one writer: rank 0
        if Trainer._check_params(params):
            self.params = params
        if save_log:
            os.makedirs(log_dir, exist_ok=True)
            self.model_dir = os.path.join(log_dir, "models")
            os.makedirs(self.model_dir, exist_ok=True)
        # the full training state, {log_dir}/resume/{step}.pkl next to models/: written by rank 0 with every weights save,
        # read by every rank of a resumed run
        self.resume_dir = os.path.join(log_dir, "resume")
        if save_log:
            os.makedirs(self.resume_dir, exist_ok=True)
        self.logger = _Logger(log_dir, params["run_name"], env.__class__.__name__, save_log) if self.rank == 0 else None
        self.save_log = save_log
        self.steps = params["training_steps"]
        self.eval_interval = params["eval_interval"]
        self.eval_epi = params["eval_epi"]
        self.save_interval = params["save_interval"]
        self.update_steps = 0
        self.key = np.random.default_rng([seed, 7])
        self.start_step = 0
        # the share of every training batch that starts in the given scenes: n_scene of the n_env_train global envs
        self.scenes, self.scene_jitter = scenes, float(scene_jitter)
        # mining: the pool takes the place of the scenes in every collect; the given scenes are its pinned slots
        self.pool, self.mine_back = None, int(mine_back)
        if scene_priority and int(mine_scenes) == 0:
            raise ValueError("Trainer: scene_priority needs mine_scenes: it is a mode of the pool of mined scenes")
        if int(mine_scenes) != 0:
            if self.world > 1:
                raise ValueError("Trainer: mine_scenes runs on one rank: every rank would keep a pool of its own failures and the "
                                 "ranks' windows would no longer be what one device runs")
            if self.mine_back < 0:
                raise ValueError(f"Trainer: mine_back must be >= 0 (got {mine_back})")
            self.pool = ScenePool(env, int(mine_scenes), pinned=scenes, priority=bool(scene_priority), draw_seed=int(seed))
        source = self.pool if self.pool is not None else scenes
        self.n_scene = scene_count(scene_frac, n_env_train) if source is not None else 0
        if source is None and (float(scene_frac) != 0.0 or self.scene_jitter != 0.0):
            raise ValueError("Trainer: scene_frac / scene_jitter need scenes (given ones, or mine_scenes for a pool of mined ones)")
        if source is not None and not (0.0 < float(scene_frac) <= 1.0 and self.scene_jitter >= 0.0 and self.n_scene >= 1):
            raise ValueError(f"Trainer: with scenes, scene_frac must be in (0, 1] and give at least one of the {n_env_train} "
                             f"training envs, and scene_jitter must be >= 0 (got {scene_frac}, {scene_jitter})")
        if resume:
            self._resume()

    # ---- the state at step s is the state BEFORE iteration s: the loop saves it after eval and the weights save, before it
    # draws the keys of iteration s, so a resumed run repeats the evaluation and the save of step s and goes on from there ----
    def state_dict(self, step: int) -> dict:
        d = {"algo": self.algo.state_dict(),
             "trainer": {"key": CK.generator_state(self.key), "step": int(step), "update_steps": int(self.update_steps)}}
        if self.pool is not None:
            d["scene_pool"] = self.pool.state_dict()
        return d

    def _save_scenes(self, step: int):
        """the pinned and mined scenes of the pool as a scenes file, {log_dir}/scenes/{step}.npz (test.py --scenes reads it);
        nothing while the pool holds none"""
        sc = self.pool.to_scenes()
        if sc is not None:
            os.makedirs(os.path.join(self.log_dir, "scenes"), exist_ok=True)
            path = os.path.join(self.log_dir, "scenes", f"{step}.npz")
            if not self.pool.priority:
                return sc.save(path)
            st = self.pool.stats()         # a priority pool: the statistics of the saved slots as extra arrays (read_npz ignores them)
            write_npz(path, sc.env_id, sc.num_agents, sc.rows["agent"], sc.rows["goal"], sc.rows.get("obst"), sc.obst_key, sc.names,
                      extra={k: st[k][:sc.S] for k in ("score", "visits", "last")})

    def _save_state(self, step: int):
        CK.save_state(self.state_dict(step), os.path.join(self.resume_dir, f"{step}.pkl"))
        for old in CK.state_steps(self.resume_dir)[:-KEEP_STATES]:
            os.remove(os.path.join(self.resume_dir, f"{old}.pkl"))

    def _resume(self):
        """every rank loads the newest state (the ranks' generators are identical by construction, so rank 0's file serves
        all); rank 0 drops the metrics records the stopped run wrote at or after that step"""
        s = CK.latest_state(self.resume_dir)
        if s is None:
            raise no_state_error(self.log_dir)
        tree = CK.load_state(os.path.join(self.resume_dir, f"{s}.pkl"))
        tr = tree["trainer"]
        if int(tr["step"]) != s:
            raise ValueError(f"{self.resume_dir}/{s}.pkl holds the state of step {int(tr['step'])}")
        if self.pool is not None:
            if "scene_pool" not in tree:
                raise ValueError(f"{self.resume_dir}/{s}.pkl holds no scene pool: the stopped run did not mine scenes")
            self.pool.load_state_dict(tree["scene_pool"])
        self.algo.load_state_dict(tree["algo"])
        CK.set_generator_state(self.key, tr["key"])
        self.start_step, self.update_steps = s, int(tr["update_steps"])
        path = self.logger.path if self.logger is not None else None
        if path is not None and os.path.exists(path):
            def before(ln):                      # a line torn by the stop does not parse: it goes too
                try:
                    return json.loads(ln)["step"] < s
                except (ValueError, KeyError, TypeError):
                    return False
            with open(path) as f:
                kept = [ln for ln in f if before(ln)]
            with open(path + ".tmp", "w") as f:
                f.writelines(kept)
                f.flush()
                os.fsync(f.fileno())
            os.replace(path + ".tmp", path)
        if self.rank == 0:
            print(f"> resuming {self.log_dir} at step {s}", flush=True)

    @staticmethod
    def _check_params(params: dict) -> bool:
        for k in ("run_name", "training_steps", "eval_interval", "eval_epi", "save_interval"):
            assert k in params, f"{k} not found in params"
        assert params["eval_interval"] > 0 and params["eval_epi"] >= 1 and params["save_interval"] > 0
        return True

    def evaluate(self, test_keys) -> dict:
        """reductions of trainer.py:105-125 on deterministic rollouts."""
        r = self.algo.collect_deterministic(test_keys, env=self.env_test)
        rewards = r.rewards.cpu().numpy()            # [E, T]
        costs = r.costs.cpu().numpy()                # [E, T, n, nh]
        total = rewards.sum(-1)
        return {
            "eval/reward": float(total.mean()), "eval/reward_final": float(rewards[:, -1].mean()),
            "eval/cost": float(np.maximum(costs, 0.0).max(-1).max(-1).sum(-1).mean()),
            "eval/unsafe_frac": float((costs.max(-1).max(-2) >= 1e-6).mean()),
            "_reward_min": float(total.min()), "_reward_max": float(total.max()),
        }

    def evaluate_scenes(self, scenes=None) -> dict:
        """every given scene (default: self.scenes) rolled once on env_test: deterministic, not jittered; the reductions of
        evaluate"""
        scenes = self.scenes if scenes is None else scenes
        r = self.algo.collect_deterministic(np.arange(1, scenes.S + 1), env=self.env_test, scenes=scenes)
        rewards, costs = r.rewards.cpu().numpy(), r.costs.cpu().numpy()
        return {"eval/scene_reward": float(rewards.sum(-1).mean()),
                "eval/scene_cost": float(np.maximum(costs, 0.0).max(-1).max(-1).sum(-1).mean()),
                "eval/scene_unsafe_frac": float((costs.max(-1).max(-2) >= 1e-6).mean())}

    def train(self):
        start_time = time()
        assert self.n_env_test <= 1000, "n_env_test must be less than or equal to 1_000"
        test_keys = np.random.default_rng([self.seed, 11]).integers(1, 2 ** 62, size=1000)[:self.n_env_test]
        for step in range(self.start_step, self.steps + 1):
            if step % self.eval_interval == 0 and self.rank == 0:
                ev = self.evaluate(test_keys)
                rmin, rmax = ev.pop("_reward_min"), ev.pop("_reward_max")
                print(f"step: {step:3}, time: {time() - start_time:5.0f}s, reward: {ev['eval/reward']:9.4f}, "
                      f"min/max reward: {rmin:7.2f}/{rmax:7.2f}, cost: {ev['eval/cost']:8.4f}, "
                      f"unsafe_frac: {ev['eval/unsafe_frac']:6.2f}", flush=True)
                held = self.pool.to_scenes() if self.pool is not None else self.scenes     # a pool: its pinned + filled slots
                if held is not None:
                    ev.update(self.evaluate_scenes(held))
                    print(f"           scenes: reward: {ev['eval/scene_reward']:9.4f}, cost: {ev['eval/scene_cost']:8.4f}, "
                          f"unsafe_frac: {ev['eval/scene_unsafe_frac']:6.2f}", flush=True)
                self.logger.log(ev, step=self.update_steps)
            if self.save_log and step % self.save_interval == 0:
                self.algo.save(os.path.join(self.model_dir), step)
                self._save_state(step)
                if self.pool is not None:
                    self._save_scenes(step)
            keys = self.key.integers(1, 2 ** 62, size=self.n_env_train)        # the global batch, identical on every rank
            share = self.n_env_train // self.world
            lo, hi = self.rank * share, (self.rank + 1) * share
            source = self.pool if self.pool is not None else self.scenes
            if source is None:
                rollouts = self.algo.collect(None, keys[lo:hi])
            elif self.pool is not None and self.pool.priority:      # draw, collect, mine, score, evicting push: all on the device
                drawn = self.pool.draw(self.n_env_train, self.n_scene, step, lo, hi)
                rollouts = self.algo.collect(None, keys[lo:hi], scenes=self.pool, jitter=self.scene_jitter, scene_of=self.pool.drawn(drawn))
                record = self.algo.rollout_record(rollouts)
                mined = self.pool.score_from(record, drawn, self.pool.mix_flags(hi - lo), step, self.mine_back, 1e-6)
                self.pool.push_from(record, self.mine_back, 1e-6, step=step, mined=mined)
            else:
                scene_of = mix_assignment(self.n_env_train, self.n_scene, source.S, step, lo, hi)
                rollouts = self.algo.collect(None, keys[lo:hi], scenes=source, jitter=self.scene_jitter, scene_of=scene_of)
            if self.pool is not None and not self.pool.priority:
                # the envs that started in scenes included: a jittered scene that still fails is a failure
                self.pool.push_from(self.algo.rollout_record(rollouts), self.mine_back, 1e-6)
            update_info = self.algo.update(rollouts, step)                      # global values on every rank (Engine.info)
            if self.logger is not None:
                self.logger.log(update_info, step=self.update_steps)
            self.update_steps += 1
