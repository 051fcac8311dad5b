"""User-given start scenes: where an episode begins when it does not begin at the sampled reset.

The reference ships no way to start an episode anywhere but at reset; its env_states is a Python pytree a user can fill by hand.
Here the state is a device record, so a scene is given as template rows — agents and goals in the record's own layout,
obstacles as (cx, cy, w, h, theta) or (ox, oy) — and dgppo_env_scene_load (csrc/env_scene.hip) forms the record from them.

    scenes = Scenes(env, agent, goal, rect=rect)          # or Scenes.load("headon.npz", env)
    ro = algo.collect_deterministic(keys, env=env, scenes=scenes)     # episode b starts in scene b % S

Scenes also come out of rollouts: the state a few steps before an episode's first unsafe step is a scene from which this policy
fails (dgppo_env_scene_mine).  Scenes.mine(env, record) reads them back as a Scenes; ScenePool keeps them on the device, in a ring
that a training run refills from every rollout (dgppo_env_scene_pool_push) and starts a share of its next batch in.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import _native as N
from .. import ops_env as OE

f32 = np.float32


class SceneStart(NamedTuple):
    """what the engine's rollouts take as `start`: the scenes, which scene every env starts in (host ints [B]; None: env b
    takes scene b % S) and how far the agents are moved off their template positions (0: not at all)"""
    scenes: "Scenes"
    scene_ids: Optional[np.ndarray] = None
    jitter: float = 0.0


class SceneMix(NamedTuple):
    """the `start` of a rollout whose batch mixes sampled and given starts (dgppo_env_scene_mix): every env is reset from its
    seed, then env b with scene_of[b] >= 0 (host ints [B]) restarts in that scene, moved by up to `jitter`; an env whose scene
    stays invalid keeps its reset and is counted in the engine's scene_fallback"""
    scenes: "Scenes"
    scene_of: np.ndarray
    jitter: float = 0.0


class SceneMixDrawn(NamedTuple):
    """SceneMix whose scene_of is the device int32 [B] tensor that ScenePool.draw wrote (dgppo_env_scene_pool_draw): trusted to be
    in range, so the start copies nothing to the host and waits for nothing.  flags (device int32 [B], or None) receives the
    validity bits of the envs scene_of names; the rollout whose record is scored passes it, its deterministic twin passes None"""
    scenes: "ScenePool"
    scene_of: torch.Tensor
    flags: Optional[torch.Tensor] = None
    jitter: float = 0.0


class SceneDraw(NamedTuple):
    """what collect(..., scene_of=) takes in place of host ints under a priority pool (ScenePool.drawn): the device int32 [B] tensor
    the pool drew, and the device int32 [B] buffer the scored rollout's validity bits go to"""
    scene_of: torch.Tensor
    flags: Optional[torch.Tensor] = None


def mix_assignment(n_total: int, n_scene: int, S: int, step: int, lo: int, hi: int) -> np.ndarray:
    """int32 [hi - lo]: the scene_of window of the global envs lo .. hi - 1 of a batch of n_total envs of which n_scene start in
    one of S scenes.  Global env g is a scene env iff (g + 1) n_scene // n_total > g n_scene // n_total, which spreads them
    evenly; its ordinal is k = g n_scene // n_total and its scene (k + step) % S, so the scenes rotate over the iterations;
    every other env gets -1.  A function of the global index alone: the ranks' windows together are what one device runs."""
    n_total, n_scene, S, step, lo, hi = (int(v) for v in (n_total, n_scene, S, step, lo, hi))
    if not (0 <= n_scene <= n_total and S >= 1 and 0 <= lo <= hi <= n_total):
        raise ValueError(f"mix_assignment: need 0 <= n_scene <= n_total, S >= 1 and 0 <= lo <= hi <= n_total (got n_total "
                         f"{n_total}, n_scene {n_scene}, S {S}, window [{lo}, {hi}))")
    g = np.arange(lo, hi, dtype=np.int64)
    k = g * n_scene // n_total
    return np.where((g + 1) * n_scene // n_total > k, (k + step) % S, -1).astype(np.int32)


def decode_flags(bits: int) -> str:
    """the names of the validity bits of dgppo_env_scene_load that are set"""
    return " | ".join(name for k, name in enumerate(N.SCENE_BITS) if int(bits) >> k & 1) or "valid"


def check_templates(cfg: N.EnvCfg, agent, goal, rect=None, disc=None, names=None) -> Dict[str, np.ndarray]:
    """the host half of Scenes(): kind, shapes and names against cfg -> dict(agent, goal[, obst], names) of float32 arrays with
    a leading S.  Raises ValueError; touches no device."""
    if cfg.is_vmas:
        raise ValueError("Scenes: VMASReverseTransport has no scene entry point (its record has a body and a scene row, "
                         "no goal / obstacle rows)")
    agent, goal = np.ascontiguousarray(agent, f32), np.ascontiguousarray(goal, f32)
    if agent.ndim != 3 or agent.shape[0] < 1:
        raise ValueError(f"Scenes: agent must be [S, n, sd] with S >= 1 (got shape {agent.shape})")
    S = agent.shape[0]
    shapes = OE.scene_template_shapes(cfg)
    given = {"agent": agent, "goal": goal}
    which = "rect" if cfg.is_lidar else "disc"
    other, other_name = (disc, "disc") if cfg.is_lidar else (rect, "rect")
    if other is not None:
        raise ValueError(f"Scenes: {other_name} rows are for the {'MPE' if cfg.is_lidar else 'LiDAR'} kinds; env kind {cfg.kind} "
                         f"takes {which}")
    obst = rect if cfg.is_lidar else disc
    if cfg.n_obs > 0:
        if obst is None:
            raise ValueError(f"Scenes: {which} [S, {cfg.n_obs}, {shapes['obst'][1]}] is required (the env has {cfg.n_obs} obstacles)")
        given["obst"] = np.ascontiguousarray(obst, f32)
    elif obst is not None:
        raise ValueError(f"Scenes: the env has no obstacles, {which} must be None")
    for name, x in given.items():
        if tuple(x.shape) != (S,) + shapes[name]:
            shown = which if name == "obst" else name
            raise ValueError(f"Scenes: {shown}: expected shape {(S,) + shapes[name]}, got {tuple(x.shape)}")
    names = [f"scene{s}" for s in range(S)] if names is None else [str(x) for x in names]
    if len(names) != S:
        raise ValueError(f"Scenes: {len(names)} names for {S} scenes")
    given["names"] = names
    return given


def write_npz(path, env_id: str, num_agents: int, agent, goal, obst, obst_key: Optional[str], names: Sequence[str],
              extra: Optional[Dict[str, np.ndarray]] = None) -> None:
    """the file format of Scenes.save: env_id, num_agents, agent, goal, rect or disc (absent without obstacles), names; extra:
    further arrays under their own names (a priority pool's statistics), which read_npz does not look at"""
    out = dict(env_id=np.array(env_id), num_agents=np.array(int(num_agents), np.int64), agent=np.asarray(agent, f32),
               goal=np.asarray(goal, f32), names=np.array(list(names), dtype=np.str_))
    out.update(extra or {})
    if obst is not None:
        out[obst_key] = np.asarray(obst, f32)
    with open(path, "wb") as f:          # a file object: numpy appends no suffix
        np.savez(f, **out)


def read_npz(path) -> dict:
    """-> dict(env_id, num_agents, agent, goal, rect, disc, names); rect / disc None where the file has none"""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("env_id", "num_agents", "agent", "goal", "names") if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a scenes file: no {missing}")
        return dict(env_id=str(z["env_id"]), num_agents=int(z["num_agents"]), agent=z["agent"], goal=z["goal"],
                    rect=z["rect"] if "rect" in z.files else None, disc=z["disc"] if "disc" in z.files else None,
                    names=[str(x) for x in z["names"]])


def check_file(path, env_id: str, num_agents: int) -> dict:
    """read_npz of a file that must hold scenes of env kind env_id with num_agents agents; ValueError otherwise.  Touches no
    device: train.py asks before it starts a rank"""
    z = read_npz(path)
    if z["env_id"] != env_id or z["num_agents"] != num_agents:
        raise ValueError(f"{path}: scenes of {z['env_id']} with {z['num_agents']} agents, the env is {env_id} with {num_agents}")
    return z


class Scenes:
    """S start scenes of one environment: template rows checked against env.cfg, uploaded once, and validated by one
    dgppo_env_scene_load call (B = S, no jitter): a scene with a non-finite word, an agent outside the area, two overlapping
    agents or an agent inside an obstacle raises ValueError naming the scene and what is wrong with it.  Goals are checked for
    finiteness only: a goal behind a wall is a legitimate hard scene.
      agent [S, n, sd], goal [S, n_goals, sd]   rows in the record's layout (x, y, vx, vy; bicycle_rows for LidarBicycleTarget)
      rect  [S, n_obs, 5]                        LiDAR kinds: cx, cy, w, h, theta
      disc  [S, n_obs, 2]                        MPE kinds: ox, oy
      names                                      S strings (default scene0, scene1, ...)"""

    def __init__(self, env, agent, goal, rect=None, disc=None, names=None):
        cfg = env.cfg
        rows = check_templates(cfg, agent, goal, rect, disc, names)
        self.env_id, self.num_agents, self.cfg = env.KIND, int(cfg.n_agents), cfg
        self.names = rows.pop("names")
        self.rows: Dict[str, np.ndarray] = rows                      # host copies: agent, goal[, obst]
        self.S = int(rows["agent"].shape[0])
        dev = env.device
        self.dev: Dict[str, torch.Tensor] = {k: torch.from_numpy(v).to(dev) for k, v in rows.items()}
        st = OE.State.empty(cfg, self.S, dev)
        flags = torch.zeros(self.S, dtype=torch.int32, device=dev)
        OE.scene_load(cfg, self.dev, None, None, 0.0, st, flags)
        bad = [(s, int(b)) for s, b in enumerate(flags.cpu().tolist()) if b]
        if bad:
            raise ValueError("Scenes: invalid scene(s): " + "; ".join(f"{self.names[s]} (#{s}): {decode_flags(b)}" for s, b in bad))

    @property
    def obst_key(self) -> Optional[str]:
        return None if "obst" not in self.rows else ("rect" if self.cfg.is_lidar else "disc")

    def start(self, scene_ids=None, jitter: float = 0.0) -> SceneStart:
        """the `start` argument of the engine's rollouts"""
        return SceneStart(self, None if scene_ids is None else np.asarray(scene_ids), float(jitter))

    def mix(self, scene_of, jitter: float = 0.0) -> SceneMix:
        """the `start` argument of a rollout that mixes the sampled reset (scene_of[b] < 0) with these scenes"""
        return SceneMix(self, np.asarray(scene_of), float(jitter))

    def save(self, path) -> None:
        write_npz(path, self.env_id, self.num_agents, self.rows["agent"], self.rows["goal"], self.rows.get("obst"), self.obst_key,
                  self.names)

    @classmethod
    def load(cls, path, env) -> "Scenes":
        z = check_file(path, env.KIND, env.num_agents)
        return cls(env, z["agent"], z["goal"], rect=z["rect"], disc=z["disc"], names=z["names"])

    @classmethod
    def mine(cls, env, record, back: int = 8, thresh: float = 1e-6, max_scenes: Optional[int] = None,
             names=None) -> Optional["Scenes"]:
        """failure scenes of a rollout record (engine.RolloutData; its time-major fields are enough, before or after
        finalize()): for every env whose cost reaches `thresh` at some step first >= 1, the state `back` steps earlier
        (t0 = max(first - back, 0)) as a scene, where that state is a valid one (dgppo_env_scene_mine's flags).  The taken
        envs are kept in env order, the first max_scenes of them; None when there is none.  names: one string per kept
        scene, or a function (env index, first, t0, who) -> string; default env{b}_t{t0}_first{first}_a{agent}.  The result
        carries .mined = dict(env, first, t0, who): host int arrays, one entry per scene (who = agent * n_cost + cost column).
        The state is the situation, not the rest of the episode: it restarts with a zero actor carry and a fresh step count."""
        cfg = env.cfg
        if cfg.is_vmas:
            raise ValueError("Scenes.mine: VMASReverseTransport has no scene entry point")
        B = int(record.agent_tm.shape[1])
        out = OE.alloc_mined(cfg, B, record.agent_tm.device)
        OE.scene_mine(cfg, record.agent_tm, record.cost_tm, record.goal, record.obst, back, thresh, out)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        took = np.flatnonzero((host["first"] >= 1) & (host["flags"] == 0))
        if max_scenes is not None:
            took = took[:max(int(max_scenes), 0)]
        if len(took) == 0:
            return None
        first, t0, who = host["first"][took], host["t0"][took], host["who"][took]
        if names is None:
            names = lambda b, f, t, w: f"env{b}_t{t}_first{f}_a{w // cfg.n_cost}"
        if callable(names):
            names = [names(int(b), int(f), int(t), int(w)) for b, f, t, w in zip(took, first, t0, who)]
        obst = host["obst"][took] if "obst" in host else None
        sc = cls(env, host["agent"][took], host["goal"][took], rect=obst if cfg.is_lidar else None,
                 disc=None if cfg.is_lidar else obst, names=names)
        sc.mined = dict(env=took.astype(np.int64), first=first.astype(np.int64), t0=t0.astype(np.int64), who=who.astype(np.int64))
        return sc

    @staticmethod
    def bicycle_rows(x, y, heading, speed) -> np.ndarray:
        """[..., 5] agent or goal rows of LidarBicycleTarget in the record's layout: x, y, cos(heading), sin(heading), speed
        (lidar_bicycle_target.py:48-50)"""
        x, y, heading, speed = np.broadcast_arrays(np.asarray(x, f32), np.asarray(y, f32), np.asarray(heading, f32),
                                                   np.asarray(speed, f32))
        return np.stack([x, y, np.cos(heading).astype(f32), np.sin(heading).astype(f32), speed], axis=-1).astype(f32)


def check_pool(capacity: int, n_pinned: int) -> None:
    """the host half of ScenePool(): ValueError; touches no device"""
    if int(capacity) < 1 or int(capacity) <= int(n_pinned):
        raise ValueError(f"ScenePool: capacity must be >= 1 and larger than the number of pinned scenes, so that the ring of mined "
                         f"scenes has a slot (got capacity {capacity}, {n_pinned} pinned)")


def check_pool_priority(capacity: int, beta: float, age_cap: int, min_visits: int, evict_w: float, draw_seed: int) -> None:
    """the host half of ScenePool(priority=True): ValueError; touches no device"""
    if int(capacity) > OE.POOL_MAX_M:
        raise ValueError(f"ScenePool: with priority, capacity must be <= {OE.POOL_MAX_M} (got {capacity})")
    if not 0.0 < float(beta) <= 1.0:
        raise ValueError(f"ScenePool: beta must be in (0, 1] (got {beta})")
    if int(age_cap) != age_cap or not 1 <= int(age_cap) <= OE.POOL_MAX_AGE:
        raise ValueError(f"ScenePool: age_cap must be an int in [1, {OE.POOL_MAX_AGE}] (got {age_cap})")
    if int(min_visits) != min_visits or int(min_visits) < 0:
        raise ValueError(f"ScenePool: min_visits must be an int >= 0 (got {min_visits})")
    if not 0.0 <= float(evict_w) <= 1.0:
        raise ValueError(f"ScenePool: evict_w must be in [0, 1] (got {evict_w})")
    if int(draw_seed) != draw_seed or not 0 <= int(draw_seed) < 2 ** 64:
        raise ValueError(f"ScenePool: draw_seed must be an int in [0, 2^64) (got {draw_seed})")


class ScenePool:
    """A device-resident pool of M = capacity scenes for a training run that mines its own failures: the scenes of `pinned` in
    slots 0 .. P-1, never overwritten, and behind them a ring of R = M - P slots that push_from() fills with the failure scenes of
    a rollout record (dgppo_env_scene_mine, dgppo_env_scene_pool_push), oldest overwritten first.  It has what the engine and
    SceneMix read of a Scenes (.dev, .S = M, .cfg, .names, .mix), so collect(..., scenes=pool, scene_of=...) works unchanged.
    An empty ring slot holds NaN words: dgppo_env_scene_mix gives an env that draws it the NONFINITE bit and leaves its sampled
    reset standing, so an empty slot means "sampled reset" (counted in rollout/scene_fallback), mix_assignment keeps S = M from
    the first iteration, and no count has to come back to the host before a rollout.
      state (device int32 [4])   head, filled, pushed_total, taken_last (dgppo_env_scene_pool_push)
    priority=True (csrc/env_scene_pool.hip) keeps, per slot, score (the EMA, with weight beta, of the failed fraction of the slot's
    replays), visits and last (the step of its last replay or write), and an int32 [8] state (the four words above, evicted_last,
    dropped_last, replays_last, replay_fails_last).  draw() gives every scene env a live slot in proportion to q(score) *
    min(1 + step - last, age_cap) with q = 4 s (1 - s) in integers (Philox keyed by draw_seed), so an empty slot is never drawn;
    score_from() folds what the replays of a rollout did into the statistics; push_from() writes empty slots first and then
    evicts the filled ones with visits >= min_visits and 4 s (1 - s) <= evict_w — solved and hopeless ones — instead of the oldest."""

    def __init__(self, env, capacity: int, pinned: Optional[Scenes] = None, priority: bool = False, beta: float = 0.3,
                 age_cap: int = 16, min_visits: int = 2, evict_w: float = 0.36, draw_seed: int = 0):
        cfg = env.cfg
        if cfg.is_vmas:
            raise ValueError("ScenePool: VMASReverseTransport has no scene entry point")
        self.P = 0 if pinned is None else int(pinned.S)
        check_pool(capacity, self.P)
        self.priority = bool(priority)
        if self.priority:
            check_pool_priority(capacity, beta, age_cap, min_visits, evict_w, draw_seed)
        self.beta, self.age_cap, self.min_visits = float(beta), int(age_cap), int(min_visits)
        self.evict_w, self.draw_seed = float(evict_w), int(draw_seed)
        if pinned is not None and (pinned.cfg.kind, pinned.cfg.n_agents, pinned.cfg.n_obs) != (cfg.kind, cfg.n_agents, cfg.n_obs):
            raise ValueError("ScenePool: the pinned scenes are of another env")
        self.env, self.cfg, self.S = env, cfg, int(capacity)
        self.env_id, self.num_agents = env.KIND, int(cfg.n_agents)
        dev = env.device
        self.dev: Dict[str, torch.Tensor] = {k: torch.full((self.S,) + s, float("nan"), device=dev)
                                             for k, s in OE.scene_template_shapes(cfg).items()}
        if pinned is not None:
            for k, v in self.dev.items():
                v[:self.P].copy_(pinned.dev[k])
        self.pinned_names = [] if pinned is None else list(pinned.names)
        self._stats: Optional[Dict[str, torch.Tensor]] = OE.alloc_pool_stats(self.S, dev) if self.priority else None
        self.state = self._stats["state"] if self.priority else torch.zeros(4, dtype=torch.int32, device=dev)
        self._mined: Dict[int, Dict[str, torch.Tensor]] = {}      # scene_mine's outputs per batch size, allocated once
        self._drawn: Dict[int, torch.Tensor] = {}                 # draw's scene_of per batch size, allocated once
        self._flags: Dict[int, torch.Tensor] = {}                 # the mix flags of a drawn start per batch size

    @property
    def names(self):
        return self.pinned_names + [f"pool{m}" for m in range(self.P, self.S)]

    def mix(self, scene_of, jitter: float = 0.0) -> SceneMix:
        return SceneMix(self, np.asarray(scene_of), float(jitter))

    def _need_priority(self, what: str):
        if not self.priority:
            raise ValueError(f"ScenePool.{what} needs ScenePool(..., priority=True)")

    def _mine(self, record, back: int, thresh: float) -> Dict[str, torch.Tensor]:
        B = int(record.agent_tm.shape[1])
        if B not in self._mined:
            self._mined[B] = OE.alloc_mined(self.cfg, B, self.state.device)
        out = self._mined[B]
        OE.scene_mine(self.cfg, record.agent_tm, record.cost_tm, record.goal, record.obst, back, thresh, out)
        return out

    def draw(self, n_total: int, n_scene: int, step: int, lo: int, hi: int) -> torch.Tensor:
        """priority mode: the device int32 scene_of of the global envs lo .. hi - 1 of a batch of n_total envs of which n_scene are
        scene envs (those of mix_assignment), every one with a live slot drawn by priority, or -1 while none is live; one launch,
        no sync.  The tensor is the pool's own, one per window size: the next draw of that size overwrites it"""
        self._need_priority("draw")
        B = int(hi) - int(lo)
        if B < 0:
            raise ValueError(f"ScenePool.draw: need lo <= hi (got [{lo}, {hi}))")
        if B not in self._drawn:
            self._drawn[B] = torch.empty(B, dtype=torch.int32, device=self.state.device)
        OE.scene_pool_draw(self.cfg, self._stats, self.P, self.age_cap, step, self.draw_seed, n_total, n_scene, lo, self._drawn[B])
        return self._drawn[B]

    def mix_flags(self, B: int) -> torch.Tensor:
        """priority mode: the pool's device int32 [B] buffer for the validity bits of a drawn mix of B envs (score_from reads it)"""
        self._need_priority("mix_flags")
        if B not in self._flags:
            self._flags[B] = torch.zeros(int(B), dtype=torch.int32, device=self.state.device)
        return self._flags[B]

    def drawn(self, scene_of: torch.Tensor) -> SceneDraw:
        """what draw() returned, as collect(..., scenes=pool, scene_of=) takes it, with mix_flags of its size for the bits"""
        return SceneDraw(scene_of, self.mix_flags(int(scene_of.shape[0])))

    def mix_drawn(self, scene_of: torch.Tensor, flags: Optional[torch.Tensor] = None, jitter: float = 0.0) -> SceneMixDrawn:
        """the `start` argument of a rollout that starts the envs draw() named in their slots"""
        self._need_priority("mix_drawn")
        return SceneMixDrawn(self, scene_of, flags, float(jitter))

    def score_from(self, record, scene_of: torch.Tensor, mix_flags: torch.Tensor, step: int, back: int = 8,
                   thresh: float = 1e-6) -> Dict[str, torch.Tensor]:
        """priority mode: mine the record (engine.RolloutData) of the rollout that draw()'s scene_of started and whose scene mix
        wrote mix_flags, and fold what its replays did into score, visits and last.  -> what was mined, which a push_from of the
        same record, back and thresh takes as `mined` so as not to mine again.  No sync"""
        self._need_priority("score_from")
        out = self._mine(record, back, thresh)
        OE.scene_pool_score(self.cfg, scene_of, mix_flags, out["first"], self._stats, self.beta, step)
        return out

    def push_from(self, record, back: int = 8, thresh: float = 1e-6, step: int = 0, mined=None) -> None:
        """mine the record (engine.RolloutData), unless score_from's `mined` of it is given, and push its taken envs into the ring:
        two launches, no sync.  Priority mode: the evicting push (dgppo_env_scene_pool_push_evict), the written slots' `last` set
        to `step`"""
        out = self._mine(record, back, thresh) if mined is None else mined
        if self.priority:
            OE.scene_pool_push_evict(self.cfg, out, self.dev, self.P, self._stats, self.min_visits, self.evict_w, step)
        else:
            OE.scene_pool_push(self.cfg, out, self.dev, self.P, self.state)

    def fill(self):
        """-> (filled, pushed_total, taken_last); one host sync"""
        _, filled, pushed, taken = self.state.cpu().tolist()[:4]
        return int(filled), int(pushed), int(taken)

    def stats(self) -> Dict[str, np.ndarray]:
        """priority mode: score, visits, last ([M]) and state ([8]) on the host; one sync"""
        self._need_priority("stats")
        packed = torch.cat([self._stats[k].view(torch.int32) for k in OE.POOL_STATS + ("state",)]).cpu().numpy()
        M = self.S
        return {"score": packed[:M].view(f32).copy(), "visits": packed[M:2 * M].copy(), "last": packed[2 * M:3 * M].copy(),
                "state": packed[3 * M:].copy()}

    def to_scenes(self) -> Optional[Scenes]:
        """the pinned and the filled slots as a host Scenes (the ring fills from its first slot on); None while there is none"""
        k = self.P + self.fill()[0]
        if k == 0:
            return None
        rows = {name: v[:k].cpu().numpy() for name, v in self.dev.items()}
        obst = rows.get("obst")
        return Scenes(self.env, rows["agent"], rows["goal"], rect=obst if self.cfg.is_lidar else None,
                      disc=None if self.cfg.is_lidar else obst, names=self.names[:k])

    def state_dict(self) -> dict:
        d = {k: v.cpu().numpy() for k, v in self.dev.items()}
        d["state"] = self.state.cpu().numpy()
        d["pinned"] = int(self.P)
        if self.priority:
            d["stats"] = {k: self._stats[k].cpu().numpy() for k in OE.POOL_STATS}
        return d

    def load_state_dict(self, d: dict) -> None:
        if int(d.get("pinned", -1)) != self.P or any(k not in d or tuple(d[k].shape) != tuple(v.shape) for k, v in self.dev.items()):
            raise ValueError("ScenePool: the stored pool does not fit this one (capacity, pinned scenes or env differ)")
        if ("stats" in d) != self.priority:
            raise ValueError(f"ScenePool: the stored pool is {'a priority pool' if 'stats' in d else 'a plain ring'}, this one is "
                             f"{'a priority pool' if self.priority else 'a plain ring'}: the two modes do not load each other")
        for k, v in self.dev.items():
            v.copy_(torch.from_numpy(np.ascontiguousarray(d[k], f32)))
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(d["state"], np.int32)))
        if self.priority:
            for k in OE.POOL_STATS:
                self._stats[k].copy_(torch.from_numpy(np.ascontiguousarray(d["stats"][k], f32 if k == "score" else np.int32)))
