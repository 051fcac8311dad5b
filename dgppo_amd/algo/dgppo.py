"""DGPPO with the reference's constructor / method surface (dgppo/algo/dgppo.py:27-321 through
informarl_lagr.py:27-123 and informarl.py:30-256), driving the HIP engine.

Differences that cannot be avoided and are recorded in DESIGN.md: PRNG keys are integer seeds (JAX threefry streams are not
reproducible); `params` are flax-named trees of numpy arrays snapshotted from the device buffers."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import engine as EN
from .. import init as INIT
from .. import nets
from .. import ops_nn as K
from ..trainer.data import (ActionLandscape, ActionRolloutLandscape, CostLandscape, JointLookaheadShieldLog, Landscape,
                            LookaheadShieldLog, Rollout,
                            RolloutLandscape, ShieldLog)
from ..utils import checkpoint as CK
from ..utils.graph import GraphsTuple
from .base import Algorithm


class _LazyGraphs:
    """rollout.graph / rollout.next_graph: GraphsTuple fields of all (env, t), materialised on first access."""

    def __init__(self, env, ro: EN.RolloutData, offset: int):
        self._env, self._ro, self._off, self._g = env, ro, offset, None

    def _mat(self):
        if self._g is None:
            ro, T, off = self._ro.finalize(), self._ro.T, self._off
            B = ro.B
            flat = lambda x: x[:, off:off + T].reshape((B * T,) + x.shape[2:]).contiguous()
            rep = lambda x: x.repeat_interleave(T, dim=0)
            g = self._env.graph_batch(self._env.record_state(ro, flat, rep))
            unf = lambda x: x.view((B, T) + x.shape[1:]) if torch.is_tensor(x) else x
            es = g.env_states
            es = type(es)(*[_unflatten_tree(v, B, T) for v in es])
            self._g = GraphsTuple(*[unf(getattr(g, f)) for f in GraphsTuple._fields[:8]], es, None)
        return self._g

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._mat(), name)

    def _replace(self, **kw):
        return self._mat()._replace(**kw)


def _unflatten_tree(v, B, T):
    if torch.is_tensor(v):
        return v.view((B, T) + v.shape[1:])
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        return type(v)(*[_unflatten_tree(x, B, T) for x in v])
    return v


def _check_rnn_options(use_rnn: bool, use_lstm: bool, rnn_layers: int):
    """GRU or LSTM cells, any number of stacked layers (dgppo/nn/rnn.py:17-29), or --no-rnn"""
    assert rnn_layers >= 1


def _n_cells(use_rnn: bool, rnn_layers: int) -> int:
    return rnn_layers if use_rnn else 0


def _grid_axis(what: str, name: str, v, m: int, area: float, lo: float = 0.0) -> np.ndarray:
    """one axis of a landscape grid in fp32: the given lines, or linspace(lo, area, m)"""
    if v is None:
        if int(m) < 1:
            raise ValueError(f"{what}: {name}: the grid is empty")
        v = np.linspace(lo, area, int(m))
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    if v.size == 0 or not np.isfinite(v).all():
        raise ValueError(f"{what}: {name} must be a non-empty array of finite coordinates")
    return v


class DGPPO(Algorithm):
    def __init__(self, env, node_dim: int, edge_dim: int, state_dim: int, action_dim: int, n_agents: int,
                 actor_gnn_layers: int = 2, Vl_gnn_layers: int = 2, Vh_gnn_layers: int = 1, gamma: float = 0.99,
                 lr_actor: float = 3e-4, lr_Vl: float = 1e-3, lr_Vh: float = 1e-3, batch_size: int = 8192,
                 epoch_ppo: int = 1, clip_eps: float = 0.25, gae_lambda: float = 0.95, coef_ent: float = 1e-2,
                 max_grad_norm: float = 2.0, seed: int = 0, use_rnn: bool = True, rnn_layers: int = 1, rnn_step: int = 16,
                 use_lstm: bool = False, alpha: float = 10.0, cbf_eps: float = 1e-2, cbf_weight: float = 1.0,
                 train_steps: int = 1e5, cbf_schedule: bool = True, allreduce=None, world: int = 1, rank: int = 0, **kwargs):
        super().__init__(env, node_dim, edge_dim, action_dim, n_agents)
        _check_rnn_options(use_rnn, use_lstm, rnn_layers)
        assert epoch_ppo >= 1
        assert node_dim == env.node_dim and action_dim == 2
        self.state_dim = state_dim
        self.seed = seed
        self.epoch_ppo, self.use_rnn, self.rnn_layers, self.use_lstm = epoch_ppo, use_rnn, rnn_layers, use_lstm
        self.hp = EN.Hyper(gamma=gamma, gae_lambda=gae_lambda, clip_eps=clip_eps, coef_ent=coef_ent,
                           max_grad_norm=max_grad_norm, lr_actor=lr_actor, lr_Vl=lr_Vl, lr_Vh=lr_Vh, batch_size=batch_size,
                           rnn_step=rnn_step, alpha=alpha, cbf_eps=cbf_eps, cbf_weight=cbf_weight, cbf_schedule=cbf_schedule,
                           train_steps=int(train_steps), actor_gnn_layers=actor_gnn_layers, Vl_gnn_layers=Vl_gnn_layers,
                           Vh_gnn_layers=Vh_gnn_layers, use_rnn=use_rnn, rnn_layers=rnn_layers, use_lstm=bool(use_lstm and use_rnn))
        self.device = env.device
        self.engine = EN.Engine(env.cfg, self.hp, self.device, T=env.max_episode_steps, allreduce=allreduce, world=world,
                                use_graphs=True, multi_stream=True, rank=rank)
        self._init_dp(seed, world, rank)
        nc, lstm = _n_cells(use_rnn, rnn_layers), self.hp.use_lstm
        self.engine.policy.load_tree(INIT.init_policy(seed, node_dim, action_dim, actor_gnn_layers, nc, lstm))
        self.engine.Vl.load_tree(INIT.init_value(seed, node_dim, 1, Vl_gnn_layers, 2, rnn_layers=nc, lstm=lstm))
        # the constraint-value net is built with ValueNet's default of one cell (dgppo.py:83-95)
        self.engine.Vh.load_tree(INIT.init_value(seed, node_dim, env.n_cost, Vh_gnn_layers, 3, rnn_layers=min(nc, 1)))
        # np.random.randint(0, 102400) at trace time in the reference (distribution.py:40)
        self.engine.set_entropy_noise(int(np.random.randint(0, 102400)))
        # (n_rnn_layers, n_agents, n_carries, rnn_state_dim), zeros (informarl.py:115-124)
        # (n_rnn_layers, n_agents, n_carries, 64): one carry for GRU / no cell, (c, h) for LSTM (informarl.py:115-124)
        self.init_rnn_state = torch.zeros(rnn_layers, n_agents, 2 if self.hp.use_lstm else 1, nets.HID, device=self.device)
        self._rng = np.random.default_rng([seed, 99])
        self._single = nets.Arena(self.device)

    # ---- data parallelism: batch_size and the keys handed to collect() are this rank's SHARE; everything random
    # that must agree across the ranks comes from generators every rank seeds identically ----
    def _init_dp(self, seed: int, world: int, rank: int):
        self.world, self.rank = int(world), int(rank)
        self._perm_rng = np.random.default_rng([seed, 4242])
        self.perm_fn = None                   # tests: B -> permutation of this rank's env indices

    def _perm(self, B: int) -> np.ndarray:
        """minibatch order of one epoch.  One device: host np.random like the reference (dgppo.py:155-156).  Several ranks: the
        SAME permutation of the local env indices on every rank, from a generator all ranks seed identically — minibatch k
        of the job is the union of the ranks' k-th slices."""
        if self.perm_fn is not None:
            return np.asarray(self.perm_fn(B))
        if self.world == 1:
            perm = np.arange(B)
            np.random.shuffle(perm)
            return perm
        return self._perm_rng.permutation(B)

    def _draw_keys(self, B_local: int) -> np.ndarray:
        """B_local fresh keys of THIS rank out of world * B_local drawn identically on every rank (a function of the global
        env index, so the union over the ranks is what one device would draw for the global batch)"""
        x = self._rng.integers(1, 2 ** 62, size=B_local * self.world)
        return x[self.rank * B_local:(self.rank + 1) * B_local]

    # ---- carry layout: the reference's (n_layers, n_agents, n_carries = 1, 64) <-> the engine's packed rows [n, L * 64] ----
    def _carry_dims(self):
        nc = 2 if self.hp.use_lstm else 1
        return max(self.engine.HC // (nets.HID * nc), 1), nc

    def _pack_carry(self, rnn_state) -> torch.Tensor:
        """(L, n, n_carries, 64) -> packed rows [n, L * n_carries * 64] (per layer: carry 0, carry 1)"""
        n, (L, nc) = self.n_agents, self._carry_dims()
        x = torch.as_tensor(rnn_state, dtype=torch.float32, device=self.device).reshape(-1, n, nc, nets.HID)[:L]
        return x.permute(1, 0, 2, 3).reshape(n, self.engine.HC).contiguous()

    def _unpack_carry(self, rows: torch.Tensor) -> torch.Tensor:
        """[..., n, L * n_carries * 64] -> [..., L, n, n_carries, 64]"""
        n, (L, nc) = self.n_agents, self._carry_dims()
        lead = rows.shape[:-2]
        x = rows.reshape(lead + (n, L, nc, nets.HID))
        k = len(lead)
        return x.permute(tuple(range(k)) + (k + 1, k, k + 2, k + 3))

    # ---- reference properties ----
    @property
    def config(self) -> dict:
        hp = self.hp
        return {"cost_weight": 0.0, "actor_gnn_layers": hp.actor_gnn_layers, "Vl_gnn_layers": hp.Vl_gnn_layers,
                "gamma": hp.gamma, "lr_actor": hp.lr_actor, "lr_Vl": hp.lr_Vl, "batch_size": hp.batch_size,
                "epoch_ppo": self.epoch_ppo, "clip_eps": hp.clip_eps, "gae_lambda": hp.gae_lambda, "coef_ent": hp.coef_ent,
                "max_grad_norm": hp.max_grad_norm, "seed": self.seed, "use_rnn": self.use_rnn, "rnn_layers": self.rnn_layers,
                "rnn_step": hp.rnn_step, "use_lstm": self.use_lstm, "cost_schedule": False, "lr_Vh": hp.lr_Vh,
                "Vh_gnn_layers": hp.Vh_gnn_layers, "lagr_init": 0.78, "lr_lagr": 1e-7, "alpha": hp.alpha,
                "cbf_eps": hp.cbf_eps, "cbf_weight": hp.cbf_weight, "cbf_schedule": hp.cbf_schedule}

    @property
    def params(self):
        e = self.engine
        return {"policy": e.policy.to_tree(), "Vl": e.Vl.to_tree(), "Vh": e.Vh.to_tree()}

    def _maybe_load(self, params):
        if params is not None:
            for k, net in self.engine.nets.items():
                if k in params:
                    net.load_tree(params[k])

    # ---- single-graph act / step (B = 1 view of the batched kernels) ----
    def _policy_single(self, graph: GraphsTuple, rnn_state):
        env, cfg = self._env, self._env.cfg
        st = env._state_of(graph)
        n = cfg.n_agents
        feats = self.engine._feats("one", st, 1)
        h0 = self._pack_carry(rnn_state)
        hs = torch.empty(n, self.engine.HC, device=self.device)
        act = self.engine.policy.forward(feats, n_seq=n, T=1, h0=h0, tag="one", hs_out=hs, train=False)
        return act["ms"], self._unpack_carry(hs)

    def act(self, graph: GraphsTuple, rnn_state, params=None):
        self._maybe_load(params)
        ms, new_rnn = self._policy_single(graph, rnn_state)
        action = torch.empty(self.n_agents, 2, device=self.device)
        K.policy_head(ms, None, None, action, None, None, self.n_agents, 1)
        return action, new_rnn

    def step(self, graph: GraphsTuple, rnn_state, key, params=None):
        self._maybe_load(params)
        ms, new_rnn = self._policy_single(graph, rnn_state)
        from .. import ops_env as OE
        eps = torch.empty(self.n_agents, 2, device=self.device)
        OE.randn(int(key), 0, eps.view(-1))
        action = torch.empty(self.n_agents, 2, device=self.device)
        log_pi = torch.empty(self.n_agents, device=self.device)
        K.policy_head(ms, eps, None, action, log_pi, None, self.n_agents, 0)
        return action, log_pi, new_rnn

    # ---- collect / update ----
    def _seeds(self, keys) -> torch.Tensor:
        if torch.is_tensor(keys):
            return keys.to(self.device, torch.int64)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(keys).astype(np.uint64).view(np.int64))).to(self.device)

    def _scene_start(self, scenes, scene_ids, jitter, B_local: int, scene_of=None):
        """the engine's `start` of a collect call: None without scenes (the sampled reset), else (scenes, ids, jitter).  Episode b
        starts in scene scene_ids[b]; without a list, in scene g % S of its GLOBAL env index g = rank * B_local + b, so that the
        union over the ranks is what one device would run for the global batch.  scene_of (one int per key, this rank's window
        of env.scenes.mix_assignment) asks for a mix instead: episode b starts at its sampled reset where scene_of[b] < 0 and in
        scene scene_of[b] otherwise (env.scenes.SceneMix).  scene_of = an env.scenes.SceneDraw (ScenePool.drawn of the device
        tensor ScenePool.draw returned for this rank's window, `scenes` being that priority pool) asks for the same mix without a
        host copy (env.scenes.SceneMixDrawn); the validity bits of the scored rollout go to its flags."""
        from ..env.scenes import SceneDraw
        if scenes is None:
            if scene_ids is not None or scene_of is not None or float(jitter) != 0.0:
                raise ValueError("scene_ids / scene_of / jitter need scenes: without them the episodes start at the sampled reset")
            return None
        drawn, scene_of = (scene_of, None) if isinstance(scene_of, SceneDraw) else (None, scene_of)
        if drawn is not None:
            if scene_ids is not None:
                raise ValueError("scene_of and scene_ids exclude each other: a mix names every env's scene itself")
            if not getattr(scenes, "priority", False):
                raise ValueError("a drawn scene_of needs scenes=ScenePool(..., priority=True), the pool whose draw() it is")
            if tuple(drawn.scene_of.shape) != (B_local,):
                raise ValueError(f"scene_of must have one entry per key ({B_local}), got shape {tuple(drawn.scene_of.shape)}")
        if scene_of is not None:
            if scene_ids is not None:
                raise ValueError("scene_of and scene_ids exclude each other: a mix names every env's scene itself")
            if np.shape(scene_of) != (B_local,):
                raise ValueError(f"scene_of must have one entry per key ({B_local}), got shape {np.shape(scene_of)}")
        cfg, mine = scenes.cfg, self._env.cfg
        if (cfg.kind, cfg.n_agents, cfg.n_obs) != (mine.kind, mine.n_agents, mine.n_obs):
            raise ValueError(f"scenes of env kind {cfg.kind} with {cfg.n_agents} agents and {cfg.n_obs} obstacles do not fit this "
                             f"algo's env (kind {mine.kind}, {mine.n_agents} agents, {mine.n_obs} obstacles)")
        if drawn is not None:
            return scenes.mix_drawn(drawn.scene_of, drawn.flags, jitter)
        if scene_of is not None:
            return scenes.mix(scene_of, jitter)
        if scene_ids is None and self.world > 1:
            scene_ids = (self.rank * B_local + np.arange(B_local)) % scenes.S
        return scenes.start(scene_ids, jitter)

    def _wrap(self, ro: EN.RolloutData, env=None) -> Rollout:
        ro.finalize()
        env = self._env if env is None else env
        r = Rollout(_LazyGraphs(env, ro, 0), ro.actions, self._unpack_carry(ro.rnn_states), ro.rewards, ro.costs,
                    torch.zeros(ro.B, ro.T, dtype=torch.bool, device=self.device), ro.log_pis, _LazyGraphs(env, ro, 1))
        self._last_rollouts = getattr(self, "_last_rollouts", {})
        self._last_rollouts[id(r.actions)] = ro
        return r

    def collect(self, params, keys, scenes=None, scene_ids=None, jitter: float = 0.0, scene_of=None) -> Rollout:
        """algo.collect(params, keys): one stochastic rollout per key (informarl.py:254-256).  scenes (env.Scenes): the
        episodes — and those of the deterministic companion rollout — start in the given scenes instead of at the sampled
        reset (_scene_start); with scene_of only the envs it names do, and the companion rollout gets the same mix with its own
        seeds; scene_of may be what a priority pool drew, on the device (ScenePool.drawn).  Not in the reference."""
        self._maybe_load(params)
        seeds = self._seeds(keys)
        start = self._scene_start(scenes, scene_ids, jitter, int(seeds.shape[0]), scene_of)
        # the deterministic rollout that update() needs for the constraint-value targets (dgppo.py:139-141) uses the same
        # parameters as this collect: it is launched alongside on a second stream and handed to update()
        det_seeds = self._seeds(self._draw_keys(int(seeds.shape[0])))
        ro, det = self.engine.rollout_pair(seeds, det_seeds, noise_seed=int(self._rng.integers(1, 2 ** 62)),
                                           **({} if start is None else {"start": start}))
        self._pending_det = (ro, det)
        return self._wrap(ro)

    def collect_deterministic(self, keys, env=None, scenes=None, scene_ids=None, jitter: float = 0.0) -> Rollout:
        eng = self.engine
        if env is not None and env is not self._env:
            assert env.cfg.kind == self._env.cfg.kind and env.num_agents == self.n_agents
        seeds = self._seeds(keys)
        pend = getattr(self, "_pending_det", None)
        if pend is not None and pend[1].B == int(seeds.shape[0]):
            # this rollout reuses the record buffers of the deterministic rollout that collect() prepared for update():
            # drop the hand-over, update() will produce its own
            self._pending_det = None
        ro = eng.rollout(seeds, False, start=self._scene_start(scenes, scene_ids, jitter, int(seeds.shape[0])))
        return self._wrap(ro, env)

    def collect_stochastic(self, keys, env=None, scenes=None, scene_ids=None, jitter: float = 0.0) -> Rollout:
        """stochastic test rollouts (test.py:78-83 with --stochastic: algo.step inside test_rollout), batched"""
        if env is not None and env is not self._env:
            assert env.cfg.kind == self._env.cfg.kind and env.num_agents == self.n_agents
        seeds = self._seeds(keys)
        ro = self.engine.rollout(seeds, True, noise_seed=int(self._rng.integers(1, 2 ** 62)),
                                 start=self._scene_start(scenes, scene_ids, jitter, int(seeds.shape[0])))
        return self._wrap(ro, env)

    def rollout_record(self, rollout: Rollout, what: str = "rollout_record") -> EN.RolloutData:
        """the device record behind a Rollout that one of this algo's collect methods returned (until update() consumes it)"""
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError(f"{what}() needs a Rollout produced by this algo's collect methods")
        return ro

    def mine_scenes(self, rollout: Rollout, back: int = 8, thresh: float = 1e-6, max_scenes=None, names=None):
        """the failure scenes of a rollout that one of this algo's collect methods returned (env.Scenes.mine on its record): for
        every episode that becomes unsafe at some step >= 1, the state `back` steps before as a scene; None when there is none.
        Not in the reference."""
        if self._env.cfg.is_vmas:
            raise ValueError("mine_scenes: VMASReverseTransport has no scene entry point")
        from ..env.scenes import Scenes
        return Scenes.mine(self._env, self.rollout_record(rollout, "mine_scenes"), back=back, thresh=thresh, max_scenes=max_scenes,
                           names=names)

    def collect_shielded(self, keys, env=None, grid: int = 8, us=None, vs=None, margin: float = 0.0, scenes=None, scene_ids=None,
                         jitter: float = 0.0):
        """-> (Rollout, ShieldLog): deterministic test episodes in which every agent's action passes through the learned barrier
        as a runtime filter (Engine.rollout_shielded): the policy's action is kept where cbf_deriv of the agent's own Vh
        (dgppo.py:246-250) is <= -margin for it, otherwise replaced by the nearest admissible action of the grid us x vs
        (default: linspace(-1, 1, grid) in fp32 on both axes), or by the least violating one where nothing is admissible.  The
        Rollout is a deterministic one in every respect (landscapes, render_video); the log says what the shield did.  Not in
        the reference."""
        self.engine.require_landscape("collect_shielded")
        if env is not None and env is not self._env:
            assert env.cfg.kind == self._env.cfg.kind and env.num_agents == self.n_agents
        us = _grid_axis("collect_shielded", "us", us, grid, 1.0, lo=-1.0)
        vs = _grid_axis("collect_shielded", "vs", vs, grid, 1.0, lo=-1.0)
        if not np.isfinite(float(margin)):
            raise ValueError("collect_shielded: margin must be finite")
        seeds = self._seeds(keys)
        ro, log = self.engine.rollout_shielded(seeds, us, vs, float(margin),
                                               start=self._scene_start(scenes, scene_ids, jitter, int(seeds.shape[0])))
        r = self._wrap(ro, env)
        em = lambda x: x.transpose(0, 1).contiguous().cpu().numpy()
        return r, ShieldLog(em(log["policy_action"]), ro.actions.cpu().numpy(), em(log["index"]), em(log["flag"]), em(log["h"]),
                            em(log["Vh"]), us, vs, float(margin), float(self.engine.hp.alpha), float(self.engine.cfg.dt))

    def vh_landscape(self, rollout: Rollout, index: int, agent: int, frames=None, nx: int = 64, ny: int = 64, xs=None,
                     ys=None) -> Landscape:
        """The learned constraint-value function of `agent` over a grid of positions, in frozen frames of episode `index` of a
        rollout that collect_deterministic / collect_stochastic returned: in every frame the agent is moved to each grid
        point (velocity kept, LiDAR cast again) and Vh evaluated with the carry of that step.  frames: frame numbers in
        [0, T) (default: all); xs / ys: grid lines (default: linspace(0, area_size, nx / ny) in fp32).  Not in the reference:
        it is the producer of what its renderer draws as viz_opts["cbf"] (dgppo/env/plot.py:348-372,437-447)."""
        self.engine.require_landscape()
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError("vh_landscape() needs a Rollout produced by this algo's collect methods")
        area = float(self._env.cfg.area_size)
        xs, ys = _grid_axis("vh_landscape", "xs", xs, nx, area), _grid_axis("vh_landscape", "ys", ys, ny, area)
        frames = np.arange(ro.T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
        Vh = self.engine.vh_landscape(ro, int(index), int(agent), frames, xs, ys)
        return Landscape(xs, ys, Vh.cpu().numpy(), int(agent), frames.astype(np.int64))

    def cost_landscape(self, rollout: Rollout, index: int, agent: int, frames=None, nx: int = 64, ny: int = 64, xs=None,
                       ys=None) -> CostLandscape:
        """The environment's own cost h = get_cost over the grid vh_landscape sweeps (same arguments and defaults): in every
        frame `agent` is moved to each grid point (LiDAR cast again) and the cost of every agent evaluated.  It is what the
        learned Vh is supposed to bound (Vh >= h), and it needs no network: every algorithm has it (for HCBFCRPO it is the
        hand-crafted CBF itself)."""
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError("cost_landscape() needs a Rollout produced by this algo's collect methods")
        area = float(self._env.cfg.area_size)
        xs, ys = _grid_axis("cost_landscape", "xs", xs, nx, area), _grid_axis("cost_landscape", "ys", ys, ny, area)
        frames = np.arange(ro.T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
        cost = self.engine.cost_landscape(ro, int(index), int(agent), frames, xs, ys)
        return CostLandscape(xs, ys, cost.cpu().numpy(), int(agent), frames.astype(np.int64))

    def rollout_landscape(self, rollout: Rollout, index: int, agent: int, frames=None, nx: int = 64, ny: int = 64, xs=None,
                          ys=None, horizon: int = 32) -> RolloutLandscape:
        """What Vh is trained to predict, over the grid vh_landscape sweeps (same arguments and defaults): in every frame
        `agent` is moved to each grid point (velocity kept, LiDAR cast again) and the deterministic policy rolled `horizon`
        steps forward from there, with the actor's carry of that frame.  value is the discounted-to-max constraint return of
        those steps (compute_dec_ocp_gae, dgppo/algo/utils.py:38-45, at gae_lambda = 1, started from the last cost instead of
        a learned tail), worst the largest cost met: {worst >= 0} is the set of positions from which the policy becomes unsafe
        within the horizon — what {Vh >= 0} is meant to cover, and what the instantaneous cost_landscape understates.  It
        needs only the policy: every algorithm has it.  Not in the reference."""
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError("rollout_landscape() needs a Rollout produced by this algo's collect methods")
        area = float(self._env.cfg.area_size)
        xs, ys = _grid_axis("rollout_landscape", "xs", xs, nx, area), _grid_axis("rollout_landscape", "ys", ys, ny, area)
        frames = np.arange(ro.T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
        value, worst = self.engine.rollout_landscape(ro, int(index), int(agent), frames, xs, ys, int(horizon))
        return RolloutLandscape(xs, ys, value.cpu().numpy(), worst.cpu().numpy(), int(agent), frames.astype(np.int64),
                                int(horizon), float(self.engine.hp.gamma))

    def collect_lookahead_shielded(self, keys, env=None, grid: int = 8, us=None, vs=None, margin: float = 0.0,
                                   horizon: int = 8, rounds: int = 1, scenes=None, scene_ids=None, jitter: float = 0.0):
        """-> (Rollout, LookaheadShieldLog): deterministic test episodes in which every agent's action passes through a
        lookahead filter (Engine.rollout_lookahead_shielded): for the policy's action and every action of the grid us x vs
        (default: linspace(-1, 1, grid) in fp32 on both axes) the environment is forked, the candidate played, and the policy
        rolled `horizon` steps on; the policy's action is kept where the agent's own worst cost over those steps is <= -margin,
        otherwise replaced by the nearest admissible grid action, or by the least bad one where nothing is admissible.  It
        filters on what Vh is meant to predict, not on the prediction, and needs only the simulator and the policy: every
        algorithm has it.  An agent's candidates are judged with everyone else playing the policy (with rounds >= 2 the joint
        action the agents settle on is rolled as well: below), and the what-if rollouts run past the episode's end.  The Rollout is a deterministic one in every respect (landscapes, render_video); the log
        says what the shield did.  Not in the reference.
        rounds >= 2 -> (Rollout, JointLookaheadShieldLog): the agents' picks are re-judged jointly, up to `rounds` rounds per
        step (Engine.lookahead_select_rounds): the joint action held is rolled as everyone's candidate 0, and in every round
        after the first one agent per environment may still move.  The log's `joint` says per step whether the joint action
        that was played had been rolled (2: rolled and admissible for every agent, 1: rolled and not admissible, 0: not
        rolled — the rounds ran out while agents were still moving), `rounds_used` how many rounds judged the step."""
        if env is not None and env is not self._env:
            assert env.cfg.kind == self._env.cfg.kind and env.num_agents == self.n_agents
        what = "collect_lookahead_shielded"
        us, vs = _grid_axis(what, "us", us, grid, 1.0, lo=-1.0), _grid_axis(what, "vs", vs, grid, 1.0, lo=-1.0)
        if not np.isfinite(float(margin)):
            raise ValueError(f"{what}: margin must be finite")
        if int(horizon) < 1:
            raise ValueError(f"{what}: horizon must be >= 1 (got {horizon})")
        if int(rounds) < 1:
            raise ValueError(f"{what}: rounds must be >= 1 (got {rounds})")
        em = lambda x: x.transpose(0, 1).contiguous().cpu().numpy()
        seeds = self._seeds(keys)
        start = self._scene_start(scenes, scene_ids, jitter, int(seeds.shape[0]))
        if int(rounds) == 1:
            ro, log = self.engine.rollout_lookahead_shielded(seeds, us, vs, int(horizon), float(margin), start=start)
            r = self._wrap(ro, env)
            return r, LookaheadShieldLog(em(log["policy_action"]), ro.actions.cpu().numpy(), em(log["index"]), em(log["flag"]),
                                         em(log["s"]), us, vs, float(margin), int(horizon))
        ro, log = self.engine.rollout_lookahead_shielded(seeds, us, vs, int(horizon), float(margin), rounds=int(rounds), start=start)
        r = self._wrap(ro, env)
        return r, JointLookaheadShieldLog(em(log["policy_action"]), ro.actions.cpu().numpy(), em(log["index"]), em(log["flag"]),
                                          em(log["s"]), us, vs, float(margin), int(horizon), em(log["joint"]),
                                          em(log["rounds_used"]), int(rounds))

    def action_landscape(self, rollout: Rollout, index: int, agent: int, frames=None, nu: int = 32, nv: int = 32, us=None,
                         vs=None) -> ActionLandscape:
        """The discrete control barrier condition the advantage is shaped by (dgppo.py:246-250), over a grid of actions of
        `agent` in frames of episode `index` of a rollout that collect_deterministic / collect_stochastic returned: in every
        frame t the agent's state is stepped with each grid action (everyone else keeps their recorded action), Vh is evaluated
        on that next graph with the carry of step t + 1, and cbf = (Vh_next - Vh[t]) / dt + alpha * Vh[t].  frames: frame
        numbers in [0, T) (default: all); us / vs: grid lines of the two action components (default: linspace(-1, 1, nu / nv) in
        fp32).  Not in the reference."""
        self.engine.require_landscape("action_landscape")
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError("action_landscape() needs a Rollout produced by this algo's collect methods")
        us = _grid_axis("action_landscape", "us", us, nu, 1.0, lo=-1.0)
        vs = _grid_axis("action_landscape", "vs", vs, nv, 1.0, lo=-1.0)
        frames = np.arange(ro.T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
        cbf, Vh_next, Vh = self.engine.action_landscape(ro, int(index), int(agent), frames, us, vs)
        actions = np.clip(ro.actions[int(index), :, int(agent)].cpu().numpy()[frames], -1.0, 1.0).astype(np.float32)
        return ActionLandscape(us, vs, cbf.cpu().numpy(), Vh_next.cpu().numpy(), Vh.cpu().numpy(), actions, int(agent),
                               frames.astype(np.int64), float(self.engine.hp.alpha), float(self.engine.cfg.dt))

    def action_rollout_landscape(self, rollout: Rollout, index: int, agent: int, frames=None, nu: int = 32, nv: int = 32,
                                 us=None, vs=None, horizon: int = 32) -> ActionRolloutLandscape:
        """What the actions action_landscape sweeps lead to, measured (same grid arguments and defaults): in every frame t of
        episode `index` of a rollout that one of this algo's collect methods returned, `agent` plays each grid action for ONE
        step — everyone else their recorded action — and the deterministic policy is rolled on until the costs of the
        `horizon` states after that step are known.  value / worst fold them as rollout_landscape does and hold every agent's
        row: the swept agent's own row says which actions doom the agent itself within the horizon (the lookahead shield's
        criterion), the other rows what its single action does to its neighbours.  It needs the simulator and the policy only:
        every algorithm has it.  The what-if rollouts run past the episode's end and follow the unshielded policy whatever
        produced the rollout.  Not in the reference."""
        ro = getattr(self, "_last_rollouts", {}).get(id(rollout.actions))
        if ro is None:
            raise ValueError("action_rollout_landscape() needs a Rollout produced by this algo's collect methods")
        us = _grid_axis("action_rollout_landscape", "us", us, nu, 1.0, lo=-1.0)
        vs = _grid_axis("action_rollout_landscape", "vs", vs, nv, 1.0, lo=-1.0)
        frames = np.arange(ro.T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
        value, worst = self.engine.action_rollout_landscape(ro, int(index), int(agent), frames, us, vs, int(horizon))
        actions = np.clip(ro.actions[int(index), :, int(agent)].cpu().numpy()[frames], -1.0, 1.0).astype(np.float32)
        return ActionRolloutLandscape(us, vs, value.cpu().numpy(), worst.cpu().numpy(), actions, int(agent),
                                      frames.astype(np.int64), int(horizon), float(self.engine.hp.gamma))

    def update(self, rollout: Rollout, step: int) -> dict:
        ro = self._last_rollouts.pop(id(rollout.actions), None)
        if ro is None:
            raise ValueError("update() needs a Rollout produced by this algo's collect()")
        self._last_rollouts.clear()
        # deterministic rollout for the constraint-value targets (dgppo.py:139-141): produced next to collect()
        pend = getattr(self, "_pending_det", None)
        self._pending_det = None
        if pend is not None and pend[0] is ro:
            det = pend[1]
        else:
            det = self.engine.rollout(self._seeds(self._draw_keys(ro.B)), False)
        info = {}
        for _ in range(self.epoch_ppo):                      # dgppo.py:154-172: every epoch reshuffles and recomputes the targets
            # with the current parameters; the det rollout is shared (:140-141)
            info = self.engine.update(ro, det, int(step), self._perm(ro.B))
        return info

    # ---- checkpoints: {dir}/{step}/{actor,Vl,Vh}.pkl with flax-named params (informarl_lagr.py:311-327) ----
    def save(self, save_dir: str, step: int):
        model_dir = os.path.join(save_dir, str(step))
        os.makedirs(model_dir, exist_ok=True)
        p = self.params
        for fname, key in (("actor.pkl", "policy"), ("Vl.pkl", "Vl"), ("Vh.pkl", "Vh")):
            with open(os.path.join(model_dir, fname), "wb") as f:
                CK.save_tree(p[key], f)

    def load(self, load_dir: str, step: int):
        path = os.path.join(load_dir, str(step))
        for fname, key in (("actor.pkl", "policy"), ("Vl.pkl", "Vl"), ("Vh.pkl", "Vh")):
            with open(os.path.join(path, fname), "rb") as f:   # weights-only unpickler: nothing in the file is executed
                self.engine.nets[key].load_tree(CK.load_tree(f))

    # ---- the whole training state, to continue a stopped run (not in the reference; InforMARL, InforMARLLagr and HCBFCRPO
    # inherit it): the engine's buffers and every generator that decides a later batch, stored as numbers ----
    def state_dict(self) -> dict:
        return {"engine": self.engine.state_dict(), "rng": CK.generator_state(self._rng),
                "perm_rng": CK.generator_state(self._perm_rng), "np_random": CK.global_numpy_state()}

    def load_state_dict(self, d: dict) -> None:
        """on a constructed algo: overrides what construction drew (the entropy noise and the global np.random it came from)"""
        for k in ("engine", "rng", "perm_rng", "np_random"):
            if k not in d:
                raise ValueError(f"algo state has no '{k}' entry")
        self.engine.load_state_dict(d["engine"])             # ValueError before anything changes if it does not fit
        CK.set_generator_state(self._rng, d["rng"])
        CK.set_generator_state(self._perm_rng, d["perm_rng"])
        CK.set_global_numpy_state(d["np_random"])
        self._pending_det = None                             # rollouts of the parameters that were just replaced
        self._last_rollouts = {}

    def save_state(self, path: str):
        CK.save_state(self.state_dict(), path)

    def load_state(self, path: str):
        self.load_state_dict(CK.load_state(path))
