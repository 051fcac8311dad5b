"""Batched DGPPO engine: rollout collection and the update, orchestrating the HIP kernels (no torch arithmetic on the
hot path — torch tensors are storage, copies/transposes are data movement).

Reference behaviour reproduced (file:line relative to /root/reference):
  rollout / test_rollout            dgppo/trainer/utils.py:22-86   (pre-step carry stored when stochastic, post-step when det)
  DGPPO.update / update_inner       dgppo/algo/dgppo.py:136-294
  update_Vl / update_policy         dgppo/algo/informarl.py:357-457
  update_Vh                         dgppo/algo/dgppo.py:296-321
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Optional

import numpy as np
import os
import torch

from . import _native as N
from . import nets
from . import ops_algo as OA
from . import ops_env as OE
from . import ops_nn as K
from .utils import checkpoint as CK


@dataclasses.dataclass
class Hyper:
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_eps: float = 0.25
    coef_ent: float = 1e-2
    max_grad_norm: float = 2.0
    lr_actor: float = 3e-4
    lr_Vl: float = 1e-3
    lr_Vh: float = 1e-3
    batch_size: int = 16384
    rnn_step: int = 16
    alpha: float = 10.0
    cbf_eps: float = 1e-2
    cbf_weight: float = 1.0
    cbf_schedule: bool = True
    train_steps: int = 100000
    actor_gnn_layers: int = 2
    Vl_gnn_layers: int = 2
    Vh_gnn_layers: int = 1
    use_rnn: bool = True              # --no-rnn: networks without a recurrent cell (policy.py:31-32, value.py:38-39)
    use_lstm: bool = False            # --use-lstm: flax LSTMCell instead of GRUCell in the policy and Vl (rnn.py:22-24)
    rnn_layers: int = 1               # stacked cells (dgppo/nn/rnn.py:17-29); the DGPPO constraint-value net keeps ONE
    lagr_init: float = 0.78           # InforMARL-Lagrangian: initial multipliers, their step size (informarl_lagr.py:52-53)
    lr_lagr: float = 1e-7
    cost_weight: float = 0.0          # InforMARL: weight of sum(max(cost, 0)) in the stage cost (informarl.py:329)
    cost_schedule: bool = False       # InforMARL: x5 at 50 % and again x5 at 75 % of train_steps (informarl.py:189-198)


class RolloutData:
    """Compact rollout record (SURVEY §7 'compact rollout storage'): time-major while collecting, env-major afterwards.  The
    actor carry stays time-major (rnn_tm): the update reads it where the rollout wrote it (ops_nn.H0Map), and the env-major
    views of it (_rnn_em, rnn_states) are made on first access after a rollout, in a buffer that is allocated once."""
    _rnn_em_buf = None          # [B, T+2, n, HC], persistent
    _rnn_em_fresh = False       # _rnn_em_buf holds this rollout's carries

    def __init__(self, cfg: N.EnvCfg, B: int, T: int, device, stochastic: bool, carry_dim: int = nets.HID):
        n = cfg.n_agents
        self.cfg, self.B, self.T, self.stochastic = cfg, B, T, stochastic
        z = lambda *s: torch.empty(*s, device=device)
        # the env state (ops_env.record_fields): step_tm / step hold the per-step fields time-major [T+1, B, ...] / env-major
        # [B, T+1, ...] (after finalize()), env the per-env ones [B, ...].  Each is also an attribute (agent_tm, hits_tm,
        # body_tm; agent, hits, body; goal, obst, scene), None where the kind has no such field.
        step, env = OE.record_fields(cfg)
        self.step_tm = {k: z(T + 1, B, *shape) for k, shape in step.items()}
        self.env = {k: z(B, *shape) for k, shape in env.items()}
        self.step: Dict[str, torch.Tensor] = {}
        for k in OE.STEP_FIELDS:
            setattr(self, k + "_tm", self.step_tm.get(k))
            setattr(self, k, None)
        for k in OE.ENV_FIELDS:
            setattr(self, k, self.env.get(k))
        self.action_tm = z(T, B, n, 2)
        self.log_pi_tm = z(T, B, n) if stochastic else None
        # packed actor carry [h_0 | h_1 | ...] of the stacked cells: rnn_tm, slots 0..T, is the rollout's.  It is the head of a
        # [T+2, ...] allocation whose last slot is spare: the value pre-pass puts the final carry behind the T stored ones of
        # either kind of record and reads all T+1 in place (Engine.values_prepass).
        self._rnn_all = torch.zeros(T + 2, B, n, carry_dim, device=device)
        self.rnn_tm = self._rnn_all[:T + 1]
        self.reward_tm = z(T, B)
        self.cost_tm = z(T, B, n, cfg.n_cost)
        self._env_major = False
        # the env state of every step of the time-major record (views, made once: the rollout loop is bound by its host side)
        views = {k: v.unbind(0) for k, v in self.step_tm.items()}
        self.states_tm = [OE.State({k: v[t] for k, v in views.items()}, self.env) for t in range(T + 1)]

    def prefix(self, B: int) -> "RolloutData":
        """the time-major record of the first B envs of this one, on the same storage: every step of every field is a dense
        [B, ...] view, the steps keep this record's stride (the shield rounds roll blocks of any size in one block record)"""
        if not 1 <= B <= self.B:
            raise ValueError(f"RolloutData.prefix: {B} envs of a record of {self.B}")
        if B == self.B:
            return self
        v = object.__new__(RolloutData)
        v.cfg, v.B, v.T, v.stochastic = self.cfg, B, self.T, self.stochastic
        v.step_tm = {k: x[:, :B] for k, x in self.step_tm.items()}
        v.env = {k: x[:B] for k, x in self.env.items()}
        v.step = {}
        for k in OE.STEP_FIELDS:
            setattr(v, k + "_tm", v.step_tm.get(k))
            setattr(v, k, None)
        for k in OE.ENV_FIELDS:
            setattr(v, k, v.env.get(k))
        cut = lambda x: None if x is None else x[:, :B]
        v.action_tm, v.log_pi_tm, v._rnn_all = cut(self.action_tm), cut(self.log_pi_tm), cut(self._rnn_all)
        v.rnn_tm = v._rnn_all[:self.T + 1]
        v.reward_tm, v.cost_tm = cut(self.reward_tm), cut(self.cost_tm)
        v._env_major = False
        v.states_tm = [OE.State({k: x[t] for k, x in v.step_tm.items()}, v.env) for t in range(self.T + 1)]
        return v

    def finalize(self):
        """time-major -> env-major copies (pure data movement).  The env-major buffers are allocated once per record and
        rewritten in place afterwards, so that device pointers stay valid for captured HIP graphs of the update."""
        if self._env_major:
            return self

        def tr(name, x):
            if x is None:
                return None
            cur = getattr(self, name, None)
            want = (x.shape[1], x.shape[0]) + tuple(x.shape[2:])
            if cur is None or tuple(cur.shape) != want:
                cur = torch.empty(want, device=x.device, dtype=x.dtype)
            cur.copy_(x.transpose(0, 1))
            return cur
        for k, v in self.step_tm.items():                             # agent [B, T+1, n, sd], hits [B, T+1, n, k, 2], ...
            self.step[k] = tr(k, v)
            setattr(self, k, self.step[k])
        self.actions = tr("actions", self.action_tm)                  # [B, T, n, 2]
        self.log_pis = tr("log_pis", self.log_pi_tm) if self.stochastic else None
        self._rnn_em_fresh = False                                    # the carry: _rnn_em / rnn_states, on first access
        self.rewards = tr("rewards", self.reward_tm)                  # [B, T]
        self.costs = tr("costs", self.cost_tm)                        # [B, T, n, n_cost]
        self._env_major = True
        return self

    @property
    def _rnn_em(self) -> torch.Tensor:
        """[B, T+2, n, HC]: the env-major copy of the carry record (slot for slot, the spare one included), made on first
        access after finalize()"""
        if not self._rnn_em_fresh:
            x = self._rnn_all
            want = (x.shape[1], x.shape[0]) + tuple(x.shape[2:])
            cur = self._rnn_em_buf
            if cur is None or tuple(cur.shape) != want:
                cur = torch.empty(want, device=x.device, dtype=x.dtype)
            cur.copy_(x.transpose(0, 1))
            self._rnn_em_buf, self._rnn_em_fresh = cur, True
        return self._rnn_em_buf

    @property
    def rnn_states(self) -> torch.Tensor:
        """[B, T, n, HC] stored carry of step t: pre-step (rollout, trainer/utils.py:46-51) or post-step (test_rollout, :71-77)"""
        T = self.T
        return self._rnn_em[:, :T] if self.stochastic else self._rnn_em[:, 1:T + 1]


class OptState:
    def __init__(self, n: int, device):
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.state = torch.zeros(N.OPT_STATE_FLOATS, device=device)


class Engine:
    def __init__(self, cfg: N.EnvCfg, hyper: Hyper, device, T: int = 128,
                 allreduce: Optional[Callable[[torch.Tensor], None]] = None, world: int = 1, prepass_graphs: int = 1 << 20,
                 use_graphs: bool = False, multi_stream: bool = False, algo: str = "dgppo", rank: int = 0,
                 fused_step: bool = True, lean_attn0: bool = True, carry_in_place: bool = True):
        self.cfg, self.hp, self.device, self.T = cfg, hyper, device, T
        assert algo in ("dgppo", "informarl", "hcbfcrpo", "informarl_lagr"), algo
        # "informarl" / "hcbfcrpo": no constraint-value network and no deterministic rollout (informarl.py, hcbfcrpo.py);
        # "informarl_lagr": a constraint-value network with global information and its own recurrent carry, trained on the
        # stochastic rollout, plus per-(agent, component) Lagrange multipliers (informarl_lagr.py)
        self.algo = algo
        # HIP-graph replay of the launch-bound rollout loop (18 small kernels per env step).  Opt-in because the record
        # buffers then belong to the engine: a RolloutData stays valid only until the next rollout of the same kind.
        self.use_graphs = use_graphs and os.environ.get("DGPPO_HIPGRAPH", "1") != "0"
        # run the Vl / Vh / policy updates of a minibatch on three HIP streams (they are independent)
        self.multi_stream = multi_stream and os.environ.get("DGPPO_MULTI_STREAM", "1") != "0"
        self._side_streams = None
        # one launch per rollout step for head sampling + env.step + the next step's features and layer-0 queries, where the
        # C ABI has such a kernel for the configuration (dgppo_env_act_step_feats_supported); else the four launches
        self.fused_step = bool(fused_step) and OE.act_step_feats_supported(cfg, nets.input_width(cfg), nets.H_HEADS)
        # the first layer's attention without edge features and saved weights (nets.Net); False: the general entry points
        self.lean_attn0 = bool(lean_attn0)
        # the Vh minibatch pass reads the deterministic record's carry rows in place, through the minibatch's env ids
        # (ops_nn.H0Map); False: the gathered copy h0_det of every minibatch, as before (tests compare the two)
        self.carry_in_place = bool(carry_in_place)
        self._ro_cache: Dict[tuple, dict] = {}
        self._upd_graph: dict = {}
        self.n_cost = cfg.n_cost              # 2, or 3 with MPEConnectSpread's connectivity cost
        # ONE flat fp32 buffer [g_policy | g_Vl | g_Vh | scalars]: each network's gradient buffer is a
        # 16-byte-aligned slice of it and the loss/metric sums of the minibatch (stats rows 0..2) sit at its tail, so the
        # data-parallel update needs a single all-reduce per minibatch.  Row 3 of the stats (the per-iteration safe count)
        # lies outside the reduced range.
        spec = [("policy", "policy", hyper.actor_gnn_layers, 2), ("Vl", "Vl", hyper.Vl_gnn_layers, 1)]
        if algo == "dgppo":
            spec.append(("Vh", "Vh", hyper.Vh_gnn_layers, self.n_cost))
        elif algo == "informarl_lagr":
            spec.append(("Vh", "Vhg", hyper.Vh_gnn_layers, self.n_cost))
        # recurrent options (train.py --no-rnn / --rnn-layers): the policy and Vl (and the Lagrangian Vh) stack rnn_layers
        # cells; DGPPO's constraint-value net is built with the ValueNet default of ONE layer (dgppo.py:83-95) and reads layer
        # 0 of the actor's carry
        def rnn_kw(name):
            if not hyper.use_rnn:
                return dict(rnn="none", rnn_layers=0)
            if name == "Vh" and algo == "dgppo":        # ValueNet(use_lstm=False) with the default single cell (dgppo.py:83-95)
                return dict(rnn="gru", rnn_layers=1)
            return dict(rnn="lstm" if hyper.use_lstm else "gru", rnn_layers=hyper.rnn_layers)
        sizes = [nets.make_layout(kind, cfg.node_dim, layers, n_out, **rnn_kw(k)).size for k, kind, layers, n_out in spec]
        offs, tot = [], 0
        for sz in sizes:
            offs.append(tot)
            tot += (sz + 3) // 4 * 4
        self.flat_grads = torch.zeros(tot + 4 * 8, device=device)
        self.n_reduced = tot + 3 * 8
        self.stats = self.flat_grads[tot:tot + 32].view(4, 8)
        built = {k: nets.Net(kind, cfg, layers, n_out, device, grads=self.flat_grads[o:o + sz], lean_attn0=self.lean_attn0, **rnn_kw(k))
                 for (k, kind, layers, n_out), o, sz in zip(spec, offs, sizes)}
        if algo == "informarl_lagr":
            self.lagr = torch.full((cfg.n_agents, self.n_cost), float(hyper.lagr_init), device=device)   # informarl_lagr.py:107
            self.lagr_sums = torch.zeros(cfg.n_agents * self.n_cost, device=device)
        self.policy, self.Vl, self.Vh = built["policy"], built["Vl"], built.get("Vh")
        self.HC = self.policy.carry_dim              # width of the stored actor carry
        self.opt = {k: OptState(net.layout.size, device) for k, net in self.nets.items()}
        self.arena = nets.Arena(device)
        # allreduce(flat): in-place SUM over the data-parallel ranks of the flat buffer above (dgppo_comm_allreduce_sum_f32 on
        # the caller's stream); the 1/world is applied inside dgppo_clip_adam_step (grad_scale), not by a separate pass
        self.allreduce = allreduce
        self.world, self.rank = int(world), int(rank)
        assert self.world >= 1 and (allreduce is not None or self.world == 1), "world > 1 needs an allreduce"
        assert 0 <= self.rank < self.world, f"rank {rank} outside world {world}"
        self.prepass_graphs = int(os.environ.get("DGPPO_PREPASS_GRAPHS", prepass_graphs))      # tuning override
        self.lam_pow = OA.lam_pow_table(hyper.gae_lambda, T, device)
        # the constant entropy noise of SURVEY A.7 (distribution.py:40: seed drawn once at trace time)
        self.eps_hat = torch.zeros(cfg.n_agents, 2, device=device)
        # envs whose reset could not place a valid scene within the kernels' loop bounds (dgppo_env_reset_checked): counted on
        # the device by every rollout, read at the iteration's one host sync (info) — training on such a batch is an error
        self.reset_failed = torch.zeros(1, dtype=torch.int32, device=device)
        # envs of a mixed start (env.scenes.SceneMix) whose scene stayed invalid and that kept their sampled reset instead
        # (dgppo_env_scene_mix): counted next to reset_failed, reported by info() as rollout/scene_fallback, never an error.
        # Under a pool of mined scenes (env.scenes.ScenePool) an empty ring slot holds NaN words and means "sampled reset", so
        # while the ring is not full the counter also holds the envs that drew an empty slot
        self.scene_fallback = torch.zeros(1, dtype=torch.int32, device=device)
        self._mix_used = False
        self._mix_pool = None
        self.grad_hook: Optional[Callable[[str, nets.Net, int], None]] = None   # (net name, net, minibatch) before the optimiser
        self._mb = 0

    @property
    def nets(self) -> Dict[str, nets.Net]:
        d = {"policy": self.policy, "Vl": self.Vl}
        if self.Vh is not None:
            d["Vh"] = self.Vh
        return d

    def set_entropy_noise(self, seed: int):
        OE.randn(seed, 0, self.eps_hat.view(-1))

    # ------------------------------------------------------------------------------------------------------------------
    # the whole training state (resuming a stopped run): parameters, optimiser moments, entropy noise, multipliers
    # ------------------------------------------------------------------------------------------------------------------
    _CFG_IDENTITY = ("kind", "n_agents", "n_obs", "n_rays", "top_k", "node_dim", "n_cost")

    def _identity(self) -> dict:
        """what a state dict must agree on with the engine it is loaded into, in the order it is compared.  Strings are
        uint8 arrays (the weights-only reader of utils/checkpoint.py takes no str leaves)."""
        ident = {"algo": CK.encode_str(self.algo)}
        ident.update({f"cfg.{k}": int(getattr(self.cfg, k)) for k in self._CFG_IDENTITY})
        for f in dataclasses.fields(Hyper):
            v = getattr(self.hp, f.name)
            ident[f"hyper.{f.name}"] = int(v) if isinstance(v, (bool, int)) else float(v)
        ident["T"], ident["world"] = int(self.T), int(self.world)
        ident.update({f"size.{k}": int(net.layout.size) for k, net in self.nets.items()})
        return ident

    def _state_tensors(self) -> Dict[str, torch.Tensor]:
        """every device buffer of the state, by its path in the state dict"""
        t = {}
        for k, net in self.nets.items():
            opt = self.opt[k]
            t.update({f"{k}/params": net.params, f"{k}/m": opt.m, f"{k}/v": opt.v, f"{k}/state": opt.state})
        t["eps_hat"] = self.eps_hat
        if self.algo == "informarl_lagr":
            t["lagr"] = self.lagr
        return t

    def state_dict(self) -> dict:
        """nested dict (str keys; numpy arrays, ints and floats as leaves) of everything an update reads and writes"""
        out = {"identity": self._identity()}
        for path, x in self._state_tensors().items():
            node = out
            *dirs, leaf = path.split("/")
            for d in dirs:
                node = node.setdefault(d, {})
            node[leaf] = x.detach().cpu().numpy().copy()
        return out

    def load_state_dict(self, d: dict) -> None:
        """ValueError naming the first identity field that differs, before any buffer is touched; then copies INTO the
        existing tensors — captured HIP graphs hold their addresses and read the loaded values on their next replay."""
        mine, theirs = self._identity(), d.get("identity", {})
        show = lambda v: repr(CK.decode_str(v)) if isinstance(v, np.ndarray) else repr(v)
        for k, v in mine.items():
            if k not in theirs:
                raise ValueError(f"state dict does not fit this engine: it has no identity field '{k}'")
            if not np.array_equal(np.asarray(v), np.asarray(theirs[k])):
                raise ValueError(f"state dict does not fit this engine: '{k}' is {show(theirs[k])} there, {show(v)} here")
        src = {}
        for path, x in self._state_tensors().items():
            node = d
            for part in path.split("/"):
                node = node.get(part) if isinstance(node, dict) else None
            if not isinstance(node, np.ndarray) or node.dtype != np.float32 or node.shape != tuple(x.shape):
                raise ValueError(f"state dict does not fit this engine: '{path}' is not a float32 array of shape {tuple(x.shape)}")
            src[path] = node
        for path, x in self._state_tensors().items():
            x.copy_(torch.from_numpy(src[path]).to(self.device))
        for net in self.nets.values():
            net.prepare()                       # the prepared GNN weights follow the parameters

    # ------------------------------------------------------------------------------------------------------------------
    # rollout
    # ------------------------------------------------------------------------------------------------------------------
    def _feats(self, tag, st: OE.State, n_env, n_time=1, slots=1, env_ids=None):
        """graph features of n_env x n_time states: dense [n_env, ...] states, or (slots = T + 1) the env-major record from
        st's first (env, step) on, of the envs env_ids if given"""
        f = nets.GraphFeats(self.cfg, n_env * n_time, self.arena, tag)
        return f.compute_record(st.step, slots, st.env, env_ids, n_env, n_time)

    def _rollout_steps(self, ro: RolloutData, eps, B: int, stochastic: bool, start: int = 0):
        """the env steps start .. ro.T - 1 of a rollout from the state and carry in slot `start` of the record: policy forward
        (GNN + GRU + head) and env.step, all on the current stream.  The step count is the record's (self.T in rollout(), the
        horizon in rollout_landscape(); lookahead_select() starts at slot 1, behind its forced first step)."""
        cfg, T, n = self.cfg, ro.T, self.cfg.n_agents
        tag = "ro" if stochastic else "rod"    # separate scratch per kind: the two rollouts may run on different streams
        if self.fused_step:
            # features and queries of step 0 from the stand-alone kernels; every step's launch then leaves those of the next
            # state in the same buffers, which the next forward reads
            pol, R = self.policy, B * n
            feats = self._feats(tag, ro.states_tm[start], B)
            Mcat, cvec = pol.pp("gnn0.Mcat"), pol.pp("gnn0.cvec")
            qt0 = pol.arena.get(f"{tag}.qt0", R, Mcat.shape[1])
            K.dense_fwd(feats.Xa, Mcat, cvec, qt0)
            for t in range(start, T):
                act = pol.forward(feats, n_seq=R, T=1, h0=ro.rnn_tm[t].view(R, self.HC), tag=tag,
                                  hs_out=ro.rnn_tm[t + 1].view(R, self.HC), train=False, qt0=qt0)
                nxt = dict(Xa=feats.Xa, Xo=feats.Xo, efeat=feats.efeat, emask=feats.emask, Fp=feats.Fp, Mcat=Mcat, cvec=cvec,
                           qt0=qt0, H=nets.H_HEADS) if t + 1 < T else {}      # nothing reads the features of the last state
                OE.act_step_feats(cfg, ro.states_tm[t], act["ms"], eps[t] if stochastic else None, ro.action_tm[t],
                                  ro.log_pi_tm[t] if stochastic else None, ro.states_tm[t + 1], ro.reward_tm[t], ro.cost_tm[t],
                                  **nxt)
                feats.edges_from_rows = cfg.state_dim == 4     # the step's edges are differences of the rows it wrote, too
            return
        for t in range(start, T):
            feats = self._feats(tag, ro.states_tm[t], B)
            act = self.policy.forward(feats, n_seq=B * n, T=1, h0=ro.rnn_tm[t].view(B * n, self.HC), tag=tag,
                                      hs_out=ro.rnn_tm[t + 1].view(B * n, self.HC), train=False)
            a_t = ro.action_tm[t].view(B * n, 2)
            if stochastic:
                K.policy_head(act["ms"], eps[t], None, a_t, ro.log_pi_tm[t].view(B * n), None, n, 0)
            else:
                K.policy_head(act["ms"], None, None, a_t, None, None, n, 1)
            OE.step(cfg, ro.states_tm[t], ro.action_tm[t], ro.states_tm[t + 1], ro.reward_tm[t], ro.cost_tm[t])

    def _start(self, seeds: torch.Tensor, st: OE.State, start=None):
        """slot 0 of a rollout's record: the sampled reset of seeds, or — start = (scenes, scene_ids | None, jitter), an
        env.scenes.SceneStart — the user-given scenes (ops_env.scene_start: env b in scene scene_ids[b], or b % S; agents moved by
        up to `jitter`, drawn from seeds).  Either way sensed, and envs without a valid scene counted in reset_failed.
        start = an env.scenes.SceneMix: the reset of every env, then the scenes of those scene_of names (ops_env.mixed_start);
        an env whose scene stays invalid keeps its reset and is counted in scene_fallback, not in reset_failed.
        start = an env.scenes.SceneMixDrawn: the same mix with the device scene_of a priority pool drew; the bits of the envs it
        names go to start.flags where that is given."""
        if start is None:
            return OE.reset(self.cfg, seeds, st, self.reset_failed)
        from .env.scenes import SceneMix, SceneMixDrawn
        if isinstance(start, SceneMixDrawn):                   # scene_of stays on the device: no copy, no sync
            self._mix_used, self._mix_pool = True, start.scenes
            return OE.mixed_start_drawn(self.cfg, seeds, st, start.scenes.dev, start.scene_of, float(start.jitter), start.flags,
                                        self.reset_failed, self.scene_fallback)
        if isinstance(start, SceneMix):
            self._mix_used = True
            # a pool of mined scenes (env.scenes.ScenePool): info() reports its fill next to scene_fallback
            self._mix_pool = start.scenes if hasattr(start.scenes, "fill") else None
            return OE.mixed_start(self.cfg, seeds, st, start.scenes.dev, start.scene_of, float(start.jitter), self.reset_failed,
                                  self.scene_fallback)
        scenes, scene_ids, jitter = start
        OE.scene_start(self.cfg, scenes.dev, scene_ids, seeds, float(jitter), st, None, self.reset_failed)

    def rollout(self, seeds: torch.Tensor, stochastic: bool, noise_seed: int = 0, start=None) -> RolloutData:
        """start: None, or where the episodes begin instead of at the reset (_start); everything after slot 0 is the same"""
        cfg, T = self.cfg, self.T
        B = int(seeds.shape[0])
        n = cfg.n_agents
        slot = None
        if self.use_graphs:
            # persistent record buffers per (B, kind): eager + capture on the first call, replayed afterwards
            slot = self._ro_cache.setdefault((B, stochastic), {"ro": None, "graph": None, "gen": -1, "calls": 0})
            if slot["ro"] is None:
                slot["ro"] = RolloutData(cfg, B, T, self.device, stochastic, self.HC)
            ro = slot["ro"]
            ro._env_major = False
        else:
            ro = RolloutData(cfg, B, T, self.device, stochastic, self.HC)
        self._start(seeds, ro.states_tm[0], start)                 # with the sense pass that fills hits_tm[0]
        ro.rnn_tm[0].zero_()                                   # init_rnn_state = zeros (informarl.py:115-124)
        eps = None
        if stochastic:
            # the sampling noise of step t is one row of world * B * n * 2 normals, of which this rank fills the window of
            # its envs: the union of the ranks' rollouts is the single-device rollout of the global batch
            eps = self.arena.get("ro.eps", T, B * n, 2)
            OE.randn_rows(noise_seed, eps.view(T, B * n * 2), self.world * B * n * 2, self.rank * B * n * 2)
        if slot is None:
            self._rollout_steps(ro, eps, B, stochastic)
            return ro
        slot["calls"] += 1
        if slot["graph"] is not None and slot["gen"] != self._arena_generation():
            slot["graph"] = None                               # a scratch buffer moved: the captured pointers are stale
        if slot["graph"] is not None:
            slot["graph"].replay()
            K.FLOPS[0] += slot.get("flops", 0.0)               # the replayed launches never pass through the Python wrappers
            return ro
        # first call (or stale graph): eager launches — they also size every scratch buffer — then capture the same loop
        # right away, so that the second call already replays (one warm-up iteration is enough for steady state)
        f0 = K.FLOPS[0]
        self._rollout_steps(ro, eps, B, stochastic)
        slot["flops"] = K.FLOPS[0] - f0
        if not slot.get("failed", False):
            graph = torch.cuda.CUDAGraph()
            try:
                # thread-local error mode: other threads (the RCCL watchdog of torch.distributed) keep issuing HIP calls
                # while this thread captures; in the default global mode those would invalidate the capture.
                # Capturing records the launches without executing them: the results of the eager pass above stand.
                f1 = K.FLOPS[0]
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    self._rollout_steps(ro, eps, B, stochastic)
                K.FLOPS[0] = f1 + slot["flops"]                 # capture records, the replay below executes once
                slot["graph"], slot["gen"] = graph, self._arena_generation()
                # the first launch of a ~2300-node graph uploads it to the device (~100 ms): pay that here, in the same
                # warm-up call (same inputs, so it rewrites the record with identical values)
                graph.replay()
            except Exception as ex:                             # keep training: eager launches are always correct
                slot["failed"] = True
                torch.cuda.synchronize()
                print(f"[dgppo_amd] HIP-graph capture of the rollout loop failed ({type(ex).__name__}: {ex}); "
                      f"continuing with eager launches", flush=True)
        return ro

    def _update_generation(self) -> int:
        """scratch buffers the minibatch step touches: the engine's arena and every network's"""
        return self.arena.generation + sum(net.arena.generation + net.ws_arena.generation for net in self.nets.values())

    def _arena_generation(self) -> int:
        """scratch buffers the rollout loop touches live in the engine's arena (features) and the policy's (activations)"""
        return self.arena.generation + self.policy.arena.generation

    def rollout_pair(self, seeds: torch.Tensor, det_seeds: torch.Tensor, noise_seed: int = 0, start=None):
        """the stochastic training rollout and the deterministic rollout of the same parameters (informarl.py:254-256 and
        dgppo.py:139-141).  They are independent, so with multi_stream they run on two HIP streams side by side.  Under a drawn mix
        (env.scenes.SceneMixDrawn) both read the same scene_of; only the stochastic one, whose record is scored, writes flags."""
        from .env.scenes import SceneMixDrawn
        det_start = start._replace(flags=None) if isinstance(start, SceneMixDrawn) else start
        if not (self.multi_stream and self.device.type == "cuda"):
            return self.rollout(seeds, True, noise_seed, start), self.rollout(det_seeds, False, start=det_start)
        main = torch.cuda.current_stream(self.device)
        s0, s1 = self._net_streams()[:2]
        out = [None, None]
        for k, (st, sd, stoch) in enumerate(((s0, seeds, True), (s1, det_seeds, False))):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                out[k] = self.rollout(sd, stoch, noise_seed if stoch else 0, start if stoch else det_start)
        main.wait_stream(s0)
        main.wait_stream(s1)
        return out[0], out[1]

    # ------------------------------------------------------------------------------------------------------------------
    # value pre-passes (dgppo.py:204-229, 262-264)
    # ------------------------------------------------------------------------------------------------------------------
    def _block_feats(self, tag, ro: RolloutData, e0, Eb, t0, n_time, env_ids=None):
        """features of steps t0 .. t0 + n_time - 1 of Eb envs of the env-major record: envs e0 .. e0 + Eb - 1, or env_ids"""
        envs = slice(e0, None) if env_ids is None else slice(None)
        st = OE.State({k: v[envs, t0] for k, v in ro.step.items()}, {k: v[envs] for k, v in ro.env.items()})
        return self._feats(tag, st, Eb, n_time, self.T + 1, env_ids)

    def _carry_mapped(self) -> bool:
        """the Vh minibatch pass reads the deterministic record's carry through ops_nn.H0Map: DGPPO with one actor GRU cell (the stored carry rows are
        Vh's own 64 floats) on the GPU, unless the engine was built with carry_in_place=False"""
        return (self.algo == "dgppo" and self.carry_in_place and self.hp.use_rnn and self.HC == nets.HID
                and self.device.type == "cuda")

    def _mb_carry(self, det: RolloutData, ids: torch.Tensor) -> K.H0Map:
        """the carry rows the Vh minibatch pass reads for the envs `ids` (int32, on the device): the stored carries of the
        deterministic record where the rollout wrote them — the post-step carry of step t is slot t + 1 of the time-major
        record"""
        tm = det.rnn_tm
        return K.H0Map(tm[1], tm.stride(1), tm.stride(0), self.T, self.cfg.n_agents, int(ids.numel()), ids=ids, n_env_src=det.B)

    def _vh_carry(self, ro: RolloutData, e0: int, Eb: int) -> torch.Tensor:
        """[Eb, T, n, H]: the carry the constraint-value net reads for (env, t), t < T — layer 0 of the actor's stored carry
        of that step (rnn.py:20: rnn_state[0]; pre-step in a stochastic record, post-step in a deterministic one)"""
        return ro.rnn_states[e0:e0 + Eb][..., :nets.HID]

    def _final_carry(self, ro: RolloutData, e0: int, Eb: int) -> torch.Tensor:
        """[Eb * n, HC]: the actor's packed carry after the last step — its GRU on next_graph[-1] from rnn_states[-1]
        (dgppo.py:222-226)"""
        T, n, HC = self.T, self.cfg.n_agents, self.HC
        fin = self._block_feats("fin", ro, e0, Eb, T, 1)
        if self.carry_in_place:                  # the stored carry of step T - 1, a dense block of the time-major record
            h_last = ro.rnn_tm[T - 1 if ro.stochastic else T, e0:e0 + Eb].view(Eb * n, HC)
        else:
            h_last = self.arena.get("pre.hlast", Eb * n, HC)
            h_last.view(Eb, n, HC).copy_(ro.rnn_states[e0:e0 + Eb, T - 1])
        hstar = self.arena.get("pre.hstar", Eb * n, HC)
        self.policy.forward(fin, n_seq=Eb * n, T=1, h0=h_last, tag="fin", hs_out=hstar, train=False)
        return hstar

    def values_prepass(self, ro: RolloutData, want_Vl: bool, want_Vh: bool = True):
        """-> Vl [B,T+1] (or None), Vh [B,T+1,n,nh] of one rollout, with the reference's carry conventions."""
        cfg, T, B = self.cfg, self.T, ro.B
        n, nh, H = cfg.n_agents, self.n_cost, nets.HID
        kind = "ro" if ro.stochastic else "det"      # persistent outputs (stable pointers for the captured update graph)
        Vl_buf = self.arena.get(f"tg.Vl.{kind}", B, T + 1) if want_Vl else None
        Vh_buf = self.arena.get(f"tg.Vh.{kind}", B, T + 1, n, nh) if want_Vh else None
        block = max(1, min(B, self.prepass_graphs // (T + 1)))
        for e0 in range(0, B, block):
            Eb = min(block, B - e0)
            feats = self._block_feats("pre", ro, e0, Eb, 0, T + 1)
            if want_Vl:
                act = self.Vl.forward(feats, n_seq=Eb, T=T + 1, h0=None, tag="pre", train=False)
                Vl_buf[e0:e0 + Eb].copy_(act["v"].view(Eb, T + 1))
            if not want_Vh:
                continue
            HC = self.HC
            hstar = self._final_carry(ro, e0, Eb)
            restore = False
            # the constraint-value net has ONE cell and reads layer 0 of the actor's packed carry (rnn.py:20: rnn_state[0])
            if not self.hp.use_rnn:
                h0 = None
            elif HC == H and self.carry_in_place:
                # the T stored carries of an env lie one time stride apart in the time-major record: the final carry goes into
                # the slot behind them and the kernel reads all T+1 through the map.  That slot is the spare one (T+1) of a
                # deterministic record.  In a stochastic record it is slot T, which holds the rollout's carry after the last
                # step: that waits in the spare slot while Vh reads and is put back below, so outside this function rnn_tm is
                # always the rollout's.  h_last read the slot before.
                s0 = 0 if ro.stochastic else 1
                tm = ro._rnn_all
                if ro.stochastic:
                    tm[T + 1, e0:e0 + Eb].copy_(tm[T, e0:e0 + Eb])
                tm[s0 + T, e0:e0 + Eb].copy_(hstar.view(Eb, n, H))
                h0 = K.H0Map(tm[s0, e0:], tm.stride(1), tm.stride(0), T + 1, n, Eb, n_env_src=B - e0)
                restore = ro.stochastic
            elif HC == H:
                # the T stored carries of an env already lie side by side in the env-major record: the final carry goes into
                # the slot behind them (slot T of a stochastic record, the spare slot T+1 of a deterministic one — nothing
                # else reads either) and the kernel reads all T+1 in place, one block per env.  h_last reads the slot before.
                s0 = 0 if ro.stochastic else 1
                ro._rnn_em[e0:e0 + Eb, s0 + T].copy_(hstar.view(Eb, n, H))
                h0 = K.H0Blocks(ro._rnn_em[e0, s0], (T + 1) * n, (T + 2) * n * H, Eb)
            else:                                          # stacked actor cells: layer 0 of the packed carry, gathered
                h0_all = self.arena.get("pre.h0all", Eb, T + 1, n, H)
                h0_all[:, :T].copy_(self._vh_carry(ro, e0, Eb))
                h0_all[:, T].copy_(hstar.view(Eb, n, HC)[..., :H])
                h0 = h0_all.view(-1, H)
            # the head writes the block's values where the targets read them
            self.Vh.forward(feats, n_seq=Eb * (T + 1) * n, T=1, h0=h0, tag="pre", train=False,
                            v_out=Vh_buf[e0:e0 + Eb].view(Eb * (T + 1) * n, nh))
            if restore:
                ro._rnn_all[T, e0:e0 + Eb].copy_(ro._rnn_all[T + 1, e0:e0 + Eb])
        return Vl_buf, Vh_buf

    # ------------------------------------------------------------------------------------------------------------------
    # Vh landscape (the producer of the arrays dgppo/env/plot.py:348-372,437-447 draws; the reference ships none)
    # ------------------------------------------------------------------------------------------------------------------
    def require_landscape(self, what: str = "vh_landscape"):
        """ValueError unless vh_landscape / action_landscape serve this engine: DGPPO's constraint-value net on a LiDAR / MPE
        kind"""
        if self.algo != "dgppo":
            why = {"informarl_lagr": "its constraint-value net carries its own scan state, which needs a sequence pass first"}
            raise ValueError(f"{what}: algo '{self.algo}' is not supported: "
                             + why.get(self.algo, "it has no constraint-value network"))
        if self.cfg.is_vmas:
            raise ValueError(f"{what}: VMASReverseTransport is not supported")

    def vh_landscape(self, ro: RolloutData, env_index: int, agent_id: int, frame_ids, xs, ys,
                     events: Optional[list] = None) -> torch.Tensor:
        """-> Vh [F, ny, nx, n, n_cost]: the constraint values of env `env_index` of the env-major record in frame
        frame_ids[f] (a subset of [0, T)) with agent `agent_id` moved to (xs[ix], ys[iy]) and its LiDAR cast again there.
        Every graph of frame t gets the carry values_prepass hands to Vh for (env, t).  Walked in sub-grids of at most
        prepass_graphs graphs: whole frames, else rows of one frame, else pieces of one row.  events: a list that receives one
        (start, features done, Vh done) triple of device events per sub-grid (tools/bench_landscape.py)."""
        self.require_landscape()
        cfg, T = self.cfg, self.T
        n, nh, H = cfg.n_agents, self.n_cost, nets.HID
        ro.finalize()
        if not 0 <= int(env_index) < ro.B:
            raise ValueError(f"vh_landscape: env_index {env_index} outside [0, {ro.B})")
        if not 0 <= int(agent_id) < n:
            raise ValueError(f"vh_landscape: agent_id {agent_id} outside [0, {n})")
        frames = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if frames.size == 0 or frames.min() < 0 or frames.max() >= T:
            raise ValueError(f"vh_landscape: frame_ids must be a non-empty subset of [0, {T})")
        xs, ys = K.sweep_axis(xs, "xs", self.device), K.sweep_axis(ys, "ys", self.device)
        nx, ny, F = int(xs.numel()), int(ys.numel()), int(frames.size)
        e = int(env_index)
        step = {k: v[e] for k, v in ro.step.items()}
        env = {k: v[e] for k, v in ro.env.items()}
        rc, rs = OE._rays(cfg, self.device)
        carry = self._vh_carry(ro, e, 1)[0] if self.hp.use_rnn else None            # [T, n, H]
        out = torch.empty(F, ny, nx, n, nh, device=self.device)
        ids_dev = torch.from_numpy(frames.astype(np.int32)).to(self.device)      # once per call; the sub-grids pass slices
        cap = max(1, self.prepass_graphs)
        fb = max(1, cap // (ny * nx))
        yb = ny if cap >= ny * nx else max(1, cap // nx)
        xb = nx if cap >= nx else cap
        for f0 in range(0, F, fb):
            f1 = min(F, f0 + fb)
            fr = frames[f0:f1]
            for y0 in range(0, ny, yb):
                y1 = min(ny, y0 + yb)
                for x0 in range(0, nx, xb):
                    x1 = min(nx, x0 + xb)
                    P = (y1 - y0) * (x1 - x0)
                    Gb = (f1 - f0) * P
                    feats = nets.GraphFeats(cfg, Gb, self.arena, "land")
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events is not None else None
                    if ev:
                        ev[0].record()
                    feats.compute_sweep(step, env, ids_dev[f0:f1], f1 - f0, agent_id, xs[x0:x1], ys[y0:y1], rc, rs,
                                        frame_max=int(fr.max()))
                    if ev:
                        ev[1].record()
                    h0 = None
                    if carry is not None:
                        h0 = self.arena.get("land.h0", Gb * n, H)
                        for j, t in enumerate(fr):               # the carry of step t, for every grid point of that frame
                            h0.view(f1 - f0, P, n, H)[j].copy_(carry[int(t)].unsqueeze(0).expand(P, n, H))
                    act = self.Vh.forward(feats, n_seq=Gb * n, T=1, h0=h0, tag="land", train=False)
                    out[f0:f1, y0:y1, x0:x1].copy_(act["v"].view(f1 - f0, y1 - y0, x1 - x0, n, nh))
                    if ev:
                        ev[2].record()
                        events.append(tuple(ev))
        return out

    def cost_landscape(self, ro: RolloutData, env_index: int, agent_id: int, frame_ids, xs, ys) -> torch.Tensor:
        """-> cost [F, ny, nx, n, n_cost]: the environment's own cost (get_cost) of every agent of env `env_index` of the
        env-major record in frame frame_ids[f] (a subset of [0, T)) with agent `agent_id` moved to (xs[ix], ys[iy]) and its
        LiDAR cast again there: what the learned Vh of vh_landscape is supposed to bound, at the same swept positions.  It
        needs no network and no carry, so every algo and --no-rnn engines have it; one dgppo_cost_sweep launch writes the
        result in place."""
        cfg, T = self.cfg, self.T
        if cfg.is_vmas:
            raise ValueError("cost_landscape: VMASReverseTransport is not supported")
        n = cfg.n_agents
        ro.finalize()
        if not 0 <= int(env_index) < ro.B:
            raise ValueError(f"cost_landscape: env_index {env_index} outside [0, {ro.B})")
        if not 0 <= int(agent_id) < n:
            raise ValueError(f"cost_landscape: agent_id {agent_id} outside [0, {n})")
        frames = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if frames.size == 0 or frames.min() < 0 or frames.max() >= T:
            raise ValueError(f"cost_landscape: frame_ids must be a non-empty subset of [0, {T})")
        xs, ys = K.sweep_axis(xs, "xs", self.device), K.sweep_axis(ys, "ys", self.device)
        nx, ny, F = int(xs.numel()), int(ys.numel()), int(frames.size)
        e = int(env_index)
        step = {k: v[e] for k, v in ro.step.items()}
        env = {k: v[e] for k, v in ro.env.items()}
        rc, rs = OE._rays(cfg, self.device)
        out = torch.empty(F, ny, nx, n, self.n_cost, device=self.device)
        K.cost_sweep(cfg, step["agent"], n * cfg.state_dim, env.get("obst"), step.get("hits"), n * cfg.top_k * 2, rc, rs,
                     frames, F, int(agent_id), xs, ys, out.view(F * ny * nx, n, self.n_cost))
        return out

    def rollout_landscape(self, ro: RolloutData, env_index: int, agent_id: int, frame_ids, xs, ys, horizon: int,
                          events: Optional[list] = None, records: Optional[list] = None):
        """-> (value, worst), each [F, ny, nx, n, n_cost]: what Vh is trained to predict, measured.  Vh is fitted to the
        discounted-to-max constraint return of the policy's own future (compute_dec_ocp_gae, dgppo/algo/utils.py:38-45), so
        for every grid point the env of frame frame_ids[f] (a subset of [0, T)) of env `env_index` with agent `agent_id`
        moved to (xs[ix], ys[iy]) is forked (dgppo_env_sweep_fork: LiDAR cast again, the actor's pre-step carry of that frame
        — ro._rnn_em[e, t], valid in stochastic and deterministic records alike, all HC columns) and rolled `horizon` steps
        forward with the deterministic policy, whatever kind the source record is (eager launches of _rollout_steps, so the
        one-launch and the four-launch step both serve).  value folds the horizon's costs as the training target does at
        gae_lambda = 1, started from the last cost instead of a learned tail (dgppo_constraint_return, hp.gamma); worst is
        their maximum over the steps: >= 0 exactly where an agent becomes unsafe within the horizon.  The rollouts run past
        the episode's end where t + horizon > T: there is no done flag in these environments.  It needs only the policy, so
        every algo and --no-rnn engines have it.  Walked as vh_landscape walks its grid — whole frames, else rows of one
        frame, else pieces of one row — in sub-grids of Gb envs with Gb * (horizon + 1) <= prepass_graphs.
        events: a list that receives one (start, fork done, steps done, fold done) tuple of device events per sub-grid
        (tools/bench_rollout_landscape.py).  records: a list that receives (f0, f1, y0, y1, x0, x1, finalized record) per
        sub-grid (the tests re-derive every step of those)."""
        cfg, T = self.cfg, self.T
        if cfg.is_vmas:
            raise ValueError("rollout_landscape: VMASReverseTransport is not supported")
        n, nh, HC = cfg.n_agents, self.n_cost, self.HC
        ro.finalize()
        if not 0 <= int(env_index) < ro.B:
            raise ValueError(f"rollout_landscape: env_index {env_index} outside [0, {ro.B})")
        if not 0 <= int(agent_id) < n:
            raise ValueError(f"rollout_landscape: agent_id {agent_id} outside [0, {n})")
        frames = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if frames.size == 0 or frames.min() < 0 or frames.max() >= T:
            raise ValueError(f"rollout_landscape: frame_ids must be a non-empty subset of [0, {T})")
        horizon = int(horizon)
        if horizon < 1:
            raise ValueError(f"rollout_landscape: horizon must be >= 1 (got {horizon})")
        xs, ys = K.sweep_axis(xs, "xs", self.device), K.sweep_axis(ys, "ys", self.device)
        nx, ny, F = int(xs.numel()), int(ys.numel()), int(frames.size)
        e = int(env_index)
        step = {k: v[e] for k, v in ro.step.items()}
        env = {k: v[e] for k, v in ro.env.items()}
        carry = ro._rnn_em[e] if self.hp.use_rnn else None                       # [T + 2, n, HC]: slot t = pre-step carry of t
        value = torch.empty(F, ny, nx, n, nh, device=self.device)
        worst = torch.empty(F, ny, nx, n, nh, device=self.device)
        ids_dev = torch.from_numpy(frames.astype(np.int32)).to(self.device)      # once per call; the sub-grids pass slices
        cap = max(1, self.prepass_graphs // (horizon + 1))
        fb = max(1, cap // (ny * nx))
        yb = ny if cap >= ny * nx else max(1, cap // nx)
        xb = nx if cap >= nx else cap
        recs: Dict[int, RolloutData] = {}            # one record per sub-grid size, unless the caller keeps the records
        for f0 in range(0, F, fb):
            f1 = min(F, f0 + fb)
            fr = frames[f0:f1]
            for y0 in range(0, ny, yb):
                y1 = min(ny, y0 + yb)
                for x0 in range(0, nx, xb):
                    x1 = min(nx, x0 + xb)
                    Gb = (f1 - f0) * (y1 - y0) * (x1 - x0)
                    rec = recs.get(Gb) if records is None else None
                    if rec is None:
                        rec = recs[Gb] = RolloutData(cfg, Gb, horizon, self.device, False, HC)
                    rec._env_major = False
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if events is not None else None
                    if ev:
                        ev[0].record()
                    if carry is None:
                        rec.rnn_tm[0].zero_()
                    OE.sweep_fork(cfg, step, env, ids_dev[f0:f1], f1 - f0, int(agent_id), xs[x0:x1], ys[y0:y1], rec.states_tm[0],
                                  carry, n * HC, rec.rnn_tm[0].view(Gb * n, HC) if carry is not None else None,
                                  frame_max=int(fr.max()))
                    if ev:
                        ev[1].record()
                    self._rollout_steps(rec, None, Gb, False)
                    if ev:
                        ev[2].record()
                    val = self.arena.get("rl.value", Gb, n, nh)
                    wor = self.arena.get("rl.worst", Gb, n, nh)
                    OA.constraint_return(rec.cost_tm, self.hp.gamma, val, wor)
                    value[f0:f1, y0:y1, x0:x1].copy_(val.view(f1 - f0, y1 - y0, x1 - x0, n, nh))
                    worst[f0:f1, y0:y1, x0:x1].copy_(wor.view(f1 - f0, y1 - y0, x1 - x0, n, nh))
                    if ev:
                        ev[3].record()
                        events.append(tuple(ev))
                    if records is not None:
                        records.append((f0, f1, y0, y1, x0, x1, rec.finalize()))
        return value, worst

    def action_landscape(self, ro: RolloutData, env_index: int, agent_id: int, frame_ids, us, vs,
                         events: Optional[list] = None):
        """-> (cbf, Vh_next, Vh): the discrete barrier condition DGPPO's advantage is shaped by (dgppo.py:246-250) with the
        action of agent `agent_id` at step t = frame_ids[f] (a subset of [0, T)) of env `env_index` swept over (us[iu], vs[iv]).
        Vh_next [F, nv, nu, n, n_cost] is Vh of the graph of frame t + 1 in which that agent's row is agent_step_euler(its row
        of frame t, clip_action((us[iu], vs[iv]))) and every other agent keeps its recorded next state, with the carry
        values_prepass hands to Vh for (env, t + 1) (the final carry for t = T - 1; the carry does not depend on the swept
        action); Vh [F, n, n_cost] is values_prepass' Vh[env, t]; cbf = (Vh_next - Vh) / dt + alpha * Vh, <= 0 where the net
        admits the action.  Walked in sub-grids of at most prepass_graphs graphs, as vh_landscape is.  events: as there.
        Vh comes from a values_prepass of the whole record (that is what makes it bit-equal to it), which rewrites the
        pre-pass' persistent output buffers with the values they already hold for these parameters."""
        self.require_landscape("action_landscape")
        cfg, T = self.cfg, self.T
        n, nh, H = cfg.n_agents, self.n_cost, nets.HID
        ro.finalize()
        if not 0 <= int(env_index) < ro.B:
            raise ValueError(f"action_landscape: env_index {env_index} outside [0, {ro.B})")
        if not 0 <= int(agent_id) < n:
            raise ValueError(f"action_landscape: agent_id {agent_id} outside [0, {n})")
        frames = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if frames.size == 0 or frames.min() < 0 or frames.max() >= T:
            raise ValueError(f"action_landscape: frame_ids must be a non-empty subset of [0, {T})")
        us, vs = K.sweep_axis(us, "us", self.device), K.sweep_axis(vs, "vs", self.device)
        nu, nv, F = int(us.numel()), int(vs.numel()), int(frames.size)
        e = int(env_index)
        ids_dev = torch.from_numpy(frames.astype(np.int32)).to(self.device)      # once per call; the sub-grids pass slices
        _, Vh_all = self.values_prepass(ro, want_Vl=False)
        Vh = Vh_all[e].index_select(0, ids_dev.long())                           # [F, n, nh]
        carry = None
        if self.hp.use_rnn:                                                      # [T, n, H]: the carry of the graph of frame t + 1
            carry = torch.empty(T, n, H, device=self.device)
            carry[:T - 1].copy_(self._vh_carry(ro, e, 1)[0, 1:])
            if int(frames.max()) == T - 1:
                carry[T - 1].copy_(self._final_carry(ro, e, 1).view(n, self.HC)[:, :H])
        step = {k: v[e] for k, v in ro.step.items()}
        env = {k: v[e] for k, v in ro.env.items()}
        Vh_next = torch.empty(F, nv, nu, n, nh, device=self.device)
        cap = max(1, self.prepass_graphs)
        fb = max(1, cap // (nv * nu))
        vb = nv if cap >= nv * nu else max(1, cap // nu)
        ub = nu if cap >= nu else cap
        for f0 in range(0, F, fb):
            f1 = min(F, f0 + fb)
            fr = frames[f0:f1]
            for v0 in range(0, nv, vb):
                v1 = min(nv, v0 + vb)
                for u0 in range(0, nu, ub):
                    u1 = min(nu, u0 + ub)
                    P = (v1 - v0) * (u1 - u0)
                    Gb = (f1 - f0) * P
                    feats = nets.GraphFeats(cfg, Gb, self.arena, "act")
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events is not None else None
                    if ev:
                        ev[0].record()
                    feats.compute_action_sweep(step, env, ids_dev[f0:f1], f1 - f0, agent_id, us[u0:u1], vs[v0:v1],
                                               frame_max=int(fr.max()))
                    if ev:
                        ev[1].record()
                    h0 = None
                    if carry is not None:
                        h0 = self.arena.get("act.h0", Gb * n, H)
                        for j, t in enumerate(fr):               # the carry of step t + 1, for every grid point of that frame
                            h0.view(f1 - f0, P, n, H)[j].copy_(carry[int(t)].unsqueeze(0).expand(P, n, H))
                    act = self.Vh.forward(feats, n_seq=Gb * n, T=1, h0=h0, tag="act", train=False)
                    Vh_next[f0:f1, v0:v1, u0:u1].copy_(act["v"].view(f1 - f0, v1 - v0, u1 - u0, n, nh))
                    if ev:
                        ev[2].record()
                        events.append(tuple(ev))
        Vh_b = Vh.view(F, 1, 1, n, nh)
        cbf = (Vh_next - Vh_b) / float(cfg.dt) + float(self.hp.alpha) * Vh_b
        return cbf, Vh_next, Vh.clone()

    def action_rollout_landscape(self, ro: RolloutData, env_index: int, agent_id: int, frame_ids, us, vs, horizon: int,
                                 events: Optional[list] = None, records: Optional[list] = None):
        """-> (value, worst), each [F, nv, nu, n, n_cost]: what the actions action_landscape judges by the learned barrier lead
        to, measured.  For every frame t = frame_ids[f] (a subset of [0, T)) of env `env_index` and every grid action (us[iu],
        vs[iv]) the env of frame t is forked (dgppo_env_action_sweep_fork) with agent `agent_id` playing the grid action in the
        coming step and everyone else their RECORDED action of step t (action_landscape's convention; the step clips, the fork
        does not), the plain env step applies that joint action, and the deterministic policy is rolled on (_rollout_steps from
        slot 1) until the costs of the `horizon` states after the forced step are known.  It starts from the carry the policy
        left after its forward on frame t — ro._rnn_em[e, t + 1], which does not depend on the action taken and is valid in
        stochastic and deterministic records alike.  value / worst fold those costs as rollout_landscape does
        (dgppo_constraint_return, hp.gamma) and hold EVERY agent's row: the swept agent's own row is what the lookahead shield
        calls s, the others say what its single action does to its neighbours.  The rollouts run past the episode's end (no
        done flag) and follow the unshielded policy whatever produced the record.  It needs the simulator and the policy only:
        every algo, --no-rnn engines and stacked cells have it.  Walked as action_landscape walks its grid — whole frames, else
        rows of one frame, else pieces of one row — in sub-grids of Gb envs with Gb * (horizon + 2) <= prepass_graphs, never
        fewer than one env; the last step of a block record exists only to evaluate the cost of the last state.
        events: a list that receives one (start, fork and forced step done, policy steps done, fold done) tuple of device
        events per sub-grid (tools/bench_action_rollout.py).  records: a list that receives (f0, f1, v0, v1, u0, u1, block
        record) per sub-grid, time-major as rolled (the tests re-derive every step of those)."""
        cfg, T = self.cfg, self.T
        if cfg.is_vmas:
            raise ValueError("action_rollout_landscape: VMASReverseTransport is not supported")
        n, nh, HC = cfg.n_agents, self.n_cost, self.HC
        ro.finalize()
        if not 0 <= int(env_index) < ro.B:
            raise ValueError(f"action_rollout_landscape: env_index {env_index} outside [0, {ro.B})")
        if not 0 <= int(agent_id) < n:
            raise ValueError(f"action_rollout_landscape: agent_id {agent_id} outside [0, {n})")
        frames = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if frames.size == 0 or frames.min() < 0 or frames.max() >= T:
            raise ValueError(f"action_rollout_landscape: frame_ids must be a non-empty subset of [0, {T})")
        horizon = int(horizon)
        if horizon < 1:
            raise ValueError(f"action_rollout_landscape: horizon must be >= 1 (got {horizon})")
        us, vs = K.sweep_axis(us, "us", self.device), K.sweep_axis(vs, "vs", self.device)
        nu, nv, F = int(us.numel()), int(vs.numel()), int(frames.size)
        e = int(env_index)
        step = {k: v[e] for k, v in ro.step.items()}
        env = {k: v[e] for k, v in ro.env.items()}
        actions = ro.actions[e]                                                  # [T, n, 2]
        carry = ro._rnn_em[e, 1:] if self.hp.use_rnn else None                   # [T + 1, n, HC]: slot t = the carry after frame t
        if carry is not None and int(frames.max()) == T - 1:
            # values_prepass parks the final carry of a stochastic record in slot T (nothing else reads it there): the carry
            # after frame T - 1 is put back from the time-major record, and values_prepass writes its own again before it reads
            ro._rnn_em[e, T].copy_(ro.rnn_tm[T, e])
        value = torch.empty(F, nv, nu, n, nh, device=self.device)
        worst = torch.empty(F, nv, nu, n, nh, device=self.device)
        ids_dev = torch.from_numpy(frames.astype(np.int32)).to(self.device)      # once per call; the sub-grids pass slices
        cap = max(1, self.prepass_graphs // (horizon + 2))
        fb = max(1, cap // (nv * nu))
        vb = nv if cap >= nv * nu else max(1, cap // nu)
        ub = nu if cap >= nu else cap
        recs: Dict[int, RolloutData] = {}            # one record per sub-grid size, unless the caller keeps the records
        for f0 in range(0, F, fb):
            f1 = min(F, f0 + fb)
            fr = frames[f0:f1]
            for v0 in range(0, nv, vb):
                v1 = min(nv, v0 + vb)
                for u0 in range(0, nu, ub):
                    u1 = min(nu, u0 + ub)
                    Gb = (f1 - f0) * (v1 - v0) * (u1 - u0)
                    rec = recs.get(Gb) if records is None else None
                    if rec is None:
                        rec = recs[Gb] = RolloutData(cfg, Gb, horizon + 1, self.device, False, HC)
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if events is not None else None
                    if ev:
                        ev[0].record()
                    if carry is None:
                        rec.rnn_tm[1].zero_()
                    OE.action_sweep_fork(cfg, step, env, actions, ids_dev[f0:f1], f1 - f0, int(agent_id), us[u0:u1], vs[v0:v1],
                                         rec.states_tm[0], rec.action_tm[0], carry, n * HC,
                                         rec.rnn_tm[1].view(Gb * n, HC) if carry is not None else None, frame_max=int(fr.max()))
                    OE.step(cfg, rec.states_tm[0], rec.action_tm[0], rec.states_tm[1], rec.reward_tm[0], rec.cost_tm[0])
                    if ev:
                        ev[1].record()
                    self._rollout_steps(rec, None, Gb, False, start=1)
                    if ev:
                        ev[2].record()
                    val = self.arena.get("arl.value", Gb, n, nh)
                    wor = self.arena.get("arl.worst", Gb, n, nh)
                    OA.constraint_return(rec.cost_tm[1:horizon + 1], self.hp.gamma, val, wor)
                    value[f0:f1, v0:v1, u0:u1].copy_(val.view(f1 - f0, v1 - v0, u1 - u0, n, nh))
                    worst[f0:f1, v0:v1, u0:u1].copy_(wor.view(f1 - f0, v1 - v0, u1 - u0, n, nh))
                    if ev:
                        ev[3].record()
                        events.append(tuple(ev))
                    if records is not None:
                        records.append((f0, f1, v0, v1, u0, u1, rec))
        return value, worst

    # ------------------------------------------------------------------------------------------------------------------
    # barrier shield: the deterministic rollout with every agent's action filtered through the learned barrier
    # ------------------------------------------------------------------------------------------------------------------
    def rollout_shielded(self, seeds: torch.Tensor, us, vs, margin: float = 0.0, events: Optional[list] = None, start=None):
        """-> (RolloutData, log): a deterministic record (the conventions of rollout(seeds, False)) in which, at every step,
        every agent's action is filtered through the barrier condition the policy is trained under (dgppo.py:246-250).  The
        candidates of an agent are its own policy action (index 0) and the grid (us[iu], vs[iv]) (index 1 + iv * nu + iu).  Per
        step: the policy forward gives a_pol and the post-step carry; Vh of the graph of state t with layer 0 of that carry is
        Vh_t; a provisional step with a_pol gives the next state (its positions and hits are final: they do not depend on the
        action) and one more policy forward on it the carry c' that Vh reads for frame t + 1; the what-if graphs of every
        (env, agent, candidate) — the agent's row stepped by the candidate, everyone else as provisionally stepped — go through
        Vh with layer 0 of c' (dgppo_graph_feats_team_action_sweep, walked in blocks of environments of at most prepass_graphs
        graphs); dgppo_shield_select picks per agent, on its own row; the final step with the chosen actions overwrites state
        t + 1.  Reward and cost belong to the pre-step state and keep their values.
        log (time-major device tensors): policy_action [T, B, n, 2], index / flag [T, B, n] (int32; flag 0 kept, 1 replaced by an
        admissible candidate, 2 nothing admissible), h [T, B, n, P], Vh [T, B, n, nh].  Eager launches; the record is a fresh one.
        events: a list that receives one tuple of device events per step (tools/bench_shield.py): start, policy and Vh_t done,
        provisional step and c' done, then (features, Vh forward, select) done per env block, the final step done."""
        self.require_landscape("rollout_shielded")
        cfg, T = self.cfg, self.T
        n, nh, H, HC = cfg.n_agents, self.n_cost, nets.HID, self.HC
        us, vs = K.sweep_axis(us, "us", self.device), K.sweep_axis(vs, "vs", self.device)
        margin = float(margin)
        if not np.isfinite(margin):
            raise ValueError("rollout_shielded: margin must be finite")
        nu, nv = int(us.numel()), int(vs.numel())
        P = 1 + nu * nv
        B = int(seeds.shape[0])
        dev = self.device
        ro = RolloutData(cfg, B, T, dev, False, HC)
        self._start(seeds, ro.states_tm[0], start)
        ro.rnn_tm[0].zero_()
        log = dict(policy_action=torch.empty(T, B, n, 2, device=dev), index=torch.empty(T, B, n, dtype=torch.int32, device=dev),
                   flag=torch.empty(T, B, n, dtype=torch.int32, device=dev), h=torch.empty(T, B, n, P, device=dev),
                   Vh=torch.empty(T, B, n, nh, device=dev))
        use_rnn = self.hp.use_rnn
        block = max(1, min(B, max(1, self.prepass_graphs) // (n * P)))
        dt, alpha = float(cfg.dt), float(self.hp.alpha)

        def mark(ev):
            if ev is not None:
                ev.append(torch.cuda.Event(enable_timing=True))
                ev[-1].record()
        for t in range(T):
            st, nst = ro.states_tm[t], ro.states_tm[t + 1]
            ev = [] if events is not None else None
            mark(ev)
            # 1. policy forward: a_pol and h_{t+1}
            feats = self._feats("sh", st, B)
            h_next = ro.rnn_tm[t + 1].view(B * n, HC)
            act = self.policy.forward(feats, n_seq=B * n, T=1, h0=ro.rnn_tm[t].view(B * n, HC), tag="sh", hs_out=h_next,
                                      train=False)
            a_pol = log["policy_action"][t]
            K.policy_head(act["ms"], None, None, a_pol.view(B * n, 2), None, None, n, 1)
            # 2. Vh_t with the carry a deterministic record hands it: layer 0 of h_{t+1}
            h0 = None
            if use_rnn:
                h0 = h_next
                if HC != H:
                    h0 = self.arena.get("sh.h0", B * n, H)
                    h0.copy_(h_next[:, :H])
            v = self.Vh.forward(feats, n_seq=B * n, T=1, h0=h0, tag="sh", train=False)["v"]
            Vh_t = log["Vh"][t]
            Vh_t.copy_(v.view(B, n, nh))
            mark(ev)
            # 3. provisional step and the carry c' of frame t + 1
            OE.step(cfg, st, a_pol, nst, ro.reward_tm[t], ro.cost_tm[t])
            cl0 = None
            if use_rnn:
                cprime = self.arena.get("sh.cprime", B * n, HC)
                self.policy.forward(self._feats("sh", nst, B), n_seq=B * n, T=1, h0=h_next, tag="sh", hs_out=cprime, train=False)
                cl0 = cprime.view(B, n, HC)[..., :H]
            mark(ev)
            # 4. - 6. what-if graphs, Vh, selection: blocks of environments
            for e0 in range(0, B, block):
                Eb = min(block, B - e0)
                sl = slice(e0, e0 + Eb)
                Gb = Eb * n * P
                cut = lambda s: OE.State({k: x[sl] for k, x in s.step.items()}, {k: x[sl] for k, x in s.env.items()})
                wf = nets.GraphFeats(cfg, Gb, self.arena, "shw").compute_team_action_sweep(cut(st), cut(nst), a_pol[sl], us, vs)
                mark(ev)
                hw = None
                if use_rnn:
                    hw = self.arena.get("shw.h0", Gb * n, H)
                    hw.view(Eb, n * P, n, H).copy_(cl0[sl].unsqueeze(1).expand(Eb, n * P, n, H))
                vn = self.Vh.forward(wf, n_seq=Gb * n, T=1, h0=hw, tag="shw", train=False)["v"]
                mark(ev)
                K.shield_select(vn.view(Gb * n, nh), Vh_t[sl], a_pol[sl], us, vs, dt, alpha, margin, ro.action_tm[t][sl],
                                log["index"][t][sl], log["flag"][t][sl], log["h"][t][sl])
                mark(ev)
            # 7. the step that counts
            OE.step(cfg, st, ro.action_tm[t], nst, ro.reward_tm[t], ro.cost_tm[t])
            mark(ev)
            if ev is not None:
                events.append(tuple(ev))
        return ro, log

    # ------------------------------------------------------------------------------------------------------------------
    # lookahead shield: every agent's action filtered by forked policy rollouts — the simulator and the policy, no Vh
    # ------------------------------------------------------------------------------------------------------------------
    def lookahead_select(self, st: OE.State, carry_next, a_pol, us, vs, horizon: int, margin: float, action, index, flag, s,
                         records: Optional[list] = None, t: int = 0, mark: Optional[Callable[[], None]] = None):
        """The core of one lookahead-shield step on a dense state `st` of B envs: for every (env e, agent i, candidate p) —
        candidate 0 is a_pol[e, i], candidate 1 + iv * nu + iu is (us[iu], vs[iv]), the numbering of dgppo_shield_select — env e
        is forked (dgppo_env_team_action_fork) with agent i playing the candidate and everyone else a_pol[e], the plain env step
        applies that joint action, and the deterministic policy is rolled on from there (_rollout_steps from slot 1, with the
        carry carry_next [B * n, HC] the policy left after its forward on `st`; None without an RNN) until the costs of the
        `horizon` states after the forced step are known.  s [B, n, P] is the worst of those costs on the agent's own row;
        dgppo_lookahead_select admits a candidate iff s <= -margin and picks per agent by dgppo_shield_select's rules ->
        action [B, n, 2] (clipped), index / flag [B, n] int32.  us / vs: ops_nn.sweep_axis tensors.
        Walked in blocks of whole environments: Eb envs, G = Eb * n * P what-if envs in a record of horizon + 1 steps, with
        G * (horizon + 2) <= prepass_graphs and never fewer than one env.  The last step of the block record exists only to
        evaluate the cost of the last state.
        Two limits, as in rollout_shielded: agent i's candidates are judged with everyone else playing the policy, so when
        several agents are replaced in the same step the joint outcome is not one that was rolled (lookahead_select_rounds rolls
        it, and says where it could not); and the what-if rollouts run past the episode's end (there is no done flag in these
        environments).
        records: a list that receives (t, e0, Eb, block record) per block (time-major, as rolled; the tests re-derive every
        step of those); without it the block records are reused from call to call.  mark: called after the fork and forced
        step, after the policy steps and after the selection of every block (rollout_lookahead_shielded's events)."""
        cfg = self.cfg
        if cfg.is_vmas:
            raise ValueError("lookahead_select: VMASReverseTransport is not supported")
        n, HC = cfg.n_agents, self.HC
        H = int(horizon)
        if H < 1:
            raise ValueError(f"lookahead_select: horizon must be >= 1 (got {horizon})")
        margin = float(margin)
        if not np.isfinite(margin):
            raise ValueError("lookahead_select: margin must be finite")
        if self.hp.use_rnn and carry_next is None:
            raise ValueError("lookahead_select: this engine's policy has a recurrent cell: carry_next is required")
        if not self.hp.use_rnn:
            carry_next = None
        B = int(a_pol.shape[0])
        P = 1 + int(us.numel()) * int(vs.numel())
        block = max(1, min(B, max(1, self.prepass_graphs) // (n * P * (H + 2))))
        cache = self._la_records = getattr(self, "_la_records", {})
        for e0 in range(0, B, block):
            Eb = min(block, B - e0)
            sl = slice(e0, e0 + Eb)
            G = Eb * n * P
            rec = cache.get((G, H)) if records is None else None
            if rec is None:
                rec = RolloutData(cfg, G, H + 1, self.device, False, HC)
                if records is None:
                    if len(cache) >= 2:                 # a call walks two block sizes at most: the full block and the last one
                        cache.clear()
                    cache[(G, H)] = rec
            cut = OE.State({k: x[sl] for k, x in st.step.items()}, {k: x[sl] for k, x in st.env.items()})
            if carry_next is None:
                rec.rnn_tm[1].zero_()
            OE.team_action_fork(cfg, cut, a_pol[sl], us, vs, rec.states_tm[0], rec.action_tm[0],
                                carry_next[e0 * n:(e0 + Eb) * n] if carry_next is not None else None,
                                rec.rnn_tm[1].view(G * n, HC) if carry_next is not None else None)
            OE.step(cfg, rec.states_tm[0], rec.action_tm[0], rec.states_tm[1], rec.reward_tm[0], rec.cost_tm[0])
            if mark:
                mark()
            self._rollout_steps(rec, None, G, False, start=1)
            if mark:
                mark()
            K.lookahead_select(rec.cost_tm[1:H + 1], a_pol[sl], us, vs, margin, action[sl], index[sl], flag[sl], s[sl])
            if mark:
                mark()
            if records is not None:
                records.append((int(t), e0, Eb, rec))

    def lookahead_select_rounds(self, st: OE.State, carry_next, a_pol, us, vs, horizon: int, margin: float, rounds: int, action,
                                index, flag, s, joint, rounds_used, records: Optional[list] = None, t: int = 0,
                                mark: Optional[Callable[[], None]] = None):
        """lookahead_select in rounds that roll the joint action the agents settle on.  The joint action held, A = `action`
        [B, n, 2], starts as a_pol with index = 0 and every env active.  Round r < rounds, on the active envs: every (env, agent,
        candidate) is forked from A (dgppo_env_team_action_fork_ids: candidate 0 is what the agent holds, everyone else plays
        A), stepped and rolled exactly as in lookahead_select, and dgppo_lookahead_reselect picks per agent — nearest to the
        POLICY's action among the admissible — and commits: every agent in round 0 (which is lookahead_select's verdict), in
        later rounds only the lowest-numbered agent that wants to move.  One mover per round, because agents that re-judge
        simultaneously can dodge and return in lockstep for ever; one mover leaves a joint action whose every other row was
        the one rolled.  An env stays active while some agent moved; the rounds end when no env is active.
        -> action, index (the grid number of what is held, 0: the policy's action), flag (of the action held: 0 policy's and
        admissible, 1 replaced and admissible, 2 not admissible), s [B, n, P] (the fold of the env's LAST round), joint [B]
        int32 (2: the joint action held was rolled as candidate 0 and is admissible for every agent; 1: rolled, not admissible
        for some agent, nobody found better; 0: some agent moved in the env's last round — the joint action held was NOT
        rolled, the limit of lookahead_select is back for that env) and rounds_used [B] int32 (the rounds that judged the env).
        rounds = 1 gives lookahead_select's action, index, flag and s.  One host sync per round but the last (the active list,
        torch.nonzero).  The active list is walked in blocks of at most as many envs as lookahead_select's, in prefixes of ONE
        block record of that capacity.  records: receives (t, r, env ids of the block, block record); the records are then
        fresh ones.  mark: as in lookahead_select, per block of every round."""
        cfg = self.cfg
        fn = "lookahead_select_rounds"
        if cfg.is_vmas:
            raise ValueError(f"{fn}: VMASReverseTransport is not supported")
        n, HC = cfg.n_agents, self.HC
        H, R = int(horizon), int(rounds)
        if H < 1:
            raise ValueError(f"{fn}: horizon must be >= 1 (got {horizon})")
        if R < 1:
            raise ValueError(f"{fn}: rounds must be >= 1 (got {rounds})")
        margin = float(margin)
        if not np.isfinite(margin):
            raise ValueError(f"{fn}: margin must be finite")
        if self.hp.use_rnn and carry_next is None:
            raise ValueError(f"{fn}: this engine's policy has a recurrent cell: carry_next is required")
        if not self.hp.use_rnn:
            carry_next = None
        B = int(a_pol.shape[0])
        P = 1 + int(us.numel()) * int(vs.numel())
        block = max(1, min(B, max(1, self.prepass_graphs) // (n * P * (H + 2))))
        full = None
        if records is None:
            key = (block * n * P, H)
            if getattr(self, "_lar_record", (None, None))[0] != key:          # ONE record, whatever the active counts turn out to be
                self._lar_record = (key, RolloutData(cfg, key[0], H + 1, self.device, False, HC))
            full = self._lar_record[1]
        action.copy_(a_pol)
        index.zero_()
        changed = torch.zeros(B, dtype=torch.int32, device=self.device)
        used = np.zeros(B, np.int32)
        ids = np.arange(B, dtype=np.int32)
        for r in range(R):
            ids_dev = torch.from_numpy(ids).to(self.device)
            used[ids] += 1
            if r > 0:
                changed.zero_()
            for m0 in range(0, ids.size, block):
                blk = ids[m0:m0 + block]
                Mb = int(blk.size)
                G = Mb * n * P
                rec = full.prefix(G) if full is not None else RolloutData(cfg, G, H + 1, self.device, False, HC)
                if carry_next is None:
                    rec.rnn_tm[1].zero_()
                OE.team_action_fork_ids(cfg, st, action, blk, us, vs, rec.states_tm[0], rec.action_tm[0], carry_next,
                                        rec.rnn_tm[1].view(G * n, HC) if carry_next is not None else None,
                                        ids_dev=ids_dev[m0:m0 + Mb])
                OE.step(cfg, rec.states_tm[0], rec.action_tm[0], rec.states_tm[1], rec.reward_tm[0], rec.cost_tm[0])
                if mark:
                    mark()
                self._rollout_steps(rec, None, G, False, start=1)
                if mark:
                    mark()
                K.lookahead_reselect(rec.cost_tm[1:H + 1], blk, a_pol, us, vs, margin, 0 if r == 0 else 1, action, index, flag,
                                     joint, changed, s, ids_dev=ids_dev[m0:m0 + Mb])
                if mark:
                    mark()
                if records is not None:
                    records.append((int(t), r, blk.copy(), rec))
            if r + 1 == R:
                break
            ids = torch.nonzero(changed).flatten().to(torch.int32).cpu().numpy()   # ascending; the round's one host sync
            if ids.size == 0:
                break
        rounds_used.copy_(torch.from_numpy(used), non_blocking=False)

    def rollout_lookahead_shielded(self, seeds: torch.Tensor, us, vs, horizon: int, margin: float = 0.0,
                                   events: Optional[list] = None, records: Optional[list] = None, rounds: int = 1,
                                   start=None):
        """-> (RolloutData, log): a deterministic record (the conventions of rollout(seeds, False)) in which, at every step,
        every agent's action is filtered by what it leads to within `horizon` steps of the simulator, the learned Vh left out:
        what rollout_shielded trusts Vh to predict is rolled here.  Per step t: the policy forward on state t gives a_pol and
        the post-step carry h_{t+1} (written to rnn_tm[t + 1]; it does not depend on the action taken); lookahead_select forks
        state t per (env, agent, candidate), applies the forced joint action, rolls the deterministic policy and picks per
        agent on the worst own-row cost of the `horizon` states that follow (admissible iff <= -margin); the step with the
        chosen actions writes state t + 1.  Reward and cost belong to the pre-step state.  It needs the simulator and the policy
        only: every algo and --no-rnn engines have it.  The limits stated at lookahead_select hold: the others are assumed to
        play the policy, and the what-if rollouts run past the episode's end.
        log (time-major device tensors): policy_action [T, B, n, 2], index / flag [T, B, n] (int32; flag 0 kept, 1 replaced by
        an admissible candidate, 2 nothing admissible), s [T, B, n, P].  Eager launches; the record is a fresh one.
        events: a list that receives one tuple of device events per step (tools/bench_lookahead_shield.py): start, policy
        forward done, then (fork and forced step, policy steps, select) done per env block, the final step done.
        records: as in lookahead_select.
        rounds: 1 is the path above, untouched.  rounds >= 2 selects with lookahead_select_rounds — up to `rounds` rounds per
        step, one mover per env in every round after the first — and the log gains joint [T, B] and rounds_used [T, B] (int32;
        joint 2: the joint action played was rolled and is admissible for every agent, 1: rolled and not admissible, 0: not
        rolled); the events then hold one (fork and forced step, policy steps, select) triple per block of every round, and
        records receives lookahead_select_rounds' tuples."""
        cfg, T = self.cfg, self.T
        if cfg.is_vmas:
            raise ValueError("rollout_lookahead_shielded: VMASReverseTransport is not supported")
        n, HC = cfg.n_agents, self.HC
        H = int(horizon)
        if H < 1:
            raise ValueError(f"rollout_lookahead_shielded: horizon must be >= 1 (got {horizon})")
        margin = float(margin)
        if not np.isfinite(margin):
            raise ValueError("rollout_lookahead_shielded: margin must be finite")
        R = int(rounds)
        if R < 1:
            raise ValueError(f"rollout_lookahead_shielded: rounds must be >= 1 (got {rounds})")
        us, vs = K.sweep_axis(us, "us", self.device), K.sweep_axis(vs, "vs", self.device)
        P = 1 + int(us.numel()) * int(vs.numel())
        B = int(seeds.shape[0])
        dev = self.device
        ro = RolloutData(cfg, B, T, dev, False, HC)
        self._start(seeds, ro.states_tm[0], start)
        ro.rnn_tm[0].zero_()
        log = dict(policy_action=torch.empty(T, B, n, 2, device=dev), index=torch.empty(T, B, n, dtype=torch.int32, device=dev),
                   flag=torch.empty(T, B, n, dtype=torch.int32, device=dev), s=torch.empty(T, B, n, P, device=dev))
        if R > 1:
            log.update(joint=torch.empty(T, B, dtype=torch.int32, device=dev),
                       rounds_used=torch.empty(T, B, dtype=torch.int32, device=dev))
        for t in range(T):
            st = ro.states_tm[t]
            ev = [] if events is not None else None

            def mark():
                if ev is not None:
                    ev.append(torch.cuda.Event(enable_timing=True))
                    ev[-1].record()
            mark()
            # 1. policy forward: a_pol and h_{t+1}
            feats = self._feats("la", st, B)
            h_next = ro.rnn_tm[t + 1].view(B * n, HC)
            act = self.policy.forward(feats, n_seq=B * n, T=1, h0=ro.rnn_tm[t].view(B * n, HC), tag="la", hs_out=h_next,
                                      train=False)
            a_pol = log["policy_action"][t]
            K.policy_head(act["ms"], None, None, a_pol.view(B * n, 2), None, None, n, 1)
            mark()
            # 2. - 5. fork, forced step, policy steps, selection: blocks of environments
            if R == 1:
                self.lookahead_select(st, h_next if self.hp.use_rnn else None, a_pol, us, vs, H, margin, ro.action_tm[t],
                                      log["index"][t], log["flag"][t], log["s"][t], records=records, t=t, mark=mark)
            else:
                self.lookahead_select_rounds(st, h_next if self.hp.use_rnn else None, a_pol, us, vs, H, margin, R,
                                             ro.action_tm[t], log["index"][t], log["flag"][t], log["s"][t], log["joint"][t],
                                             log["rounds_used"][t], records=records, t=t, mark=mark)
            # 6. the step that counts
            OE.step(cfg, st, ro.action_tm[t], ro.states_tm[t + 1], ro.reward_tm[t], ro.cost_tm[t])
            mark()
            if ev is not None:
                events.append(tuple(ev))
        return ro, log

    # ------------------------------------------------------------------------------------------------------------------
    # update
    # ------------------------------------------------------------------------------------------------------------------
    def cbf_weight_at(self, step: int) -> float:
        hp = self.hp
        w = hp.cbf_weight
        if hp.cbf_schedule:  # optax.piecewise_constant_schedule (dgppo.py:73-80)
            if step >= int(hp.train_steps * 0.5):
                w *= 2
            if step >= int(hp.train_steps * 0.75):
                w *= 2
        return w

    def cost_weight_at(self, step: int) -> float:
        hp = self.hp
        w = hp.cost_weight
        if hp.cost_schedule:  # optax.piecewise_constant_schedule(init, {0.5*steps: 5, 0.75*steps: 5}) (informarl.py:189-196)
            if step >= int(hp.train_steps * 0.5):
                w *= 5
            if step >= int(hp.train_steps * 0.75):
                w *= 5
        return w

    def targets_hcbfcrpo(self, ro: RolloutData, step: int):
        """HCBFCRPO (hcbfcrpo.py:120-186): DGPPO's targets with the hand-crafted CBF Vh := env.get_cost(graph).  For
        t < T that is the stored cost (cost is evaluated on the pre-step graph); the final entry is the cost of
        next_graph[-1], obtained from one more env.step call whose other outputs are discarded."""
        cfg, T, B, hp = self.cfg, self.T, ro.B, self.hp
        n, nh, dev = cfg.n_agents, self.n_cost, self.device
        Vl, _ = self.values_prepass(ro, want_Vl=True, want_Vh=False)
        fin = OE.State({k: v[:, T].contiguous() for k, v in ro.step.items()}, ro.env)
        A = self.arena
        fin_cost = A.get("tg.fin_cost", B, n, nh)
        OE.step(cfg, fin, torch.zeros(B, n, 2, device=dev), fin.like(), torch.empty(B, device=dev), fin_cost)
        Vh = A.get("tg.Vh.crafted", B, T + 1, n, nh)
        Vh[:, :T].copy_(ro.costs)
        Vh[:, T].copy_(fin_cost)
        Qh = A.get("tg.Qh", B, T, n, nh)
        Ql = A.get("tg.Ql", B, T)
        OA.gae(ro.costs, ro.rewards, Vh, Vl, self.lam_pow, hp.gamma, hp.gae_lambda, Qh, Ql)
        adv = A.get("tg.adv", B, T, n)
        self.stats.zero_()
        OA.advantage(Ql, Vl, Vh, cfg.dt, hp.alpha, hp.cbf_eps, self.cbf_weight_at(step), adv, self.stats[3])
        return dict(Vl=Vl, Vh=Vh, Ql=Ql, Qh=Qh, adv=adv)

    def targets_informarl(self, ro: RolloutData, step: int):
        """InforMARL (informarl.py:309-336): Vl pass, Dec-OCP GAE with Vh := Vl and the cost-shaped stage cost, advantage
        = -(Ql - Vl) normalised per env."""
        cfg, T, B, hp = self.cfg, self.T, ro.B, self.hp
        n, nh, dev = cfg.n_agents, self.n_cost, self.device
        Vl, _ = self.values_prepass(ro, want_Vl=True, want_Vh=False)
        A = self.arena
        Vh = A.get("tg.Vh.bcast", B, T + 1, n, nh)
        Vh.copy_(Vl.view(B, T + 1, 1, 1).expand(B, T + 1, n, nh))
        shaped = A.get("tg.shaped", B, T)
        OA.shaped_reward(ro.rewards, ro.costs, self.cost_weight_at(step), shaped)
        Qh = A.get("tg.Qh", B, T, n, nh)
        Ql = A.get("tg.Ql", B, T)
        OA.gae(ro.costs, shaped, Vh, Vl, self.lam_pow, hp.gamma, hp.gae_lambda, Qh, Ql)
        adv = A.get("tg.adv", B, T, n)
        self.stats.zero_()
        OA.advantage(Ql, Vl, None, cfg.dt, 0.0, 0.0, 0.0, adv, self.stats[3])
        return dict(Vl=Vl, Ql=Ql, Qh=Qh, adv=adv)

    def targets_lagr(self, ro: RolloutData, step: int):
        """InforMARL-Lagrangian (informarl_lagr.py:177-235): Vl and Vh scans (each with its own zero-initialised carry, final
        value on next_graph[-1] = one more scan step), Dec-OCP GAE on the clipped costs, advantage with the multipliers."""
        cfg, T, B, hp = self.cfg, self.T, ro.B, self.hp
        n, nh, A = cfg.n_agents, self.n_cost, self.arena
        Vl, _ = self.values_prepass(ro, want_Vl=True, want_Vh=False)
        Vh = A.get("tg.Vh.lagr", B, T + 1, n, nh)
        block = max(1, min(B, self.prepass_graphs // (T + 1)))
        for e0 in range(0, B, block):
            Eb = min(block, B - e0)
            feats = self._block_feats("pre", ro, e0, Eb, 0, T + 1)
            act = self.Vh.forward(feats, n_seq=Eb * n, T=T + 1, h0=None, tag="pre", train=False)
            Vh[e0:e0 + Eb].copy_(act["v"].view(Eb, T + 1, n, nh))
        cpos = A.get("tg.costs_pos", B, T, n, nh)
        OA.relu_fwd(ro.costs, cpos)                                  # jnp.clip(rollout.costs, a_min=0)
        Qh = A.get("tg.Qh", B, T, n, nh)
        Ql = A.get("tg.Ql", B, T)
        OA.gae(cpos, ro.rewards, Vh, Vl, self.lam_pow, hp.gamma, hp.gae_lambda, Qh, Ql)
        adv = A.get("tg.adv", B, T, n)
        Ah = A.get("tg.Ah", B, T, n, nh)
        self.stats.zero_()
        OA.advantage_lagr(Ql, Vl, Qh, Vh, self.lagr, adv, Ah)
        return dict(Vl=Vl, Vh=Vh, Ql=Ql, Qh=Qh, adv=adv, Ah=Ah)

    def _net_streams(self):
        if self._side_streams is None:
            self._side_streams = [torch.cuda.Stream(self.device) for _ in range(3)]
        return self._side_streams

    def _opt_step(self, name: str, lr: float):
        """NaN check -> norm -> clip -> Adam on one network (trainer/utils.py:89-118 + optax); in the data-parallel path the
        gradients were summed over the ranks just before and are read as g / world."""
        net, opt = self.nets[name], self.opt[name]
        if self.grad_hook is not None:
            self.grad_hook(name, net, self._mb)
        OA.clip_adam_step(net.params, net.grads, opt.m, opt.v, opt.state, lr, self.hp.max_grad_norm,
                          grad_scale=1.0 / self.world)
        net.prepare()

    def targets(self, ro: RolloutData, det: RolloutData, step: int):
        """Vl/Vh pre-passes, the two GAEs and the advantage merge (dgppo.py:204-273)."""
        cfg, T, B, hp = self.cfg, self.T, ro.B, self.hp
        n, nh = cfg.n_agents, self.n_cost
        Vl, Vh = self.values_prepass(ro, want_Vl=True)
        _, Vh_det = self.values_prepass(det, want_Vl=False)
        A = self.arena
        Qh = A.get("tg.Qh", B, T, n, nh)
        Ql = A.get("tg.Ql", B, T)
        OA.gae(ro.costs, ro.rewards, Vh, Vl, self.lam_pow, hp.gamma, hp.gae_lambda, Qh, Ql)
        Qh_det = A.get("tg.Qh_det", B, T, n, nh)
        Ql_det = A.get("tg.Ql_det", B, T)
        OA.gae(det.costs, det.rewards, Vh_det, Vl, self.lam_pow, hp.gamma, hp.gae_lambda, Qh_det, Ql_det)
        adv = A.get("tg.adv", B, T, n)
        self.stats.zero_()
        OA.advantage(Ql, Vl, Vh, cfg.dt, hp.alpha, hp.cbf_eps, self.cbf_weight_at(step), adv, self.stats[3])
        return dict(Vl=Vl, Vh=Vh, Vh_det=Vh_det, Ql=Ql, Qh=Qh, Qh_det=Qh_det, adv=adv)

    def update(self, ro: RolloutData, det: RolloutData, step: int, perm: np.ndarray) -> dict:
        cfg, T, B, hp = self.cfg, self.T, ro.B, self.hp
        n, nh, H = cfg.n_agents, self.n_cost, nets.HID
        informarl = self.algo in ("informarl", "hcbfcrpo")          # these baselines train only Vl and the policy
        lagr = self.algo == "informarl_lagr"
        import time as _time
        th = [_time.perf_counter()]                # host-side issue times of the phases (diagnostics: self.host_ms)
        ro.finalize()
        if self.algo == "dgppo":
            det.finalize()
            if hp.use_rnn and not self._carry_mapped():
                det.rnn_states                       # the gathered form reads the env-major copy: made here, not under capture
        assert B * T >= hp.batch_size, "n_env_train * T must be >= batch_size (dgppo.py:153)"
        Eb = hp.batch_size // T
        assert B % Eb == 0 and T % hp.rnn_step == 0, "B % (batch_size // T) == 0 and T % rnn_step == 0 required (SURVEY A.11)"
        C = T // hp.rnn_step
        tg = (self.targets_informarl(ro, step) if self.algo == "informarl" else
              self.targets_hcbfcrpo(ro, step) if self.algo == "hcbfcrpo" else
              self.targets_lagr(ro, step) if lagr else self.targets(ro, det, step))
        th.append(_time.perf_counter())
        perm = np.asarray(perm)
        assert perm.size == 0 or (0 <= int(perm.min()) and int(perm.max()) < B), "perm holds env ids outside [0, B)"
        idx_all = torch.from_numpy(np.ascontiguousarray(perm.astype(np.int32))).to(self.device)   # int32 once per update
        n_mb = B // Eb
        G = Eb * T
        R = G * n
        is_cuda = self.device.type == "cuda"
        reduce = self.allreduce is not None
        A = self.arena
        # static inputs of one minibatch step: the env ids of the minibatch and everything gathered by them
        mb_idx32 = A.get("mb.idx32", Eb, dtype=torch.int32)
        Ql_mb = A.get("mb.Ql", Eb, T)
        act_mb = A.get("mb.act", Eb, T, n, 2)
        lp_old_mb = A.get("mb.lp_old", Eb, T, n)
        adv_mb = A.get("mb.adv", Eb, T, n)
        # one actor cell of width H: Vh's GRU reads the carry rows of the envs mb_idx32 in the record (_mb_carry); stacked cells
        # keep the gathered copy of layer 0 (their rows are HC wide, of which Vh reads the first H)
        h0_mapped = self._carry_mapped()
        if self.algo == "dgppo":
            h0_det = None if h0_mapped else A.get("mb.h0_det", Eb, T, n, H)
            Qh_det_mb = A.get("mb.Qh_det", Eb, T, n, nh)
        if lagr:
            Qh_mb = A.get("mb.Qh", Eb, T, n, nh)
            Vh_mb = A.get("mb.Vh", Eb, T + 1, n, nh)
            Ah_mb = A.get("mb.Ah", Eb, T, n, nh)

        ctx = {}

        def lagr_step(apply_now: bool):
            """update_lagr (informarl_lagr.py:286-309) with the UPDATED policy: log pi of the stored actions over whole
            episodes (zero carry), then the multiplier step — at once on one device; with a gradient exchange only this
            rank's sums here, the all-reduce of the sums and the step follow in exchange_lagr()."""
            full = self.policy.forward(ctx["feats"], n_seq=Eb * n, T=T, h0=None, tag="lg", train=False)
            lp_full = A.get("mb.lp_full", R)
            K.policy_head(full["ms"], self.eps_hat, act_mb.view(R, 2), None, lp_full, A.get("mb.ent_full", R), n, 2)
            if apply_now:
                OA.lagr_update(lp_full.view(Eb, T, n), lp_old_mb, Vh_mb, Ah_mb, self.lagr, self.lagr_sums, hp.gamma, hp.lr_lagr)
            else:
                OA.lagr_sums(lp_full.view(Eb, T, n), lp_old_mb, Vh_mb, Ah_mb, self.lagr_sums, hp.gamma)

        def body_pre():
            """device work of ONE minibatch up to the gradient exchange (dgppo.py:276-289): gathers and the three forward /
            backward passes (with the optimiser steps when there is no exchange) — reads the minibatch's env ids from
            mb_idx32."""
            main = torch.cuda.current_stream(self.device) if is_cuda else None
            side = self._net_streams() if (self.multi_stream and main is not None) else None
            self.stats[:3].zero_()
            # everything the three updates read is produced on the main stream first
            feats = ctx["feats"] = self._block_feats("mb", ro, 0, Eb, 0, T, env_ids=mb_idx32)
            pairs = [(tg["Ql"], Ql_mb)]
            if self.algo == "dgppo":
                feats_det = self._block_feats("mbd", det, 0, Eb, 0, T, env_ids=mb_idx32)
                full = None
                if h0_mapped:
                    pass
                elif self.HC == H:
                    pairs.append((det.rnn_states, h0_det))
                else:                                          # stacked cells: gather the packed carry, keep layer 0
                    full = A.get("mb.h0_det_full", Eb, T, n, self.HC)
                    pairs.append((det.rnn_states, full))
                pairs.append((tg["Qh_det"], Qh_det_mb))
            if lagr:
                pairs += [(tg["Qh"], Qh_mb), (tg["Vh"], Vh_mb), (tg["Ah"], Ah_mb)]
            pairs += [(ro.actions, act_mb), (ro.log_pis, lp_old_mb), (tg["adv"], adv_mb)]
            K.gather_rows(pairs, mb_idx32)                     # every per-env input of the minibatch in one launch
            if self.algo == "dgppo" and full is not None:
                h0_det.copy_(full[..., :H])

            def update_Vl():      # informarl.py:357-385: chunks of rnn_step with zero initial carry
                act = self.Vl.forward(feats, n_seq=Eb * C, T=hp.rnn_step, h0=None, tag="tr")
                dv = A.get("mb.dv", G, 1)
                K.value_loss(act["v"], Ql_mb.view(G, 1), dv, self.stats[0])
                self.Vl.zero_grads()
                self.Vl.backward(act, dv)
                if not reduce:
                    self._opt_step("Vl", hp.lr_Vl)

            def update_Vh():
                if lagr:          # informarl_lagr.py:252-284: chunks of rnn_step, zero initial carry, stochastic rollout
                    act = self.Vh.forward(feats, n_seq=Eb * C * n, T=hp.rnn_step, h0=None, tag="tr")
                    target = Qh_mb
                else:             # dgppo.py:296-321: the deterministic rollout with its stored carry
                    if h0_mapped:
                        h0 = self._mb_carry(det, mb_idx32)
                    else:
                        h0 = h0_det.view(R, H) if hp.use_rnn else None
                    act = self.Vh.forward(feats_det, n_seq=R, T=1, h0=h0, tag="tr")
                    target = Qh_det_mb
                dvh = A.get("mb.dvh", R, nh)
                K.value_loss(act["v"], target.view(R, nh), dvh, self.stats[1])
                self.Vh.zero_grads()
                self.Vh.backward(act, dvh)
                if not reduce:
                    self._opt_step("Vh", hp.lr_Vh)

            def update_policy():  # informarl.py:405-457
                act = self.policy.forward(feats, n_seq=Eb * C * n, T=hp.rnn_step, h0=None, tag="tr")
                lp = A.get("mb.lp", R)
                ent = A.get("mb.ent", R)
                dms = A.get("mb.dms", R, 4)
                K.policy_head(act["ms"], self.eps_hat, act_mb.view(R, 2), None, lp, ent, n, 2, lp_old_mb.view(R),
                              adv_mb.view(R), dms, self.stats[2], hp.clip_eps, hp.coef_ent)
                self.policy.zero_grads()
                self.policy.backward(act, dms)
                if not reduce:
                    self._opt_step("policy", hp.lr_actor)
                if lagr and not reduce:
                    lagr_step(apply_now=True)

            if informarl:
                update_Vh = lambda: None                       # noqa: E731  (no constraint-value network)
            if side is None:
                update_Vl(); update_Vh(); update_policy()
            else:
                # the three networks share no state: one HIP stream each, joined before the next minibatch touches the
                # shared inputs again (most of these kernels are latency-bound and leave CUs idle on their own)
                ready = main.record_event()
                for fn, st in ((update_policy, side[0]), (update_Vl, side[1]), (update_Vh, side[2])):
                    with torch.cuda.stream(st):
                        st.wait_event(ready)
                        fn()
                for st in side:
                    main.wait_stream(st)

        def body_post():
            """after the exchange: every rank applies the identical NaN-check -> norm -> clip -> Adam (replicas stay
            bit-identical)"""
            self._opt_step("Vl", hp.lr_Vl)
            if not informarl:
                self._opt_step("Vh", hp.lr_Vh)
            self._opt_step("policy", hp.lr_actor)
            if lagr:
                lagr_step(apply_now=False)

        def exchange_lagr():
            # the `.mean()` of the multiplier step runs over the GLOBAL minibatch: all-reduce the n * nh sums, then every rank
            # applies the identical step (informarl_lagr.py:300-306)
            self.allreduce(self.lagr_sums)
            OA.lagr_apply(self.lagr, self.lagr_sums, self.world * Eb * T, hp.lr_lagr)

        def exchange():
            # data-parallel exchange: ONE all-reduce(sum) of [g_policy | g_Vl | g_Vh | loss sums] per minibatch
            # once the three backward passes have joined
            self.allreduce(self.flat_grads[:self.n_reduced])

        def step_body():
            body_pre()
            if reduce:
                exchange()
                body_post()
                if lagr:
                    exchange_lagr()

        # The minibatch step is ~400 launches of 10-100 us kernels: issuing them from Python costs about as much host time
        # as they take on the device.  With use_graphs the step is captured once into a HIP graph (all its operands live in
        # persistent buffers; only mb_idx32 changes) and replayed for every further minibatch and iteration.  Not with a
        # gradient hook (a Python callback).  With a gradient exchange the step is TWO graphs — everything before the
        # collective, and the optimiser steps after it — with the collective issued eagerly between the replays, so that no
        # communication library call is ever recorded into a graph.
        slot = None
        if self.use_graphs and is_cuda and self.grad_hook is None:
            key = (self.algo, B, Eb, ro.agent.data_ptr(), det.agent.data_ptr() if det is not None else 0,
                   det.rnn_tm.data_ptr() if det is not None else 0,
                   tg["adv"].data_ptr(), tg["Ql"].data_ptr(), mb_idx32.data_ptr(), self._update_generation())
            slot = self._upd_graph
            if slot.get("key") != key:
                slot.clear()
                slot["key"] = key
        for mb in range(n_mb):
            self._mb = mb
            mb_idx32.copy_(idx_all[mb * Eb:(mb + 1) * Eb])
            if slot is not None and slot.get("graph") is not None:
                slot["graph"].replay()
                if reduce:
                    exchange()
                    slot["graph_post"].replay()
                    if lagr:
                        exchange_lagr()
                K.FLOPS[0] += slot["flops"]
                continue
            f0 = K.FLOPS[0]
            step_body()
            if slot is not None and not slot.get("failed", False):
                slot["flops"] = K.FLOPS[0] - f0
                if slot.get("key")[-1] != self._update_generation():      # the eager pass grew a scratch buffer: try again later
                    slot["key"] = slot["key"][:-1] + (self._update_generation(),)
                    continue
                graph = torch.cuda.CUDAGraph()
                try:
                    f1 = K.FLOPS[0]
                    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                        body_pre()
                    if reduce:
                        gpost = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gpost, capture_error_mode="thread_local"):
                            body_post()
                        slot["graph_post"] = gpost
                    K.FLOPS[0] = f1
                    slot["graph"] = graph
                except Exception as ex:                             # keep training: eager launches are always correct
                    slot["failed"] = True
                    torch.cuda.synchronize()
                    print(f"[dgppo_amd] HIP-graph capture of the minibatch step failed ({type(ex).__name__}: {ex}); "
                          f"continuing with eager launches", flush=True)
        th.append(_time.perf_counter())
        self._last = dict(Ql_mb=Ql_mb, G=G, R=R, nh=nh, B=B, Qh_mb=Qh_mb if lagr else None)
        out = self.info(ro)
        th.append(_time.perf_counter())
        # host time spent ISSUING finalize + targets, then the minibatch loop, then waiting for the device in info()
        self.host_ms = {"issue_targets": 1e3 * (th[1] - th[0]), "issue_minibatches": 1e3 * (th[2] - th[1]),
                        "wait_device": 1e3 * (th[3] - th[2])}
        return out

    def info(self, ro: RolloutData) -> dict:
        """scalars of the LAST minibatch (dgppo.py:292) with the reference's key names; one host sync.  Under data
        parallelism every value is GLOBAL: the loss / metric sums (stats rows 0..2) travelled with the gradients, the safe
        count and the target / log-pi extrema are reduced here over the host control plane (two tiny gloo collectives)."""
        from . import dist as D
        L = self._last
        s = self.stats.cpu().numpy().copy()
        n_bad = int(self.reset_failed.item())
        if n_bad:
            self.reset_failed.zero_()
            raise RuntimeError(f"env reset: {n_bad} environment(s) of the last rollouts got no valid scene within the kernels' "
                               f"rejection-loop bounds (too many agents / obstacles for the area?) — the batch is invalid")
        s[:3] /= self.world                                   # rows 0..2 were summed over the ranks with the gradients
        G, R, nh, B = L["G"], L["R"], L["nh"], L["B"]
        o = {k: self.opt[k].state[:8].cpu().numpy() for k in self.opt}
        pol_loss = s[2, 0] / R - self.hp.coef_ent * s[2, 1] / R
        lagr = self.algo == "informarl_lagr"
        ext = [float(L["Ql_mb"].max()), -float(L["Ql_mb"].min()), -float(ro.log_pis.min())]
        if lagr:
            ext += [float(L["Qh_mb"].max()), -float(L["Qh_mb"].min())]
        ext = D.host_allreduce(np.asarray(ext, np.float64), "max", self.world)
        sums = [s[3, 0]]
        mixed, self._mix_used = self._mix_used, False         # the same on every rank: the mix is a function of the flags
        if mixed:
            sums.append(float(self.scene_fallback.item()))
            self.scene_fallback.zero_()
        sums = D.host_allreduce(np.asarray(sums, np.float64), "sum", self.world)
        safe = float(sums[0])
        out = {
            "Vl/loss": float(s[0, 0] / G), "Vl/grad_norm": float(o["Vl"][4]), "Vl/has_nan": float(o["Vl"][5]),
            "Vl/max_target": float(ext[0]), "Vl/min_target": float(-ext[1]),
            "policy/loss": float(pol_loss), "policy/grad_norm": float(o["policy"][4]), "policy/has_nan": float(o["policy"][5]),
            "policy/log_pi_min": float(-ext[2]), "policy/clip_frac": float(s[2, 2] / R),
            "policy/entropy": float(s[2, 1] / R), "policy/total_variation_dist": float(0.5 * s[2, 3] / R),
        }
        if lagr:   # informarl_lagr.py:278-282,309
            out.update({"Vh/loss": float(s[1, 0] / (R * nh)), "Vh/grad_norm": float(o["Vh"][4]), "Vh/has_nan": float(o["Vh"][5]),
                        "Vh/max_target": float(ext[3]), "Vh/min_target": float(-ext[4]),
                        "policy/lagr_mean": float(self.lagr.mean())})
        if self.algo == "dgppo":       # InforMARL logs only the Vl and policy keys (informarl.py:357-457)
            out.update({"Vh/loss_Vh": float(s[1, 0] / (R * nh)), "Vh/grad_Vh_norm": float(o["Vh"][4]),
                        "Vh/grad_Vh_has_nan": float(o["Vh"][5])})
        if self.algo in ("dgppo", "hcbfcrpo"):   # hcbfcrpo.py:204
            out["eval/safe_data"] = safe / (self.world * B * self.T * self.cfg.n_agents)
        if mixed:                      # envs of this iteration's rollouts, over all ranks, that kept their reset; with a pool
            out["rollout/scene_fallback"] = float(sums[1])   # of mined scenes also those that drew a slot still empty
            pool, self._mix_pool = self._mix_pool, None
            if pool is not None:       # one rank only (train.py refuses more): the ring after this iteration's push
                st = pool.stats() if getattr(pool, "priority", False) else None      # one copy carries the fill too
                filled, pushed, taken = pool.fill() if st is None else (int(v) for v in st["state"][1:4])
                out.update({"rollout/scene_pool_fill": float(filled), "rollout/scene_pool_pushed": float(pushed),
                            "rollout/scene_pool_taken": float(taken)})
                if st is not None:             # what the iteration's score call and evicting push counted
                    live = pool.P + int(st["state"][1])
                    out.update({"rollout/scene_replay_fail_frac": float(st["state"][7]) / max(float(st["state"][6]), 1.0),
                                "rollout/scene_pool_evicted": float(st["state"][4]),
                                "rollout/scene_pool_dropped": float(st["state"][5]),
                                "rollout/scene_pool_score_mean": float(st["score"][:live].mean()) if live else 0.0})
        return out
