"""Torch-tensor wrappers over the environment entry points of the C ABI (include/dgppo_hip.h).
Tensors are storage only; all arithmetic runs in the HIP kernels."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as N


STEP_FIELDS, ENV_FIELDS = ("agent", "hits", "body"), ("goal", "obst", "scene")     # every name record_fields can give


def record_fields(cfg: N.EnvCfg) -> tuple[Dict[str, tuple], Dict[str, tuple]]:
    """The compact record of an env kind: name -> trailing shape of the fields kept per (env, step) and of those kept per env.
    LiDAR / MPE: agent states (+ the top-k LiDAR hit points) per step, goals (+ obstacle records) per env;
    VMASReverseTransport: agents and the box (x, y, vx, vy) per step, scene = goal | 3 obstacle centres per env."""
    n, sd = cfg.n_agents, cfg.state_dim
    if cfg.is_vmas:
        return {"agent": (n, 4), "body": (4,)}, {"scene": (8,)}
    step, env = {"agent": (n, sd)}, {"goal": (cfg.n_goals, sd)}
    if cfg.is_lidar and cfg.n_obs > 0:
        step["hits"] = (n, cfg.top_k, 2)
    if cfg.n_obs > 0:
        env["obst"] = (cfg.n_obs, cfg.obst_stride)
    return step, env


class State:
    """Compact env state of any kind (device tensors with some leading batch shape): `step` and `env` hold the fields
    record_fields names, also readable as attributes (st.agent, st.hits, st.body, ...).  A field that is not held reads as
    None: obst / hits of a kind without obstacles, hits before sensing."""

    def __init__(self, step: Dict[str, torch.Tensor], env: Dict[str, torch.Tensor]):
        self.step = {k: v for k, v in step.items() if v is not None}
        self.env = {k: v for k, v in env.items() if v is not None}

    def __getattr__(self, name):
        if name in STEP_FIELDS:
            return self.step.get(name)
        if name in ENV_FIELDS:
            return self.env.get(name)
        raise AttributeError(name)

    @classmethod
    def empty(cls, cfg: N.EnvCfg, B: int, device) -> "State":
        step, env = record_fields(cfg)
        z = lambda shapes: {k: torch.empty(B, *s, device=device) for k, s in shapes.items()}
        return cls(z(step), z(env))

    def like(self) -> "State":
        """uninitialised per-step fields of the same shapes next to the same per-env fields: where a step writes to"""
        return State({k: torch.empty_like(v) for k, v in self.step.items()}, self.env)


def ray_tables(n_rays: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """cos/sin(linspace(-pi, pi-2pi/R, R)) in fp32 (dgppo/env/utils.py:51)."""
    thetas = np.linspace(-np.pi, np.pi - 2 * np.pi / n_rays, n_rays).astype(np.float32)
    rc = torch.from_numpy(np.cos(thetas).astype(np.float32)).to(device)
    rs = torch.from_numpy(np.sin(thetas).astype(np.float32)).to(device)
    return rc, rs


_RAYS: Dict[tuple, tuple] = {}


def _rays(cfg: N.EnvCfg, device):
    """the ray tables of a LiDAR kind, built once per (n_rays, device).  Building them copies from the host, which a HIP-graph
    capture does not allow: the first call has to be an eager one.  Engine.rollout sees to that: its reset and sense pass run
    outside the captured region, and the step loop runs eagerly once before it is captured."""
    if not cfg.is_lidar:
        return None, None
    key = (cfg.n_rays, device)
    if key not in _RAYS:
        _RAYS[key] = ray_tables(cfg.n_rays, device)
    return _RAYS[key]


def _graph_state_dim(cfg: N.EnvCfg) -> int:
    """columns of GraphsTuple.states: VMASReverseTransport's nodes carry none (vmas_reverse_transport.py:308)"""
    return 0 if cfg.is_vmas else cfg.state_dim


def alloc_graph(cfg: N.EnvCfg, B: int, device) -> Dict[str, torch.Tensor]:
    Nn, E = cfg.num_nodes, cfg.num_edges
    return dict(
        nodes=torch.empty(B, Nn, cfg.node_dim, device=device),
        edges=torch.empty(B, E, 4, device=device),
        states=torch.empty(B, Nn, _graph_state_dim(cfg), device=device),
        receivers=torch.empty(B, E, dtype=torch.int32, device=device),
        senders=torch.empty(B, E, dtype=torch.int32, device=device),
        node_type=torch.empty(B, Nn, dtype=torch.int32, device=device),
        n_node=torch.empty(B, dtype=torch.int32, device=device),
        n_edge=torch.empty(B, dtype=torch.int32, device=device),
    )


def _graph_out(cfg: N.EnvCfg, g: Dict[str, torch.Tensor], B: int) -> N.GraphOut:
    Nn, E = cfg.num_nodes, cfg.num_edges
    N.expect_shape(g["nodes"], (B, Nn, cfg.node_dim), "graph.nodes")
    N.expect_shape(g["edges"], (B, E, 4), "graph.edges")
    N.expect_shape(g["states"], (B, Nn, _graph_state_dim(cfg)), "graph.states")
    N.expect_shape(g["receivers"], (B, E), "graph.receivers")
    N.expect_shape(g["senders"], (B, E), "graph.senders")
    N.expect_shape(g["node_type"], (B, Nn), "graph.node_type")
    N.expect_shape(g["n_node"], (B,), "graph.n_node")
    N.expect_shape(g["n_edge"], (B,), "graph.n_edge")
    go = N.GraphOut()
    go.nodes = N.ptr(g["nodes"], name="graph.nodes")
    go.edges = N.ptr(g["edges"], name="graph.edges")
    go.states = N.ptr(g["states"], name="graph.states")
    go.receivers = N.ptr(g["receivers"], torch.int32, "graph.receivers")
    go.senders = N.ptr(g["senders"], torch.int32, "graph.senders")
    go.node_type = N.ptr(g["node_type"], torch.int32, "graph.node_type")
    go.n_node = N.ptr(g["n_node"], torch.int32, "graph.n_node")
    go.n_edge = N.ptr(g["n_edge"], torch.int32, "graph.n_edge")
    return go


def _check_state(cfg: N.EnvCfg, B: int, **given):
    """every field of the kind's record is given and has its shape, but for hits: they may be missing (before sensing), and
    the callers check the ones they get"""
    for fields in record_fields(cfg):
        for name, shape in fields.items():
            if given.get(name) is not None:
                N.expect_shape(given[name], (B,) + shape, name)
            elif name != "hits":
                raise ValueError(f"{name} is required by env kind {cfg.kind}")


def env_step(cfg: N.EnvCfg, agent, action, goal, obst, hits, ray_cos, ray_sin,
             next_agent, next_hits, reward, cost, graph: Optional[Dict[str, torch.Tensor]] = None):
    """dgppo_env_step.  action=None -> sense-only (graph of the given state)."""
    B = agent.shape[0]
    _check_state(cfg, B, agent=agent, goal=goal, obst=obst)
    n = cfg.n_agents
    if hits is not None:
        N.expect_shape(hits, (B, n, cfg.top_k, 2), "hits")
    if action is not None:
        N.expect_shape(action, (B, n, 2), "action")
        N.expect_shape(reward, (B,), "reward")
        N.expect_shape(cost, (B, n, cfg.n_cost), "cost")
    if next_agent is not None:
        N.expect_shape(next_agent, (B, n, cfg.state_dim), "next_agent")
    if next_hits is not None:
        N.expect_shape(next_hits, (B, n, cfg.top_k, 2), "next_hits")
    if cfg.is_lidar and cfg.n_obs > 0:
        N.expect_shape(ray_cos, (cfg.n_rays,), "ray_cos")
        N.expect_shape(ray_sin, (cfg.n_rays,), "ray_sin")
    go = _graph_out(cfg, graph, B) if graph is not None else None
    rc = N.lib().dgppo_env_step(
        C.byref(cfg), N.ptr(agent, name="agent"), N.ptr(action, name="action"), N.ptr(goal, name="goal"),
        N.ptr(obst, name="obst"), N.ptr(hits, name="hits"), N.ptr(ray_cos, name="ray_cos"), N.ptr(ray_sin, name="ray_sin"),
        N.ptr(next_agent, name="next_agent"), N.ptr(next_hits, name="next_hits"), N.ptr(reward, name="reward"),
        N.ptr(cost, name="cost"), C.byref(go) if go is not None else None, C.c_int32(B), N.stream_ptr())
    N.check(rc, "dgppo_env_step")


def graph_materialize(cfg: N.EnvCfg, agent, goal, obst, hits, graph: Dict[str, torch.Tensor]):
    B = agent.shape[0]
    _check_state(cfg, B, agent=agent, goal=goal, obst=obst)
    if hits is not None:
        N.expect_shape(hits, (B, cfg.n_agents, cfg.top_k, 2), "hits")
    go = _graph_out(cfg, graph, B)
    rc = N.lib().dgppo_graph_materialize(
        C.byref(cfg), N.ptr(agent, name="agent"), N.ptr(goal, name="goal"), N.ptr(obst, name="obst"),
        N.ptr(hits, name="hits"), C.byref(go), C.c_int32(B), N.stream_ptr())
    N.check(rc, "dgppo_graph_materialize")


def env_reset(cfg: N.EnvCfg, seeds: torch.Tensor, agent, goal, obst, n_failed: torch.Tensor = None):
    """n_failed: optional int32 device counter (caller-zeroed), += 1 per env whose bounded rejection loops ran out — read it at
    the next host sync and do not use the batch when it is non-zero (dgppo_env_reset_checked)."""
    B = seeds.shape[0]
    _check_state(cfg, B, agent=agent, goal=goal, obst=obst)
    if n_failed is not None:
        N.expect_shape(n_failed, (1,), "n_failed")
    rc = N.lib().dgppo_env_reset_checked(C.byref(cfg), N.ptr(seeds, torch.int64, "seeds"), N.ptr(agent, name="agent"),
                                         N.ptr(goal, name="goal"), N.ptr(obst, name="obst"),
                                         N.ptr(n_failed, torch.int32, "n_failed"), C.c_int32(B), N.stream_ptr())
    N.check(rc, "dgppo_env_reset")


def randn_rows(seed: int, out: torch.Tensor, global_row_len: int, col_offset: int):
    """out [rows, row_len] = the column window [col_offset, col_offset + row_len) of randn(seed) viewed as rows of
    global_row_len (data-parallel rollouts: a rank's share of the global noise)."""
    rows = int(out.shape[0])
    row_len = out.numel() // max(rows, 1)
    rc = N.lib().dgppo_randn_rows(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), N.ptr(out, name="out"), C.c_int64(rows),
                                  C.c_int64(row_len), C.c_int64(global_row_len), C.c_int64(col_offset), N.stream_ptr())
    N.check(rc, "dgppo_randn_rows")


def randn(seed: int, offset: int, out: torch.Tensor):
    rc = N.lib().dgppo_randn(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint64(offset), N.ptr(out, name="out"),
                             C.c_int64(out.numel()), N.stream_ptr())
    N.check(rc, "dgppo_randn")


# ---- VMASReverseTransport (include/dgppo_hip.h dgppo_vmas_*): agent [B, n, 4], body [B, 4], scene [B, 8] ------------------
def _check_vmas(cfg: N.EnvCfg, agent, body, scene, B):
    if not cfg.is_vmas:
        raise ValueError(f"env kind {cfg.kind} is not VMASReverseTransport")
    _check_state(cfg, B, agent=agent, body=body, scene=scene)


def vmas_reset(cfg: N.EnvCfg, seeds: torch.Tensor, agent, body, scene, n_failed: torch.Tensor = None):
    """dgppo_vmas_reset_checked; n_failed as in env_reset."""
    B = seeds.shape[0]
    _check_vmas(cfg, agent, body, scene, B)
    if n_failed is not None:
        N.expect_shape(n_failed, (1,), "n_failed")
    rc = N.lib().dgppo_vmas_reset_checked(C.byref(cfg), N.ptr(seeds, torch.int64, "seeds"), N.ptr(agent, name="agent"),
                                          N.ptr(body, name="body"), N.ptr(scene, name="scene"),
                                          N.ptr(n_failed, torch.int32, "n_failed"), C.c_int32(B), N.stream_ptr())
    N.check(rc, "dgppo_vmas_reset_checked")


def vmas_step(cfg: N.EnvCfg, agent, body, scene, action, next_agent, next_body, reward, cost,
              graph: Optional[Dict[str, torch.Tensor]] = None):
    """dgppo_vmas_step: reward / cost of the pre-step state, the optional graph of the post-step state."""
    B = agent.shape[0]
    _check_vmas(cfg, agent, body, scene, B)
    n = cfg.n_agents
    N.expect_shape(action, (B, n, 2), "action")
    N.expect_shape(next_agent, (B, n, 4), "next_agent")
    N.expect_shape(next_body, (B, 4), "next_body")
    N.expect_shape(reward, (B,), "reward")
    N.expect_shape(cost, (B, n, 2), "cost")
    go = _graph_out(cfg, graph, B) if graph is not None else None
    rc = N.lib().dgppo_vmas_step(
        C.byref(cfg), N.ptr(agent, name="agent"), N.ptr(body, name="body"), N.ptr(scene, name="scene"),
        N.ptr(action, name="action"), N.ptr(next_agent, name="next_agent"), N.ptr(next_body, name="next_body"),
        N.ptr(reward, name="reward"), N.ptr(cost, name="cost"), C.byref(go) if go is not None else None, C.c_int32(B),
        N.stream_ptr())
    N.check(rc, "dgppo_vmas_step")


def vmas_graph_materialize(cfg: N.EnvCfg, agent, body, scene, graph: Dict[str, torch.Tensor]):
    B = agent.shape[0]
    _check_vmas(cfg, agent, body, scene, B)
    go = _graph_out(cfg, graph, B)
    rc = N.lib().dgppo_vmas_graph_materialize(C.byref(cfg), N.ptr(agent, name="agent"), N.ptr(body, name="body"),
                                              N.ptr(scene, name="scene"), C.byref(go), C.c_int32(B), N.stream_ptr())
    N.check(rc, "dgppo_vmas_graph_materialize")


# ---- the operations over a State of any kind: the only place that knows which entry points serve which kind ---------------
def sense(cfg: N.EnvCfg, st: State, graph: Optional[Dict[str, torch.Tensor]] = None):
    """fills st.hits (allocated here if the state has none yet) from the rest of the state: the sense-only dgppo_env_step,
    which also writes the graph of the state if asked"""
    s, e = st.step, st.env
    if "hits" not in s:
        s["hits"] = torch.empty(s["agent"].shape[:-2] + record_fields(cfg)[0]["hits"], device=s["agent"].device)
    rc, rs = _rays(cfg, s["agent"].device)
    env_step(cfg, s["agent"], None, e["goal"], e.get("obst"), None, rc, rs, None, s["hits"], None, None, graph)


def reset(cfg: N.EnvCfg, seeds: torch.Tensor, st: State, n_failed: torch.Tensor = None,
          graph: Optional[Dict[str, torch.Tensor]] = None):
    """the episode start of seeds [B] into st (State.empty), sensed where the record has hits; n_failed as in env_reset"""
    if cfg.is_vmas:
        vmas_reset(cfg, seeds, st.agent, st.body, st.scene, n_failed)
    else:
        env_reset(cfg, seeds, st.agent, st.goal, st.obst, n_failed)
    if "hits" in st.step:
        sense(cfg, st, graph)
    elif graph is not None:
        materialize(cfg, st, graph)


def scene_template_shapes(cfg: N.EnvCfg) -> Dict[str, tuple]:
    """name -> trailing shape of the template rows dgppo_env_scene_load reads per scene: agent and goal rows in the record's own
    layout, obstacles as (cx, cy, w, h, theta) for the LiDAR kinds and (ox, oy) for the MPE kinds (no entry without obstacles)"""
    shapes = {"agent": (cfg.n_agents, cfg.state_dim), "goal": (cfg.n_goals, cfg.state_dim)}
    if cfg.n_obs > 0:
        shapes["obst"] = (cfg.n_obs, 5 if cfg.is_lidar else 2)
    return shapes


def scene_load(cfg: N.EnvCfg, scenes_dev: Dict[str, torch.Tensor], scene_ids, seeds, jitter: float, st: State, flags=None,
               n_failed=None):
    """dgppo_env_scene_load: the dense state st (State.empty, B envs) from the S template scenes scenes_dev (device tensors by
    scene_template_shapes, each with a leading S).  Env b takes scene scene_ids[b] — a host array or list of B ints, checked here
    against [0, S) (a tensor is read back for that) — or b % S without a list.  jitter > 0 moves every agent's x, y by up to that
    much, drawn from seeds [B] (int64 tensor) and retried up to 16 times until the scene is valid; seeds may be None at jitter
    0.  flags [B] int32 (optional) receives the validity bits (N.SCENE_BITS, 0 = valid), n_failed as in env_reset: touched only
    at jitter > 0.  hits are not sensed here: scene_start does that.  Every refusal is raised before anything is launched."""
    fn = "scene_load"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    B = int(st.agent.shape[0])
    _check_state(cfg, B, agent=st.agent, goal=st.goal, obst=st.obst)
    shapes = scene_template_shapes(cfg)
    agent_t = scenes_dev.get("agent")
    if not torch.is_tensor(agent_t) or agent_t.ndim != 3 or agent_t.shape[0] < 1:
        raise ValueError(f"{fn}: scenes_dev['agent'] must be a [S, n, sd] tensor with S >= 1")
    S = int(agent_t.shape[0])
    for name, shape in shapes.items():
        if not torch.is_tensor(scenes_dev.get(name)):
            raise ValueError(f"{fn}: scenes_dev has no {name}")
        N.expect_shape(scenes_dev[name], (S,) + shape, f"scenes_dev.{name}")
    jitter = float(jitter)
    if not jitter >= 0.0:
        raise ValueError(f"{fn}: jitter must be >= 0 (got {jitter})")
    if seeds is None and jitter > 0.0:
        raise ValueError(f"{fn}: seeds are required with jitter > 0")
    if seeds is not None:
        N.expect_shape(seeds, (B,), "seeds")
    ids_dev = None
    if scene_ids is not None:
        ids = np.asarray(scene_ids.cpu() if torch.is_tensor(scene_ids) else scene_ids)
        if ids.shape != (B,) or ids.dtype.kind not in "iu":
            raise ValueError(f"{fn}: scene_ids must be {B} ints (got shape {ids.shape}, dtype {ids.dtype})")
        if B and (int(ids.min()) < 0 or int(ids.max()) >= S):
            raise ValueError(f"{fn}: scene_ids outside [0, {S})")
        ids_dev = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(st.agent.device)
    if flags is not None:
        N.expect_shape(flags, (B,), "flags")
    if n_failed is not None:
        N.expect_shape(n_failed, (1,), "n_failed")
    rc = N.lib().dgppo_env_scene_load(
        C.byref(cfg), N.ptr(agent_t, name="scenes_dev.agent"), N.ptr(scenes_dev["goal"], name="scenes_dev.goal"),
        N.ptr(scenes_dev.get("obst") if cfg.n_obs > 0 else None, name="scenes_dev.obst"), S, N.ptr(ids_dev, torch.int32, "scene_ids"),
        N.ptr(seeds, torch.int64, "seeds"), jitter, N.ptr(st.agent, name="agent"), N.ptr(st.goal, name="goal"),
        N.ptr(st.obst, name="obst"), N.ptr(flags, torch.int32, "flags"), N.ptr(n_failed, torch.int32, "n_failed"), B,
        N.stream_ptr())
    N.check(rc, "dgppo_env_scene_load")


def scene_start(cfg: N.EnvCfg, scenes_dev: Dict[str, torch.Tensor], scene_ids, seeds, jitter: float, st: State, flags=None,
                n_failed=None, graph: Optional[Dict[str, torch.Tensor]] = None):
    """the episode start of user-given scenes into st: scene_load, then what reset does after its kernel — sensed where the
    record has hits, the graph written where one is asked for"""
    scene_load(cfg, scenes_dev, scene_ids, seeds, jitter, st, flags, n_failed)
    if "hits" in st.step:
        sense(cfg, st, graph)
    elif graph is not None:
        materialize(cfg, st, graph)


def _scene_mix_operands(cfg: N.EnvCfg, scenes_dev, seeds, jitter, st: State, flags, n_fallback, fn: str = "scene_mix"):
    """every refusal of scene_mix but those of scene_of -> (S, jitter); launches nothing"""
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    B = int(st.agent.shape[0])
    _check_state(cfg, B, agent=st.agent, goal=st.goal, obst=st.obst)
    shapes = scene_template_shapes(cfg)
    agent_t = scenes_dev.get("agent")
    if not torch.is_tensor(agent_t) or agent_t.ndim != 3 or agent_t.shape[0] < 1:
        raise ValueError(f"{fn}: scenes_dev['agent'] must be a [S, n, sd] tensor with S >= 1")
    S = int(agent_t.shape[0])
    for name, shape in shapes.items():
        if not torch.is_tensor(scenes_dev.get(name)):
            raise ValueError(f"{fn}: scenes_dev has no {name}")
        N.expect_shape(scenes_dev[name], (S,) + shape, f"scenes_dev.{name}")
    jitter = float(jitter)
    if not jitter >= 0.0:
        raise ValueError(f"{fn}: jitter must be >= 0 (got {jitter})")
    if seeds is None:
        raise ValueError(f"{fn}: seeds are required")
    N.expect_shape(seeds, (B,), "seeds")
    if flags is not None:
        N.expect_shape(flags, (B,), "flags")
    if n_fallback is not None:
        N.expect_shape(n_fallback, (1,), "n_fallback")
    return S, jitter


def _scene_mix_checked(cfg: N.EnvCfg, scenes_dev, scene_of, seeds, jitter, st: State, flags, n_fallback):
    """every refusal of scene_mix -> (S, jitter, scene_of as int32 on the host); launches nothing"""
    fn = "scene_mix"
    S, jitter = _scene_mix_operands(cfg, scenes_dev, seeds, jitter, st, flags, n_fallback)
    B = int(st.agent.shape[0])
    if scene_of is None:
        raise ValueError(f"{fn}: scene_of is required")
    of = np.asarray(scene_of.cpu() if torch.is_tensor(scene_of) else scene_of)
    if of.shape != (B,) or of.dtype.kind not in "iu":
        raise ValueError(f"{fn}: scene_of must be {B} ints (got shape {of.shape}, dtype {of.dtype})")
    if B and int(of.max()) >= S:
        raise ValueError(f"{fn}: scene_of outside [-inf, {S})")
    return S, jitter, np.ascontiguousarray(np.maximum(of.astype(np.int64), -1), np.int32)


def _scene_mix_launch(cfg: N.EnvCfg, scenes_dev, S: int, of, seeds, jitter: float, st: State, flags, n_fallback):
    """of: the checked host array, or a device int32 tensor that is trusted to be in range (scene_pool_draw wrote it)"""
    of_dev = of if torch.is_tensor(of) else torch.from_numpy(of).to(st.agent.device)
    rc = N.lib().dgppo_env_scene_mix(
        C.byref(cfg), N.ptr(scenes_dev["agent"], name="scenes_dev.agent"), N.ptr(scenes_dev["goal"], name="scenes_dev.goal"),
        N.ptr(scenes_dev.get("obst") if cfg.n_obs > 0 else None, name="scenes_dev.obst"), S, N.ptr(of_dev, torch.int32, "scene_of"),
        N.ptr(seeds, torch.int64, "seeds"), jitter, N.ptr(st.agent, name="agent"), N.ptr(st.goal, name="goal"),
        N.ptr(st.obst, name="obst"), N.ptr(flags, torch.int32, "flags"), N.ptr(n_fallback, torch.int32, "n_fallback"),
        int(st.agent.shape[0]), N.stream_ptr())
    N.check(rc, "dgppo_env_scene_mix")


def scene_mix(cfg: N.EnvCfg, scenes_dev: Dict[str, torch.Tensor], scene_of, seeds, jitter: float, st: State, flags=None,
              n_fallback=None):
    """dgppo_env_scene_mix: some envs of the dense state st, which already holds a valid reset, restart in the template scenes
    scenes_dev (as scene_load takes them).  scene_of — a host array or list of B ints, checked here against [-inf, S) (a tensor
    is read back for that) — keeps env b where it is negative and names its scene otherwise; seeds [B] (int64 tensor) and
    jitter as in scene_load.  An env whose scene is or stays invalid keeps its reset: flags [B] int32 (optional; kept envs'
    entries are not written) receives its bits and n_fallback (optional int32 [1], caller-zeroed) gains 1.  hits are not
    sensed here: mixed_start does that.  Every refusal is raised before anything is launched."""
    S, jitter, of = _scene_mix_checked(cfg, scenes_dev, scene_of, seeds, jitter, st, flags, n_fallback)
    _scene_mix_launch(cfg, scenes_dev, S, of, seeds, jitter, st, flags, n_fallback)


def mixed_start(cfg: N.EnvCfg, seeds: torch.Tensor, st: State, scenes_dev: Dict[str, torch.Tensor], scene_of, jitter: float,
                n_failed=None, n_fallback=None, graph: Optional[Dict[str, torch.Tensor]] = None):
    """the episode start of a training batch that mixes sampled and given starts: the reset of every env (n_failed as in
    env_reset), scene_mix over it (n_fallback as there), then what reset does after its kernel — sensed where the record has
    hits, the graph written where one is asked for.  The mix's refusals come before the reset is launched."""
    S, jitter, of = _scene_mix_checked(cfg, scenes_dev, scene_of, seeds, jitter, st, None, n_fallback)
    env_reset(cfg, seeds, st.agent, st.goal, st.obst, n_failed)
    _scene_mix_launch(cfg, scenes_dev, S, of, seeds, jitter, st, None, n_fallback)
    if "hits" in st.step:
        sense(cfg, st, graph)
    elif graph is not None:
        materialize(cfg, st, graph)


def mixed_start_drawn(cfg: N.EnvCfg, seeds: torch.Tensor, st: State, scenes_dev: Dict[str, torch.Tensor], scene_of: torch.Tensor,
                      jitter: float, flags=None, n_failed=None, n_fallback=None, graph: Optional[Dict[str, torch.Tensor]] = None):
    """mixed_start with the scene_of that scene_pool_draw wrote: a device int32 [B] tensor, trusted to be in range, so nothing is
    copied to the host and nothing waits for the device.  flags [B] int32 (optional) receives the bits of the envs scene_of names
    (scene_pool_score reads them)."""
    fn = "mixed_start_drawn"
    S, jitter = _scene_mix_operands(cfg, scenes_dev, seeds, jitter, st, flags, n_fallback, fn)
    if not (torch.is_tensor(scene_of) and scene_of.is_cuda and scene_of.dtype == torch.int32):
        raise ValueError(f"{fn}: scene_of must be the device int32 tensor of scene_pool_draw (scene_mix takes host lists)")
    N.expect_shape(scene_of, (int(st.agent.shape[0]),), "scene_of")
    env_reset(cfg, seeds, st.agent, st.goal, st.obst, n_failed)
    _scene_mix_launch(cfg, scenes_dev, S, scene_of, seeds, jitter, st, flags, n_fallback)
    if "hits" in st.step:
        sense(cfg, st, graph)
    elif graph is not None:
        materialize(cfg, st, graph)


MINED_FIELDS = ("first", "who", "t0", "flags")          # the int32 [B] outputs of scene_mine, next to the template rows


def alloc_mined(cfg: N.EnvCfg, B: int, device) -> Dict[str, torch.Tensor]:
    """the outputs of scene_mine for B envs: first, who, t0, flags (int32 [B]) and the template rows agent, goal[, obst]
    (scene_template_shapes with a leading B), uninitialised"""
    out = {k: torch.empty(B, dtype=torch.int32, device=device) for k in MINED_FIELDS}
    out.update({k: torch.empty(B, *s, device=device) for k, s in scene_template_shapes(cfg).items()})
    return out


def _time_major(x: torch.Tensor, lead: int, B: int, tail: tuple, name: str) -> int:
    """x [lead, B, *tail], dense but for its step stride -> Bs, the envs per time slot of its allocation (x may be the first B
    envs of a wider record: RolloutData.prefix)"""
    N.expect_shape(x, (lead, B) + tuple(tail), name)
    row = int(np.prod(tail))
    inner = tuple(int(np.prod(tail[k + 1:])) for k in range(len(tail)))
    st = x.stride()
    if tuple(st[2:]) != inner or st[1] != row or st[0] % row or st[0] < B * row:
        raise ValueError(f"{name}: a time-major record [T, B, ...] with dense rows is required (strides {tuple(st)})")
    return int(st[0]) // row


def scene_mine(cfg: N.EnvCfg, agent_tm, cost_tm, goal, obst, back: int, thresh: float, out: Dict[str, torch.Tensor]):
    """dgppo_env_scene_mine: for every env of the time-major record agent_tm [T+1, B, n, sd], cost_tm [T, B, n, n_cost] (dense,
    or the first B envs of a wider record: the step stride is read off the tensors) with the per-env rows goal [B, ng, sd] and
    obst [B, n_obs, stride] (None without obstacles), the first step with a cost word >= thresh, and the state `back` steps
    before it as template rows, into out (alloc_mined).  Every refusal is raised before anything is launched."""
    fn = "scene_mine"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    if not (torch.is_tensor(agent_tm) and agent_tm.ndim == 4 and agent_tm.shape[0] >= 2):
        raise ValueError(f"{fn}: agent_tm must be a [T+1, B, n, sd] tensor with T >= 1")
    T, B = int(agent_tm.shape[0]) - 1, int(agent_tm.shape[1])
    n, sd = cfg.n_agents, cfg.state_dim
    Bs = _time_major(agent_tm, T + 1, B, (n, sd), "agent_tm")
    if _time_major(cost_tm, T, B, (n, cfg.n_cost), "cost_tm") != Bs:
        raise ValueError(f"{fn}: agent_tm and cost_tm must be views of records with the same number of envs")
    _check_state(cfg, B, agent=agent_tm[0], goal=goal, obst=obst)
    back, thresh = int(back), float(thresh)
    if back < 0:
        raise ValueError(f"{fn}: back must be >= 0 (got {back})")
    if not np.isfinite(thresh):
        raise ValueError(f"{fn}: thresh must be finite (got {thresh})")
    for k in MINED_FIELDS:
        N.expect_shape(out[k], (B,), f"out.{k}")
    for k, s in scene_template_shapes(cfg).items():
        N.expect_shape(out[k], (B,) + s, f"out.{k}")
    if B == 0:
        return
    for x, name in ((agent_tm, "agent_tm"), (cost_tm, "cost_tm")):
        if not x.is_cuda or x.dtype != torch.float32:
            raise TypeError(f"{fn}: {name} must be a float32 tensor on the GPU")
    i32 = torch.int32
    rc = N.lib().dgppo_env_scene_mine(
        C.byref(cfg), C.c_void_p(agent_tm.data_ptr()), C.c_void_p(cost_tm.data_ptr()), Bs, N.ptr(goal, name="goal"),
        N.ptr(obst if cfg.n_obs > 0 else None, name="obst"), T, back, thresh, N.ptr(out["first"], i32, "out.first"),
        N.ptr(out["who"], i32, "out.who"), N.ptr(out["t0"], i32, "out.t0"), N.ptr(out["flags"], i32, "out.flags"),
        N.ptr(out["agent"], name="out.agent"), N.ptr(out["goal"], name="out.goal"),
        N.ptr(out.get("obst") if cfg.n_obs > 0 else None, name="out.obst"), B, N.stream_ptr())
    N.check(rc, "dgppo_env_scene_mine")


def scene_pool_push(cfg: N.EnvCfg, mined: Dict[str, torch.Tensor], pool: Dict[str, torch.Tensor], fixed: int, state, slot_of=None):
    """dgppo_env_scene_pool_push: the rows of the taken envs of `mined` (scene_mine's outputs: first >= 1 and flags == 0) into
    the ring of pool slots fixed .. M-1 of `pool` (agent, goal[, obst], each [M, ...] in the template shapes), in env order from
    state[0] = head on; state (int32 [4] on the device: head, filled, pushed_total, taken_last) is advanced, slot_of (int32 [B],
    optional) receives every env's slot or -1.  Every refusal is raised before anything is launched."""
    fn = "scene_pool_push"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    shapes = scene_template_shapes(cfg)
    B, M = int(mined["first"].shape[0]), int(pool["agent"].shape[0])
    fixed = int(fixed)
    if not (M >= 1 and 0 <= fixed < M):
        raise ValueError(f"{fn}: need M >= 1 and 0 <= fixed < M (got M {M}, fixed {fixed})")
    N.expect_shape(mined["flags"], (B,), "mined.flags")
    for k, s in shapes.items():
        N.expect_shape(mined[k], (B,) + s, f"mined.{k}")
        N.expect_shape(pool[k], (M,) + s, f"pool.{k}")
    N.expect_shape(state, (4,), "state")
    if slot_of is not None:
        N.expect_shape(slot_of, (B,), "slot_of")
    i32, obst = torch.int32, cfg.n_obs > 0
    rc = N.lib().dgppo_env_scene_pool_push(
        C.byref(cfg), N.ptr(mined["first"], i32, "mined.first"), N.ptr(mined["flags"], i32, "mined.flags"),
        N.ptr(mined["agent"], name="mined.agent"), N.ptr(mined["goal"], name="mined.goal"),
        N.ptr(mined["obst"] if obst else None, name="mined.obst"), N.ptr(pool["agent"], name="pool.agent"),
        N.ptr(pool["goal"], name="pool.goal"), N.ptr(pool["obst"] if obst else None, name="pool.obst"), M, fixed,
        N.ptr(state, i32, "state"), N.ptr(slot_of, i32, "slot_of"), B, N.stream_ptr())
    N.check(rc, "dgppo_env_scene_pool_push")


# ---- the pool by priority (csrc/env_scene_pool.hip) ---------------------------------------------------------------------------
POOL_MAX_M, POOL_MAX_AGE = 65536, 1024
POOL_STATS = ("score", "visits", "last")


def alloc_pool_stats(M: int, device) -> Dict[str, torch.Tensor]:
    """the per-slot statistics of a pool of M slots, as a new pool has them (every score 0.5, no visit, last step 0), the int32 [8]
    state, and the scratch of the three entry points: tally int32 [2 M] (zero between calls), cum int64 [M], order int32 [M]"""
    i32 = torch.int32
    return {"score": torch.full((M,), 0.5, device=device), "visits": torch.zeros(M, dtype=i32, device=device),
            "last": torch.zeros(M, dtype=i32, device=device), "state": torch.zeros(8, dtype=i32, device=device),
            "tally": torch.zeros(2 * M, dtype=i32, device=device), "cum": torch.empty(M, dtype=torch.int64, device=device),
            "order": torch.empty(M, dtype=i32, device=device)}


def _check_pool_stats(fn: str, stats: Dict[str, torch.Tensor], M: int):
    if not 1 <= M <= POOL_MAX_M:
        raise ValueError(f"{fn}: M must be in [1, {POOL_MAX_M}] (got {M})")
    for k in POOL_STATS + ("cum", "order"):
        N.expect_shape(stats[k], (M,), f"stats.{k}")
    N.expect_shape(stats["tally"], (2 * M,), "stats.tally")
    N.expect_shape(stats["state"], (8,), "stats.state")


def scene_pool_score(cfg: N.EnvCfg, scene_of, mix_flags, first, stats: Dict[str, torch.Tensor], beta: float, step: int):
    """dgppo_env_scene_pool_score: what the replays of a rollout did — scene_of [B] from scene_pool_draw, mix_flags [B] from the
    rollout's scene mix, first [B] from scene_mine of its record, all device int32 — folded into stats (alloc_pool_stats):
    score, visits, last of every replayed slot, state[6] = replays, state[7] = failed replays.  Two launches, no sync."""
    fn = "scene_pool_score"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    M, B = int(stats["score"].shape[0]), int(scene_of.shape[0])
    _check_pool_stats(fn, stats, M)
    beta = float(beta)
    if not 0.0 < beta <= 1.0:
        raise ValueError(f"{fn}: beta must be in (0, 1] (got {beta})")
    N.expect_shape(mix_flags, (B,), "mix_flags")
    N.expect_shape(first, (B,), "first")
    i32 = torch.int32
    rc = N.lib().dgppo_env_scene_pool_score(
        C.byref(cfg), N.ptr(scene_of, i32, "scene_of"), N.ptr(mix_flags, i32, "mix_flags"), N.ptr(first, i32, "first"),
        N.ptr(stats["score"], name="stats.score"), N.ptr(stats["visits"], i32, "stats.visits"), N.ptr(stats["last"], i32, "stats.last"),
        N.ptr(stats["tally"], i32, "stats.tally"), M, beta, int(step), N.ptr(stats["state"], i32, "stats.state"), B, N.stream_ptr())
    N.check(rc, "dgppo_env_scene_pool_score")


def scene_pool_draw(cfg: N.EnvCfg, stats: Dict[str, torch.Tensor], fixed: int, age_cap: int, step: int, draw_seed: int, n_total: int,
                    n_scene: int, lo: int, scene_of: torch.Tensor):
    """dgppo_env_scene_pool_draw: scene_of (device int32 [B]) of the global envs lo .. lo + B - 1 of a batch of n_total envs of
    which n_scene start in a slot: the scene envs are those of env.scenes.mix_assignment, each draws a live slot in proportion
    to q(score) * min(1 + max(step - last, 0), age_cap); every other env, and every env while no slot is live, gets -1.  One
    launch, no sync.  Every refusal is raised before anything is launched."""
    fn = "scene_pool_draw"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    M, B = int(stats["score"].shape[0]), int(scene_of.shape[0])
    _check_pool_stats(fn, stats, M)
    fixed, age_cap, step, n_total, n_scene, lo = (int(v) for v in (fixed, age_cap, step, n_total, n_scene, lo))
    if not 0 <= fixed < M:
        raise ValueError(f"{fn}: fixed must be in [0, M) (got {fixed}, M {M})")
    if not 1 <= age_cap <= POOL_MAX_AGE:
        raise ValueError(f"{fn}: age_cap must be in [1, {POOL_MAX_AGE}] (got {age_cap})")
    if not (1 <= n_total < 2 ** 31 and 0 <= n_scene <= n_total):
        raise ValueError(f"{fn}: need 1 <= n_total < 2^31 and 0 <= n_scene <= n_total (got n_total {n_total}, n_scene {n_scene})")
    if not (0 <= lo and lo + B <= n_total):
        raise ValueError(f"{fn}: the window [{lo}, {lo + B}) lies outside the batch of {n_total}")
    i32 = torch.int32
    rc = N.lib().dgppo_env_scene_pool_draw(
        C.byref(cfg), N.ptr(stats["score"], name="stats.score"), N.ptr(stats["last"], i32, "stats.last"),
        N.ptr(stats["state"], i32, "stats.state"), M, fixed, age_cap, step, int(draw_seed) & (2 ** 64 - 1), n_total, n_scene, lo,
        N.ptr(stats["cum"], torch.int64, "stats.cum"), N.ptr(scene_of, i32, "scene_of"), B, N.stream_ptr())
    N.check(rc, "dgppo_env_scene_pool_draw")


def scene_pool_push_evict(cfg: N.EnvCfg, mined: Dict[str, torch.Tensor], pool: Dict[str, torch.Tensor], fixed: int,
                          stats: Dict[str, torch.Tensor], min_visits: int, evict_w: float, step: int, slot_of=None):
    """dgppo_env_scene_pool_push_evict: scene_pool_push with eviction by priority: the taken envs of `mined` go to the empty ring
    slots first, then over the filled ones with visits >= min_visits and w(score) <= evict_w, in ring order from head; the rest
    are dropped.  A written slot restarts at score 0.5, no visit, last = step; stats["state"] (int32 [8]) is advanced.  One launch,
    no sync.  Every refusal is raised before anything is launched."""
    fn = "scene_pool_push_evict"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no scene entry point")
    shapes = scene_template_shapes(cfg)
    B, M = int(mined["first"].shape[0]), int(pool["agent"].shape[0])
    fixed, min_visits, evict_w = int(fixed), int(min_visits), float(evict_w)
    _check_pool_stats(fn, stats, M)
    if not 0 <= fixed < M:
        raise ValueError(f"{fn}: fixed must be in [0, M) (got {fixed}, M {M})")
    if min_visits < 0:
        raise ValueError(f"{fn}: min_visits must be >= 0 (got {min_visits})")
    if not 0.0 <= evict_w <= 1.0:
        raise ValueError(f"{fn}: evict_w must be in [0, 1] (got {evict_w})")
    N.expect_shape(mined["flags"], (B,), "mined.flags")
    for k, s in shapes.items():
        N.expect_shape(mined[k], (B,) + s, f"mined.{k}")
        N.expect_shape(pool[k], (M,) + s, f"pool.{k}")
    if slot_of is not None:
        N.expect_shape(slot_of, (B,), "slot_of")
    i32, obst = torch.int32, cfg.n_obs > 0
    rc = N.lib().dgppo_env_scene_pool_push_evict(
        C.byref(cfg), N.ptr(mined["first"], i32, "mined.first"), N.ptr(mined["flags"], i32, "mined.flags"),
        N.ptr(mined["agent"], name="mined.agent"), N.ptr(mined["goal"], name="mined.goal"),
        N.ptr(mined["obst"] if obst else None, name="mined.obst"), N.ptr(pool["agent"], name="pool.agent"),
        N.ptr(pool["goal"], name="pool.goal"), N.ptr(pool["obst"] if obst else None, name="pool.obst"),
        N.ptr(stats["score"], name="stats.score"), N.ptr(stats["visits"], i32, "stats.visits"), N.ptr(stats["last"], i32, "stats.last"),
        N.ptr(stats["order"], i32, "stats.order"), M, fixed, min_visits, evict_w, int(step), N.ptr(stats["state"], i32, "stats.state"),
        N.ptr(slot_of, i32, "slot_of"), B, N.stream_ptr())
    N.check(rc, "dgppo_env_scene_pool_push_evict")


def step(cfg: N.EnvCfg, st: State, action, nst: State, reward, cost, graph: Optional[Dict[str, torch.Tensor]] = None):
    """one env step from st into the per-step fields of nst (st.like()): reward [B] and cost [B, n, n_cost] of the pre-step
    state, the optional graph of the post-step state"""
    s, e, ns = st.step, st.env, nst.step         # the dicts: cheaper than attributes, and this runs in every rollout step
    if cfg.is_vmas:
        return vmas_step(cfg, s["agent"], s["body"], e["scene"], action, ns["agent"], ns["body"], reward, cost, graph)
    rc, rs = _rays(cfg, s["agent"].device)
    env_step(cfg, s["agent"], action, e["goal"], e.get("obst"), s.get("hits"), rc, rs, ns["agent"], ns.get("hits"), reward,
             cost, graph)


def act_step_feats_supported(cfg: N.EnvCfg, Fp: int, H: int) -> bool:
    """does the configuration have the one-launch rollout step (dgppo_env_act_step_feats) at node width Fp and H heads?"""
    return bool(N.lib().dgppo_env_act_step_feats_supported(C.byref(cfg), C.c_int32(Fp), C.c_int32(H)))


def act_step_feats(cfg: N.EnvCfg, st: State, ms, eps, action, log_pi, nst: State, reward, cost, Xa=None, Xo=None, efeat=None,
                   emask=None, Fp: int = 8, Mcat=None, cvec=None, qt0=None, H: int = 3, max_blocks: int = 0):
    """dgppo_env_act_step_feats: the action from the head output ms [B * n, 4] (eps [B * n, 2] given: sampled, with log_pi
    [B, n]; eps None: tanh(mean)), the env step from st into nst with it, and — where given — the graph features Xa / Xo /
    efeat / emask of the new state (GraphFeats buffers) and its layer-0 queries qt0 = Xa Mcat + cvec"""
    s, e, ns = st.step, st.env, nst.step
    agent = s["agent"]
    B, n = agent.shape[0], cfg.n_agents
    rc, rs = _rays(cfg, agent.device)
    sample = eps is not None
    N.expect_shape(ms, (B * n, 4), "ms")
    N.expect_shape(action, (B, n, 2), "action")
    N.expect_shape(ns["agent"], (B, n, cfg.state_dim), "next_agent")
    N.expect_shape(ns["hits"], (B, n, cfg.top_k, 2), "next_hits")
    N.expect_shape(reward, (B,), "reward")
    N.expect_shape(cost, (B, n, cfg.n_cost), "cost")
    if sample:
        N.expect_shape(eps, (B * n, 2), "eps")
        N.expect_shape(log_pi, (B, n), "log_pi")
    if Xa is not None:
        S = cfg.fan_in
        N.expect_shape(Xa, (B * n, Fp), "Xa")
        N.expect_shape(Xo, (B * (cfg.num_nodes - 1 - n), Fp), "Xo")
        N.expect_shape(efeat, (B * n, S, 4), "efeat")
        N.expect_shape(emask, (B * n, S), "emask")
    if qt0 is not None:
        N.expect_shape(Mcat, (Fp, H * Fp), "Mcat")
        N.expect_shape(cvec, (H * Fp,), "cvec")
        N.expect_shape(qt0, (B * n, H * Fp), "qt0")
    rc_ = N.lib().dgppo_env_act_step_feats(
        C.byref(cfg), N.ptr(agent, name="agent"), N.ptr(e["goal"], name="goal"), N.ptr(e.get("obst"), name="obst"),
        N.ptr(s.get("hits"), name="hits"), N.ptr(rc, name="ray_cos"), N.ptr(rs, name="ray_sin"), N.ptr(ms, name="ms"),
        N.ptr(eps, name="eps"), C.c_int32(1 if sample else 0), N.ptr(action, name="action"),
        N.ptr(log_pi if sample else None, name="log_pi"), N.ptr(ns["agent"], name="next_agent"),
        N.ptr(ns["hits"], name="next_hits"), N.ptr(reward, name="reward"), N.ptr(cost, name="cost"), N.ptr(Xa, name="Xa"),
        N.ptr(Xo if Xa is not None else None, name="Xo"), N.ptr(efeat if Xa is not None else None, name="efeat"),
        N.ptr(emask if Xa is not None else None, name="emask"), C.c_int32(Fp), N.ptr(Mcat, name="Mcat"),
        N.ptr(cvec, name="cvec"), N.ptr(qt0, name="qt0"), C.c_int32(H), C.c_int32(max_blocks), C.c_int32(B), N.stream_ptr())
    N.check(rc_, "dgppo_env_act_step_feats")


def sweep_fork(cfg: N.EnvCfg, step: Dict[str, torch.Tensor], env: Dict[str, torch.Tensor], frame_ids, n_frames: int,
               agent_id: int, xs, ys, out: State, carry=None, carry_st: int = 0, carry_out=None, frame_max=None):
    """dgppo_env_sweep_fork: the G = n_frames * ny * nx what-if envs of a sweep into `out` (State.empty(cfg, G, device)) — env
    (f * ny + iy) * nx + ix is frame frame_ids[f] of ONE env with agent `agent_id` at (xs[ix], ys[iy]), its LiDAR cast again
    there.  `step` holds that env's per-step fields [T + 1, ...], `env` its per-env rows (GraphFeats.compute_sweep's operands);
    xs / ys are ops_nn.sweep_axis tensors; frame_ids as in ops_nn.graph_feats_sweep.  carry: a base tensor whose [n, HC] rows of
    frame t start at t * carry_st floats, copied into carry_out [G * n, HC] for every grid point of the frame; None: no carry.
    Every refusal is raised before anything is launched."""
    from . import ops_nn as K                     # the grid and record checks the sweep bindings share
    fn = "sweep_fork"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no sweep entry point")
    n, sd, k = cfg.n_agents, cfg.state_dim, cfg.top_k
    agent, hits, obst, goal = step["agent"], step.get("hits"), env.get("obst"), env["goal"]
    nx, ny, ids, ids_dev, last = K._sweep_grid(fn, cfg, frame_ids, n_frames, agent_id, xs, ys, frame_max)
    G = n_frames * ny * nx
    rc, rs = _rays(cfg, agent.device)
    cast = K._sweep_record(fn, cfg, agent, n * sd, obst, hits, n * k * 2, rc, rs, last, None, G)
    N.expect_shape(goal, (cfg.n_goals, sd), "goal")
    o_step, o_env = out.step, out.env
    for fields, held in zip(record_fields(cfg), (o_step, o_env)):
        for name, shape in fields.items():
            if held.get(name) is None:
                raise ValueError(f"{fn}: out has no {name}")
            N.expect_shape(held[name], (G,) + shape, f"out.{name}")
    HC = 0
    if carry is not None:
        if carry_out is None or carry_out.ndim != 2 or carry_out.shape[0] != G * n:
            raise ValueError(f"{fn}: carry_out must be [G * n, HC] = [{G * n}, HC]")
        HC = int(carry_out.shape[1])
        K._check_strided(fn, "carry", carry, 0, int(carry_st), (n, HC), None, 1, last + 1)
    if ids is not None:
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(agent.device)
    raw = lambda t_: C.c_void_p(t_.data_ptr())       # a view into the record: only its trailing block is dense (checked above)
    rc_ = N.lib().dgppo_env_sweep_fork(
        C.byref(cfg), raw(agent), n * sd, N.ptr(goal, name="goal"), N.ptr(obst, name="obst"), raw(hits) if cast else None,
        n * k * 2, N.ptr(rc if cast else None, name="ray_cos"), N.ptr(rs if cast else None, name="ray_sin"),
        N.ptr(ids_dev, torch.int32, "frame_ids"), n_frames, int(agent_id), N.ptr(xs, name="xs"), nx, N.ptr(ys, name="ys"), ny,
        raw(carry) if carry is not None else None, int(carry_st), HC, N.ptr(o_step["agent"], name="out.agent"),
        N.ptr(o_env["goal"], name="out.goal"), N.ptr(o_env.get("obst"), name="out.obst"),
        N.ptr(o_step.get("hits") if cast else None, name="out.hits"),
        N.ptr(carry_out if carry is not None else None, name="carry_out"), N.stream_ptr())
    N.check(rc_, "dgppo_env_sweep_fork")


def team_action_fork(cfg: N.EnvCfg, st: State, a_pol, us, vs, out: State, action_out, carry=None, carry_out=None):
    """dgppo_env_team_action_fork: the G = B * n * P what-if envs of one lookahead-shield step into `out` (State.empty(cfg, G,
    device)), P = 1 + nv * nu — env (e * n + i) * P + p is a copy of env e of the dense state `st` (B envs), and action_out
    [G, n, 2] its joint action: a_pol[e] [n, 2] with row i replaced by candidate p (0: a_pol[e, i]; 1 + iv * nu + iu: (us[iu],
    vs[iv]); unclipped, the step clips).  us / vs are ops_nn.sweep_axis tensors.  carry [B * n, HC] is copied into carry_out
    [G * n, HC] for every copy of its env; None: no carry.  Every refusal is raised before anything is launched."""
    from . import ops_nn as K                     # the operand checks the shield bindings share
    fn = "team_action_fork"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no fork entry point")
    n = cfg.n_agents
    if not (torch.is_tensor(a_pol) and a_pol.ndim == 3):
        raise ValueError(f"{fn}: a_pol must be a [B, n, 2] tensor")
    B = int(a_pol.shape[0])
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.ndim == 1 and t_.numel() > 0):
            raise ValueError(f"{fn}: {name} must be a non-empty 1-D tensor (sweep_axis)")
    P = 1 + int(us.numel()) * int(vs.numel())
    G = B * n * P
    operands = [("a_pol", a_pol, (B, n, 2)), ("action_out", action_out, (G, n, 2))]
    for fields, src, dst in zip(record_fields(cfg), (st.step, st.env), (out.step, out.env)):
        for name, shape in fields.items():
            if src.get(name) is None:
                raise ValueError(f"{fn}: the state has no {name}")
            if dst.get(name) is None:
                raise ValueError(f"{fn}: out has no {name}")
            operands += [(name, src[name], (B,) + shape), (f"out.{name}", dst[name], (G,) + shape)]
    HC = 0
    if carry is not None:
        if not (torch.is_tensor(carry) and carry.ndim == 2 and carry.shape[0] == B * n and carry.shape[1] >= 1):
            raise ValueError(f"{fn}: carry must be [B * n, HC] = [{B * n}, HC]")
        HC = int(carry.shape[1])
        if carry_out is None:
            raise ValueError(f"{fn}: carry_out is required with a carry")
        operands += [("carry", carry, (B * n, HC)), ("carry_out", carry_out, (G * n, HC))]
    K._shaped(fn, operands)
    nu, nv = K._shield_axes(fn, us, vs)
    cast = cfg.is_lidar and cfg.n_obs > 0
    s, e, o_s, o_e = st.step, st.env, out.step, out.env
    rc = N.lib().dgppo_env_team_action_fork(
        C.byref(cfg), N.ptr(s["agent"], name="agent"), N.ptr(e["goal"], name="goal"), N.ptr(e.get("obst"), name="obst"),
        N.ptr(s["hits"] if cast else None, name="hits"), N.ptr(a_pol, name="a_pol"), N.ptr(carry, name="carry"), HC, B,
        N.ptr(us, name="us"), nu, N.ptr(vs, name="vs"), nv, N.ptr(o_s["agent"], name="out.agent"),
        N.ptr(o_e["goal"], name="out.goal"), N.ptr(o_e.get("obst"), name="out.obst"),
        N.ptr(o_s["hits"] if cast else None, name="out.hits"), N.ptr(action_out, name="action_out"),
        N.ptr(carry_out if carry is not None else None, name="carry_out"), N.stream_ptr())
    N.check(rc, "dgppo_env_team_action_fork")


def team_action_fork_ids(cfg: N.EnvCfg, st: State, a_base, env_ids, us, vs, out: State, action_out, carry=None, carry_out=None,
                         ids_dev=None):
    """dgppo_env_team_action_fork_ids: team_action_fork for the envs env_ids of the dense state `st` (B envs) only, with the
    joint action a_base [B, n, 2] — the action held after the shield rounds so far — in the place of the policy's.  Output env
    (m * n + i) * P + p of the G = len(env_ids) * n * P in `out` is a copy of env env_ids[m]; row i of action_out [G, n, 2] is
    candidate p (0: a_base[e, i] itself), every other row a_base[e]'s; carry [B * n, HC] rows of env e go to carry_out
    [G * n, HC].  env_ids: a 1-D host array of ints in [0, B) (checked here; the kernel trusts it), or None for every env in
    order.  ids_dev: the same list as an int32 device tensor, where the caller has uploaded it already.  Every refusal is raised
    before anything is launched."""
    from . import ops_nn as K
    fn = "team_action_fork_ids"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no fork entry point")
    n = cfg.n_agents
    if not (torch.is_tensor(a_base) and a_base.ndim == 3):
        raise ValueError(f"{fn}: a_base must be a [B, n, 2] tensor")
    B = int(a_base.shape[0])
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.ndim == 1 and t_.numel() > 0):
            raise ValueError(f"{fn}: {name} must be a non-empty 1-D tensor (sweep_axis)")
    ids, M = K.env_id_list(fn, env_ids, B, unique=False)
    P = 1 + int(us.numel()) * int(vs.numel())
    G = M * n * P
    operands = [("a_base", a_base, (B, n, 2)), ("action_out", action_out, (G, n, 2))]
    for fields, src, dst in zip(record_fields(cfg), (st.step, st.env), (out.step, out.env)):
        for name, shape in fields.items():
            if src.get(name) is None:
                raise ValueError(f"{fn}: the state has no {name}")
            if dst.get(name) is None:
                raise ValueError(f"{fn}: out has no {name}")
            operands += [(name, src[name], (B,) + shape), (f"out.{name}", dst[name], (G,) + shape)]
    HC = 0
    if carry is not None:
        if not (torch.is_tensor(carry) and carry.ndim == 2 and carry.shape[0] == B * n and carry.shape[1] >= 1):
            raise ValueError(f"{fn}: carry must be [B * n, HC] = [{B * n}, HC]")
        HC = int(carry.shape[1])
        if carry_out is None:
            raise ValueError(f"{fn}: carry_out is required with a carry")
        operands += [("carry", carry, (B * n, HC)), ("carry_out", carry_out, (G * n, HC))]
    K._shaped(fn, operands)
    nu, nv = K._shield_axes(fn, us, vs)
    ids = K.env_ids_device(fn, ids, ids_dev, a_base.device)
    cast = cfg.is_lidar and cfg.n_obs > 0
    s, e, o_s, o_e = st.step, st.env, out.step, out.env
    rc = N.lib().dgppo_env_team_action_fork_ids(
        C.byref(cfg), N.ptr(s["agent"], name="agent"), N.ptr(e["goal"], name="goal"), N.ptr(e.get("obst"), name="obst"),
        N.ptr(s["hits"] if cast else None, name="hits"), N.ptr(a_base, name="a_base"), N.ptr(carry, name="carry"), HC, B,
        N.ptr(ids, torch.int32, "env_ids"), M, N.ptr(us, name="us"), nu, N.ptr(vs, name="vs"), nv,
        N.ptr(o_s["agent"], name="out.agent"), N.ptr(o_e["goal"], name="out.goal"), N.ptr(o_e.get("obst"), name="out.obst"),
        N.ptr(o_s["hits"] if cast else None, name="out.hits"), N.ptr(action_out, name="action_out"),
        N.ptr(carry_out if carry is not None else None, name="carry_out"), N.stream_ptr())
    N.check(rc, "dgppo_env_team_action_fork_ids")


def action_sweep_fork(cfg: N.EnvCfg, step: Dict[str, torch.Tensor], env: Dict[str, torch.Tensor], actions, frame_ids,
                      n_frames: int, agent_id: int, us, vs, out: State, action_out, carry=None, carry_st: int = 0, carry_out=None,
                      frame_max=None):
    """dgppo_env_action_sweep_fork: the G = n_frames * nv * nu what-if envs of an action rollout landscape into `out`
    (State.empty(cfg, G, device)) — env (f * nv + iv) * nu + iu is a copy of frame frame_ids[f] of ONE env, and action_out
    [G, n, 2] its joint action: the recorded rows of that frame with row `agent_id` replaced by (us[iu], vs[iv]) (unclipped, the
    step clips).  `step` holds that env's per-step fields [T + 1, ...], `env` its per-env rows (sweep_fork's operands), `actions`
    its recorded actions [T, n, 2]; us / vs are ops_nn.sweep_axis tensors; frame_ids as in ops_nn.graph_feats_sweep.  carry: a
    base tensor whose [n, HC] rows of frame t start at t * carry_st floats — the carries AFTER each frame's policy forward —
    copied into carry_out [G * n, HC] for every grid action of the frame; None: no carry.  Nothing is cast: the hits are the
    recorded ones.  Every refusal is raised before anything is launched."""
    from . import ops_nn as K                     # the grid and record checks the sweep bindings share
    fn = "action_sweep_fork"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no fork entry point")
    n, sd, k = cfg.n_agents, cfg.state_dim, cfg.top_k
    agent, hits, obst, goal = step["agent"], step.get("hits"), env.get("obst"), env["goal"]
    cast = cfg.is_lidar and cfg.n_obs > 0
    o_step, o_env = out.step, out.env
    # what is wrong with the call itself comes first, then shapes, then frame strides; only then where the operands live
    if not 0 <= int(agent_id) < n:
        raise ValueError(f"{fn}: agent_id {agent_id} outside [0, {n})")
    if int(n_frames) < 1:
        raise ValueError(f"{fn}: n_frames must be >= 1 (got {n_frames})")
    if not cast and (hits is not None or o_step.get("hits") is not None):
        raise ValueError(f"{fn}: hits are for the kinds that cast rays (LiDAR with obstacles)")
    if cast and hits is None:
        raise ValueError(f"{fn}: hits is required for a LiDAR kind with obstacles")
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.ndim == 1 and t_.numel() > 0):
            raise ValueError(f"{fn}: {name} must be a non-empty 1-D tensor (sweep_axis)")
    G = int(n_frames) * int(vs.numel()) * int(us.numel())
    shapes = [("action_out", action_out, (G, n, 2)), ("goal", goal, (cfg.n_goals, sd))]
    if cfg.n_obs > 0:
        if obst is None:
            raise ValueError(f"{fn}: obst is required when n_obs > 0")
        shapes.append(("obst", obst, (cfg.n_obs, cfg.obst_stride)))
    for fields, held in zip(record_fields(cfg), (o_step, o_env)):
        for name, shape in fields.items():
            if held.get(name) is None:
                raise ValueError(f"{fn}: out has no {name}")
            shapes.append((f"out.{name}", held[name], (G,) + shape))
    HC = 0
    if carry is not None:
        if carry_out is None or not torch.is_tensor(carry_out) or carry_out.ndim != 2 or carry_out.shape[0] != G * n:
            raise ValueError(f"{fn}: carry_out must be [G * n, HC] = [{G * n}, HC]")
        HC = int(carry_out.shape[1])
        shapes.append(("carry_out", carry_out, (G * n, HC)))
    for name, t_, shape in shapes:
        if not torch.is_tensor(t_) or tuple(t_.shape) != tuple(shape):
            got = tuple(t_.shape) if torch.is_tensor(t_) else type(t_).__name__
            raise ValueError(f"{fn}: {name}: expected shape {tuple(shape)}, got {got}")
    # a record field [frames, ...] is read at its own frame stride (a view of a larger slab serves as it is)
    fst = lambda t_, inner: int(t_.stride(0)) if torch.is_tensor(t_) and t_.ndim == len(inner) + 1 and t_.shape[0] > 1 \
        else int(np.prod(inner))
    strided = [("agent", agent, fst(agent, (n, sd)), (n, sd)), ("actions", actions, fst(actions, (n, 2)), (n, 2))]
    if cast:
        strided.append(("hits", hits, fst(hits, (n, k, 2)), (n, k, 2)))
    if carry is not None:
        strided.append(("carry", carry, int(carry_st), (n, HC)))
    for name, t_, st_, inner in strided:
        if not torch.is_tensor(t_):
            raise ValueError(f"{fn}: {name} must be a tensor")
        if st_ < int(np.prod(inner)):
            raise ValueError(f"{fn}: the frame stride of {name} ({st_}) is shorter than its {inner} rows")
    nu, nv, ids, ids_dev, last = K._sweep_grid(fn, cfg, frame_ids, n_frames, agent_id, us, vs, frame_max, ("us", "vs"))
    K._shaped(fn, shapes)
    for name, t_, st_, inner in strided:
        K._check_strided(fn, name, t_, 0, st_, inner, None, 1, last + 1)
    if ids is not None:
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(agent.device)
    raw = lambda t_: C.c_void_p(t_.data_ptr())       # a view into the record: only its trailing block is dense (checked above)
    rc_ = N.lib().dgppo_env_action_sweep_fork(
        C.byref(cfg), raw(agent), strided[0][2], N.ptr(goal, name="goal"), N.ptr(obst, name="obst"), raw(hits) if cast else None,
        strided[2][2] if cast else 0, raw(actions), strided[1][2], raw(carry) if carry is not None else None, int(carry_st), HC,
        N.ptr(ids_dev, torch.int32, "frame_ids"), n_frames, int(agent_id), N.ptr(us, name="us"), nu, N.ptr(vs, name="vs"), nv,
        N.ptr(o_step["agent"], name="out.agent"), N.ptr(o_env["goal"], name="out.goal"), N.ptr(o_env.get("obst"), name="out.obst"),
        N.ptr(o_step.get("hits") if cast else None, name="out.hits"), N.ptr(action_out, name="action_out"),
        N.ptr(carry_out if carry is not None else None, name="carry_out"), N.stream_ptr())
    N.check(rc_, "dgppo_env_action_sweep_fork")


def materialize(cfg: N.EnvCfg, st: State, graph: Dict[str, torch.Tensor]):
    if cfg.is_vmas:
        return vmas_graph_materialize(cfg, st.agent, st.body, st.scene, graph)
    graph_materialize(cfg, st.agent, st.goal, st.obst, st.hits, graph)
