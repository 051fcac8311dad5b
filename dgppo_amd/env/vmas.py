"""VMASReverseTransport (dgppo/env/vmas/vmas_reverse_transport.py): n agents push a hollow box to a goal past three disc
obstacles, with the VMAS-style contact physics of dgppo/env/vmas/physax.  The step, reset and graph run in
csrc/env_vmas.hip (dgppo_vmas_* of include/dgppo_hip.h); this class is the reference's Python surface over them."""
from __future__ import annotations

import pathlib
import types
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import ops_env as OE
from ..utils.graph import GraphsTuple
from .base import MultiAgentEnv


class VMASReverseTransportState(NamedTuple):
    """vmas_reverse_transport.py:23-29 (field order of the reference)"""
    box_pos: torch.Tensor
    box_vel: torch.Tensor
    a_pos: torch.Tensor
    a_vel: torch.Tensor
    goal_pos: torch.Tensor
    o_pos: torch.Tensor


class VMASReverseTransport(MultiAgentEnv):
    AGENT = 0
    KIND = "VMASReverseTransport"
    PARAMS = {"comm_radius": 0.4, "default_area_size": 0.8, "dist2goal": 0.01, "agent_radius": 0.03}

    def __init__(self, num_agents: int, area_size: Optional[float] = None, max_step: int = 64, dt: float = 0.1,
                 params: Optional[dict] = None, device: Optional[torch.device] = None):
        # :45-63: the arena, the package and the obstacles are fixed by the task, whatever the caller passes.  Not through
        # MultiAgentEnv.__init__: that reads car_radius, n_obs, ... of PARAMS and writes to it, and this task's has neither
        self.half_width = 0.8
        self.agent_radius = 0.03
        self._params = dict(self.PARAMS) if params is None else params
        self._num_agents = num_agents
        self._area_size = 2 * self.half_width
        self._dt = dt
        self._max_step = max_step
        self._device = device
        self.package_width = self.package_length = 0.6
        self.package_mass = 10.0
        self.obs_radius = 0.15
        self.n_obs = 3
        self.frame_skip = 4
        if not 1 <= num_agents <= 16:
            raise ValueError(f"VMASReverseTransport supports 1 to 16 agents (got {num_agents})")
        self.cfg = N.make_vmas_cfg(num_agents, dt)
        self.num_goals = 0

    # ---- reference attribute surface (:65-88, 313-320) ----
    @property
    def state_dim(self) -> int:
        return 4

    @property
    def node_dim(self) -> int:
        return 20

    @property
    def edge_dim(self) -> int:
        return 4

    @property
    def action_dim(self) -> int:
        return 2

    @property
    def n_cost(self) -> int:
        return 2

    @property
    def cost_components(self) -> Tuple[str, ...]:
        return "agent collisions", "obstacle collisions"

    def state_lim(self, state=None):
        return None

    def action_lim(self):
        return -torch.ones(2), torch.ones(2)

    # ---- the compact state: agent [B, n, 4], body [B, 4] (box x, y, vx, vy), scene [B, 8] (goal | o0 | o1 | o2) ----
    def _env_states(self, st: OE.State):
        o = st.scene[..., 2:8].reshape(st.scene.shape[:-1] + (3, 2))
        return VMASReverseTransportState(st.body[..., 0:2], st.body[..., 2:4], st.agent[..., 0:2], st.agent[..., 2:4],
                                         st.scene[..., 0:2], o)

    # ---- reference single-graph interface = B = 1 view ----
    def _state_of(self, graph: GraphsTuple) -> OE.State:
        return self._batch_of_env_state(graph.env_states)

    def _batch_of_env_state(self, es: VMASReverseTransportState, lidar_data=None) -> OE.State:
        f = lambda x: torch.as_tensor(x, dtype=torch.float32, device=self.device)
        n = self.num_agents
        agent = torch.cat([f(es.a_pos).reshape(n, 2), f(es.a_vel).reshape(n, 2)], -1).reshape(1, n, 4).contiguous()
        body = torch.cat([f(es.box_pos).reshape(2), f(es.box_vel).reshape(2)]).reshape(1, 4).contiguous()
        scene = torch.cat([f(es.goal_pos).reshape(2), f(es.o_pos).reshape(6)]).reshape(1, 8).contiguous()
        return OE.State(dict(agent=agent, body=body), dict(scene=scene))

    def get_reward(self, graph: GraphsTuple, action=None):
        st = self._state_of(graph)
        zero = torch.zeros(1, self.num_agents, 2, device=self.device)
        return self.step_batch(st, zero)[1][0]

    # ---- rendering (:321-431) ----
    def render_video(self, rollout, video_path, Ta_is_unsafe=None, viz_opts: Optional[dict] = None, dpi: int = 100,
                     index: Optional[int] = None, max_frames: Optional[int] = None, **kwargs) -> pathlib.Path:
        """One episode: the arena, the goal, the obstacles, the box and the agents, with the distance and cost texts of the
        reference.  `.mp4` needs an ffmpeg binary; without one the frames go to a `.gif` (the path written is returned)."""
        if viz_opts:
            raise NotImplementedError(f"viz_opts {sorted(viz_opts)}: CBF / Vh overlays are not built")
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from . import plot

        es = rollout.graph.env_states
        npy = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        pick = (lambda x: npy(x)[index]) if index is not None else (lambda x: npy(x))
        box, a_pos, goal, o_pos = pick(es.box_pos), pick(es.a_pos), pick(es.goal_pos)[0], pick(es.o_pos)[0]
        costs = pick(rollout.costs)
        T = box.shape[0] if max_frames is None else min(box.shape[0], max_frames)
        hw, d2g = self.half_width, self._params["dist2goal"]
        fig, ax = plt.subplots(1, 1, figsize=(6, 6), dpi=dpi)
        ax.set_xlim(-1.01 * hw, 1.01 * hw)
        ax.set_ylim(-1.01 * hw, 1.01 * hw)
        ax.set_aspect("equal")
        ax.add_patch(plt.Rectangle((-hw, -hw), 2 * hw, 2 * hw, fc="none", ec="C3"))
        ax.add_patch(plt.Circle(goal, d2g, color="C5", alpha=0.5))
        for k in range(self.n_obs):
            ax.add_patch(plt.Circle(o_pos[k], self.obs_radius, fc="C0", ec="none", alpha=0.7))
        off = np.array([-self.package_length / 2, -self.package_width / 2])
        box_patch = plt.Rectangle(off, self.package_length, self.package_width, ec="C3", fc="none")
        box_centre = plt.Circle((0, 0), 0.5 * d2g, fc="C3", ec="none", zorder=6)
        ax.add_patch(box_patch)
        ax.add_patch(box_centre)
        agents = [plt.Circle((0, 0), self.agent_radius, color=f"C{i % 10}", zorder=5) for i in range(self.num_agents)]
        for p in agents:
            ax.add_patch(p)
        txt = dict(size=10, color="k", va="bottom", ha="right", transform=ax.transAxes)
        goal_text = ax.text(0.99, 1.00, "", **txt)
        obs_text = ax.text(0.99, 1.04, "", **txt)
        kk_text = ax.text(0.99, 1.08, "", **txt)
        cost_text = ax.text(0.99, 1.12, "", **txt)

        obs_r = self.obs_radius
        artists = [box_patch, box_centre, *agents, goal_text, obs_text, kk_text, cost_text]

        def draw(t):
            for i, p in enumerate(agents):
                p.set_center(tuple(a_pos[t, i]))
            box_patch.set_xy(off + box[t])
            box_centre.set_center(tuple(box[t]))
            d_obs = np.linalg.norm(box[t] - o_pos, axis=-1) - obs_r
            obs_text.set_text("dist_obs=[{}]".format(", ".join("{:+.3f}".format(d) for d in d_obs)))
            goal_text.set_text("dist_goal={:.3f}".format(np.linalg.norm(box[t] - goal)))
            kk_text.set_text("kk={:04}".format(t))
            cost_text.set_text("cost={}".format(", ".join("{:+.3f}".format(c) for c in costs[t].max(0))))
            return artists

        # the interface plot._write drives (fig, artists(), draw(t), close()), as plot._Scene provides it
        scene = types.SimpleNamespace(fig=fig, artists=lambda: artists, draw=draw, close=lambda: plt.close(fig))
        return plot._write(scene, T, video_path)
