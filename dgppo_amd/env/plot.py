"""Episode rendering for test.py (the reference's dgppo/env/plot.py:206 `render_mpe` and :468
`render_lidar`, called through `env.render_video`, dgppo/env/lidar_env/base.py:209-221, dgppo/env/mpe/base.py).

Host-side only (matplotlib): one episode's GraphsTuple sequence is copied to NumPy once, then every frame moves the
agent circles, rebuilds the edge segments from (senders, receivers) minus the pad node, and rewrites the cost / reward /
unsafe / step texts.  What a frame shows follows the reference: agents in blue with their index, goals in green,
obstacles in dark red (rectangles for the LiDAR family, discs for MPE), communication edges in grey, agent-goal edges in
green, LiDAR hit points as the far end of agent-hit edges.  The container is whatever matplotlib can write here: `.mp4`
needs an ffmpeg binary (the reference's default); without one the same frames go to an animated `.gif` next to the
requested path (Pillow writer) and the path actually written is returned."""
from __future__ import annotations

import pathlib
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

AGENT_COLOR, GOAL_COLOR, OBS_COLOR, COMM_COLOR = "#0068ff", "#2fdd00", "#8a0000", "0.2"


class Episode(NamedTuple):
    """one episode on the host: T frames of a fixed-topology padded graph"""
    states: np.ndarray        # [T, N, sd]   node states, pad node last
    senders: np.ndarray       # [T, E]
    receivers: np.ndarray     # [T, E]
    rewards: np.ndarray       # [T]
    costs: np.ndarray         # [T, n, n_cost]
    rect_points: Optional[np.ndarray]   # [n_obs, 4, 2] LiDAR rectangles (static within an episode) or None
    discs: Optional[np.ndarray]         # [n_obs, 2] MPE obstacle centres or None


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def episode_from_rollout(rollout, index: Optional[int] = None) -> Episode:
    """Slice one episode out of a Rollout.  `rollout.graph` carries [T, ...] (a single episode, as the reference passes
    it) or [B, T, ...] (this build's batched rollouts: pick `index`)."""
    g = rollout.graph
    batched = g.states.ndim == 4
    if batched and index is None:
        if g.states.shape[0] != 1:
            raise ValueError("batched rollout: pass the episode index")
        index = 0
    pick = (lambda a: _np(a[index])) if batched else _np       # slice on the device, copy one episode
    es = g.env_states
    rect = discs = None
    if getattr(es, "obstacle", None) is not None:
        pts = pick(es.obstacle.points)                         # [T, n_obs, 4, 2] or [n_obs, 4, 2]
        rect = pts[0] if pts.ndim == 4 else pts
    elif getattr(es, "obs", None) is not None:
        o = pick(es.obs)
        discs = (o[0] if o.ndim == 3 else o)[:, :2]
    return Episode(pick(g.states), pick(g.senders), pick(g.receivers), pick(rollout.rewards), pick(rollout.costs), rect,
                   discs)


def frame_edges(ep: Episode, t: int, n_agent: int, n_goal: int) -> Tuple[np.ndarray, np.ndarray]:
    """segments [e, 2, 2] of frame t and a flag per segment: sender is a goal node.  Edges touching the pad node (the last
    node) are dropped — masked edges are re-routed pad -> pad by the graph builder (utils/graph.py:212-247)."""
    pad = ep.states.shape[1] - 1
    s, r = ep.senders[t], ep.receivers[t]
    keep = (s != pad) & (r != pad)
    s, r = s[keep], r[keep]
    pos = ep.states[t, :, :2]
    seg = np.stack([pos[s], pos[r]], axis=1)
    finite = np.isfinite(seg).all(axis=(1, 2))                # a LiDAR hit point can be NaN (parallel ray): not drawable
    return seg[finite], ((s >= n_agent) & (s < n_agent + n_goal))[finite]


def unsafe_agents(ep: Episode, t: int, Ta_is_unsafe=None) -> np.ndarray:
    """indices of the agents flagged unsafe at frame t (test.py:103-105: any cost component >= 0)"""
    if Ta_is_unsafe is not None:
        return np.flatnonzero(_np(Ta_is_unsafe)[t])
    return np.flatnonzero((ep.costs[t] >= 0.0).any(axis=-1))


def _centred_scale(h: np.ndarray):
    """-> (norm, levels): one colour scale for a whole episode of contours, centred at 0 (15 levels)"""
    from matplotlib.colors import CenteredNorm
    half = float(np.nanmax(np.abs(h))) if np.isfinite(h).any() else 1.0
    norm = CenteredNorm(vcenter=0.0, halfrange=half if half > 0.0 else 1.0)
    return norm, np.linspace(-norm.halfrange, norm.halfrange, 15)


def _drawable(z: np.ndarray) -> bool:
    return bool(np.isfinite(z).all()) and z.shape[0] >= 2 and z.shape[1] >= 2


class _Scene:
    """the artists of one figure; `draw(t)` moves them to frame t"""

    def __init__(self, ep: Episode, side_length: float, n_agent: int, n_goal: int, r: float, obs_r: float,
                 cost_components: Sequence[str], Ta_is_unsafe, dpi: int, landscape=None, cost_landscape=None,
                 action_landscape=None, rollout_landscape=None, action_rollout_landscape=None):
        if action_rollout_landscape is not None:
            R = action_rollout_landscape
            for name, other in (("landscape", landscape), ("cost_landscape", cost_landscape),
                                ("action_landscape", action_landscape), ("rollout_landscape", rollout_landscape)):
                if other is not None and int(other.agent) != int(R.agent):
                    raise ValueError(f"action_rollout_landscape is swept for agent {int(R.agent)}, {name} for agent "
                                     f"{int(other.agent)}")
            if action_landscape is not None and not (np.array_equal(np.asarray(action_landscape.us), np.asarray(R.us))
                                                     and np.array_equal(np.asarray(action_landscape.vs), np.asarray(R.vs))):
                raise ValueError("action_landscape and action_rollout_landscape are swept over different grids")
        if rollout_landscape is not None:
            for name, other in (("landscape", landscape), ("cost_landscape", cost_landscape),
                                ("action_landscape", action_landscape)):
                if other is not None and int(other.agent) != int(rollout_landscape.agent):
                    raise ValueError(f"rollout_landscape is swept for agent {int(rollout_landscape.agent)}, {name} for agent "
                                     f"{int(other.agent)}")
            for name, other in (("landscape", landscape), ("cost_landscape", cost_landscape)):
                if other is not None and not (np.array_equal(np.asarray(other.xs), np.asarray(rollout_landscape.xs))
                                              and np.array_equal(np.asarray(other.ys), np.asarray(rollout_landscape.ys))):
                    raise ValueError(f"{name} and rollout_landscape are swept over different grids")
        if action_landscape is not None:
            for name, other in (("landscape", landscape), ("cost_landscape", cost_landscape)):
                if other is not None and int(other.agent) != int(action_landscape.agent):
                    raise ValueError(f"action_landscape is swept for agent {int(action_landscape.agent)}, {name} for agent "
                                     f"{int(other.agent)}")
        if landscape is not None and cost_landscape is not None:
            if int(landscape.agent) != int(cost_landscape.agent):
                raise ValueError(f"landscape is swept for agent {int(landscape.agent)}, cost_landscape for agent "
                                 f"{int(cost_landscape.agent)}")
            if not (np.array_equal(np.asarray(landscape.xs), np.asarray(cost_landscape.xs))
                    and np.array_equal(np.asarray(landscape.ys), np.asarray(cost_landscape.ys))):
                raise ValueError("landscape and cost_landscape are swept over different grids")
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        from matplotlib.collections import LineCollection, PatchCollection
        from matplotlib.patches import Circle, Polygon

        self.ep, self.n_agent, self.n_goal = ep, n_agent, n_goal
        self.cost_components, self.Ta_is_unsafe = tuple(cost_components), Ta_is_unsafe
        self.fig, ax = plt.subplots(1, 1, figsize=(10, 10), dpi=dpi)
        self.ax = ax
        ax.set_xlim(0.0, side_length)
        ax.set_ylim(0.0, side_length)
        ax.set_aspect("equal")
        ax.axis("off")
        ax.add_patch(plt.Rectangle((0, 0), side_length, side_length, fill=False, edgecolor="0.6", linewidth=1.0, zorder=0))
        if ep.rect_points is not None and len(ep.rect_points):
            ax.add_collection(PatchCollection([Polygon(p, closed=True) for p in ep.rect_points], facecolor=OBS_COLOR,
                                              edgecolor="none", alpha=0.8, zorder=1))
        if ep.discs is not None and len(ep.discs):
            ax.add_collection(PatchCollection([Circle(c, obs_r) for c in ep.discs], facecolor=OBS_COLOR, edgecolor="none",
                                              zorder=1))
        pos0 = ep.states[0, :, :2]
        self.goal_circles = [Circle(pos0[n_agent + j], r, color=GOAL_COLOR, linewidth=0.0, zorder=5) for j in range(n_goal)]
        self.agent_circles = [Circle(pos0[i], r, color=AGENT_COLOR, linewidth=0.0, zorder=6) for i in range(n_agent)]
        for c in self.goal_circles + self.agent_circles:
            ax.add_patch(c)
        self.edges = LineCollection([], linewidths=2, alpha=0.5, zorder=3)
        ax.add_collection(self.edges)
        font = dict(size=16, color="k", transform=ax.transAxes)
        self.cost_text = ax.text(0.02, 1.00, "", va="bottom", **font)
        self.unsafe_text = ax.text(0.99, 1.00, "", va="bottom", ha="right", **font)
        self.step_text = ax.text(0.99, 1.04, "", va="bottom", ha="right", **font)
        self.labels = [ax.text(pos0[i, 0], pos0[i, 1], f"{i}", size=20, color="k", ha="center", va="center", clip_on=True,
                               zorder=7) for i in range(n_agent)]
        self._plt = plt
        # Vh landscape under the agents (dgppo/env/plot.py:348-372): one colour scale for the whole episode, centred at 0.
        # The true cost (trainer.data.CostLandscape) is drawn the same way when it comes alone; next to a Vh landscape it
        # only adds its own zero contour, dashed, so the learned and the true unsafe sets can be compared frame by frame
        self.landscape, self.cost_landscape = landscape, cost_landscape
        self.contours = self.zero_line = self.cost_zero_line = None
        self._cost_h = None
        filled = landscape if landscape is not None else cost_landscape
        if filled is not None:
            if landscape is not None and cost_landscape is not None:
                self._cost_h = np.asarray(cost_landscape.h(), dtype=np.float64)
                self._cost_row = {int(t): k for k, t in enumerate(np.asarray(cost_landscape.frames).reshape(-1))}
            h = np.asarray(filled.h(), dtype=np.float64)
            self._h = h
            self._frame_row = {int(t): k for k, t in enumerate(np.asarray(filled.frames).reshape(-1))}
            if h.shape[1] < 2 or h.shape[2] < 2:
                print(f"(landscape grid {h.shape[2]} x {h.shape[1]}: contours need at least 2 lines each way, none are drawn)")
            self._xy = np.meshgrid(np.asarray(filled.xs, dtype=np.float64), np.asarray(filled.ys, dtype=np.float64))
            self._norm, self._levels = _centred_scale(h)
            sm = plt.cm.ScalarMappable(norm=self._norm, cmap="RdBu_r")
            self.fig.colorbar(sm, ax=ax, fraction=0.046, pad=0.04)
            self.cbf_text = ax.text(0.5, 1.04, f"{'CBF' if landscape is not None else 'Cost'} for {int(filled.agent)}",
                                    va="bottom", ha="center", **font)
        # rollout landscape (trainer.data.RolloutLandscape): the boundary of the set from which the policy becomes unsafe within
        # the horizon — the zero contour of its h(), dotted, over whatever else is drawn
        self.rollout_landscape = rollout_landscape
        self.rollout_zero_line = None
        if rollout_landscape is not None:
            self._ro_h = np.asarray(rollout_landscape.h(), dtype=np.float64)
            self._ro_row = {int(t): k for k, t in enumerate(np.asarray(rollout_landscape.frames).reshape(-1))}
            self._ro_xy = np.meshgrid(np.asarray(rollout_landscape.xs, dtype=np.float64),
                                      np.asarray(rollout_landscape.ys, dtype=np.float64))
            if self._ro_h.shape[1] < 2 or self._ro_h.shape[2] < 2:
                print(f"(rollout landscape grid {self._ro_h.shape[2]} x {self._ro_h.shape[1]}: contours need at least 2 lines each "
                      f"way, none are drawn)")

        # action landscape (trainer.data.ActionLandscape): an inset over the action square, the swept agent's largest cbf_deriv
        # component as filled contours (<= 0: the net admits the action), the zero contour in black, the recorded action marked
        self.action_landscape = action_landscape
        self.act_ax = self.act_contours = self.act_zero_line = self.act_marker = None
        if action_landscape is not None:
            A = action_landscape
            self._act_h = np.asarray(A.h(), dtype=np.float64)
            self._act_row = {int(t): k for k, t in enumerate(np.asarray(A.frames).reshape(-1))}
            self._act_taken = np.asarray(A.actions, dtype=np.float64).reshape(-1, 2)
            us, vs = np.asarray(A.us, dtype=np.float64), np.asarray(A.vs, dtype=np.float64)
            if self._act_h.shape[1] < 2 or self._act_h.shape[2] < 2:
                print(f"(action grid {self._act_h.shape[2]} x {self._act_h.shape[1]}: contours need at least 2 lines each way, "
                      f"none are drawn)")
            self._act_uv = np.meshgrid(us, vs)
            self._act_norm, self._act_levels = _centred_scale(self._act_h)
            self._action_inset(us, vs, f"cbf_deriv of {int(A.agent)} over its action")
        # action rollout landscape (trainer.data.ActionRolloutLandscape): what those actions lead to, measured.  Next to an action
        # landscape it only adds the zero contour of its h(), dashed, to that inset: the boundary of the actions that doom the
        # agent within the horizon.  Alone it gets the inset to itself: filled contours of h(), the zero contour in black, the
        # recorded action marked
        self.action_rollout_landscape = action_rollout_landscape
        self.act_ro_zero_line = None
        if action_rollout_landscape is not None:
            R = action_rollout_landscape
            self._aro_h = np.asarray(R.h(), dtype=np.float64)
            self._aro_row = {int(t): k for k, t in enumerate(np.asarray(R.frames).reshape(-1))}
            us, vs = np.asarray(R.us, dtype=np.float64), np.asarray(R.vs, dtype=np.float64)
            self._aro_uv = np.meshgrid(us, vs)
            if self._aro_h.shape[1] < 2 or self._aro_h.shape[2] < 2:
                print(f"(action rollout grid {self._aro_h.shape[2]} x {self._aro_h.shape[1]}: contours need at least 2 lines each "
                      f"way, none are drawn)")
            if action_landscape is None:
                self._aro_taken = np.asarray(R.actions, dtype=np.float64).reshape(-1, 2)
                self._aro_norm, self._aro_levels = _centred_scale(self._aro_h)
                self._action_inset(us, vs, f"worst cost of {int(R.agent)} within {int(R.horizon)} steps over its action")

    def _action_inset(self, us, vs, title: str):
        """the inset over the action square, with the marker of the recorded action; hidden until a frame is drawn in it"""
        self.act_ax = self.ax.inset_axes([0.76, 0.02, 0.22, 0.22], zorder=8)
        self.act_ax.set_xlim(min(-1.0, float(us.min())), max(1.0, float(us.max())))
        self.act_ax.set_ylim(min(-1.0, float(vs.min())), max(1.0, float(vs.max())))
        self.act_ax.set_aspect("equal")
        self.act_ax.set_xticks([-1, 0, 1])
        self.act_ax.set_yticks([-1, 0, 1])
        self.act_ax.tick_params(labelsize=8)
        self.act_ax.set_title(title, fontsize=9)
        self.act_marker, = self.act_ax.plot([], [], marker="x", color="k", markersize=8, markeredgewidth=2, linestyle="none",
                                            zorder=5)
        self.act_ax.set_visible(False)

    def artists(self):
        extra = [a for a in (self.contours, self.zero_line, self.cost_zero_line, self.rollout_zero_line,
                             getattr(self, "cbf_text", None), self.act_ax) if a is not None]
        return [*self.agent_circles, *self.goal_circles, self.edges, self.cost_text, self.unsafe_text, self.step_text,
                *self.labels, *extra]

    def _draw_landscape(self, t: int):
        """the contours are rebuilt for every frame, as plot.py:437-447 does; a frame the landscape does not cover shows none"""
        for a in (self.contours, self.zero_line, self.cost_zero_line):
            if a is not None:
                a.remove()
        self.contours = self.zero_line = self.cost_zero_line = None
        X, Y = self._xy
        k = self._frame_row.get(int(t))
        if k is not None and _drawable(self._h[k]):
            z = self._h[k]
            self.contours = self.ax.contourf(X, Y, z, levels=self._levels, cmap="RdBu_r", norm=self._norm, alpha=0.5, zorder=2,
                                             extend="both")
            if z.min() < 0.0 <= z.max():             # h >= 0 is unsafe (Landscape.h): a maximum of exactly 0 counts
                self.zero_line = self.ax.contour(X, Y, z, levels=[0.0], colors="k", linewidths=2.0, zorder=4)
        k = self._cost_row.get(int(t)) if self._cost_h is not None else None
        if k is not None and _drawable(self._cost_h[k]):
            z = self._cost_h[k]
            if z.min() < 0.0 <= z.max():             # the true unsafe set's boundary, dashed
                self.cost_zero_line = self.ax.contour(X, Y, z, levels=[0.0], colors="k", linewidths=2.0, linestyles="dashed",
                                                      zorder=4)

    def _draw_rollout_landscape(self, t: int):
        """the dotted zero contour of frame t, rebuilt like the contours above; a frame the rollout landscape does not hold, or
        one whose slice holds a NaN or does not change sign, shows none"""
        if self.rollout_zero_line is not None:
            self.rollout_zero_line.remove()
        self.rollout_zero_line = None
        k = self._ro_row.get(int(t))
        if k is not None and _drawable(self._ro_h[k]):
            z = self._ro_h[k]
            if z.min() < 0.0 <= z.max():             # h >= 0: unsafe within the horizon (RolloutLandscape.h)
                X, Y = self._ro_xy
                self.rollout_zero_line = self.ax.contour(X, Y, z, levels=[0.0], colors="k", linewidths=2.0, linestyles="dotted",
                                                         zorder=4)

    def _draw_action_landscape(self, t: int):
        """the inset of frame t, rebuilt like the contours above; a frame the action landscape does not hold shows no inset"""
        for a in (self.act_contours, self.act_zero_line):
            if a is not None:
                a.remove()
        self.act_contours = self.act_zero_line = None
        k = self._act_row.get(int(t))
        self.act_ax.set_visible(k is not None)
        if k is None:
            return
        U, V = self._act_uv
        z = self._act_h[k]
        if _drawable(z):
            self.act_contours = self.act_ax.contourf(U, V, z, levels=self._act_levels, cmap="RdBu_r", norm=self._act_norm,
                                                     extend="both")
            if z.min() <= 0.0 < z.max():             # cbf_deriv <= 0 is admitted: the boundary exists where the sign changes
                self.act_zero_line = self.act_ax.contour(U, V, z, levels=[0.0], colors="k", linewidths=1.5)
        self.act_marker.set_data([self._act_taken[k, 0]], [self._act_taken[k, 1]])

    def _draw_action_rollout_landscape(self, t: int):
        """frame t of the action rollout landscape: the dashed zero contour in the action landscape's inset, or — alone — the
        inset itself, rebuilt like the contours above; a frame it does not hold adds nothing (alone: shows no inset)"""
        alone = self.action_landscape is None
        for a in (self.act_ro_zero_line, *((self.act_contours,) if alone else ())):
            if a is not None:
                a.remove()
        self.act_ro_zero_line = None
        k = self._aro_row.get(int(t))
        if alone:
            self.act_contours = None
            self.act_ax.set_visible(k is not None)
        if k is None:
            return
        U, V = self._aro_uv
        z = self._aro_h[k]
        if _drawable(z):
            if alone:
                self.act_contours = self.act_ax.contourf(U, V, z, levels=self._aro_levels, cmap="RdBu_r", norm=self._aro_norm,
                                                         extend="both")
            if z.min() < 0.0 <= z.max():             # h >= 0: the action dooms the agent within the horizon
                self.act_ro_zero_line = self.act_ax.contour(U, V, z, levels=[0.0], colors="k", linewidths=1.5,
                                                            linestyles="solid" if alone else "dashed")
        if alone:
            self.act_marker.set_data([self._aro_taken[k, 0]], [self._aro_taken[k, 1]])

    def draw(self, t: int):
        ep, n = self.ep, self.n_agent
        if self.landscape is not None or self.cost_landscape is not None:
            self._draw_landscape(t)
        if self.rollout_landscape is not None:
            self._draw_rollout_landscape(t)
        if self.action_landscape is not None:
            self._draw_action_landscape(t)
        if self.action_rollout_landscape is not None:
            self._draw_action_rollout_landscape(t)
        pos = ep.states[t, :, :2]
        for i, c in enumerate(self.agent_circles):
            c.set_center(tuple(pos[i]))
            self.labels[i].set_position(tuple(pos[i]))
        for j, c in enumerate(self.goal_circles):
            c.set_center(tuple(pos[n + j]))
        seg, from_goal = frame_edges(ep, t, n, self.n_goal)
        self.edges.set_segments(list(seg))
        self.edges.set_colors([GOAL_COLOR if g else COMM_COLOR for g in from_goal])
        worst = ep.costs[t].max(axis=0)                        # per component: the worst agent (plot.py cost text)
        lines = [f"{name}: {worst[k]:8.3f}" for k, name in enumerate(self.cost_components[:len(worst)])]
        self.cost_text.set_text("Cost:\n  " + "\n  ".join(lines) + f"\nReward: {ep.rewards[t]:.3f}")
        self.unsafe_text.set_text("Unsafe: {}".format(unsafe_agents(ep, t, self.Ta_is_unsafe).tolist()))
        self.step_text.set_text(f"kk={t:04}")
        return self.artists()

    def close(self):
        self._plt.close(self.fig)


def _write(scene: _Scene, n_frames: int, video_path: pathlib.Path, fps: int = 33) -> pathlib.Path:
    from matplotlib import animation
    video_path = pathlib.Path(video_path)
    video_path.parent.mkdir(parents=True, exist_ok=True)
    anim = animation.FuncAnimation(scene.fig, scene.draw, frames=n_frames, init_func=scene.artists, interval=1000 // fps,
                                   blit=False)
    out, writer = video_path, None
    if video_path.suffix.lower() == ".gif":
        writer = animation.PillowWriter(fps=fps)
    elif not animation.writers.is_available("ffmpeg"):
        out = video_path.with_suffix(".gif")
        writer = animation.PillowWriter(fps=fps)
        print(f"(no ffmpeg binary: writing {out.name} instead of {video_path.name})")
    else:
        writer = animation.FFMpegWriter(fps=fps)
    anim.save(str(out), writer=writer)
    scene.close()
    return out


def _render(rollout, video_path, side_length, dim, n_agent, r, obs_r, cost_components, Ta_is_unsafe, viz_opts, dpi, n_goal,
            index=None, max_frames=None, landscape=None, cost_landscape=None, action_landscape=None, rollout_landscape=None,
            action_rollout_landscape=None, **kwargs) -> pathlib.Path:
    if dim != 2:
        raise NotImplementedError("only the planar environments of SURVEY §8 are rendered (dim == 2)")
    if viz_opts:
        raise NotImplementedError(f"viz_opts {sorted(viz_opts)}: CBF / Vh overlays are not built")
    ep = episode_from_rollout(rollout, index)
    n_goal = n_agent if n_goal is None else n_goal
    scene = _Scene(ep, float(side_length), n_agent, n_goal, r, obs_r, cost_components, Ta_is_unsafe, dpi, landscape,
                   cost_landscape, action_landscape, rollout_landscape, action_rollout_landscape)
    T = ep.states.shape[0] if max_frames is None else min(ep.states.shape[0], max_frames)
    return _write(scene, T, video_path)


def render_lidar(rollout, video_path, side_length: float, dim: int, n_agent: int, n_rays: int, r: float,
                 cost_components: Tuple[str, ...], Ta_is_unsafe=None, viz_opts: Optional[dict] = None, dpi: int = 100,
                 n_goal: Optional[int] = None, landscape=None, cost_landscape=None, action_landscape=None,
                 rollout_landscape=None, action_rollout_landscape=None, **kwargs) -> pathlib.Path:
    """dgppo/env/plot.py:468 (LiDAR family: rectangle obstacles, `n_rays` hit nodes per agent).  landscape: a
    trainer.data.Landscape of this episode, drawn as the reference draws viz_opts["cbf"] (plot.py:348-372,437-447).
    cost_landscape: a trainer.data.CostLandscape, drawn the same way when alone ("Cost for k"), as a dashed zero contour over
    the Vh contours when both are given.  action_landscape: a trainer.data.ActionLandscape, drawn in an inset over the action
    square (filled contours of the swept agent's cbf_deriv, black zero contour, the recorded action marked); it combines with
    the other two, for the same agent.  rollout_landscape: a trainer.data.RolloutLandscape: the zero contour of its h() — the
    boundary of the set from which the policy becomes unsafe within the horizon — dotted, over whatever else is drawn, for the
    same agent and grid.  action_rollout_landscape: a trainer.data.ActionRolloutLandscape: next to an action_landscape of the same
    agent and the same us / vs, the zero contour of its h() — the boundary of the actions that doom the agent within the horizon
    — dashed inside that inset; alone, an inset of its own with h() as filled contours and the action taken marked."""
    return _render(rollout, video_path, side_length, dim, n_agent, r, 0.0, cost_components, Ta_is_unsafe, viz_opts, dpi,
                   n_goal, landscape=landscape, cost_landscape=cost_landscape, action_landscape=action_landscape,
                   rollout_landscape=rollout_landscape, action_rollout_landscape=action_rollout_landscape, **kwargs)


def render_mpe(rollout, video_path, side_length: float, dim: int, n_agent: int, n_obs: int, r: float, obs_r: float,
               cost_components: Tuple[str, ...], Ta_is_unsafe=None, viz_opts: Optional[dict] = None, dpi: int = 100,
               n_goal: Optional[int] = None, landscape=None, cost_landscape=None, action_landscape=None,
               rollout_landscape=None, action_rollout_landscape=None, **kwargs) -> pathlib.Path:
    """dgppo/env/plot.py:206 (MPE family: disc obstacles of radius obs_r).  landscape / cost_landscape / action_landscape /
    rollout_landscape / action_rollout_landscape: as in render_lidar."""
    return _render(rollout, video_path, side_length, dim, n_agent, r, obs_r, cost_components, Ta_is_unsafe, viz_opts, dpi,
                   n_goal, landscape=landscape, cost_landscape=cost_landscape, action_landscape=action_landscape,
                   rollout_landscape=rollout_landscape, action_rollout_landscape=action_rollout_landscape, **kwargs)
