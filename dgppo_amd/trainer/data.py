"""The rollout record handed between `algo.collect`, `algo.update` and the trainer.  Field names and order are API: they
are the reference's (dgppo/trainer/data.py:8-16).  `graph` / `next_graph` are lazy views here — the engine stores compact
records and materialises GraphsTuples with a HIP kernel only when someone reads them."""
from __future__ import annotations

import collections
from typing import NamedTuple

import numpy as np

_FIELDS = ("graph", "actions", "rnn_states", "rewards", "costs", "dones", "log_pis", "next_graph")


class Rollout(collections.namedtuple("Rollout", _FIELDS)):
    """[B, T, ...] arrays; `log_pis` may be None (deterministic rollouts)."""
    __slots__ = ()

    def _dim(self, field: str, axis: int) -> int:
        return int(getattr(self, field).shape[axis])

    # the four size helpers of the reference (data.py:18-32)
    length = property(lambda self: self._dim("rewards", 0), doc="number of environments B")
    time_horizon = property(lambda self: self._dim("rewards", 1), doc="steps per environment T")
    num_agents = property(lambda self: self._dim("costs", 2), doc="agents per environment")
    n_data = property(lambda self: self._dim("rewards", 0) * self._dim("rewards", 1), doc="B * T")


class Landscape(NamedTuple):
    """The constraint-value function of one agent swept over a grid of positions in frozen frames of an episode
    (`DGPPO.vh_landscape`): what the reference's renderer draws as the "CBF" contours (dgppo/env/plot.py:348-372)."""
    xs: np.ndarray        # [nx] fp32 grid lines
    ys: np.ndarray        # [ny]
    Vh: np.ndarray        # [F, ny, nx, n, n_cost]: Vh of every agent with `agent` standing at (xs[ix], ys[iy]) in frame frames[f]
    agent: int            # the swept agent
    frames: np.ndarray    # [F] frame numbers of the episode

    def h(self) -> np.ndarray:
        """[F, ny, nx]: the swept agent's largest Vh component.  >= 0 exactly where the net calls that agent unsafe — the rule
        test.py applies to the costs (any component >= 0)."""
        return np.asarray(self.Vh)[:, :, :, int(self.agent), :].max(axis=-1)


class CostLandscape(NamedTuple):
    """The environment's own cost of one agent swept over a grid of positions in frozen frames of an episode
    (`DGPPO.cost_landscape`): the ground truth the learned `Landscape` is supposed to bound, at the same swept positions."""
    xs: np.ndarray        # [nx] fp32 grid lines
    ys: np.ndarray        # [ny]
    cost: np.ndarray      # [F, ny, nx, n, n_cost]: get_cost of every agent with `agent` standing at (xs[ix], ys[iy]) in frame frames[f]
    agent: int            # the swept agent
    frames: np.ndarray    # [F] frame numbers of the episode

    def h(self) -> np.ndarray:
        """[F, ny, nx]: the swept agent's largest cost component.  >= 0 exactly where test.py's unsafe rule fires for that
        agent (any component >= 0)."""
        return np.asarray(self.cost)[:, :, :, int(self.agent), :].max(axis=-1)


class RolloutLandscape(NamedTuple):
    """What Vh is trained to predict, measured: from every grid point the policy is rolled `horizon` steps forward
    (`DGPPO.rollout_landscape`) and the costs it meets are folded as the training target folds them (compute_dec_ocp_gae,
    dgppo/algo/utils.py:38-45, at gae_lambda = 1 and started from the last cost instead of a learned tail)."""
    xs: np.ndarray        # [nx] fp32 grid lines
    ys: np.ndarray        # [ny]
    value: np.ndarray     # [F, ny, nx, n, n_cost]: the discounted-to-max constraint return of the horizon from (xs[ix], ys[iy])
    worst: np.ndarray     # [F, ny, nx, n, n_cost]: the largest cost met within the horizon
    agent: int            # the swept agent
    frames: np.ndarray    # [F] frame numbers of the episode
    horizon: int          # steps rolled from every grid point
    gamma: float

    def h(self) -> np.ndarray:
        """[F, ny, nx]: the swept agent's largest `worst` component.  >= 0 exactly where that agent becomes unsafe, by the rule
        test.py applies to the costs (any component >= 0), within the horizon."""
        return np.asarray(self.worst)[:, :, :, int(self.agent), :].max(axis=-1)

    def v(self) -> np.ndarray:
        """[F, ny, nx]: the swept agent's largest `value` component: what Landscape.h() is supposed to equal."""
        return np.asarray(self.value)[:, :, :, int(self.agent), :].max(axis=-1)


class ShieldLog(NamedTuple):
    """What the barrier shield did in the episodes of `DGPPO.collect_shielded`, env-major like the Rollout next to it.  The
    candidates of an agent are its policy action (index 0) and the grid points (us[iu], vs[iv]) (index 1 + iv * nu + iu);
    h = max_c ((Vh_next - Vh) / dt + alpha * Vh) on the agent's own row, admissible where h <= -margin."""
    policy_action: np.ndarray   # [B, T, n, 2]: what the policy wanted
    action: np.ndarray          # [B, T, n, 2]: what was executed (the Rollout's actions)
    index: np.ndarray           # [B, T, n] int32: the candidate executed
    flag: np.ndarray            # [B, T, n] int32: 0 kept, 1 replaced by an admissible candidate, 2 nothing admissible
    h: np.ndarray               # [B, T, n, P]: the barrier value of every candidate, P = 1 + nv * nu
    Vh: np.ndarray              # [B, T, n, n_cost]: Vh of the graph of step t
    us: np.ndarray              # [nu] fp32 grid lines of the first action component
    vs: np.ndarray              # [nv] of the second
    margin: float
    alpha: float
    dt: float


class LookaheadShieldLog(NamedTuple):
    """What the lookahead shield did in the episodes of `collect_lookahead_shielded`, env-major like the Rollout next to it.
    The candidates are numbered as in ShieldLog; s is the worst cost the agent itself meets in the `horizon` states after
    playing the candidate, everyone else and every later step following the policy; admissible where s <= -margin."""
    policy_action: np.ndarray   # [B, T, n, 2]: what the policy wanted
    action: np.ndarray          # [B, T, n, 2]: what was executed (the Rollout's actions)
    index: np.ndarray           # [B, T, n] int32: the candidate executed
    flag: np.ndarray            # [B, T, n] int32: 0 kept, 1 replaced by an admissible candidate, 2 nothing admissible
    s: np.ndarray               # [B, T, n, P]: the worst rolled cost of every candidate, P = 1 + nv * nu
    us: np.ndarray              # [nu] fp32 grid lines of the first action component
    vs: np.ndarray              # [nv] of the second
    margin: float
    horizon: int


class JointLookaheadShieldLog(NamedTuple):
    """LookaheadShieldLog of `collect_lookahead_shielded(rounds >= 2)`: the picks were re-judged in rounds that roll the joint
    action held (Engine.lookahead_select_rounds).  index is the grid number of the action held (0: the policy's), flag describes
    that action (0 the policy's and admissible, 1 replaced and admissible, 2 not admissible), s is the fold of the step's last
    round: candidate 0 there is the action the agent held in that round, everyone else playing the joint action held."""
    policy_action: np.ndarray   # [B, T, n, 2]
    action: np.ndarray          # [B, T, n, 2]
    index: np.ndarray           # [B, T, n] int32
    flag: np.ndarray            # [B, T, n] int32
    s: np.ndarray               # [B, T, n, P]
    us: np.ndarray              # [nu]
    vs: np.ndarray              # [nv]
    margin: float
    horizon: int
    joint: np.ndarray           # [B, T] int32: 2 the joint action played was rolled and is admissible for every agent, 1 rolled
                                # and not admissible for some agent, 0 NOT rolled (an agent moved in the step's last round)
    rounds_used: np.ndarray     # [B, T] int32: the rounds that judged the step, 1 .. rounds
    rounds: int                 # the cap


class ActionLandscape(NamedTuple):
    """The discrete control barrier condition of DGPPO (dgppo/algo/dgppo.py:246-250) with one agent's action swept over a grid
    in frames of an episode (`DGPPO.action_landscape`): cbf = (Vh_next - Vh) / dt + alpha * Vh, where Vh_next is the learned
    constraint value of the state one step ahead had `agent` taken (us[iu], vs[iv]) and everyone else their recorded action."""
    us: np.ndarray        # [nu] fp32 grid lines of the first action component
    vs: np.ndarray        # [nv] of the second
    cbf: np.ndarray       # [F, nv, nu, n, n_cost]: cbf_deriv of every agent (a neighbour's value moves too)
    Vh_next: np.ndarray   # [F, nv, nu, n, n_cost]: Vh of the graph after the step
    Vh: np.ndarray        # [F, n, n_cost]: Vh of the recorded graph of frame frames[f]
    actions: np.ndarray   # [F, 2]: the recorded action of `agent` in frame frames[f], clipped as the environment clips it
    agent: int            # the agent whose action is swept
    frames: np.ndarray    # [F] frame numbers of the episode
    alpha: float
    dt: float

    def h(self) -> np.ndarray:
        """[F, nv, nu]: the swept agent's largest cbf component.  <= 0 exactly where the net admits the action (every
        component of cbf_deriv <= 0)."""
        return np.asarray(self.cbf)[:, :, :, int(self.agent), :].max(axis=-1)


class ActionRolloutLandscape(NamedTuple):
    """What the actions an ActionLandscape judges by the learned barrier lead to, measured (`DGPPO.action_rollout_landscape`):
    in frames of an episode `agent` plays (us[iu], vs[iv]) for ONE step, everyone else their recorded action, and the
    deterministic policy is rolled on until the costs of the `horizon` states after that step are known; they are folded as
    RolloutLandscape folds them."""
    us: np.ndarray        # [nu] fp32 grid lines of the first action component
    vs: np.ndarray        # [nv] of the second
    value: np.ndarray     # [F, nv, nu, n, n_cost]: the discounted-to-max constraint return of the horizon, every agent's row
    worst: np.ndarray     # [F, nv, nu, n, n_cost]: the largest cost met within the horizon
    actions: np.ndarray   # [F, 2]: the recorded action of `agent` in frame frames[f], clipped as the environment clips it
    agent: int            # the agent whose action is swept
    frames: np.ndarray    # [F] frame numbers of the episode
    horizon: int          # states after the forced step whose costs are folded
    gamma: float

    def h(self) -> np.ndarray:
        """[F, nv, nu]: the swept agent's largest `worst` component (a NaN propagates): what the lookahead shield calls s.
        >= 0 exactly where the action dooms the agent itself within the horizon."""
        return np.asarray(self.worst)[:, :, :, int(self.agent), :].max(axis=-1)

    def h_others(self) -> np.ndarray:
        """[F, nv, nu]: the same over the rows of all OTHER agents (a NaN propagates): what this agent's single action does
        to its neighbours.  All NaN for a team of one."""
        w = np.asarray(self.worst)
        rest = np.delete(w, int(self.agent), axis=3)
        if rest.shape[3] == 0:
            return np.full(w.shape[:3], np.nan, dtype=w.dtype)
        return rest.max(axis=(3, 4))
