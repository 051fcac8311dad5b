"""Evaluation statistics of the reference's test.py (test.py:103-141): per-episode reward / cost / safe rate and the
aggregate safe-rate mean and standard deviation.  Host reductions on the arrays a test rollout returns.

`unsafe_mask` follows test.py:103-105 — `any(env.get_cost(graph) >= 0, axis=-1)` on the T pre-step graphs of a rollout —
and `Rollout.costs[t]` IS `get_cost(graph[t])` (cost is evaluated on the pre-step graph, lidar_env/base.py:170-171), so the
mask is taken from the stored costs instead of re-deriving the graphs."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List

import numpy as np
import yaml


def unsafe_mask(costs: np.ndarray) -> np.ndarray:
    """costs [..., n_agents, n_cost] -> bool [..., n_agents]  (test.py:103-105)."""
    return np.any(np.asarray(costs) >= 0.0, axis=-1)


def episode_stats(rewards: np.ndarray, costs: np.ndarray) -> Dict[str, np.ndarray]:
    """rewards [E, T], costs [E, T, n, nh] -> per-episode reward sum, cost max, safe rate (test.py:118-127) and the
    per-(episode, agent) unsafe flag `max_t is_unsafe` used by the aggregate (test.py:131)."""
    rewards, costs = np.asarray(rewards), np.asarray(costs)
    is_unsafe = unsafe_mask(costs)                               # [E, T, n]
    ever_unsafe = is_unsafe.max(axis=1)                          # [E, n]
    return {
        "reward": rewards.sum(axis=1),
        "cost": costs.reshape(costs.shape[0], -1).max(axis=1),
        "safe_rate": 1.0 - ever_unsafe.mean(axis=1),
        "ever_unsafe": ever_unsafe,
    }


def aggregate(stats: Dict[str, np.ndarray]) -> Dict[str, float]:
    """test.py:131-138: safe mean / std over all (episode, agent) pairs, reward and cost mean / min / max."""
    safe = 1.0 - stats["ever_unsafe"].astype(np.float64)
    r, c = stats["reward"], stats["cost"]
    return {"reward": float(r.mean()), "reward_min": float(r.min()), "reward_max": float(r.max()),
            "cost": float(c.mean()), "cost_min": float(c.min()), "cost_max": float(c.max()),
            "safe_mean": float(safe.mean()), "safe_std": float(safe.std())}


def csv_line(env, epi: int, agg: Dict[str, float]) -> str:
    """the row test.py:142-146 appends to test_log.csv"""
    return (f"{env.num_agents},{epi},{env.max_episode_steps},{env.area_size},{env.params['n_obs']},"
            f"{agg['safe_mean'] * 100:.3f},{agg['safe_std'] * 100:.3f}\n")


# ---- config.yaml --------------------------------------------------------------------------------------------------
class _ConfigLoader(yaml.SafeLoader):
    """SafeLoader that also understands the one python tag the reference's train.py writes (`yaml.dump(args)` of an
    argparse.Namespace, train.py:119-121) by reading it as a plain mapping.  Nothing from the file is executed."""


_ConfigLoader.add_constructor("tag:yaml.org,2002:python/object:argparse.Namespace",
                              lambda loader, node: loader.construct_mapping(node, deep=True))


def load_config(path: str) -> SimpleNamespace:
    """{log_dir}/config.yaml -> attribute access like the reference's `config.env`, `config.num_agents`, ...
    (test.py:36-38 uses yaml.UnsafeLoader; this loader refuses every other python tag)."""
    with open(path, "r") as f:
        data = yaml.load(f, Loader=_ConfigLoader)
    if not isinstance(data, dict):
        raise ValueError(f"{path}: expected a mapping, got {type(data).__name__}")
    return SimpleNamespace(**data)


def latest_step(model_path: str) -> int:
    """test.py:53-55: the largest all-digit directory name under models/"""
    import os
    steps: List[int] = [int(m) for m in os.listdir(model_path) if m.isdigit()]
    if not steps:
        raise FileNotFoundError(f"no checkpoints under {model_path}")
    return max(steps)


def landscape_agreement(land, cost) -> Dict[str, np.ndarray]:
    """How the learned landscape (trainer.data.Landscape) agrees with the true one (CostLandscape) of the same agent, grid
    and frames.  Vh >= h should hold, so the unsafe set of the net should cover the true one.  Per frame [F], over the points
    where both h() are finite: `points`, `unsafe` (true h >= 0), `missed` (true h >= 0 where the net says h < 0: a truly
    unsafe point called safe), `conservative` (true h < 0 where the net says h >= 0); `nan` counts the other points.
    missed_frac = missed.sum() / max(unsafe.sum(), 1), conservative_frac likewise over the truly safe points."""
    same = (int(land.agent) == int(cost.agent)
            and np.array_equal(np.asarray(land.xs), np.asarray(cost.xs)) and np.array_equal(np.asarray(land.ys), np.asarray(cost.ys))
            and np.array_equal(np.asarray(land.frames).reshape(-1), np.asarray(cost.frames).reshape(-1)))
    if not same:
        raise ValueError("landscape_agreement: the two landscapes differ in xs, ys, agent or frames")
    hv, hc = np.asarray(land.h()), np.asarray(cost.h())
    ok = np.isfinite(hv) & np.isfinite(hc)
    count = lambda m: (m & ok).sum(axis=(1, 2)).astype(np.int64)
    points, unsafe = count(ok), count(hc >= 0.0)
    missed, conservative = count((hc >= 0.0) & (hv < 0.0)), count((hc < 0.0) & (hv >= 0.0))
    safe = points - unsafe
    return dict(points=points, unsafe=unsafe, missed=missed, conservative=conservative, nan=(~ok).sum(axis=(1, 2)).astype(np.int64),
                missed_frac=float(missed.sum() / max(int(unsafe.sum()), 1)),
                conservative_frac=float(conservative.sum() / max(int(safe.sum()), 1)))


def rollout_agreement(rl, land=None, cost=None) -> Dict[str, np.ndarray]:
    """How a RolloutLandscape (trainer.data) — the set of positions from which the policy becomes unsafe within the horizon —
    compares with the learned Landscape and the instantaneous CostLandscape of the same agent, grid and frames.  A point is
    `doomed` where rl.h() >= 0.  Per frame [F], each count over the points where its operands' h() are finite:
    always `points`, `doomed` and doomed_frac = doomed.sum() / max(points.sum(), 1);
    with `land`: `missed` (doomed where the net says h < 0: what a barrier exists to rule out), `conservative` (not doomed
    within the horizon where the net says h >= 0), missed_frac = missed.sum() / max(the doomed points counted, 1),
    conservative_frac likewise over the points not doomed, and value_error = the mean |Vh - value| over the finite entries of
    the swept agent's row;
    with `cost`: `latent` (safe now, cost h < 0, but doomed: the failures cost_landscape cannot show) and latent_frac =
    latent.sum() / max(the currently safe points counted, 1)."""
    for name, other in (("land", land), ("cost", cost)):
        if other is None:
            continue
        same = (int(rl.agent) == int(other.agent)
                and np.array_equal(np.asarray(rl.xs), np.asarray(other.xs)) and np.array_equal(np.asarray(rl.ys), np.asarray(other.ys))
                and np.array_equal(np.asarray(rl.frames).reshape(-1), np.asarray(other.frames).reshape(-1)))
        if not same:
            raise ValueError(f"rollout_agreement: rl and {name} differ in xs, ys, agent or frames")
    hr = np.asarray(rl.h())
    fin = np.isfinite(hr)
    count = lambda m: m.sum(axis=(1, 2)).astype(np.int64)
    points, doomed = count(fin), count(fin & (hr >= 0.0))
    out = dict(points=points, doomed=doomed, doomed_frac=float(doomed.sum() / max(int(points.sum()), 1)))
    if land is not None:
        hv = np.asarray(land.h())
        ok = fin & np.isfinite(hv)
        missed, conservative = count(ok & (hr >= 0.0) & (hv < 0.0)), count(ok & (hr < 0.0) & (hv >= 0.0))
        n_doomed, n_free = int(count(ok & (hr >= 0.0)).sum()), int(count(ok & (hr < 0.0)).sum())
        a = int(rl.agent)
        d = np.abs(np.asarray(land.Vh, dtype=np.float64)[:, :, :, a] - np.asarray(rl.value, dtype=np.float64)[:, :, :, a])
        d = d[np.isfinite(d)]
        out.update(missed=missed, conservative=conservative, missed_frac=float(missed.sum() / max(n_doomed, 1)),
                   conservative_frac=float(conservative.sum() / max(n_free, 1)),
                   value_error=float(d.mean()) if d.size else float("nan"))
    if cost is not None:
        hc = np.asarray(cost.h())
        ok = fin & np.isfinite(hc)
        latent = count(ok & (hc < 0.0) & (hr >= 0.0))
        out.update(latent=latent, latent_frac=float(latent.sum() / max(int(count(ok & (hc < 0.0)).sum()), 1)))
    return out


def action_admissibility(A) -> Dict[str, np.ndarray]:
    """What the learned barrier admits in an action landscape (trainer.data.ActionLandscape): a grid action is admitted where
    A.h() <= 0, i.e. every component of the swept agent's cbf_deriv is <= 0; a NaN is not admitted.  Per frame [F]: `points`
    (nv * nu), `admitted`, and `taken` — whether the action the agent actually took is admitted, decided from the record's own
    values and not from the nearest grid point: cbf_deriv = (Vh[t + 1] - Vh[t]) / dt + alpha * Vh[t] with both values out of
    A.Vh, so it is known (1 / 0) where A.frames also holds t + 1 and -1 elsewhere (always for the last frame of an episode,
    whose successor values_prepass evaluates but the landscape does not keep).  `empty_frames`: the frame numbers with no
    admitted action.  admissible_frac = admitted.sum() / points.sum(), empty_frac = len(empty_frames) / F,
    taken_admitted_frac = (taken == 1).sum() / max((taken >= 0).sum(), 1)."""
    h = np.asarray(A.h())
    F = h.shape[0]
    frames = np.asarray(A.frames).reshape(-1).astype(np.int64)
    if frames.size != F:
        raise ValueError(f"action_admissibility: {frames.size} frame numbers for {F} frames")
    admitted = (h <= 0.0).sum(axis=(1, 2)).astype(np.int64)          # a NaN compares false
    points = np.full(F, h.shape[1] * h.shape[2], dtype=np.int64)
    Vh = np.asarray(A.Vh)[:, int(A.agent)]                            # [F, n_cost]
    row = {int(t): k for k, t in enumerate(frames)}
    taken = np.full(F, -1, dtype=np.int64)
    for k, t in enumerate(frames):
        nxt = row.get(int(t) + 1)
        if nxt is not None:
            cbf = (Vh[nxt] - Vh[k]) / np.float32(A.dt) + np.float32(A.alpha) * Vh[k]
            taken[k] = int(bool((cbf <= 0.0).all()))
    empty = frames[admitted == 0]
    return dict(points=points, admitted=admitted, taken=taken, empty_frames=empty,
                admissible_frac=float(admitted.sum() / max(int(points.sum()), 1)), empty_frac=float(empty.size / max(F, 1)),
                taken_admitted_frac=float((taken == 1).sum() / max(int((taken >= 0).sum()), 1)))


def action_rollout_agreement(R, A=None) -> Dict[str, np.ndarray]:
    """What a single action decides, measured (trainer.data.ActionRolloutLandscape R), and how the learned barrier's verdict
    on the same actions (ActionLandscape A of the same agent, us, vs and frames) compares.  A point is `doomed` where
    R.h() >= 0 (rollout_agreement's convention).  Per frame [F], over the finite entries of R.h(): `points`, `doomed`;
    doomed_frac = doomed.sum() / max(points.sum(), 1); `empty_frames` — the frame numbers in which every finite point is
    doomed (frames without a finite point are not among them) — and empty_frac = len(empty_frames) / F; decisive_frac — the
    share of frames whose grid holds doomed and not-doomed points alike, so that the one action decides.
    For n > 1: others_doomed_frac and others_decisive_frac, the same two notions on R.h_others().
    With A: `missed` (admitted by the barrier, A.h() <= 0, but doomed: a false admit of the filter the barrier shield relies
    on), `conservative` (rejected but not doomed), both [F] and counted where both h() are finite; missed_frac = missed.sum()
    / max(the doomed points counted, 1), conservative_frac likewise over the points not doomed."""
    if A is not None:
        same = (int(R.agent) == int(A.agent)
                and np.array_equal(np.asarray(R.us), np.asarray(A.us)) and np.array_equal(np.asarray(R.vs), np.asarray(A.vs))
                and np.array_equal(np.asarray(R.frames).reshape(-1), np.asarray(A.frames).reshape(-1)))
        if not same:
            raise ValueError("action_rollout_agreement: R and A differ in us, vs, agent or frames")
    count = lambda m: m.sum(axis=(1, 2)).astype(np.int64)

    def verdict(h):
        fin = np.isfinite(h)
        points, doomed = count(fin), count(fin & (h >= 0.0))
        return fin, points, doomed

    hr = np.asarray(R.h())
    F = hr.shape[0]
    frames = np.asarray(R.frames).reshape(-1).astype(np.int64)
    if frames.size != F:
        raise ValueError(f"action_rollout_agreement: {frames.size} frame numbers for {F} frames")
    fin, points, doomed = verdict(hr)
    empty = frames[(points > 0) & (doomed == points)]
    decisive = (doomed > 0) & (doomed < points)
    out = dict(points=points, doomed=doomed, doomed_frac=float(doomed.sum() / max(int(points.sum()), 1)), empty_frames=empty,
               empty_frac=float(empty.size / max(F, 1)), decisive_frac=float(decisive.sum() / max(F, 1)))
    if np.asarray(R.worst).shape[3] > 1:
        _, po, do = verdict(np.asarray(R.h_others()))
        out.update(others_doomed_frac=float(do.sum() / max(int(po.sum()), 1)),
                   others_decisive_frac=float(((do > 0) & (do < po)).sum() / max(F, 1)))
    if A is not None:
        ha = np.asarray(A.h())
        ok = fin & np.isfinite(ha)
        missed, conservative = count(ok & (ha <= 0.0) & (hr >= 0.0)), count(ok & (ha > 0.0) & (hr < 0.0))
        n_doomed, n_free = int(count(ok & (hr >= 0.0)).sum()), int(count(ok & (hr < 0.0)).sum())
        out.update(missed=missed, conservative=conservative, missed_frac=float(missed.sum() / max(n_doomed, 1)),
                   conservative_frac=float(conservative.sum() / max(n_free, 1)))
    return out


def shield_stats(log) -> Dict[str, np.ndarray]:
    """What the barrier shield did per episode (trainer.data.ShieldLog, arrays [B, T, n, ...]), each [B]:
    `intervention_frac` — the share of (step, agent) pairs whose action was replaced (flag != 0), `infeasible_frac` — the share
    in which the barrier admitted no candidate (flag == 2), `mean_deviation` — the mean over (step, agent) of the Euclidean
    distance |a_shield - a_pol| between the executed action and the policy's, both clipped as the environment clips them."""
    flag = np.asarray(log.flag)
    if flag.ndim != 3:
        raise ValueError(f"shield_stats: flag must be [B, T, n], got shape {flag.shape}")
    a, p = np.asarray(log.action, dtype=np.float64), np.asarray(log.policy_action, dtype=np.float64)
    if a.shape != flag.shape + (2,) or p.shape != a.shape:
        raise ValueError(f"shield_stats: action {a.shape} / policy_action {p.shape} do not fit flag {flag.shape}")
    B = flag.shape[0]
    dev = np.sqrt(((np.clip(a, -1.0, 1.0) - np.clip(p, -1.0, 1.0)) ** 2).sum(axis=-1))
    return dict(intervention_frac=(flag != 0).reshape(B, -1).mean(axis=1), infeasible_frac=(flag == 2).reshape(B, -1).mean(axis=1),
                mean_deviation=dev.reshape(B, -1).mean(axis=1))


def joint_shield_stats(log) -> Dict[str, np.ndarray]:
    """What the rounds of the lookahead shield reached per episode (trainer.data.JointLookaheadShieldLog, joint / rounds_used
    [B, T]), each [B]: `joint_verified_frac` — the share of steps whose played joint action was rolled and found admissible for
    every agent (joint == 2), `joint_unrolled_frac` — the share whose played joint action was not rolled (joint == 0: the
    rounds ran out), `mean_rounds` — the mean number of rounds per step."""
    joint, used = np.asarray(log.joint), np.asarray(log.rounds_used)
    if joint.ndim != 2 or used.shape != joint.shape:
        raise ValueError(f"joint_shield_stats: joint {joint.shape} / rounds_used {used.shape} must both be [B, T]")
    return dict(joint_verified_frac=(joint == 2).mean(axis=1), joint_unrolled_frac=(joint == 0).mean(axis=1),
                mean_rounds=used.astype(np.float64).mean(axis=1))
