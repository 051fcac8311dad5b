"""Rollouts of the engine on the configurations that have an act-step instance (INSTANCES of tests/test_act_step_gpu.py: the
wave-per-env kernel, and with fused_step the one launch per step that training and bench.py run), every stored quantity
re-derived step by step by the oracle policy and the oracle env — with the one launch and with the four, eager and as the replay
of the captured HIP graph, and again after optimiser steps have moved the parameters under the prepared weights and the captured
graph.  Bars as in tests/test_engine_gpu.py: 1e-5 for actions, log-probabilities and carries, exact env outputs (the
bicycle's dynamics within 1e-6, then exact sensing of the device's own state)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import env_np as E
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_act_step_gpu import INSTANCES  # noqa: E402
from test_engine_gpu import _check_rollout_stepwise, _np_rollout, _setup  # noqa: E402

pytestmark = pytest.mark.gpu
B, T_, BS, RS = 6, 8, 16, 4                      # three minibatches of two envs, chunks of four steps
TOL = 1e-5                                       # the action bar of _check_rollout_stepwise


def _seeds(dev):
    return torch.arange(1, B + 1, dtype=torch.int64, device=dev) * 104729


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "four-launches"])
@pytest.mark.parametrize("kind,n,n_obs", INSTANCES)
def test_wave_instance_rollout_matches_oracle_stepwise(cuda, kind, n, n_obs, fused, graphs):
    """stochastic + deterministic rollouts on every act-step instance; with HIP graphs the checked rollout is the replay"""
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, B, T_, cuda, BS, RS, fused_step=fused, use_graphs=graphs)
    assert eng.fused_step == fused and eng.use_graphs == graphs
    seeds = _seeds(cuda)
    for stochastic in (True, False):
        if graphs:                                # first call: eager launches and the capture
            eng.rollout(seeds + 17, stochastic, noise_seed=4)
            assert eng._ro_cache[(B, stochastic)]["graph"] is not None, "the rollout loop was not captured"
        _check_rollout_stepwise(eng, ocfg, trees, seeds, stochastic, 5, n_obs)
        if graphs:
            assert eng._ro_cache[(B, stochastic)]["calls"] == 2 and eng._ro_cache[(B, stochastic)]["graph"] is not None


def _oracle_mode_actions(tree, ocfg, r):
    """the oracle policy's deterministic actions along the stored trajectory r (its own carry from zero) -> [B, T, n, 2]"""
    n = ocfg.n_agents
    h = torch.zeros(r["agent"].shape[0], n, 64)
    out = []
    for t in range(r["actions"].shape[1]):
        g = T.graph_to_torch(E.get_graph(ocfg, r["agent"][:, t], r["goal"], r["obst"], r["hits"][:, t]))
        with torch.no_grad():
            a, h = T.policy_mode(tree, g, h, n)
        out.append(a.numpy())
    return np.stack(out, axis=1)


def _with_old_first_layer(new, old):
    """the tree `new` with the first GNN layer of `old`: what a policy with stale layer-0 weights alone computes"""
    mixed = T.tree_map(lambda t: t, new)
    gnn = dict(mixed["params"]["PolicyNet_0"]["GraphTransformerGNN_0"])
    gnn["GraphTransformer_0"] = old["params"]["PolicyNet_0"]["GraphTransformerGNN_0"]["GraphTransformer_0"]
    mixed["params"]["PolicyNet_0"] = dict(mixed["params"]["PolicyNet_0"], GraphTransformerGNN_0=gnn)
    return mixed


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 4, 2), ("LidarSpread", 8, 3)])
def test_rollout_after_an_update_follows_the_new_parameters(cuda, kind, n, n_obs, graphs):
    """One pass of Engine.update (three minibatches: three Adam steps per network) between rollouts of the same engine; the
    rollouts after it, re-derived by the oracle from the engine's NEW parameters.  The fused step reads the prepared layer-0
    weights gnn0.Mcat / gnn0.cvec directly and, with HIP graphs, the checked rollout is the replay of a loop captured before
    the update: a weight left at its old value anywhere on that path moves the actions off the oracle's.
    That the 1e-5 bar would see it is asserted, not assumed: along the checked trajectory the oracle's own actions under the
    old tree, and under the new tree with only the old first GNN layer, differ from the new tree's by more than 10 x 1e-5.
    Measured on an MI355X, the largest action difference after the three Adam steps (lr 3e-4), eager and replay alike:
    LidarSpread n = 4: 8.2e-2 under the old tree, 4.0e-3 with the old first layer only; n = 8: 1.9e-1 and 5.4e-3 — at least
    40 times the asserted margin, so one pass of the update is enough."""
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, B, T_, cuda, BS, RS, use_graphs=graphs, multi_stream=graphs)
    assert eng.fused_step and eng.use_graphs == graphs
    seeds = _seeds(cuda)
    to_torch = lambda tree: T.tree_map(lambda a: torch.from_numpy(np.ascontiguousarray(a)), tree)
    # a first iteration sizes every scratch buffer (a buffer that grows in the first update makes the next rollout capture
    # its loop anew), so that the rollout checked below is a true replay of a loop captured BEFORE the update under test
    ro, det = eng.rollout_pair(seeds, seeds + 1000, noise_seed=3)
    eng.update(ro, det, 0, np.array([4, 1, 5, 0, 2, 3]))
    for it in (1, 2):
        ro, det = eng.rollout_pair(seeds + it, seeds + 1000 + it, noise_seed=3 + it)
    captured = {s: eng._ro_cache[(B, s)]["graph"] for s in (True, False)} if graphs else {}
    assert all(g is not None for g in captured.values()), "the rollout loop was not captured"
    old, before = to_torch(eng.policy.to_tree()), eng.policy.params.clone()
    info = eng.update(ro, det, 1, np.array([2, 5, 0, 3, 1, 4]))
    assert info["policy/has_nan"] == 0.0 and float(eng.opt["policy"].state[2]) == 2 * (B // (BS // T_))
    moved = float((eng.policy.params - before).abs().max())
    assert moved > 1e-4, f"the policy parameters moved by {moved:.3e} only"
    new = to_torch(eng.policy.to_tree())
    trees = dict(trees, policy=new)
    for stochastic in (True, False):
        rec = _check_rollout_stepwise(eng, ocfg, trees, seeds + 50, stochastic, 9, n_obs)
        if graphs:
            assert eng._ro_cache[(B, stochastic)]["graph"] is captured[stochastic], "the rollout was not a replay"
    # the margin of the check above, on the deterministic record just verified
    r = _np_rollout(rec)
    a_new = _oracle_mode_actions(new, ocfg, r)
    np.testing.assert_allclose(r["actions"], a_new, atol=TOL)
    for label, stale in (("old tree", old), ("old first GNN layer", _with_old_first_layer(new, old))):
        d = float(np.abs(_oracle_mode_actions(stale, ocfg, r) - a_new).max())
        print(f"{kind} n={n} graphs={graphs}: oracle actions under the {label} differ from the new tree's by {d:.3e}")
        assert d > 10 * TOL, f"a rollout with the {label} would pass the {TOL:g} bar: its actions differ by {d:.3e} only"
