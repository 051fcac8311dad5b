"""Engine.update held to the oracle at EVERY minibatch, teacher-forced: a hook records, just before each optimiser step,
the parameters, gradients and optimiser state of the network; afterwards each step is compared on the device's own inputs
to that step, so that no comparison inherits the rounding of an earlier one (Adam's first steps are ~ lr * sign(g): a
gradient entry near zero may change sign between fp32 and float64 and move a free-running oracle by 2 lr).

  (a) per-leaf gradients of minibatch mb against autograd through the oracle at the parameters snapshotted at mb;
  (b) the float64 clip + Adam step on the device's (p, g, m, v, count) equals the next snapshot (the final state at the end);
  (c) the logged scalars against the oracle's for the LAST minibatch at the last snapshot;
  (d) a precondition on the CPU: the oracle gradient of minibatch mb at the mb - 1 snapshot differs from the one at the mb
      snapshot by more than 4x the tolerance of (a) — a stale prepared weight or a skipped step could not pass (a);
  (e) DGPPO / LidarSpread: the next iteration's rollouts and value pre-passes read the moved parameters.

Largest error of a logged scalar against the oracle over all cases, measured on an MI355X (bar: 1e-5 * max(1, |oracle|)):
  Vl/loss 7.2e-7 (bar 3.5e-5), Vh/loss_Vh 2.4e-7 (1.5e-5), Vh/loss 0, policy/loss 1.9e-6 (1.3e-4; |loss| = 13.3),
  policy/entropy 9.5e-7 (8.2e-5; |entropy| = 8.2), policy/total_variation_dist 6.0e-8 (1e-5); the clip count equals the
  oracle's in every case with no row on the clip boundary; */grad_norm within 1.3e-4 of its triangle bound.  No tolerance is
  widened from the 1e-5 bar.  Precondition (d): the smallest margin over all cases is 16 000x the tolerance of (a).
With the learning rates of (d) the policy moves far in one step: from the second minibatch on most rows are clipped
(18 to 48 of 48), so the policy gradient there is mostly the entropy term's and that of the rows still inside the clip range.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import algo_ref as A
from oracle import dgppo_ref as R
from oracle import nn_torch as T

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_engine_gpu import _check_minibatch_grads, _check_rollout_stepwise, _close, _np_rollout, _setup  # noqa: E402

pytestmark = pytest.mark.gpu

T_, RS, BS = 8, 4, 16                                   # Eb = 2 envs per minibatch, 2 chunks of 4 steps per env
GRAD_TOL = 5e-5                                         # _check_minibatch_grads' per-entry tolerance
LR = dict(lr_actor=1e-2, lr_Vl=1e-2, lr_Vh=1e-2)        # one step moves the weights visibly: see (d)
PERM = {6: np.array([4, 1, 5, 0, 3, 2]), 4: np.array([2, 0, 3, 1])}
# what dgppo_clip_adam_step receives for its default betas / eps: the fp32 values
B1, B2, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
LOSS_KEYS = ("Vl/loss", "Vh/loss_Vh", "Vh/loss", "policy/loss", "policy/entropy", "policy/total_variation_dist")
SCALAR_TOL = {k: 1e-5 for k in LOSS_KEYS}               # the fp32 bar of _close, per key


def _torch_tree(tree, grad=False):
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return T.tree_map((lambda a: leaf(a).requires_grad_()) if grad else leaf, tree)


def _recording_hook(eng, snaps):
    """grad_hook that keeps, per (network, minibatch), what dgppo_clip_adam_step is about to read"""
    def hook(name, net, mb):
        assert (name, mb) not in snaps, f"the hook fired twice for {name} in minibatch {mb}"
        opt = eng.opt[name]
        s = dict(p=net.params.detach().clone(), g=net.grads.detach().clone(), m=opt.m.clone(), v=opt.v.clone(),
                 state=opt.state[:8].clone(), p_tree=net.to_tree(), g_tree=net.to_tree(net.grads))
        if eng.algo == "informarl_lagr":
            s["lagr"] = eng.lagr.clone()
        snaps[(name, mb)] = s
    return hook


def _final_state(eng):
    return {name: dict(p=net.params.detach().clone(), m=eng.opt[name].m.clone(), v=eng.opt[name].v.clone(),
                       state=eng.opt[name].state[:8].clone()) for name, net in eng.nets.items()}


def _grad_gap(leaf_a, leaf_b, name):
    """largest entry of |grad a - grad b| over the leaves of one network"""
    ga = dict(T.tree_leaves(T.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), leaf_a[name])))
    gb = dict(T.tree_leaves(T.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), leaf_b[name])))
    return max(float((ga[k].double() - gb[k].double()).abs().max()) for k in ga)


def _check_trajectory(eng, snaps, info, perm, losses, tg_np, r, label):
    """(d), (a), (b), (c) of the module docstring after eng.update(...).  losses(leaf, idx, detail): the oracle's minibatch
    losses, which also leave the gradients in `leaf`.  -> {logged key: |error| against the oracle}"""
    hp, names = eng.hp, tuple(eng.nets)
    Eb = hp.batch_size // eng.T
    n_mb = len(perm) // Eb
    rows = Eb * eng.T * eng.cfg.n_agents
    assert n_mb >= 2 and set(snaps) == {(name, mb) for name in names for mb in range(n_mb)}
    fin = _final_state(eng)
    idx = [perm[mb * Eb:(mb + 1) * Eb] for mb in range(n_mb)]
    assert all(list(i) != sorted(i) for i in idx), "every minibatch gathers unordered env ids"
    own, want, detail = [], [], []                  # the oracle on minibatch mb at the parameters snapshotted at mb
    for mb in range(n_mb):
        own.append({k: _torch_tree(snaps[(k, mb)]["p_tree"], grad=True) for k in names})
        detail.append({})
        want.append(losses(own[mb], idx[mb], detail[mb]))
    # (d) the previous snapshot gives a visibly different gradient on the same minibatch (CPU, oracle only)
    for mb in range(1, n_mb):
        stale = {k: _torch_tree(snaps[(k, mb - 1)]["p_tree"], grad=True) for k in names}
        losses(stale, idx[mb], None)
        for k in names:
            g = dict(T.tree_leaves(T.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), own[mb][k])))
            bound = GRAD_TOL * max(max(float(v.abs().max()) for v in g.values()), 1e-3)
            margin = _grad_gap(own[mb], stale, k) / bound
            print(f"{label} (d) minibatch {mb} {k}: stale-parameter gradient differs by {margin:.1f} x the tolerance of (a)")
            assert margin > 4.0, f"{label}: (a) could not see a stale {k} step at minibatch {mb} (margin {margin:.2f})"
    # (a) gradients of every minibatch
    gstat = [_check_minibatch_grads(own[mb], {k: snaps[(k, mb)]["g_tree"] for k in names}, names, GRAD_TOL,
                                    f"{label} minibatch {mb}: ") for mb in range(n_mb)]
    # (b) the optimiser step between consecutive snapshots
    lrs = {"policy": hp.lr_actor, "Vl": hp.lr_Vl, "Vh": hp.lr_Vh}
    c = lambda x: x.cpu().numpy()
    for k in names:
        for mb in range(n_mb):
            s, nxt = snaps[(k, mb)], (snaps[(k, mb + 1)] if mb + 1 < n_mb else fin[k])
            p, g, m, v, st = (c(s[q]) for q in ("p", "g", "m", "v", "state"))
            assert st[2] == mb, f"{label} {k}: Adam count {st[2]} entering minibatch {mb}"
            assert float(np.abs(p).max()) < 4.0, "the 2e-6 bound on the parameters is tied to |p| < 4"
            pr, mr, vr, cr, norm, bad = A.clip_adam(p, g, m, v, int(st[2]), float(np.float32(lrs[k])),
                                                    float(np.float32(hp.max_grad_norm)), B1, B2, EPS)
            assert not bad and cr == mb + 1
            where = f"{label} {k} after the step of minibatch {mb}"
            np.testing.assert_allclose(c(nxt["p"]), pr, rtol=0, atol=2e-6, err_msg=where)
            np.testing.assert_allclose(c(nxt["m"]), mr, rtol=1e-4, atol=1e-8, err_msg=where)
            np.testing.assert_allclose(c(nxt["v"]), vr, rtol=1e-4, atol=1e-10, err_msg=where)
            sn = c(nxt["state"])
            assert sn[2] == mb + 1 and sn[5] == 0.0, where
            np.testing.assert_allclose(sn[4], norm, rtol=1e-5, err_msg=where)
    # (c) logged scalars: the last minibatch at the last snapshot
    last = n_mb - 1
    w, d = want[last], detail[last]
    for key, arr in (("Vl", tg_np["Ql"]), ("Vh", tg_np.get("Qh") if eng.algo == "informarl_lagr" else None)):
        if arr is not None:
            assert info[f"{key}/max_target"] == float(arr[idx[last]].max()), f"{label} {key}/max_target"
            assert info[f"{key}/min_target"] == float(arr[idx[last]].min()), f"{label} {key}/min_target"
    assert info["policy/log_pi_min"] == float(r["log_pis"].min())
    nan_keys = [k for k in info if k.endswith("has_nan")]
    assert len(nan_keys) == len(names) and all(info[k] == 0.0 for k in nan_keys)
    # clip_frac is a count over the rows: it may differ by the rows whose rho lies within log_pi's own tolerance
    # (1e-5 * max(1, |log_pi|)) of 1 +- clip_eps
    reach = 1e-5 * d["lp"].abs().clamp_min(1.0)
    border = int((((d["rho"] / (1 - hp.clip_eps) - 1).abs() < reach) | ((d["rho"] / (1 + hp.clip_eps) - 1).abs() < reach)).sum())
    assert border <= 0.02 * rows, f"{label}: {border} of {rows} rows on the clip boundary: choose other seeds"
    got_clip, want_clip = info["policy/clip_frac"] * rows, int(d["clipped"].sum())
    assert abs(w["policy/clip_frac"] * rows - want_clip) < 1e-3
    print(f"{label} (c) clipped rows {got_clip:.3f} (oracle {want_clip}, on the boundary {border}) of {rows}")
    errs = {}
    for k in LOSS_KEYS:
        assert (k in info) == (k in w), f"{label}: {k} logged {k in info}, in the oracle {k in w}"
        if k in w:
            errs[k] = abs(info[k] - w[k])
            print(f"{label} (c) {k}: {info[k]!r} oracle {w[k]!r} error {errs[k]:.3e} bar {SCALAR_TOL[k] * max(1.0, abs(w[k])):.3e}")
    assert {"Vl/loss", "policy/loss", "policy/entropy", "policy/total_variation_dist"} <= set(errs) and len(errs) == 2 + len(names)
    norm_key = {"Vl": "Vl/grad_norm", "policy": "policy/grad_norm",
                "Vh": "Vh/grad_norm" if eng.algo == "informarl_lagr" else "Vh/grad_Vh_norm"}
    for k in names:
        # | ||g_dev|| - ||g_ref|| | <= ||g_dev - g_ref|| <= sqrt(P) x the per-entry bound of (a); the logged fp32 norm
        # is within (b)'s 1e-5 of ||g_dev||
        gs = gstat[last][k]
        dev_norm = float(np.sqrt((c(snaps[(k, last)]["g"]).astype(np.float64) ** 2).sum()))
        bound = np.sqrt(gs["count"]) * gs["bound"] + 1e-5 * dev_norm
        err = abs(info[norm_key[k]] - gs["norm"])
        print(f"{label} (c) {norm_key[k]}: {info[norm_key[k]]!r} oracle {gs['norm']!r} error {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{label} {norm_key[k]}: {err:.3e} > {bound:.3e}"
    assert abs(got_clip - want_clip) <= border + 1e-3, f"{label}: clip count {got_clip} vs {want_clip} (+- {border})"
    for k, e in errs.items():
        assert e <= SCALAR_TOL[k] * max(1.0, abs(w[k])), f"{label} {k}: {info[k]!r} vs oracle {w[k]!r}: error {e:.3e}"
    return errs


def _hpd(hp):
    return dict(gamma=hp.gamma, gae_lambda=hp.gae_lambda, alpha=hp.alpha, cbf_eps=hp.cbf_eps, rnn_step=RS,
                clip_eps=hp.clip_eps, coef_ent=hp.coef_ent)


def _run(eng, ocfg, cuda, B, step, label):
    """rollouts with the usual seeds, the device's targets, one update under the recording hook, then the checker.
    -> (ro, det, snaps, info)"""
    algo = eng.algo
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3).finalize()
    det = eng.rollout(seeds + 1000, False).finalize() if algo == "dgppo" else None
    tg = (eng.targets_informarl(ro, step) if algo == "informarl" else eng.targets_hcbfcrpo(ro, step) if algo == "hcbfcrpo" else
          eng.targets_lagr(ro, step) if algo == "informarl_lagr" else eng.targets(ro, det, step))
    tg_np = {k: v.cpu().numpy().copy() for k, v in tg.items()}
    r, d = _np_rollout(ro), (_np_rollout(det) if det is not None else None)
    hpd, eps_hat = _hpd(eng.hp), eng.eps_hat.cpu().clone()
    if algo == "informarl_lagr":
        losses = lambda leaf, idx, detail: R.minibatch_losses_lagr(leaf, ocfg, r, tg_np, idx, hpd, eps_hat, detail)
    else:
        losses = lambda leaf, idx, detail: R.minibatch_losses(leaf, ocfg, r, d, tg_np, idx, hpd, eps_hat, detail)
    snaps = {}
    eng.grad_hook = _recording_hook(eng, snaps)
    perm = PERM[B]
    info = eng.update(ro, det, step, perm)
    torch.cuda.synchronize()
    eng.grad_hook = None
    _check_trajectory(eng, snaps, info, perm, losses, tg_np, r, label)
    return dict(ro=ro, det=det, r=r, tg_np=tg_np, snaps=snaps, info=info, perm=perm, hpd=hpd, eps_hat=eps_hat)


@pytest.mark.parametrize("kind,n,n_obs", [("LidarSpread", 3, 2), ("MPESpread", 3, 3)])
def test_dgppo_update_every_minibatch_against_the_oracle(cuda, kind, n, n_obs):
    """three minibatches of unordered env ids; for LidarSpread also (e): after the update, fresh rollouts and the value
    pre-passes are held to the oracle evaluated at the parameters the update left behind."""
    B, step = 6, 60
    cfg, ocfg, hp, eng, trees = _setup(kind, n, n_obs, B, T_, cuda, BS, RS, hyper_kw=LR)
    _run(eng, ocfg, cuda, B, step, f"dgppo {kind}")
    assert float(eng.opt["policy"].state[2]) == 3
    if kind != "LidarSpread":
        return
    new = {k: _torch_tree(net.to_tree()) for k, net in eng.nets.items()}
    for k in new:
        old = dict(T.tree_leaves(trees[k]))
        moved = max(float((a - old[path]).abs().max()) for path, a in T.tree_leaves(new[k]))
        assert moved > 1e-3, f"{k} did not move: (e) would repeat test_rollout_matches_oracle_stepwise"
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 104729 + 17
    ro = _check_rollout_stepwise(eng, ocfg, new, seeds, True, 9, n_obs)
    det = _check_rollout_stepwise(eng, ocfg, new, seeds + 1000, False, 0, n_obs)
    tg = eng.targets(ro, det, step + 1)
    wt = R.targets(new, ocfg, _np_rollout(ro), _np_rollout(det), _hpd(hp), eng.cbf_weight_at(step + 1))
    for k in ("Vl", "Vh", "Vh_det", "Ql", "Qh", "Qh_det"):
        _close(tg[k], wt[k], f"after the update: {k}")


def test_data_parallel_path_update_every_minibatch_against_the_oracle(cuda):
    """Engine(allreduce=..., world=1): the three backward passes into the flat gradient buffer first, then the three
    optimiser steps (body_post); a sum over one rank is the identity, so the oracle is the single-device one."""
    B = 4
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, BS, RS, hyper_kw=LR, allreduce=lambda flat: None, world=1)
    assert eng.allreduce is not None
    _run(eng, ocfg, cuda, B, 60, "data-parallel path")


@pytest.mark.parametrize("algo", ["informarl", "hcbfcrpo"])
def test_baselines_update_every_minibatch_against_the_oracle(cuda, algo):
    B = 4
    hyper_kw = dict(LR, cost_weight=0.3, cost_schedule=True) if algo == "informarl" else LR
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, BS, RS, hyper_kw=hyper_kw, algo=algo)
    assert set(eng.nets) == {"policy", "Vl"}
    out = _run(eng, ocfg, cuda, B, 60 if algo == "informarl" else 80, algo)
    assert "Vh/loss_Vh" not in out["info"] and ("eval/safe_data" in out["info"]) == (algo == "hcbfcrpo")


def test_informarl_lagr_update_every_minibatch_and_multiplier_step_against_the_oracle(cuda):
    """plus: after EACH minibatch the multipliers equal A.lagr_update on the oracle's whole-episode log pi of the device's
    post-step policy for that minibatch's envs, starting from the device's previous multipliers."""
    from dgppo_amd import engine as EN
    kind, n, n_obs, B = "LidarSpread", 3, 2, 4
    cfg, ocfg, hp0, eng0, trees = _setup(kind, n, n_obs, B, T_, cuda, BS, RS)
    hp = EN.Hyper(batch_size=BS, rnn_step=RS, train_steps=100, lagr_init=0.4, lr_lagr=0.05, **LR)
    eng = EN.Engine(cfg, hp, cuda, T=T_, algo="informarl_lagr", multi_stream=True)
    gen = torch.Generator().manual_seed(21)
    trees["Vh"] = T.tree_map(lambda t: t + 0.05 * torch.randn(t.shape, generator=gen), T.init_value(5, cfg.node_dim, 2, 1, global_info=True))
    for k, net in eng.nets.items():
        net.load_tree(trees[k])
    eng.set_entropy_noise(77)
    out = _run(eng, ocfg, cuda, B, 0, "informarl_lagr")
    snaps, perm, r, tg_np = out["snaps"], out["perm"], out["r"], out["tg_np"]
    Eb = BS // T_
    n_mb = B // Eb
    assert np.all(snaps[("policy", 0)]["lagr"].cpu().numpy() == np.float32(0.4))
    for mb in range(n_mb):
        idx = perm[mb * Eb:(mb + 1) * Eb]
        before = snaps[("policy", mb)]["lagr"].cpu().numpy()
        after = (snaps[("policy", mb + 1)]["lagr"] if mb + 1 < n_mb else eng.lagr).cpu().numpy()
        new_pol = _torch_tree(snaps[("policy", mb + 1)]["p_tree"] if mb + 1 < n_mb else eng.policy.to_tree())
        lp_new = R.log_pi_full_episode({"policy": new_pol}, ocfg, r, idx, out["eps_hat"])
        want = A.lagr_update(before, lp_new, r["log_pis"][idx], tg_np["Vh"][idx][:, :T_], tg_np["Ah"][idx], hp.gamma, hp.lr_lagr)
        assert not np.array_equal(after, before), f"the multipliers did not move in minibatch {mb}"
        np.testing.assert_allclose(after, want, atol=2e-6, err_msg=f"multipliers after minibatch {mb}")
    assert abs(out["info"]["policy/lagr_mean"] - float(want.mean())) < 1e-5


@pytest.mark.parametrize("use_rnn,rnn_layers,use_lstm", [(False, 1, False), (True, 2, False), (True, 1, True)])
def test_rnn_options_update_every_minibatch_against_the_oracle(cuda, use_rnn, rnn_layers, use_lstm):
    B = 4
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, BS, RS, use_rnn=use_rnn, rnn_layers=rnn_layers,
                                       use_lstm=use_lstm, hyper_kw=LR, multi_stream=True)
    _run(eng, ocfg, cuda, B, 10, f"rnn={use_rnn} x{rnn_layers} lstm={use_lstm}")
