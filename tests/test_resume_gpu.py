"""Resuming a stopped run on the GPU: Engine.state_dict / load_state_dict into an engine whose graphs are captured, the algo
surface (save_state / load_state with every generator), and `train.py --resume` against an uninterrupted run, on one rank
and on two.

What "continues" promises ("Resuming a stopped run"): everything that is a function of the state alone is bit-exact
— the restored buffers, the rollouts of the resume iteration, the evaluation at the resume step, the keys and the minibatch
order.  Updates use float atomics in the weight-gradient reductions, so after updates a resumed run follows the
uninterrupted one as two uninterrupted runs follow each other: 2e-5 of the parameter scale after one update
(test_multi_stream_update_equals_single_stream), 5e-5 of scale over up to three iterations (_assert_params_follow)."""
import json
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 5. engine round trip ---------------------------------------------------------------------------------------------
def _engine(algo, cuda, seed, n=3, noise=77):
    from dgppo_amd import _native as N, engine as EN, init
    B, T_, rs, bs = 8, 8, 4, 16
    cfg = N.make_env_cfg(N.ENV_KINDS["LidarSpread"], n, 2)
    hp = EN.Hyper(batch_size=bs, rnn_step=rs, train_steps=100, lagr_init=0.5, lr_lagr=1e-2)
    eng = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=True, multi_stream=True, algo=algo)
    eng.policy.load_tree(init.init_policy(seed, cfg.node_dim, 2, 2))
    eng.Vl.load_tree(init.init_value(seed, cfg.node_dim, 1, 2, 2))
    if algo == "dgppo":
        eng.Vh.load_tree(init.init_value(seed, cfg.node_dim, cfg.n_cost, 1, 3))
    elif algo == "informarl_lagr":
        eng.Vh.load_tree(init.init_value(seed, cfg.node_dim, cfg.n_cost, 1, 3, global_info=True))
    eng.set_entropy_noise(noise)
    return eng, B


def _iteration(eng, B, it, cuda):
    seeds = (torch.arange(1, B + 1, dtype=torch.int64, device=cuda) + 50 * it) * 7919
    ro = eng.rollout(seeds, True, noise_seed=3 + it)
    det = eng.rollout(seeds + 1000, False) if eng.algo == "dgppo" else None
    info = eng.update(ro, det, it, np.random.default_rng(it).permutation(B))
    torch.cuda.synchronize()
    return info


def _record(ro):
    """every field of a finalized rollout record, by name"""
    ro.finalize()
    out = {f"step.{k}": v for k, v in ro.step.items()}
    out.update({f"env.{k}": v for k, v in ro.env.items()})
    out.update(actions=ro.actions, rnn_states=ro.rnn_states, rewards=ro.rewards, costs=ro.costs)
    if ro.stochastic:
        out["log_pis"] = ro.log_pis
    return out


def _assert_same_record(a, b, label):
    ra, rb = _record(a), _record(b)
    assert set(ra) == set(rb)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), f"{label}: {k} differs"


@pytest.mark.parametrize("algo", ["dgppo", "informarl", "hcbfcrpo", "informarl_lagr"])
def test_engine_state_round_trip_into_a_captured_engine(cuda, algo):
    X, B = _engine(algo, cuda, seed=0)
    _iteration(X, B, 0, cuda)
    Y, _ = _engine(algo, cuda, seed=1, noise=5)
    _iteration(Y, B, 7, cuda)                              # Y's graphs are captured, its buffers hold a run of its own
    assert Y._ro_cache[(B, True)]["graph"] is not None and Y._upd_graph.get("graph") is not None
    assert not torch.equal(X.policy.params, Y.policy.params) and not torch.equal(X.eps_hat, Y.eps_hat)
    ptrs = {k: t.data_ptr() for k, t in Y._state_tensors().items()}
    sd = X.state_dict()

    # a state of another configuration is refused by name, before anything is written
    before = {k: t.clone() for k, t in Y._state_tensors().items()}
    other_n, _ = _engine(algo, cuda, seed=0, n=4)
    with pytest.raises(ValueError, match="n_agents"):
        Y.load_state_dict(other_n.state_dict())
    other_algo, _ = _engine("informarl" if algo == "dgppo" else "dgppo", cuda, seed=0)
    with pytest.raises(ValueError, match="'algo'"):
        Y.load_state_dict(other_algo.state_dict())
    torn = dict(sd, policy=dict(sd["policy"], m=sd["policy"]["m"][:-1]))
    with pytest.raises(ValueError, match="policy/m"):
        Y.load_state_dict(torn)
    for k, t in Y._state_tensors().items():
        assert torch.equal(t, before[k]), f"{k} changed by a refused load"

    # the tree is what the weights-only file functions accept, and it survives them
    from dgppo_amd.utils import checkpoint as CK
    sd = CK.loads_tree(pickle.dumps(sd))
    Y.load_state_dict(sd)
    names = set(Y._state_tensors())
    want = {f"{k}/{p}" for k in X.nets for p in ("params", "m", "v", "state")} | {"eps_hat"}
    assert names == want | ({"lagr"} if algo == "informarl_lagr" else set())
    for k, t in Y._state_tensors().items():
        assert t.data_ptr() == ptrs[k], f"{k} was rebound"
        assert torch.equal(t, X._state_tensors()[k]), f"{k} differs after the load"
    assert float(X.opt["policy"].state[2]) == float(Y.opt["policy"].state[2]) == 4.0
    assert float(X.opt["policy"].m.abs().max()) > 0
    if algo == "informarl_lagr":
        assert float((X.lagr - 0.5).abs().max()) > 1e-6, "the multipliers did not move: the check would be vacuous"

    # Y's captured graphs read the loaded values: rollouts are bit-equal, stochastic and deterministic
    seeds = (torch.arange(1, B + 1, dtype=torch.int64, device=cuda) + 900) * 7919
    rx, ry = X.rollout(seeds, True, 31), Y.rollout(seeds, True, 31)
    _assert_same_record(rx, ry, "stochastic rollout after the load")
    dx, dy = X.rollout(seeds + 1000, False), Y.rollout(seeds + 1000, False)
    _assert_same_record(dx, dy, "deterministic rollout after the load")

    # ... and so does the captured minibatch step: one more update on both, same rollouts and permutation
    perm = np.random.default_rng(5).permutation(B)
    det = algo == "dgppo"
    ix = X.update(rx, dx if det else None, 1, perm)
    iy = Y.update(ry, dy if det else None, 1, perm)
    torch.cuda.synchronize()
    for name in X.nets:
        pa, pb = X.nets[name].params, Y.nets[name].params
        assert float(X.opt[name].state[2]) == float(Y.opt[name].state[2]) == 8.0
        err = float((pa - pb).abs().max())
        print(f"[resume] {algo} {name}: |dp| = {err:.3e}, scale {float(pa.abs().max()):.3g}")
        assert err <= 2e-5 * max(1.0, float(pa.abs().max())), f"{name}: parameters differ by {err:.3e}"
    if algo == "informarl_lagr":
        assert float((X.lagr - Y.lagr).abs().max()) <= 2e-5 * max(1.0, float(X.lagr.abs().max()))
    for k in ("Vl/loss", "Vh/loss_Vh", "policy/loss", "policy/entropy"):          # as in the multi-stream test
        if k in ix:
            assert abs(ix[k] - iy[k]) <= 1e-4 * max(1.0, abs(ix[k])), k


# ---- 6. algo round trip -----------------------------------------------------------------------------------------------
def test_algo_save_state_load_state(cuda, tmp_path):
    from dgppo.algo import make_algo
    from dgppo.env import make_env
    env = make_env("LidarSpread", 3, num_obs=1, max_step=16)

    def mk(algo="dgppo"):
        return make_algo(algo=algo, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=env.num_agents, batch_size=128, rnn_step=8, train_steps=10, seed=3)
    saved_global = np.random.get_state()
    try:
        np.random.seed(3)                                   # as train.py does before it builds the algo
        a1 = mk()
        for it in range(2):
            a1.update(a1.collect(None, np.arange(1, 17) + 100 * it), it)
        path = str(tmp_path / "2.pkl")
        a1.save_state(path)
        assert os.listdir(tmp_path) == ["2.pkl"]
        perm1 = a1._perm(16)                                # a1's next minibatch order (moves the global np.random on)
        a2 = mk()                                           # draws its own entropy-noise seed from the moved global state
        assert not torch.equal(a1.engine.eps_hat, a2.engine.eps_hat)
        with pytest.raises(ValueError, match="'algo'"):
            mk("informarl").load_state(path)
        a2.load_state(path)
        np.testing.assert_array_equal(a2._perm(16), perm1)
        for k, t in a1.engine._state_tensors().items():
            assert torch.equal(t, a2.engine._state_tensors()[k]), k
        assert a1._rng.bit_generator.state == a2._rng.bit_generator.state
        assert a1._perm_rng.bit_generator.state == a2._perm_rng.bit_generator.state
        keys = np.arange(1, 17) + 5000
        r1, r2 = a1.collect(None, keys), a2.collect(None, keys)
        for f in ("actions", "log_pis", "rewards", "costs", "rnn_states"):
            assert torch.equal(getattr(r1, f), getattr(r2, f)), f
        assert torch.equal(r1.graph.states, r2.graph.states)
        # the deterministic companion rollout: its keys and the noise seed were drawn inside collect()
        d1, d2 = a1._pending_det[1].finalize(), a2._pending_det[1].finalize()
        for f in ("agent", "actions", "rewards", "costs"):
            assert torch.equal(getattr(d1, f), getattr(d2, f)), f"deterministic {f}"
        assert a1._rng.bit_generator.state == a2._rng.bit_generator.state
    finally:
        np.random.set_state(saved_global)


# ---- 7. / 8. the command line -----------------------------------------------------------------------------------------
def _train(tmp_path, extra, gpus=1, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "1",
           "--steps", "4", "--n-env-train", "16", "--batch-size", "2048", "--n-env-test", "4", "--eval-interval", "1",
           "--save-interval", "2", "--log-dir", str(tmp_path / "logs")]
    if gpus > 1:
        cmd += ["--gpus", str(gpus)]
    for i in range(0, len(extra), 2):                       # a later occurrence of a flag wins in argparse
        cmd += extra[i:i + 2]
    env = dict(os.environ, DGPPO_DIST_BACKEND="gloo") if gpus > 1 else None
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


def _rows(run_dir):
    return [json.loads(ln) for ln in open(os.path.join(run_dir, "metrics.jsonl"))]


def _weights_follow(dir_a, dir_b, tol):
    """max |a - b| over a network's leaves <= tol x the network's largest |weight|, for every {actor,Vl,Vh}.pkl"""
    from dgppo_amd.utils import checkpoint as CK

    def leaves(t):
        return [x for v in t.values() for x in leaves(v)] if isinstance(t, dict) else [np.asarray(t)]
    worst = 0.0
    for fname in ("actor.pkl", "Vl.pkl", "Vh.pkl"):
        la, lb = (leaves(CK.load_state(os.path.join(d, fname))) for d in (dir_a, dir_b))
        assert len(la) == len(lb)
        scale = max(float(np.abs(x).max()) for x in la)
        err = max(float(np.abs(x - y).max()) for x, y in zip(la, lb))
        print(f"[resume] {fname}: |resumed - uninterrupted| = {err:.3e} = {err / scale:.3e} of scale {scale:.3g}")
        worst = max(worst, err / scale)
    assert worst <= tol, f"the resumed run's weights are {worst:.3e} of scale from the uninterrupted run's (bound {tol:g})"


def _resume_against_uninterrupted(tmp_path, gpus):
    out = _train(tmp_path, [], gpus)
    assert out.returncode == 0, out.stderr[-3000:]
    root = tmp_path / "logs" / "LidarSpread" / "dgppo"
    runs = os.listdir(root)
    assert len(runs) == 1, runs                             # one writer: another rank's run directory would be a second one
    run_a, run_b = root / runs[0], tmp_path / "stopped"
    assert sorted(os.listdir(run_a)) == ["config.yaml", "metrics.jsonl", "models", "resume"]
    assert sorted(os.listdir(run_a / "resume")) == ["2.pkl", "4.pkl", "flags.yaml"]
    import yaml
    flags = yaml.safe_load(open(run_a / "resume" / "flags.yaml"))
    assert flags["steps"] == 4 and flags["gpus"] == gpus and flags["batch_size"] == 2048 and "resume" not in flags
    assert not any(ln.startswith("resume:") for ln in open(run_a / "config.yaml"))      # config.yaml keeps its keys
    # the stopped run: A's directory with step 2 as the newest state; the metrics of steps 2..4 are still in the file
    shutil.copytree(run_a, run_b)
    shutil.rmtree(run_b / "models" / "4")
    os.remove(run_b / "resume" / "4.pkl")
    config_before = open(run_b / "config.yaml").read()
    out_b = _train(tmp_path, ["--resume", str(run_b)], gpus)
    assert out_b.returncode == 0, out_b.stderr[-3000:]
    assert "step:   2" in out_b.stdout and "step:   1" not in out_b.stdout and "step:   4" in out_b.stdout
    assert os.listdir(root) == runs                         # no new run directory
    assert sorted(os.listdir(run_b)) == ["config.yaml", "metrics.jsonl", "models", "resume"]
    assert open(run_b / "config.yaml").read() == config_before
    assert sorted(os.listdir(run_b / "resume")) == ["2.pkl", "4.pkl", "flags.yaml"]
    assert sorted(os.listdir(run_b / "models")) == ["0", "2", "4"]
    for s in ("0", "2", "4"):
        assert sorted(os.listdir(run_b / "models" / s)) == ["Vh.pkl", "Vl.pkl", "actor.pkl"]
    rows_a, rows_b = _rows(run_a), _rows(run_b)
    assert [(r["step"], sorted(r)) for r in rows_b] == [(r["step"], sorted(r)) for r in rows_a]      # no duplicate, no gap
    assert [r for r in rows_b if r["step"] < 2] == [r for r in rows_a if r["step"] < 2]
    ev = lambda rows: [r for r in rows if r["step"] == 2 and "eval/reward" in r]
    assert len(ev(rows_a)) == 1 and ev(rows_b) == ev(rows_a)                # a function of the restored weights alone
    # the weights saved again at the resume step are the stopped run's, bit for bit
    for fname in ("actor.pkl", "Vl.pkl", "Vh.pkl"):
        assert open(run_b / "models" / "2" / fname, "rb").read() == open(run_a / "models" / "2" / fname, "rb").read()
    _weights_follow(str(run_a / "models" / "4"), str(run_b / "models" / "4"), 5e-5)
    return run_b


def test_train_py_resume_follows_the_uninterrupted_run(cuda, tmp_path):
    """Two iterations (2 and 3) after the resume at step 2, compared with the run that never stopped."""
    run_b = _resume_against_uninterrupted(tmp_path, 1)
    out = _train(tmp_path, ["--resume", str(run_b), "--steps", "5"])
    assert out.returncode != 0 and "--steps" in out.stderr and "--gpus" not in out.stderr, out.stderr[-2000:]
    out = _train(tmp_path, ["--resume", str(tmp_path / "no_such_run")])
    assert out.returncode != 0 and "weights only" in out.stderr, out.stderr[-2000:]


def test_train_py_resume_two_ranks(cuda, tmp_path):
    """`--gpus 2` (two gloo ranks on this GPU, started and supervised by train.py itself): every rank loads rank 0's file."""
    _resume_against_uninterrupted(tmp_path, 2)
