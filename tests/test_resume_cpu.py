"""Resuming a stopped run, the parts that need no GPU: the state-file functions of dgppo_amd/utils/checkpoint.py, the
Trainer's save / retention / resume logic with a stub algo, and train.py's flag comparison."""
import importlib.util
import json
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from dgppo_amd.trainer.trainer import Trainer
from dgppo_amd.utils import checkpoint as CK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. round trip ----------------------------------------------------------------------------------------------------
def test_state_tree_round_trips_and_generators_continue(tmp_path):
    gen = np.random.default_rng([3, 99])
    gen.integers(1, 2 ** 62, size=5)
    gen.integers(0, 2 ** 31, dtype=np.uint32)            # leaves a buffered half draw (has_uint32 = 1)
    legacy = np.random.RandomState(5)
    legacy.standard_normal(3)                            # leaves a cached gaussian
    saved_global = np.random.get_state()
    try:
        np.random.set_state(legacy.get_state())
        tree = {"buf": {"params": np.arange(7, dtype=np.float32) / 3, "state": np.zeros(520, np.float32)},
                "name": CK.encode_str("informarl_lagr"), "lr": 1e-7, "step": 4,
                "rng": CK.generator_state(gen), "np_random": CK.global_numpy_state()}
        want_gen = gen.integers(1, 2 ** 62, size=8)
        want_perm = np.arange(10)
        np.random.shuffle(want_perm)
        want_norm = np.random.standard_normal(3)
        assert isinstance(tree["rng"]["state"], int) and tree["rng"]["state"] >= 2 ** 64      # a 128-bit integer, not an object
        assert tree["np_random"]["key"].dtype == np.uint32 and tree["np_random"]["key"].shape == (624,)
        path = str(tmp_path / "4.pkl")
        CK.save_state(tree, path)
        got = CK.load_state(path)
        np.testing.assert_array_equal(got["buf"]["params"], tree["buf"]["params"])
        assert got["buf"]["params"].dtype == np.float32
        assert CK.decode_str(got["name"]) == "informarl_lagr" and got["lr"] == 1e-7 and got["step"] == 4
        assert got["rng"] == tree["rng"]
        gen2 = np.random.default_rng(0)
        CK.set_generator_state(gen2, got["rng"])
        np.testing.assert_array_equal(gen2.integers(1, 2 ** 62, size=8), want_gen)
        np.random.seed(123)
        CK.set_global_numpy_state(got["np_random"])
        perm = np.arange(10)
        np.random.shuffle(perm)
        np.testing.assert_array_equal(perm, want_perm)
        np.testing.assert_array_equal(np.random.standard_normal(3), want_norm)
    finally:
        np.random.set_state(saved_global)


def test_state_file_still_refuses_str_leaves_and_objects(tmp_path):
    with pytest.raises(pickle.UnpicklingError):
        CK.save_state({"algo": "dgppo"}, str(tmp_path / "0.pkl"))
    assert os.listdir(tmp_path) == []                                               # refused before a file is opened
    with open(tmp_path / "1.pkl", "wb") as f:
        pickle.dump({"algo": "dgppo"}, f)
    with pytest.raises(pickle.UnpicklingError):
        CK.load_state(str(tmp_path / "1.pkl"))
    with open(tmp_path / "2.pkl", "wb") as f:
        pickle.dump({"rng": np.random.default_rng(0)}, f)                           # a pickled generator object
    with pytest.raises(pickle.UnpicklingError):
        CK.load_state(str(tmp_path / "2.pkl"))


# ---- 2. partial writes ------------------------------------------------------------------------------------------------
def test_latest_state_ignores_everything_but_numbered_files(tmp_path):
    d = tmp_path / "resume"
    assert CK.latest_state(str(d)) is None                                          # no directory
    d.mkdir()
    assert CK.latest_state(str(d)) is None
    for name in ("flags.yaml", "8.pkl.tmp", "best.pkl", "7.pkl.bak", "-3.pkl", "1e3.pkl", ".pkl"):
        (d / name).write_bytes(b"x")
    assert CK.latest_state(str(d)) is None
    CK.save_state({"v": 1}, str(d / "2.pkl"))
    CK.save_state({"v": 2}, str(d / "10.pkl"))
    assert CK.latest_state(str(d)) == 10 and CK.state_steps(str(d)) == [2, 10]      # numeric, not lexicographic


def test_truncated_tmp_next_to_a_good_file_changes_nothing(tmp_path):
    path = str(tmp_path / "6.pkl")
    tree = {"w": np.linspace(0, 1, 1000, dtype=np.float32), "step": 6}
    CK.save_state(tree, path)
    assert sorted(os.listdir(tmp_path)) == ["6.pkl"]                                # no .tmp after a successful save
    good = open(path, "rb").read()
    with open(str(tmp_path / "8.pkl.tmp"), "wb") as f:                              # a later save that was killed half way
        f.write(good[:len(good) // 2])
    with open(path + ".tmp", "wb") as f:                                            # and a torn rewrite of the same step
        f.write(good[:100])
    assert CK.latest_state(str(tmp_path)) == 6
    got = CK.load_state(path)
    np.testing.assert_array_equal(got["w"], tree["w"])
    assert got["step"] == 6
    CK.save_state(tree, path)                                                       # the next save replaces the torn .tmp
    assert sorted(os.listdir(tmp_path)) == ["6.pkl", "8.pkl.tmp"]


# ---- 3. Trainer resume against an uninterrupted run -------------------------------------------------------------------
class _Env:
    pass


class _Rollout:
    def __init__(self, rewards, costs):
        self.rewards, self.costs = rewards, costs


class _StubAlgo:
    """records what the Trainer hands it; its 'weights' and a generator of its own are its whole state"""
    world, rank = 1, 0

    def __init__(self):
        self.w = np.zeros(3, np.float32)
        self.rng = np.random.default_rng(17)
        self.rng.random(4)                                # whatever construction draws is overridden by load_state_dict
        self.calls = []
        self.saved = []

    def collect_deterministic(self, keys, env=None):      # evaluation: a function of the weights and the keys alone
        k = torch.from_numpy((np.asarray(keys) % 97).astype(np.float32))
        rewards = k[:, None] * 0.01 + float(self.w.sum()) + torch.arange(4)[None, :]
        costs = (rewards[:, :, None, None] - 5.0).expand(len(keys), 4, 2, 2) * 0.1
        return _Rollout(rewards, costs)

    def collect(self, params, keys):
        self.calls.append(("collect", tuple(int(k) for k in keys), float(self.rng.random())))
        return keys

    def update(self, rollout, step):
        self.calls.append(("update", tuple(int(k) for k in rollout), int(step)))
        self.w += self.rng.random(3).astype(np.float32)
        return {"loss": float(self.w[0]), "noise": float(self.rng.random())}

    def save(self, save_dir, step):
        os.makedirs(os.path.join(save_dir, str(step)), exist_ok=True)
        self.saved.append(step)

    def state_dict(self):
        return {"w": self.w.copy(), "rng": CK.generator_state(self.rng)}

    def load_state_dict(self, d):
        self.w[:] = d["w"]
        CK.set_generator_state(self.rng, d["rng"])


def _trainer(log_dir, algo, resume=False, steps=6):
    return Trainer(env=_Env(), env_test=_Env(), algo=algo, gamma=0.99, n_env_train=4, n_env_test=3, log_dir=str(log_dir), seed=1,
                   params={"run_name": "t", "training_steps": steps, "eval_interval": 1, "eval_epi": 1, "save_interval": 2},
                   resume=resume)


def test_trainer_resume_follows_the_uninterrupted_run(tmp_path):
    a_dir, b_dir = tmp_path / "A", tmp_path / "B"
    algo_a = _StubAlgo()
    tr_a = _trainer(a_dir, algo_a)
    tr_a.train()
    assert tr_a.update_steps == 7 and algo_a.saved == [0, 2, 4, 6]
    assert sorted(os.listdir(a_dir / "resume")) == ["4.pkl", "6.pkl"]                # the two newest, no .tmp
    assert sorted(os.listdir(a_dir / "models")) == ["0", "2", "4", "6"]              # weights saves are not pruned
    # B: A's directory as a run killed during iteration 5 leaves it — the state of step 4 is the newest, the metrics of
    # steps 4 and 5 are already on disk — plus the flags file that train.py writes and that must survive
    shutil.copytree(a_dir, b_dir)
    os.remove(b_dir / "resume" / "6.pkl")
    shutil.rmtree(b_dir / "models" / "6")
    (b_dir / "resume" / "flags.yaml").write_text("steps: 6\n")
    lines_a = open(a_dir / "metrics.jsonl").read().splitlines()
    kept = [ln for ln in lines_a if json.loads(ln)["step"] <= 5]
    (b_dir / "metrics.jsonl").write_text("\n".join(kept) + "\n" + lines_a[len(kept)][:17])      # the last line torn
    algo_b = _StubAlgo()
    tr_b = _trainer(b_dir, algo_b, resume=True)
    assert tr_b.start_step == 4 and tr_b.update_steps == 4
    tr_b.train()
    first = next(i for i, c in enumerate(algo_a.calls) if c[0] == "update" and c[2] == 4) - 1
    assert algo_a.calls[first][0] == "collect"
    assert algo_b.calls == algo_a.calls[first:] and [c[2] for c in algo_b.calls if c[0] == "update"] == [4, 5, 6]
    assert tr_b.update_steps == tr_a.update_steps == 7
    np.testing.assert_array_equal(algo_b.w, algo_a.w)
    assert algo_b.saved == [4, 6]
    assert open(b_dir / "metrics.jsonl").read().splitlines() == lines_a              # no duplicate, no gap
    assert sorted(os.listdir(b_dir)) == ["metrics.jsonl", "models", "resume"]        # no metrics.jsonl.tmp left
    assert sorted(os.listdir(b_dir / "resume")) == ["4.pkl", "6.pkl", "flags.yaml"]
    assert sorted(os.listdir(b_dir / "models")) == ["0", "2", "4", "6"]
    # the state of step s is the state BEFORE iteration s: step, update counter and the key generator ahead of its draw
    st = CK.load_state(str(a_dir / "resume" / "4.pkl"))
    assert set(st) == {"algo", "trainer"} and st["trainer"]["step"] == 4 and st["trainer"]["update_steps"] == 4
    key = np.random.default_rng(0)
    CK.set_generator_state(key, st["trainer"]["key"])
    assert tuple(int(k) for k in key.integers(1, 2 ** 62, size=4)) == algo_a.calls[first][1]


def test_trainer_resume_without_state_raises(tmp_path):
    with pytest.raises(FileNotFoundError, match="weights only"):
        _trainer(tmp_path / "nothing", _StubAlgo(), resume=True)
    old = tmp_path / "old"                                 # a run written before full-state checkpoints: weights, no state
    (old / "models" / "2").mkdir(parents=True)
    (old / "resume").mkdir()
    (old / "resume" / "2.pkl.tmp").write_bytes(b"torn")
    with pytest.raises(FileNotFoundError, match="weights only"):
        _trainer(old, _StubAlgo(), resume=True)


# ---- 4. train.py's flag comparison ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_cli():
    spec = importlib.util.spec_from_file_location("train_cli_for_resume_test", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_ARGV = ["--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "1", "--steps", "4", "--n-env-train", "16",
         "--batch-size", "2048", "--lr-lagr", "1e-7"]


def test_resume_flag_is_optional_and_kept_out_of_the_stored_flags(train_cli):
    a = train_cli.build_parser().parse_args(_ARGV)
    assert a.resume is None
    stored = train_cli._flags_to_store(a)
    assert "resume" not in stored and set(stored) == set(vars(a)) - {"resume"}
    assert train_cli.build_parser().parse_args(_ARGV + ["--resume", "some/run"]).resume == "some/run"
    names = [n[-1] for n, _, _ in train_cli.FLAGS]
    assert names[-2:] == ["--gpus", "--resume"]


def test_resume_flag_check(train_cli, tmp_path):
    import yaml
    parse = train_cli.build_parser().parse_args
    stored = yaml.safe_load(yaml.safe_dump(train_cli._flags_to_store(parse(_ARGV + ["--log-dir", "/a", "--name", "first"]))))
    train_cli.check_resume_flags(parse(_ARGV), stored)                                        # identical: accepted
    train_cli.check_resume_flags(parse(_ARGV + ["--resume", "x", "--log-dir", "/b", "--name", "second"]), stored)
    with pytest.raises(SystemExit) as ex:
        train_cli.check_resume_flags(parse(_ARGV[:8] + ["--steps", "5"] + _ARGV[10:] + ["--gpus", "2"]), stored)
    msg = str(ex.value)
    assert "--steps" in msg and "--gpus" in msg and "--seed" not in msg and "--log-dir" not in msg and "--name" not in msg
    with pytest.raises(SystemExit, match="--lr-actor"):
        train_cli.check_resume_flags(parse(_ARGV + ["--lr-actor", "1e-4"]), stored)
    with pytest.raises(SystemExit, match="--no-rnn"):
        train_cli.check_resume_flags(parse(_ARGV + ["--no-rnn"]), stored)
    # through the run directory: accepted, refused with the flags named, refused together with --debug, and a directory
    # without flags.yaml refused like one without state
    run = tmp_path / "run"
    (run / "resume").mkdir(parents=True)
    (run / "resume" / "flags.yaml").write_text(yaml.safe_dump(stored))
    train_cli.check_resume(parse(_ARGV))                                                      # no --resume: nothing to check
    train_cli.check_resume(parse(_ARGV + ["--resume", str(run)]))
    with pytest.raises(SystemExit, match="--seed"):
        train_cli.check_resume(parse(_ARGV + ["--resume", str(run), "--seed", "3"]))
    with pytest.raises(SystemExit, match="--debug"):
        train_cli.check_resume(parse(_ARGV + ["--resume", str(run), "--debug"]))
    with pytest.raises(FileNotFoundError, match="weights only"):
        train_cli.check_resume(parse(_ARGV + ["--resume", str(tmp_path / "old_run")]))
