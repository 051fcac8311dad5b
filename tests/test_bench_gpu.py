"""`bench.py --gpus N` on the GPU box: the self-launched, supervised multi-rank path (two ranks sharing the one GPU over the
gloo data plane — RCCL needs one device per rank and multi-GPU boxes are the driver's), small sizes.  Then one rank: what
a plain run reports and dumps (--dump-outputs), and what --full adds."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *flags, timeout=600):
    env = dict(os.environ, DGPPO_DIST_BACKEND="gloo", **extra_env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DGPPO_RDZV_FILE"):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--n-env", "256", "--batch-size", "4096",
                        "--steps", "1", "--warmup", "1", "--no-cpu-baseline", *flags], capture_output=True, text=True, env=env,
                       timeout=timeout, cwd=ROOT)
    return r, time.time() - t0


def test_two_supervised_ranks_print_one_json_line(cuda):
    r, _ = _run({})
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_envs"] == 512
    assert out["value"] == pytest.approx(2 * 256 * 128 / (out["ms_per_step"] * 1e-3), rel=1e-6)
    assert out["multi_gpu"]["allreduce_selfcheck"] == "passed"
    assert "all-reduce self-check passed" in r.stderr and "multi-GPU diagnostics" in r.stderr


def test_a_rank_that_dies_takes_the_job_down_within_seconds(cuda):
    """DGPPO_BENCH_FAULT_RANK=1: rank 1 exits (code 3) once the communicator is up; rank 0 goes on into its first all-reduce
    and would wait there for its peer.  The supervising parent must stop it and return non-zero with the reason."""
    r, dt = _run({"DGPPO_BENCH_FAULT_RANK": "1"})
    assert r.returncode != 0
    assert "[launch] FAILED" in r.stderr and "(1, 3)" in r.stderr, r.stderr[-3000:]
    assert dt < 240, f"took {dt:.0f} s"            # dominated by two `import torch` + engine construction, not by a timeout


def _run_one(*flags, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DGPPO_RDZV_FILE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n-env", "256", "--batch-size", "4096",
                        *flags], capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_given_steps_and_dumps_the_last_ones_outputs(cuda, tmp_path):
    """a plain run: exactly --steps timed iterations, the headline keys, none of the --full measurements, and the arrays of
    the last timed iteration under --dump-outputs (float32 / float64, <= 64 MB, a seeded sample of the envs)"""
    import numpy as np
    d = tmp_path / "out"
    out = _run_one("--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
    assert out["steps"] == 2 and out["ms_per_step_stats"]["n"] == 2
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] == pytest.approx(256 * 128 / (out["ms_per_step"] * 1e-3), rel=1e-6)
    for k in ("roofline", "cpu_baseline", "rollout_only_env_steps_per_s_per_gpu"):
        assert k not in out
    arrays = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert set(arrays) == set(out["dumped_outputs"]["arrays"])
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["rollout_rewards"].shape == (128, 128) and arrays["det_costs"].shape == (128, 128, 8, 2)
    for name in ("policy_params", "Vl_params", "Vh_params", "rollout_actions", "rollout_log_pis"):
        assert np.isfinite(arrays[name]).all(), name
    assert float(arrays["info_policy_loss"]) == pytest.approx(out["last_info"]["policy/loss"], rel=1e-6)
    # same arguments, same outputs: the last iteration's rollouts bit for bit, its updated parameters up to the order of the
    # gradient sums
    _run_one("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "again"))
    for name, a in arrays.items():
        b = np.load(tmp_path / "again" / f"{name}.npy")
        if name.startswith(("rollout_", "det_")):
            assert np.array_equal(a, b, equal_nan=True), name
        elif name.endswith("_params"):
            assert np.abs(a - b).max() <= 1e-2 * np.abs(a).max(), name


def test_full_run_adds_the_separate_measurements(cuda):
    out = _run_one("--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert out["rollout_only_env_steps_per_s_per_gpu"] > 0
    assert out["roofline"]["us_per_launch"] > 0 and out["roofline"]["at_4x_envs"]["envs"] == 1024
    assert "cpu_baseline" not in out
