#!/usr/bin/env python
"""Training entry point of the MI355X build.  The command line is the reference's (train.py:133-182): every flag keeps
its name, type and default so that existing launch scripts work unchanged; the flag table below is the single source of
truth for them."""
import argparse
import datetime
import os

import numpy as np
import yaml

from dgppo.algo import make_algo
from dgppo.env import Scenes, make_env
from dgppo.trainer.trainer import Trainer, no_state_error, scene_count
from dgppo.trainer.utils import is_connected

# (flags, kind, default)   kind: a type -> typed option, "flag" -> store_true, "req:<type>" -> required option
_T = {"int": int, "float": float, "str": str}
FLAGS = [
    (("--env",), "req:str", None), (("-n", "--num-agents"), "req:int", None), (("--algo",), "req:str", None),
    (("--obs",), "req:int", None),
    (("--seed",), "int", 0), (("--steps",), "int", 200000), (("--name",), "str", None), (("--debug",), "flag", False),
    (("--cost-weight",), "float", 0.0), (("--n-rays",), "int", 32), (("--full-observation",), "flag", False),
    (("--clip-eps",), "float", 0.25), (("--lagr-init",), "float", 0.5), (("--lr-lagr",), "float", 1e-7),
    (("--cbf-weight",), "float", 1.0), (("--cbf-eps",), "float", 1e-2), (("--alpha",), "float", 10.0),
    (("--no-cbf-schedule",), "flag", False), (("--cost-schedule",), "flag", False), (("--no-rnn",), "flag", False),
    (("--actor-gnn-layers",), "int", 2), (("--Vl-gnn-layers",), "int", 2), (("--Vh-gnn-layers",), "int", 1),
    (("--lr-actor",), "float", 3e-4), (("--lr-Vl",), "float", 1e-3), (("--lr-Vh",), "float", 1e-3),
    (("--rnn-layers",), "int", 1), (("--use-lstm",), "flag", False), (("--coef-ent",), "float", 1e-2),
    (("--rnn-step",), "int", 16), (("--n-env-train",), "int", 128), (("--batch-size",), "int", 16384),
    (("--n-env-test",), "int", 32), (("--log-dir",), "str", "./logs"), (("--eval-interval",), "int", 50),
    (("--eval-epi",), "int", 1), (("--save-interval",), "int", 50),
    # not in the reference: a device-resident pool of M scenes mined from the policy's own recent failures (the state --mine-back
    # steps before a rollout's first unsafe step); the share --scene-frac of every batch starts there, the scenes of --scenes FILE
    # are pinned in its first slots (README "Mining failure scenes")
    (("--mine-scenes",), "int", 0), (("--mine-back",), "int", 8),
    # not in the reference: the pool by priority: slots are drawn in proportion to 4 s (1 - s) of their failure score s and to their
    # staleness, empty slots never, and a push evicts solved and hopeless slots instead of the oldest (README "Mining failure scenes")
    # (--mine-priority is the same flag under the family name of the pool's other flags)
    (("--scene-priority", "--mine-priority"), "flag", False),
    # not in the reference: a share P of every training batch starts in the designed scenes of FILE (env.Scenes.save), moved by
    # up to J, the rest at the sampled reset; every evaluation also rolls each scene once (README "Training on scenes")
    (("--scenes",), "str", None), (("--scene-frac",), "float", 0.0), (("--scene-jitter",), "float", 0.0),
    # not in the reference (it is single-device): data-parallel training, one process per GPU
    (("--gpus",), "int", 1),
    # continue the stopped run in RUN_DIR from its newest full-state checkpoint; every other flag as in the stopped run
    (("--resume",), "str", None),
]
# flags a resumed run may give differently: where it logs and what it is called play no part in the computation
_RESUME_FREE = ("resume", "log_dir", "name", "debug")
# flags newer than full-state checkpoints: a stopped run that does not record them ran without them, at their defaults
_RESUME_LATER = ("scenes", "scene_frac", "scene_jitter", "mine_scenes", "mine_back", "scene_priority")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__)
    for names, kind, default in FLAGS:
        if kind == "flag":
            ap.add_argument(*names, action="store_true", default=False)
        elif kind.startswith("req:"):
            ap.add_argument(*names, type=_T[kind[4:]], required=True)
        else:
            ap.add_argument(*names, type=_T[kind], default=default)
    return ap


def _long(names) -> str:
    """the flag's first long name: what argparse derives the attribute from, and what messages call it"""
    return next(n for n in names if n.startswith("--"))


def _dest(names) -> str:
    return _long(names).lstrip("-").replace("-", "_")


def _flags_to_store(a) -> dict:
    """what config.yaml and resume/flags.yaml record of the command line: everything but --resume"""
    return {k: v for k, v in vars(a).items() if k != "resume"}


def check_resume_flags(a, stored: dict) -> None:
    """the shares, the minibatch order and the schedules depend on the flags (--gpus and --steps included), so a resumed run
    must repeat those of the stopped one (`stored`: its resume/flags.yaml).  SystemExit naming every flag that differs."""
    diff = []
    for names, _, default in FLAGS:
        k = _dest(names)
        if k in _RESUME_FREE:
            continue
        if k in _RESUME_LATER:
            stored = {k: default, **stored}
        if k not in stored:
            diff.append(f"{_long(names)} (not recorded by the stopped run)")
        elif stored[k] != getattr(a, k):
            diff.append(f"{_long(names)} ({stored[k]!r} in the stopped run, {getattr(a, k)!r} now)")
    if diff:
        raise SystemExit("train.py --resume: these flags differ from the stopped run's: " + ", ".join(diff))


def check_resume(a) -> None:
    """needs no GPU: called before any rank is started"""
    if a.resume is None:
        return
    if a.debug:
        raise SystemExit("train.py: --resume cannot be combined with --debug (a debug run writes nothing)")
    path = os.path.join(a.resume, "resume", "flags.yaml")
    if not os.path.isfile(path):
        raise no_state_error(a.resume)
    with open(path) as f:
        check_resume_flags(a, yaml.safe_load(f) or {})


def check_mining(a) -> None:
    """--mine-scenes / --mine-back; needs no GPU.  SystemExit naming the flag at fault"""
    if a.mine_scenes == 0:
        if a.scene_priority:
            raise SystemExit("train.py: --scene-priority needs --mine-scenes: it is a mode of the pool of mined scenes")
        if a.mine_back != 8:
            raise SystemExit("train.py: --mine-back needs --mine-scenes: it says how many steps before a failure the mined scene starts")
        return
    if a.mine_scenes < 1:
        raise SystemExit(f"train.py: --mine-scenes must be >= 1, the capacity of the pool (got {a.mine_scenes})")
    if a.mine_back < 0:
        raise SystemExit(f"train.py: --mine-back must be >= 0 (got {a.mine_back})")
    if a.scene_priority and a.mine_scenes > 65536:
        raise SystemExit(f"train.py: --scene-priority takes a pool of at most 65536 scenes (got --mine-scenes {a.mine_scenes})")
    if a.scene_frac == 0.0:
        raise SystemExit("train.py: --mine-scenes needs --scene-frac: the share of every batch that starts in the pool")
    if a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("train.py: --mine-scenes runs on one rank (--gpus 1, no launcher): every rank would keep a pool of its own "
                         "failures, and the ranks' windows together would no longer be what one device runs (DESIGN.md §9)")
    if a.scenes is not None and os.path.isfile(a.scenes):
        from dgppo_amd.env.scenes import check_pool, read_npz
        try:
            check_pool(a.mine_scenes, read_npz(a.scenes)["agent"].shape[0])
        except ValueError as ex:
            raise SystemExit(f"train.py: --mine-scenes: {ex}")


def check_scenes(a) -> None:
    """needs no GPU: called before any rank is started.  SystemExit naming the flag at fault"""
    check_mining(a)
    if a.scenes is None and a.mine_scenes == 0:
        for flag, v in (("--scene-frac", a.scene_frac), ("--scene-jitter", a.scene_jitter)):
            if v != 0.0:
                raise SystemExit(f"train.py: {flag} needs --scenes FILE, or --mine-scenes M for a pool of mined scenes")
        return
    if not 0.0 < a.scene_frac <= 1.0:
        raise SystemExit(f"train.py: --scene-frac must be in (0, 1] with --scenes / --mine-scenes (got {a.scene_frac})")
    if not a.scene_jitter >= 0.0:
        raise SystemExit(f"train.py: --scene-jitter must be >= 0 (got {a.scene_jitter})")
    if a.env == "VMASReverseTransport":
        raise SystemExit(f"train.py: {'--scenes' if a.scenes is not None else '--mine-scenes'}: VMASReverseTransport has no scene "
                         f"entry point")
    few = f"train.py: --scene-frac {a.scene_frac} of --n-env-train {a.n_env_train} is less than one environment"
    if a.scenes is None:                             # a pool of mined scenes alone: no file to look at
        if scene_count(a.scene_frac, a.n_env_train) < 1:
            raise SystemExit(few)
        return
    if not os.path.isfile(a.scenes):
        raise SystemExit(f"train.py: --scenes {a.scenes}: no such file")
    from dgppo_amd.env.scenes import check_file
    try:
        check_file(a.scenes, a.env, a.num_agents)
    except ValueError as ex:
        raise SystemExit(f"train.py: --scenes: {ex}")
    if scene_count(a.scene_frac, a.n_env_train) < 1:
        raise SystemExit(few)


def _unique_run_dir(root: str, seed: int):
    """{root}/seed{seed}_{MMDDhhmmss}_{4 random capitals}, bumped until it does not exist (train.py:81-93)."""
    tag = "".join(chr(c) for c in np.random.default_rng().integers(65, 91, size=4))
    stamp = int(datetime.datetime.now().strftime("%m%d%H%M%S"))
    while os.path.exists(f"{root}/seed{seed}_{stamp}_{tag}"):
        stamp += 1
    return f"{root}/seed{seed}_{stamp}_{tag}", stamp, tag


def _algo_kwargs(a, env, world: int = 1) -> dict:
    """what the reference hands to make_algo (train.py:44-77); --batch-size is the GLOBAL minibatch, a rank trains on its
    1/world share of it"""
    return dict(
        algo=a.algo, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
        action_dim=env.action_dim, n_agents=env.num_agents, seed=a.seed, train_steps=a.steps, batch_size=a.batch_size // world,
        gamma=0.99, max_grad_norm=2.0, clip_eps=a.clip_eps, coef_ent=a.coef_ent,
        actor_gnn_layers=a.actor_gnn_layers, Vl_gnn_layers=a.Vl_gnn_layers, Vh_gnn_layers=a.Vh_gnn_layers,
        lr_actor=a.lr_actor, lr_Vl=a.lr_Vl, lr_Vh=a.lr_Vh,
        use_rnn=not a.no_rnn, rnn_layers=a.rnn_layers, rnn_step=a.rnn_step, use_lstm=a.use_lstm,
        alpha=a.alpha, cbf_eps=a.cbf_eps, cbf_weight=a.cbf_weight, cbf_schedule=not a.no_cbf_schedule,
        cost_weight=a.cost_weight, cost_schedule=a.cost_schedule, lagr_init=a.lagr_init, lr_lagr=a.lr_lagr)


def _setup_ranks(a):
    """-> (rank, world, allreduce, close).  `--gpus N` under `python -m torch.distributed.run --nproc-per-node N` (or any
    launcher that sets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*) uses that environment; a bare `python train.py --gpus N` has
    started its own supervised ranks in main() before getting here.  Each rank binds to GPU LOCAL_RANK, joins the gloo
    control plane and the RCCL communicator of the C ABI, and proves the all-reduce with a known-answer check."""
    import torch
    from dgppo_amd import dist as D
    rank, local_rank, world = D.env_info()
    if world != a.gpus:
        raise SystemExit(f"train.py: --gpus {a.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    if world == 1:
        return 0, 1, None, (lambda: None)
    backend = os.environ.get("DGPPO_DIST_BACKEND", "rccl")
    n_dev = torch.cuda.device_count()
    if world > n_dev and backend != "gloo":
        raise SystemExit(f"train.py: {world} ranks but {n_dev} GPU(s) visible (DGPPO_DIST_BACKEND=gloo rehearses several "
                         f"ranks on one GPU)")
    assert a.n_env_train % world == 0 and a.batch_size % world == 0, "--n-env-train and --batch-size must be multiples of --gpus"
    torch.cuda.set_device(local_rank % max(n_dev, 1))
    D.init_control_plane()
    allreduce, close = D.make_allreduce(world, backend)
    D.selfcheck_allreduce(allreduce, rank, world, torch.device("cuda", torch.cuda.current_device()))
    if rank == 0:
        print(f"> data-parallel: {world} ranks, data plane {backend} (RCCL version {D.rccl_version()}), "
              f"{a.n_env_train // world} envs and a minibatch share of {a.batch_size // world} per rank", flush=True)

    def close_all():
        close()
        D.shutdown(world)
    return rank, world, allreduce, close_all


def train(a):
    rank, world, allreduce, close = _setup_ranks(a)
    if rank == 0:
        print(f"> Running train.py {a}")
    np.random.seed(a.seed)
    if a.debug or rank != 0:
        os.environ["WANDB_MODE"] = "disabled"
    elif not is_connected():
        os.environ["WANDB_MODE"] = "offline"

    def new_env():
        return make_env(env_id=a.env, num_agents=a.num_agents, num_obs=a.obs, n_rays=a.n_rays,
                        full_observation=a.full_observation)

    env, env_test = new_env(), new_env()
    algo = make_algo(**_algo_kwargs(a, env, world), allreduce=allreduce, world=world, rank=rank)
    scenes = None if a.scenes is None else Scenes.load(a.scenes, env)

    root = f"{a.log_dir}/{a.env}/{a.algo}"
    write = not a.debug and rank == 0                # one writer (rank 0); the other ranks never touch the log directory
    if write:
        os.makedirs(root, exist_ok=True)
    if a.resume is not None:                         # the stopped run's directory, nothing new beside it
        log_dir = a.resume
        run_name = f"{a.algo}_{os.path.basename(os.path.normpath(log_dir))}"
    else:
        log_dir, stamp, tag = _unique_run_dir(root, a.seed)
        run_name = f"{a.algo}_seed{a.seed:03}_{stamp}_{tag}"
        if a.name is not None:
            run_name = f"{run_name}_{a.name}_seed{a.seed:03}_{stamp}_{tag}"
    schedule = {"run_name": run_name, "training_steps": a.steps, "eval_interval": a.eval_interval, "eval_epi": a.eval_epi,
                "save_interval": a.save_interval}
    trainer = Trainer(env=env, env_test=env_test, algo=algo, gamma=0.99, log_dir=log_dir, n_env_train=a.n_env_train,
                      n_env_test=a.n_env_test, seed=a.seed, params=schedule, save_log=write, rank=rank, world=world,
                      resume=a.resume is not None, scenes=scenes, scene_frac=a.scene_frac, scene_jitter=a.scene_jitter,
                      **({} if a.mine_scenes == 0 else {"mine_scenes": a.mine_scenes, "mine_back": a.mine_back}),
                      **({"scene_priority": True} if a.scene_priority else {}))
    if write and a.resume is None:   # plain mappings (the reference dumps the argparse.Namespace object itself; test.py reads both)
        with open(f"{log_dir}/config.yaml", "w") as f:
            yaml.safe_dump(_flags_to_store(a), f)
            yaml.safe_dump(algo.config, f)
        # the flags alone, for --resume to compare with: config.yaml is one mapping in which algo.config's keys win
        with open(f"{trainer.resume_dir}/flags.yaml", "w") as f:
            yaml.safe_dump(_flags_to_store(a), f)
    trainer.train()
    close()


def main(argv=None):
    import sys
    argv = sys.argv[1:] if argv is None else list(argv)
    a = build_parser().parse_args(argv)
    check_resume(a)
    check_scenes(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher environment: start the ranks ourselves, before this process touches the GPU, and supervise them
        # (per-rank logs, everything stops on the first failure — dgppo_amd/launch.py)
        from dgppo_amd import launch
        here = os.path.dirname(os.path.abspath(__file__))
        sys.exit(launch.spawn_ranks(os.path.abspath(__file__), argv, a.gpus, launch.default_log_dir(here),
                                    stall_seconds=float(os.environ.get("DGPPO_STALL_SECONDS", "900"))))
    train(a)


if __name__ == "__main__":
    main()
