#!/usr/bin/env python
"""Drop-in for the reference's test.py (same flags and defaults, test.py:159-189) on the MI355X implementation: load
`{path}/config.yaml` and `{path}/models/{step}/{actor,Vl,Vh}.pkl`, run `--epi` test episodes with the deterministic
(or `--stochastic`) policy, print per-episode reward / cost / safe rate and the aggregate, optionally append
`test_log.csv`.  All episodes run as ONE batched rollout on the GPU (the reference loops over episodes on the host).
Unless `--no-video`, every episode is rendered to `{path}/videos/{step}/` (test.py:150-159; `.gif` when no ffmpeg binary
is available for `.mp4`).  `--landscape AGENT` (not a flag of the reference) also sweeps that agent over a
`--landscape-grid`-squared grid in every frame of every episode, writes the learned constraint values to
`{path}/videos/{step}/{stamp}_{name}_landscape.npz` and draws them as contours in the animation.  `--cost-landscape AGENT`
does the same with the environment's own cost (`{stamp}_{name}_cost.npz`; every algorithm has it); with both flags for the
same agent the animation shows the learned contours with the true zero line dashed, and a line per episode says how much of
the truly unsafe set the net misses.  `--action-landscape AGENT` sweeps that agent's ACTION over the `--landscape-grid`-squared
grid of [-1, 1]^2 in every frame and evaluates the discrete barrier condition the policy is trained under
(`DGPPO.action_landscape`): `{stamp}_{name}_action.npz`, an inset in the animation, and a line per episode saying how much of
the action square the learned barrier admits, in how many frames it admits nothing, and how often the action taken lies
inside.  `--shield` runs the episodes with the learned barrier as a runtime filter (`DGPPO.collect_shielded`): every agent's
action is kept where the barrier admits it and otherwise replaced by the nearest admissible action of a `--shield-grid`-squared
grid of [-1, 1]^2 (`--shield-margin M`: admissible means cbf_deriv <= -M).  Every line and file then describes the shielded
episodes; one more line per episode says how often the shield stepped in, and `{stamp}_{name}_shield.npz` holds its log.
`--rollout-landscape AGENT` measures what the constraint values are trained to predict: from every point of the
`--landscape-grid`-squared grid, in every frame, the deterministic policy is rolled `--rollout-horizon K` steps forward with
that agent displaced there (`DGPPO.rollout_landscape`; every algorithm has it) and the costs it meets are folded as the
training target folds them.  `{stamp}_{name}_rollout.npz` holds the folded value, the worst cost met and the statistics; a
line per episode says how much of the grid is doomed (unsafe within the horizon) and, with `--landscape` / `--cost-landscape`
for the same agent, how much of the doomed set the learned Vh misses and how much of it is still safe now (which the
instantaneous cost cannot show); the animation shows the doomed set's boundary dotted.  With `--shield` the what-if rollouts
follow the UNSHIELDED policy: they say what the policy alone would do from each point, not what the filter would make of it.
`--shield --shield-horizon H` (H >= 1) replaces the learned barrier by a lookahead (`collect_lookahead_shielded`; every
algorithm has it): for the policy's action and every action of the `--shield-grid`-squared grid the environment is forked, the
candidate played and the policy rolled H steps on, and an action is admissible where the agent's own worst cost over those
steps is <= -M (`--shield-margin M`).  The lines, `test_log.csv`, the landscapes and the video then describe those episodes, and
`{stamp}_{name}_shield.npz` holds `policy_action`, `action`, `index`, `flag`, `s` (the worst rolled cost of every candidate),
`us`, `vs`, `margin`, `horizon` and the three statistics.  `--shield-horizon 0` (the default) is the one-step barrier shield.
`--shield-rounds R` (with `--shield --shield-horizon H`, R >= 2) re-judges the picks jointly, up to R rounds per step
(`collect_lookahead_shielded(rounds=R)`): the joint action the agents hold is rolled as everyone's candidate 0, and in every
round after the first one agent per environment may still move.  One more line per episode says for how many steps the joint
action played was rolled and admissible for every agent (joint_verified_frac), for how many it was not rolled because the
rounds ran out (joint_unrolled_frac), and how many rounds a step took (mean_rounds); `{stamp}_{name}_shield.npz` also holds
`joint`, `rounds_used`, `rounds` and the three numbers.  `--shield-rounds 1` (the default) is the shield without rounds.
`--action-rollout-landscape AGENT` measures what the actions `--action-landscape` judges lead to (`action_rollout_landscape`;
every algorithm has it): in every frame that agent plays each action of the `--landscape-grid`-squared grid of [-1, 1]^2 for one
step, everyone else their recorded action, and the deterministic policy is rolled on until the costs of the
`--rollout-horizon K` states after that step are known.  `{stamp}_{name}_action_rollout.npz` holds `us`, `vs`, `value`, `worst`
(every agent's row), `actions`, `agent`, `frames`, `horizon`, `gamma` and the statistics; a line per episode says how much of the
action grid dooms the agent within the horizon, in how many frames the one action decides that, and, with `--action-landscape`
for the same agent, how many of the doomed actions the learned barrier admits (missed_frac) and how many of the others it
rejects (conservative_frac); the animation shows the doomed set's boundary dashed in the action inset.  It works with
`--stochastic` and with either shield; the what-if rollouts follow the deterministic, unshielded policy.
`--scenes FILE` starts the episodes in designed situations instead of at the sampled reset: FILE is a `.npz` of `dgppo.env.Scenes`
(`Scenes.save`; S scenes of this env and team size), episode i runs scene (offset + i) % S and its line names the scene.
`--scene-jitter J` (with `--scenes`, J > 0) moves every agent by up to J off its place in the scene, drawn from the episode's
seed, so that several episodes of one scene differ.  Everything else — both shields, the rounds, every landscape, the video,
`test_log.csv` — describes those episodes as it would the sampled ones.
`--mine-scenes OUT.npz` turns the failures of the episodes into such a file (`algo.mine_scenes`, `Scenes.mine`): for every episode
whose cost reaches 0 at some step >= 1 — the rule of the unsafe marks in the video — the state `--mine-back K` (default 8) steps
earlier becomes the scene `epi{i}_t{t0}_a{agent}`, where it is a valid one; a line per mined episode names the first unsafe step,
the start step, the agent and the cost component.  It works with every other flag (the shields, `--stochastic`, `--scenes`); with
nothing mined a line says so and no file is written.  A mined state restarts with a zero actor carry and a fresh step counter:
the situation is reproduced, not the rest of the episode."""
import argparse
import datetime
import os
import pathlib

import numpy as np

from dgppo.algo import make_algo
from dgppo.env import Scenes, make_env
from dgppo_amd.trainer import evaluate as EV


VMAS_MINE = "--mine-scenes: VMASReverseTransport has no scene entry point"


def mine(args, algo, env, ro):
    """--mine-scenes OUT.npz: the failures of the episodes as a scenes file, by this file's own unsafe rule (a cost >= 0, the rule
    of the `unsafe` array the video marks): for every episode that becomes unsafe at some step >= 1 and whose state --mine-back
    steps earlier is a valid scene, that state.  One line per mined episode, then the count; with nothing mined, no file"""
    back = MINE_BACK_DEFAULT if args.mine_back is None else args.mine_back
    n_cost = int(env.cfg.n_cost)
    scenes = algo.mine_scenes(ro, back=back, thresh=0.0,
                              names=lambda b, first, t0, who: f"epi{args.offset + b}_t{t0}_a{who // n_cost}")
    if scenes is None:
        print(f"mined scenes: none (no episode became unsafe after its first step from a valid state); {args.mine_scenes} not written")
        return None
    m = scenes.mined
    for b, first, t0, who in zip(m["env"], m["first"], m["t0"], m["who"]):
        print(f"epi: {b}, mined: first unsafe at step {first}, scene starts at step {t0}, agent {who // n_cost}, "
              f"cost {env.cost_components[who % n_cost]}")
    scenes.save(args.mine_scenes)
    print(f"mined scenes: {scenes.S} of {ro.actions.shape[0]} episodes -> {args.mine_scenes}")
    return scenes


def test(args):
    print(f"> Running test.py {args}")
    np.random.seed(args.seed)
    config = EV.load_config(os.path.join(args.path, "config.yaml"))
    if args.mine_scenes is not None and (config.env if args.env is None else args.env) == "VMASReverseTransport":
        raise SystemExit(VMAS_MINE)
    num_agents = config.num_agents if args.num_agents is None else args.num_agents
    env = make_env(env_id=config.env if args.env is None else args.env, num_agents=num_agents,
                   num_obs=config.obs if args.obs is None else args.obs, max_step=args.max_step,
                   full_observation=args.full_observation)
    model_path = os.path.join(args.path, "models")
    step = EV.latest_step(model_path) if args.step is None else args.step
    print("step: ", step)
    algo = make_algo(
        algo=config.algo, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
        action_dim=env.action_dim, n_agents=env.num_agents, cost_weight=config.cost_weight,
        actor_gnn_layers=config.actor_gnn_layers, Vl_gnn_layers=config.Vl_gnn_layers,
        Vh_gnn_layers=getattr(config, "Vh_gnn_layers", 1), lr_actor=config.lr_actor, lr_Vl=config.lr_Vl, max_grad_norm=2.0,
        seed=config.seed, use_rnn=config.use_rnn, rnn_layers=config.rnn_layers, use_lstm=config.use_lstm,
        alpha=getattr(config, "alpha", 10.0))
    algo.load(model_path, step)

    # episode seeds: the reference takes jr.split(PRNGKey(seed), 1000)[:epi][offset:] (test.py:90-93); RNG streams are not
    # comparable across libraries (threefry vs Philox), the structure (1000 draws, prefix, offset) is kept
    keys = np.random.default_rng([args.seed, 13]).integers(1, 2 ** 62, size=1000)[:args.epi][args.offset:]
    if len(keys) == 0:
        raise SystemExit("no episodes to run (--epi / --offset)")
    shield_log = None
    where, scene_of = {}, None                  # --scenes: the start of every collect call below, and the scene name per episode
    if args.scenes is not None:
        scenes = Scenes.load(args.scenes, env)
        ids = (args.offset + np.arange(len(keys))) % scenes.S
        where = dict(scenes=scenes, scene_ids=ids, jitter=args.scene_jitter)
        scene_of = [scenes.names[s] for s in ids]
    if args.shield and args.shield_horizon >= 1:
        ro, shield_log = algo.collect_lookahead_shielded(keys, env=env, grid=args.shield_grid, margin=args.shield_margin,
                                                         horizon=args.shield_horizon,
                                                         **({"rounds": args.shield_rounds} if args.shield_rounds > 1 else {}),
                                                         **where)
    elif args.shield:
        ro, shield_log = algo.collect_shielded(keys, env=env, grid=args.shield_grid, margin=args.shield_margin, **where)
    elif args.stochastic:
        ro = algo.collect_stochastic(keys, env=env, **where)
    else:
        ro = algo.collect_deterministic(keys, env=env, **where)
    stats = EV.episode_stats(ro.rewards.cpu().numpy(), ro.costs.cpu().numpy())
    for i in range(len(keys)):
        scene = "" if scene_of is None else f"scene: {scene_of[i]}, "
        print(f"epi: {i}, {scene}reward: {stats['reward'][i]:.3f}, cost: {stats['cost'][i]:.3f}, "
              f"safe rate: {stats['safe_rate'][i] * 100:.3f}%")
    agg = EV.aggregate(stats)
    print(f"reward: {agg['reward']:.3f}, min/max reward: {agg['reward_min']:.3f}/{agg['reward_max']:.3f}, "
          f"cost: {agg['cost']:.3f}, min/max cost: {agg['cost_min']:.3f}/{agg['cost_max']:.3f}, "
          f"safe_rate: {agg['safe_mean'] * 100:.3f}%")
    if shield_log is not None:
        sh = EV.shield_stats(shield_log)
        for i in range(len(keys)):
            print(f"epi: {i}, shield: stepped in for {sh['intervention_frac'][i] * 100:.3f}% of the actions (intervention_frac), "
                  f"found nothing admissible for {sh['infeasible_frac'][i] * 100:.3f}% (infeasible_frac), moved the action by "
                  f"{sh['mean_deviation'][i]:.4f} on average (mean_deviation)")
    joint = None
    if shield_log is not None and args.shield_rounds > 1:
        joint = EV.joint_shield_stats(shield_log)
        for i in range(len(keys)):
            print(f"epi: {i}, shield rounds: the joint action played was rolled and admissible for every agent in "
                  f"{joint['joint_verified_frac'][i] * 100:.3f}% of the steps (joint_verified_frac), not rolled in "
                  f"{joint['joint_unrolled_frac'][i] * 100:.3f}% (joint_unrolled_frac), {joint['mean_rounds'][i]:.3f} rounds per "
                  f"step (mean_rounds)")
    if args.mine_scenes is not None:
        mine(args, algo, env, ro)
    if args.log:
        with open(os.path.join(args.path, "test_log.csv"), "a") as f:
            f.write(EV.csv_line(env, args.epi, agg))
    if (not args.no_video or args.landscape is not None or args.cost_landscape is not None or args.action_landscape is not None
            or args.rollout_landscape is not None or shield_log is not None or args.action_rollout_landscape is not None):
        videos_dir = pathlib.Path(args.path) / "videos" / f"{step}"
        videos_dir.mkdir(exist_ok=True, parents=True)
        stamp = datetime.datetime.now().strftime("%m%d-%H%M")
        unsafe = (ro.costs >= 0.0).any(dim=-1).cpu().numpy()          # [B, T, n]  (test.py:103-105)
        for i in range(len(keys)):
            name = (f"n{num_agents}_epi{i:02}_reward{stats['reward'][i]:.3f}_cost{stats['cost'][i]:.3f}"
                    f"_sr{stats['safe_rate'][i] * 100:.0f}")
            extra = {}
            if shield_log is not None:
                out = videos_dir / f"{stamp}_{name}_shield.npz"
                if args.shield_horizon >= 1:
                    per_epi = {k: getattr(shield_log, k)[i] for k in ("policy_action", "action", "index", "flag", "s")}
                    if joint is not None:
                        per_epi.update(joint=shield_log.joint[i], rounds_used=shield_log.rounds_used[i],
                                       rounds=shield_log.rounds, **{k: v[i] for k, v in joint.items()})
                    np.savez(out, us=shield_log.us, vs=shield_log.vs, margin=shield_log.margin, horizon=shield_log.horizon,
                             **per_epi, **{k: v[i] for k, v in sh.items()})
                else:
                    per_epi = {k: getattr(shield_log, k)[i] for k in ("policy_action", "action", "index", "flag", "h", "Vh")}
                    np.savez(out, us=shield_log.us, vs=shield_log.vs, margin=shield_log.margin, alpha=shield_log.alpha,
                             dt=shield_log.dt, **per_epi, **{k: v[i] for k, v in sh.items()})
                print(f"shield: {out}")
            if args.landscape is not None:
                land = algo.vh_landscape(ro, i, args.landscape, nx=args.landscape_grid, ny=args.landscape_grid)
                out = videos_dir / f"{stamp}_{name}_landscape.npz"
                np.savez(out, xs=land.xs, ys=land.ys, Vh=land.Vh, agent=land.agent, frames=land.frames)
                print(f"landscape: {out}")
                extra["landscape"] = land
            if args.cost_landscape is not None:
                cost = algo.cost_landscape(ro, i, args.cost_landscape, nx=args.landscape_grid, ny=args.landscape_grid)
                more = {}
                if args.landscape == args.cost_landscape:
                    more = EV.landscape_agreement(extra["landscape"], cost)
                    print(f"epi: {i}, agent {cost.agent}: the learned Vh misses {more['missed_frac'] * 100:.3f}% of the truly "
                          f"unsafe points (missed_frac), calls {more['conservative_frac'] * 100:.3f}% of the safe ones unsafe "
                          f"(conservative_frac)")
                out = videos_dir / f"{stamp}_{name}_cost.npz"
                np.savez(out, xs=cost.xs, ys=cost.ys, cost=cost.cost, agent=cost.agent, frames=cost.frames, **more)
                print(f"cost landscape: {out}")
                extra["cost_landscape"] = cost
            if args.action_landscape is not None:
                A = algo.action_landscape(ro, i, args.action_landscape, nu=args.landscape_grid, nv=args.landscape_grid)
                adm = EV.action_admissibility(A)
                print(f"epi: {i}, agent {A.agent}: the learned barrier admits {adm['admissible_frac'] * 100:.3f}% of the action "
                      f"grid (admissible_frac), nothing in {adm['empty_frac'] * 100:.3f}% of the frames (empty_frac), the action "
                      f"taken in {adm['taken_admitted_frac'] * 100:.3f}% of them (taken_admitted_frac)")
                out = videos_dir / f"{stamp}_{name}_action.npz"
                np.savez(out, us=A.us, vs=A.vs, cbf=A.cbf, Vh_next=A.Vh_next, Vh=A.Vh, actions=A.actions, agent=A.agent,
                         frames=A.frames, alpha=A.alpha, dt=A.dt, **adm)
                print(f"action landscape: {out}")
                extra["action_landscape"] = A
            if args.rollout_landscape is not None:
                rl = algo.rollout_landscape(ro, i, args.rollout_landscape, nx=args.landscape_grid, ny=args.landscape_grid,
                                            horizon=args.rollout_horizon)
                same = lambda key, flag: extra.get(key) if flag == args.rollout_landscape else None
                agree = EV.rollout_agreement(rl, land=same("landscape", args.landscape),
                                             cost=same("cost_landscape", args.cost_landscape))
                line = (f"epi: {i}, agent {rl.agent}: within {rl.horizon} steps the policy becomes unsafe from "
                        f"{agree['doomed_frac'] * 100:.3f}% of the grid (doomed_frac)")
                if "missed_frac" in agree:
                    line += (f", the learned Vh misses {agree['missed_frac'] * 100:.3f}% of those points (missed_frac), calls "
                             f"{agree['conservative_frac'] * 100:.3f}% of the others unsafe (conservative_frac) and is "
                             f"{agree['value_error']:.4f} off the measured return on average (value_error)")
                if "latent_frac" in agree:
                    line += f", {agree['latent_frac'] * 100:.3f}% of the points safe now are doomed (latent_frac)"
                print(line)
                out = videos_dir / f"{stamp}_{name}_rollout.npz"
                np.savez(out, xs=rl.xs, ys=rl.ys, value=rl.value, worst=rl.worst, agent=rl.agent, frames=rl.frames,
                         horizon=rl.horizon, gamma=rl.gamma, **agree)
                print(f"rollout landscape: {out}")
                extra["rollout_landscape"] = rl
            if args.action_rollout_landscape is not None:
                R = algo.action_rollout_landscape(ro, i, args.action_rollout_landscape, nu=args.landscape_grid,
                                                  nv=args.landscape_grid, horizon=args.rollout_horizon)
                A = extra.get("action_landscape") if args.action_landscape == args.action_rollout_landscape else None
                agree = EV.action_rollout_agreement(R, A)
                line = (f"epi: {i}, agent {R.agent}: {agree['doomed_frac'] * 100:.3f}% of the action grid dooms the agent within "
                        f"{R.horizon} steps (doomed_frac), everything in {agree['empty_frac'] * 100:.3f}% of the frames "
                        f"(empty_frac), the one action decides it in {agree['decisive_frac'] * 100:.3f}% of them (decisive_frac)")
                if "others_doomed_frac" in agree:
                    line += (f", {agree['others_doomed_frac'] * 100:.3f}% of the grid dooms another agent (others_doomed_frac, "
                             f"decisive in {agree['others_decisive_frac'] * 100:.3f}% of the frames: others_decisive_frac)")
                if "missed_frac" in agree:
                    line += (f", the learned barrier admits {agree['missed_frac'] * 100:.3f}% of the doomed actions (missed_frac) "
                             f"and rejects {agree['conservative_frac'] * 100:.3f}% of the others (conservative_frac)")
                print(line)
                out = videos_dir / f"{stamp}_{name}_action_rollout.npz"
                np.savez(out, **R._asdict(), **agree)
                print(f"action rollout landscape: {out}")
                extra["action_rollout_landscape"] = R
            if args.no_video:
                continue
            out = env.render_video(ro, videos_dir / f"{stamp}_{name}.mp4", unsafe[i], {}, dpi=args.dpi, index=i, **extra)
            print(f"video: {out}")
    return agg


# the reference's flags (test.py:159-189): (names, kind, default); kind is a type name or "flag"
FLAGS = [
    (("--path",), "req:str", None), (("--no-video",), "flag", False), (("--epi",), "int", 5), (("--step",), "int", None),
    (("--obs",), "int", None), (("--stochastic",), "flag", False), (("--full-observation",), "flag", False),
    (("--debug",), "flag", False), (("--cpu",), "flag", False), (("--max-step",), "int", None), (("--log",), "flag", False),
    (("-n", "--num-agents"), "int", None), (("--seed",), "int", 1234), (("--env",), "str", None), (("--offset",), "int", 0),
    (("--dpi",), "int", 100),
    # not the reference's flags: the Vh landscape of one agent (DGPPO.vh_landscape) over an N x N grid, per episode
    (("--landscape",), "int", None), (("--landscape-grid",), "int", 64),
]
# the true-cost landscape of one agent (DGPPO.cost_landscape) over the --landscape-grid grid, per episode
COST_FLAGS = [(("--cost-landscape",), "int", None)]
# the barrier condition over one agent's actions (DGPPO.action_landscape), --landscape-grid squared, per episode
ACTION_FLAGS = [(("--action-landscape",), "int", None)]
# the learned barrier as a runtime filter on every agent's action (DGPPO.collect_shielded): an N x N grid of replacement actions,
# admissible where cbf_deriv <= -M
SHIELD_FLAGS = [(("--shield",), "flag", False), (("--shield-grid",), "int", 8), (("--shield-margin",), "float", 0.0)]
# what Vh is trained to predict, measured (DGPPO.rollout_landscape): the policy rolled K steps forward from every point of the
# --landscape-grid grid with one agent displaced there, per episode
ROLLOUT_FLAGS = [(("--rollout-landscape",), "int", None), (("--rollout-horizon",), "int", 32)]
# with --shield: filter by forked policy rollouts of H steps instead of the learned barrier (collect_lookahead_shielded; every
# algorithm has it); 0: the one-step barrier shield
LOOKAHEAD_FLAGS = [(("--shield-horizon",), "int", 0)]
# what one agent's actions lead to, measured (action_rollout_landscape; every algorithm has it): each action of the
# --landscape-grid grid played for one step, then the policy rolled until --rollout-horizon further costs are known, per episode
ACTION_ROLLOUT_FLAGS = [(("--action-rollout-landscape",), "int", None)]
# with --shield --shield-horizon H: re-judge the picks jointly, up to R rounds per step, one mover per round after the first
# (collect_lookahead_shielded(rounds=R)); 1: the shield without rounds
ROUNDS_FLAGS = [(("--shield-rounds",), "int", 1)]
# start the episodes in the scenes of a dgppo.env.Scenes file instead of at the sampled reset (episode i: scene (offset + i) % S);
# --scene-jitter J moves every agent by up to J off its place, drawn from the episode's seed
SCENE_FLAGS = [(("--scenes",), "str", None), (("--scene-jitter",), "float", 0.0)]
# write the failures of these episodes as a dgppo.env.Scenes file: for every episode that becomes unsafe at some step >= 1, the state
# --mine-back steps earlier (Scenes.mine); every flag that takes --scenes then works on OUT.npz
MINE_FLAGS = [(("--mine-scenes",), "str", None), (("--mine-back",), "int", None)]
MINE_BACK_DEFAULT = 8


def build_parser() -> argparse.ArgumentParser:
    types = {"int": int, "str": str, "float": float}
    ap = argparse.ArgumentParser(description=__doc__)
    for names, kind, default in (FLAGS + COST_FLAGS + ACTION_FLAGS + SHIELD_FLAGS + ROLLOUT_FLAGS + LOOKAHEAD_FLAGS
                                 + ACTION_ROLLOUT_FLAGS + ROUNDS_FLAGS + SCENE_FLAGS + MINE_FLAGS):
        if kind == "flag":
            ap.add_argument(*names, action="store_true", default=False)
        elif kind.startswith("req:"):
            ap.add_argument(*names, type=types[kind[4:]], required=True)
        else:
            ap.add_argument(*names, type=types[kind], default=default)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.cpu:
        raise SystemExit("--cpu: this build has no CPU product path (the HIP library is required)")
    if args.shield and args.stochastic:
        raise SystemExit("--shield --stochastic: the shield filters the deterministic policy; drop one of the two flags")
    if args.shield_horizon < 0:
        raise SystemExit(f"--shield-horizon must be >= 0 (got {args.shield_horizon})")
    if args.shield_horizon >= 1 and not args.shield:
        raise SystemExit("--shield-horizon needs --shield: it sets how far the shield looks ahead")
    if args.shield_rounds < 1:
        raise SystemExit(f"--shield-rounds must be >= 1 (got {args.shield_rounds})")
    if args.shield_rounds > 1 and not (args.shield and args.shield_horizon >= 1):
        raise SystemExit("--shield-rounds needs --shield and --shield-horizon >= 1: the rounds re-judge the lookahead shield's picks")
    if not args.scene_jitter >= 0.0:
        raise SystemExit(f"--scene-jitter must be >= 0 (got {args.scene_jitter})")
    if args.scene_jitter > 0.0 and args.scenes is None:
        raise SystemExit("--scene-jitter needs --scenes: it moves the agents off their places in the given scenes")
    if args.mine_back is not None and args.mine_scenes is None:
        raise SystemExit("--mine-back needs --mine-scenes: it says how many steps before a failure the mined scene starts")
    if args.mine_back is not None and args.mine_back < 0:
        raise SystemExit(f"--mine-back must be >= 0 (got {args.mine_back})")
    if args.mine_scenes is not None and args.env == "VMASReverseTransport":
        raise SystemExit(VMAS_MINE)
    return test(args)


if __name__ == "__main__":
    main()
