"""Start scenes on the device: dgppo_env_scene_load against the NumPy restatement (tests/scenes_np.py) word for word, then through
Engine.rollout against oracle/env_np.py, through Engine.rollout_lookahead_shielded on the committed head-on scene against what
tests/lookahead_rounds_np.py derives by the oracle alone, and through test.py --scenes in-process."""
import ctypes as C
import glob
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
import lookahead_rounds_np as R  # noqa: E402
import scenes_np as SN  # noqa: E402
from test_lookahead_shield_gpu import _engine, _load_test_py, _record_words, _run_dir, _same_words  # noqa: E402
from test_scenes_cpu import GOLDEN, retry_case, stuck_case  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
f32 = np.float32
TRIG_WORDS = [5, 6] + list(range(8, 16))         # of a rectangle record: device cosf / sinf and what is formed from them
TRIG_ATOL = 1e-6                                  # what tests/test_env_gpu.py allows the same words of the reset kernel
SENT = -7


def _cfg(kind_name, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(N.ENV_KINDS[kind_name], n, n_obs)


def _d(x, cuda, dtype=f32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).to(cuda)


def _words(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _templates(cfg, S, seed):
    """S random scenes inside the default area: positions in [0.1, 1.4], velocities, headings and widths of any sign that fits"""
    rng = np.random.default_rng(seed)
    n, ng, no, sd = cfg.n_agents, cfg.n_goals, cfg.n_obs, cfg.state_dim
    agent = rng.uniform(-0.5, 0.5, size=(S, n, sd)).astype(f32)
    agent[..., :2] = rng.uniform(0.1, 1.4, size=(S, n, 2))
    goal = np.zeros((S, ng, sd), f32)
    goal[..., :2] = rng.uniform(0.1, 1.4, size=(S, ng, 2))
    obst = None
    if no > 0 and cfg.is_lidar:
        obst = np.concatenate([rng.uniform(0.1, 1.4, size=(S, no, 2)), rng.uniform(0.1, 0.3, size=(S, no, 2)),
                               rng.uniform(-np.pi, np.pi, size=(S, no, 1))], axis=-1).astype(f32)
    elif no > 0:
        obst = rng.uniform(0.1, 1.4, size=(S, no, 2)).astype(f32)
    return agent, goal, obst


def _load(cuda, cfg, agent_t, goal_t, obst_t, ids, seeds, jitter, B, want_flags=True, n_failed0=0):
    """OE.scene_load into buffers prefilled with NaN / a sentinel -> (State, flags [B] or None, n_failed)"""
    from dgppo_amd import ops_env as OE
    st = OE.State.empty(cfg, B, cuda)
    for v in list(st.step.values()) + list(st.env.values()):
        v.fill_(float("nan"))
    flags = torch.full((B,), SENT, dtype=torch.int32, device=cuda) if want_flags else None
    n_failed = torch.full((1,), n_failed0, dtype=torch.int32, device=cuda)
    rows = {"agent": _d(agent_t, cuda), "goal": _d(goal_t, cuda)}
    if obst_t is not None:
        rows["obst"] = _d(obst_t, cuda)
    OE.scene_load(cfg, rows, ids, _d(seeds, cuda, np.int64), jitter, st, flags, n_failed)
    torch.cuda.synchronize()
    return st, None if flags is None else flags.cpu().numpy(), int(n_failed.item())


def _check(cfg, st, flags, n_failed, want, name, n_failed0=0):
    """every output word against the restatement: bit-exact, but for the trig words of rectangle records (TRIG_ATOL)"""
    np.testing.assert_array_equal(_words(st.agent), want["agent"].view(np.uint32), err_msg=f"{name}: agent")
    np.testing.assert_array_equal(_words(st.goal), want["goal"].view(np.uint32), err_msg=f"{name}: goal")
    if cfg.n_obs > 0:
        got = st.obst.cpu().numpy()
        if cfg.is_lidar:
            exact = [w for w in range(16) if w not in TRIG_WORDS]
            np.testing.assert_array_equal(got[..., exact].view(np.uint32), want["obst"][..., exact].view(np.uint32), err_msg=f"{name}: rect")
            err = np.abs(got[..., TRIG_WORDS].astype(np.float64) - want["obst"][..., TRIG_WORDS])
            assert np.isnan(err).sum() == 0 and float(err.max()) <= TRIG_ATOL, f"{name}: rect trig words off by {err.max():.3e}"
        else:
            np.testing.assert_array_equal(got.view(np.uint32), want["obst"].view(np.uint32), err_msg=f"{name}: disc rows")
    else:
        assert st.obst is None
    if flags is not None:
        np.testing.assert_array_equal(flags, want["flags"], err_msg=f"{name}: flags")
    assert n_failed == n_failed0 + want["n_failed"], f"{name}: n_failed {n_failed}"


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------------
SHAPES = [("LidarSpread", n, no) for n in (1, 2, 3) for no in (0, 1, 3)] + [("LidarBicycleTarget", 2, 1), ("MPESpread", 2, 2),
                                                                             ("LidarLine", 2, 1), ("MPEFormation", 3, 1)]


@pytest.mark.parametrize("kind,n,n_obs", SHAPES, ids=["-".join(map(str, c)) for c in SHAPES])
def test_load_equals_the_restatement(cuda, kind, n, n_obs):
    """S = 1 and S = 3 at B = 5 (the default ids wrap; an explicit list repeats a scene) and S = 3 at B = 65 (a second block and
    its tail); without jitter and seeds, and with a jitter of 0.02; with and without the flags output.  Random scenes: some are
    invalid, which is part of what is compared"""
    cfg = _cfg(kind, n, n_obs)
    assert (cfg.state_dim, cfg.n_goals) == {"LidarBicycleTarget": (5, 2), "LidarLine": (4, 2), "MPEFormation": (4, 1)}.get(kind, (4, n))
    seen = 0
    for S, B, ids in ((1, 5, None), (3, 5, None), (3, 5, [2, 2, 0, 1, 2]), (3, 65, None)):
        agent_t, goal_t, obst_t = _templates(cfg, S, 100 * n + 10 * n_obs + S)
        seeds = (np.arange(1, B + 1, dtype=np.int64) * 104729) + S
        for jitter, sd in ((0.0, None), (0.02, seeds)):
            name = f"{kind} {n}/{n_obs} S={S} B={B} ids={ids} jitter={jitter}"
            want = SN.scene_load_np(cfg, agent_t, goal_t, obst_t, ids, sd, jitter, B)
            st, flags, n_failed = _load(cuda, cfg, agent_t, goal_t, obst_t, ids, sd, jitter, B, n_failed0=3)
            _check(cfg, st, flags, n_failed, want, name, n_failed0=3)
            assert jitter > 0 or n_failed == 3, "without jitter the counter is the caller's"
            seen |= int(np.bitwise_or.reduce(want["flags"]))
            if B == 5:
                st2, none, _ = _load(cuda, cfg, agent_t, goal_t, obst_t, ids, sd, jitter, B, want_flags=False)
                assert none is None
                for k, v in {**st.step, **st.env}.items():
                    np.testing.assert_array_equal(_words(v), _words(getattr(st2, k)), err_msg=f"{name}: {k} without flags")
    print(f"{kind} {n}/{n_obs}: validity bits met {seen:#x}")


def test_nan_payload_and_each_bit_in_one_env(cuda):
    """LidarSpread 2 / 1, five scenes at B = 5: scene 1 has an agent outside the area, scene 2 overlapping agents, scene 3 an agent
    in the rectangle, scene 4 a NaN with a payload in a goal row — copied as it is; scene 0 and every neighbour's flag stay 0"""
    cfg = _cfg("LidarSpread", 2, 1)
    agent = np.tile(np.array([[[0.3, 0.3, 0.1, 0.0], [0.6, 1.2, 0.0, -0.1]]], f32), (5, 1, 1))
    goal = np.zeros((5, 2, 4), f32)
    goal[:, :, :2] = [[1.2, 1.2], [0.2, 0.9]]
    rect = np.tile(np.array([[[1.0, 0.5, 0.2, 0.4, 0.3]]], f32), (5, 1, 1))
    agent[1, 1, 0] = 1.6
    agent[2, 1, :2] = [0.36, 0.37]
    agent[3, 0, :2] = [1.0, 0.5]
    goal.view(np.uint32)[4, 1, 2] = 0x7FC12345
    want = SN.scene_load_np(cfg, agent, goal, rect, None, None, 0.0, 5)
    assert want["flags"].tolist() == [0, SN.OUT_OF_AREA, SN.AGENTS_OVERLAP, SN.AGENT_IN_OBSTACLE, SN.NONFINITE]
    st, flags, n_failed = _load(cuda, cfg, agent, goal, rect, None, None, 0.0, 5, n_failed0=7)
    _check(cfg, st, flags, n_failed, want, "bits", n_failed0=7)
    assert n_failed == 7, "an invalid scene without jitter is written and flagged, not counted"
    assert int(_words(st.goal)[4, 1, 2]) == 0x7FC12345
    # the same scenes in another order: the flags follow the scene, not the env
    ids = [3, 0, 4, 0, 1]
    st, flags, _ = _load(cuda, cfg, agent, goal, rect, ids, None, 0.0, 5)
    assert flags.tolist() == [SN.AGENT_IN_OBSTACLE, 0, SN.NONFINITE, 0, SN.OUT_OF_AREA]
    # MPE: inside a disc
    mpe = _cfg("MPESpread", 2, 2)
    a = np.array([[[0.3, 0.3, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]] * 3, f32)
    disc = np.array([[[0.3, 0.42], [0.9, 0.2]], [[0.3, 0.39], [0.9, 0.2]], [[0.3, 0.42], [0.9, 0.2]]], f32)
    want = SN.scene_load_np(mpe, a, np.zeros((3, 2, 4), f32), disc, None, None, 0.0, 3)
    assert want["flags"].tolist() == [0, SN.AGENT_IN_OBSTACLE, 0]
    st, flags, n_failed = _load(cuda, mpe, a, np.zeros((3, 2, 4), f32), disc, None, None, 0.0, 3)
    _check(mpe, st, flags, n_failed, want, "disc")


def test_jitter_retries(cuda):
    """the two retry cases of the CPU file: flags and n_failed equal the restatement's for every env, and so does every agent word
    — the attempts' positions all differ, so equal words mean the same attempt was kept"""
    cfg, agent, goal, rect, seeds, J = retry_case()
    want = SN.scene_load_np(cfg, agent, goal, rect, None, seeds, J, len(seeds))
    assert want["attempt"].max() >= 1 and want["n_failed"] == 0
    st, flags, n_failed = _load(cuda, cfg, agent, goal, rect, None, seeds, J, len(seeds))
    _check(cfg, st, flags, n_failed, want, "coincident agents")
    assert flags.tolist() == [0] * len(seeds)
    print(f"coincident agents: attempts kept {want['attempt'].tolist()}")
    cfg, agent, goal, rect, seeds, J = stuck_case()
    want = SN.scene_load_np(cfg, agent, goal, rect, None, seeds, J, len(seeds))
    assert want["attempt"].tolist() == [SN.ATTEMPTS - 1] * len(seeds) and want["n_failed"] == len(seeds)
    st, flags, n_failed = _load(cuda, cfg, agent, goal, rect, None, seeds, J, len(seeds), n_failed0=2)
    _check(cfg, st, flags, n_failed, want, "inside a rectangle", n_failed0=2)
    assert flags.tolist() == [SN.AGENT_IN_OBSTACLE] * len(seeds) and n_failed == 2 + len(seeds)
    st, none, n_failed = _load(cuda, cfg, agent, goal, rect, None, seeds, J, len(seeds), want_flags=False)
    assert n_failed == len(seeds), "counted without a flags output, too"


def test_host_refusals_launch_nothing(cuda):
    """every refusal of the entry point returns non-zero and leaves the outputs as they were"""
    from dgppo_amd import _native as N
    lib = N.lib()
    cfg = _cfg("LidarSpread", 2, 1)
    agent_t, goal_t, obst_t = _templates(cfg, 1, 5)
    B = 4
    t = dict(agent_t=_d(agent_t, cuda), goal_t=_d(goal_t, cuda), obst_t=_d(obst_t, cuda),
             seeds=torch.arange(1, B + 1, dtype=torch.int64, device=cuda), agent=torch.full((B, 2, 4), float("nan"), device=cuda),
             goal=torch.full((B, 2, 4), float("nan"), device=cuda), obst=torch.full((B, 1, 16), float("nan"), device=cuda),
             flags=torch.full((B,), SENT, dtype=torch.int32, device=cuda), n_failed=torch.full((1,), SENT, dtype=torch.int32, device=cuda))
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}

    def call(cfg=cfg, S=1, jitter=0.0, B=B, **over):
        q = {**p, **over}
        return lib.dgppo_env_scene_load(C.byref(cfg), q["agent_t"], q["goal_t"], q["obst_t"], S, None, q["seeds"], jitter, q["agent"],
                                        q["goal"], q["obst"], q["flags"], q["n_failed"], B, N.stream_ptr())
    bad_cfg = _cfg("LidarSpread", 2, 1)
    bad_cfg.kind = 17
    for kw in (dict(cfg=bad_cfg), dict(cfg=N.make_env_cfg(N.VMAS_REVERSE_TRANSPORT, 2, 0)), dict(S=0), dict(S=-3), dict(B=-1),
               dict(jitter=-0.1), dict(jitter=float("nan")), dict(agent_t=None), dict(goal_t=None), dict(agent=None), dict(goal=None),
               dict(obst_t=None), dict(obst=None), dict(cfg=_cfg("LidarSpread", 2, 0)), dict(cfg=_cfg("LidarSpread", 2, 0), obst_t=None),
               dict(jitter=0.1, seeds=None), dict(cfg=_cfg("LidarSpread", 65, 1))):
        assert call(**kw) != 0, kw
        assert lib.dgppo_last_error(), kw
    torch.cuda.synchronize()
    for k in ("agent", "goal", "obst"):
        assert bool(torch.isnan(t[k]).all()), f"{k} was written by a refused call"
    assert t["flags"].tolist() == [SENT] * B and t["n_failed"].tolist() == [SENT]
    assert call() == 0                                      # and the call they were all one step away from
    torch.cuda.synchronize()
    assert not bool(torch.isnan(t["agent"]).any()) and t["n_failed"].tolist() == [SENT] and SENT not in t["flags"].tolist()


# ---- 2. through the engine ----------------------------------------------------------------------------------------------------------------
def _scenes(name, kind, n, n_obs):
    from dgppo.env import Scenes, make_env
    env = make_env(kind, n, num_obs=n_obs)
    return Scenes.load(os.path.join(GOLDEN, name), env)


def test_scenes_class_on_the_device(cuda, tmp_path):
    """load, the validation's ValueError naming scene and bits, save -> load word for word"""
    from dgppo.env import Scenes, make_env
    sc = _scenes("lidarspread_n2_lookahead.npz", "LidarSpread", 2, 1)
    assert sc.S == 2 and sc.names == ["mover0", "mover1"] and sorted(sc.dev) == ["agent", "goal", "obst"]
    sc.save(tmp_path / "again.npz")
    env = make_env("LidarSpread", 2, num_obs=1)
    again = Scenes.load(tmp_path / "again.npz", env)
    for k in sc.dev:
        _same_words(again.dev[k], sc.dev[k], k)
    agent = sc.rows["agent"].copy()
    agent[1, 0, :2] = [0.68, 0.75]                            # the middle of the square
    agent[1, 1, 0] = -0.2
    with pytest.raises(ValueError, match=r"mover1 \(#1\): OUT_OF_AREA \| AGENT_IN_OBSTACLE"):
        Scenes(env, agent, sc.rows["goal"], rect=sc.rows["obst"], names=sc.names)
    with pytest.raises(ValueError, match="the env is LidarSpread with 3"):
        Scenes.load(tmp_path / "again.npz", make_env("LidarSpread", 3, num_obs=1))
    mpe = _scenes("mpespread_n3_swap_wall.npz", "MPESpread", 3, 2)
    assert mpe.obst_key == "disc" and tuple(mpe.dev["obst"].shape) == (2, 2, 2)


def test_engine_rollout_from_scenes_follows_the_oracle(cuda):
    """Engine.rollout(seeds, False, start=...) at T = 4 on the lookahead fixture, B = 3 (scenes 0, 1, 0): slot 0 is the loaded scene
    with the hits ops_env.sense gives it; from there every step is oracle/env_np.py's on the device's own action (rewards, costs,
    next states and hits bit for bit) and the action the oracle policy's within 1e-5: the rules of tests/test_rollout_oracle_gpu.py.
    start=None is the call without the argument, word for word"""
    from dgppo_amd import ops_env as OE
    from test_engine_gpu import _np_rollout, _setup
    B, T_ = 3, 4
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 2, 1, B, T_, cuda, 16, 4)
    sc = _scenes("lidarspread_n2_lookahead.npz", "LidarSpread", 2, 1)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 104729
    ro = eng.rollout(seeds, False, start=sc.start()).finalize()
    torch.cuda.synchronize()
    assert int(eng.reset_failed.item()) == 0
    r = _np_rollout(ro)
    want = SN.scene_load_np(cfg, sc.rows["agent"], sc.rows["goal"], sc.rows["obst"], None, None, 0.0, B)
    st = OE.State({"agent": _d(want["agent"], cuda)}, {"goal": _d(want["goal"], cuda), "obst": _d(want["obst"], cuda)})
    OE.sense(cfg, st)
    np.testing.assert_array_equal(r["agent"][:, 0].view(np.uint32), want["agent"].view(np.uint32))
    np.testing.assert_array_equal(r["goal"].view(np.uint32), want["goal"].view(np.uint32))
    np.testing.assert_array_equal(r["obst"].view(np.uint32), want["obst"].view(np.uint32))    # theta = 0: cos and sin are exact
    np.testing.assert_array_equal(np.ascontiguousarray(r["hits"][:, 0]).view(np.uint32), _words(st.hits))
    tab = E.ray_table(32)
    hits0, _ = E.lidar_sense(ocfg, want["agent"][..., :2], want["obst"], *tab)
    np.testing.assert_array_equal(np.ascontiguousarray(r["hits"][:, 0]).view(np.uint32), hits0.view(np.uint32))
    h = torch.zeros(B, 2, 64)
    for t in range(T_):
        g = T.graph_to_torch(E.get_graph(ocfg, r["agent"][:, t], r["goal"], r["obst"], r["hits"][:, t]))
        with torch.no_grad():
            a, h = T.policy_mode(trees["policy"], g, h, 2)
        np.testing.assert_allclose(r["actions"][:, t], a.numpy(), atol=1e-5)
        np.testing.assert_allclose(r["rnn_states"][:, t], h.numpy(), atol=1e-5)
        out = E.env_step(ocfg, r["agent"][:, t], r["goal"], r["obst"], r["hits"][:, t], r["actions"][:, t], tab)
        np.testing.assert_array_equal(r["rewards"][:, t], out["reward"])
        np.testing.assert_array_equal(r["costs"][:, t], out["cost"])
        np.testing.assert_array_equal(r["agent"][:, t + 1], out["next_agent"])
        np.testing.assert_array_equal(r["hits"][:, t + 1], out["next_hits"])
    assert not np.array_equal(r["agent"][0], r["agent"][1]) and np.array_equal(r["agent"][0], r["agent"][2]), "scenes 0, 1, 0"
    # an explicit list and a jitter: slot 0 is the restatement's
    ids = np.array([1, 1, 0])
    rj = _np_rollout(eng.rollout(seeds, False, start=sc.start(ids, 0.01)).finalize())
    wj = SN.scene_load_np(cfg, sc.rows["agent"], sc.rows["goal"], sc.rows["obst"], ids, seeds.cpu().numpy(), 0.01, B)
    np.testing.assert_array_equal(rj["agent"][:, 0].view(np.uint32), wj["agent"].view(np.uint32))
    assert wj["flags"].tolist() == [0, 0, 0] and int(eng.reset_failed.item()) == 0
    # start=None: today's path
    a, b = eng.rollout(seeds, False).finalize(), None
    ra = {k: v.clone() for k, v in _record_words(a).items()}
    b = eng.rollout(seeds, False, start=None).finalize()
    for k, v in _record_words(b).items():
        _same_words(v, ra[k], f"start=None: {k}")


def test_failed_scene_loads_land_in_reset_failed(cuda):
    """Scenes() refuses an invalid scene outright, so a load can only fail under jitter.  The engine reads nothing of a start but
    its device rows: the CPU file's stuck case (an agent deep inside a square, jitter 1e-3) goes in as bare rows, every env fails,
    and the engine counts them where it counts failed resets"""
    import types
    from dgppo.env import Scenes, SceneStart, make_env
    from test_engine_gpu import _setup
    cfg, agent, goal, rect, seeds, J = retry_case()
    with pytest.raises(ValueError, match=r"scene0 \(#0\): AGENTS_OVERLAP"):
        Scenes(make_env("LidarSpread", 2, num_obs=0), agent, goal)
    cfg, agent, goal, rect, seeds, J = stuck_case()
    with pytest.raises(ValueError, match=r"scene0 \(#0\): AGENT_IN_OBSTACLE"):
        Scenes(make_env("LidarSpread", 2, num_obs=1), agent, goal, rect=rect)
    _, _, _, eng, _ = _setup("LidarSpread", 2, 1, 4, 2, cuda, 16, 2)
    rows = types.SimpleNamespace(dev=dict(agent=_d(agent, cuda), goal=_d(goal, cuda), obst=_d(rect, cuda)))
    sd = torch.from_numpy(seeds[:4]).to(cuda)
    assert int(eng.reset_failed.item()) == 0
    eng.rollout(sd, False, start=SceneStart(rows, None, J))
    assert int(eng.reset_failed.item()) == 4
    eng.reset_failed.zero_()
    eng.rollout(sd, False, start=SceneStart(rows, None, 0.0))          # without jitter the caller decides: nothing is counted
    assert int(eng.reset_failed.item()) == 0


def test_hip_graph_engine_equals_the_eager_one(cuda, monkeypatch):
    """an engine built under DGPPO_HIPGRAPH=0 and a default one with use_graphs: torch.equal records on the first call (eager
    launches and the capture) and the second (the replay), deterministic and stochastic; the scene load runs outside the captured
    region, so a second call with other scenes replays onto them"""
    from dgppo_amd import engine as EN
    from test_engine_gpu import _setup
    B, T_ = 3, 4
    monkeypatch.setenv("DGPPO_HIPGRAPH", "0")
    cfg, ocfg, hp, eng_e, trees = _setup("LidarSpread", 2, 1, B, T_, cuda, 16, 4, use_graphs=True)
    monkeypatch.delenv("DGPPO_HIPGRAPH")
    eng_g = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=True)
    assert not eng_e.use_graphs and eng_g.use_graphs
    for k, net in eng_g.nets.items():
        net.load_tree(trees[k])
    sc = _scenes("lidarspread_n2_lookahead.npz", "LidarSpread", 2, 1)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    for call, ids in enumerate((None, [1, 0, 1])):
        for stochastic in (False, True):
            a = eng_e.rollout(seeds, stochastic, noise_seed=3 + call, start=sc.start(ids, 0.005)).finalize()
            b = eng_g.rollout(seeds, stochastic, noise_seed=3 + call, start=sc.start(ids, 0.005)).finalize()
            for name in ("agent", "hits", "goal", "obst", "actions", "log_pis", "rnn_states", "rewards", "costs"):
                x, y = getattr(a, name), getattr(b, name)
                if x is None:
                    assert y is None
                    continue
                assert torch.equal(x, y), f"call {call} stochastic={stochastic}: {name} differs"
    assert eng_g._ro_cache[(B, True)]["graph"] is not None and eng_g._ro_cache[(B, False)]["calls"] == 2


# ---- 3. the point of it all: the head-on scene through the lookahead shield --------------------------------------------------------------
def test_headon_scene_through_the_lookahead_shield(cuda):
    """LidarSpread 2 / 1 with zeroed policy parameters (its action is exactly 0), the committed head-on scene, the 3 x 3 grid,
    horizon 12.  Step 0 with rounds = 4 gives what lookahead_rounds_np derives by the oracle alone: the joint action was rolled
    and is admissible (joint == 2) after three rounds, agent 0 holds on (index 5: the grid's (0, 0)), agent 1 dodges down (index
    2), and both own-row folds are SCENE_A_SAFE.  With rounds = 1 both dodge down: index (2, 2)"""
    H, us, vs = R.SCENE_A_H, R.SCENE_A_US, R.SCENE_A_VS
    zero = np.zeros((1, 2, 2), f32)
    want4 = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 4)
    want1 = R.rounds_np(R.scene_a_fold(), zero, us, vs, 0.0, 1)
    assert want4["index"].tolist() == [[5, 2]] and want4["joint"].tolist() == [2] and want1["index"].tolist() == [[2, 2]]
    cfg, eng = _engine("LidarSpread", 2, 1, 2, cuda)
    eng.policy.params.zero_()
    eng.policy.prepare()
    sc = _scenes("lidarspread_n2_headon.npz", "LidarSpread", 2, 1)
    seeds = torch.tensor([5], dtype=torch.int64, device=cuda)
    ro, log = eng.rollout_lookahead_shielded(seeds, us, vs, H, rounds=4, start=sc.start())
    torch.cuda.synchronize()
    _, agent, goal, obst = R.scene_a()
    np.testing.assert_array_equal(_words(ro.states_tm[0].agent), agent.view(np.uint32))
    np.testing.assert_array_equal(_words(ro.states_tm[0].obst), obst.view(np.uint32))
    assert bool((log["policy_action"][0] == 0).all()), "zero parameters give the zero action"
    assert log["joint"][0].tolist() == want4["joint"].tolist() == [2]
    assert log["index"][0].tolist() == want4["index"].tolist() and log["flag"][0].tolist() == want4["flag"].tolist()
    assert log["rounds_used"][0].tolist() == want4["rounds_used"].tolist() == [3]
    s = log["s"][0].cpu().numpy()
    print(f"rounds 4: s bit-equal to the oracle's: {np.array_equal(s, want4['s'])}; own-row folds {s[0, :, 0].tolist()}")
    assert s[0, :, 0].tolist() == [R.SCENE_A_SAFE, R.SCENE_A_SAFE]
    np.testing.assert_array_equal(_words(ro.action_tm[0]), want4["action"].view(np.uint32))
    ro1, log1 = eng.rollout_lookahead_shielded(seeds, us, vs, H, rounds=1, start=sc.start())
    assert log1["index"][0].tolist() == [[2, 2]] and log1["flag"][0].tolist() == want1["flag"].tolist()
    np.testing.assert_array_equal(_words(ro1.action_tm[0]), want1["action"].view(np.uint32))


# ---- 4. test.py --scenes, in-process ------------------------------------------------------------------------------------------------------
def test_cli_runs_the_shield_on_scenes(cuda, tmp_path, capsys):
    n, Tn = 2, 3
    run = _run_dir(tmp_path, "dgppo", n, Tn)
    mod = _load_test_py()
    common = ["--path", str(run), "--no-video", "--max-step", str(Tn), "--shield", "--shield-horizon", "4", "--shield-rounds", "2",
              "--shield-grid", "2"]
    mod.main(common + ["--epi", "2", "--scenes", os.path.join(GOLDEN, "lidarspread_n2_headon.npz")])
    printed = capsys.readouterr().out
    assert "epi: 0, scene: headon, reward" in printed and "epi: 1, scene: headon, reward" in printed
    assert printed.count("scene: headon") == 2 and printed.count("joint_verified_frac") == 2
    files = sorted(glob.glob(str(run / "videos" / "0" / "*_shield.npz")))
    assert len(files) >= 1                                    # both episodes are the same scene: same name, one file or two
    z = np.load(files[0])
    assert z["policy_action"].shape == (Tn, n, 2) and int(z["horizon"]) == 4 and int(z["rounds"]) == 2
    # two scenes, an offset: episode 0 of the run is scene (1 + 0) % 2
    mod.main(common + ["--epi", "2", "--offset", "1", "--scenes", os.path.join(GOLDEN, "lidarspread_n2_lookahead.npz"),
                       "--scene-jitter", "0.01"])
    printed = capsys.readouterr().out
    assert "epi: 0, scene: mover1, reward" in printed and "mover0" not in printed
    mod.main(["--path", str(run), "--no-video", "--max-step", str(Tn), "--epi", "3", "--scenes",
              os.path.join(GOLDEN, "lidarspread_n2_lookahead.npz")])
    printed = capsys.readouterr().out
    assert [ln.split(",")[1].strip() for ln in printed.splitlines() if ln.startswith("epi: ")] == ["scene: mover0", "scene: mover1",
                                                                                                   "scene: mover0"]
    with pytest.raises(ValueError, match="scenes of MPESpread"):
        mod.main(["--path", str(run), "--no-video", "--scenes", os.path.join(GOLDEN, "mpespread_n3_swap_wall.npz")])
