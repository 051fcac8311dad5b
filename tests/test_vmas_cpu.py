"""VMASReverseTransport without a GPU: known answers that pin the NumPy restatement (tests/vmas_np.py), the make_env surface
and the host-side checks of the C ABI."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vmas_np as V  # noqa: E402

f32 = np.float32


def _far_scene(B=1):
    """goal and obstacles far from a box at the origin"""
    return np.tile(np.array([0.4, 0.0, -0.6, 0.6, 0.6, 0.6, -0.6, -0.6], f32), (B, 1))


def test_free_flight_matches_closed_form_with_drag():
    a = np.zeros((1, 1, 4), f32)
    a[0, 0, 2:] = (0.05, -0.02)
    body = np.zeros((1, 4), f32)
    for act in ((0.6, -0.4), (3.0, -2.0)):                       # the second is clipped to (1, -1)
        na, nb, contact = V.physics(a, body, np.array([[act]], f32))
        assert not contact.any()
        u = 0.5 * np.clip(np.array(act), -1, 1)
        p, v = np.zeros(2), np.array([0.05, -0.02])
        for _ in range(4):                                       # vel *= 0.75 at the first of 5 substeps of dt 0.02
            v = v * 0.75
            for _ in range(5):
                v = v + u * 0.02
                p = p + v * 0.02
        np.testing.assert_allclose(na[0, 0, :2], p, atol=2e-7)
        np.testing.assert_allclose(na[0, 0, 2:], v, atol=2e-7)
        assert np.array_equal(nb, body)                          # nothing touches the box


def test_wall_contact_pushes_agent_in_and_box_out():
    px, py = f32(0.3 - 0.03), f32(0.01)                          # 0.03 from the right side, inside the margin 0.0367
    fx, fy, on = V.contact_force(np.array([px]), np.array([py]), np.array([f32(0)]), np.array([f32(0)]))
    # pushed inward along -x; the y component is the fp32 quirk cos(fp32(pi/2)) != 0 of the side direction, ~1e-8 of fx
    assert on[0] and fx[0] < 0 and abs(fy[0]) < 1e-7 * abs(fx[0])
    a = np.array([[[px, py, 0, 0]]], f32)
    body = np.zeros((1, 4), f32)
    na, nb, contact = V.physics(a, body, np.zeros((1, 1, 2), f32))
    assert contact[0] and na[0, 0, 2] < 0 and nb[0, 2] > 0
    # equal and opposite forces, masses 1 and 10, drag on both: the total momentum stays zero
    assert abs(float(na[0, 0, 2]) + 10 * float(nb[0, 2])) < 1e-6 and abs(float(nb[0, 3])) < 1e-7
    # far from every side: no force
    fx, fy, on = V.contact_force(np.array([f32(0.1)]), np.array([f32(0.1)]), np.array([f32(0)]), np.array([f32(0)]))
    assert not on[0] and fx[0] == 0 and fy[0] == 0


def test_cost_and_reward_known_answers():
    body = np.zeros((1, 4), f32)
    scene = _far_scene()
    scene[0, 2:4] = (0.1, 0.0)                                   # obstacle 0 at 0.1 from the box centre
    agent = np.zeros((1, 3, 4), f32)
    agent[0, 0, :2], agent[0, 1, :2], agent[0, 2, :2] = (0.0, 0.0), (0.05, 0.0), (-0.2, 0.2)
    m = V.cost_margins(agent, body, scene)
    np.testing.assert_allclose(m[0, :, 0], [4 * (0.06 - 0.05), 4 * (0.06 - 0.05), 4 * (0.06 - np.hypot(0.2, 0.2))], atol=1e-6)
    np.testing.assert_allclose(m[0, :, 1], 2 * (0.15 - 0.1), atol=1e-6)
    c = V.get_cost(agent, body, scene)
    np.testing.assert_allclose(c[0, :2, 0], 0.04 + 0.5, atol=1e-6)            # positive margin: + 0.5
    assert c[0, 2, 0] == -1.0                                                  # 4 (0.06 - 0.283) - 0.5 < -1: clipped
    np.testing.assert_allclose(c[0, :, 1], 0.1 + 0.5, atol=1e-6)
    # one agent: the eye term (1e6) drives the agent column to -1
    c1 = V.get_cost(agent[:, :1], body, scene)
    assert c1.shape == (1, 1, 2) and c1[0, 0, 0] == -1.0
    # reward: -0.01 |goal - box| - 0.001 [|goal - box| > 0.01]
    scene[0, :2] = (0.3, 0.4)
    np.testing.assert_allclose(V.get_reward(body, scene), [-0.005 - 0.001], atol=1e-8)
    scene[0, :2] = (0.003, 0.004)
    np.testing.assert_allclose(V.get_reward(body, scene), [-0.00005], atol=1e-9)


def test_node_feature_columns_flag_and_stable_obstacle_order():
    # dyadic coordinates: obstacles 0 and 1 tie exactly at 0.5 from the box, obstacle 2 is nearest at 0.375
    body = np.array([[0.125, -0.25, 0.3, -0.4]], f32)
    scene = np.array([[0.5, 0.5, 0.125, 0.25, 0.125, -0.75, 0.5, -0.25]], f32)
    agent = np.array([[[0.125 + 0.595, -0.25, 0.01, 0.02], [0.125 + 0.585, -0.25 - 0.1, -0.01, 0.0]]], f32)
    X = V.node_feats(agent, body, scene)
    assert X.shape == (1, 2, 20)
    np.testing.assert_array_equal(X[0, :, 0:4], agent[0])
    np.testing.assert_array_equal(X[0, :, 4:8], np.tile(body, (2, 1)))
    np.testing.assert_array_equal(X[0, 0, 8:10], [0.375, 0.75])
    assert X[0, 0, 10] == 1.0 and X[0, 1, 10] == 0.0                         # |a - box| > 0.59 on some axis
    d = np.sqrt(np.array([0.25, 0.25, 0.140625]) + 1e-6)
    np.testing.assert_allclose(X[0, 0, 17:20], [d[2], d[0], d[1]], rtol=1e-6)   # obstacle 2 first, then the tie in index order
    np.testing.assert_allclose(X[0, 0, 11:13], np.array([0.375, 0.0]) / d[2], rtol=1e-6)
    np.testing.assert_allclose(X[0, 0, 13:15], np.array([0.0, 0.5]) / d[0], rtol=1e-6)
    np.testing.assert_allclose(X[0, 0, 15:17], np.array([0.0, -0.5]) / d[1], rtol=1e-6)
    np.testing.assert_array_equal(X[0, 1, 11:], X[0, 0, 11:])               # the obstacle columns are per env


@pytest.mark.parametrize("n", [1, 3, 5])
def test_graph_shapes_and_pad_routing(n):
    rng = np.random.default_rng(n)
    agent = rng.uniform(-0.3, 0.3, (2, n, 4)).astype(f32)
    body = rng.uniform(-0.1, 0.1, (2, 4)).astype(f32)
    g = V.get_graph(agent, body, _far_scene(2))
    assert g["nodes"].shape == (2, n + 1, 20) and g["edges"].shape == (2, n * n, 4) and g["states"].shape == (2, n + 1, 0)
    assert (g["n_node"] == n + 1).all() and (g["n_edge"] == n * n).all()
    assert (g["node_type"][:, :n] == 0).all() and (g["node_type"][:, n] == -1).all() and (g["nodes"][:, n] == 0).all()
    for i in range(n):
        for j in range(n):
            e = i * n + j
            want = (n, n) if i == j else (i, j)
            assert (g["receivers"][0, e], g["senders"][0, e]) == want
            np.testing.assert_array_equal(g["edges"][:, e], agent[:, i] - agent[:, j])


def test_reset_restatement_places_agents_in_the_box():
    agent, body, scene, failed = V.reset(np.arange(1, 9) * 7919, 4)
    assert failed == 0
    rel = agent[..., :2] - body[:, None, :2]
    assert (rel > -0.2 - 1e-6).all() and (rel < 0.04 + 1e-6).all()
    d = np.linalg.norm(agent[:, :, None, :2] - agent[:, None, :, :2], axis=-1) + np.eye(4) * 9
    assert (d > 0.06).all()
    np.testing.assert_allclose(np.linalg.norm(body[:, :2], axis=-1), 0.49, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(scene[:, :2], axis=-1), 0.49, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(scene[:, 2:].reshape(-1, 3, 2), axis=-1), 0.49 - 0.225, atol=1e-6)
    assert (np.abs(agent[..., 2:]) <= 0.01).all() and (body[:, 2:] == 0).all()


def test_make_env_attributes():
    from dgppo_amd.env import make_env, VMASReverseTransport
    env = make_env("VMASReverseTransport", 3, num_obs=0)
    assert isinstance(env, VMASReverseTransport)
    assert env.area_size == pytest.approx(1.6) and env.dt == pytest.approx(0.03) and env.max_episode_steps == 128
    assert (env.node_dim, env.edge_dim, env.state_dim, env.action_dim, env.n_cost) == (20, 4, 4, 2, 2)
    assert env.cost_components == ("agent collisions", "obstacle collisions")
    assert env.params["n_obs"] == 0 and env.n_obs == 3 and env.params["agent_radius"] == 0.03
    lo, hi = env.action_lim()
    assert lo.tolist() == [-1, -1] and hi.tolist() == [1, 1]
    assert env.cfg.num_nodes == 4 and env.cfg.num_edges == 9 and env.cfg.fan_in == 3


def test_vmas_wheel_still_raises():
    from dgppo_amd.env import make_env
    with pytest.raises(NotImplementedError):
        make_env("VMASWheel", 3)


def _declared():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names.update(m.group(1) for m in re.finditer(r"\b(dgppo_[a-z0-9_]+)\s*\(", src))
    return names


def test_abi_declares_exports_and_guards_the_vmas_kind():
    from dgppo_amd import _native as N
    lib = N.lib()
    new = {"dgppo_vmas_reset_checked", "dgppo_vmas_step", "dgppo_vmas_graph_materialize", "dgppo_vmas_graph_feats"}
    assert new <= _declared() and all(hasattr(lib, s) for s in new)
    lib.dgppo_env_num_nodes.restype = C.c_int32
    lib.dgppo_env_num_edges.restype = C.c_int32
    for n in (1, 3, 16):
        cfg = N.make_env_cfg(N.ENV_KINDS["VMASReverseTransport"], n, 3)
        assert lib.dgppo_env_num_nodes(C.byref(cfg)) == n + 1 and lib.dgppo_env_num_edges(C.byref(cfg)) == n * n
    cfg = N.make_env_cfg(10, 3, 0)
    z = [None] * 16
    # the entry points of the other kinds refuse the VMAS record and name the one to use
    assert lib.dgppo_env_step(C.byref(cfg), *z[:11], None, C.c_int32(4), None) == -1
    assert b"dgppo_vmas_step" in lib.dgppo_last_error()
    assert lib.dgppo_graph_materialize(C.byref(cfg), *z[:5], C.c_int32(4), None) == -1
    assert b"dgppo_vmas_graph_materialize" in lib.dgppo_last_error()
    assert lib.dgppo_env_reset(C.byref(cfg), *z[:4], C.c_int32(4), None) == -1
    assert b"dgppo_vmas_reset_checked" in lib.dgppo_last_error()
    assert lib.dgppo_env_reset_checked(C.byref(cfg), *z[:5], C.c_int32(4), None) == -1
    assert b"dgppo_vmas_reset_checked" in lib.dgppo_last_error()
    assert lib.dgppo_graph_feats(C.byref(cfg), None, C.c_int64(0), C.c_int64(0), None, None, None, C.c_int64(0),
                                 C.c_int64(0), None, C.c_int32(1), C.c_int32(1), None, None, None, None, C.c_int32(20),
                                 None) == -1
    assert b"dgppo_vmas_graph_feats" in lib.dgppo_last_error()
    # ... and the VMAS entry points refuse the other kinds, more than 16 agents and densities the reset cannot place
    other = N.make_env_cfg(0, 3, 1)
    assert lib.dgppo_vmas_reset_checked(C.byref(other), *z[:5], C.c_int32(4), None) == -1
    assert b"not VMASReverseTransport" in lib.dgppo_last_error()
    big = N.make_env_cfg(10, 17, 0)
    assert lib.dgppo_env_num_nodes(C.byref(big)) == -1 and b"[1,16]" in lib.dgppo_last_error()
    dense = N.make_env_cfg(10, 16, 0)
    assert lib.dgppo_vmas_reset_checked(C.byref(dense), *z[:5], C.c_int32(4), None) == -1
    assert b"cannot be placed" in lib.dgppo_last_error()
    bad = N.make_env_cfg(10, 3, 0)
    bad.n_goals = 3
    assert lib.dgppo_env_num_nodes(C.byref(bad)) == -1


def test_render_video_of_a_restated_episode(tmp_path):
    """env.render_video draws the box, goal, obstacles and agents of one episode (vmas_reverse_transport.py:321-431)"""
    import types
    from dgppo_amd.env import make_env, VMASReverseTransportState
    n, T = 3, 4
    env = make_env("VMASReverseTransport", n, num_obs=0)
    agent, body, scene, _ = V.reset(np.array([5, 6]), n)
    rng = np.random.default_rng(0)
    A, Bd, C = [agent], [body], []
    for _ in range(T - 1):
        out = V.env_step(A[-1], Bd[-1], scene, rng.uniform(-1, 1, (2, n, 2)).astype(f32))
        A.append(out["next_agent"]); Bd.append(out["next_body"]); C.append(out["cost"])
    C.append(V.get_cost(A[-1], Bd[-1], scene))
    A, Bd, C = np.stack(A, 1), np.stack(Bd, 1), np.stack(C, 1)          # [2, T, ...]
    es = VMASReverseTransportState(Bd[..., :2], Bd[..., 2:], A[..., :2], A[..., 2:], np.repeat(scene[:, None, :2], T, 1),
                                   np.repeat(scene[:, None, 2:].reshape(2, 1, 3, 2), T, 1))
    ro = types.SimpleNamespace(graph=types.SimpleNamespace(env_states=es), costs=C)
    out = env.render_video(ro, tmp_path / "vmas.gif", None, {}, dpi=30, index=1)
    assert out.exists() and out.stat().st_size > 500
    from PIL import Image, ImageSequence
    with Image.open(out) as im:
        assert sum(1 for _ in ImageSequence.Iterator(im)) == T
