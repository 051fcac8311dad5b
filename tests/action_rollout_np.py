"""The action rollout landscape restated in NumPy: the layout of dgppo_env_action_sweep_fork (include/dgppo_hip.h) and the fold
dgppo_constraint_return applies to the rolled costs.  Shared by tests/test_action_rollout_cpu.py and
tests/test_action_rollout_gpu.py; the hand-made scene is lookahead_np's."""
import numpy as np

f32 = np.float32


def fork_np(step, env, actions, frame_ids, n_frames, agent_id, us, vs, carry=None):
    """step: name -> [T + 1, ...] per-step fields of ONE env; env: name -> its per-env rows; actions [T, n, 2]; carry
    [T', n, HC] (slot t: the carry AFTER frame t's policy forward) or None; frame_ids: frame numbers or None (0 .. n_frames - 1)
    -> (fields of the G = n_frames * nv * nu envs, action [G, n, 2], carry [G * n, HC] or None), all uint32.
    Env (f * nv + iv) * nu + iu is a copy of frame frame_ids[f]; row agent_id of its joint action is (us[iu], vs[iv]), every
    other row the recorded one of that frame.  Words only: nothing is clipped, a NaN keeps its payload."""
    w = lambda x: np.ascontiguousarray(x, f32).view(np.uint32)
    us, vs = w(np.asarray(us, f32).reshape(-1)), w(np.asarray(vs, f32).reshape(-1))
    nu, nv = us.size, vs.size
    fids = np.arange(n_frames) if frame_ids is None else np.asarray(frame_ids, np.int64).reshape(-1)
    assert fids.size == n_frames
    P = nv * nu
    out = {k: np.repeat(w(v)[fids], P, axis=0) for k, v in step.items()}
    out.update({k: np.repeat(w(v)[None], n_frames * P, axis=0) for k, v in env.items()})
    act = np.repeat(w(actions)[fids], P, axis=0).reshape(n_frames, nv, nu, -1, 2)
    act[:, :, :, agent_id, 0] = us[None, None, :]
    act[:, :, :, agent_id, 1] = vs[None, :, None]
    c = None
    if carry is not None:
        c = np.repeat(w(carry)[fids], P, axis=0)
        c = c.reshape(-1, c.shape[-1])
    return out, act.reshape(n_frames * P, -1, 2), c


def nanmax(a, b):
    """jnp.maximum: a NaN in either operand gives a NaN"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), f32(np.nan), np.maximum(a, b)).astype(f32)


def fold_np(cost, gamma):
    """cost [K, G, n, nh] -> (value, worst) [G, n, nh], dgppo_constraint_return's arithmetic in fp32: V = h[K-1]; for k = K-2 ..
    0: m = max_c h[k][c], V[c] = max(h[k][c], (1 - gamma) * m + gamma * V[c]) — one multiply, one multiply and one add, in that
    order; worst = max_k h[k].  Every max propagates NaN."""
    cost = np.asarray(cost, f32)
    g, omg = f32(gamma), f32(1.0 - float(gamma))
    V, W = cost[-1].copy(), cost[-1].copy()
    for k in range(cost.shape[0] - 2, -1, -1):
        h = cost[k]
        m = h[..., 0]
        for c in range(1, h.shape[-1]):
            m = nanmax(m, h[..., c])
        dm = (omg * m).astype(f32)[..., None]
        V = nanmax(h, (dm + (g * V).astype(f32)).astype(f32))
        W = nanmax(W, h)
    return V, W
