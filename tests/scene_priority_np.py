"""Restatement of the pool by priority (csrc/env_scene_pool.hip: dgppo_env_scene_pool_score, dgppo_env_scene_pool_draw,
dgppo_env_scene_pool_push_evict) and of its priority q, in Python ints and NumPy float32 with the kernels' operation order.
Everything compared against it is integers, copied words, or fp32 values formed by the same single operations."""
import numpy as np

from oracle import env_np as EN

f32 = np.float32
MAX_M, MAX_AGE = 65536, 1024


# ---- the priority: written once here, once in the kernels ----------------------------------------------------------------------
def w_clamp(v):
    """a NaN or a value below 0 -> 0, a value above 1 -> 1; float32 array or scalar"""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        v = np.where(v >= f32(0), v, f32(0)).astype(f32)
        return np.where(v > f32(1), f32(1), v).astype(f32)


def w(s):
    s = np.asarray(s, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return w_clamp((f32(4) * s).astype(f32) * (f32(1) - s).astype(f32))


def q_w(wv):
    """(uint32)(w * 65535.0f) + 1, truncated: int64 in [1, 65536]"""
    return (np.asarray(wv, f32) * f32(65535)).astype(f32).astype(np.uint32).astype(np.int64) + 1


def q(s):
    return q_w(w(s))


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def scene_envs(n_total, n_scene, lo, B):
    """-> (is_scene bool [B], k [B] Python ints) of the global envs lo .. lo + B - 1"""
    is_scene, ks = np.zeros(B, bool), []
    for b in range(B):
        g = lo + b
        k = g * n_scene // n_total
        is_scene[b] = (g + 1) * n_scene // n_total > k
        ks.append(k)
    return is_scene, ks


def weights(score, last, fixed, filled, step, age_cap):
    """Q [M] as Python ints"""
    M = len(score)
    live = np.arange(M) < max(fixed, fixed + int(filled))
    age = np.minimum(1 + np.maximum(int(step) - np.asarray(last, np.int64), 0), int(age_cap))
    return [int(v) for v in np.where(live, q(score) * age, 0)]


def pick(Q, t):
    """the smallest m whose inclusive prefix sum of Q exceeds t (0 <= t < sum Q)"""
    acc = 0
    for m, v in enumerate(Q):
        acc += v
        if acc > t:
            return m
    raise AssertionError(f"t = {t} is not below the total {acc}")


def draw_t(k, step, draw_seed, total):
    wd = EN.philox4x32((k, int(step) & 0xFFFFFFFF, 0, 0), (draw_seed & 0xFFFFFFFF, (draw_seed >> 32) & 0xFFFFFFFF))
    u = (wd[0] << 32) | wd[1]
    return (u * total) >> 64


def draw_Q(Q, ks, step, draw_seed):
    """the slots of the scene envs with ordinals ks under the weights Q (Python ints); -1 for all while the total is 0"""
    total = sum(Q)
    if total == 0:
        return [-1] * len(ks)
    cum = np.cumsum(np.asarray(Q, object))                    # exact ints
    out = []
    for k in ks:
        t = draw_t(k, step, draw_seed, total)
        lo, hi = 0, len(Q) - 1
        while lo < hi:                                         # any search gives the same smallest m: the prefix sums are monotone
            mid = (lo + hi) // 2
            if cum[mid] > t:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
    return out


def draw_np(score, last, state, fixed, age_cap, step, draw_seed, n_total, n_scene, lo, B):
    """-> scene_of int32 [B]"""
    Q = weights(score, last, fixed, state[1], step, age_cap)
    is_scene, ks = scene_envs(n_total, n_scene, lo, B)
    out = np.full(B, -1, np.int32)
    idx = np.flatnonzero(is_scene)
    out[idx] = draw_Q(Q, [ks[b] for b in idx], step, draw_seed)
    return out


# ---- the score ---------------------------------------------------------------------------------------------------------------------
def score_np(scene_of, mix_flags, first, score, visits, last, beta, step, state):
    """-> (score, visits, last, state) after the call (copies)"""
    score, visits, last = np.array(score, f32), np.array(visits, np.int32), np.array(last, np.int32)
    state = [int(v) for v in state]
    M, beta = len(score), f32(beta)
    r, f = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for b, m in enumerate(scene_of):
        if m < 0 or m >= M or mix_flags[b] != 0:              # mix_flags[b] is not looked at where scene_of[b] < 0
            continue
        r[m] += 1
        f[m] += int(first[b] >= 0)
    for m in np.flatnonzero(r > 0):
        y = f32(f32(f[m]) / f32(r[m]))
        score[m] = f32(score[m] + f32(beta * f32(y - score[m])))
        visits[m] += r[m]
        last[m] = step
    state[6], state[7] = int(r.sum()), int(f.sum())
    return score, visits, last, state


# ---- the evicting push -------------------------------------------------------------------------------------------------------------
def taken(first, flags):
    return (np.asarray(first) >= 1) & (np.asarray(flags) == 0)


def push_evict_np(first, flags, rows, pool, fixed, score, visits, last, min_visits, evict_w, step, state):
    """rows / pool: dict name -> float32 [B, ...] / [M, ...] (None entries skipped).
    -> (pool, score, visits, last, state, slot_of [B] int32) after the push (copies)"""
    M = len(score)
    R = M - fixed
    score, visits, last = np.array(score, f32), np.array(visits, np.int32), np.array(last, np.int32)
    state = [int(v) for v in state]
    head, filled, pushed = state[0], state[1], state[2]
    out = {k: None if v is None else v.copy() for k, v in pool.items()}
    wv = w(score)
    targets = list(range(filled, R))                          # the empties, ascending; then the evictable, in ring order from head
    n_empty = len(targets)
    for i in range(R):
        p = (head + i) % R
        if p < filled and visits[fixed + p] >= min_visits and wv[fixed + p] <= f32(evict_w):
            targets.append(p)
    slot_of = np.full(len(first), -1, np.int32)
    took = np.flatnonzero(taken(first, flags))
    for r, b in enumerate(took):
        if r >= len(targets):
            break
        m = fixed + targets[r]
        slot_of[b] = m
        for k, v in out.items():
            if v is not None:
                v.view(np.uint32)[m] = rows[k].view(np.uint32)[b]
        score[m], visits[m], last[m] = f32(0.5), 0, step
    count = len(took)
    written = min(count, len(targets))
    to_empty = min(written, n_empty)
    evicted = written - to_empty
    if evicted > 0:
        state[0] = (targets[written - 1] + 1) % R
    state[1] = filled + to_empty
    state[2] = pushed + written
    state[3], state[4], state[5] = count, evicted, count - written
    return out, score, visits, last, state, slot_of
