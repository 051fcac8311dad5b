"""Kernel-level GPU parity of the entry points between the env step and the networks: the tanh-Normal head's saturated
branches, the LSTM scan, the advantage / shaped-reward / Lagrangian kernels, clip + Adam and the small elementwise kernels,
each against a float64 evaluation of the same operation (oracle/algo_ref.py in numpy, oracle/nn_torch.py in torch), at the
sizes where a kernel changes behaviour: one row, ragged last workgroup, past the capped grid (stride loops), ragged last
tile.  Tolerances are the project's (1e-5 forward, 2e-5 / 3e-5 gradients, relative to the output scale); where another
number is used, the comment next to it says where it comes from."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import algo_ref as A
from oracle import nn_torch as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _close(got, want, tol=1e-5, name=""):
    """max abs error <= tol * max(1, max |want|): the scaling of tests/test_nn_gpu.py"""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print(f"{name}: max abs err {err:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})")
    assert err <= tol * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3e})"


def _close_each(got, want, tol, name=""):
    """the same tolerance with the scale taken per element, |got - want| <= tol * max(1, |want|): one large entry does not
    widen the bound of the others"""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ratio = (got - want).abs() / want.abs().clamp_min(1.0)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{name}: max scaled err {worst:.3e} (bound {tol:.3e})")
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert worst <= tol, f"{name}: max |got - want| / max(1, |want|) = {worst:.3e} > {tol:.1e}"


def _np_close(got, want, tol, name=""):
    err = np.abs(np.asarray(got, f64) - np.asarray(want, f64))
    scale = max(1.0, float(np.abs(want).max())) if err.size else 1.0
    worst = float(err.max()) if err.size else 0.0
    print(f"{name}: max abs err {worst:.3e} (scale {scale:.3e}, bound {tol * scale:.3e})")
    assert worst <= tol * scale, f"{name}: max abs err {worst:.3e} (scale {scale:.3e})"


# ----------------------------------------------------------------------------------------------------------------------
# 1. tanh-Normal head (dgppo_policy_head)
# ----------------------------------------------------------------------------------------------------------------------
_BANDS = (("u > 0", 0.2, 4.0), ("-5 < u < 0", -4.9, -0.1), ("-10 < u <= -5", -9.9, -5.0), ("-20 < u < -10", -19.5, -10.1))


def _band_index(u):
    """0: u > 0, 1: (-5, 0], 2: (-10, -5], 3: (-20, -10], 4: below — the second boundary is log_ndtr's old cut-off, the third
    its new one"""
    return np.where(u > 0, 0, np.where(u > -5, 1, np.where(u > -10, 2, np.where(u > -20, 3, 4))))


def saturated_head_inputs(seed=11, per_cell=16):
    """Rows whose stored action is saturated (|a| >= 0.999) in dimension 0, in dimension 1, or in both, with the mean solved
    from a chosen u = (+-mean - atanh 0.999) / std so that u falls into each band of _BANDS on each side.  Returns float32
    ms [rows, 4], action [rows, 2] and the bookkeeping (which dims are saturated, their side)."""
    g = np.random.default_rng(seed)
    sat, side, band, mag = [], [], [], []
    for which in ((True, False), (False, True), (True, True)):
        for b in range(len(_BANDS)):
            for s in (1.0, -1.0):
                for m in (1.0, 0.999):
                    for _ in range(per_cell):
                        sat.append(which); side.append(s); band.append(b); mag.append(m)
    sat = np.array(sat); side = np.array(side)[:, None]; band = np.array(band); mag = np.array(mag)[:, None]
    rows = len(band)
    lo = np.array([_BANDS[b][1] for b in band])[:, None]
    hi = np.array([_BANDS[b][2] for b in band])[:, None]
    u = lo + (hi - lo) * g.random((rows, 2))
    std_sat = 0.05 + 0.95 * g.random((rows, 2))
    std_in = 0.3 + 0.7 * g.random((rows, 2))                 # interior dimensions: not what this test measures
    std = np.where(sat, std_sat, std_in)
    mean = np.where(sat, side * (T.INV_THRESH + u * std), g.normal(size=(rows, 2)))
    act = np.where(sat, side * mag, np.clip(np.tanh(g.normal(size=(rows, 2))), -0.99, 0.99))
    std_trans = np.log(np.expm1(std - T.STD_MIN)) - T.STD_INIT_INV      # softplus^-1
    ms = torch.from_numpy(np.concatenate([mean, std_trans], 1).astype(f32))
    return ms, torch.from_numpy(act.astype(f32)), sat, side


def head_reference(ms, a_in, eps_hat, lp_old, adv, n, clip_eps=0.25, coef_ent=0.01):
    """float64 oracle of eval_action + the PPO surrogate and its autograd gradient w.r.t. ms"""
    rows = ms.shape[0]
    msr = ms.double().requires_grad_()
    mean_r, std_r = msr[:, :2], torch.nn.functional.softplus(msr[:, 2:] + T.STD_INIT_INV) + T.STD_MIN
    lp = T.tanh_normal_log_prob(a_in.double(), mean_r, std_r)
    ent = T.tanh_normal_entropy(mean_r, std_r, eps_hat.double()[torch.arange(rows) % n])
    rho = torch.exp(lp - lp_old.double())
    l1, l2 = -rho * adv.double(), -torch.clamp(rho, 1 - clip_eps, 1 + clip_eps) * adv.double()
    loss = torch.maximum(l1, l2).mean() - coef_ent * ent.mean()
    loss.backward()
    # rows whose clip decision an error of log_pi within its own tolerance (1e-5 * max(1, |log_pi|)) could move: rho within that
    # relative distance of 1 +- clip_eps
    reach = 1e-5 * lp.detach().abs().clamp_min(1.0)
    border = (((rho.detach() / (1 - clip_eps) - 1).abs() < reach) | ((rho.detach() / (1 + clip_eps) - 1).abs() < reach)).sum()
    return dict(lp=lp.detach(), ent=ent.detach(), dms=msr.grad, loss=loss.detach(), clipped=(l2 > l1).sum(), border=border,
                tv=0.5 * (rho.detach() - 1).abs().mean())


def _head_eval(cuda, ms, a_in, eps_hat, lp_old, adv, n, with_loss=True, stats=None):
    from dgppo_amd import ops_nn as K_
    rows = ms.shape[0]
    lp = torch.full((rows,), float("nan"), device=cuda)
    ent = torch.full((rows,), float("nan"), device=cuda)
    dms = torch.full((rows, 4), float("nan"), device=cuda) if with_loss else None
    stats = torch.zeros(8, device=cuda) if stats is None else stats
    K_.policy_head(ms.to(cuda), eps_hat.to(cuda), a_in.to(cuda), None, lp, ent, n, 2,
                   lp_old.to(cuda) if with_loss else None, adv.to(cuda) if with_loss else None, dms, stats, 0.25, 0.01)
    torch.cuda.synchronize()
    return lp, ent, dms, stats


def _check_head_stats(stats, ref, rows, name, calls=1):
    """stats[0..3] of `calls` accumulated calls.  The number of clipped rows is an integer: it equals the oracle's, except
    for rows that sit on the clip boundary to within the tolerance of log_pi (none in the small cases)."""
    s = stats.cpu().double() / calls
    _close(s[0] / rows - 0.01 * s[1] / rows, ref["loss"], 1e-5, name + " loss")
    print(f"{name}: clipped rows {float(s[2]):.0f} (oracle {int(ref['clipped'])}, on the boundary {int(ref['border'])})")
    assert abs(float(s[2]) - int(ref["clipped"])) <= int(ref["border"]), name + " clip count"
    _close(0.5 * s[3] / rows, ref["tv"], 1e-5, name + " tv")
    assert float(stats[4:].abs().max()) == 0.0


def test_policy_head_saturated_actions_in_every_tail_band(cuda):
    """Stored actions +-1.0 and +-0.999 in either or both dimensions, with the current mean placed so that the argument u of
    log Phi lies above 0, in (-5, 0), in (-10, -5] and in (-20, -10) — the last two are where log_ndtrf_ / dlog_ndtrf_ leave
    the erfc form.  log_pi, entropy, the gradient and the four diagnostics against autograd of the float64 oracle
    (torch.special.log_ndtr).  log_pi and the gradient are held per element, |err| <= tol * max(1, |want|), band by band: a
    row with log_pi = -200 must not widen the bound of a row at u = -5."""
    n = 8
    ms, a_in, sat, side = saturated_head_inputs()
    rows = ms.shape[0]
    # ---- conditions on the inputs, on the CPU: every (band, side, dimension) cell holds >= 16 rows after the float32
    # rounding of ms, and every std lies in [0.05, 1]
    std64 = np.logaddexp(0.0, ms[:, 2:].double().numpy() + T.STD_INIT_INV) + T.STD_MIN
    u64 = (side * ms[:, :2].double().numpy() - T.INV_THRESH) / std64
    bi = np.where(sat, _band_index(u64), -1)
    assert std64.min() >= 0.05 - 1e-6 and std64.max() <= 1.0 + 1e-6
    for d in range(2):
        for b in range(4):
            for s in (1.0, -1.0):
                cnt = int(((bi[:, d] == b) & (side[:, 0] == s)).sum())
                assert cnt >= 16, f"band {_BANDS[b][0]} side {s:+.0f} dim {d}: {cnt} rows"
    assert not (bi == 4).any()
    assert (np.abs(a_in.numpy())[sat] >= 0.999).all() and (np.abs(a_in.numpy())[~sat] < 0.999).all()
    g = torch.Generator().manual_seed(5)
    eps_hat = torch.randn(n, 2, generator=g)
    adv = torch.randn(rows, generator=g)
    noise = 0.3 * torch.randn(rows, generator=g)
    with torch.no_grad():
        std_t = torch.nn.functional.softplus(ms[:, 2:].double() + T.STD_INIT_INV) + T.STD_MIN
        lp_old = (T.tanh_normal_log_prob(a_in.double(), ms[:, :2].double(), std_t) + noise.double()).float()
    ref = head_reference(ms, a_in, eps_hat, lp_old, adv, n)
    lp, ent, dms, stats = _head_eval(cuda, ms, a_in, eps_hat, lp_old, adv, n)
    row_band = torch.from_numpy(bi.max(axis=1))
    for b in range(4):
        m = row_band == b
        _close_each(lp.cpu()[m], ref["lp"][m], 1e-5, f"log_pi, band {_BANDS[b][0]}")
    _close(ent, ref["ent"], 1e-5, "entropy")
    # The gradient of the MEAN loss carries 1 / rows; the per-row gradient (times rows) is held to the scale of its own band.
    # In the band (-20, -10) log_pi reaches -400, where fp32 resolves it to 3e-5, and so does the ratio
    # rho = exp(log_pi - log_pi_old) that multiplies every gradient entry: the same formulas evaluated in float32 on the CPU
    # from the same inputs deviate from the float64 oracle by 4.7e-5 of that band's scale (the other bands: 5.6e-6, 4.6e-6,
    # 7.2e-6).  That band alone is allowed 4 times the measured deviation.
    for b, tol in enumerate((2e-5, 2e-5, 2e-5, 4 * 4.7e-5)):
        m = row_band == b
        _close(dms.cpu()[m] * rows, ref["dms"][m] * rows, tol, f"dms * rows, band {_BANDS[b][0]}")
    _check_head_stats(stats, ref, rows, "saturated")


@pytest.mark.parametrize("rows,n", [(1, 1), (1000, 8), (163840, 1), (163840, 3), (163840, 16)])
def test_policy_head_shapes(cuda, rows, n):
    """one row; a ragged last workgroup; 163 840 rows = 640 workgroups of 256 over the grid of 512, so the stride loop runs,
    with 1, 3 and 16 agents (the entropy noise is indexed row % n_agents).  Eval without the loss leaves stats bit-unchanged
    and gives the same log_pi / entropy; two calls into the same stats accumulate."""
    g = torch.Generator().manual_seed(rows + n)
    ms = torch.randn(rows, 4, generator=g)
    ms[:, :2] *= 1.5
    eps = torch.randn(rows, 2, generator=g)
    with torch.no_grad():
        std = torch.nn.functional.softplus(ms[:, 2:] + T.STD_INIT_INV) + T.STD_MIN
        # stored actions are samples of the distribution they are evaluated under (some saturate on the side of their mean).
        # An action unrelated to the mean would sit dozens of (small) standard deviations away, log_pi would reach -3000,
        # and the PPO ratio exp(log_pi - log_pi_old), which fp32 resolves to |log_pi| * 2^-24, would be known to 2e-4 only:
        # the gradient check would then measure that, not the kernel.
        a_in = torch.tanh(ms[:, :2] + std * eps)
        lp_old = (T.tanh_normal_log_prob(a_in.double(), ms[:, :2].double(), std.double())
                  + 0.3 * torch.randn(rows, generator=g).double()).float()
    eps_hat = torch.randn(n, 2, generator=g)
    adv = torch.randn(rows, generator=g)
    ref = head_reference(ms, a_in, eps_hat, lp_old, adv, n)
    # condition on the inputs (CPU): the ratio's fp32 resolution stays a quarter of the gradient tolerance or less
    assert float(ref["lp"].abs().max()) * 2.0 ** -24 <= 2e-5 / 4, float(ref["lp"].abs().max())
    assert rows < 1000 or (a_in.abs() >= 0.999).any()
    lp, ent, dms, stats = _head_eval(cuda, ms, a_in, eps_hat, lp_old, adv, n)
    _close(lp, ref["lp"], 1e-5, "log_pi")
    _close(ent, ref["ent"], 1e-5, "entropy")
    _close(dms, ref["dms"], 2e-5, "dms")
    _close(dms * rows, ref["dms"] * rows, 2e-5, "dms * rows")
    _check_head_stats(stats, ref, rows, f"rows={rows}")
    # without the loss: same log_pi / entropy bit for bit, stats untouched
    before = torch.randn(8, generator=g).to(cuda)
    keep = before.clone()
    lp2, ent2, _, _ = _head_eval(cuda, ms, a_in, eps_hat, lp_old, adv, n, with_loss=False, stats=before)
    assert torch.equal(before, keep), "eval without dms must not touch stats"
    assert torch.equal(lp2, lp) and torch.equal(ent2, ent)
    # a second call with the loss accumulates onto the first
    _, _, dms3, stats = _head_eval(cuda, ms, a_in, eps_hat, lp_old, adv, n, stats=stats)
    assert torch.equal(dms3, dms)
    _check_head_stats(stats, ref, rows, f"rows={rows}, two calls", calls=2)


# ----------------------------------------------------------------------------------------------------------------------
# 2. LSTM scan (dgppo_lstm_fwd / dgppo_lstm_bwd)
# ----------------------------------------------------------------------------------------------------------------------
def lstm_case(n_grp, T_, n_inner, carry0, dtype=torch.float64):
    """inputs of one LSTM case and the oracle's forward + autograd backward in `dtype`"""
    g = torch.Generator().manual_seed(n_grp + T_)
    p = T.init_lstm(g)
    for k in ("hi", "hf", "hg", "ho"):                       # init_lstm zeroes the hidden biases
        p[k]["bias"] = torch.randn(64, generator=g) * 0.1
    n_seq = n_grp * n_inner
    rows = n_seq * T_
    x = torch.randn(rows, 64, generator=g)                   # row = (grp * T + tau) * n_inner + i
    c0 = torch.randn(n_seq, 64, generator=g) * 0.5 if carry0 else None
    h0 = torch.tanh(torch.randn(n_seq, 64, generator=g)) * 0.5 if carry0 else None
    dhs = torch.randn(rows, 64, generator=g)
    pd = T.tree_map(lambda t: t.to(dtype).requires_grad_(), p)
    xd = x.to(dtype).requires_grad_()
    zero = torch.zeros(n_grp, n_inner, 64, dtype=dtype)
    c0d = c0.to(dtype).view(n_grp, n_inner, 64) if carry0 else zero
    h0d = h0.to(dtype).view(n_grp, n_inner, 64) if carry0 else zero
    hs, cs = T.lstm_scan(pd, c0d, h0d, xd.view(n_grp, T_, n_inner, 64))
    (hs.reshape(rows, 64) * dhs.to(dtype)).sum().backward()
    with torch.no_grad():
        cprev = torch.cat([c0d[:, None], cs[:, :-1]], 1).reshape(rows, 64)
        hprev = torch.cat([h0d[:, None], hs[:, :-1]], 1).reshape(rows, 64)
        pre = [T.dense(pd["i" + q], xd) + T.dense(pd["h" + q], hprev) for q in "ifgo"]
        gates = torch.cat([torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.tanh(pre[2]), torch.sigmoid(pre[3])], 1)
    want = dict(hs=hs.detach().reshape(rows, 64), cs=cs.detach().reshape(rows, 64), cprev=cprev, hprev=hprev, gates=gates,
                dx=xd.grad, dWi=torch.cat([pd["i" + q]["kernel"].grad for q in "ifgo"], 1),
                dWh=torch.cat([pd["h" + q]["kernel"].grad for q in "ifgo"], 1),
                dbh=torch.cat([pd["h" + q]["bias"].grad for q in "ifgo"]))
    return p, x, c0, h0, dhs, want


# (1, 129, 1): one sequence, the pre-pass length.  The project's tolerances hold for this chain too: a float32 CPU run of
# the oracle loop deviates from the float64 one by 2.4e-7 (hs), 1.8e-7 (cs), 6.0e-7 (gates), 2.7e-7 of scale (dx), 4.0e-7
# (dWi), 4.6e-7 (dWh), 2.3e-7 (dbh); 4 times that is far below 1e-5 / 2e-5 / 3e-5, so the case needs no bound of its own.
@pytest.mark.parametrize("n_grp,T_,n_inner,carry0", [
    (5, 16, 8, False), (70, 1, 3, True), (9, 7, 1, True),
    (3, 5, 3, False),            # 9 sequences: ragged last tile (1 live sequence of 4) with n_inner > 1
    (3, 5, 3, True),
    (1, 129, 1, False),
    (2051, 2, 8, True),          # 16 408 sequences = 4102 tiles over a grid of 512: every workgroup runs the tile loop 8-9 times
    (2051, 2, 8, False),
    (8195, 1, 1, True)])         # 2049 tiles: workgroup 0 alone takes a fifth pass, with three live sequences
def test_lstm_scan(cuda, n_grp, T_, n_inner, carry0):
    """the twin of test_gru_scan: forward outputs and saved activations against a float64 loop over the oracle's lstm_cell,
    the call without saved activations bit-identical, and dz through everything the header derives from it (dx = dz Wi^T,
    dWi = x^T dz, dWh = hprev^T dz, dbh = colsum dz; products formed on the host in float64)."""
    from dgppo_amd import ops_nn as K_
    p, x, c0, h0, dhs, want = lstm_case(n_grp, T_, n_inner, carry0)
    n_seq = n_grp * n_inner
    rows = n_seq * T_
    Wi = torch.cat([p["i" + q]["kernel"] for q in "ifgo"], 1)
    Wh = torch.cat([p["h" + q]["kernel"] for q in "ifgo"], 1).contiguous().to(cuda)
    bh = torch.cat([p["h" + q]["bias"] for q in "ifgo"]).to(cuda)
    zi = (x.double() @ Wi.double()).float().to(cuda)
    nan = lambda *shape: torch.full(shape, float("nan"), device=cuda)
    dev = lambda t: None if t is None else t.to(cuda)
    cs, hs, cprev, hprev, gates = nan(rows, 64), nan(rows, 64), nan(rows, 64), nan(rows, 64), nan(rows, 256)
    K_.lstm_fwd(zi, Wh, bh, dev(c0), dev(h0), cs, hs, cprev, hprev, gates, n_seq, T_, n_inner)
    cs2, hs2 = nan(rows, 64), nan(rows, 64)
    K_.lstm_fwd(zi, Wh, bh, dev(c0), dev(h0), cs2, hs2, None, None, None, n_seq, T_, n_inner)
    torch.cuda.synchronize()
    assert torch.equal(hs2, hs) and torch.equal(cs2, cs), "the call without saved activations must give the same hs / cs"
    for k, got in (("hs", hs), ("cs", cs), ("cprev", cprev), ("hprev", hprev), ("gates", gates)):
        assert torch.isfinite(got).all(), f"lstm {k}: rows left unwritten"
        _close(got, want[k], 1e-5, "lstm " + k)
    dz = nan(rows, 256)
    K_.lstm_bwd(dev(dhs), Wh, cprev, gates, dz, n_seq, T_, n_inner)
    torch.cuda.synchronize()
    assert torch.isfinite(dz).all(), "lstm dz: rows left unwritten"
    dzc = dz.cpu().double()
    _close(dzc @ Wi.double().T, want["dx"], 2e-5, "lstm dx")
    _close(x.double().T @ dzc, want["dWi"], 3e-5, "lstm dWi")
    _close(hprev.cpu().double().T @ dzc, want["dWh"], 3e-5, "lstm dWh")
    _close(dzc.sum(0), want["dbh"], 3e-5, "lstm dbh")
    for q in range(4):                                       # per gate block: a small block must not hide behind a large one
        sl = slice(64 * q, 64 * q + 64)
        _close((x.double().T @ dzc)[:, sl], want["dWi"][:, sl], 3e-5, f"lstm dWi[{'ifgo'[q]}]")
        _close((hprev.cpu().double().T @ dzc)[:, sl], want["dWh"][:, sl], 3e-5, f"lstm dWh[{'ifgo'[q]}]")
        _close(dzc.sum(0)[sl], want["dbh"][sl], 3e-5, f"lstm dbh[{'ifgo'[q]}]")


# ----------------------------------------------------------------------------------------------------------------------
# 3. advantage, shaped reward, Lagrangian (csrc/gae.hip)
# ----------------------------------------------------------------------------------------------------------------------
ADV_SHAPES = [(1, 1, 1, 1), (3, 7, 1, 3), (5, 255, 16, 2), (2, 257, 3, 1), (2, 1000, 4, 2), (4096, 128, 8, 2)]
DT, ALPHA, CBF_EPS, CBF_W = 0.03, 10.0, 1e-2, 2.0


def adv_inputs(B, T_, n, nh):
    r = np.random.default_rng(B + T_)
    Ql = r.normal(size=(B, T_)).astype(f32)
    Vl = r.normal(size=(B, T_ + 1)).astype(f32)
    Vh = (r.normal(size=(B, T_ + 1, n, nh)) * 0.02 - 0.03).astype(f32)
    return Ql, Vl, Vh


def cbf_deriv(Vh, dt, alpha):
    """dgppo.py:246 in the dtype of Vh"""
    t = Vh.dtype.type
    return (Vh[:, 1:] - Vh[:, :-1]) / t(dt) + t(alpha) * Vh[:, :-1]


def _run_advantage(cuda, Ql, Vl, Vh, dt, alpha, eps, w, n):
    from dgppo_amd import ops_algo as O
    d = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    B, T_ = Ql.shape
    adv = torch.full((B, T_, n), float("nan"), device=cuda)
    stats = torch.zeros(8, device=cuda)
    O.advantage(d(Ql), d(Vl), d(Vh), dt, alpha, eps, w, adv, stats)
    torch.cuda.synchronize()
    return adv.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("B,T_,n,nh", ADV_SHAPES)
def test_advantage_shapes(cuda, B, T_, n, nh):
    """dgppo_advantage with the CBF terms over one step, one agent, nh = 1 and 3, T below / at / above the 256 threads of the
    workgroup, and the benchmark size, against the float64 numpy oracle.  As in test_advantage, gate flips and numeric
    error are counted separately and at most 4 flips pass; the inputs are first shown (CPU) to leave the float32 and float64
    oracles at most 4 gate decisions apart."""
    Ql, Vl, Vh = adv_inputs(B, T_, n, nh)
    d32, d64 = cbf_deriv(Vh, DT, ALPHA), cbf_deriv(Vh.astype(f64), DT, ALPHA)
    assert int(((d32 <= 0).min(-1) != (d64 <= 0).min(-1)).sum()) <= 4, "inputs: float32 and float64 gates disagree > 4 times"
    sd = (Ql - Vl[:, :-1]).astype(f64).std(axis=1)
    assert (sd.min() > 0.1) if T_ > 1 else (sd.max() == 0.0)
    want, safe = A.advantage(Ql.astype(f64), Vl.astype(f64), Vh.astype(f64), DT, ALPHA, CBF_EPS, CBF_W)
    got, stats = _run_advantage(cuda, Ql, Vl, Vh, DT, ALPHA, CBF_EPS, CBF_W, n)
    rounding_level = (np.abs(d32) < 1e-5).any(axis=-1)
    err = np.abs(got.astype(f64) - want)
    bad = ~(err <= 1e-5 * np.maximum(1, np.abs(want)))
    print(f"advantage {B, T_, n, nh}: max err {np.nanmax(err):.3e}, flips {int((bad & rounding_level).sum())}, safe {safe:.3f}")
    assert not (bad & ~rounding_level).any(), "numeric error above 1e-5 away from the gate threshold"
    assert (bad & rounding_level).sum() <= 4, "gate flips at the threshold should be a handful at most"
    assert abs(stats[0] / (B * T_ * n) - safe) < 1e-3
    if T_ > 1:
        assert 0.05 < safe < 0.95
    else:
        # T = 1: the standardised advantage is exactly 0, so the result is the CBF term alone whatever Ql and Vl are
        got2, _ = _run_advantage(cuda, Ql + f32(3.5), Vl * f32(-2.0), Vh, DT, ALPHA, CBF_EPS, CBF_W, n)
        assert np.array_equal(got, got2)


@pytest.mark.parametrize("B,T_,n,nh", ADV_SHAPES)
def test_advantage_without_cbf_terms(cuda, B, T_, n, nh):
    """Vh == NULL (InforMARL): the advantage half of informarl_targets (informarl.py:334-336); every (t, agent) pair counts
    as safe, so stats[0] receives B * T * n exactly."""
    Ql, Vl, _ = adv_inputs(B, T_, n, nh)
    want = A.informarl_advantage(Ql.astype(f64), Vl.astype(f64), n)
    got, stats = _run_advantage(cuda, Ql, Vl, None, DT, ALPHA, CBF_EPS, CBF_W, n)
    err = np.abs(got.astype(f64) - want)
    print(f"advantage(no Vh) {B, T_, n}: max err {err.max():.3e}")
    assert (err <= 1e-5 * np.maximum(1, np.abs(want))).all()
    assert stats[0] == float(B * T_ * n)
    assert not stats[1:].any()


def test_advantage_hard_gate_exact(cuda):
    """dt = 1/32, alpha = 8, cbf_eps = 2^-5 and Vh on the grid of multiples of 2^-8: (v1 - v0) * 32 + 8 * v0 is exact in fp32
    whether the kernel multiplies by the reciprocal, divides or fuses, and a non-zero derivative is at least 2^-5 away
    from the gate.  With planted exact ties (v1 = 0.75 v0: derivative 0, safe) and entries at derivative = -cbf_eps, no
    gate flip is allowed at all and stats[0] is the oracle's count."""
    B, T_, n, nh = 6, 64, 5, 2
    dt, alpha, eps = 1.0 / 32, 8.0, 2.0 ** -5
    r = np.random.default_rng(17)
    Vh = (r.integers(-256, 257, size=(B, T_ + 1, n, nh)) / 256.0).astype(f32)
    j = r.integers(-64, 65, size=(B, n, nh))
    j[j == 0] = 7
    for t in range(0, T_ - 1, 6):
        both = (t // 6) % 2 == 0                             # a tie in every component, or in component 0 only
        Vh[:, t, :, 0], Vh[:, t + 1, :, 0] = (4 * j[..., 0] / 256.0), (3 * j[..., 0] / 256.0)
        if both:
            Vh[:, t, :, 1], Vh[:, t + 1, :, 1] = (4 * j[..., 1] / 256.0), (3 * j[..., 1] / 256.0)
        Vh[:, t + 3, :, 1], Vh[:, t + 4, :, 1] = 3 / 256.0, 2 / 256.0        # derivative -2^-5 = -cbf_eps
    Ql = r.normal(size=(B, T_)).astype(f32)
    Vl = r.normal(size=(B, T_ + 1)).astype(f32)
    assert np.array_equal(Vh * 256, np.round(Vh * 256)) and np.abs(Vh).max() <= 1
    d32, d64 = cbf_deriv(Vh, dt, alpha), cbf_deriv(Vh.astype(f64), dt, alpha)
    assert np.array_equal(d32.astype(f64), d64), "the derivative must be exact in fp32"
    assert np.abs(d64[d64 != 0]).min() >= 2.0 ** -5
    assert (d64 == 0).sum() >= 100 and (d64 == -eps).sum() >= 100
    assert (Ql - Vl[:, :-1]).astype(f64).std(axis=1).min() > 0.1
    want, safe = A.advantage(Ql.astype(f64), Vl.astype(f64), Vh.astype(f64), dt, alpha, eps, CBF_W)
    n_safe = int((d64 <= 0).min(-1).sum())
    assert 0.05 < safe < 0.95 and ((d64 == 0).any(-1) & (d64 <= 0).min(-1)).any(), "a tie must decide some gate"
    got, stats = _run_advantage(cuda, Ql, Vl, Vh, dt, alpha, eps, CBF_W, n)
    err = np.abs(got.astype(f64) - want)
    print(f"hard gate: max err {err.max():.3e}, safe {safe:.3f}")
    assert (err <= 1e-5 * np.maximum(1, np.abs(want))).all(), "no gate flip is allowed on exactly representable derivatives"
    assert stats[0] == float(n_safe)


def test_advantage_propagates_nan_like_the_reference(cuda):
    """jnp.maximum(deriv + eps, 0).max(-1) and the per-env mean propagate NaN (dgppo.py:241-256): a NaN value Vh[b, t, agent, h]
    marks adv[b, t - 1, agent] and adv[b, t, agent]; a NaN Ql[b, t] marks the safe entries of env b (the unsafe ones take
    where(...) = 0) — exactly where the oracle has them, and nothing else changes."""
    B, T_, n, nh = 4, 40, 3, 2
    Ql, Vl, Vh = adv_inputs(B, T_, n, nh)
    clean, _ = _run_advantage(cuda, Ql, Vl, Vh, DT, ALPHA, CBF_EPS, CBF_W, n)
    Vh[1, 17, 2, 1] = np.nan
    Ql[2, 5] = np.nan
    want, _ = A.advantage(Ql.astype(f64), Vl.astype(f64), Vh.astype(f64), DT, ALPHA, CBF_EPS, CBF_W)
    nanw = np.isnan(want)
    safe2 = (cbf_deriv(Vh.astype(f64), DT, ALPHA)[2] <= 0).min(-1)
    assert nanw[1].sum() == 2 and nanw[1, 16, 2] and nanw[1, 17, 2] and not nanw[[0, 3]].any()
    assert np.array_equal(nanw[2], safe2) and 0 < safe2.sum() < safe2.size
    got, _ = _run_advantage(cuda, Ql, Vl, Vh, DT, ALPHA, CBF_EPS, CBF_W, n)
    assert np.array_equal(np.isnan(got), nanw), "NaN pattern of the advantage differs from the oracle's"
    assert (np.abs(np.nan_to_num(got) - np.nan_to_num(want)) <= 1e-5 * np.maximum(1, np.abs(np.nan_to_num(want)))).all()
    assert np.array_equal(got[[0, 3]], clean[[0, 3]]), "envs without a NaN must not change"


@pytest.mark.parametrize("rows", [1, 255, 257, 4096 * 128])
def test_shaped_reward(cuda, rows):
    """dgppo_shaped_reward = reward - w * sum_agents sum_components max(cost, 0) (the T_l line of informarl.py:329, negated)
    in float64; costs of both signs, weight 0 and non-zero.  Bound: 1e-6 of the output scale."""
    from dgppo_amd import ops_algo as O
    B, T_ = (4096, 128) if rows == 4096 * 128 else (1, rows)
    for n, nh in ((1, 1), (3, 2), (8, 3), (16, 2)):
        r = np.random.default_rng(rows + n)
        cost = r.uniform(-1, 1, size=(B, T_, n, nh)).astype(f32)
        rew = (-r.uniform(0, 1, size=(B, T_))).astype(f32)
        cd, rd = torch.from_numpy(cost).to(cuda), torch.from_numpy(rew).to(cuda)
        for w in (0.0, 0.7):
            out = torch.full((B, T_), float("nan"), device=cuda)
            O.shaped_reward(rd, cd, w, out)
            want = A.shaped_reward(rew.astype(f64), cost.astype(f64), float(f32(w)))
            _np_close(out.cpu().numpy(), want, 1e-6, f"shaped_reward rows={rows} n={n} nh={nh} w={w}")
            if w == 0.0:
                assert torch.equal(out, rd)


def test_shaped_reward_and_relu_fwd_propagate_nan(cuda):
    """jnp.maximum(cost, 0) and jnp.clip(costs, a_min=0) keep a NaN cost (informarl.py:329, informarl_lagr.py:213): the row of
    the shaped reward / the element of the clipped costs is NaN, and every other output keeps its bits."""
    from dgppo_amd import ops_algo as O
    B, T_, n, nh = 3, 50, 4, 2
    r = np.random.default_rng(8)
    cost = r.uniform(-1, 1, size=(B, T_, n, nh)).astype(f32)
    rew = (-r.uniform(0, 1, size=(B, T_))).astype(f32)
    d = lambda x: torch.from_numpy(x).to(cuda)
    clean, clean_relu = torch.empty(B, T_, device=cuda), torch.empty(B, T_, n, nh, device=cuda)
    O.shaped_reward(d(rew), d(cost), 0.7, clean)
    O.relu_fwd(d(cost), clean_relu)
    cost[1, 20, 2, 1] = np.nan                                # a positive-side and a first-component NaN
    cost[2, 49, 0, 0] = np.nan
    out, relu = torch.empty(B, T_, device=cuda), torch.empty(B, T_, n, nh, device=cuda)
    O.shaped_reward(d(rew), d(cost), 0.7, out)
    O.relu_fwd(d(cost), relu)
    want = A.shaped_reward(rew.astype(f64), cost.astype(f64), float(f32(0.7)))
    assert np.isnan(want).sum() == 2 and np.isnan(want[1, 20]) and np.isnan(want[2, 49])
    assert np.array_equal(np.isnan(out.cpu().numpy()), np.isnan(want)), "NaN pattern of the shaped reward"
    keep = ~torch.from_numpy(np.isnan(want)).to(cuda)
    assert torch.equal(out[keep], clean[keep])
    wr = torch.clamp_min(d(cost), 0.0)                        # propagates NaN
    assert torch.equal(torch.isnan(relu), torch.isnan(wr)) and int(torch.isnan(relu).sum()) == 2
    assert torch.equal(relu[~torch.isnan(wr)], clean_relu[~torch.isnan(wr)])
    assert torch.equal(torch.nan_to_num(relu), torch.nan_to_num(wr))


def _lagr_inputs(B, T_, n, nh, seed):
    r = np.random.default_rng(seed)
    Ql = r.normal(size=(B, T_)).astype(f32); Vl = r.normal(size=(B, T_ + 1)).astype(f32)
    Qh = r.normal(size=(B, T_, n, nh)).astype(f32); Vh = r.normal(size=(B, T_ + 1, n, nh)).astype(f32)
    lagr = r.uniform(0, 1, size=(n, nh)).astype(f32)
    return r, Ql, Vl, Qh, Vh, lagr


@pytest.mark.parametrize("B,T_,n,nh", [(2, 5, 1, 1), (3, 300, 4, 3), (2, 128, 16, 4)])   # the last: n * nh = 64, the limit
def test_advantage_lagr_shapes(cuda, B, T_, n, nh):
    from dgppo_amd import ops_algo as O
    _, Ql, Vl, Qh, Vh, lagr = _lagr_inputs(B, T_, n, nh, B + T_)
    d = lambda x: torch.from_numpy(x).to(cuda)
    adv = torch.full((B, T_, n), float("nan"), device=cuda); Ah = torch.full((B, T_, n, nh), float("nan"), device=cuda)
    O.advantage_lagr(d(Ql), d(Vl), d(Qh), d(Vh), d(lagr), adv, Ah)
    wA, wAh = A.advantage_lagr(*(x.astype(f64) for x in (Ql, Vl, Qh, Vh, lagr)))
    np.testing.assert_allclose(Ah.cpu().numpy(), wAh, atol=1e-5)
    np.testing.assert_allclose(adv.cpu().numpy(), wA, atol=1e-5)


def test_advantage_lagr_refuses_more_than_192_columns(cuda):
    """n * nh = 193 exceeds the kernel's shared arrays (64 agents x 3 costs = 192 columns): refused with a negative return
    before anything is launched"""
    from dgppo_amd import ops_algo as O
    B, T_, n, nh = 1, 2, 193, 1
    _, Ql, Vl, Qh, Vh, lagr = _lagr_inputs(B, T_, n, nh, 1)
    d = lambda x: torch.from_numpy(x).to(cuda)
    adv = torch.full((B, T_, n), float("nan"), device=cuda); Ah = torch.full((B, T_, n, nh), float("nan"), device=cuda)
    with pytest.raises(ValueError, match="advantage_lagr"):
        O.advantage_lagr(d(Ql), d(Vl), d(Qh), d(Vh), d(lagr), adv, Ah)
    torch.cuda.synchronize()
    assert torch.isnan(adv).all() and torch.isnan(Ah).all()


def test_lagr_update_strided_and_split(cuda):
    """dgppo_lagr_update past the 512 x 256 grid (70 envs x 128 steps x 16 agents = 143 360 rows) with Vh addressed through
    an env stride larger than (T + 1) n nh — the gap and the unused step T hold NaN, so a wrong stride or a read of step T
    shows —, a second step that drives multipliers to the clip at 0, and the data-parallel halves: dgppo_lagr_sums on two
    unequal parts into one `sums`, then dgppo_lagr_apply with the global row count."""
    from dgppo_amd import _native as N
    B, T_, n, nh = 70, 128, 16, 2
    r, _, _, _, Vh, lagr0 = _lagr_inputs(B, T_, n, nh, 23)
    Ah = r.normal(size=(B, T_, n, nh)).astype(f32)
    lp_new = (r.normal(size=(B, T_, n)) * 0.3).astype(f32); lp_old = (r.normal(size=(B, T_, n)) * 0.3).astype(f32)
    assert B * T_ * n > 512 * 256
    stride = (T_ + 1) * n * nh + 37
    buf = np.full((B, stride), np.nan, f32)
    buf[:, :T_ * n * nh] = Vh[:, :T_].reshape(B, -1)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    lpn, lpo, Ahd, Vhd = d(lp_new), d(lp_old), d(Ah), d(buf)
    omg = 1.0 - 0.99

    def update(lg, sums, lr):
        N.check(N.lib().dgppo_lagr_update(N.ptr(lpn), N.ptr(lpo), N.ptr(Vhd), C.c_int64(stride), N.ptr(Ahd), N.ptr(lg), N.ptr(sums),
                                          B, T_, n, nh, C.c_float(omg), C.c_float(lr), N.stream_ptr()), "dgppo_lagr_update")

    def split_update(lg, sums, lr, cut=23):
        for e0, e1 in ((0, cut), (cut, B)):
            N.check(N.lib().dgppo_lagr_sums(N.ptr(lpn[e0:e1]), N.ptr(lpo[e0:e1]), N.ptr(Vhd[e0:e1]), C.c_int64(stride),
                                            N.ptr(Ahd[e0:e1]), N.ptr(sums), e1 - e0, T_, n, nh, C.c_float(omg), N.stream_ptr()),
                    "dgppo_lagr_sums")
        assert float(sums.abs().max()) > 0.0
        N.check(N.lib().dgppo_lagr_apply(N.ptr(lg), N.ptr(sums), n * nh, C.c_int64(B * T_), C.c_float(lr), N.stream_ptr()),
                "dgppo_lagr_apply")

    for step in (update, split_update):
        lagr = lagr0.copy()
        lg = d(lagr0.copy()); sums = torch.zeros(n * nh, device=cuda)
        for lr in (0.5, 50.0):                                 # the second step drives some multipliers to the clip at 0
            step(lg, sums, lr)
            lagr = A.lagr_update(lagr.astype(f64), lp_new.astype(f64), lp_old.astype(f64), Vh[:, :T_].astype(f64), Ah.astype(f64),
                                 0.99, lr)
            got = lg.cpu().numpy()
            assert np.isfinite(got).all(), "NaN from the gap behind each env's values: wrong stride"
            np.testing.assert_allclose(got, lagr, atol=1e-5 * max(1.0, float(np.abs(lagr).max())))
            assert float(sums.abs().max()) == 0.0
        assert (lagr == 0).any() and (lagr > 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# 4. clip + Adam (dgppo_clip_adam_step)
# ----------------------------------------------------------------------------------------------------------------------
# non-default hyper-parameters, rounded to fp32 so that kernel and float64 oracle start from the same numbers
LR, B1, B2, EPS, MAX_NORM = (float(f32(v)) for v in (1e-3, 0.8, 0.99, 1e-6, 0.5))
# parameters of the size of network weights: |p| < 1, so one fp32 rounding of p is <= 3e-8 and twenty of them stay far below
# the 2e-6 bound on the parameters, which then measures the update arithmetic (at |p| > 4 twenty roundings alone reach it)
PARAM_SCALE = 0.1


def _adam_state(cuda, p):
    from dgppo_amd import _native as N
    n = p.size
    return (torch.from_numpy(p.copy()).to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda),
            torch.zeros(N.OPT_STATE_FLOATS, device=cuda))


def _adam_step(pd, g, m, v, st, scale=1.0):
    from dgppo_amd import ops_algo as O
    O.clip_adam_step(pd, g if torch.is_tensor(g) else torch.from_numpy(g).to(pd.device), m, v, st, LR, MAX_NORM, B1, B2, EPS, scale)


def _grad_with_norm(r, n, target):
    z = r.normal(size=n)
    return (z / np.sqrt((z * z).sum()) * target).astype(f32)


@pytest.mark.parametrize("n", [1, 63, 257, 62660, 262144 + 5, 3_000_001])
def test_clip_adam_sizes(cuda, n):
    """20 steps against A.clip_adam in float64: below one wave, ragged workgroup, past the 256 x 256 threads of the statistics
    grid and past the 1024 x 256 of the update grid (both stride loops); gradient norms below and above max_norm and one
    gradient whose single non-zero entry equals max_norm (norm == max_norm exactly: no clipping, fmaxf takes either)."""
    r = np.random.default_rng(n)
    p = (r.normal(size=n) * PARAM_SCALE).astype(f32)
    pd, m, v, st = _adam_state(cuda, p)
    pr, mr, vr, cr = p.astype(f64), np.zeros(n), np.zeros(n), 0
    seen = set()
    for k in range(20):
        if k == 7:
            g = np.zeros(n, f32); g[(n * 2) // 3] = MAX_NORM
        else:
            g = _grad_with_norm(r, n, MAX_NORM * (0.3 if k % 3 == 1 else 4.0))
        _adam_step(pd, g, m, v, st)
        pr, mr, vr, cr, norm, bad = A.clip_adam(pr, g, mr, vr, cr, LR, MAX_NORM, B1, B2, EPS)
        seen.add("eq" if k == 7 else ("below" if norm < MAX_NORM else "above"))
        s = st.cpu().numpy()
        assert not bad and s[5] == 0.0 and s[2] == cr == k + 1 and s[3] == k + 1
        np.testing.assert_allclose(s[4], norm, rtol=1e-5)
        if k == 7:
            assert s[4] == MAX_NORM
        np.testing.assert_allclose(pd.cpu().numpy(), pr, rtol=0, atol=2e-6)
    assert seen == {"eq", "below", "above"}
    np.testing.assert_allclose(m.cpu().numpy(), mr, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(v.cpu().numpy(), vr, rtol=1e-4, atol=1e-10)


@pytest.mark.parametrize("n", [257, 262144 + 5])
def test_clip_adam_grad_scale_and_determinism(cuda, n):
    """gradients 4 g with grad_scale = 0.25 give the bits of g with grad_scale = 1 (a power of two scales exactly), and the
    same inputs twice give the same bits: the norm is reduced in a fixed order (the header's promise to the data-parallel
    replicas)."""
    r = np.random.default_rng(n + 1)
    p = (r.normal(size=n) * PARAM_SCALE).astype(f32)
    runs = [_adam_state(cuda, p) for _ in range(3)]
    for k in range(5):
        g = _grad_with_norm(r, n, MAX_NORM * (0.3 if k == 1 else 4.0))
        gd = torch.from_numpy(g).to(cuda)
        _adam_step(runs[0][0], gd, *runs[0][1:])
        _adam_step(runs[1][0], gd, *runs[1][1:])
        _adam_step(runs[2][0], 4 * gd, *runs[2][1:], scale=0.25)
        torch.cuda.synchronize()
        for other, what in ((runs[1], "repeat"), (runs[2], "grad_scale")):
            for a, b, nm in zip(runs[0][:3], other[:3], ("params", "m", "v")):
                assert torch.equal(a, b), f"{what}: {nm} differ at step {k}"
            assert torch.equal(runs[0][3][2:6], other[3][2:6]), f"{what}: state[2..5] differ at step {k}"


@pytest.mark.parametrize("n", [63, 262144 + 5])
def test_clip_adam_non_finite_and_overflowing_gradients(cuda, n):
    """+inf, -inf and NaN each skip the step (optax.apply_if_finite: parameters and moments keep their bits, the Adam count
    stays, the step counter and the flag move) and the next finite step continues from the old count.  FINITE entries whose
    squares overflow fp32 (1e20) are not a skip: trainer/utils.py:109-118 gets norm = inf, divides by it and takes a counted
    Adam step with a zero gradient."""
    r = np.random.default_rng(n + 2)
    p = (r.normal(size=n) * PARAM_SCALE).astype(f32)
    pd, m, v, st = _adam_state(cuda, p)
    pr, mr, vr, cr = p.astype(f64), np.zeros(n), np.zeros(n), 0
    total = 0

    def finite_step(g, g_ref=None):
        nonlocal pr, mr, vr, cr, total
        _adam_step(pd, g, m, v, st)
        pr, mr, vr, cr, norm, bad = A.clip_adam(pr, g if g_ref is None else g_ref, mr, vr, cr, LR, MAX_NORM, B1, B2, EPS)
        total += 1
        s = st.cpu().numpy()
        assert not bad and s[5] == 0.0 and s[2] == cr and s[3] == total
        np.testing.assert_allclose(pd.cpu().numpy(), pr, rtol=0, atol=2e-6)
        return s

    for k in range(3):
        finite_step(_grad_with_norm(r, n, MAX_NORM * 4.0))
    for bad_value in (np.inf, -np.inf, np.nan):
        keep = [t.clone() for t in (pd, m, v)]
        g = _grad_with_norm(r, n, MAX_NORM * 4.0)
        g[n // 2] = bad_value
        _adam_step(pd, g, m, v, st)
        total += 1
        s = st.cpu().numpy()
        assert s[5] == 1.0 and s[2] == cr and s[3] == total
        for a, b, nm in zip((pd, m, v), keep, ("params", "m", "v")):
            assert torch.equal(a, b), f"{nm} changed on a {bad_value} gradient"
        finite_step(_grad_with_norm(r, n, MAX_NORM * 0.3))
    g = _grad_with_norm(r, n, MAX_NORM * 4.0)
    g[::3] = 1e20
    with np.errstate(over="ignore"):
        assert np.isfinite(g).all() and np.isinf((g * g).sum(dtype=f32))
    s = finite_step(g, g_ref=np.zeros(n))
    assert np.isposinf(s[4])
    s = finite_step(_grad_with_norm(r, n, MAX_NORM * 4.0))
    np.testing.assert_allclose(m.cpu().numpy(), mr, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(v.cpu().numpy(), vr, rtol=1e-4, atol=1e-10)


# ----------------------------------------------------------------------------------------------------------------------
# 5. small elementwise entry points
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 65536 + 1])
def test_value_loss(cuda, count):
    """optax.l2_loss(v, target).mean() (informarl.py:374): stats[0] += sum 1/2 (v - t)^2 onto a non-zero start, dv within one
    ulp of (v - t) / count; 65 537 elements = 257 workgroups over the grid of 256 (stride loop)."""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(count)
    v, t = torch.randn(count, generator=g), torch.randn(count, generator=g)
    dv = torch.full((count,), float("nan"), device=cuda)
    stats = torch.zeros(8, device=cuda)
    stats[0] = 3.0
    K_.value_loss(v.to(cuda), t.to(cuda), dv, stats)
    torch.cuda.synchronize()
    d = v.double() - t.double()
    _close(stats[0].cpu() - 3.0, (0.5 * d * d).sum(), 1e-5, "value loss sum")
    _close((stats[0].cpu() - 3.0) / count, (0.5 * d * d).mean(), 1e-5, "value loss mean")
    assert float(stats[1:].abs().max()) == 0.0
    # v - t of two fp32 numbers is one IEEE operation, the same on both sides; the quotient is what is measured
    want = (v - t).double() / count
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(f32))).double()
    err = (dv.cpu().double() - want).abs()
    print(f"value_loss dv: max err {float((err / ulp).max()):.3f} ulp")
    assert (err <= ulp).all()


@pytest.mark.parametrize("G,n,D", [(1, 1, 2), (37, 3, 64), (4096, 16, 64)])
def test_mean_agents(cuda, G, n, D):
    """value.py:33 and its backward: forward mean over agents, backward 1 (dP / n, optionally through a ReLU mask) and
    backward 2 (broadcast-add onto existing content).  The backward forms are one IEEE operation per element: exact."""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(G + n + D)
    x = torch.randn(G * n, D, generator=g)
    y = torch.full((G, D), float("nan"), device=cuda)
    K_.mean_agents(x.to(cuda), y, G, n, D)
    _close(y, x.double().view(G, n, D).mean(1), 1e-5, "mean_agents forward")
    dP = torch.randn(G, D, generator=g).to(cuda)
    mask = torch.randn(G * n, D, generator=g)
    mask[::5, ::3] = 0.0
    mask[1::7, 1::4] = float("nan")                            # not > 0: masked
    mask = mask.to(cuda)
    wide = dP[:, None, :].expand(G, n, D).reshape(G * n, D)
    zero = torch.zeros(G * n, D, device=cuda)
    quot = torch.from_numpy(wide.cpu().numpy() / f32(n)).to(cuda)      # the IEEE quotient (numpy divides; it does not scale by 1 / n)
    b1 = torch.full((G * n, D), float("nan"), device=cuda)
    K_.mean_agents(dP, b1, G, n, D, backward=1)
    assert torch.equal(b1, quot)
    b1m = torch.full((G * n, D), float("nan"), device=cuda)
    K_.mean_agents(dP, b1m, G, n, D, backward=1, relu_mask=mask)
    assert torch.equal(b1m, torch.where(mask > 0, quot, zero))
    base = torch.randn(G * n, D, generator=g).to(cuda)
    b2 = base.clone()
    K_.mean_agents(dP, b2, G, n, D, backward=2)
    assert torch.equal(b2, base + wide)
    b2m = base.clone()
    K_.mean_agents(dP, b2m, G, n, D, backward=2, relu_mask=mask)
    assert torch.equal(b2m, torch.where(mask > 0, base + wide, zero))


def test_relu_bwd_edge_values(cuda):
    """dx = dy * (y > 0), in place: +0, -0 and NaN are not > 0, a positive subnormal is"""
    from dgppo_amd import ops_nn as K_
    g = torch.Generator().manual_seed(2)
    count = 70001
    y = torch.randn(count, generator=g)
    special = torch.tensor([0.0, -0.0, float("nan"), 1e-40, -1e-40, 1.4e-45, float("inf"), -float("inf")])
    y[:8 * 100] = special.repeat(100)
    y[-8:] = special
    dy = torch.randn(count, generator=g)
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert want[3] == dy[3] and want[5] == dy[5] and want[0] == 0 and want[2] == 0, "the CPU reference keeps subnormals"
    dyd = dy.to(cuda)
    K_.relu_bwd(dyd, y.to(cuda))
    assert torch.equal(dyd.cpu(), want)
