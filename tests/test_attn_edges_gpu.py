"""The five attention kernel families (attn_slot8.hip, attn_bd.hip, attn_wg.hip MFMA and VALU, attn_tiled.hip) where unit-scale
operands, a live slot per receiver and H = 3 / Kp % 4 == 0 never take them: saturated, tied and one-hot softmax rows on exactly
representable operands, receivers without any live slot and with exactly one, head counts 1..8, padded and odd widths of zcat,
and the refusals of the entry points.  Every comparison is against float64 (oracle/nn_torch.py attn_fixed_fan_in and its
autograd) at the suite's 2e-5 of the output scale; no number here comes from the kernels.

Which family a call takes is decided by attn_family (attn.hip) from the shape alone; _family below restates it, and every case
asserts the families its docstring names, so that a case cannot land on another kernel unnoticed."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_large_team_gpu import _image_bytes  # noqa: E402
from test_nn_gpu import _attn_check, _attn_inputs, _attn_materialise_xo, _attn_reference, _attn_run, _attn_run_xo  # noqa: E402

pytestmark = pytest.mark.gpu
LS, LBT, VMAS = 0, 2, 10          # LidarSpread, LidarBicycleTarget, VMASReverseTransport


def _cfg(kind, n, n_obs):
    from dgppo_amd import _native as N
    return N.make_env_cfg(kind, n, n_obs)


def _kp(F, H, extra=0):
    """the smallest width of zcat the one-wave and MFMA families take: F + H (F + 4) + 1 rounded up to 4 (+ extra)"""
    return (F + H * (F + 4) + 1 + 3) // 4 * 4 + extra


# ---- attn_family (attn.hip), restated -----------------------------------------------------------------------------------
def _mfma_smem(cfg, F, H, bwd):
    n, S, Ns = cfg.n_agents, cfg.fan_in, cfg.num_nodes - 1
    RT, CT = (n * H + 15) // 16, (Ns + 15) // 16
    fl = CT * 16 * (F + 1) + RT * 16 * (F + 1) + RT * 16 * (CT * 16 + 1) + 8 + n * S * 5 + 2 * n * H * ((S + 3) // 4 * 4)
    if bwd:
        fl += RT * 16 * (CT * 16 + 1) + RT * 16 * (F + 5)
    return 4 * fl


def _bd_shape(cfg, F, H):
    """(PS, hits, AB) of the block-diagonal instantiation, or None (attn_bd_shape in attn_bd.hip)"""
    n, Ns = cfg.n_agents, cfg.num_nodes - 1
    if F != 32 or not 1 <= H <= 4 or n > 16:
        return None
    n_priv = Ns - n - cfg.n_goals
    hits = cfg.is_lidar and n_priv > 0
    if hits and (cfg.obs_slots != 8 or n_priv != n * 8):
        return None
    PS = ((n + cfg.n_goals if hits else Ns) + 7) // 8
    return (PS, hits, (n + 7) // 8) if 1 <= PS <= 4 else None


def _family(cfg, F, H, Kp, bwd=False, dXa=False):
    if _image_bytes(cfg, F, H, bwd) > 64 * 1024:
        return "TILED"
    if Kp % 4 == 0 and F == 8 and H == 3 and cfg.n_agents <= 32 and cfg.fan_in <= 64 and not (bwd and dXa):
        return "SLOT8"
    if Kp % 4 == 0 and _bd_shape(cfg, F, H) is not None:
        return "BD"
    if F % 4 == 0 and Kp % 4 == 0 and cfg.fan_in <= 64 and _mfma_smem(cfg, F, H, bwd) <= 64 * 1024 and (not bwd or F >= 16):
        return "MFMA"
    return "VALU"


def _families(cfg, F, H, Kp):
    """families of the forward, the backward with input gradients and the dqt-only backward, e.g. "SLOT8/VALU/SLOT8" """
    return "/".join((_family(cfg, F, H, Kp), _family(cfg, F, H, Kp, True, True), _family(cfg, F, H, Kp, True, False)))


def _run(cfg, F, H, Kp, G, inp, dev):
    got = _attn_run(cfg, F, H, Kp, G, inp, dev)
    if inp.get("Xo_raw") is not None:
        got.update(_attn_run_xo(cfg, F, H, Kp, G, inp, dev))
    return got


def _pad_columns_zero(got, F, H):
    kc = F + H * (F + 4)
    for k in ("z", "z@xo"):
        if k in got:
            assert (got[k][:, kc + 1:] == 0).all(), f"{k}: columns past the constant are not 0"


# ======================================================================================================================
# 2. saturated, tied and one-hot softmax rows on exactly representable operands
# ======================================================================================================================
def _tied_inputs(cfg, F, H, Kp, G, seed, xo):
    """operands on the exact grid of _attn_inputs (qt in [-4, 4], [-8, 8] at F <= 8; uniform, but every fourth receiver's query
    rows are -q, 0 or q, which brings logits of 100 within reach of the narrow layers), masks with p = 0.3 (first slot kept, NaN
    edge features behind them), and in every graph two exact ties: agent row a0 copied onto agent row a1 (both slots forced live
    at every receiver) and hit row m0 of one agent copied onto its hit row m1 (both forced live).  Returns the operands and the
    tied pairs [K, 3] = (receiver row g * n + i, slot, slot)."""
    n, S, ng = cfg.n_agents, cfg.fan_in, cfg.n_goals
    n_other = cfg.num_nodes - 1 - n
    gen = torch.Generator().manual_seed(seed)
    em = (torch.rand(G, n, S, generator=gen) > 0.3).float()
    em[:, :, 0] = 1.0
    pick = lambda hi: [int(v) for v in torch.randperm(hi, generator=gen)[:2]]
    ties, copies = [], []
    for g in range(G):
        (a0, a1), (m0, m1), ih = pick(n), pick(8), int(torch.randint(0, n, (1,), generator=gen))
        em[g, :, a0] = em[g, :, a1] = 1.0
        h0, h1 = n + cfg.goal_slots + m0, n + cfg.goal_slots + m1
        em[g, ih, h0] = em[g, ih, h1] = 1.0
        ties += [(g * n + i, a0, a1) for i in range(n)] + [(g * n + ih, h0, h1)]
        copies.append((g * n + a0, g * n + a1, g * n_other + ng + ih * 8 + m0, g * n_other + ng + ih * 8 + m1))
    q = 8 if F <= 8 else 4
    inp = _attn_inputs(cfg, F, H, Kp, G, gen, 0.3, em=em, grid=q, xo=xo)
    inp["qt"][::4] = q * torch.sign(inp["qt"][::4])                # every fourth receiver asks at the ends of the range
    other = inp["Xo_raw"] if xo else inp["Xo"]
    for xa0, xa1, o0, o1 in copies:
        inp["Xa"][xa1] = inp["Xa"][xa0]
        other[o1] = other[o0]
    if xo:
        _attn_materialise_xo(inp)
    return inp, torch.tensor(ties)


def _saturation(want, inp, ties):
    """what keeps a case from being vacuous, from the float64 reference alone"""
    live = inp["em"].bool()[..., None].expand_as(want["at"])
    a, lg = want["at"][live], want["logits"][live]
    tied = want["at"][ties[:, 0], ties[:, 1]]
    return {"largest |logit| >= 100": float(lg.abs().max()) >= 100.0,
            "a row one-hot to 1e-12": bool((want["at"].max(1).values >= 1.0 - 1e-12).any()),
            "a live weight below 1e-45": bool((a < 1e-45).any()),
            ">= 1 % of the live weights in (1e-3, 0.999)": float(((a > 1e-3) & (a < 0.999)).double().mean()) >= 0.01,
            "a tied pair of weight >= 0.1": bool((tied >= 0.1).any()),
            "every reference output finite": all(bool(torch.isfinite(v).all()) for v in want.values())}


def _check_saturated(cfg, F, H, Kp, G, seed, xo, dev, name):
    inp, ties = _tied_inputs(cfg, F, H, Kp, G, seed, xo)
    want = _attn_reference(cfg, F, H, Kp, G, inp)
    held = _saturation(want, inp, ties)
    assert all(held.values()), (name, held)                       # before any kernel call
    assert torch.equal(want["logits"].float().double(), want["logits"]), "the logits are not exact in fp32"
    got = _run(cfg, F, H, Kp, G, inp, dev)
    _attn_check(got, want, name)                                   # finite, and 2e-5 of the output scale
    for k in ("at", "at@xo"):
        if k in got:
            at = got[k].cpu()
            # equal logits (exact in fp32 whatever the order), one maximum, one exp, one 1 / den per (receiver, head): equal bits
            assert torch.equal(at[ties[:, 0], ties[:, 1]], at[ties[:, 0], ties[:, 2]]), f"{name} {k}: tied weights differ"
            assert float((at.double().sum(1) - 1.0).abs().max()) <= 2e-5, f"{name} {k}: live weights do not sum to 1"
    _pad_columns_zero(got, F, H)


# (id, kind, n, n_obs, F, Kp, _xo entry points too, families fwd / bwd / dqt-only bwd, seed at G = 5, seed at G = 1)
SATURATED = [
    ("slot8", LS, 8, 3, 8, 48, False, "SLOT8/VALU/SLOT8", 1, 2),
    ("bd", LS, 8, 3, 32, 144, True, "BD/BD/BD", 1, 1),
    ("bd-ab2", LBT, 16, 8, 32, 144, True, "BD/BD/BD", 1, 1),
    ("mfma", LS, 8, 3, 16, 80, False, "MFMA/MFMA/MFMA", 1, 3),
    ("mfma-valu", LS, 8, 3, 12, 64, False, "MFMA/VALU/VALU", 4, 8),
    ("valu", LS, 8, 3, 6, 40, False, "VALU/VALU/VALU", 1, 2),
    ("f64", LS, 8, 3, 64, 272, False, "MFMA/VALU/VALU", 1, 1),
    ("tiled8", LS, 27, 3, 8, 48, False, "TILED/TILED/TILED", 1, 1),
    ("tiled32", LS, 27, 3, 32, 144, False, "TILED/TILED/TILED", 1, 1),
]


@pytest.mark.parametrize("G", [5, 1])
@pytest.mark.parametrize("case", SATURATED, ids=[c[0] for c in SATURATED])
def test_saturated_tied_and_one_hot_softmax(cuda, case, G):
    """Every family, forward and backward, on operands whose logits are the same numbers in fp32 and float64 (integers times
    multiples of 1/4): logits beyond +-100 (exp overflows at 88.7 without the max subtraction), rows that are one-hot to 1e-12,
    live weights that underflow in fp32, and exact ties.  Families by shape, at H = 3: LidarSpread (8, 3) F = 8 SLOT8 forward and
    dqt-only backward, VALU backward with dXa; F = 32 BD with the _xo triple, also at LidarBicycleTarget (16, 8) (AB = 2);
    F = 16 MFMA both ways; F = 12 MFMA forward, VALU backward; F = 6 VALU; F = 64 (logits reach 200) MFMA forward and, its
    backward image being 67 KB, VALU backward; LidarSpread (27, 3), the smallest team whose four passes all exceed the 64 KB
    image, TILED at F = 8 and F = 32.  Asserted on the float64 reference before any launch: see _saturation.  Then: finite,
    2e-5 of the scale, tied weights bit-equal, live weights summing to 1 within 2e-5, zeros past the constant column."""
    name, kind, n, n_obs, F, Kp, xo, fams, seed5, seed1 = case
    cfg, H = _cfg(kind, n, n_obs), 3
    assert _families(cfg, F, H, Kp) == fams
    if xo:
        from dgppo_amd import ops_nn as K_
        assert K_.attn_xo_supported(cfg, F, H, Kp)
    _check_saturated(cfg, F, H, Kp, G, seed5 if G == 5 else seed1, xo, cuda, f"{name} G={G}")


def test_saturated_persistent_forward(cuda):
    """LidarSpread (2, 1), F = 32, G = 4 * 16 * CUs + 2: the persistent block-diagonal forward (its own copy of the softmax, see
    test_attention_persistent_forward for the bound on G), plain and with recomputed rows, held to float64 directly on the
    saturated, tied operands, and bit-equal to its 512-graph chunks, which take the one-graph-per-wave kernel.  A second set of
    operands (randn) has receivers whose only live slot is one goal slot: weight exactly 1 there."""
    from dgppo_amd import ops_nn as K_
    cfg, F, H, Kp = _cfg(LS, 2, 1), 32, 3, 144
    n, S = cfg.n_agents, cfg.fan_in
    n_other = cfg.num_nodes - 1 - n
    assert _families(cfg, F, H, Kp) == "BD/BD/BD" and _bd_shape(cfg, F, H) == (1, True, 1) and K_.attn_xo_supported(cfg, F, H, Kp)
    G = 4 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 2
    inp, ties = _tied_inputs(cfg, F, H, Kp, G, 11, True)
    want = _attn_reference(cfg, F, H, Kp, G, inp)
    held = _saturation(want, inp, ties)
    assert all(held.values()), held
    em1 = (torch.rand(G, n, S, generator=torch.Generator().manual_seed(12)) > 0.3).float()
    em1[:, :, 0] = 1.0
    single = torch.zeros(G, n, dtype=torch.bool)
    single[torch.arange(G), torch.arange(G) % n] = torch.arange(G) % 3 == 0
    em1[single] = 0.0
    goal = (n + torch.arange(G) % cfg.goal_slots)[:, None].expand(G, n)
    em1[single, goal[single]] = 1.0
    inp1 = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(13), 0.3, em=em1, xo=True)
    want1 = _attn_reference(cfg, F, H, Kp, G, inp1)
    for tag, ops, ref in (("saturated", inp, want), ("single goal slot", inp1, want1)):
        d = {k: v.to(cuda) for k, v in ops.items()}

        def fwd(g0, g1, fused):
            z = torch.full(((g1 - g0) * n, Kp), float("nan"), device=cuda)
            at = torch.full(((g1 - g0) * n, S, H), float("nan"), device=cuda)
            r, o = slice(g0 * n, g1 * n), slice(g0 * n_other, g1 * n_other)
            if fused:
                K_.attn_fwd_xo(cfg, F, H, Kp, d["qt"][r], d["Xa"][r], d["Xo_raw"][o], d["Wo"], d["bo"], d["ef"][r], d["em"][r], z, at, g1 - g0)
            else:
                K_.attn_fwd(cfg, F, H, Kp, d["qt"][r], d["Xa"][r], d["Xo"][o], d["ef"][r], d["em"][r], z, at, g1 - g0)
            return z, at

        for fused in (False, True):
            z, at = fwd(0, G, fused)
            zc, atc = zip(*(fwd(g0, min(g0 + 512, G), fused) for g0 in range(0, G, 512)))
            torch.cuda.synchronize()
            _attn_check({"z": z, "at": at}, ref, f"persistent {tag} fused={fused}")
            assert torch.equal(z, torch.cat(zc)) and torch.equal(at, torch.cat(atc)), f"persistent forward differs ({tag}, fused={fused})"
            at = at.cpu()
            assert float((at.double().sum(1) - 1.0).abs().max()) <= 2e-5
            if ops is inp:
                assert torch.equal(at[ties[:, 0], ties[:, 1]], at[ties[:, 0], ties[:, 2]]), "tied weights differ"
            else:
                rows = single.reshape(-1)
                assert int(rows.sum()) > G // 4
                assert torch.equal(at[rows], em1.reshape(G * n, S)[rows][..., None].expand(-1, -1, H)), "single live slot: weight not 1 / 0"


# ======================================================================================================================
# 3. receivers with no live slot, and with exactly one
# ======================================================================================================================
def _exact_rows(cfg, F, H, Kp, got, want, em, name):
    """the exact statements about dead receivers (no live slot) and single receivers (one live slot) in every output of a run"""
    S = cfg.fan_in
    em = em.reshape(-1, S)
    dead, single = em.sum(1) == 0, em.sum(1) == 1
    kc = F + H * (F + 4)
    for k, v in got.items():
        v, out = v.cpu(), k.split("@")[0]
        if out == "at":
            assert (v[dead] == 0).all(), f"{name} {k}: a dead receiver has attention"
            assert torch.equal(v[single], em[single][..., None].expand(-1, -1, H)), f"{name} {k}: single live slot: weight not 1 / 0"
        elif out == "z":
            assert (v[dead][:, F:kc] == 0).all(), f"{name} {k}: a dead receiver has an aggregate"
            assert torch.equal(v[:, kc], want["z"][:, kc].float()), f"{name} {k}: constant column"
            assert (v[:, kc + 1:] == 0).all(), f"{name} {k}: pad columns"
            assert torch.equal(v[:, :F], want["z"][:, :F].float()), f"{name} {k}: z[:, :F] is not the receiver's own row"
        elif out in ("dq", "dq_only"):
            assert (v[dead] == 0).all(), f"{name} {k}: a dead receiver has a query gradient"
            assert (v[single] == 0).all(), f"{name} {k}: a softmax over one slot has a gradient"
    return int(dead.sum()), int(single.sum())


def _vmas_masks(n, G, gen):
    """goal-less topology, S = n: per graph receivers (i + g) % 3 == 0 are dead, == 1 have one live slot, the rest are random
    (p = 0.3); from n = 9 the whole first 8-agent group is dead in graph 0 and the whole second one in graph 1"""
    em = (torch.rand(G, n, n, generator=gen) > 0.3).float()
    for g in range(G):
        for i in range(n):
            if (i + g) % 3 == 0:
                em[g, i] = 0.0
            elif (i + g) % 3 == 1:
                em[g, i] = 0.0
                em[g, i, (5 * i + g) % n] = 1.0
    if n >= 9:
        em[0, :8] = 0.0
        em[1, 8:] = 0.0
    return em


@pytest.mark.parametrize("F,Kp", [(8, 48), (32, 144), (16, 80), (6, 40)])
@pytest.mark.parametrize("n", [1, 3, 9, 16])
def test_dead_and_single_slot_receivers_without_goal_slots(cuda, n, F, Kp):
    """VMASReverseTransport (agent slots only, S = Ns = n), the one kind whose receivers can lose every slot: dead receivers, receivers
    with one live slot and random ones share an 8-agent group (a -INFINITY maximum next to finite ones in one lane group); at
    n = 9 and 16 a whole 8-agent group is dead.  Families at H = 3: F = 8 SLOT8 (VALU for the backward with dXa), F = 32 BD with
    PS = AB = 1 (n = 1, 3) and PS = AB = 2 (n = 9, 16), F = 16 MFMA, F = 6 VALU.  A dead receiver: attention, aggregate, constant
    column and dqt row exactly 0, z[:, :F] its own row; it still sends (dXa against float64).  A single live slot: weight exactly
    1.0, dqt exactly 0.  Pad columns 0 (every Kp here has two)."""
    cfg, H, G = _cfg(VMAS, n, 0), 3, 7
    assert cfg.fan_in == n and cfg.num_nodes - 1 == n and cfg.goal_slots == 0
    fams = {8: "SLOT8/VALU/SLOT8", 32: "BD/BD/BD", 16: "MFMA/MFMA/MFMA", 6: "VALU/VALU/VALU"}[F]
    assert _families(cfg, F, H, Kp) == fams
    if F == 32:
        assert _bd_shape(cfg, F, H) == ((n + 7) // 8, False, (n + 7) // 8)
    gen = torch.Generator().manual_seed(100 * n + F)
    em = _vmas_masks(n, G, gen)
    alive = em.sum(2) > 0
    if n >= 3:
        assert any(bool(alive[g, :8].any()) and not bool(alive[g, :8].all()) for g in range(G)), "no group mixes dead and live receivers"
    if n >= 9:
        assert not alive[0, :8].any() and not alive[1, 8:].any()
    inp = _attn_inputs(cfg, F, H, Kp, G, gen, 0.3, em=em)
    want = _attn_reference(cfg, F, H, Kp, G, inp)
    assert torch.equal(want["z"][:, F + H * (F + 4)], alive.reshape(-1).double())       # the corrected oracle: 0 for the dead
    got = _run(cfg, F, H, Kp, G, inp, cuda)
    _attn_check(got, want, f"VMAS n={n} F={F}")
    n_dead, n_single = _exact_rows(cfg, F, H, Kp, got, want, em, f"VMAS n={n} F={F}")
    assert n_dead >= 2 and n_single >= 2


@pytest.mark.parametrize("case", SATURATED, ids=[c[0] for c in SATURATED])
def test_single_goal_slot_receivers(cuda, case):
    """The topologies with goal slots, every family of test_saturated_tied_and_one_hot_softmax (same shapes, randn operands,
    G = 5): per graph the receivers (i + g) % 3 == 0 have every slot masked except one goal slot, the least the contract of
    dgppo_attn_fwd allows.  Weight exactly 1.0 there and 0.0 elsewhere, dqt exactly 0, constant column 1, everything against
    float64."""
    name, kind, n, n_obs, F, Kp, xo, fams, _, _ = case
    cfg, H, G = _cfg(kind, n, n_obs), 3, 5
    S = cfg.fan_in
    assert _families(cfg, F, H, Kp) == fams and cfg.goal_slots >= 1
    gen = torch.Generator().manual_seed(7 * n + F)
    em = (torch.rand(G, n, S, generator=gen) > 0.3).float()
    em[:, :, 0] = 1.0
    for g in range(G):
        for i in range(n):
            if (i + g) % 3 == 0:
                em[g, i] = 0.0
                em[g, i, n + (i + g) % cfg.goal_slots] = 1.0
    inp = _attn_inputs(cfg, F, H, Kp, G, gen, 0.3, em=em, xo=xo)
    want = _attn_reference(cfg, F, H, Kp, G, inp)
    assert (want["z"][:, F + H * (F + 4)] == 1).all()
    got = _run(cfg, F, H, Kp, G, inp, cuda)
    _attn_check(got, want, name)
    n_dead, n_single = _exact_rows(cfg, F, H, Kp, got, want, em, name)
    assert n_dead == 0 and n_single >= G * n // 3


# ======================================================================================================================
# 4. head counts and padded widths
# ======================================================================================================================
HEADS = ([("bd", LS, 8, 3, 32, H, extra, True) for H in (1, 2, 4) for extra in (0, 8)] +
         [("bd-ab2", LBT, 16, 8, 32, 4, 0, True)] +
         [("wg", LS, 8, 3, F, H, 0, False) for F in (16, 12, 6) for H in (1, 2, 4, 8)] +
         [("wg", LS, 8, 3, 8, H, 0, False) for H in (1, 2, 4)] +
         [("tiled", LS, 27, 3, F, H, 0, False) for F in (8, 32) for H in (1, 4)])
HEAD_FAMILIES = {
    ("bd", 32): "BD/BD/BD", ("bd-ab2", 32): "BD/BD/BD",
    # H = 8 at F = 16: the backward's matrix-core image (73 KB) no longer fits, so it takes the VALU kernel
    ("wg", 16): {1: "MFMA/MFMA/MFMA", 2: "MFMA/MFMA/MFMA", 4: "MFMA/MFMA/MFMA", 8: "MFMA/VALU/VALU"},
    ("wg", 12): "MFMA/VALU/VALU", ("wg", 6): "VALU/VALU/VALU",
    ("wg", 8): "MFMA/VALU/VALU",                                   # F = 8 with H != 3 leaves SLOT8
    # LidarSpread (27, 3): at F = 8 only H >= 3 exceeds the 64 KB image (H = 4: both passes; H = 1: none, and the matrix-core image of its 270 nodes is 93 KB: VALU)
    ("tiled", 8): {1: "VALU/VALU/VALU", 4: "TILED/TILED/TILED"}, ("tiled", 32): "TILED/TILED/TILED",
}


@pytest.mark.parametrize("case", HEADS, ids=[f"{c[0]}-F{c[4]}-H{c[5]}-Kp+{c[6]}" for c in HEADS])
def test_head_counts_and_padded_widths(cuda, case):
    """attn_check admits 1 <= H <= 8 and attn_bd_shape H <= 4; every test before this file calls with H = 3.  randn operands,
    G = 5, masks with p = 0.3 (first slot kept), forward, backward with and without dXa and relu_xo, against float64.  BD and the
    _xo triple: H = 1, 2, 4 at LidarSpread (8, 3), F = 32, Kp the smallest multiple of 4 and 8 more, and H = 4 at
    LidarBicycleTarget (16, 8) (AB = 2).  MFMA / VALU: H = 1, 2, 4, 8 at F = 16, 12, 6, and F = 8 with H = 1, 2, 4, which leaves
    SLOT8.  TILED: H = 1, 4 at LidarSpread (27, 3); its receiver tile shrinks until the LDS stage holds H = 4 (16 receivers do at
    this shape: 52 KB), so the refusal "one receiver tile needs ... of LDS" is not reachable through the head count.  The
    families each (shape, H) takes are in HEAD_FAMILIES."""
    tag, kind, n, n_obs, F, H, extra, xo = case
    cfg, G, Kp = _cfg(kind, n, n_obs), 5, _kp(F, H, extra)
    fams = HEAD_FAMILIES[(tag, F)]
    assert _families(cfg, F, H, Kp) == (fams[H] if isinstance(fams, dict) else fams)
    if xo:
        from dgppo_amd import ops_nn as K_
        assert K_.attn_xo_supported(cfg, F, H, Kp)
    inp = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(1000 * F + 10 * H + extra), 0.3, xo=xo)
    got = _run(cfg, F, H, Kp, G, inp, cuda)
    _attn_check(got, _attn_reference(cfg, F, H, Kp, G, inp), f"{tag} F={F} H={H} Kp={Kp}")
    _pad_columns_zero(got, F, H)


@pytest.mark.parametrize("F,Kp", [(8, 45), (8, 47), (32, 141)])
def test_widths_that_are_no_multiple_of_four(cuda, F, Kp):
    """Kp % 4 != 0 (45 and 141 are the exact widths F + 3 (F + 4) + 1): SLOT8, BD and MFMA move zcat rows in 16-byte pieces,
    so attn_family sends these shapes to the VALU workgroup kernels, which address single floats.  Against float64, zeros in
    every column past the constant; the _xo entry points refuse F = 32 / Kp = 141 and dgppo_attn_xo_supported says 0."""
    from dgppo_amd import ops_nn as K_
    cfg, H, G = _cfg(LS, 8, 3), 3, 5
    assert _families(cfg, F, H, Kp) == "VALU/VALU/VALU"
    inp = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(Kp), 0.3)
    got = _attn_run(cfg, F, H, Kp, G, inp, cuda)
    _attn_check(got, _attn_reference(cfg, F, H, Kp, G, inp), f"F={F} Kp={Kp}")
    _pad_columns_zero(got, F, H)
    if F == 32:
        assert K_.attn_xo_supported(cfg, F, H, 144) and not K_.attn_xo_supported(cfg, F, H, Kp)
        xin = _attn_inputs(cfg, F, H, Kp, G, torch.Generator().manual_seed(Kp), 0.3, xo=True)
        with pytest.raises(ValueError, match="no fused kernel"):
            _attn_run_xo(cfg, F, H, Kp, G, xin, cuda)


def test_attention_refusals(cuda):
    """what attn_check and the entry points refuse: a negative code with a message (ValueError through the wrappers), and no
    output touched.  H = 0 and 9, F = 65, Kp one below F + H (F + 4) + 1, dXo without dXa, a NULL Xo on a topology with other
    nodes; G = 0 returns 0 and touches nothing."""
    import ctypes as C
    from dgppo_amd import _native as N, ops_nn as K_
    cfg, G = _cfg(LS, 8, 3), 2
    n, S = cfg.n_agents, cfg.fan_in
    R, n_other = G * n, cfg.num_nodes - 1 - n
    ones = lambda *shp: torch.ones(shp, device=cuda)
    nan = lambda *shp: torch.full(shp, float("nan"), device=cuda)

    def both(F, H, Kp, msg_fwd, msg_bwd, xo=True, dxa=True, dxo=True):
        Xo = ones(G * n_other, F) if xo else None
        z, at, dq, dXa, dXo = nan(R, Kp), nan(R, S, H), nan(R, H * F), nan(R, F), nan(G * n_other, F)
        if msg_fwd is not None:
            with pytest.raises(ValueError, match=msg_fwd):
                K_.attn_fwd(cfg, F, H, Kp, ones(R, H * F), ones(R, F), Xo, ones(R, S, 4), ones(R, S), z, at, G)
        with pytest.raises(ValueError, match=msg_bwd):
            K_.attn_bwd(cfg, F, H, Kp, ones(R, Kp), ones(R, S, H), ones(R, H * F), ones(R, F), Xo, ones(R, S, 4), dq,
                        dXa if dxa else None, dXo if dxo else None, G)
        torch.cuda.synchronize()
        for k, v in dict(z=z, at=at, dq=dq, dXa=dXa, dXo=dXo).items():
            assert torch.isnan(v).all(), f"{k} was touched by a refused call"

    both(8, 0, 48, "bad F=8 H=0", "bad F=8 H=0")
    both(8, 9, 128, "bad F=8 H=9", "bad F=8 H=9")
    both(65, 3, 276, "bad F=65 H=3", "bad F=65 H=3")
    both(8, 3, 44, "Kp=44 too small", "Kp=44 too small")
    both(32, 3, 140, "Kp=140 too small", "Kp=140 too small")
    both(8, 3, 48, "attn_fwd: Xo is NULL", "attn_bwd: Xo is NULL", xo=False)
    both(32, 3, 144, None, "attn_bwd: dXo needs dXa", dxa=False)
    # G = 0 through the C entry points, with buffers a G = 2 call would fill
    F, H, Kp = 32, 3, 144
    z, at, dq, dXa, dXo = nan(R, Kp), nan(R, S, H), nan(R, H * F), nan(R, F), nan(G * n_other, F)
    p = N.ptr
    rc_f = N.lib().dgppo_attn_fwd(C.byref(cfg), F, H, Kp, p(ones(R, H * F)), p(ones(R, F)), p(ones(G * n_other, F)), p(ones(R, S, 4)),
                                  p(ones(R, S)), p(z), p(at), 0, N.stream_ptr())
    rc_b = N.lib().dgppo_attn_bwd(C.byref(cfg), F, H, Kp, p(ones(R, Kp)), p(ones(R, S, H)), p(ones(R, H * F)), p(ones(R, F)),
                                  p(ones(G * n_other, F)), p(ones(R, S, 4)), p(dq), p(dXa), p(dXo), 0, 0, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc_f == 0 and rc_b == 0
    for k, v in dict(z=z, at=at, dq=dq, dXa=dXa, dXo=dXo).items():
        assert torch.isnan(v).all(), f"{k} was touched by a G = 0 call"
