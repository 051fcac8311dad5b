"""The rows-per-wave backward chain of the MLP trunk (mlp_gi_bwd_rw_kernel<WG>, csrc/nn_fused.hip) behind dgppo_mlp_gi_bwd_w
(WG: with the trunk's weight gradients) and dgppo_mlp_gi_bwd, and the launch rule that chooses it.

Reference and bounds are those of tests/test_trunk_bwd_w_gpu.py: the float64 autograd construction of its _case, 2e-5 for dx /
dpre*, 3e-6 sqrt(M) + 1e-6 for dW* / dbias*, 3e-5 for dg* / db*, each relative to max(1, |want|).

Launch rule (dgppo_mlp_gi_bwd_w / dgppo_mlp_gi_bwd, one place for both): the rows-per-wave form runs when M > 0 and dgi is
16-byte aligned, on min(ceil(ceil(M / 16) / 8), CUs) workgroups of 8 waves, wave w of workgroup b walking the 16-row tiles
w * grid + b, + 8 * grid, ...; every other call runs mlp_gi_bwd_kernel<WG>.  There is no M range the new form gives up.
Shapes: one tile and its edges (1, 15, 16, 17, 31, 33), one tile per wave of a workgroup and one row either side (127, 129: one
workgroup, two), and 16 (8 CUs + 3) + 5 rows: every workgroup full, three waves of the first ones with a tile more, a ragged
last tile.

Every row operand of a call is the first M rows of a buffer with 16 more: NaN in the inputs, zeros in the outputs.  A kernel that
read a row >= M instead of clamping, or let a clamped lane contribute, shows NaN in dW* / dg*; one that wrote one leaves a
non-zero row."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_trunk_bwd_w_gpu import _case, _close  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
FORMS = ["masked_x_is_mask", "masked_separate_x", "unmasked_separate_x"]
WKEYS = ("dW2", "dbias2", "dW1", "dbias1")
LKEYS = ("dg2", "db2", "dg1", "db1")


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _ms(dev):
    return [1, 15, 16, 17, 31, 33, 16 * 8 - 1, 16 * 8 + 1, 16 * (8 * _cus(dev) + 3) + 5]


def _takes_rw(dgi):
    """the launch rule: which kernel a call with this dgi runs"""
    return dgi.shape[0] > 0 and dgi.data_ptr() % 16 == 0


def _grid(M, dev):
    tiles = (M + 15) // 16
    return min((tiles + 7) // 8, _cus(dev))


def _padded(t, dev, fill, width=None, col0=0):
    """t's rows as the first rows of a device buffer with PAD more rows (and `width` columns, t at column col0), the rest `fill`"""
    M, K = t.shape
    buf = torch.full((M + PAD, width or K), fill, device=dev)
    buf[:M, col0:col0 + K] = t.to(dev)
    return buf, buf[:M, col0:col0 + K]


def _run(c, dev, form, wg, with_dpre=True, dgi_off=0, dW0=None, saves=None):
    """one call of mlp_gi_bwd_w (wg) or mlp_gi_bwd on case c; returns the outputs (views of their padded buffers under '<k>_buf'),
    the mask and the dgi tensor that was passed"""
    from dgppo_amd import ops_nn as K_
    M = c["M"]
    nan = float("nan")
    sv = {k: _padded(v, dev, nan)[1] for k, v in (saves or c["saves"]).items()}
    P = {k: v.to(dev).contiguous() for k, v in c["P"].items()}
    if dgi_off:
        flat = torch.full(((M + PAD) * 192 + 4,), nan, device=dev)
        dgi = flat[dgi_off:dgi_off + M * 192].view(M, 192)
        dgi.copy_(c["dgi"])
    else:
        dgi = _padded(c["dgi"], dev, nan)[1]
    if form == "masked_x_is_mask":
        x = mask = _padded(c["X"], dev, nan)[1]
    else:
        x = _padded(c["X"], dev, nan, width=80, col0=8)[1]
        mask = _padded(c["mask"], dev, nan)[1] if form == "masked_separate_x" else None
    o = {}
    for k in ("dx", "dpre2", "dpre1"):
        if k == "dx" or with_dpre:
            o[k + "_buf"], o[k] = _padded(torch.full((M, 64), nan), dev, 0.0)
    o.update({k: torch.zeros(64, device=dev) for k in LKEYS})
    if wg:
        for k, shp in zip(WKEYS, ((64, 64), (64,), (64, 64), (64,))):
            o[k] = dW0[k].to(dev).contiguous() if dW0 is not None else torch.zeros(*shp, device=dev)
        K_.mlp_gi_bwd_w(dgi, P["Wi"], P["W2"], P["W1"], P["g2"], P["g1"], sv["p2"], sv["y2"], sv["st2"], sv["p1"], sv["y1"],
                        sv["st1"], x, mask, o["dx"], o["dg2"], o["db2"], o["dg1"], o["db1"], o["dW2"], o["dbias2"], o["dW1"],
                        o["dbias1"], o.get("dpre2"), o.get("dpre1"))
    else:
        K_.mlp_gi_bwd(dgi, P["Wi"], P["W2"], P["W1"], P["g2"], P["g1"], sv["p2"], sv["y2"], sv["st2"], sv["p1"], sv["y1"],
                      sv["st1"], mask, o["dpre2"], o["dpre1"], o["dx"], o["dg2"], o["db2"], o["dg1"], o["db1"])
    return o, mask, dgi


def _rows_past_m_untouched(o, M):
    for k in ("dx", "dpre2", "dpre1"):
        if k + "_buf" in o:
            assert not bool(o[k + "_buf"][M:].any()), f"{k}: a row >= M was written"


def _against_float64(o, c, mask, wg, tag):
    M, w = c["M"], c["want"]
    mk = mask.cpu() if mask is not None else None
    _close(o["dx"], w["dx"] * (mk > 0) if mk is not None else w["dx"], 2e-5, f"{tag} dx")
    for k in ("dpre2", "dpre1"):
        if k in o:
            _close(o[k], w[k], 2e-5, f"{tag} {k}")
    if wg:
        for k in WKEYS:
            _close(o[k], w[k], 3e-6 * math.sqrt(M) + 1e-6, f"{tag} {k} M={M}")
    for k in LKEYS:
        _close(o[k], w[k], 3e-5, f"{tag} {k} M={M}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mi", range(9))
def test_rows_per_wave_chain(cuda, mi, form):
    """WG with and without the dpre outputs and the chain alone, all three through the rows-per-wave kernel: float64 bounds,
    dx / dpre* bit-equal between the three, dg* / db* bit-equal up to two workgroups and within the bound of a reordered sum of
    n = workgroups terms beyond, rows >= M untouched"""
    M = _ms(cuda)[mi]
    c = _case(M)
    runs = {}
    for tag, wg, with_dpre in (("w+dpre", True, True), ("w", True, False), ("chain", False, True)):
        o, mask, dgi = _run(c, cuda, form, wg, with_dpre)
        torch.cuda.synchronize()
        assert _takes_rw(dgi)
        _rows_past_m_untouched(o, M)
        _against_float64(o, c, mask, wg, f"{form} {tag}")
        runs[tag] = o
    a, b, n = runs["w+dpre"], runs["w"], runs["chain"]
    # two launches on the same inputs, and the two entry points
    assert torch.equal(a["dx"], b["dx"]) and torch.equal(a["dx"], n["dx"]), "dx differs between launches / entry points"
    for k in ("dpre2", "dpre1"):
        assert torch.equal(a[k], n[k]), f"{k} differs from mlp_gi_bwd"
    grid = _grid(M, cuda)
    for k in LKEYS:
        if grid <= 2:
            assert torch.equal(a[k], n[k]) and torch.equal(a[k], b[k]), f"{k} differs ({grid} workgroups)"
        else:
            bound = 2.0 * (grid - 1) * 2.0 ** -24 * c["sabs"][k]
            for other in (b, n):
                err = float((a[k].double() - other[k].double()).abs().max())
                print(f"{k} ({grid} workgroups): {err:.3e} bound {bound:.3e}")
                assert err <= bound, f"{k}: {err:.3e} > {bound:.3e}"
    if grid <= 2:   # one atomicAdd per workgroup and element into zeros: a defined sum
        for k in WKEYS:
            assert torch.equal(a[k], b[k]), f"{k} differs between two launches ({grid} workgroups)"


@pytest.mark.parametrize("wg", [True, False])
@pytest.mark.parametrize("mi", [3, 7, 8])
def test_misaligned_dgi_takes_the_tile_kernel(cuda, mi, wg):
    """dgi one float past a 16-byte boundary: the launch rule sends the call to mlp_gi_bwd_kernel<WG>; it meets the same float64
    bounds as the aligned call, and the two agree to the sum of both bounds"""
    M = _ms(cuda)[mi]
    c = _case(M)
    o0, mask, dgi0 = _run(c, cuda, "masked_x_is_mask", wg)
    o1, _, dgi1 = _run(c, cuda, "masked_x_is_mask", wg, dgi_off=1)
    torch.cuda.synchronize()
    assert dgi0.data_ptr() % 16 == 0 and dgi1.data_ptr() % 16 == 4
    assert _takes_rw(dgi0) and not _takes_rw(dgi1)
    for o, tag in ((o0, "aligned"), (o1, "misaligned")):
        _rows_past_m_untouched(o, M)
        _against_float64(o, c, mask, wg, tag)
    for k in ("dx", "dpre2", "dpre1"):
        _close(o1[k], o0[k].double(), 2 * 2e-5, f"misaligned vs aligned {k}")


@pytest.mark.parametrize("mi", [3, 7, 8])
def test_accumulates_immediate_and_deferred(cuda, mi):
    """dW* / dbias* add onto what they hold, at once and through a BwdWBatch flush"""
    from dgppo_amd import ops_nn as K_
    M = _ms(cuda)[mi]
    c = _case(M)
    g = torch.Generator().manual_seed(7)
    dW0 = {k: torch.randn(*shp, generator=g) for k, shp in zip(WKEYS, ((64, 64), (64,), (64, 64), (64,)))}
    tol = 3e-6 * math.sqrt(M) + 1e-6
    now, _, _ = _run(c, cuda, "masked_x_is_mask", True, False, dW0=dW0)
    torch.cuda.synchronize()
    keep = {}

    def alloc(n):
        keep["ws"] = torch.empty(n, device=cuda)
        return keep["ws"]
    with K_.BwdWBatch(cuda, alloc):
        later, _, _ = _run(c, cuda, "masked_x_is_mask", True, False, dW0=dW0)
    torch.cuda.synchronize()
    for k in WKEYS:
        _close(now[k], dW0[k].double() + c["want"][k], tol, f"immediate {k} M={M}")
        _close(later[k], dW0[k].double() + c["want"][k], tol, f"deferred {k} M={M}")
    assert torch.equal(later["dx"], now["dx"])


@pytest.mark.parametrize("wg", [True, False])
def test_dead_row_and_capped_rstd(cuda, wg):
    """a row whose y1 and y2 are all <= 0 has dx exactly 0; a constant p2 row (var = 0: rstd at its cap 1 / sqrt(1e-6)) stays
    finite; neither makes a weight or LayerNorm gradient non-finite"""
    M = 45
    c = _case(M)
    sv = {k: v.clone() for k, v in c["saves"].items()}
    dead, flat = 19, 33
    sv["y1"][dead] = 0.0
    sv["y2"][dead] = -sv["y2"][dead].abs()
    sv["p2"][flat] = 0.25
    sv["st2"][flat, 0] = 0.25
    sv["st2"][flat, 1] = 1.0 / math.sqrt(1e-6)
    o, _, dgi = _run(c, cuda, "unmasked_separate_x", wg, saves=sv)
    torch.cuda.synchronize()
    assert _takes_rw(dgi)
    assert bool((o["dx"][dead] == 0).all()), "dx of a row with no active unit is not exactly zero"
    for k in ("dx", "dpre2", "dpre1") + LKEYS + (WKEYS if wg else ()):
        assert bool(torch.isfinite(o[k]).all()), f"{k} is not finite"
    _rows_past_m_untouched(o, M)
