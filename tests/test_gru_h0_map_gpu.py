"""The carry map of the one-step GRU passes (dgppo_gru_fwd_h0_map, dgppo_gru_bwd_w_t1_map): sequence s = (cell c, agent a),
cell c = (e, t), carry at base + env * env_stride + t * time_stride + a * 64 with env = ids[e] or e — against the same calls on
the dense carry that torch.index_select builds from the same record.  Data movement only: hs, gates and dgi must be bit-equal,
and so must dWi, dWh, dbi, dbhn while at most two workgroups add into zeroed outputs (a + b == b + a; asserted per case).

The record has 5 envs x 4 time slots, slot 0 filled with NaN and the map's base at slot 1 (3 usable slots), time-major
[4, 5, n, 64] or env-major [5, 4, n, 64]; ids = a prefix of a permutation (3 envs), the identity (5), a list of 24 with repeats,
or none.  Sequence counts 27 / 32 / 70 where n_inner divides them (the library refuses other counts), else the neighbouring
multiples: a ragged last 16-row tile, whole tiles, several tiles; a map smaller than the smallest count is used in full.  One
larger case reaches the 32-row tiles with more than one tile per workgroup."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
H = 64
N_ENV, N_SLOT, N_TIME = 5, 4, 3
COUNTS = {1: (27, 32, 70), 3: (27, 48, 69), 8: (24, 32, 72)}


def _ids(kind, cuda, n=24):
    g = torch.Generator().manual_seed(11)
    if kind == "none":
        return None
    if kind == "identity":
        ids = torch.arange(N_ENV)
    elif kind == "perm-prefix":
        ids = torch.randperm(N_ENV, generator=g)[:3]
    else:                                                   # "repeated"
        ids = torch.randint(0, N_ENV, (n,), generator=g)
        ids[1] = ids[0]                                     # a repeat for certain
    return ids.to(torch.int32).to(cuda)


def _record(cuda, layout, n_inner):
    """(record tensor, base view at slot 1 as [env, time, n, 64] whatever the layout)"""
    g = torch.Generator().manual_seed(5 + n_inner)
    if layout == "time-major":
        rec = torch.randn(N_SLOT, N_ENV, n_inner, H, generator=g)
        rec[0] = float("nan")
        rec = rec.to(cuda)
        return rec, rec[1:].transpose(0, 1)
    rec = torch.randn(N_ENV, N_SLOT, n_inner, H, generator=g)
    rec[:, 0] = float("nan")
    rec = rec.to(cuda)
    return rec, rec[:, 1:]


def _map_and_dense(K, cuda, layout, n_inner, ids_kind, n_ids=24):
    rec, view = _record(cuda, layout, n_inner)              # view [env, time, n, 64], a strided window of rec
    ids = _ids(ids_kind, cuda, n_ids)
    n_env = N_ENV if ids is None else int(ids.numel())
    m = K.H0Map(view, view.stride(0), view.stride(1), N_TIME, n_inner, n_env, ids=ids, n_env_src=N_ENV)
    dense = view if ids is None else torch.index_select(view, 0, ids.long())
    dense = dense.reshape(-1, H).contiguous()
    assert not torch.isnan(dense).any()
    return rec, m, dense


def _weights(cuda):
    g = torch.Generator().manual_seed(7)
    return (0.3 * torch.randn(H, 192, generator=g)).to(cuda), (0.1 * torch.randn(H, generator=g)).to(cuda)


def _bits_equal(a, b, what):
    assert not torch.isnan(b).any(), f"{what}: the dense reference holds NaN"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what} differs"


def _compare(K, cuda, m, dense, n_seq, n_inner, label, weight_grads=True):
    Wh, bhn = _weights(cuda)
    g = torch.Generator().manual_seed(n_seq)
    gi = torch.randn(n_seq, 192, generator=g).to(cuda)
    x = torch.randn(n_seq, H, generator=g).to(cuda)
    dhs = torch.randn(n_seq, H, generator=g).to(cuda)
    h0d = dense[:n_seq].contiguous()
    fwd, bwd = [], []
    for h0 in (m, h0d):
        hs = torch.full((n_seq, H), float("nan"), device=cuda)
        gates = torch.full((n_seq, 4 * H), float("nan"), device=cuda)
        if h0 is m:
            K.gru_fwd_h0_map(gi, Wh, bhn, m, hs, None, gates, n_seq, 1, n_inner)
        else:
            K.gru_fwd(gi, Wh, bhn, h0d, hs, None, gates, n_seq, 1, n_inner)
        fwd.append((hs, gates))
    _bits_equal(fwd[0][0], fwd[1][0], f"{label}: hs")
    _bits_equal(fwd[0][1], fwd[1][1], f"{label}: gates")
    gates = fwd[1][1]
    wsbuf = torch.empty(16 << 20, device=cuda)
    owed = []
    for h0 in (m, h0d, h0d):                        # the dense form twice: is it reproducible at this size?
        dgi = torch.full((n_seq, 192), float("nan"), device=cuda)
        dW = (torch.zeros(H, 192, device=cuda), torch.zeros(192, device=cuda), torch.zeros(H, 192, device=cuda),
              torch.zeros(H, device=cuda))
        with K.BwdWBatch(cuda, lambda n: wsbuf) as batch:
            K.gru_bwd_w_t1(x, h0, dhs, gates, dgi, *dW)
            owed.append(len(batch.descs))          # slab reductions the launcher left to a second stage
        bwd.append((dgi,) + dW)
    torch.cuda.synchronize()
    _bits_equal(bwd[0][0], bwd[1][0], f"{label}: dgi")
    if weight_grads:
        # precondition of bit-equal weight gradients, asked of the launcher and of the reference, not assumed: no second stage is
        # owed (it adds straight into the zeroed outputs, which it does for a few workgroups of at least 64 rows: two addends
        # per element up to 128 rows, whose sum does not depend on their order), and the dense form repeats its own bits
        assert owed == [0, 0, 0], f"{label}: the pass split its sums over a second stage: {owed}"
        assert n_seq <= 128
        for nm, a, b in zip(("dWi", "dbi", "dWh", "dbhn"), bwd[1][1:], bwd[2][1:]):
            _bits_equal(a, b, f"{label}: dense form twice: {nm}")
        for nm, a, b in zip(("dWi", "dbi", "dWh", "dbhn"), bwd[0][1:], bwd[1][1:]):
            _bits_equal(a, b, f"{label}: {nm}")
    else:
        # many workgroups, sums in slabs and a second stage: the same addends, possibly in another order.  1e-5 of the scale is
        # far above the float32 rounding of 54 000 reordered addends and far below what a wrong row would give
        for nm, a, b in zip(("dWi", "dbi", "dWh", "dbhn"), bwd[0][1:], bwd[1][1:]):
            scale = max(1.0, float(b.abs().max()))
            assert float((a - b).abs().max()) <= 1e-5 * scale, (label, nm, float((a - b).abs().max()), scale)


def _cases():
    out = []
    for n_inner in (1, 3, 8):
        for layout in ("time-major", "env-major"):
            for ids_kind in ("perm-prefix", "identity", "repeated", "none"):
                cap = {"perm-prefix": 3, "identity": N_ENV, "repeated": 24, "none": N_ENV}[ids_kind] * N_TIME * n_inner
                counts = [c for c in COUNTS[n_inner] if c <= cap] or [cap]
                for c in counts:
                    out.append(pytest.param(n_inner, layout, ids_kind, c, id=f"n{n_inner}-{layout}-{ids_kind}-{c}"))
    return out


@pytest.mark.parametrize("n_inner,layout,ids_kind,n_seq", _cases())
def test_mapped_h0_equals_the_index_select_copy(cuda, n_inner, layout, ids_kind, n_seq):
    from dgppo_amd import ops_nn as K
    rec, m, dense = _map_and_dense(K, cuda, layout, n_inner, ids_kind)
    assert torch.equal(m.dense().view(torch.int32), dense.view(torch.int32))          # H0Map.dense is that copy too
    _compare(K, cuda, m, dense, n_seq, n_inner, f"n_inner={n_inner} {layout} {ids_kind} n_seq={n_seq}")


@pytest.mark.parametrize("n_inner", [1, 3, 8])
def test_blocks_special_case_keeps_its_bits(cuda, n_inner):
    """env-major record without ids, time_stride = n_inner * 64: the map is H0Blocks with rows_per_block = n_time * n_inner"""
    from dgppo_amd import ops_nn as K
    rec, m, dense = _map_and_dense(K, cuda, "env-major", n_inner, "none")
    assert m.time_stride == n_inner * H
    n_seq = N_ENV * N_TIME * n_inner
    Wh, bhn = _weights(cuda)
    gi = torch.randn(n_seq, 192, generator=torch.Generator().manual_seed(3)).to(cuda)
    outs = []
    for blocks in (False, True):
        hs = torch.full((n_seq, H), float("nan"), device=cuda)
        gates = torch.full((n_seq, 4 * H), float("nan"), device=cuda)
        if blocks:
            K.gru_fwd_h0_blocks(gi, Wh, bhn, K.H0Blocks(rec[:, 1], N_TIME * n_inner, N_SLOT * n_inner * H, N_ENV), hs, None, gates,
                                n_seq, 1, n_inner)
        else:
            K.gru_fwd_h0_map(gi, Wh, bhn, m, hs, None, gates, n_seq, 1, n_inner)
        outs.append((hs, gates))
    torch.cuda.synchronize()
    _bits_equal(outs[0][0], outs[1][0], "hs")
    _bits_equal(outs[0][1], outs[1][1], "gates")


def test_large_pass_32_row_tiles_several_per_workgroup(cuda):
    """6000 ids x 3 slots x 3 agents = 54 000 sequences: 1688 tiles of 32 rows, more than the resident workgroups"""
    from dgppo_amd import ops_nn as K
    rec, m, dense = _map_and_dense(K, cuda, "time-major", 3, "repeated", n_ids=6000)
    _compare(K, cuda, m, dense, 6000 * N_TIME * 3, 3, "large", weight_grads=False)


def test_misaligned_map_is_refused_not_launched(cuda):
    from dgppo_amd import _native as N
    lib = N.lib()
    Wh, bhn = _weights(cuda)
    n, M = 3, 18
    z = lambda *s: torch.zeros(*s, device=cuda)
    gi, hs, rec, ids = z(M, 192), z(M, H), z(4, 4, n, H), torch.zeros(2, dtype=torch.int32, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    i64 = C.c_int64

    def fwd(base, es, ts):
        return lib.dgppo_gru_fwd_h0_map(p(gi), p(Wh), p(bhn), base, p(ids), 2, 3, i64(es), i64(ts), p(hs), None, None, M, n,
                                        N.stream_ptr())
    x, dhs, gates, dgi = z(M, H), z(M, H), z(M, 256), z(M, 192)
    dWi, dbi, dWh, dbhn = z(H, 192), z(192), z(H, 192), z(H)

    def bwd(base, es, ts):
        return lib.dgppo_gru_bwd_w_t1_map(p(x), H, base, p(ids), 2, 3, n, i64(es), i64(ts), p(dhs), p(gates), p(dgi), p(dWi), 192,
                                          p(dbi), p(dWh), 192, p(dbhn), M, None, i64(0), None, N.stream_ptr())
    es, ts = 4 * n * H, n * H
    for call in (fwd, bwd):
        assert call(p(rec), es, ts) == 0, lib.dgppo_last_error()
        assert call(C.c_void_p(rec.data_ptr() + 4), es, ts) == -1 and b"aligned" in lib.dgppo_last_error()
        assert call(p(rec), es + 2, ts) == -1 and b"multiples of 4" in lib.dgppo_last_error()
        assert call(p(rec), es, ts + 1) == -1 and b"multiples of 4" in lib.dgppo_last_error()
        assert call(None, es, ts) == -1
    # fewer carries in the map than sequences in the pass
    assert lib.dgppo_gru_fwd_h0_map(p(gi), p(Wh), p(bhn), p(rec), p(ids), 1, 3, i64(es), i64(ts), p(hs), None, None, M, n,
                                    N.stream_ptr()) == -1 and b"fewer" in lib.dgppo_last_error()
    torch.cuda.synchronize()
