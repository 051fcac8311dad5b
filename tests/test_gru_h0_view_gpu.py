"""dgppo_gru_fwd_h0_blocks: the GRU scan with its initial carry read in place from a blocked buffer (sequence s at
h0 + (s / rows_per_block) * block_stride + (s % rows_per_block) * 64) equals dgppo_gru_fwd on the gathered contiguous carry,
bit for bit — hs, and gates / hprev when they are saved.  T = 1 with 1, 5 and 300 blocks of 3 and of 24 rows (one partial
16-row tile, tiles that straddle blocks, several tiles per workgroup), block_stride larger than and equal to a block; and a
T = 16 scan, whose n_inner row addressing must not notice where h0 came from."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
H = 64


def _weights(cuda):
    g = torch.Generator().manual_seed(7)
    return ((0.3 * torch.randn(H, 192, generator=g)).to(cuda), (0.1 * torch.randn(H, generator=g)).to(cuda))


def _pair(cuda, n_blocks, rpb, gap_rows, T, n_inner, save):
    """(blocked outputs, contiguous outputs) of the two entry points on the same carries"""
    from dgppo_amd import ops_nn as K
    Wh, bhn = _weights(cuda)
    n_seq, stride = n_blocks * rpb, (rpb + gap_rows) * H
    g = torch.Generator().manual_seed(n_blocks * 100 + rpb)
    buf = torch.full((n_blocks * stride,), float("nan"))                # NaN in the gaps: a stray read shows in the result
    blocks = buf.view(n_blocks, rpb + gap_rows, H)
    blocks[:, :rpb] = torch.randn(n_blocks, rpb, H, generator=g)
    buf = buf.to(cuda)
    h0_dense = buf.view(n_blocks, rpb + gap_rows, H)[:, :rpb].reshape(n_seq, H).contiguous()
    gi = torch.randn(n_seq * T, 192, generator=g).to(cuda)
    outs = []
    for blocked in (True, False):
        hs = torch.full((n_seq * T, H), float("nan"), device=cuda)
        hprev = torch.full((n_seq * T, H), float("nan"), device=cuda) if save else None
        gates = torch.full((n_seq * T, 4 * H), float("nan"), device=cuda) if save else None
        if blocked:
            K.gru_fwd_h0_blocks(gi, Wh, bhn, K.H0Blocks(buf, rpb, stride, n_blocks), hs, hprev, gates, n_seq, T, n_inner)
        else:
            K.gru_fwd(gi, Wh, bhn, h0_dense, hs, hprev, gates, n_seq, T, n_inner)
        torch.cuda.synchronize()
        outs.append((hs, hprev, gates))
    return outs


def _assert_same(outs, label):
    for name, a, b in zip(("hs", "hprev", "gates"), *outs):
        if a is None:
            assert b is None
            continue
        assert not torch.isnan(b).any(), f"{label}: the contiguous reference holds NaN in {name}"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: {name} differs"


@pytest.mark.parametrize("save", [False, True], ids=["inference", "saved"])
@pytest.mark.parametrize("gap_rows", [0, 3], ids=["stride-equal", "stride-larger"])
@pytest.mark.parametrize("rpb", [3, 24])
@pytest.mark.parametrize("n_blocks", [1, 5, 300])
def test_gru_h0_blocks_equals_contiguous_h0(cuda, n_blocks, rpb, gap_rows, save):
    _assert_same(_pair(cuda, n_blocks, rpb, gap_rows, 1, 3, save), f"{n_blocks} x {rpb} rows, gap {gap_rows}")


def test_gru_h0_blocks_keeps_n_inner_rows_for_T16(cuda):
    """T = 16, n_inner = 3: sequence s steps through rows ((s / 3) * 16 + tau) * 3 + s % 3 while its carry comes from block
    s / 6 — two groups per block"""
    _assert_same(_pair(cuda, 5, 6, 2, 16, 3, True), "T=16")


def test_gru_h0_blocks_refusals(cuda):
    import ctypes as C
    from dgppo_amd import _native as N
    lib = N.lib()
    Wh, bhn = _weights(cuda)
    gi, hs, h0 = torch.zeros(6, 192, device=cuda), torch.zeros(6, H, device=cuda), torch.zeros(8, H, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda h0p, rpb, bs: lib.dgppo_gru_fwd_h0_blocks(p(gi), p(Wh), p(bhn), h0p, rpb, C.c_int64(bs), p(hs), None, None, 6, 1, 3,
                                                            N.stream_ptr())
    assert call(None, 3, 4 * H) == -1 and b"h0" in lib.dgppo_last_error()
    assert call(p(h0), 0, 4 * H) == -1 and b"rows_per_block" in lib.dgppo_last_error()
    assert call(p(h0), 3, 2 * H) == -1 and b"block_stride" in lib.dgppo_last_error()          # blocks would overlap
    assert call(C.c_void_p(h0.data_ptr() + 4), 3, 4 * H) == -1 and b"aligned" in lib.dgppo_last_error()
