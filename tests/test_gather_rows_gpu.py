"""dgppo_gather_rows (csrc/gather.hip) through ops_nn.gather_rows: one launch copies dst_k[e] = src_k[ids[e]] for up to 8
tensors that share the id list — torch.index_select along dim 0 of each, bit for bit.  Row sizes on both sides of the 16-byte
path (4 B, 12 B, 64 B, 4100 B), a source slice that starts 4 bytes past a 16-byte boundary with a row stride larger than the
row, one and seven ids, repeated ids, one and eight descriptors per call; and the refusals before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROW_FLOATS = (1, 3, 16, 1025)        # 4 B, 12 B, 64 B, 4100 B
N_SRC = 9


def _sources(cuda, seed, kinds):
    """(src, name) per kind: dense rows, or (`slice`) columns 1.. of a wider buffer — 4 bytes past a 16-byte boundary, the row
    stride one float larger than the row"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for rf, sliced in kinds:
        if sliced:
            wide = torch.randn(N_SRC, rf + 1, generator=g).to(cuda)
            src = wide[:, 1:]
            assert src.data_ptr() % 16 == 4 and src.stride(0) == rf + 1
        else:
            src = torch.randn(N_SRC, rf, generator=g).to(cuda)
        out.append(src)
    return out


def _check(cuda, srcs, ids):
    from dgppo_amd import ops_nn as K
    idx32 = torch.tensor(ids, dtype=torch.int32, device=cuda)
    dsts = [torch.full((len(ids),) + tuple(s.shape[1:]), float("nan") if s.is_floating_point() else -1, device=cuda, dtype=s.dtype)
            for s in srcs]
    K.gather_rows(list(zip(srcs, dsts)), idx32)
    torch.cuda.synchronize()
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        want = torch.index_select(s, 0, idx32.long())
        assert torch.equal(d.view(torch.int32), want.contiguous().view(torch.int32)), f"descriptor {k}: rows of {tuple(s.shape)} differ"


@pytest.mark.parametrize("ids", [(4,), (8, 0, 3, 3, 5, 0, 7)], ids=["one-id", "seven-ids-repeated"])
@pytest.mark.parametrize("rf", ROW_FLOATS)
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "misaligned-slice"])
def test_gather_rows_one_descriptor_equals_index_select(cuda, rf, sliced, ids):
    _check(cuda, _sources(cuda, 10 * rf + sliced, [(rf, sliced)]), ids)


@pytest.mark.parametrize("ids", [(4,), (8, 0, 3, 3, 5, 0, 7)], ids=["one-id", "seven-ids-repeated"])
def test_gather_rows_eight_descriptors_in_one_launch(cuda, ids):
    """every row size dense and sliced in ONE call: descriptors of both access widths side by side; one source has several
    trailing dimensions and one is int32"""
    srcs = _sources(cuda, 3, [(rf, sl) for rf in ROW_FLOATS for sl in (False, True)])
    srcs[2] = torch.randn(N_SRC, 2, 4, 2).to(cuda)[:, :, :, :]                      # 64-byte rows as [2, 4, 2]
    srcs[5] = torch.arange(N_SRC * 16, dtype=torch.int32, device=cuda).view(N_SRC, 16)
    assert len(srcs) == 8
    _check(cuda, srcs, ids)


def test_gather_rows_view_along_dim1_of_a_record(cuda):
    """the update's carry gather: rows [T, n, 64] of a [B, T + 2, n, 64] record from slot 1 on"""
    rec = torch.randn(N_SRC, 5, 3, 64).to(cuda)
    _check(cuda, [rec[:, 1:4], rec[:, :3]], (2, 2, 8, 0))


def test_gather_rows_refusals_come_before_any_launch(cuda):
    from dgppo_amd import _native as N, ops_nn as K
    lib = N.lib()
    src = torch.randn(4, 4, device=cuda)
    dst = torch.full((2, 4), float("nan"), device=cuda)
    ids = torch.tensor([1, 2], dtype=torch.int32, device=cuda)
    d = (K.GatherDesc * 1)(K.GatherDesc(src.data_ptr(), dst.data_ptr(), 6, 16))      # row_bytes % 4 != 0
    assert lib.dgppo_gather_rows(d, 1, C.c_void_p(ids.data_ptr()), 2, N.stream_ptr()) == -1
    assert b"multiple of 4" in lib.dgppo_last_error()
    for s_ptr, d_ptr in ((0, dst.data_ptr()), (src.data_ptr(), 0)):                  # NULL source / destination
        d = (K.GatherDesc * 1)(K.GatherDesc(s_ptr, d_ptr, 16, 16))
        assert lib.dgppo_gather_rows(d, 1, C.c_void_p(ids.data_ptr()), 2, N.stream_ptr()) == -1
        assert b"NULL" in lib.dgppo_last_error()
    d = (K.GatherDesc * 1)(K.GatherDesc(src.data_ptr(), dst.data_ptr(), 16, 16))
    assert lib.dgppo_gather_rows(d, 1, None, 2, N.stream_ptr()) == -1 and b"NULL" in lib.dgppo_last_error()   # NULL ids
    assert lib.dgppo_gather_rows(d, 9, C.c_void_p(ids.data_ptr()), 2, N.stream_ptr()) == -1                   # > 8 descriptors
    torch.cuda.synchronize()
    assert torch.isnan(dst).all(), "a refused call wrote to its destination"
    with pytest.raises(ValueError, match="does not fit"):
        K.gather_rows([(src, torch.empty(3, 4, device=cuda))], ids)
    with pytest.raises(TypeError, match="int32"):
        K.gather_rows([(src, dst)], ids.long())
