"""Engine level, LidarSpread n = 3, B = 8, T = 16, a stochastic and a deterministic record:
the value pre-pass that reads the stored carry in place (one spare slot in the env-major carry record, no [B, T+1, n, 64]
copy) returns what the copying path returned, bit for bit and on a second call too; and one update() with captured graphs
and three streams (its minibatch prelude: ONE gather launch on int32 ids) logs what the plain engine logs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_engine_gpu import _setup  # noqa: E402

pytestmark = pytest.mark.gpu
B, T_, RS, BS = 8, 16, 4, 32


def _reference_prepass(eng, ro):
    """values_prepass as it was before the carry was read in place: gather the T stored carries and the final one into a
    dense [B, T+1, n, 64] buffer and hand that to Vh.forward"""
    from dgppo_amd import nets
    cfg, n, nh, Hd = eng.cfg, eng.cfg.n_agents, eng.n_cost, nets.HID
    feats = eng._block_feats("refpre", ro, 0, B, 0, T_ + 1)
    Vl = eng.Vl.forward(feats, n_seq=B, T=T_ + 1, h0=None, tag="refpre", train=False)["v"].view(B, T_ + 1).clone()
    fin = eng._block_feats("reffin", ro, 0, B, T_, 1)
    h_last = ro.rnn_states[:, T_ - 1].reshape(B * n, Hd).contiguous()
    hstar = torch.empty(B * n, Hd, device=h_last.device)
    eng.policy.forward(fin, n_seq=B * n, T=1, h0=h_last, tag="reffin", hs_out=hstar, train=False)
    h0_all = torch.empty(B, T_ + 1, n, Hd, device=h_last.device)
    h0_all[:, :T_].copy_(ro.rnn_states)
    h0_all[:, T_].copy_(hstar.view(B, n, Hd))
    Vh = eng.Vh.forward(feats, n_seq=B * (T_ + 1) * n, T=1, h0=h0_all.view(-1, Hd), tag="refpre", train=False)["v"]
    return Vl, Vh.view(B, T_ + 1, n, nh).clone()


def test_values_prepass_in_place_equals_the_copying_path(cuda):
    cfg, ocfg, hp, eng, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, BS, RS)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    for stochastic in (True, False):
        ro = eng.rollout(seeds + (0 if stochastic else 1000), stochastic, noise_seed=3).finalize()
        states = ro.rnn_states.clone()
        assert tuple(ro.rnn_states.shape) == (B, T_, 3, 64)
        assert torch.equal(ro.rnn_states, ro.rnn_tm[:T_ if stochastic else T_ + 1][-T_:].transpose(0, 1))
        want_Vl, want_Vh = _reference_prepass(eng, ro)          # before the first in-place pass touches the spare slot
        for call in range(2):
            Vl, Vh = eng.values_prepass(ro, want_Vl=True)
            torch.cuda.synchronize()
            assert torch.equal(Vl, want_Vl), f"stochastic={stochastic} call {call}: Vl differs"
            assert torch.equal(Vh, want_Vh), f"stochastic={stochastic} call {call}: Vh differs"
            assert torch.equal(ro.rnn_states, states), "the pre-pass changed a stored carry"
        assert not torch.equal(Vh[:, T_], Vh[:, T_ - 1])
    assert "pre.h0all" not in eng.arena.bufs, "the dense carry buffer is still allocated"


def test_update_graphs_and_streams_equals_plain_engine(cuda):
    """one update() with use_graphs=True, multi_stream=True against one with both off, every info() key within 1e-4 of its
    scale: the bound tests/test_engine_gpu.py::test_multi_stream_update_equals_single_stream holds its pair to (fp32
    reduction-order noise of the atomics; the graph pair of that file is held to 1e-5 and is contained in this one)"""
    from dgppo_amd import engine as EN
    cfg, ocfg, hp, eng_a, trees = _setup("LidarSpread", 3, 2, B, T_, cuda, BS, RS)
    eng_b = EN.Engine(cfg, hp, cuda, T=T_, use_graphs=True, multi_stream=True)
    for k, net in eng_b.nets.items():
        net.load_tree(trees[k])
    eng_b.set_entropy_noise(77)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    perm = np.random.default_rng(5).permutation(B)
    infos = []
    for eng in (eng_a, eng_b):
        ro = eng.rollout(seeds, True, noise_seed=3)
        det = eng.rollout(seeds + 1000, False)
        infos.append(eng.update(ro, det, 10, perm))
        torch.cuda.synchronize()
    assert set(infos[0]) == set(infos[1]) and len(infos[0]) >= 12
    for k in infos[0]:
        assert abs(infos[0][k] - infos[1][k]) <= 1e-4 * max(1.0, abs(infos[0][k])), (k, infos[0][k], infos[1][k])
    assert eng_b._upd_graph.get("graph") is not None, "the minibatch step was never captured"
    for name in ("Vl", "Vh", "policy"):
        assert float(eng_a.opt[name].state[2]) == float(eng_b.opt[name].state[2]) == B // (BS // T_)
