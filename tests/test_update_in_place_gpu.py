"""Engine level: the update that reads the actor's carry record where the rollout wrote it (time-major rnn_tm through
ops_nn.H0Map: no env-major transpose in finalize(), no carry gather per minibatch) against the same engine built with
carry_in_place=False (the transposed copy, the blocked pre-pass read and the gathered h0_det).  LidarSpread n = 4 / 2 obstacles and n = 8 / 3, B = 8 envs,
T = 8, batch 32 (two minibatches of 4 envs), with and without captured graphs, two iterations on the same engines (the second
replays the captured graphs on the same record buffers).

Data movement only, so values_prepass outputs, the minibatch feature tensors and the carry rows the Vh pass reads must be
bit-equal.  After a full update() the weight-gradient reduces use atomics, so the old path need not equal itself: EIGHT
engines of the old path give, for every tensor of parameters and for every logged scalar on its own, the largest difference
among their 28 pairs in this iteration, and the new path may differ from an old engine in that tensor or scalar by at most
twice that.  Where all eight old engines agree bit for bit on everything, bit equality is required of the new path.

The sampled spread is a count of float32 steps, and a quantity's step is all it can resolve: with twice the bare spread and no
more, eight old engines that agreed on `policy/total_variation_dist` (0.0954365) failed a new engine that was ONE ulp
(7.5e-9) away, in the policy update, which this change does not touch; any number K of old engines leaves that chance at
1 / (K + 1) per quantity.  So the spread of a quantity is taken as known to one ulp of that quantity: the bound is
2 x (spread + 1 ulp), the ulp being float32's at the scalar's value or at the tensor's largest parameter.  That is 2.4e-7
relative at the most; an error of 1e-6 in Vh's loss or gradient norm fails.  No pooling over tensors or iterations.
rnn_states must be the transpose of the time-major carry record when first asked for, before and after an update (agent
and hits, still transposed in finalize(), are checked alongside)."""
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
B, T_, RS, BS = 8, 8, 4, 32


def _engines(cuda, n, n_obs, use_graphs):
    out = []
    for in_place in (True,) + (False,) * 8:
        cfg, ocfg, hp, eng, trees = _setup("LidarSpread", n, n_obs, B, T_, cuda, BS, RS, use_graphs=use_graphs,
                                           carry_in_place=in_place)
        out.append(eng)
    return out


def _expected_views(ro):
    """what finalize() has always produced, straight from the time-major record"""
    T = ro.T
    rnn = ro.rnn_tm[:T] if ro.stochastic else ro.rnn_tm[1:T + 1]
    want = {"rnn_states": rnn.transpose(0, 1).clone()}
    for k, v in ro.step_tm.items():
        want[k] = v.transpose(0, 1).clone()
    return want


def _check_views(ro, want, label):
    for k, w in want.items():
        got = getattr(ro, k)
        assert tuple(got.shape) == tuple(w.shape), f"{label}: {k} shape {tuple(got.shape)}"
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                           w.view(torch.int32) if w.dtype == torch.float32 else w), f"{label}: {k} differs"


def _same_bits(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what} differs"


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("n,n_obs", [(4, 2), (8, 3)])
def test_update_reads_the_record_in_place(cuda, n, n_obs, use_graphs):
    from dgppo_amd import nets
    new, *olds = _engines(cuda, n, n_obs, use_graphs)
    old_a = olds[0]
    assert new._carry_mapped() and not any(o._carry_mapped() for o in olds)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=cuda) * 7919
    Eb = BS // T_
    for it in range(2):
        perm = np.random.default_rng(5 + it).permutation(B)
        if it > 0:              # one common state again: the spread of the first update must not reach the second's rollouts
            state = old_a.state_dict()
            new.load_state_dict(state)
            for o in olds[1:]:
                o.load_state_dict(state)
        recs = []
        for eng in (new, *olds):
            ro = eng.rollout(seeds + it, True, noise_seed=3 + it).finalize()
            det = eng.rollout(seeds + 1000 + it, False).finalize()
            recs.append((ro, det))
        # the rollouts are the same rollouts, word for word (the spare carry slot behind them belongs to the pre-pass)
        for r_new, r_old in zip(recs[0], recs[1]):
            _same_bits(r_new.rnn_tm[:T_ + 1], r_old.rnn_tm[:T_ + 1], f"it {it}: rnn_tm")
            _same_bits(r_new.agent_tm, r_old.agent_tm, f"it {it}: agent_tm")
        want = [[_expected_views(r) for r in pair] for pair in recs]
        if it == 0:                                     # (in the second iteration the first access comes after the update)
            for r, w in zip(recs[0], want[0]):
                _check_views(r, w, f"it {it} before the update, stochastic={r.stochastic}")
        # value pre-passes of both records
        for k in range(2):
            outs = [eng.values_prepass(pair[k], want_Vl=True) for eng, pair in zip((new, old_a), recs)]
            outs = [(a.clone(), b.clone()) for a, b in outs]
            _same_bits(outs[0][0], outs[1][0], f"it {it}: Vl of record {k}")
            _same_bits(outs[0][1], outs[1][1], f"it {it}: Vh of record {k}")
            assert not torch.isnan(outs[1][1]).any()
        # the inputs of a minibatch: features of both records and the carry rows of the Vh pass
        ids = torch.from_numpy(perm[:Eb].astype(np.int32)).to(cuda)
        for k in range(2):
            f_new = new._block_feats("t_mb", recs[0][k], 0, Eb, 0, T_, env_ids=ids)
            f_old = old_a._block_feats("t_mb", recs[1][k], 0, Eb, 0, T_, env_ids=ids)
            for nm in ("Xa", "Xo", "efeat", "emask"):
                _same_bits(getattr(f_new, nm), getattr(f_old, nm), f"it {it}: {nm} of record {k}")
        rows_new = new._mb_carry(recs[0][1], ids).dense()
        rows_old = torch.index_select(recs[1][1].rnn_states, 0, ids.long()).reshape(Eb * T_ * n, nets.HID)
        _same_bits(rows_new, rows_old, f"it {it}: the carry rows of the Vh minibatch pass")
        # one full update each
        infos = [eng.update(ro, det, 10 + it, perm) for eng, (ro, det) in zip((new, *olds), recs)]
        torch.cuda.synchronize()
        for r, w in zip(recs[0], want[0]):
            _check_views(r, w, f"it {it} after the update, stochastic={r.stochastic}")
        assert all(set(i) == set(infos[0]) for i in infos) and len(infos[0]) >= 12
        p_diff = lambda x, y, name: float((x.nets[name].params - y.nets[name].params).abs().max())
        ulp = lambda v: float(np.spacing(np.float32(abs(v))))
        pairs = [(i, j) for i in range(len(olds)) for j in range(i + 1, len(olds))]
        sp_p = {name: max(p_diff(olds[i], olds[j], name) for i, j in pairs) for name in new.nets}
        sp_i = {key: max(abs(infos[1 + i][key] - infos[1 + j][key]) for i, j in pairs) for key in infos[0]}
        reproducible = all(v == 0.0 for v in sp_p.values()) and all(v == 0.0 for v in sp_i.values())
        for name in new.nets:
            assert torch.isfinite(new.nets[name].params).all()
            got = p_diff(new, old_a, name)
            bound = 0.0 if reproducible else 2.0 * (sp_p[name] + ulp(float(old_a.nets[name].params.abs().max())))
            print(f"n={n} graphs={use_graphs} it={it}: {name} params: old spread {sp_p[name]:.3e}, new-old {got:.3e}, bound {bound:.3e}")
            assert got <= bound, (it, name, got, sp_p[name], bound)
        for key in infos[0]:
            assert np.isfinite(infos[0][key]), (key, infos[0][key])
            got = abs(infos[0][key] - infos[1][key])
            bound = 0.0 if reproducible else 2.0 * (sp_i[key] + ulp(infos[1][key]))
            print(f"n={n} graphs={use_graphs} it={it}: {key}: old spread {sp_i[key]:.3e}, new-old {got:.3e}, bound {bound:.3e}")
            assert got <= bound, (it, key, infos[0][key], infos[1][key], sp_i[key], bound)
    if use_graphs:
        assert new._upd_graph.get("graph") is not None, "the minibatch step was never captured"
    assert "mb.h0_det" not in new.arena.bufs, "the gathered carry copy is still allocated"
