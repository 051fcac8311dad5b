"""Torch-tensor wrappers over the network entry points of the C ABI (include/dgppo_hip.h).
Matrices may be row-strided views (unit inner stride): (pointer, leading dimension) are passed to the kernels."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as N

# Matrix-core work actually enqueued, in flops (2 per multiply-add of the UNPADDED operand shapes), accumulated by the
# wrappers below; bench.py reads it to report MFMA utilisation from executed work rather than from SURVEY's per-node
# estimate.  (Host-side bookkeeping only; the engine re-adds a rollout's count when it replays a captured HIP graph.)
FLOPS = [0.0]


def _mat(t: torch.Tensor, name: str):
    """2-D fp32 CUDA tensor with unit inner stride -> (ptr, ld, rows, cols)."""
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must have unit inner stride")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    return C.c_void_p(t.data_ptr()), int(ld), int(t.shape[0]), int(t.shape[1])


def _p(t: Optional[torch.Tensor], name="tensor", dtype=torch.float32):
    return N.ptr(t, dtype, name)


def dense_fwd(X, W, bias, Y, act: int = 0, accumulate: bool = False, trans_w: bool = False, relu_mask=None):
    """Y = act(X @ W + bias)   (trans_w: X @ W.T with W stored [N, K]); relu_mask: Y = where(relu_mask > 0, Y, 0) last."""
    xp, ldx, M, K = _mat(X, "X")
    wp, ldw, wr, wc = _mat(W, "W")
    yp, ldy, My, Ncol = _mat(Y, "Y")
    Kw, Nw = (wc, wr) if trans_w else (wr, wc)
    if Kw != K or Nw != Ncol or My != M:
        raise ValueError(f"dense_fwd: shape mismatch X{tuple(X.shape)} W{tuple(W.shape)} trans={trans_w} Y{tuple(Y.shape)}")
    if bias is not None:
        N.expect_shape(bias, (Ncol,), "bias")
    mp, ldm = C.c_void_p(0), 0
    if relu_mask is not None:
        mp, ldm, Mm, Nm = _mat(relu_mask, "relu_mask")
        if (Mm, Nm) != (M, Ncol):
            raise ValueError(f"dense_fwd: relu_mask {tuple(relu_mask.shape)} does not match Y {tuple(Y.shape)}")
    FLOPS[0] += 2.0 * M * K * Ncol
    rc = N.lib().dgppo_dense_fwd(xp, ldx, wp, ldw, _p(bias, "bias"), yp, ldy, M, K, Ncol, int(act), int(accumulate),
                                 int(trans_w), mp, ldm, N.stream_ptr())
    N.check(rc, "dgppo_dense_fwd")


def mlp_gi_fwd(X, W1, b1, g1, be1, W2, b2, g2, be2, Wi, bi, gi, saves=None):
    """gi = relu(LN(relu(LN(X W1 + b1)) W2 + b2)) Wi + bi in one kernel; saves = (p1, y1, st1, p2, y2, st2) or None.
    gi None: the trunk alone (its y2 is the result, for gi_gru1_head_fwd); saves may then be (None, None, None, None, y2, None)."""
    xp, ldx, M, K = _mat(X, "X")
    if K != 64:
        raise ValueError(f"mlp_gi_fwd: X must be [M, 64], got {tuple(X.shape)}")
    for t, shp, nm in ((W1, (64, 64), "W1"), (W2, (64, 64), "W2"), (Wi, (64, 192), "Wi"), (b1, (64,), "b1"), (g1, (64,), "g1"),
                       (be1, (64,), "be1"), (b2, (64,), "b2"), (g2, (64,), "g2"), (be2, (64,), "be2"), (bi, (192,), "bi")):
        N.expect_shape(t, shp, nm)
    if gi is not None:
        N.expect_shape(gi, (M, 192), "gi")
    sv = [None] * 6
    if saves is not None:
        for t, shp, nm in zip(saves, ((M, 64), (M, 64), (M, 2), (M, 64), (M, 64), (M, 2)), ("p1", "y1", "st1", "p2", "y2", "st2")):
            if t is not None:
                N.expect_shape(t, shp, nm)
        sv = list(saves)
    FLOPS[0] += 2.0 * M * (64 * 64 * 2 + (64 * 192 if gi is not None else 0))
    rc = N.lib().dgppo_mlp_gi_fwd(xp, ldx, _p(W1), _p(b1), _p(g1), _p(be1), _p(W2), _p(b2), _p(g2), _p(be2), _p(Wi), _p(bi),
                                  *[_p(t) for t in sv], _p(gi), M, N.stream_ptr())
    N.check(rc, "dgppo_mlp_gi_fwd")


def mlp_gi_bwd(dgi, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, relu_mask, dpre2, dpre1, dx, dg2, db2, dg1, db1):
    """activation gradients of the mlp_gi_fwd chain in one kernel (dgppo_mlp_gi_bwd): dgi [M,192] -> dpre2, dpre1, dx [M,64];
    dg* / db* [64] accumulate the LayerNorm parameter gradients; relu_mask [M,64] or None masks dx."""
    M = dgi.shape[0]
    N.expect_shape(dgi, (M, 192), "dgi")
    for t, shp, nm in ((Wi, (64, 192), "Wi"), (W2, (64, 64), "W2"), (W1, (64, 64), "W1"), (g2, (64,), "g2"), (g1, (64,), "g1"),
                       (p2, (M, 64), "p2"), (y2, (M, 64), "y2"), (st2, (M, 2), "st2"), (p1, (M, 64), "p1"), (y1, (M, 64), "y1"),
                       (st1, (M, 2), "st1"), (dpre2, (M, 64), "dpre2"), (dpre1, (M, 64), "dpre1"), (dx, (M, 64), "dx"),
                       (dg2, (64,), "dg2"), (db2, (64,), "db2"), (dg1, (64,), "dg1"), (db1, (64,), "db1")):
        N.expect_shape(t, shp, nm)
    mp, ldm = (None, 0)
    if relu_mask is not None:
        mp, ldm, Mm, Km = _mat(relu_mask, "relu_mask")
        if (Mm, Km) != (M, 64):
            raise ValueError(f"mlp_gi_bwd: relu_mask must be [M, 64], got {tuple(relu_mask.shape)}")
    FLOPS[0] += 2.0 * M * (64 * 64 * 2 + 64 * 192)
    rc = N.lib().dgppo_mlp_gi_bwd(_p(dgi), _p(Wi), _p(W2), _p(W1), _p(g2), _p(g1), _p(p2), _p(y2), _p(st2), _p(p1), _p(y1), _p(st1),
                                  mp if mp is not None else C.c_void_p(0), ldm, _p(dpre2), _p(dpre1), _p(dx), 64,
                                  _p(dg2), _p(db2), _p(dg1), _p(db1), M, N.stream_ptr())
    N.check(rc, "dgppo_mlp_gi_bwd")


def gru1_head_fwd(gi, Wh, bhn, h0, W1, b1, W2, b2, hs, hprev, gates, u, out):
    """one GRU step (T = 1) + head Dense(s): out = (h' W1 + b1) [W2 + b2]; see dgppo_gru1_head_fwd in the header."""
    M = gi.shape[0]
    n_out = out.shape[1]
    N.expect_shape(gi, (M, 192), "gi"); N.expect_shape(Wh, (64, 192), "Wh"); N.expect_shape(bhn, (64,), "bhn")
    N.expect_shape(hs, (M, 64), "hs"); N.expect_shape(out, (M, n_out), "out")
    if h0 is not None:
        N.expect_shape(h0, (M, 64), "h0")
    if W2 is not None:
        N.expect_shape(W1, (64, 64), "W1"); N.expect_shape(b1, (64,), "b1")
        N.expect_shape(W2, (64, n_out), "W2"); N.expect_shape(b2, (n_out,), "b2")
    else:
        N.expect_shape(W1, (64, n_out), "W1"); N.expect_shape(b1, (n_out,), "b1")
    for t, shp, nm in ((hprev, (M, 64), "hprev"), (gates, (M, 256), "gates"), (u, (M, 64), "u")):
        if t is not None:
            N.expect_shape(t, shp, nm)
    FLOPS[0] += 2.0 * M * (64 * 192 + (64 * 64 + 64 * n_out if W2 is not None else 64 * n_out))
    rc = N.lib().dgppo_gru1_head_fwd(_p(gi), _p(Wh), _p(bhn), _p(h0), _p(W1), _p(b1), _p(W2), _p(b2), _p(hs), _p(hprev),
                                     _p(gates), _p(u), _p(out), M, n_out, N.stream_ptr())
    N.check(rc, "dgppo_gru1_head_fwd")


_WS: dict = {}   # (device index, stream handle) -> scratch tensor for dense_bwd_w's partial sums (caller-owned, see the header)


def _bwd_w_workspace(device, K: int, Ncol: int) -> torch.Tensor:
    lib = N.lib()
    lib.dgppo_dense_bwd_w_workspace_bytes.restype = C.c_int64
    need = int(lib.dgppo_dense_bwd_w_workspace_bytes(C.c_int32(K), C.c_int32(Ncol)))
    need = min(need, 64 << 20)                      # a smaller buffer only shrinks the grid
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


class ReduceDesc(C.Structure):
    """struct dgppo_reduce_desc"""
    _fields_ = [("part", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("part_stride", C.c_int32), ("slabs", C.c_int32),
                ("ldw", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("pending", C.c_int32)]


class BwdWBatch:
    """Weight gradients of one backward pass with their second stage (slab reduction) deferred: every dense_bwd_w inside
    `with BwdWBatch(device, alloc):` launches only its partial-slab kernel into its own region of one workspace, and leaving
    the block flushes all pending reductions with one launch per 16 (dgppo_dense_bwd_w_reduce_batch).  `alloc(n_floats)`
    returns the caller's workspace of at least that size (an arena buffer: a move is visible to captured-graph checks)."""
    _active = {}        # (device index, stream handle) -> BwdWBatch

    def __init__(self, device, alloc):
        self.device, self.alloc = device, alloc
        self.key = None
        self.descs = []
        self.offset = 0                  # bytes used in the workspace
        self.ws = None

    def __enter__(self):
        self.key = (self.device.index, torch.cuda.current_stream(self.device).cuda_stream)
        if self.key in BwdWBatch._active:
            raise RuntimeError("BwdWBatch: nested batches on one stream")
        BwdWBatch._active[self.key] = self
        return self

    def region(self, nbytes: int):
        """a 256-byte aligned region of the workspace; regions of one batch never overlap"""
        nbytes = (nbytes + 255) & ~255
        if self.ws is None or self.ws.numel() * 4 < self.offset + nbytes:
            if self.descs:               # growing may move regions that pending reductions still read: flush them first
                self.flush()
            self.ws = self.alloc(max(self.offset + nbytes, 2 * (self.ws.numel() * 4 if self.ws is not None else 0)) // 4)
        view = self.ws[self.offset // 4:(self.offset + nbytes) // 4]
        self.offset += nbytes
        return view

    def flush(self):
        if self.descs:
            arr = (ReduceDesc * len(self.descs))(*self.descs)
            N.check(N.lib().dgppo_dense_bwd_w_reduce_batch(arr, C.c_int32(len(self.descs)), N.stream_ptr()),
                    "dgppo_dense_bwd_w_reduce_batch")
        self.descs = []
        self.offset = 0

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.flush()
        finally:
            BwdWBatch._active.pop(self.key, None)
        return False


def dense_bwd_w(X, dY, dW, db=None):
    """dW += X.T @ dY ; db += dY.sum(0)   (inside `with BwdWBatch(...)`: the slab reduction is deferred to the batch's flush)"""
    xp, ldx, M, K = _mat(X, "X")
    yp, ldy, My, Ncol = _mat(dY, "dY")
    wp, ldw, Kw, Nw = _mat(dW, "dW")
    if My != M or Kw != K or Nw != Ncol:
        raise ValueError(f"dense_bwd_w: shape mismatch X{tuple(X.shape)} dY{tuple(dY.shape)} dW{tuple(dW.shape)}")
    if db is not None:
        N.expect_shape(db, (Ncol,), "db")
    FLOPS[0] += 2.0 * M * K * Ncol
    batch = BwdWBatch._active.get((X.device.index, torch.cuda.current_stream(X.device).cuda_stream)) if X.is_cuda else None
    if batch is not None:
        lib = N.lib()
        lib.dgppo_dense_bwd_w_workspace_bytes.restype = C.c_int64
        need = min(int(lib.dgppo_dense_bwd_w_workspace_bytes(C.c_int32(K), C.c_int32(Ncol))), 64 << 20)
        ws = batch.region(need)
        d = ReduceDesc()
        rc = lib.dgppo_dense_bwd_w_deferred(xp, ldx, yp, ldy, wp, ldw, _p(db, "db"), M, K, Ncol, _p(ws, "workspace"),
                                            C.c_int64(ws.numel() * 4), C.byref(d), N.stream_ptr())
        N.check(rc, "dgppo_dense_bwd_w_deferred")
        if d.pending:
            batch.descs.append(d)
        return
    ws = _bwd_w_workspace(X.device, K, Ncol)
    rc = N.lib().dgppo_dense_bwd_w(xp, ldx, yp, ldy, wp, ldw, _p(db, "db"), M, K, Ncol, _p(ws, "workspace"),
                                   C.c_int64(ws.numel() * 4), N.stream_ptr())
    N.check(rc, "dgppo_dense_bwd_w")


def dense_bwd_xw(X, dY, W, dX, dW, db=None, accumulate_mask: bool = False):
    """dense_bwd_w(X, dY, dW, db) and dense_fwd(dY, W, None, dX, trans_w=True) - with accumulate_mask: accumulate=True,
    relu_mask=X - as ONE call: the library runs them as one pass over X and dY for the GNN glue shapes (K, N) = (144, 64),
    (48, 32), (48, 64) and (32, 96) with 16-byte aligned operands - at (144, 64) only the `=` form - and as the pair otherwise
    (dgppo_dense_bwd_xw in the header; the table kXwSites in nn_dense.hip)."""
    xp, ldx, M, K = _mat(X, "X")
    yp, ldy, My, Ncol = _mat(dY, "dY")
    pp, ldp, Kp, Np = _mat(W, "W")
    dxp, lddx, Mx, Kx = _mat(dX, "dX")
    wp, ldw, Kw, Nw = _mat(dW, "dW")
    if My != M or (Kw, Nw) != (K, Ncol) or (Kp, Np) != (K, Ncol) or (Mx, Kx) != (M, K):
        raise ValueError(f"dense_bwd_xw: shape mismatch X{tuple(X.shape)} dY{tuple(dY.shape)} W{tuple(W.shape)} "
                         f"dX{tuple(dX.shape)} dW{tuple(dW.shape)}")
    if db is not None:
        N.expect_shape(db, (Ncol,), "db")
    FLOPS[0] += 4.0 * M * K * Ncol
    batch = BwdWBatch._active.get((X.device.index, torch.cuda.current_stream(X.device).cuda_stream))
    lib = N.lib()
    if batch is not None:
        lib.dgppo_dense_bwd_w_workspace_bytes.restype = C.c_int64
        ws = batch.region(min(int(lib.dgppo_dense_bwd_w_workspace_bytes(C.c_int32(K), C.c_int32(Ncol))), 64 << 20))
        d = ReduceDesc()
        pend = C.byref(d)
    else:
        ws = _bwd_w_workspace(X.device, K, Ncol)
        pend = None
    rc = lib.dgppo_dense_bwd_xw(xp, ldx, yp, ldy, pp, ldp, dxp, lddx, int(bool(accumulate_mask)), wp, ldw, _p(db, "db"), M, K,
                                Ncol, _p(ws, "workspace"), C.c_int64(ws.numel() * 4), pend, N.stream_ptr())
    N.check(rc, "dgppo_dense_bwd_xw")
    if batch is not None and d.pending:
        batch.descs.append(d)


def _check_strided(fn: str, name: str, t_, se: int, st: int, inner: tuple, env_ids, n_env: int, n_time: int):
    """a record field the feature kernels address as data_ptr + env * se + time * st, in floats (a view's own outer strides are
    ignored): the innermost record must be dense fp32 CUDA storage, and the storage must reach the last (env, time) the call
    touches"""
    if not (t_.is_cuda and t_.dtype == torch.float32):
        raise ValueError(f"{fn}: {name} must be a float32 CUDA tensor")
    want, acc = [], 1
    for d in reversed(inner):
        want.append(acc)
        acc *= d
    if tuple(t_.shape[-len(inner):]) != tuple(inner) or list(t_.stride()[-len(inner):]) != want[::-1]:
        raise ValueError(f"{fn}: the trailing {inner} block of {name} must be dense (got shape {tuple(t_.shape)}, "
                         f"strides {t_.stride()})")
    avail = t_.untyped_storage().nbytes() // 4 - t_.storage_offset()
    if env_ids is None and (n_env - 1) * se + (n_time - 1) * st + acc > avail:
        raise ValueError(f"{fn}: {name}: the strides reach beyond its storage")


def graph_feats(cfg: N.EnvCfg, agent, agent_se, agent_st, goal, obst, hits, hits_se, hits_st, env_ids, n_env, n_time,
                Xa, Xo, efeat, emask, Fp):
    """agent/hits are base tensors (any shape); strides are in floats."""
    G = n_env * n_time
    n, S = cfg.n_agents, cfg.fan_in
    n_other = cfg.num_nodes - 1 - n
    N.expect_shape(Xa, (G * n, Fp), "Xa")
    if n_other > 0:
        N.expect_shape(Xo, (G * n_other, Fp), "Xo")
    N.expect_shape(efeat, (G * n, S, 4), "efeat")
    N.expect_shape(emask, (G * n, S), "emask")
    _check_strided("graph_feats", "agent", agent, agent_se, agent_st, (n, cfg.state_dim), env_ids, n_env, n_time)
    if hits is not None:
        _check_strided("graph_feats", "hits", hits, hits_se, hits_st, (n, cfg.top_k, 2), env_ids, n_env, n_time)
    rc = N.lib().dgppo_graph_feats(
        C.byref(cfg), C.c_void_p(agent.data_ptr()), C.c_int64(agent_se), C.c_int64(agent_st), _p(goal, "goal"),
        _p(obst, "obst") if (obst is not None and not cfg.is_lidar) else C.c_void_p(0),
        C.c_void_p(hits.data_ptr()) if hits is not None else C.c_void_p(0), C.c_int64(hits_se), C.c_int64(hits_st),
        _p(env_ids, "env_ids", torch.int32), C.c_int32(n_env), C.c_int32(n_time), _p(Xa, "Xa"), _p(Xo, "Xo"),
        _p(efeat, "efeat"), _p(emask, "emask"), C.c_int32(Fp), N.stream_ptr())
    N.check(rc, "dgppo_graph_feats")


def sweep_axis(x, name: str, device) -> torch.Tensor:
    """one axis of a sweep grid as a dense fp32 device tensor: the coordinates are formed on the host (or given as a tensor)
    and only copied, so host and device agree on every bit.  An empty axis or a non-finite coordinate is a ValueError."""
    if torch.is_tensor(x):
        t_ = x.to(device=device, dtype=torch.float32).contiguous()
        ok = t_.ndim == 1 and t_.numel() > 0 and bool(torch.isfinite(t_).all())
    else:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        ok = a.ndim == 1 and a.size > 0 and bool(np.isfinite(a).all())
        t_ = torch.from_numpy(a).to(device) if ok else None
    if not ok:
        raise ValueError(f"graph_feats_sweep: {name} must be a non-empty 1-D array of finite coordinates")
    return t_


def _sweep_grid(fn: str, cfg: N.EnvCfg, frame_ids, n_frames, agent_id, xs, ys, frame_max, names=("xs", "ys")):
    """the grid and frame arguments the sweep bindings share -> nx, ny, the host frame numbers still to be copied (or
    None), the device frame numbers given (or None), the largest frame read"""
    n = cfg.n_agents
    if not 0 <= int(agent_id) < n:
        raise ValueError(f"{fn}: agent_id {agent_id} outside [0, {n})")
    for name, t_ in zip(names, (xs, ys)):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == torch.float32 and t_.ndim == 1 and t_.is_contiguous()):
            raise ValueError(f"{fn}: {name} must be a dense 1-D float32 CUDA tensor (sweep_axis)")
        if t_.numel() == 0:
            raise ValueError(f"{fn}: {name} is empty")
    ids = ids_dev = None
    if torch.is_tensor(frame_ids):                       # already on the device: the caller vouches for the largest frame
        if frame_max is None or n_frames < 1 or tuple(frame_ids.shape) != (n_frames,):
            raise ValueError(f"{fn}: a device frame_ids needs its shape (n_frames,) and frame_max")
        ids_dev, last = frame_ids, int(frame_max)
    elif frame_ids is not None:
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if ids.size != n_frames or n_frames == 0 or ids.min() < 0:
            raise ValueError(f"{fn}: frame_ids must hold n_frames >= 1 frame numbers >= 0")
        last = int(ids.max())
    else:
        if n_frames < 1:
            raise ValueError(f"{fn}: n_frames must be >= 1")
        last = n_frames - 1
    return int(xs.numel()), int(ys.numel()), ids, ids_dev, last


def _sweep_record(fn: str, cfg: N.EnvCfg, agent, agent_st, obst, hits, hits_st, ray_cos, ray_sin, last, hits_out, G) -> bool:
    """the record operands the two sweep bindings share; -> whether the kind casts rays (a LiDAR kind with obstacles)"""
    n = cfg.n_agents
    _check_strided(fn, "agent", agent, 0, agent_st, (n, cfg.state_dim), None, 1, last + 1)
    cast = cfg.is_lidar and cfg.n_obs > 0
    if cfg.n_obs > 0:
        if obst is None:
            raise ValueError(f"{fn}: obst is required when n_obs > 0")
        N.expect_shape(obst, (cfg.n_obs, cfg.obst_stride), "obst")
    if cast:
        if hits is None:
            raise ValueError(f"{fn}: hits is required for a LiDAR kind with obstacles")
        _check_strided(fn, "hits", hits, 0, hits_st, (n, cfg.top_k, 2), None, 1, last + 1)
        N.expect_shape(ray_cos, (cfg.n_rays,), "ray_cos")
        N.expect_shape(ray_sin, (cfg.n_rays,), "ray_sin")
        if hits_out is not None:
            N.expect_shape(hits_out, (G, cfg.top_k, 2), "hits_out")
    return cast


def graph_feats_sweep(cfg: N.EnvCfg, agent, agent_st, goal, obst, hits, hits_st, ray_cos, ray_sin, frame_ids, n_frames,
                      agent_id, xs, ys, Xa, Xo, efeat, emask, Fp, hits_out=None, frame_max=None):
    """dgppo_graph_feats_sweep: the features of n_frames frames of ONE env (agent / hits: base tensors read at
    frame * stride, in floats; goal / obst: that env's rows) with agent `agent_id` moved over the grid xs [nx] x ys [ny]
    (sweep_axis tensors).  frame_ids: a host sequence of frame numbers (copied to the device here), an int32 device tensor
    with frame_max = its largest entry (nothing is copied), or None (0 .. n_frames-1).
    Every refusal is raised before anything is launched."""
    fn = "graph_feats_sweep"
    n, S = cfg.n_agents, cfg.fan_in
    nx, ny, ids, ids_dev, last = _sweep_grid(fn, cfg, frame_ids, n_frames, agent_id, xs, ys, frame_max)
    G = n_frames * ny * nx
    n_other = cfg.num_nodes - 1 - n
    N.expect_shape(Xa, (G * n, Fp), "Xa")
    if n_other > 0:
        N.expect_shape(Xo, (G * n_other, Fp), "Xo")
    N.expect_shape(efeat, (G * n, S, 4), "efeat")
    N.expect_shape(emask, (G * n, S), "emask")
    N.expect_shape(goal, (cfg.n_goals, cfg.state_dim), "goal")
    cast = _sweep_record(fn, cfg, agent, agent_st, obst, hits, hits_st, ray_cos, ray_sin, last, hits_out, G)
    if ids is not None:
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(agent.device)
    null = C.c_void_p(0)
    rc = N.lib().dgppo_graph_feats_sweep(
        C.byref(cfg), C.c_void_p(agent.data_ptr()), C.c_int64(agent_st), _p(goal, "goal"),
        _p(obst, "obst") if cfg.n_obs > 0 else null, C.c_void_p(hits.data_ptr()) if cast else null, C.c_int64(hits_st),
        _p(ray_cos, "ray_cos") if cast else null, _p(ray_sin, "ray_sin") if cast else null,
        _p(ids_dev, "frame_ids", torch.int32), C.c_int32(n_frames), C.c_int32(int(agent_id)), _p(xs, "xs"), C.c_int32(nx),
        _p(ys, "ys"), C.c_int32(ny), _p(Xa, "Xa"), _p(Xo, "Xo") if n_other > 0 else null, _p(efeat, "efeat"), _p(emask, "emask"),
        _p(hits_out, "hits_out") if (cast and hits_out is not None) else null, C.c_int32(Fp), N.stream_ptr())
    N.check(rc, "dgppo_graph_feats_sweep")


def cost_sweep(cfg: N.EnvCfg, agent, agent_st, obst, hits, hits_st, ray_cos, ray_sin, frame_ids, n_frames, agent_id, xs, ys,
               cost, hits_out=None, frame_max=None):
    """dgppo_cost_sweep: the environment's cost [G, n, n_cost] of all agents over the sweep graph_feats_sweep describes
    (same operands without the goals, same frame_ids conventions, xs / ys: sweep_axis tensors; G = n_frames * ny * nx).
    hits_out [G, k, 2] is for the kinds that cast rays (LiDAR with obstacles); with any other kind it is a ValueError.
    Every refusal is raised before anything is launched."""
    fn = "cost_sweep"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no sweep entry point")
    if hits_out is not None and not (cfg.is_lidar and cfg.n_obs > 0):
        raise ValueError(f"{fn}: hits_out needs a LiDAR kind with obstacles (nothing is cast here)")
    nx, ny, ids, ids_dev, last = _sweep_grid(fn, cfg, frame_ids, n_frames, agent_id, xs, ys, frame_max)
    G = n_frames * ny * nx
    N.expect_shape(cost, (G, cfg.n_agents, cfg.n_cost), "cost")
    cast = _sweep_record(fn, cfg, agent, agent_st, obst, hits, hits_st, ray_cos, ray_sin, last, hits_out, G)
    if ids is not None:
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(agent.device)
    null = C.c_void_p(0)
    rc = N.lib().dgppo_cost_sweep(
        C.byref(cfg), C.c_void_p(agent.data_ptr()), C.c_int64(agent_st), _p(obst, "obst") if cfg.n_obs > 0 else null,
        C.c_void_p(hits.data_ptr()) if cast else null, C.c_int64(hits_st), _p(ray_cos, "ray_cos") if cast else null,
        _p(ray_sin, "ray_sin") if cast else null, _p(ids_dev, "frame_ids", torch.int32), C.c_int32(n_frames),
        C.c_int32(int(agent_id)), _p(xs, "xs"), C.c_int32(nx), _p(ys, "ys"), C.c_int32(ny), _p(cost, "cost"),
        _p(hits_out, "hits_out") if cast and hits_out is not None else null, N.stream_ptr())
    N.check(rc, "dgppo_cost_sweep")


ACTION_SWEEP_TILE = 64    # grid points per workgroup of dgppo_graph_feats_action_sweep (ACT_TILE, csrc/env_sweep.hip)


def graph_feats_action_sweep(cfg: N.EnvCfg, agent, agent_st, goal, obst, hits, hits_st, frame_ids, n_frames, agent_id, us, vs,
                             Xa, Xo, efeat, emask, Fp, frame_max=None):
    """dgppo_graph_feats_action_sweep: the features of the graphs AFTER the step of n_frames frames of ONE env (agent / hits:
    base tensors read at frame * stride, in floats; goal / obst: that env's rows) with the action of agent `agent_id` swept
    over us [nu] x vs [nv] (sweep_axis tensors; clipped to [-1, 1] like every action): graph (f, iv, iu) is frame
    frame_ids[f] + 1 with that agent's row stepped from frame frame_ids[f] by (us[iu], vs[iv]).  Nothing is cast: hits are the
    recorded ones of frame + 1.  frame_ids as in graph_feats_sweep; frame + 1 must lie inside the record.
    Every refusal is raised before anything is launched."""
    fn = "graph_feats_action_sweep"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no sweep entry point")
    n, S = cfg.n_agents, cfg.fan_in
    nu, nv, ids, ids_dev, last = _sweep_grid(fn, cfg, frame_ids, n_frames, agent_id, us, vs, frame_max, ("us", "vs"))
    G = n_frames * nv * nu
    n_other = cfg.num_nodes - 1 - n
    N.expect_shape(Xa, (G * n, Fp), "Xa")
    if n_other > 0:
        N.expect_shape(Xo, (G * n_other, Fp), "Xo")
    N.expect_shape(efeat, (G * n, S, 4), "efeat")
    N.expect_shape(emask, (G * n, S), "emask")
    N.expect_shape(goal, (cfg.n_goals, cfg.state_dim), "goal")
    # frames last and last + 1 are read
    _check_strided(fn, "agent", agent, 0, agent_st, (n, cfg.state_dim), None, 1, last + 2)
    rec_hits = cfg.is_lidar and cfg.n_obs > 0
    discs = (not cfg.is_lidar) and cfg.n_obs > 0
    if rec_hits:
        if hits is None:
            raise ValueError(f"{fn}: hits is required for a LiDAR kind with obstacles")
        _check_strided(fn, "hits", hits, 0, hits_st, (n, cfg.top_k, 2), None, 1, last + 2)
    if discs:
        if obst is None:
            raise ValueError(f"{fn}: obst is required when n_obs > 0")
        N.expect_shape(obst, (cfg.n_obs, cfg.obst_stride), "obst")
    if ids is not None:
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(agent.device)
    null = C.c_void_p(0)
    rc = N.lib().dgppo_graph_feats_action_sweep(
        C.byref(cfg), C.c_void_p(agent.data_ptr()), C.c_int64(agent_st), _p(goal, "goal"), _p(obst, "obst") if discs else null,
        C.c_void_p(hits.data_ptr()) if rec_hits else null, C.c_int64(hits_st), _p(ids_dev, "frame_ids", torch.int32),
        C.c_int32(n_frames), C.c_int32(int(agent_id)), _p(us, "us"), C.c_int32(nu), _p(vs, "vs"), C.c_int32(nv), _p(Xa, "Xa"),
        _p(Xo, "Xo") if n_other > 0 else null, _p(efeat, "efeat"), _p(emask, "emask"), C.c_int32(Fp), N.stream_ptr())
    N.check(rc, "dgppo_graph_feats_action_sweep")


def _dense(fn: str, name: str, t_, shape, dtype=torch.float32):
    """a dense CUDA operand of exactly this shape"""
    if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == dtype and t_.is_contiguous()):
        raise ValueError(f"{fn}: {name} must be a contiguous {dtype} CUDA tensor")
    if tuple(t_.shape) != tuple(shape):
        raise ValueError(f"{fn}: {name}: expected shape {tuple(shape)}, got {tuple(t_.shape)}")


def _shield_axes(fn: str, us, vs):
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == torch.float32 and t_.ndim == 1 and t_.is_contiguous()):
            raise ValueError(f"{fn}: {name} must be a dense 1-D float32 CUDA tensor (sweep_axis)")
        if t_.numel() == 0:
            raise ValueError(f"{fn}: {name} is empty")
    return int(us.numel()), int(vs.numel())


def graph_feats_team_action_sweep(cfg: N.EnvCfg, agent, next_agent, goal, obst, next_hits, a_pol, us, vs, Xa, Xo, efeat, emask,
                                  Fp):
    """dgppo_graph_feats_team_action_sweep: the features of the G = B * n * P what-if graphs of one shielded step, P = 1 + nv * nu:
    graph (e, i, p) is next_agent[e] with row i stepped from agent[e, i] by candidate p — a_pol[e, i] for p = 0, (us[iu], vs[iv])
    for p = 1 + iv * nu + iu, clipped to [-1, 1] like every action.  All operands dense: agent / next_agent [B, n, sd], goal
    [B, n_goals, sd], obst [B, n_obs, sd] (MPE kinds), next_hits [B, n, k, 2] (LiDAR kinds with obstacles), a_pol [B, n, 2].
    Every refusal is raised before anything is launched."""
    fn = "graph_feats_team_action_sweep"
    if cfg.is_vmas:
        raise ValueError(f"{fn}: VMASReverseTransport has no sweep entry point")
    n, S, sd = cfg.n_agents, cfg.fan_in, cfg.state_dim
    nu, nv = _shield_axes(fn, us, vs)
    if not (torch.is_tensor(agent) and agent.ndim == 3):
        raise ValueError(f"{fn}: agent must be a [B, n, state_dim] tensor")
    B = int(agent.shape[0])
    G = B * n * (1 + nu * nv)
    n_other = cfg.num_nodes - 1 - n
    _dense(fn, "agent", agent, (B, n, sd))
    _dense(fn, "next_agent", next_agent, (B, n, sd))
    _dense(fn, "goal", goal, (B, cfg.n_goals, sd))
    _dense(fn, "a_pol", a_pol, (B, n, 2))
    _dense(fn, "Xa", Xa, (G * n, Fp))
    if n_other > 0:
        _dense(fn, "Xo", Xo, (G * n_other, Fp))
    _dense(fn, "efeat", efeat, (G * n, S, 4))
    _dense(fn, "emask", emask, (G * n, S))
    rec_hits = cfg.is_lidar and cfg.n_obs > 0
    discs = (not cfg.is_lidar) and cfg.n_obs > 0
    if rec_hits:
        if next_hits is None:
            raise ValueError(f"{fn}: next_hits is required for a LiDAR kind with obstacles")
        _dense(fn, "next_hits", next_hits, (B, n, cfg.top_k, 2))
    if discs:
        if obst is None:
            raise ValueError(f"{fn}: obst is required when n_obs > 0")
        _dense(fn, "obst", obst, (B, cfg.n_obs, cfg.obst_stride))
    null = C.c_void_p(0)
    rc = N.lib().dgppo_graph_feats_team_action_sweep(
        C.byref(cfg), _p(agent, "agent"), _p(next_agent, "next_agent"), _p(goal, "goal"), _p(obst, "obst") if discs else null,
        _p(next_hits, "next_hits") if rec_hits else null, _p(a_pol, "a_pol"), C.c_int32(B), _p(us, "us"), C.c_int32(nu),
        _p(vs, "vs"), C.c_int32(nv), _p(Xa, "Xa"), _p(Xo, "Xo") if n_other > 0 else null, _p(efeat, "efeat"), _p(emask, "emask"),
        C.c_int32(Fp), N.stream_ptr())
    N.check(rc, "dgppo_graph_feats_team_action_sweep")


def shield_select(Vh_next, Vh_t, a_pol, us, vs, dt: float, alpha: float, margin: float, action, index, flag, h=None):
    """dgppo_shield_select on a block of E environments: Vh_next [E * n * P * n, nh] (the Vh forward of the team sweep's graphs,
    P = 1 + nv * nu), Vh_t [E, n, nh], a_pol [E, n, 2] -> action [E, n, 2], index / flag [E, n] int32 and, if given,
    h [E, n, P].  The rule is stated next to the declaration in include/dgppo_hip.h."""
    fn = "shield_select"
    nu, nv = _shield_axes(fn, us, vs)
    P = 1 + nu * nv
    if not (torch.is_tensor(Vh_t) and Vh_t.ndim == 3):
        raise ValueError(f"{fn}: Vh_t must be a [E, n, n_cost] tensor")
    E, n, nh = (int(s) for s in Vh_t.shape)
    if n < 1 or nh < 1:
        raise ValueError(f"{fn}: Vh_t must have at least one agent and one cost component")
    for name, v in (("dt", dt), ("alpha", alpha), ("margin", margin)):
        if not np.isfinite(float(v)):
            raise ValueError(f"{fn}: {name} must be finite")
    if not float(dt) > 0.0:
        raise ValueError(f"{fn}: dt must be > 0")
    _dense(fn, "Vh_t", Vh_t, (E, n, nh))
    _dense(fn, "Vh_next", Vh_next, (E * n * P * n, nh))
    _dense(fn, "a_pol", a_pol, (E, n, 2))
    _dense(fn, "action", action, (E, n, 2))
    _dense(fn, "index", index, (E, n), torch.int32)
    _dense(fn, "flag", flag, (E, n), torch.int32)
    if h is not None:
        _dense(fn, "h", h, (E, n, P))
    rc = N.lib().dgppo_shield_select(
        _p(Vh_next, "Vh_next"), _p(Vh_t, "Vh_t"), _p(a_pol, "a_pol"), C.c_int32(E), C.c_int32(n), C.c_int32(nh), _p(us, "us"),
        C.c_int32(nu), _p(vs, "vs"), C.c_int32(nv), C.c_float(float(dt)), C.c_float(float(alpha)), C.c_float(float(margin)),
        _p(action, "action"), _p(index, "index", torch.int32), _p(flag, "flag", torch.int32), _p(h, "h"), N.stream_ptr())
    N.check(rc, "dgppo_shield_select")


def _shaped(fn: str, operands):
    """operands: (name, tensor, shape[, dtype]) tuples.  Every shape is looked at before anything else — a wrong shape is named
    as such whatever else is wrong with the operands — then each has to be a dense CUDA tensor of its dtype (_dense)."""
    for name, t_, shape, *_ in operands:
        if not torch.is_tensor(t_) or tuple(t_.shape) != tuple(shape):
            got = tuple(t_.shape) if torch.is_tensor(t_) else type(t_).__name__
            raise ValueError(f"{fn}: {name}: expected shape {tuple(shape)}, got {got}")
    for name, t_, shape, *dtype in operands:
        _dense(fn, name, t_, shape, *dtype)


def lookahead_select(cost_tm, a_pol, us, vs, margin: float, action, index, flag, s=None):
    """dgppo_lookahead_select on a block of E environments: cost_tm [K, G, n, nh] are the costs of the K states after the forced
    step of the G = E * n * P what-if envs of ops_env.team_action_fork (slots 1 .. K of the block record's cost_tm; the steps may
    be strided, each is dense), P = 1 + nv * nu; a_pol [E, n, 2] -> action [E, n, 2], index / flag [E, n] int32 and, if given,
    s [E, n, P]: the worst own-row cost of every candidate.  The rule is stated next to the declaration in include/dgppo_hip.h.
    Every refusal is raised before anything is launched."""
    fn = "lookahead_select"
    if not (torch.is_tensor(a_pol) and a_pol.ndim == 3 and a_pol.shape[2] == 2 and a_pol.shape[1] >= 1):
        raise ValueError(f"{fn}: a_pol must be a [E, n, 2] tensor")
    E, n = int(a_pol.shape[0]), int(a_pol.shape[1])
    if not (torch.is_tensor(cost_tm) and cost_tm.ndim == 4):
        raise ValueError(f"{fn}: cost_tm must be a [K, G, n, nh] tensor")
    K_, nh = int(cost_tm.shape[0]), int(cost_tm.shape[3])
    if K_ < 1:
        raise ValueError(f"{fn}: K must be >= 1")
    if not 1 <= nh <= 3:
        raise ValueError(f"{fn}: n_cost {nh} outside [1, 3]")
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.ndim == 1 and t_.numel() > 0):
            raise ValueError(f"{fn}: {name} must be a non-empty 1-D tensor (sweep_axis)")
    P = 1 + int(us.numel()) * int(vs.numel())
    G = E * n * P
    if tuple(cost_tm.shape[1:]) != (G, n, nh):
        raise ValueError(f"{fn}: cost_tm: expected shape (K, {G}, {n}, {nh}), got {tuple(cost_tm.shape)}")
    if np.isnan(float(margin)):
        raise ValueError(f"{fn}: margin must not be NaN")
    _shaped(fn, [("a_pol", a_pol, (E, n, 2)), ("cost_tm[0]", cost_tm[0], (G, n, nh)), ("action", action, (E, n, 2)),
                 ("index", index, (E, n), torch.int32), ("flag", flag, (E, n), torch.int32)]
            + ([("s", s, (E, n, P))] if s is not None else []))
    nu, nv = _shield_axes(fn, us, vs)
    cost_st = int(cost_tm.stride(0)) if K_ > 1 else G * n * nh
    if cost_st < G * n * nh:
        raise ValueError(f"{fn}: the steps of cost_tm overlap (stride {cost_st} < {G * n * nh})")
    rc = N.lib().dgppo_lookahead_select(
        _p(cost_tm[0], "cost"), cost_st, K_, E, n, nh, _p(a_pol, "a_pol"), _p(us, "us"), nu, _p(vs, "vs"), nv, float(margin),
        _p(action, "action"), _p(index, "index", torch.int32), _p(flag, "flag", torch.int32), _p(s, "s"), N.stream_ptr())
    N.check(rc, "dgppo_lookahead_select")


def env_id_list(fn: str, env_ids, n_env: int, unique: bool = True):
    """the env list of the shield-round entry points, checked on the host -> (int32 host array or None, its length).  env_ids:
    None (every env, in order) or a 1-D host array of ints in [0, n_env) — the kernels trust the list, so it is checked here,
    where it costs no device sync — without repeats where `unique` (two workgroups would write one env's rows)."""
    if env_ids is None:
        return None, int(n_env)
    if torch.is_tensor(env_ids):
        if env_ids.is_cuda:
            raise ValueError(f"{fn}: env_ids must be a host array (pass the device copy as ids_dev)")
        env_ids = env_ids.numpy()
    a = np.asarray(env_ids)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{fn}: env_ids must be a 1-D array of ints")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n_env):
        raise ValueError(f"{fn}: env_ids outside [0, {n_env})")
    if unique and np.unique(a).size != a.size:
        raise ValueError(f"{fn}: env_ids repeats an env")
    return np.ascontiguousarray(a, dtype=np.int32), int(a.size)


def env_ids_device(fn: str, ids, ids_dev, device):
    """env_id_list's host list on the device: ids_dev where the caller has uploaded it already (int32, dense, the same length),
    else a fresh copy; None for no list"""
    if ids is None:
        if ids_dev is not None:
            raise ValueError(f"{fn}: ids_dev without env_ids: the host list is what is checked")
        return None
    if ids_dev is None:
        if torch.device(device).type != "cuda":
            raise ValueError(f"{fn}: the operands must be CUDA tensors")
        ids_dev = torch.from_numpy(ids).to(device)
    _dense(fn, "ids_dev", ids_dev, (ids.size,), torch.int32)
    return ids_dev


def lookahead_reselect(cost_tm, env_ids, a_ref, us, vs, margin: float, mode: int, action, index, flag, joint, changed, s=None,
                       ids_dev=None):
    """dgppo_lookahead_reselect: the selection of one shield round on the envs env_ids (None: all, in order) of E.  cost_tm
    [K, G, n, nh] are the costs of the K states after the forced step of the G = len(env_ids) * n * P what-if envs of
    ops_env.team_action_fork_ids (the steps may be strided, each is dense).  a_ref [E, n, 2] is the policy's action, action
    [E, n, 2] (in: the joint action held, candidate 0; out: the one held now) and index [E, n] int32 (in and out), flag [E, n],
    joint / changed [E] int32 and, if given, s [E, n, P].  mode 0: every agent commits its pick; 1: the lowest-numbered agent that
    wants to move moves alone.  The rule is stated next to the declaration in include/dgppo_hip.h.  env_ids / ids_dev: as in
    env_id_list / env_ids_device; rows of envs not listed are not touched.  Every refusal is raised before anything is launched."""
    fn = "lookahead_reselect"
    if not (torch.is_tensor(a_ref) and a_ref.ndim == 3 and a_ref.shape[2] == 2 and a_ref.shape[1] >= 1):
        raise ValueError(f"{fn}: a_ref must be a [E, n, 2] tensor")
    E, n = int(a_ref.shape[0]), int(a_ref.shape[1])
    if not (torch.is_tensor(cost_tm) and cost_tm.ndim == 4):
        raise ValueError(f"{fn}: cost_tm must be a [K, G, n, nh] tensor")
    K_, nh = int(cost_tm.shape[0]), int(cost_tm.shape[3])
    if K_ < 1:
        raise ValueError(f"{fn}: K must be >= 1")
    if not 1 <= nh <= 3:
        raise ValueError(f"{fn}: n_cost {nh} outside [1, 3]")
    for name, t_ in (("us", us), ("vs", vs)):
        if not (torch.is_tensor(t_) and t_.ndim == 1 and t_.numel() > 0):
            raise ValueError(f"{fn}: {name} must be a non-empty 1-D tensor (sweep_axis)")
    if int(mode) not in (0, 1):
        raise ValueError(f"{fn}: mode must be 0 or 1 (got {mode})")
    if np.isnan(float(margin)):
        raise ValueError(f"{fn}: margin must not be NaN")
    ids, M = env_id_list(fn, env_ids, E)
    P = 1 + int(us.numel()) * int(vs.numel())
    G = M * n * P
    if tuple(cost_tm.shape[1:]) != (G, n, nh):
        raise ValueError(f"{fn}: cost_tm: expected shape (K, {G}, {n}, {nh}), got {tuple(cost_tm.shape)}")
    _shaped(fn, [("a_ref", a_ref, (E, n, 2)), ("cost_tm[0]", cost_tm[0], (G, n, nh)), ("action", action, (E, n, 2)),
                 ("index", index, (E, n), torch.int32), ("flag", flag, (E, n), torch.int32), ("joint", joint, (E,), torch.int32),
                 ("changed", changed, (E,), torch.int32)] + ([("s", s, (E, n, P))] if s is not None else []))
    nu, nv = _shield_axes(fn, us, vs)
    ids = env_ids_device(fn, ids, ids_dev, a_ref.device)
    cost_st = int(cost_tm.stride(0)) if K_ > 1 else G * n * nh
    if cost_st < G * n * nh:
        raise ValueError(f"{fn}: the steps of cost_tm overlap (stride {cost_st} < {G * n * nh})")
    rc = N.lib().dgppo_lookahead_reselect(
        _p(cost_tm[0], "cost"), cost_st, K_, M, n, nh, _p(ids, "env_ids", torch.int32), _p(a_ref, "a_ref"), _p(us, "us"), nu,
        _p(vs, "vs"), nv, float(margin), int(mode), _p(action, "action"), _p(index, "index", torch.int32),
        _p(flag, "flag", torch.int32), _p(s, "s"), _p(joint, "joint", torch.int32), _p(changed, "changed", torch.int32),
        N.stream_ptr())
    N.check(rc, "dgppo_lookahead_reselect")


def vmas_graph_feats(cfg: N.EnvCfg, agent, agent_se, agent_st, body, body_se, body_st, scene, env_ids, n_env, n_time,
                     Xa, efeat, emask, Fp):
    """dgppo_vmas_graph_feats: graph_feats for VMASReverseTransport (agent [.., n, 4] and body [.., 4] records addressed
    through strides in floats, scene [B, 8] dense)."""
    G = n_env * n_time
    n = cfg.n_agents
    N.expect_shape(Xa, (G * n, Fp), "Xa")
    N.expect_shape(efeat, (G * n, n, 4), "efeat")
    N.expect_shape(emask, (G * n, n), "emask")
    _check_strided("vmas_graph_feats", "agent", agent, agent_se, agent_st, (n, 4), env_ids, n_env, n_time)
    _check_strided("vmas_graph_feats", "body", body, body_se, body_st, (4,), env_ids, n_env, n_time)
    rc = N.lib().dgppo_vmas_graph_feats(
        C.byref(cfg), C.c_void_p(agent.data_ptr()), C.c_int64(agent_se), C.c_int64(agent_st), C.c_void_p(body.data_ptr()),
        C.c_int64(body_se), C.c_int64(body_st), _p(scene, "scene"), _p(env_ids, "env_ids", torch.int32), C.c_int32(n_env),
        C.c_int32(n_time), _p(Xa, "Xa"), _p(efeat, "efeat"), _p(emask, "emask"), C.c_int32(Fp), N.stream_ptr())
    N.check(rc, "dgppo_vmas_graph_feats")


def attn_fwd(cfg, F, H, Kp, qt, Xa, Xo, efeat, emask, zcat, attn, G):
    n, S = cfg.n_agents, cfg.fan_in
    N.expect_shape(qt, (G * n, H * F), "qt")
    N.expect_shape(Xa, (G * n, F), "Xa")
    N.expect_shape(zcat, (G * n, Kp), "zcat")
    if attn is not None:                                     # None: inference, the attention weights are not kept
        N.expect_shape(attn, (G * n, S, H), "attn")
    FLOPS[0] += 2.0 * G * n * H * S * (2 * F + 4)            # logits (F) + aggregation of [x_s | e] (F + 4) per (agent, head, slot)
    rc = N.lib().dgppo_attn_fwd(C.byref(cfg), F, H, Kp, _p(qt), _p(Xa), _p(Xo), _p(efeat), _p(emask), _p(zcat), _p(attn),
                                G, N.stream_ptr())
    N.check(rc, "dgppo_attn_fwd")


def attn_bwd(cfg, F, H, Kp, dzcat, attn, qt, Xa, Xo, efeat, dqt, dXa, dXo, G, relu_xo: bool = False):
    n = cfg.n_agents
    N.expect_shape(dzcat, (G * n, Kp), "dzcat")
    N.expect_shape(dqt, (G * n, H * F), "dqt")
    if dXa is not None:
        N.expect_shape(dXa, (G * n, F), "dXa")
    FLOPS[0] += 4.0 * G * n * H * cfg.fan_in * (2 * F + 4)   # dA, dL -> dqt, dXs: twice the forward contractions
    rc = N.lib().dgppo_attn_bwd(C.byref(cfg), F, H, Kp, _p(dzcat), _p(attn), _p(qt), _p(Xa), _p(Xo), _p(efeat), _p(dqt),
                                _p(dXa), _p(dXo), int(relu_xo), G, N.stream_ptr())
    N.check(rc, "dgppo_attn_bwd")


def attn_rows_supported(cfg, F, H) -> bool:
    """can the layer's kernels do without efeat (and, backward, without saved weights)?  (dgppo_attn_fwd_rows / _bwd_rows: the
    slot-sparse first-layer kernels on the kinds with a 4-float state)"""
    return bool(N.lib().dgppo_attn_rows_supported(C.byref(cfg), F, H))


def attn_fwd_rows(cfg, F, H, Kp, qt, Xa, Xo, emask, zcat, attn, G):
    """attn_fwd with the edge features formed in the kernel as differences of the node rows: only for features whose efeat IS
    that difference (graph_feats, the act-step kernel)."""
    n, S = cfg.n_agents, cfg.fan_in
    N.expect_shape(qt, (G * n, H * F), "qt")
    N.expect_shape(Xa, (G * n, F), "Xa")
    N.expect_shape(emask, (G * n, S), "emask")
    N.expect_shape(zcat, (G * n, Kp), "zcat")
    if attn is not None:
        N.expect_shape(attn, (G * n, S, H), "attn")
    FLOPS[0] += 2.0 * G * n * H * S * (2 * F + 4) + 4.0 * G * n * S      # attn_fwd + the four differences of every slot
    rc = N.lib().dgppo_attn_fwd_rows(C.byref(cfg), F, H, Kp, _p(qt), _p(Xa), _p(Xo), _p(emask), _p(zcat), _p(attn), G,
                                     N.stream_ptr())
    N.check(rc, "dgppo_attn_fwd_rows")


def attn_bwd_rows(cfg, F, H, Kp, dzcat, attn, qt, emask, Xa, Xo, dqt, G):
    """first-layer attn_bwd (dqt only) without efeat; attn None: the weights are formed again from qt and emask."""
    n, S = cfg.n_agents, cfg.fan_in
    N.expect_shape(dzcat, (G * n, Kp), "dzcat")
    N.expect_shape(Xa, (G * n, F), "Xa")
    N.expect_shape(dqt, (G * n, H * F), "dqt")
    FLOPS[0] += 4.0 * G * n * H * S * (2 * F + 4) + 4.0 * G * n * S
    if attn is None:
        N.expect_shape(qt, (G * n, H * F), "qt")
        N.expect_shape(emask, (G * n, S), "emask")
        FLOPS[0] += 2.0 * G * n * H * S * F                               # the logits again
    else:
        N.expect_shape(attn, (G * n, S, H), "attn")
    rc = N.lib().dgppo_attn_bwd_rows(C.byref(cfg), F, H, Kp, _p(dzcat), _p(attn), _p(qt), _p(emask), _p(Xa), _p(Xo), _p(dqt), G,
                                     N.stream_ptr())
    N.check(rc, "dgppo_attn_bwd_rows")


def attn_xo_supported(cfg, F, H, Kp) -> bool:
    """does the topology have an attention kernel that recomputes the other nodes' rows (dgppo_attn_fwd_xo / _bwd_xo)?"""
    return bool(N.lib().dgppo_attn_xo_supported(C.byref(cfg), F, H, Kp))


def _wo_ptr(Wo):
    if not Wo.is_cuda or Wo.dtype != torch.float32:
        raise TypeError("Wo must be a float32 GPU tensor")
    return C.c_void_p(Wo.data_ptr())


def _wo_ld(Wo):
    if Wo.dim() != 2 or Wo.shape[0] != 8 or Wo.shape[1] < 32 or Wo.stride(1) != 1:
        raise ValueError(f"Wo must be [8, >= 32] with contiguous rows, got {tuple(Wo.shape)} strides {Wo.stride()}")
    return int(Wo.stride(0))


def attn_fwd_xo(cfg, F, H, Kp, qt, Xa, Xo_raw, Wo, bo, efeat, emask, zcat, attn, G):
    """attn_fwd with Xo = relu(Xo_raw Wo + bo) recomputed in the kernel (Xo_raw [G*n_other, 8], Wo [8, 32] rows of a wider matrix)."""
    n, S = cfg.n_agents, cfg.fan_in
    N.expect_shape(qt, (G * n, H * F), "qt")
    N.expect_shape(Xa, (G * n, F), "Xa")
    N.expect_shape(zcat, (G * n, Kp), "zcat")
    N.expect_shape(Xo_raw, (G * (cfg.num_nodes - 1 - n), 8), "Xo_raw")
    N.expect_shape(bo, (32,), "bo")
    if attn is not None:
        N.expect_shape(attn, (G * n, S, H), "attn")
    FLOPS[0] += 2.0 * G * n * H * S * (2 * F + 4) + 2.0 * G * (cfg.num_nodes - 1 - n) * 8 * 32
    rc = N.lib().dgppo_attn_fwd_xo(C.byref(cfg), F, H, Kp, _p(qt), _p(Xa), _p(Xo_raw), _wo_ptr(Wo),
                                   _wo_ld(Wo), _p(bo), _p(efeat), _p(emask), _p(zcat), _p(attn), G, N.stream_ptr())
    N.check(rc, "dgppo_attn_fwd_xo")


def attn_bwd_xo(cfg, F, H, Kp, dzcat, attn, qt, Xa, Xo_raw, Wo, bo, efeat, dqt, dXa, dXo, G, relu_xo: bool = False):
    n = cfg.n_agents
    N.expect_shape(dzcat, (G * n, Kp), "dzcat")
    N.expect_shape(dqt, (G * n, H * F), "dqt")
    N.expect_shape(Xo_raw, (G * (cfg.num_nodes - 1 - n), 8), "Xo_raw")
    if dXa is not None:
        N.expect_shape(dXa, (G * n, F), "dXa")
    FLOPS[0] += 4.0 * G * n * H * cfg.fan_in * (2 * F + 4) + 2.0 * G * (cfg.num_nodes - 1 - n) * 8 * 32
    rc = N.lib().dgppo_attn_bwd_xo(C.byref(cfg), F, H, Kp, _p(dzcat), _p(attn), _p(qt), _p(Xa), _p(Xo_raw),
                                   _wo_ptr(Wo), _wo_ld(Wo), _p(bo), _p(efeat), _p(dqt), _p(dXa), _p(dXo),
                                   int(relu_xo), G, N.stream_ptr())
    N.check(rc, "dgppo_attn_bwd_xo")


def attn_xo_workspace_floats(G: int) -> int:
    return int(N.lib().dgppo_attn_xo_workspace_bytes(int(G))) // 4


def attn_bwd_xo_dw(cfg, F, H, Kp, dzcat, attn, qt, Xa, Xo_raw, Wo, bo, efeat, dqt, dXa, dWo, dbo, workspace, G):
    """attn_bwd_xo that consumes the gradient of the recomputed rows: dWo [8, >= 32 wide rows] += Xo_raw^T (relu' * dXo),
    dbo [32] += its column sums; workspace: attn_xo_workspace_floats(G) floats."""
    n = cfg.n_agents
    N.expect_shape(dzcat, (G * n, Kp), "dzcat")
    N.expect_shape(dqt, (G * n, H * F), "dqt")
    N.expect_shape(dXa, (G * n, F), "dXa")
    N.expect_shape(Xo_raw, (G * (cfg.num_nodes - 1 - n), 8), "Xo_raw")
    N.expect_shape(dbo, (32,), "dbo")
    FLOPS[0] += 4.0 * G * n * H * cfg.fan_in * (2 * F + 4) + 4.0 * G * (cfg.num_nodes - 1 - n) * 8 * 32
    rc = N.lib().dgppo_attn_bwd_xo_dw(C.byref(cfg), F, H, Kp, _p(dzcat), _p(attn), _p(qt), _p(Xa), _p(Xo_raw), _wo_ptr(Wo), _wo_ld(Wo),
                                      _p(bo), _p(efeat), _p(dqt), _p(dXa), _wo_ptr(dWo), _wo_ld(dWo), _p(dbo), _p(workspace),
                                      C.c_int64(workspace.numel() * 4), G, N.stream_ptr())
    N.check(rc, "dgppo_attn_bwd_xo_dw")


def gnn_prep(Wq, bq, Wk, Wv, bv, We, Wu, Mcat, cvec, Wout, F, Fp, D, H, Kp):
    rc = N.lib().dgppo_gnn_prep(_p(Wq), _p(bq), _p(Wk), _p(Wv), _p(bv), _p(We), _p(Wu), _p(Mcat), _p(cvec), _p(Wout),
                                F, Fp, D, H, Kp, N.stream_ptr())
    N.check(rc, "dgppo_gnn_prep")


def gnn_unprep(dMcat, dcvec, dWout, Wq, bq, Wk, dWq, dbq, dWk, dWv, dbv, dWe, dWu, F, Fp, D, H, Kp):
    rc = N.lib().dgppo_gnn_unprep(_p(dMcat), _p(dcvec), _p(dWout), _p(Wq), _p(bq), _p(Wk), _p(dWq), _p(dbq), _p(dWk),
                                  _p(dWv), _p(dbv), _p(dWe), _p(dWu), F, Fp, D, H, Kp, N.stream_ptr())
    N.check(rc, "dgppo_gnn_unprep")


def ln_relu_fwd(x, gamma, beta, y, stats):
    M = x.shape[0]
    N.expect_shape(x, (M, 64), "x")
    N.expect_shape(y, (M, 64), "y")
    rc = N.lib().dgppo_ln_relu_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), M, N.stream_ptr())
    N.check(rc, "dgppo_ln_relu_fwd")


def ln_relu_bwd(x, y, stats, gamma, dy, dx, dgamma, dbeta):
    M = x.shape[0]
    rc = N.lib().dgppo_ln_relu_bwd(_p(x), _p(y), _p(stats), _p(gamma), _p(dy), _p(dx), _p(dgamma), _p(dbeta), M,
                                   N.stream_ptr())
    N.check(rc, "dgppo_ln_relu_bwd")


def gru_fwd(gi, Wh, bhn, h0, hs, hprev, gates, n_seq, T, n_inner):
    rows = n_seq * T
    N.expect_shape(gi, (rows, 192), "gi")
    N.expect_shape(hs, (rows, 64), "hs")
    N.expect_shape(Wh, (64, 192), "Wh")
    if h0 is not None:
        N.expect_shape(h0, (n_seq, 64), "h0")
    FLOPS[0] += 2.0 * rows * 64 * 192
    rc = N.lib().dgppo_gru_fwd(_p(gi), _p(Wh), _p(bhn), _p(h0), _p(hs), _p(hprev), _p(gates), n_seq, T, n_inner,
                               N.stream_ptr())
    N.check(rc, "dgppo_gru_fwd")


class H0Blocks:
    """initial GRU carry read in place from a blocked buffer (dgppo_gru_fwd_h0_blocks): sequence s lives at
    base + (s // rows_per_block) * block_stride + (s % rows_per_block) * 64 floats.  `base` is any float32 CUDA view whose
    first element is that of block 0 (it keeps the storage alive); n_blocks bounds what the kernel may touch."""

    def __init__(self, base: torch.Tensor, rows_per_block: int, block_stride: int, n_blocks: int):
        assert base.dtype == torch.float32 and base.is_cuda
        st = base.untyped_storage()
        last = base.storage_offset() + (n_blocks - 1) * block_stride + rows_per_block * 64
        assert n_blocks >= 1 and last * 4 <= st.nbytes(), "H0Blocks: the blocks leave the storage of base"
        self.base, self.rows_per_block, self.block_stride, self.n_blocks = base, int(rows_per_block), int(block_stride), int(n_blocks)

    @property
    def n_seq(self) -> int:
        return self.n_blocks * self.rows_per_block


def gru_fwd_h0_blocks(gi, Wh, bhn, h0: H0Blocks, hs, hprev, gates, n_seq, T, n_inner):
    rows = n_seq * T
    N.expect_shape(gi, (rows, 192), "gi")
    N.expect_shape(hs, (rows, 64), "hs")
    N.expect_shape(Wh, (64, 192), "Wh")
    if n_seq > h0.n_seq:
        raise ValueError(f"h0: {h0.n_blocks} blocks of {h0.rows_per_block} rows hold fewer than n_seq = {n_seq} carries")
    FLOPS[0] += 2.0 * rows * 64 * 192
    rc = N.lib().dgppo_gru_fwd_h0_blocks(_p(gi), _p(Wh), _p(bhn), C.c_void_p(h0.base.data_ptr()), h0.rows_per_block,
                                         C.c_int64(h0.block_stride), _p(hs), _p(hprev), _p(gates), n_seq, T, n_inner,
                                         N.stream_ptr())
    N.check(rc, "dgppo_gru_fwd_h0_blocks")


class H0Map:
    """initial GRU carry of a T = 1 pass read in place from a record (dgppo_gru_fwd_h0_map, dgppo_gru_bwd_w_t1_map): sequence s
    is cell c = s // n_inner, agent a = s % n_inner, the cell is (e, t) = (c // n_time, c % n_time), and its carry lies at
    base + env * env_stride + t * time_stride + a * 64 floats, env = ids[e] if ids is given else e.  `base` is any float32
    CUDA view whose first element is that of (env 0, t 0, agent 0) (it keeps the storage alive); n_env_src = the envs of the
    record (every id must be below it: the caller vouches for that, the ids live on the device); n_env = the envs of the pass
    (len(ids) with ids)."""

    def __init__(self, base: torch.Tensor, env_stride: int, time_stride: int, n_time: int, n_inner: int, n_env: int,
                 ids: Optional[torch.Tensor] = None, n_env_src: Optional[int] = None):
        assert base.dtype == torch.float32 and base.is_cuda
        if ids is not None:
            if ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous() or ids.dim() != 1:
                raise TypeError("H0Map: ids must be a contiguous 1-d int32 CUDA tensor")
            if int(ids.numel()) != n_env:
                raise ValueError(f"H0Map: {int(ids.numel())} ids for {n_env} envs")
        n_env_src = int(n_env if n_env_src is None else n_env_src)
        assert n_env >= 1 and n_time >= 1 and n_inner >= 1 and n_env_src >= 1 and env_stride >= 0 and time_stride >= 0
        st = base.untyped_storage()
        last = base.storage_offset() + (n_env_src - 1) * env_stride + (n_time - 1) * time_stride + n_inner * 64
        assert last * 4 <= st.nbytes(), "H0Map: the mapped rows leave the storage of base"
        self.base, self.ids = base, ids
        self.env_stride, self.time_stride = int(env_stride), int(time_stride)
        self.n_time, self.n_inner, self.n_env = int(n_time), int(n_inner), int(n_env)

    @property
    def n_seq(self) -> int:
        return self.n_env * self.n_time * self.n_inner

    def dense(self) -> torch.Tensor:
        """[n_seq, 64]: the gathered copy of the mapped rows (tests, tools)"""
        dev = self.base.device
        e = self.ids.long() if self.ids is not None else torch.arange(self.n_env, device=dev)
        t = torch.arange(self.n_time, device=dev)
        a = torch.arange(self.n_inner, device=dev)
        off = (e[:, None, None] * self.env_stride + t[None, :, None] * self.time_stride + a[None, None, :] * 64).reshape(-1)
        flat = torch.as_strided(self.base, (self.base.untyped_storage().nbytes() // 4 - self.base.storage_offset(),), (1,))
        return flat[(off[:, None] + torch.arange(64, device=dev)[None, :])].contiguous()

    def _args(self):
        return (C.c_void_p(self.base.data_ptr()), C.c_void_p(self.ids.data_ptr()) if self.ids is not None else None,
                self.n_env, self.n_time)


def gru_fwd_h0_map(gi, Wh, bhn, h0: H0Map, hs, hprev, gates, n_seq, T, n_inner):
    if T != 1 or n_inner != h0.n_inner:
        raise ValueError(f"a mapped h0 serves one-step passes of its own n_inner = {h0.n_inner} (got T = {T}, n_inner = {n_inner})")
    N.expect_shape(gi, (n_seq, 192), "gi")
    N.expect_shape(hs, (n_seq, 64), "hs")
    N.expect_shape(Wh, (64, 192), "Wh")
    if n_seq > h0.n_seq:
        raise ValueError(f"h0: the map holds {h0.n_seq} carries, fewer than n_seq = {n_seq}")
    FLOPS[0] += 2.0 * n_seq * 64 * 192
    base, ids, n_env, n_time = h0._args()
    rc = N.lib().dgppo_gru_fwd_h0_map(_p(gi), _p(Wh), _p(bhn), base, ids, n_env, n_time, C.c_int64(h0.env_stride),
                                      C.c_int64(h0.time_stride), _p(hs), _p(hprev), _p(gates), n_seq, n_inner, N.stream_ptr())
    N.check(rc, "dgppo_gru_fwd_h0_map")


def mlp_y2_ok(X) -> bool:
    """mlp_gi_fwd(gi=None) serves X: 16-byte addressable rows (the library refuses the others; the parameters of a Net are
    aligned by its layout and checked again there)"""
    return X.is_cuda and X.data_ptr() % 16 == 0 and (X.shape[0] <= 1 or X.stride(0) % 4 == 0)


def gi_gru1_head_ok(y2, h0, hs=None) -> bool:
    """the operands dgppo_gi_gru1_head_fwd accepts: y2 / hs / the base of h0 16-byte aligned, the strides of a blocked or
    mapped h0 multiples of 4 floats (what the library checks: it refuses the others, the separate launches serve them)"""
    def al(t):
        return t is None or (t.is_cuda and t.data_ptr() % 16 == 0)
    if isinstance(h0, H0Blocks):
        ok = al(h0.base) and h0.block_stride % 4 == 0
    elif isinstance(h0, H0Map):
        ok = al(h0.base) and h0.env_stride % 4 == 0 and h0.time_stride % 4 == 0
    else:
        ok = al(h0)
    return bool(ok and y2.is_cuda and al(y2) and al(hs))


def gi_gru1_head_fwd(y2, Wi, bi, Wh, bhn, h0, W1, b1, out, hs=None, gates=None):
    """gi = y2 Wi + bi (kept on chip), one GRU step from h0 and the value head out = h' W1 + b1 in one launch
    (dgppo_gi_gru1_head_fwd).  h0: None (zeros), [M, 64], H0Blocks or H0Map; out [M, n_out <= 16] may be a row-strided view;
    hs [M, 64] / gates [M, 256] are written where given."""
    M = y2.shape[0]
    op, ldo, Mo, n_out = _mat(out, "out")
    N.expect_shape(y2, (M, 64), "y2"); N.expect_shape(Wi, (64, 192), "Wi"); N.expect_shape(bi, (192,), "bi")
    N.expect_shape(Wh, (64, 192), "Wh"); N.expect_shape(bhn, (64,), "bhn")
    N.expect_shape(W1, (64, n_out), "W1"); N.expect_shape(b1, (n_out,), "b1")
    if Mo != M:
        raise ValueError(f"gi_gru1_head_fwd: out {tuple(out.shape)} does not match y2 {tuple(y2.shape)}")
    for t, shp, nm in ((hs, (M, 64), "hs"), (gates, (M, 256), "gates")):
        if t is not None:
            N.expect_shape(t, shp, nm)
    form, base, ids = 0, None, None                  # DGPPO_H0_DENSE / _BLOCKS / _MAP
    rpb = bstride = n_env = n_time = n_inner = es = ts = 0
    if isinstance(h0, H0Blocks):
        if M > h0.n_seq:
            raise ValueError(f"h0: {h0.n_blocks} blocks of {h0.rows_per_block} rows hold fewer than M = {M} carries")
        form, base, rpb, bstride = 1, C.c_void_p(h0.base.data_ptr()), h0.rows_per_block, h0.block_stride
    elif isinstance(h0, H0Map):
        if M > h0.n_seq:
            raise ValueError(f"h0: the map holds {h0.n_seq} carries, fewer than M = {M}")
        base, ids, n_env, n_time = h0._args()
        form, n_inner, es, ts = 2, h0.n_inner, h0.env_stride, h0.time_stride
    else:
        if h0 is not None:
            N.expect_shape(h0, (M, 64), "h0")
        base = _p(h0, "h0")
    FLOPS[0] += 2.0 * M * (2 * 64 * 192 + 64 * n_out)
    rc = N.lib().dgppo_gi_gru1_head_fwd(_p(y2), _p(Wi), _p(bi), _p(Wh), _p(bhn), _p(W1), _p(b1), base, form, rpb,
                                        C.c_int64(bstride), ids, n_env, n_time, n_inner, C.c_int64(es), C.c_int64(ts), op, ldo,
                                        _p(hs), _p(gates), M, n_out, N.stream_ptr())
    N.check(rc, "dgppo_gi_gru1_head_fwd")


class GatherDesc(C.Structure):
    """struct dgppo_gather_desc"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64), ("src_stride", C.c_int64)]


GATHER_MAX = 8      # DGPPO_GATHER_MAX


def gather_rows(pairs, ids):
    """dst[e] = src[ids[e]] for every (src, dst) of `pairs` (at most GATHER_MAX) in ONE launch: torch.index_select along
    dim 0 of each.  src may be a view along dim 0 / dim 1 (its rows dense, any row stride); dst contiguous; ids int32."""
    if ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous():
        raise TypeError("ids must be a contiguous int32 CUDA tensor")
    n_ids = int(ids.numel())
    if len(pairs) > GATHER_MAX:
        raise ValueError(f"gather_rows takes at most {GATHER_MAX} tensors per launch, got {len(pairs)}")
    descs = (GatherDesc * max(len(pairs), 1))()
    for k, (src, dst) in enumerate(pairs):
        if not (src.is_cuda and dst.is_cuda):
            raise RuntimeError("gather_rows: tensors must live on the GPU (the HIP path has no CPU fallback)")
        if src.dtype != dst.dtype or tuple(dst.shape) != (n_ids,) + tuple(src.shape[1:]):
            raise ValueError(f"gather_rows: pair {k}: dst {tuple(dst.shape)} {dst.dtype} does not fit src {tuple(src.shape)} "
                             f"{src.dtype} gathered by {n_ids} ids")
        if not dst.is_contiguous() or (src.shape[0] > 0 and not src[0].is_contiguous()):
            raise ValueError(f"gather_rows: pair {k}: dst and the rows of src must be contiguous")
        row = (src[0].numel() if src.shape[0] > 0 else 0) * src.element_size()
        descs[k] = GatherDesc(src.data_ptr(), dst.data_ptr(), row, src.stride(0) * src.element_size())
    rc = N.lib().dgppo_gather_rows(descs, len(pairs), C.c_void_p(ids.data_ptr()), n_ids, N.stream_ptr())
    N.check(rc, "dgppo_gather_rows")


def gru_bwd(dhs, Wh, hprev, gates, dgi, dgh, n_seq, T, n_inner):
    rows = n_seq * T
    N.expect_shape(dhs, (rows, 64), "dhs")
    N.expect_shape(dgi, (rows, 192), "dgi")
    N.expect_shape(dgh, (rows, 192), "dgh")
    FLOPS[0] += 2.0 * n_seq * (T - 1) * 64 * 192        # the first step forms no dh: nothing reads it
    rc = N.lib().dgppo_gru_bwd(_p(dhs), _p(Wh), _p(hprev), _p(gates), _p(dgi), _p(dgh), n_seq, T, n_inner, N.stream_ptr())
    N.check(rc, "dgppo_gru_bwd")


def gru_bwd_dhn(dhs, Wh, hprev, gates, dgi, dhn, n_seq, T, n_inner):
    """gru_bwd without the duplicate r / z columns: dgi [rows,192] and dhn [rows,64] (= dgh[:, 128:]) for gru_bwd_w"""
    rows = n_seq * T
    N.expect_shape(dhs, (rows, 64), "dhs")
    N.expect_shape(dgi, (rows, 192), "dgi")
    N.expect_shape(dhn, (rows, 64), "dhn")
    FLOPS[0] += 2.0 * n_seq * (T - 1) * 64 * 192
    rc = N.lib().dgppo_gru_bwd_dhn(_p(dhs), _p(Wh), _p(hprev), _p(gates), _p(dgi), _p(dhn), n_seq, T, n_inner, N.stream_ptr())
    N.check(rc, "dgppo_gru_bwd_dhn")


def _gru_bwd_w_call(name, x, hprev, rows_in, dgi, dWi, dbi, dWh, dbhn):
    """the common part of gru_bwd_w / gru_bwd_w_t1: rows_in = the dense row operands between hprev and the outputs"""
    xp, ldx, M, Kx = _mat(x, "x")
    hmap = hprev if isinstance(hprev, H0Map) else None      # gru_bwd_w_t1 alone: h0 read through the carry map
    if hmap is not None:
        if x.shape[0] > hmap.n_seq:
            raise ValueError(f"{name}: the map holds {hmap.n_seq} carries, fewer than M = {x.shape[0]}")
        Mh, Kh = x.shape[0], 64
    else:
        hp, ldh, Mh, Kh = _mat(hprev, "hprev")
    wip, ldwi, _, _ = _mat(dWi, "dWi")
    whp, ldwh, _, _ = _mat(dWh, "dWh")
    if Kx != 64 or (Mh, Kh) != (M, 64) or tuple(dWi.shape) != (64, 192) or tuple(dWh.shape) != (64, 192):
        raise ValueError(f"{name}: shape mismatch x{tuple(x.shape)} hprev{(Mh, Kh)} dWi{tuple(dWi.shape)} "
                         f"dWh{tuple(dWh.shape)}")
    for nm, (t, w) in rows_in.items():
        N.expect_shape(t, (M, w), nm)
    N.expect_shape(dgi, (M, 192), "dgi")
    N.expect_shape(dbi, (192,), "dbi"); N.expect_shape(dbhn, (64,), "dbhn")
    FLOPS[0] += 2.0 * M * 64 * (128 + 64 + 192)      # the three dense_bwd_w calls this replaces
    lib = N.lib()
    need = _workspace_bytes("dgppo_gru_bwd_w_workspace_bytes", x.device)
    batch = BwdWBatch._active.get((x.device.index, torch.cuda.current_stream(x.device).cuda_stream)) if x.is_cuda else None
    if batch is not None:
        ws = batch.region(need)
        d = (ReduceDesc * 3)()
        pend = d
    else:
        key = (x.device.index, torch.cuda.current_stream(x.device).cuda_stream, "gru")
        ws = _WS.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = _WS[key] = torch.empty(need // 4, dtype=torch.float32, device=x.device)
        pend = None
    mid = [_p(t, nm) for nm, (t, w) in rows_in.items()]
    if name == "dgppo_gru_bwd_w":
        mid = [_p(dgi, "dgi")] + mid               # (x, hprev, dgi, dhn, outputs)
    else:
        mid = mid + [_p(dgi, "dgi")]               # (x, h0, dhs, gates, dgi, outputs)
    if hmap is not None:
        base, ids, n_env, n_time = hmap._args()
        name = "dgppo_gru_bwd_w_t1_map"
        h_args = (base, ids, n_env, n_time, hmap.n_inner, C.c_int64(hmap.env_stride), C.c_int64(hmap.time_stride))
    else:
        h_args = (hp, ldh)
    rc = getattr(lib, name)(xp, ldx, *h_args, *mid, wip, ldwi, _p(dbi, "dbi"), whp, ldwh, _p(dbhn, "dbhn"), M,
                            _p(ws, "workspace"), C.c_int64(ws.numel() * 4), pend, N.stream_ptr())
    N.check(rc, name)
    if batch is not None:
        for i in range(3):
            if d[i].pending:
                batch.descs.append(ReduceDesc.from_buffer_copy(d[i]))


def gru_bwd_w(x, hprev, dgi, dhn, dWi, dbi, dWh, dbhn):
    """dWi += x.T @ dgi ; dbi += dgi.sum(0) ; dWh += hprev.T @ [dgi[:, :128] | dhn] ; dbhn += dhn.sum(0) in one pass over the
    rows (inside `with BwdWBatch(...)`: the slab reductions are deferred to the batch's flush, like dense_bwd_w's)"""
    _gru_bwd_w_call("dgppo_gru_bwd_w", x, hprev, {"dhn": (dhn, 64)}, dgi, dWi, dbi, dWh, dbhn)


def gru_bwd_w_t1(x, h0, dhs, gates, dgi, dWi, dbi, dWh, dbhn):
    """gru_bwd_dhn(T = 1, hprev = h0) and gru_bwd_w in one pass: writes dgi [M,192] (the bits gru_bwd_dhn writes) and
    accumulates the four GRU gradients; dhn stays on chip.  The gate gradients are elementwise: no product is counted.
    h0: [M, 64] rows, or an H0Map (both reads of the rows go through the map: dgppo_gru_bwd_w_t1_map)."""
    _gru_bwd_w_call("dgppo_gru_bwd_w_t1", x, h0, {"dhs": (dhs, 64), "gates": (gates, 256)}, dgi, dWi, dbi, dWh, dbhn)


_WS_BYTES: dict = {}   # (query name, device index) -> bytes: constant per device, asked once


def _workspace_bytes(query: str, device) -> int:
    key = (query, device.index)
    if key not in _WS_BYTES:
        fn = getattr(N.lib(), query)
        fn.restype = C.c_int64
        _WS_BYTES[key] = int(fn())
    return _WS_BYTES[key]


def mlp_gi_bwd_w(dgi, Wi, W2, W1, g2, g1, p2, y2, st2, p1, y1, st1, x, relu_mask, dx, dg2, db2, dg1, db1, dW2, dbias2, dW1,
                 dbias1, dpre2=None, dpre1=None):
    """mlp_gi_bwd and the trunk's weight gradients in one kernel (dgppo_mlp_gi_bwd_w): dW2 += y1.T @ dpre2, dbias2 += dpre2.sum(0),
    dW1 += x.T @ dpre1, dbias1 += dpre1.sum(0); x [M,64] is the chain's input (a row-strided view, or the relu_mask tensor).
    dpre2 / dpre1 are written only where given.  Inside `with BwdWBatch(...)` the slab reductions are deferred to its flush."""
    M = dgi.shape[0]
    N.expect_shape(dgi, (M, 192), "dgi")
    for t, shp, nm in ((Wi, (64, 192), "Wi"), (W2, (64, 64), "W2"), (W1, (64, 64), "W1"), (g2, (64,), "g2"), (g1, (64,), "g1"),
                       (p2, (M, 64), "p2"), (y2, (M, 64), "y2"), (st2, (M, 2), "st2"), (p1, (M, 64), "p1"), (y1, (M, 64), "y1"),
                       (st1, (M, 2), "st1"), (dx, (M, 64), "dx"), (dg2, (64,), "dg2"), (db2, (64,), "db2"), (dg1, (64,), "dg1"),
                       (db1, (64,), "db1"), (dbias2, (64,), "dbias2"), (dbias1, (64,), "dbias1")):
        N.expect_shape(t, shp, nm)
    for t, nm in ((dpre2, "dpre2"), (dpre1, "dpre1")):
        if t is not None:
            N.expect_shape(t, (M, 64), nm)
    xp, ldx, Mx, Kx = _mat(x, "x")
    w2p, ldw2, _, _ = _mat(dW2, "dW2")
    w1p, ldw1, _, _ = _mat(dW1, "dW1")
    if (Mx, Kx) != (M, 64) or tuple(dW2.shape) != (64, 64) or tuple(dW1.shape) != (64, 64):
        raise ValueError(f"mlp_gi_bwd_w: shape mismatch x{tuple(x.shape)} dW2{tuple(dW2.shape)} dW1{tuple(dW1.shape)}")
    mp, ldm = C.c_void_p(0), 0
    if relu_mask is not None:
        mp, ldm, Mm, Km = _mat(relu_mask, "relu_mask")
        if (Mm, Km) != (M, 64):
            raise ValueError(f"mlp_gi_bwd_w: relu_mask must be [M, 64], got {tuple(relu_mask.shape)}")
    FLOPS[0] += 2.0 * M * (64 * 64 * 2 + 64 * 192) + 2 * 2.0 * M * 64 * 64      # the chain + the two dense_bwd_w calls it replaces
    lib = N.lib()
    need = _workspace_bytes("dgppo_mlp_gi_bwd_w_workspace_bytes", dgi.device)
    batch = BwdWBatch._active.get((dgi.device.index, torch.cuda.current_stream(dgi.device).cuda_stream))
    d = (ReduceDesc * 2)()
    if batch is not None:
        ws = batch.region(need)
    else:
        key = (dgi.device.index, torch.cuda.current_stream(dgi.device).cuda_stream, "trunk")
        ws = _WS.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = _WS[key] = torch.empty(need // 4, dtype=torch.float32, device=dgi.device)
    rc = lib.dgppo_mlp_gi_bwd_w(_p(dgi), _p(Wi), _p(W2), _p(W1), _p(g2), _p(g1), _p(p2), _p(y2), _p(st2), _p(p1), _p(y1), _p(st1),
                                xp, ldx, mp, ldm, _p(dpre2), _p(dpre1), _p(dx), 64, _p(dg2), _p(db2), _p(dg1), _p(db1),
                                w2p, ldw2, _p(dbias2), w1p, ldw1, _p(dbias1), M, _p(ws, "workspace"), C.c_int64(ws.numel() * 4),
                                d if batch is not None else None, N.stream_ptr())
    N.check(rc, "dgppo_mlp_gi_bwd_w")
    if batch is not None:
        for i in range(2):
            if d[i].pending:
                batch.descs.append(ReduceDesc.from_buffer_copy(d[i]))


def head_bwd(feat, u, dout, W1, W2, dhs, dW1, db1, dW2=None, db2=None):
    """backward of the output head in one kernel (dgppo_head_bwd).  Two layers (policy; u, W2, dW2, db2 given): dW2 += u.T @ dout,
    db2 += dout.sum(0), du = dout @ W2.T, dW1 += feat.T @ du, db1 += du.sum(0), dhs = du @ W1.T.  One layer (values):
    dW1 += feat.T @ dout, db1 += dout.sum(0), dhs = dout @ W1.T.  feat may be a row-strided view.  Inside `with BwdWBatch(...)`
    the slab reductions are deferred to its flush."""
    fp, ldf, M, Kf = _mat(feat, "feat")
    n_out = int(dout.shape[1]) if dout.dim() == 2 else -1
    two = W2 is not None
    if Kf != 64 or not 1 <= n_out <= 16:
        raise ValueError(f"head_bwd: feat must be [M, 64] and dout [M, n_out <= 16], got {tuple(feat.shape)} {tuple(dout.shape)}")
    N.expect_shape(dout, (M, n_out), "dout"); N.expect_shape(dhs, (M, 64), "dhs")
    if two:
        N.expect_shape(u, (M, 64), "u"); N.expect_shape(W1, (64, 64), "W1"); N.expect_shape(W2, (64, n_out), "W2")
        N.expect_shape(db1, (64,), "db1"); N.expect_shape(db2, (n_out,), "db2")
        if tuple(dW1.shape) != (64, 64) or tuple(dW2.shape) != (64, n_out):
            raise ValueError(f"head_bwd: shape mismatch dW1{tuple(dW1.shape)} dW2{tuple(dW2.shape)}")
        w2p, ldw2, _, _ = _mat(dW2, "dW2")
        FLOPS[0] += 2.0 * M * (2 * 64 * n_out + 2 * 64 * 64)       # the four launches it replaces
    else:
        if u is not None or dW2 is not None or db2 is not None:
            raise ValueError("head_bwd: u, dW2, db2 belong to the two-layer form (W2 given)")
        N.expect_shape(W1, (64, n_out), "W1"); N.expect_shape(db1, (n_out,), "db1")
        if tuple(dW1.shape) != (64, n_out):
            raise ValueError(f"head_bwd: shape mismatch dW1{tuple(dW1.shape)}")
        w2p, ldw2 = C.c_void_p(0), 0
        FLOPS[0] += 2.0 * M * 2 * 64 * n_out
    w1p, ldw1, _, _ = _mat(dW1, "dW1")
    lib = N.lib()
    need = _workspace_bytes("dgppo_head_bwd_workspace_bytes", feat.device)
    batch = BwdWBatch._active.get((feat.device.index, torch.cuda.current_stream(feat.device).cuda_stream))
    d = (ReduceDesc * 2)()
    if batch is not None:
        ws = batch.region(need)
    else:
        key = (feat.device.index, torch.cuda.current_stream(feat.device).cuda_stream, "head")
        ws = _WS.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = _WS[key] = torch.empty(need // 4, dtype=torch.float32, device=feat.device)
    rc = lib.dgppo_head_bwd(fp, ldf, _p(u, "u"), _p(dout, "dout"), _p(W1, "W1"), _p(W2, "W2"), _p(dhs, "dhs"), w1p, ldw1,
                            _p(db1, "db1"), w2p, ldw2, _p(db2, "db2"), M, n_out, _p(ws, "workspace"), C.c_int64(ws.numel() * 4),
                            d if batch is not None else None, N.stream_ptr())
    N.check(rc, "dgppo_head_bwd")
    if batch is not None:
        for i in range(2):
            if d[i].pending:
                batch.descs.append(ReduceDesc.from_buffer_copy(d[i]))


def policy_head(ms, eps, action_in, action, log_pi, entropy, n_agents, mode, log_pi_old=None, adv=None, dms=None,
                stats=None, clip_eps=0.25, coef_ent=0.01):
    rows = ms.shape[0]
    N.expect_shape(ms, (rows, 4), "ms")
    rc = N.lib().dgppo_policy_head(_p(ms), _p(eps), _p(action_in), _p(action), _p(log_pi), _p(entropy), rows, n_agents,
                                   mode, _p(log_pi_old), _p(adv), _p(dms), _p(stats), C.c_float(clip_eps),
                                   C.c_float(coef_ent), N.stream_ptr())
    N.check(rc, "dgppo_policy_head")


def value_loss(v, target, dv, stats):
    rc = N.lib().dgppo_value_loss(_p(v), _p(target), _p(dv), _p(stats), v.numel(), N.stream_ptr())
    N.check(rc, "dgppo_value_loss")


def mean_agents(x, y, G, n, D, backward=False, relu_mask=None):
    """backward: False/0 mean, True/1 gradient of the mean, 2 broadcast-add (see the header)"""
    rc = N.lib().dgppo_mean_agents(_p(x), _p(y), G, n, D, int(backward), _p(relu_mask), N.stream_ptr())
    N.check(rc, "dgppo_mean_agents")


def relu_bwd(dy, y):
    rc = N.lib().dgppo_relu_bwd(_p(dy), _p(y), C.c_int64(dy.numel()), N.stream_ptr())
    N.check(rc, "dgppo_relu_bwd")


def lstm_fwd(zi, Wh, bh, c0, h0, cs, hs, cprev, hprev, gates, n_seq, T, n_inner):
    rows = n_seq * T
    N.expect_shape(zi, (rows, 256), "zi"); N.expect_shape(Wh, (64, 256), "Wh"); N.expect_shape(bh, (256,), "bh")
    N.expect_shape(cs, (rows, 64), "cs"); N.expect_shape(hs, (rows, 64), "hs")
    for t, nm in ((c0, "c0"), (h0, "h0")):
        if t is not None:
            N.expect_shape(t, (n_seq, 64), nm)
    FLOPS[0] += 2.0 * rows * 64 * 256
    rc = N.lib().dgppo_lstm_fwd(_p(zi), _p(Wh), _p(bh), _p(c0), _p(h0), _p(cs), _p(hs), _p(cprev), _p(hprev), _p(gates),
                                n_seq, T, n_inner, N.stream_ptr())
    N.check(rc, "dgppo_lstm_fwd")


def lstm_bwd(dhs, Wh, cprev, gates, dz, n_seq, T, n_inner):
    rows = n_seq * T
    N.expect_shape(dhs, (rows, 64), "dhs"); N.expect_shape(dz, (rows, 256), "dz")
    FLOPS[0] += 2.0 * rows * 64 * 256
    rc = N.lib().dgppo_lstm_bwd(_p(dhs), _p(Wh), _p(cprev), _p(gates), _p(dz), n_seq, T, n_inner, N.stream_ptr())
    N.check(rc, "dgppo_lstm_bwd")
