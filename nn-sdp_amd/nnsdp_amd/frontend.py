"""Callers and data formats either side of the hot path, host side:

  read_nnet                 .nnet text reader            exts/nnet_parser.jl:23-131, loadFromNnet network_files.jl:17-22
  makeIntervalsInfo         CROWN-sliced interval bounds  src/Intervals/intervals_auto_lirpa.jl:12-64 (+ auto_LiRPA 0.2 CROWN rules)
  makeQcActivs              QcActivBounded + QcActivSector src/Qc/activ.jl:45-72, makeSectorMinMax activ_sector.jl:63-90
  approxEllipsoid           sampled output ellipsoid      src/Utils/qc.jl:40-67
  findEllipsoid / findCircle / findReach2Dpoly            src/NnSdp.jl:35-95
  runScale                  beta sweep of one network      experiments/scale.jl:52-82 (batch handle)
  write_scale_csv           dump/scale column layout      experiments/scale.jl:60-82

These run once per query on the host; the interval pre-processing is native C++ inside libnnsdp_hip.so
(nnsdp_make_intervals, csrc/intervals.hpp), the SDP itself goes through runQuery -> libnnsdp_hip.so.
"""
from __future__ import annotations

import csv
from typing import List, NamedTuple, Sequence, Tuple

import ctypes as C

import numpy as np

from . import methods as M
from . import _lib


# ----------------------------------------------------------------------------- f3: .nnet reader
def read_nnet(path: str) -> M.FeedFwdNet:
    with open(path, "r") as f:
        lines = [ln.strip() for ln in f if not ln.lstrip().startswith("//")]
    head = [v for v in lines[0].split(",") if v.strip() != ""]
    nlayers = int(head[0])
    sizes = [int(v) for v in lines[1].split(",") if v.strip() != ""][: nlayers + 1]
    pos = 7                     # flag line + mins, maxes, means, ranges are not used by the path
    Ms = []
    for k in range(nlayers):
        nin, nout = sizes[k], sizes[k + 1]
        W = np.array([[float(v) for v in lines[pos + i].split(",")[:nin]] for i in range(nout)], dtype=np.float64)
        pos += nout
        b = np.array([float(lines[pos + i].split(",")[0]) for i in range(nout)], dtype=np.float64)
        pos += nout
        Ms.append(np.hstack([W, b[:, None]]))
    return M.FeedFwdNet(xdims=sizes, Ms=Ms)


def _activ_fn(net: M.FeedFwdNet):
    """makeActiv (src/MyNeuralNetwork/MyNeuralNetwork.jl:29-37)"""
    return np.tanh if M._activ_code(net.activ) == M.ACTIV_TANH else (lambda v: np.maximum(v, 0.0))


def evalFeedFwdNet(net: M.FeedFwdNet, x) -> np.ndarray:
    xk = np.asarray(x, dtype=np.float64)
    vec = xk.ndim == 1
    xk = xk[:, None] if vec else xk
    ac = _activ_fn(net)
    for Mk in net.Ms[:-1]:
        xk = ac(Mk[:, :-1] @ xk + Mk[:, -1:])
    xk = net.Ms[-1][:, :-1] @ xk + net.Ms[-1][:, -1:]
    return xk[:, 0] if vec else xk


def randomNetwork(xdims: Sequence[int], sigma: float = None, seed: int = 1234) -> M.FeedFwdNet:
    """Utils.randomNetwork (src/Utils/Utils.jl:22-26): every [W_k b_k] entry i.i.d. N(0, sigma^2).  Default sigma is the
    scaling experiments' 2 / sqrt(W ln W) with W the hidden width (scripts/make_networks.jl:43-46); numpy's generator, the
    Julia stream of the reference cannot be reproduced."""
    xdims = [int(v) for v in xdims]
    if len(xdims) < 2 or min(xdims) <= 0:
        raise ValueError("xdims needs at least two positive entries")
    if sigma is None:
        width = max(xdims[1:-1]) if len(xdims) > 2 else max(xdims)
        sigma = 2.0 / np.sqrt(width * np.log(width)) if width > 1 else 1.0
    rng = np.random.default_rng(seed)
    return M.FeedFwdNet(xdims=xdims, Ms=[rng.normal(0.0, sigma, size=(xdims[k + 1], xdims[k] + 1)) for k in range(len(xdims) - 1)])


def loadFromFileScaled(path: str, scaling=None):
    """loadFromFileScaled (src/MyNeuralNetwork/network_files.jl:84-114): W_k -> alpha_k W_k, b_k -> prod(alpha[1..k]) b_k, so
    that f'(x) = prod(alpha) f(x) for a ReLU network.  `scaling`: None / "none" (NoScaling), "sqrtlog" (SqrtLogScaling),
    ("norm", v) (FixedNormScaling(Wk_opnorm = v)), ("const", a) (FixedConstScaling(α = a)).  -> (scaled net, alphas)."""
    net = read_nnet(path)
    K = net.K
    Ws, bs = [Mk[:, :-1] for Mk in net.Ms], [Mk[:, -1] for Mk in net.Ms]
    opn = lambda W: float(np.linalg.norm(W, 2))
    if scaling is None or scaling == "none":
        al = np.ones(K)
    elif scaling == "sqrtlog":
        tgt = [np.sqrt(c * np.log(c) / K) for c in (net.xdims[k] + net.xdims[k + 1] for k in range(K))]
        al = np.array([tgt[k] / opn(Ws[k]) for k in range(K)])
    elif isinstance(scaling, tuple) and scaling[0] == "norm":
        al = np.array([float(scaling[1]) / opn(W) for W in Ws])
    elif isinstance(scaling, tuple) and scaling[0] == "const":
        al = float(scaling[1]) * np.ones(K)
    else:
        raise ValueError(f"unrecognized scaling method: {scaling}")
    Ms = [np.hstack([al[k] * Ws[k], (np.prod(al[:k + 1]) * bs[k])[:, None]]) for k in range(K)]
    return M.FeedFwdNet(xdims=list(net.xdims), Ms=Ms), al


def intervalsWorstCase(x1min, x1max, net: M.FeedFwdNet):
    """Intervals.intervalsWorstCase (src/Intervals/intervals_easy.jl:2-37): plain interval arithmetic, ReLU or tanh (both
    monotone).  -> (x_intvs, acx_intvs) like makeIntervalsInfo."""
    lo, hi = np.asarray(x1min, dtype=np.float64), np.asarray(x1max, dtype=np.float64)
    ac = _activ_fn(net)
    x_intvs, acx = [(lo, hi)], []
    for k, Mk in enumerate(net.Ms):
        W, b = Mk[:, :-1], Mk[:, -1]
        pl = np.maximum(W, 0) @ lo + np.minimum(W, 0) @ hi + b
        pu = np.maximum(W, 0) @ hi + np.minimum(W, 0) @ lo + b
        if k < net.K - 1:
            acx.append((pl, pu))
            lo, hi = ac(pl), ac(pu)
        else:
            lo, hi = pl, pu
        x_intvs.append((lo, hi))
    return x_intvs, acx


def makeSectorMinMax(acxmin, acxmax, activ=M.ReluActiv):
    """Qc.makeSectorMinMax (src/Qc/activ_sector.jl:63-90), both activations, same arithmetic (including 0/0 = NaN for a tanh
    pre-activation bound that is exactly 0, as in the reference)."""
    acxmin, acxmax = np.asarray(acxmin, dtype=np.float64), np.asarray(acxmax, dtype=np.float64)
    if len(acxmin) != len(acxmax):
        raise ValueError("acxmin / acxmax length mismatch")
    eps = 1e-4
    code = M._activ_code(activ)
    if code == M.ACTIV_RELU:
        return (acxmin > eps).astype(np.float64), 1.0 - (acxmax < -eps).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tlo, thi = np.tanh(acxmin) / acxmin, np.tanh(acxmax) / acxmax
    same = acxmin * acxmax >= 0
    return np.where(same, thi, np.minimum(tlo, thi)), np.where(same, tlo, 1.0)


def makeQcActivsIntvs(net: M.FeedFwdNet, x_intvs, acx_intvs, beta: int):
    """Qc.makeQcActivsIntvs (src/Qc/activ.jl:45-66) from given interval information."""
    acymin = np.concatenate([iv[0] for iv in x_intvs[1:-1]])
    acymax = np.concatenate([iv[1] for iv in x_intvs[1:-1]])
    smin, smax = makeSectorMinMax(np.concatenate([iv[0] for iv in acx_intvs]), np.concatenate([iv[1] for iv in acx_intvs]), net.activ)
    return [M.QcActivBounded(acymin=acymin, acymax=acymax),
            M.QcActivSector(acxdim=len(acymin), beta=int(beta), smin=smin, smax=smax, activ=net.activ)]


# ----------------------------------------------------------------------------- f1: CROWN-sliced intervals
def _intervals_native(x1min, x1max, net: M.FeedFwdNet):
    """nnsdp_make_intervals_activ (host C++ in the library, csrc/intervals.hpp): replaces the reference's per-layer
    PyCall + ONNX + auto_LiRPA round trips (src/Intervals/intervals_auto_lirpa.jl:12-64), ReLU and Tanh networks
    (BoundRelu / BoundTanh relaxations, exts/auto_lirpa_bridge.py:31-37)."""
    lib = _lib.load()
    xd = np.asarray(net.xdims, dtype=np.int32)
    K = net.K
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    lo = np.ascontiguousarray(x1min, dtype=np.float64)
    hi = np.ascontiguousarray(x1max, dtype=np.float64)
    if lo.shape != (xd[0],) or hi.shape != (xd[0],):
        raise ValueError("x1min / x1max must have xdims[0] entries")
    acdim = int(xd[1:-1].sum())
    outs = [np.zeros(acdim) for _ in range(6)] + [np.zeros(int(xd[-1])) for _ in range(2)]
    dp = _lib.c_double_p
    _lib.check(lib.nnsdp_make_intervals_activ(K, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp), M._activ_code(net.activ),
                                              lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in outs]))
    return outs


def makeIntervalsInfo(x1min, x1max, net: M.FeedFwdNet):
    """returns (x_intvs, acx_intvs): K+1 post-activation intervals and K-1 pre-activation intervals
    (Intervals.makeIntervalsInfo with the sliced auto_LiRPA method, intervals_auto_lirpa.jl:31-64)."""
    acymin, acymax, acxmin, acxmax, _, _, ymin, ymax = _intervals_native(x1min, x1max, net)
    x_intvs = [(np.asarray(x1min, dtype=np.float64), np.asarray(x1max, dtype=np.float64))]
    acx, o = [], 0
    for k in range(1, net.K):
        n = net.xdims[k]
        x_intvs.append((acymin[o:o + n], acymax[o:o + n]))
        acx.append((acxmin[o:o + n], acxmax[o:o + n]))
        o += n
    x_intvs.append((ymin, ymax))
    return x_intvs, acx


def makeQcActivs(net: M.FeedFwdNet, x1min, x1max, beta: int):
    """Qc.makeQcActivs (src/Qc/activ.jl:45-72): bounded + sector QCs from the interval pre-processing."""
    acymin, acymax, _, _, smin, smax, _, _ = _intervals_native(x1min, x1max, net)
    return [M.QcActivBounded(acymin=acymin, acymax=acymax),
            M.QcActivSector(acxdim=len(acymin), beta=int(beta), smin=smin, smax=smax, activ=net.activ)]


def _net_arrays(net: M.FeedFwdNet):
    xd = np.asarray(net.xdims, dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    return xd, Mp


class LiteralBounds(NamedTuple):
    """bounds of nlit literals  normal_i' f(x)  on nbox boxes (makeIntervalsBatch with normals):
    smin <= normal' f(x) <= smax  and  normal' f(x) <= A[i, :, b]' x + b0[i, b]  on box b; smax = A' c + |A|' r + b0 (centre, radius)"""
    smin: np.ndarray      # nlit x nbox, raw (no min / max post-fix)
    smax: np.ndarray      # nlit x nbox
    A: np.ndarray         # nlit x n0 x nbox
    b0: np.ndarray        # nlit x nbox
    # set by a call with optimised slopes (LiteralBoundsAlpha); a plain call's result has the four fields above and nothing else
    smax_plain = None
    alpha = None
    best_step = None


class LiteralBoundsAlpha(LiteralBounds):
    """LiteralBounds of a call with optimised ReLU slopes (alpha_steps > 0 or alpha0): smax / A / b0 are, per box and literal, those of
    whichever of the plain pass and the alpha iteration has the smaller smax; smax_plain (nlit x nbox) is the plain pass's smax, alpha
    (nlit x acdim x nbox) the slopes the iteration ended with (the plain rule at neurons that are not unstable) and best_step
    (nlit x nbox, int32) the iterate they came from.  As a tuple it is the four fields of LiteralBounds."""

    def __new__(cls, smin, smax, A, b0, a_smax, a_A, a_b0, alpha, best_step):
        take = a_smax < smax
        self = super().__new__(cls, smin, np.where(take, a_smax, smax), np.where(take[:, None, :], a_A, A), np.where(take, a_b0, b0))
        self.smax_plain, self.alpha, self.best_step = smax, alpha, best_step
        return self


def _alpha_args(alpha_steps, alpha0, eta0, decay, nlit, acdim, nbox):
    """the checked alpha options of makeIntervalsBatch / CrownBounder.bound: alpha0 as nbox x nlit x acdim (C order) or None"""
    if nlit is None:
        raise ValueError("optimised slopes (alpha_steps / alpha0) need literal normals")
    if alpha0 is not None:
        alpha0 = np.asarray(alpha0, dtype=np.float64)
        if alpha0.shape != (nlit, acdim, nbox):
            raise ValueError("alpha0 must be nlit x acdim x nbox")
        alpha0 = np.ascontiguousarray(alpha0.transpose(2, 0, 1))
    return int(alpha_steps), float(eta0), float(decay), alpha0


def _alpha_outs(nbox, nlit, n0, acdim):
    return [np.zeros((nbox, nlit)), np.zeros((nbox, nlit, n0)), np.zeros((nbox, nlit)), np.zeros((nbox, nlit, acdim))], \
        np.zeros((nbox, nlit), dtype=np.int32)


def _alpha_lits(louts, aouts, step):
    return LiteralBoundsAlpha(louts[0].T, louts[1].T, louts[2].transpose(1, 2, 0), louts[3].T, aouts[0].T, aouts[1].transpose(1, 2, 0),
                              aouts[2].T, aouts[3].transpose(1, 2, 0), step.T)


def _host_pool(one, nbox: int, workers: int, entry: str):
    """one(b) -> return code of a one-box library call, for every box on at most 16 threads (ctypes releases the GIL)"""
    nw = max(1, min(int(workers), 16, nbox))
    if nw == 1:
        for b in range(nbox):
            _lib.check(one(b))
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=nw) as pool:
            codes = list(pool.map(one, range(nbox)))
        if any(codes):
            raise _lib.NnsdpError(next(c for c in codes if c), f"{entry} failed for a box of the batch")


def makeIntervalsBatch(net: M.FeedFwdNet, lo, hi, backend: str = "host", workers: int = 16, return_ms: bool = False, normals=None,
                       alpha_steps: int = 0, alpha0=None, eta0: float = 0.5, decay: float = 0.9):
    """CROWN-sliced bounds of many input boxes of one network: lo / hi are xdims[0] x nbox, one column per box.
    -> (acymin, acymax, acxmin, acxmax, ymin, ymax), one column per box.
    normals (nlit x xdims[K], nlit <= 64): the literals  normal_i' f(x)  are bounded in the same call by one more backward pass whose
    head is the normal folded into the last affine layer; the six arrays (same bits) are followed by a LiteralBounds.
    backend="gpu":  nnsdp_make_intervals_batch (csrc/crown_batch.hpp), one launch, fp64; ReLU networks with every width <= 64,
                    anything else raises (no fall-back to the host).
    backend="host": nnsdp_make_intervals_activ (csrc/intervals.hpp, float32 arithmetic by design) once per box on a thread pool
                    of at most 16 workers (ctypes releases the GIL); the only one-shot route for Tanh networks (CrownBounder below
                    bounds them on the GPU) and the only route for wider layers, and the default until the kernel has been timed
                    against it (tools/split_timing.py).
    alpha_steps > 0 or alpha0 (nlit x acdim x nbox), backend="host" with normals, ReLU: the literals' upper bounds with optimised
    lower slopes of the unstable ReLUs (nnsdp_make_intervals_lits_alpha); the last element is then a LiteralBoundsAlpha.  On the
    GPU this is CrownBounder.bound (crown_backend "resident" of the split driver)."""
    lib = _lib.load()
    want_alpha = alpha_steps != 0 or alpha0 is not None
    if want_alpha and backend == "gpu":
        raise ValueError('optimised slopes (alpha) are not part of backend="gpu": use backend="host", or a CrownBounder ("resident")')
    xd, Mp = _net_arrays(net)
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    if lo.ndim != 2 or lo.shape[0] != xd[0] or hi.shape != lo.shape:
        raise ValueError("lo / hi must be xdims[0] x nbox")
    nbox = lo.shape[1]
    acdim, ny = int(xd[1:-1].sum()), int(xd[-1])
    loc, hic = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)          # column-major xdims[0] x nbox
    outs = [np.zeros((nbox, acdim)) for _ in range(4)] + [np.zeros((nbox, ny)) for _ in range(2)]
    dp = _lib.c_double_p
    ms = C.c_double(0.0)
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=np.float64)                   # nlit x ny row-major = ny x nlit column-major
        if nrm.ndim != 2 or nrm.shape[1] != ny:
            raise ValueError("normals must be nlit x xdims[K]")
        nlit, n0 = nrm.shape[0], int(xd[0])
        louts = [np.zeros((nbox, nlit)), np.zeros((nbox, nlit)), np.zeros((nbox, nlit, n0)), np.zeros((nbox, nlit))]    # smin, smax, uA, ub0
        xdp, Mpp, nrp = xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp), nrm.ctypes.data_as(dp)
        if want_alpha and backend == "host":
            steps, eta0, decay, a0 = _alpha_args(alpha_steps, alpha0, eta0, decay, nlit, acdim, nbox)
            aouts, step = _alpha_outs(nbox, nlit, n0, acdim)
            activ = M._activ_code(net.activ)

            def one_alpha(b):
                rows = [o[b].ctypes.data_as(dp) for o in outs]
                return lib.nnsdp_make_intervals_lits_alpha(net.K, xdp, Mpp, activ, loc[b].ctypes.data_as(dp), hic[b].ctypes.data_as(dp),
                                                           rows[0], rows[1], rows[2], rows[3], None, None, rows[4], rows[5], nlit, nrp,
                                                           *[o[b].ctypes.data_as(dp) for o in louts], steps, eta0, decay,
                                                           None if a0 is None else a0[b].ctypes.data_as(dp),
                                                           *[o[b].ctypes.data_as(dp) for o in aouts], step[b].ctypes.data_as(_lib.c_int32_p))

            _host_pool(one_alpha, nbox, workers, "nnsdp_make_intervals_lits_alpha")
            res = tuple(o.T for o in outs) + (_alpha_lits(louts, aouts, step),)
            return res + (ms.value,) if return_ms else res
        if backend == "gpu":
            _lib.check(lib.nnsdp_make_intervals_batch_lits(net.K, xdp, Mpp, M._activ_code(net.activ), nbox, loc.ctypes.data_as(dp),
                                                           hic.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in outs], nlit, nrp,
                                                           *[o.ctypes.data_as(dp) for o in louts], C.byref(ms)))
        elif backend == "host":
            activ = M._activ_code(net.activ)

            def one_lits(b):
                rows = [o[b].ctypes.data_as(dp) for o in outs]
                return lib.nnsdp_make_intervals_lits(net.K, xdp, Mpp, activ, loc[b].ctypes.data_as(dp), hic[b].ctypes.data_as(dp),
                                                     rows[0], rows[1], rows[2], rows[3], None, None, rows[4], rows[5], nlit, nrp,
                                                     *[o[b].ctypes.data_as(dp) for o in louts])

            _host_pool(one_lits, nbox, workers, "nnsdp_make_intervals_lits")
        else:
            raise ValueError("backend must be 'gpu' or 'host'")
        lits = LiteralBounds(louts[0].T, louts[1].T, louts[2].transpose(1, 2, 0), louts[3].T)
        res = tuple(o.T for o in outs) + (lits,)
        return res + (ms.value,) if return_ms else res
    if backend == "gpu":
        _lib.check(lib.nnsdp_make_intervals_batch(net.K, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp), M._activ_code(net.activ),
                                                  nbox, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp),
                                                  *[o.ctypes.data_as(dp) for o in outs], C.byref(ms)))
    elif backend == "host":
        activ = M._activ_code(net.activ)
        xdp, Mpp = xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp)

        def one(b):
            rows = [o[b] for o in outs]
            return lib.nnsdp_make_intervals_activ(net.K, xdp, Mpp, activ, loc[b].ctypes.data_as(dp), hic[b].ctypes.data_as(dp),
                                                  rows[0].ctypes.data_as(dp), rows[1].ctypes.data_as(dp), rows[2].ctypes.data_as(dp),
                                                  rows[3].ctypes.data_as(dp), None, None, rows[4].ctypes.data_as(dp), rows[5].ctypes.data_as(dp))

        _host_pool(one, nbox, workers, "nnsdp_make_intervals_activ")
    else:
        raise ValueError("backend must be 'gpu' or 'host'")
    if want_alpha:
        raise ValueError("optimised slopes (alpha_steps / alpha0) need literal normals")
    res = tuple(o.T for o in outs)
    return res + (ms.value,) if return_ms else res


class NodeBounds(NamedTuple):
    """bounds on nnode nodes of a ReLU split (CrownBounder.bound_nodes, makeIntervalsNodes): node b is the box lo[:, b] / hi[:, b] with
    the assignment assign[:, b] in {-1, 0, +1} (+1: z_n >= 0, -1: z_n <= 0, 0: free), and every number is valid over the points of
    the box that satisfy the forced signs.  normal_i' f(x) <= A[i, :, b]' x + b0[i, b] there, and smax = A' c + |A|' r + b0."""
    pre_lo: np.ndarray        # acdim x nnode: the pre-activation bounds, clipped at the forced neurons
    pre_hi: np.ndarray
    smin: np.ndarray          # nlit x nnode
    smax_plain: np.ndarray    # nlit x nnode: without multipliers
    smax: np.ndarray          # nlit x nnode: the best iterate of the multiplier steps, never above smax_plain
    A: np.ndarray             # nlit x n0 x nnode, of that iterate
    b0: np.ndarray            # nlit x nnode
    best_step: np.ndarray     # nlit x nnode, int32
    branch: np.ndarray        # nlit x nnode, int32: the neuron to branch on for the literal, -1 without a candidate
    infeasible: np.ndarray    # nnode, bool: a forced sign contradicts the bounds; the node's other numbers mean nothing


def _node_args(lo, hi, assign, n0, acdim):
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    if lo.ndim != 2 or lo.shape[0] != n0 or hi.shape != lo.shape:
        raise ValueError("lo / hi must be xdims[0] x nnode")
    asg = np.asarray(assign)
    if asg.shape != (acdim, lo.shape[1]):
        raise ValueError("assign must be acdim x nnode")
    if not np.isin(asg, (-1, 0, 1)).all():
        raise ValueError("assign must hold -1, 0 or +1")
    return np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T), np.ascontiguousarray(asg.T, dtype=np.int8)


def _node_outs(nnode, nlit, n0, acdim):
    dbl = [np.zeros((nnode, acdim)), np.zeros((nnode, acdim))] + [np.zeros((nnode, nlit)) for _ in range(3)] + \
        [np.zeros((nnode, nlit, n0)), np.zeros((nnode, nlit))]
    return dbl, [np.zeros((nnode, nlit), dtype=np.int32), np.zeros((nnode, nlit), dtype=np.int32), np.zeros(nnode, dtype=np.int32)]


def _node_bounds(dbl, ints):
    return NodeBounds(dbl[0].T, dbl[1].T, dbl[2].T, dbl[3].T, dbl[4].T, dbl[5].transpose(1, 2, 0), dbl[6].T, ints[0].T, ints[1].T,
                      ints[2].astype(bool))


def makeIntervalsNodes(net: M.FeedFwdNet, lo, hi, assign, normals, steps: int = 0, eta0: float = 0.5, decay: float = 0.9,
                       workers: int = 16) -> NodeBounds:
    """bounds on the nodes of a ReLU split from the float32 host routine (nnsdp_make_intervals_nodes, csrc/intervals.hpp), one call per
    node on a thread pool of at most 16 workers; no GPU needed.  lo / hi xdims[0] x nnode, assign acdim x nnode, normals nlit x xdims[K].
    The GPU route is CrownBounder.bound_nodes."""
    lib = _lib.load()
    xd, Mp = _net_arrays(net)
    n0, acdim, ny = int(xd[0]), int(xd[1:-1].sum()), int(xd[-1])
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    if nrm is not None and (nrm.ndim != 2 or nrm.shape[1] != ny):
        raise ValueError("normals must be nlit x xdims[K]")
    nlit = 0 if nrm is None else nrm.shape[0]
    loc, hic, asg = _node_args(lo, hi, assign, n0, acdim)
    nnode, dp, ip, bp = loc.shape[0], _lib.c_double_p, _lib.c_int32_p, C.POINTER(C.c_int8)
    dbl, ints = _node_outs(nnode, nlit, n0, acdim)
    xdp, Mpp, nrp, activ = xd.ctypes.data_as(ip), Mp.ctypes.data_as(dp), None if nrm is None else nrm.ctypes.data_as(dp), M._activ_code(net.activ)

    def one(b):
        return lib.nnsdp_make_intervals_nodes(net.K, xdp, Mpp, activ, loc[b].ctypes.data_as(dp), hic[b].ctypes.data_as(dp),
                                              asg[b].ctypes.data_as(bp), nlit, nrp, int(steps), float(eta0), float(decay),
                                              *[o[b].ctypes.data_as(dp) for o in dbl], ints[0][b].ctypes.data_as(ip),
                                              ints[1][b].ctypes.data_as(ip), ints[2][b:b + 1].ctypes.data_as(ip))

    if nnode:
        _lib.check(one(0))          # the refusals of the arguments, with their message
        if nnode > 1:
            _host_pool(lambda b: one(b + 1), nnode - 1, workers, "nnsdp_make_intervals_nodes")
    return _node_bounds(dbl, ints)


# ----------------------------------------------------------------------------- f2: callers of the path
def evalFeedFwdNetBatch(net: M.FeedFwdNet, X, return_ms: bool = False):
    """the network at the columns of X (xdims[0] x N) on the GPU: nnsdp_eval_network (csrc/forward.hpp, fp64 MFMA, one wave per
    16 samples).  No host fallback: raises without a GPU.  evalFeedFwdNet above is the reference's pointwise function."""
    lib = _lib.load()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != net.xdims[0]:
        raise ValueError("X must be xdims[0] x N")
    N = X.shape[1]
    xd = np.asarray(net.xdims, dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    Xc = np.ascontiguousarray(X.T)                      # column-major xdims[0] x N
    Y = np.empty((N, int(xd[-1])), dtype=np.float64)
    ms = C.c_double(0.0)
    dp = _lib.c_double_p
    _lib.check(lib.nnsdp_eval_network(net.K, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp), M._activ_code(net.activ), N,
                                      Xc.ctypes.data_as(dp), Y.ctypes.data_as(dp), C.byref(ms)))
    return (Y.T, ms.value) if return_ms else Y.T


_CONFIRM = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_double))      # nnsdp_confirm_fn
_CONFIRM_MANY = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_double))      # nnsdp_confirm_many_fn


def forestPlan(n0: int, ny: int, nlit: int, max_boxes: int, corner_points: bool = False, nroot: int = 1, group: int = 0) -> dict:
    """nnsdp_crown_forest_plan: how CrownBounder.search_many groups nroot roots (no GPU needed): the roots per group, the boxes a level
    of a group can hold and the bytes of its frontier, point / leaf-log and record buffers, each within the cap of 2^31 bytes; raises
    ValueError with the byte count when one root alone does not fit."""
    out = (C.c_int64 * 5)()
    _lib.check(_lib.load().nnsdp_crown_forest_plan(int(n0), int(ny), int(nlit), int(max_boxes), int(bool(corner_points)), int(nroot), int(group), out))
    return dict(group=int(out[0]), level_capacity=int(out[1]), frontier_bytes=int(out[2]), point_log_bytes=int(out[3]), record_bytes=int(out[4]))


class CrownBounder:
    """makeIntervalsBatch(backend="gpu") and evalFeedFwdNetBatch for many calls on one network (the nnsdp_crown handle of include/nnsdp.h):
    the network, the literal head of `normals` (nlit x xdims[K], nlit <= 64) and every device buffer stay on the GPU until close().
    ReLU and Tanh networks with every width <= 64; anything else raises (no fall-back to the host).  The ReLU results have the bits of
    makeIntervalsBatch(backend="gpu"); the Tanh kernel exists only here.
    max_width=128 (nnsdp_crown_create_wide) asks for the wide instance of the kernel (csrc/crown_wide.hpp): hidden layers up to 128
    wide, while xdims[0], xdims[K] and nlit stay at 64 or below.  It runs one workgroup per CU where the narrow one runs two, so it is
    never chosen silently; on a network of widths <= 64 it returns the bits of the narrow instance.  bound, eval, search, search_many,
    reach and info work on it; optimised slopes (alpha_steps, alpha0) do not - the alpha kernel keeps its 64-wide layout - and raise ValueError,
    and neither do bound_nodes and search_nodes (the ReLU split's node kernels keep that layout too).
    A context manager; not thread-safe."""

    _INFO = ("device_allocations", "network_uploads", "box_capacity", "sample_capacity", "bound_calls", "device_bytes", "reach_calls")
    # search_nodes: calls, status records read back (one per level), levels whose flags and points were downloaded (nnsdp_crown_info 8..10)
    _INFO_NODES = ((8, "node_searches"), (9, "node_search_levels"), (10, "node_point_downloads"))

    def __init__(self, net: M.FeedFwdNet, normals=None, max_width: int = 64):
        self._h = None
        if max_width not in (64, 128):
            raise ValueError("max_width must be 64 or 128")
        self._max_width = int(max_width)
        self._lib = _lib.load()
        self.net = net
        xd, Mp = _net_arrays(net)
        self._n0, self._acdim, self._ny = int(xd[0]), int(xd[1:-1].sum()), int(xd[-1])
        self._nlit, nrp = None, None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float64)               # nlit x ny row-major = ny x nlit column-major
            if nrm.ndim != 2 or nrm.shape[1] != self._ny:
                raise ValueError("normals must be nlit x xdims[K]")
            self._nlit, nrp = nrm.shape[0], nrm.ctypes.data_as(_lib.c_double_p)
        h = C.c_void_p()
        args = (net.K, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(_lib.c_double_p), M._activ_code(net.activ), self._nlit or 0, nrp)
        if self._max_width == 64:
            _lib.check(self._lib.nnsdp_crown_create(*args, C.byref(h)))
        else:
            _lib.check(self._lib.nnsdp_crown_create_wide(*args, self._max_width, C.byref(h)))
        self._h = h

    @property
    def max_width(self) -> int:
        """the widest hidden layer the handle's kernel takes (nnsdp_crown_info 7): 64, or 128 for the wide instance"""
        v = C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_info(self._handle(), 7, C.byref(v)))
        return int(v.value)

    def _handle(self):
        if self._h is None:
            raise ValueError("the CrownBounder is closed")
        return self._h

    def bound(self, lo, hi, return_ms: bool = False, alpha_steps: int = 0, alpha0=None, eta0: float = 0.5, decay: float = 0.9):
        """what makeIntervalsBatch(net, lo, hi, backend="gpu"[, normals=...]) returns: the six arrays, then a LiteralBounds when the
        bounder has normals, then the kernel's event time with return_ms.
        alpha_steps > 0 or alpha0 (nlit x acdim x nbox): nnsdp_crown_bound_alpha, a second kernel behind the plain one that optimises the
        lower slopes of the unstable ReLUs for the literals' upper bounds (csrc/crown_alpha.hpp); the LiteralBounds is then a
        LiteralBoundsAlpha, never looser than the plain one, and the event time covers both kernels.  ReLU bounders with normals."""
        h = self._handle()
        lo = np.asarray(lo, dtype=np.float64)
        hi = np.asarray(hi, dtype=np.float64)
        if lo.ndim != 2 or lo.shape[0] != self._n0 or hi.shape != lo.shape:
            raise ValueError("lo / hi must be xdims[0] x nbox")
        nbox, dp = lo.shape[1], _lib.c_double_p
        loc, hic = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)      # column-major xdims[0] x nbox
        outs = [np.zeros((nbox, self._acdim)) for _ in range(4)] + [np.zeros((nbox, self._ny)) for _ in range(2)]
        louts = []
        if self._nlit is not None:
            nl = self._nlit
            louts = [np.zeros((nbox, nl)), np.zeros((nbox, nl)), np.zeros((nbox, nl, self._n0)), np.zeros((nbox, nl))]    # smin, smax, uA, ub0
        ms = C.c_double(0.0)
        if alpha_steps != 0 or alpha0 is not None:
            if self._max_width != 64:
                raise ValueError("optimised slopes (alpha_steps, alpha0) are not available on a wide bounder (max_width=128)")
            steps, eta0, decay, a0 = _alpha_args(alpha_steps, alpha0, eta0, decay, self._nlit, self._acdim, nbox)
            aouts, step = _alpha_outs(nbox, self._nlit, self._n0, self._acdim)
            _lib.check(self._lib.nnsdp_crown_bound_alpha(h, nbox, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp),
                                                         *[o.ctypes.data_as(dp) for o in outs + louts], C.byref(ms), steps, eta0, decay,
                                                         None if a0 is None else a0.ctypes.data_as(dp),
                                                         *[o.ctypes.data_as(dp) for o in aouts], step.ctypes.data_as(_lib.c_int32_p)))
            res = tuple(o.T for o in outs) + (_alpha_lits(louts, aouts, step),)
            return res + (ms.value,) if return_ms else res
        _lib.check(self._lib.nnsdp_crown_bound(h, nbox, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in outs],
                                               *([o.ctypes.data_as(dp) for o in louts] or [None] * 4), C.byref(ms)))
        res = tuple(o.T for o in outs)
        if self._nlit is not None:
            res += (LiteralBounds(louts[0].T, louts[1].T, louts[2].transpose(1, 2, 0), louts[3].T),)
        return res + (ms.value,) if return_ms else res

    def bound_nodes(self, lo, hi, assign, steps: int = 0, eta0: float = 0.5, decay: float = 0.9, return_ms: bool = False):
        """nnsdp_crown_bound_nodes: bounds on the nodes of a ReLU split (csrc/crown_relu_split.hpp) -> NodeBounds (then the event time of
        both kernels with return_ms).  lo / hi xdims[0] x nnode; assign acdim x nnode in {-1, 0, +1}; steps multiplier steps per literal.
        Narrow ReLU bounders with normals; anything else raises before the GPU is touched."""
        h = self._handle()
        loc, hic, asg = _node_args(lo, hi, assign, self._n0, self._acdim)
        nnode, dp, ip = loc.shape[0], _lib.c_double_p, _lib.c_int32_p
        dbl, ints = _node_outs(nnode, self._nlit or 0, self._n0, self._acdim)
        ms = C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_bound_nodes(h, nnode, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp), asg.ctypes.data_as(C.POINTER(C.c_int8)),
                                                     int(steps), float(eta0), float(decay), *[o.ctypes.data_as(dp) for o in dbl],
                                                     *[o.ctypes.data_as(ip) for o in ints], C.byref(ms)))
        res = _node_bounds(dbl, ints)
        return (res, ms.value) if return_ms else res

    def eval(self, X, return_ms: bool = False):
        """what evalFeedFwdNetBatch(net, X) returns, from the resident network"""
        h = self._handle()
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != self._n0:
            raise ValueError("X must be xdims[0] x N")
        N, dp = X.shape[1], _lib.c_double_p
        Xc = np.ascontiguousarray(X.T)                      # column-major xdims[0] x N
        Y = np.empty((N, self._ny), dtype=np.float64)
        ms = C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_eval(h, N, Xc.ctypes.data_as(dp), Y.ctypes.data_as(dp), C.byref(ms)))
        return (Y.T, ms.value) if return_ms else Y.T

    def search(self, lo, hi, hs, *, normals=None, literal_bounds: bool = False, corner_points: bool = False, max_boxes: int = 512,
               max_depth: int = 24, chunk: int = 4096, confirm=None) -> dict:
        """nnsdp_crown_search: the bounds-only bisection search of split.verifySplit on the root box lo / hi (xdims[0] each) for the clause
        OR_i normal_i' f(x) <= hs[i], with the frontier kept on the GPU (csrc/crown_search.hpp).  The normals are the bounder's; a bounder
        without normals takes `normals` (nlit x xdims[K]) and has neither literal_bounds nor corner_points.  confirm(x) -> bool decides
        whether a point that the device flagged is a witness (None: the first flagged point is).  Returns the pieces of a SplitResult:
        verdict, visited, depth, witness (or None), kernel_ms, and the leaves as arrays in the Python loop's order: lo, hi (nleaves x
        xdims[0]), depth, proved (1 "crown", 0 open), literal (-1: never bounded), bound."""
        h, dp, ip = self._handle(), _lib.c_double_p, _lib.c_int32_p
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self._n0,) or hi.shape != (self._n0,):
            raise ValueError("lo / hi must have xdims[0] entries")
        hs = np.ascontiguousarray(hs, dtype=np.float64)
        nrp = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float64)               # nlit x ny row-major = ny x nlit column-major
            if nrm.ndim != 2 or nrm.shape != (hs.size, self._ny):
                raise ValueError("normals must be len(hs) x xdims[K]")
            nrp = nrm.ctypes.data_as(dp)
        if hs.ndim != 1 or hs.size < 1:
            raise ValueError("hs must have one threshold per literal")
        failed = []

        def call(_user, x):
            try:
                return 1 if confirm(np.ctypeslib.as_array(x, shape=(self._n0,)).copy()) else 0
            except BaseException as e:       # an exception cannot cross the C frames: the search ends at this level, it is raised again below
                failed.append(e)
                return 1

        keep = _CONFIRM(call) if confirm is not None else None
        cb = C.cast(keep, C.c_void_p) if keep is not None else None
        out = (C.c_int32 * 4)()
        wit, ms = np.zeros(self._n0), C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_search(h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), hs.size, nrp, hs.ctypes.data_as(dp),
                                                int(bool(literal_bounds)), int(bool(corner_points)), int(max_boxes), int(max_depth), int(chunk),
                                                cb, None, *[C.cast(C.byref(out, 4 * k), ip) for k in range(4)],
                                                wit.ctypes.data_as(dp), C.byref(ms)))
        if failed:
            raise failed[0]
        verdict, visited, depth, n = (int(v) for v in out)
        llo, lhi = np.zeros((n, self._n0)), np.zeros((n, self._n0))
        ldepth, lproved, llit = (np.zeros(n, dtype=np.int32) for _ in range(3))
        lbound = np.zeros(n)
        _lib.check(self._lib.nnsdp_crown_search_leaves(h, llo.ctypes.data_as(dp), lhi.ctypes.data_as(dp), ldepth.ctypes.data_as(ip),
                                                       lproved.ctypes.data_as(ip), llit.ctypes.data_as(ip), lbound.ctypes.data_as(dp)))
        return dict(verdict=("holds", "violated", "unknown")[verdict], visited=visited, depth=depth, witness=wit if verdict == 1 else None,
                    kernel_ms=ms.value, lo=llo, hi=lhi, leaf_depth=ldepth, proved=lproved, literal=llit, bound=lbound)

    def search_many(self, lo, hi, hs, *, normals=None, literal_bounds: bool = False, corner_points: bool = False, max_boxes: int = 512,
                    max_depth: int = 24, chunk: int = 4096, group: int = 0, confirm=None) -> dict:
        """nnsdp_crown_search_many: search() for the R root boxes lo / hi (xdims[0] x R) with the thresholds hs (nlit x R), one column per
        root, in one level loop on the GPU (csrc/crown_forest.hpp); max_boxes and max_depth apply to every root alone.  Per root the
        result is the one search() gives on that root, bit for bit.  group: roots that share the device buffers at a time (0: derived
        from the memory cap, forestPlan); the result does not depend on it.  confirm(r, x) -> bool decides whether a point that the
        device flagged for root r is its witness (None: the first flagged point is).  Returns per-root arrays verdict (R strings),
        visited, depth (R), witness (R x xdims[0], NaN rows where the root is not violated), one kernel_ms, and the leaves of all roots,
        one root after the other, as search() returns them: lo, hi, leaf_depth, proved, literal, bound, with leaf_start (R + 1): root
        r owns the leaves leaf_start[r] .. leaf_start[r + 1] - 1."""
        h, dp, ip = self._handle(), _lib.c_double_p, _lib.c_int32_p
        lo = np.asarray(lo, dtype=np.float64)
        hi = np.asarray(hi, dtype=np.float64)
        if lo.ndim != 2 or lo.shape[0] != self._n0 or hi.shape != lo.shape:
            raise ValueError("lo / hi must be xdims[0] x R")
        R = lo.shape[1]
        hs = np.asarray(hs, dtype=np.float64)
        if hs.ndim != 2 or hs.shape[0] < 1 or hs.shape[1] != R:
            raise ValueError("hs must be nlit x R: one threshold per literal and root")
        nlit = hs.shape[0]
        nrp = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float64)               # nlit x ny row-major = ny x nlit column-major
            if nrm.ndim != 2 or nrm.shape != (nlit, self._ny):
                raise ValueError("normals must be len(hs) x xdims[K]")
            nrp = nrm.ctypes.data_as(dp)
        loc, hic, hsc = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T), np.ascontiguousarray(hs.T)      # column-major
        failed = []

        def call(_user, r, x):
            try:
                return 1 if confirm(int(r), np.ctypeslib.as_array(x, shape=(self._n0,)).copy()) else 0
            except BaseException as e:       # an exception cannot cross the C frames: the root ends at this level, it is raised again below
                failed.append(e)
                return 1

        keep = _CONFIRM_MANY(call) if confirm is not None else None
        cb = C.cast(keep, C.c_void_p) if keep is not None else None
        verdict, visited, depth, nleaves = (np.zeros(R, dtype=np.int32) for _ in range(4))
        wit, ms = np.full((R, self._n0), np.nan), C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_search_many(h, R, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp), nlit, nrp, hsc.ctypes.data_as(dp),
                                                     int(bool(literal_bounds)), int(bool(corner_points)), int(max_boxes), int(max_depth),
                                                     int(chunk), int(group), cb, None, verdict.ctypes.data_as(ip), visited.ctypes.data_as(ip),
                                                     depth.ctypes.data_as(ip), nleaves.ctypes.data_as(ip), wit.ctypes.data_as(dp), C.byref(ms)))
        if failed:
            raise failed[0]
        start = np.zeros(R + 1, dtype=np.int64)
        np.cumsum(nleaves, out=start[1:])
        n = int(start[-1])
        llo, lhi = np.zeros((n, self._n0)), np.zeros((n, self._n0))
        ldepth, lproved, llit = (np.zeros(n, dtype=np.int32) for _ in range(3))
        lbound = np.zeros(n)
        if R:
            _lib.check(self._lib.nnsdp_crown_search_many_leaves(h, -1, llo.ctypes.data_as(dp), lhi.ctypes.data_as(dp), ldepth.ctypes.data_as(ip),
                                                                lproved.ctypes.data_as(ip), llit.ctypes.data_as(ip), lbound.ctypes.data_as(dp)))
        names = np.array(["holds", "violated", "unknown"], dtype=object)
        return dict(verdict=names[verdict], visited=visited, depth=depth, witness=wit, kernel_ms=ms.value, lo=llo, hi=lhi, leaf_depth=ldepth,
                    proved=lproved, literal=llit, bound=lbound, leaf_start=start)

    def reach(self, lo, hi, tol, *, corner_points: bool = False, max_boxes: int = 512, max_depth: int = 24, chunk: int = 4096) -> dict:
        """nnsdp_crown_reach: the bounds-only level loop of split.reachSplit on the root box lo / hi (xdims[0] each) for the bounder's
        directions, with the frontier and the incumbents kept on the GPU (csrc/crown_reach.hpp); tol: one tolerance per direction (or a
        scalar).  Returns the pieces of a ReachSplitResult: status, visited, depth, incumbent (nlit), witnesses (nlit x xdims[0]),
        kernel_ms, and the leaves as arrays in the Python loop's order: lo, hi (nleaves x xdims[0]), leaf_depth, closed (1 "crown",
        0 open), bound (nleaves x nlit)."""
        h, dp, ip = self._handle(), _lib.c_double_p, _lib.c_int32_p
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self._n0,) or hi.shape != (self._n0,):
            raise ValueError("lo / hi must have xdims[0] entries")
        nlit = self._nlit or 0
        tol = np.ascontiguousarray(tol, dtype=np.float64)
        if tol.ndim == 0:
            tol = np.full(max(nlit, 1), float(tol))
        if tol.ndim != 1 or tol.size != max(nlit, 1):
            raise ValueError("tol must be a scalar or one tolerance per direction")
        out = (C.c_int32 * 4)()
        inc, wit, ms = np.zeros(max(nlit, 1)), np.zeros((max(nlit, 1), self._n0)), C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_reach(h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), nlit, tol.ctypes.data_as(dp),
                                               int(bool(corner_points)), int(max_boxes), int(max_depth), int(chunk),
                                               *[C.cast(C.byref(out, 4 * k), ip) for k in range(4)],
                                               inc.ctypes.data_as(dp), wit.ctypes.data_as(dp), C.byref(ms)))
        status, visited, depth, n = (int(v) for v in out)
        llo, lhi, lbound = np.zeros((n, self._n0)), np.zeros((n, self._n0)), np.zeros((n, nlit))
        ldepth, lclosed = (np.zeros(n, dtype=np.int32) for _ in range(2))
        _lib.check(self._lib.nnsdp_crown_reach_leaves(h, llo.ctypes.data_as(dp), lhi.ctypes.data_as(dp), ldepth.ctypes.data_as(ip),
                                                      lclosed.ctypes.data_as(ip), lbound.ctypes.data_as(dp)))
        return dict(status=("converged", "budget")[status], visited=visited, depth=depth, incumbent=inc, witnesses=wit, kernel_ms=ms.value,
                    lo=llo, hi=lhi, leaf_depth=ldepth, closed=lclosed, bound=lbound)

    def search_nodes(self, lo, hi, hs, *, steps: int = 16, eta0: float = 0.5, decay: float = 0.9, corner_points: bool = True,
                     max_nodes: int = 4096, max_depth: int = 64, chunk: int = 4096, confirm=None) -> dict:
        """nnsdp_crown_search_nodes: the level loop of relusplit.verifyReluSplit on the root box lo / hi (xdims[0] each) for the clause
        OR_i normal_i' f(x) <= hs[i] of the bounder's literals, with the node frontier kept on the GPU (csrc/crown_node_search.hpp).
        confirm(x) -> bool decides whether a point that the device flagged is a witness (None: the first flagged point is).  Returns
        the pieces of a ReluSplitResult: verdict, reason (None, "budget", "exhausted"), visited, depth, witness (or None), kernel_ms,
        nleaves, and the closed leaves followed by the open nodes, in the Python loop's order, as arrays: assign (rows x acdim, int8),
        leaf_depth, closed_by (0 infeasible, 1 bound, -1 open), bound."""
        h, dp, ip = self._handle(), _lib.c_double_p, _lib.c_int32_p
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self._n0,) or hi.shape != (self._n0,):
            raise ValueError("lo / hi must have xdims[0] entries")
        hs = np.ascontiguousarray(hs, dtype=np.float64)
        if hs.ndim != 1 or hs.size < 1:
            raise ValueError("hs must have one threshold per literal")
        failed = []

        def call(_user, x):
            try:
                return 1 if confirm(np.ctypeslib.as_array(x, shape=(self._n0,)).copy()) else 0
            except BaseException as e:       # an exception cannot cross the C frames: the search ends at this level, it is raised again below
                failed.append(e)
                return 1

        keep = _CONFIRM(call) if confirm is not None else None
        cb = C.cast(keep, C.c_void_p) if keep is not None else None
        out = (C.c_int32 * 6)()
        wit, ms = np.zeros(self._n0), C.c_double(0.0)
        _lib.check(self._lib.nnsdp_crown_search_nodes(h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), hs.size, hs.ctypes.data_as(dp), int(steps),
                                                      float(eta0), float(decay), int(bool(corner_points)), int(max_nodes), int(max_depth),
                                                      int(chunk), cb, None, *[C.cast(C.byref(out, 4 * k), ip) for k in range(6)],
                                                      wit.ctypes.data_as(dp), C.byref(ms)))
        if failed:
            raise failed[0]
        verdict, reason, visited, depth, nleaves, nopen = (int(v) for v in out)
        n = nleaves + nopen
        assign = np.zeros((n, self._acdim), dtype=np.int8)
        ldepth, lby = (np.zeros(n, dtype=np.int32) for _ in range(2))
        lbound = np.zeros(n)
        _lib.check(self._lib.nnsdp_crown_search_nodes_leaves(h, assign.ctypes.data_as(C.POINTER(C.c_int8)), ldepth.ctypes.data_as(ip),
                                                             lby.ctypes.data_as(ip), lbound.ctypes.data_as(dp)))
        return dict(verdict=("holds", "violated", "unknown")[verdict], reason=(None, "budget", "exhausted")[reason], visited=visited, depth=depth,
                    witness=wit if verdict == 1 else None, kernel_ms=ms.value, nleaves=nleaves, assign=assign, leaf_depth=ldepth,
                    closed_by=lby, bound=lbound)

    def info(self) -> dict:
        h, v, out = self._handle(), C.c_double(0.0), {}
        for what, name in tuple(enumerate(self._INFO)) + self._INFO_NODES:
            _lib.check(self._lib.nnsdp_crown_info(h, what, C.byref(v)))
            out[name] = int(v.value)
        return out

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.check(self._lib.nnsdp_crown_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sampleTrajs(net: M.FeedFwdNet, x1min, x1max, N: int = 100000, seed: int = 1234):
    """Utils.sampleTrajs (src/Utils/qc.jl:40-47): outputs of N inputs drawn uniformly from the box, xdims[K] x N.  The draw is
    numpy's default_rng(seed) on the host (the Julia stream of the reference cannot be regenerated); the N forward passes run
    on the GPU."""
    rng = np.random.default_rng(seed)
    x1min = np.asarray(x1min, dtype=np.float64)
    x1max = np.asarray(x1max, dtype=np.float64)
    return evalFeedFwdNetBatch(net, x1min[:, None] + rng.random((net.xdims[0], N)) * (x1max - x1min)[:, None])


def approxEllipsoid(net: M.FeedFwdNet, x1min, x1max, N: int = 100000, seed: int = 1234):
    """Utils.approxEllipsoid (src/Utils/qc.jl:50-67)"""
    Y = sampleTrajs(net, x1min, x1max, N, seed)
    yc = Y.sum(axis=1) / N
    Yd = Y - yc[:, None]
    P = Yd @ Yd.T
    w, V = np.linalg.eigh(P)
    a, b = 1.0, 4.0
    if w.max() * a >= w.min() * b:
        P = V @ np.diag((w - w.min()) * ((b - a) / (w.max() - w.min())) + a) @ V.T
        P = 0.5 * (P + P.T)
    return P, yc


def findEllipsoid(net, x1min, x1max, beta: int, opts: M.AdmmSdpOptions, seed: int = 1234):
    q, P, yc = ellipsoidQuery(net, x1min, x1max, beta, seed=seed)
    soln = M.runQuery(q, opts)
    rho = max(float(soln.values["γout"][0]), 0.0)
    return np.sqrt(rho) * P, yc, soln


def findCircle(net, x1min, x1max, beta: int, opts: M.AdmmSdpOptions):
    yc = evalFeedFwdNet(net, (np.asarray(x1max, float) + np.asarray(x1min, float)) / 2)
    q = M.ReachQuery(ffnet=net, qc_input=M.QcInputBox(x1min=x1min, x1max=x1max), qc_reach=M.QcReachCircle(yc=yc),
                     qc_activs=makeQcActivs(net, x1min, x1max, beta))
    return M.runQuery(q, opts)


def findReach2Dpoly(net, x1min, x1max, beta: int, opts: M.AdmmSdpOptions, num_hplanes: int = 6, batched: bool = True,
                    share_setup: bool = False):
    """NnSdp.findReach2Dpoly (src/NnSdp.jl:73-95): one reach-hyperplane SDP per direction.  The directions share the
    network and the interval pre-processing and are independent SDPs of identical shape: solved in lockstep through
    the batch handle (`batched=False`: one after the other, as the reference does).  share_setup=True (batched only): the
    directions differ in the hyperplane normal only, so they are created as one solver family - one operator, one M^-1."""
    qc_input = M.QcInputBox(x1min=x1min, x1max=x1max)
    qc_activs = makeQcActivs(net, x1min, x1max, beta)
    normals = [np.array([np.cos(2 * np.pi * i / num_hplanes), np.sin(2 * np.pi * i / num_hplanes)]) for i in range(num_hplanes)]
    queries = [M.ReachQuery(ffnet=net, qc_input=qc_input, qc_reach=M.QcReachHplane(normal=nrm), qc_activs=qc_activs) for nrm in normals]
    solns = M.runQueries(queries, opts, share_setup=share_setup) if batched and len(queries) > 1 else [M.runQuery(q, opts) for q in queries]
    return [(nrm, s.objective_value) for nrm, s in zip(normals, solns)], solns


def ellipsoidQuery(net, x1min, x1max, beta: int, seed: int = 1234):
    """the ReachQuery NnSdp.findEllipsoid solves (src/NnSdp.jl:35-50) and the sampled shape matrix P."""
    qc_input = M.QcInputBox(x1min=x1min, x1max=x1max)
    qc_activs = makeQcActivs(net, x1min, x1max, beta)
    P, yc = approxEllipsoid(net, x1min, x1max, seed=seed)
    invP = np.linalg.inv(P)
    q = M.ReachQuery(ffnet=net, qc_input=qc_input, qc_reach=M.QcReachEllipsoid(invP=0.5 * (invP + invP.T), yc=yc), qc_activs=qc_activs)
    return q, P, yc


def runScale(net, x1min, x1max, betas: Sequence[int], opts: M.AdmmSdpOptions, saveto: str = None, batched: bool = True, seed: int = 1234):
    """The reference's headline experiment (experiments/scale.jl:52-82): findEllipsoid for every beta of a sweep on one
    network, one CSV row per beta.  The SDPs of a sweep are independent and of different sizes (the sector QC grows with
    beta): `batched` advances them in lockstep through the batch handle, each stopping on its own rule.
    -> list of (beta, QuerySolution)."""
    queries = [ellipsoidQuery(net, x1min, x1max, int(b), seed=seed)[0] for b in betas]
    solns = M.runQueries(queries, opts) if batched and len(queries) > 1 else [M.runQuery(q, opts) for q in queries]
    rows = list(zip([int(b) for b in betas], solns))
    if saveto:
        write_scale_csv(saveto, rows)
    return rows


def write_scale_csv(path: str, rows: Sequence[Tuple[int, M.QuerySolution]]):
    """beta,setup_secs,solve_secs,total_secs,obj_val,term_status,eigmax (experiments/scale.jl:60-82)."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["beta", "setup_secs", "solve_secs", "total_secs", "obj_val", "term_status", "eigmax"])
        for beta, s in rows:
            w.writerow([beta, s.setup_time, s.solve_time, s.total_time, s.objective_value, s.termination_status, s.summary["lambda_max"]])
