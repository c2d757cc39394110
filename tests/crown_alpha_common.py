"""Shared by the alpha-CROWN tests (test_crown_alpha_*.py): the numpy yardstick of the optimised-slope literal pass.  `R_at` is the
literal backward pass of literal_common.R at a given lower slope alpha of the unstable neurons, `grad` the analytic gradient of its
smax with respect to alpha, `R_alpha` the projected-gradient iteration of DESIGN.md section 5 (tests/test_crown_alpha_cpu.py pins the
yardstick itself without any product code), the cases of both test files, the raw calls of the two C entries and the checks that the
host routine and the kernel share.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np

import literal_common as lc
import nnsdp_amd as na
from nnsdp_amd import _lib

_cache = {}


def _net(Ms, dt):
    return [np.asarray(Mk[:, :-1], dtype=dt) for Mk in Ms], [np.asarray(Mk[:, -1], dtype=dt) for Mk in Ms]


def _relax(l, u, dt):
    """du, dl, bu of literal_common.R's backward, and the mask of the unstable neurons (l < 0 < u)"""
    zero = dt(0)
    lr = np.minimum(l, zero)
    ur = np.maximum(np.maximum(u, zero), lr + dt(1e-8))
    du = ur / (ur - lr)
    return du, (du > dt(0.5)).astype(dt), -lr * du, (l < zero) & (u > zero)


def pre_bounds(Ms, lo, hi, dt):
    """the raw pre-activation bounds of the hidden layers as literal_common.R computes them: [(l, u)], each nbox x width"""
    W, b = _net(Ms, dt)
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)
    c, r = (hi + lo) / dt(2), (hi - lo) / dt(2)
    nbox, zero, pre = lo.shape[0], dt(0), []
    for k in range(1, len(Ms)):
        lA = np.broadcast_to(W[k - 1], (nbox,) + W[k - 1].shape).copy()
        uA = lA.copy()
        lb = np.broadcast_to(b[k - 1], (nbox, len(b[k - 1]))).copy()
        ub = lb.copy()
        for j in range(k - 2, -1, -1):
            du, dl, bu, _ = _relax(*pre[j], dt)
            lAp, lAn, uAp, uAn = np.maximum(lA, zero), np.minimum(lA, zero), np.maximum(uA, zero), np.minimum(uA, zero)
            lb = lb + np.einsum("bit,bt->bi", lAn, bu)
            ub = ub + np.einsum("bit,bt->bi", uAp, bu)
            lA = lAp * dl[:, None, :] + lAn * du[:, None, :]
            uA = uAp * du[:, None, :] + uAn * dl[:, None, :]
            lb = lb + lA @ b[j]
            ub = ub + uA @ b[j]
            lA, uA = lA @ W[j], uA @ W[j]
        pre.append((np.einsum("biq,bq->bi", lA, c) - np.einsum("biq,bq->bi", np.abs(lA), r) + lb,
                    np.einsum("biq,bq->bi", uA, c) + np.einsum("biq,bq->bi", np.abs(uA), r) + ub))
    return pre


def _split(alpha, Ms, dt):
    """alpha (nlit x acdim x nbox) -> per hidden layer nbox x nlit x width"""
    out, o = [], 0
    for Mk in Ms[:-1]:
        d = Mk.shape[0]
        out.append(np.asarray(alpha[:, o:o + d, :], dtype=dt).transpose(2, 0, 1))
        o += d
    return out


def _join(parts):
    return np.concatenate(parts, axis=2).transpose(1, 2, 0)       # nlit x acdim x nbox


def plain_alpha(Ms, lo, hi, dt, nlit, pre=None):
    """the plain rule dl of every hidden neuron, repeated for every literal: nlit x acdim x nbox"""
    pre = pre_bounds(Ms, lo, hi, dt) if pre is None else pre
    return _join([np.repeat(_relax(l, u, dt)[1][:, None, :], nlit, axis=1) for l, u in pre])


def unstable_mask(Ms, lo, hi, dt, pre=None):
    """acdim x nbox"""
    pre = pre_bounds(Ms, lo, hi, dt) if pre is None else pre
    return np.concatenate([_relax(l, u, dt)[3] for l, u in pre], axis=1).T


def _backward(W, b, pre, head, lo, hi, dt, als):
    """the upper matrix of R's literal pass with the lower slope als[j] on the unstable neurons of layer j -> smax, uA, ub (box first),
    the coefficients lambda per layer before the slopes scale them, and the slopes used"""
    K, zero = len(W), dt(0)
    Cm = np.asarray(head, dtype=dt)
    nbox = lo.shape[0]
    Hw, Hb = Cm @ W[K - 1], Cm @ b[K - 1]
    uA = np.broadcast_to(Hw, (nbox,) + Hw.shape).copy()
    ub = np.broadcast_to(Hb, (nbox, len(Hb))).copy()
    lam, eff = [None] * (K - 1), [None] * (K - 1)
    for j in range(K - 2, -1, -1):
        du, dl, bu, uns = _relax(*pre[j], dt)
        al = np.where(uns[:, None, :], als[j], dl[:, None, :])
        lam[j], eff[j] = uA, al
        uAp, uAn = np.maximum(uA, zero), np.minimum(uA, zero)
        ub = ub + np.einsum("bit,bt->bi", uAp, bu)
        uA = uAp * du[:, None, :] + uAn * al
        ub = ub + uA @ b[j]
        uA = uA @ W[j]
    c, r = (hi + lo) / dt(2), (hi - lo) / dt(2)
    smax = np.einsum("biq,bq->bi", uA, c) + np.einsum("biq,bq->bi", np.abs(uA), r) + ub
    return smax, uA, ub, lam, eff


def _grad(W, b, pre, lo, hi, dt, uA, lam, eff):
    """g per layer (nbox x nlit x width): min(lambda, 0) z on the unstable neurons, z the pre-activation of the relaxed network that
    the backward pass chose, at the maximiser x* = c + sgn(uA) r"""
    zero = dt(0)
    c, r = (hi + lo) / dt(2), (hi - lo) / dt(2)
    a = c[:, None, :] + np.sign(uA) * r[:, None, :]
    g = []
    for j in range(len(W) - 1):
        z = a @ W[j].T + b[j]
        du, _, bu, uns = _relax(*pre[j], dt)
        g.append(np.where(uns[:, None, :], np.minimum(lam[j], zero) * z, zero))
        a = np.where(lam[j] > zero, du[:, None, :] * z + bu[:, None, :], eff[j] * z)
    return g


def R_at(Ms, lo, hi, dt, head, alpha, pre=None):
    """one literal backward pass at alpha (nlit x acdim x nbox; entries at neurons that are not unstable are ignored)
    -> smax (nlit x nbox), A (nlit x n0 x nbox), b0 (nlit x nbox)"""
    W, b = _net(Ms, dt)
    pre = pre_bounds(Ms, lo, hi, dt) if pre is None else pre
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)
    smax, uA, ub, _, _ = _backward(W, b, pre, head, lo, hi, dt, _split(alpha, Ms, dt))
    return smax.T, uA.transpose(1, 2, 0), ub.T


def grad(Ms, lo, hi, dt, head, alpha, pre=None):
    """d smax / d alpha at alpha: nlit x acdim x nbox, zero at the neurons that are not unstable"""
    W, b = _net(Ms, dt)
    pre = pre_bounds(Ms, lo, hi, dt) if pre is None else pre
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)
    _, uA, _, lam, eff = _backward(W, b, pre, head, lo, hi, dt, _split(alpha, Ms, dt))
    return _join(_grad(W, b, pre, lo, hi, dt, uA, lam, eff))


def R_alpha(Ms, lo, hi, dt, head, steps, eta0=0.5, decay=0.9, alpha0=None):
    """the whole iteration -> dict: smax, A, b0, alpha, best_step of the first iterate with the smallest smax, and `trace`
    ((steps + 1) x nlit x nbox, the smax of every iterate)"""
    W, b = _net(Ms, dt)
    pre = pre_bounds(Ms, lo, hi, dt)
    nlit = np.asarray(head).shape[0]
    lo_, hi_ = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)
    plain = _split(plain_alpha(Ms, lo, hi, dt, nlit, pre), Ms, dt)
    uns = [_relax(l, u, dt)[3][:, None, :] for l, u in pre]
    if alpha0 is None:
        als = plain
    else:
        als = [np.where(m, np.clip(a0, dt(0), dt(1)), p) for m, a0, p in zip(uns, _split(alpha0, Ms, dt), plain)]
    live = np.ones((lo_.shape[0], nlit), dtype=bool)
    best, trace = None, []
    for s in range(steps + 1):
        smax, uA, ub, lam, eff = _backward(W, b, pre, head, lo_, hi_, dt, als)
        trace.append(smax.T)
        if best is None:
            best = dict(smax=smax.copy(), A=uA.copy(), b0=ub.copy(), alpha=[e.copy() for e in eff], step=np.zeros(smax.shape, dtype=np.int32))
        else:
            m = smax < best["smax"]
            best["smax"][m], best["A"][m], best["b0"][m], best["step"][m] = smax[m], uA[m], ub[m], s
            for e, src in zip(best["alpha"], eff):
                e[m] = src[m]
        if s == steps:
            break
        g = _grad(W, b, pre, lo_, hi_, dt, uA, lam, eff)
        gmax = np.max(np.abs(np.concatenate(g, axis=2)), axis=2)             # nbox x nlit
        live &= gmax > 0                                                     # a stationary literal stops
        scale = np.where(live, dt(eta0) * dt(decay) ** s / np.where(gmax > 0, gmax, dt(1)), dt(0))
        als = [np.clip(e - scale[:, :, None] * gj, dt(0), dt(1)) for e, gj in zip(eff, g)]
    return dict(smax=best["smax"].T, A=best["A"].transpose(1, 2, 0), b0=best["b0"].T, alpha=_join(best["alpha"]),
                best_step=best["step"].T, trace=np.stack(trace))


# ---- the cases of the issue
NETS = (([3, 17, 33, 4], 14), ([1, 64, 64, 2], 15), ([5, 20, 5], 16))
STEPS = (0, 1, 3, 8)


def cases():
    """(net, lo, hi, C) for every net x literal count, five boxes each (box 0 a point, box 1 1e-6 wide), and one nbox = 1 case"""
    if "cases" not in _cache:
        out = []
        for n, (xdims, seed) in enumerate(NETS):
            net = lc.random_net(xdims, seed)
            lo, hi = lc.boxes(xdims[0], 5, seed + 50)
            for nlit in (1, 7, 17) + ((64,) if max(xdims) == 64 else ()):
                out.append((net, lo, hi, lc.literal_rows(xdims[-1], nlit, seed + 100)))
            if n == 0:
                out.append((net, lo[:, 3:4].copy(), hi[:, 3:4].copy(), lc.literal_rows(xdims[-1], 7, seed + 100)))
        _cache["cases"] = out
    return _cache["cases"]


def table_case(hw):
    """net 3-17-33-4 (seed 14), the literal y_0 - y_3 on the cube of half-width hw around the origin"""
    net = lc.random_net([3, 17, 33, 4], 14)
    return net, -hw * np.ones((3, 1)), hw * np.ones((3, 1)), np.array([[1.0, 0.0, 0.0, -1.0]])


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - ref) / (1 + np.abs(ref)))) if ref.size else 0.0


def f32_uniform(shape, seed):
    """seeded uniform slopes in [0, 1) that float32 holds exactly (the host routine keeps alpha in float32)"""
    return np.random.default_rng(seed).random(shape).astype(np.float32).astype(np.float64)


# ---- the two C entries, called directly: every array as the library wrote it, in the shapes of the Python interface
KEYS = lc.NAMES + lc.LIT_NAMES
A_KEYS = ("a_smax", "a_A", "a_b0", "alpha", "best_step")


def _buffers(nbox, n0, acdim, ny, nlit):
    outs = [np.zeros((nbox, acdim)) for _ in range(4)] + [np.zeros((nbox, ny)) for _ in range(2)]
    louts = [np.zeros((nbox, nlit)), np.zeros((nbox, nlit)), np.zeros((nbox, nlit, n0)), np.zeros((nbox, nlit))]
    aouts = [np.zeros((nbox, nlit)), np.zeros((nbox, nlit, n0)), np.zeros((nbox, nlit)), np.zeros((nbox, nlit, acdim))]
    return outs, louts, aouts, np.full((nbox, nlit), -1, dtype=np.int32)


def _result(outs, louts, aouts, step):
    res = {k: o.T for k, o in zip(lc.NAMES, outs)}
    res.update(smin=louts[0].T, smax=louts[1].T, A=louts[2].transpose(1, 2, 0), b0=louts[3].T)
    res.update(a_smax=aouts[0].T, a_A=aouts[1].transpose(1, 2, 0), a_b0=aouts[2].T, alpha=aouts[3].transpose(1, 2, 0), best_step=step.T)
    return res


def raw_gpu(bd, lo, hi, steps, eta0=0.5, decay=0.9, alpha0=None, check=True):
    """nnsdp_crown_bound_alpha on the handle of the CrownBounder bd -> dict of the ten plain arrays and the five alpha outputs; with
    check=False -> (return code, message)"""
    lib, dp = _lib.load(), _lib.c_double_p
    nbox, nlit = lo.shape[1], bd._nlit or 0
    outs, louts, aouts, step = _buffers(nbox, bd._n0, bd._acdim, bd._ny, nlit)
    loc, hic = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)
    a0 = None if alpha0 is None else np.ascontiguousarray(np.asarray(alpha0, dtype=np.float64).transpose(2, 0, 1))
    ms = C.c_double(0.0)
    rc = lib.nnsdp_crown_bound_alpha(bd._handle(), nbox, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in outs + louts],
                                     C.byref(ms), int(steps), float(eta0), float(decay), None if a0 is None else a0.ctypes.data_as(dp),
                                     *[o.ctypes.data_as(dp) for o in aouts], step.ctypes.data_as(_lib.c_int32_p))
    if not check:
        return rc, lib.nnsdp_last_error().decode()
    _lib.check(rc)
    return _result(outs, louts, aouts, step)


def raw_host(net, lo, hi, Cm, steps, eta0=0.5, decay=0.9, alpha0=None, check=True):
    """nnsdp_make_intervals_lits_alpha box by box -> the same dict"""
    lib, dp = _lib.load(), _lib.c_double_p
    xd = np.asarray(net.xdims, dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    nrm = np.ascontiguousarray(Cm, dtype=np.float64)
    nbox, nlit, n0, acdim, ny = lo.shape[1], nrm.shape[0], int(xd[0]), int(xd[1:-1].sum()), int(xd[-1])
    outs, louts, aouts, step = _buffers(nbox, n0, acdim, ny, nlit)
    loc, hic = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)
    a0 = None if alpha0 is None else np.ascontiguousarray(np.asarray(alpha0, dtype=np.float64).transpose(2, 0, 1))
    for b in range(nbox):
        rows = [o[b].ctypes.data_as(dp) for o in outs]
        rc = lib.nnsdp_make_intervals_lits_alpha(net.K, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(dp), na.methods._activ_code(net.activ),
                                                 loc[b].ctypes.data_as(dp), hic[b].ctypes.data_as(dp), rows[0], rows[1], rows[2], rows[3], None, None,
                                                 rows[4], rows[5], nlit, nrm.ctypes.data_as(dp), *[o[b].ctypes.data_as(dp) for o in louts],
                                                 int(steps), float(eta0), float(decay), None if a0 is None else a0[b].ctypes.data_as(dp),
                                                 *[o[b].ctypes.data_as(dp) for o in aouts], step[b].ctypes.data_as(_lib.c_int32_p))
        if not check:
            return rc, lib.nnsdp_last_error().decode()
        _lib.check(rc)
    return _result(outs, louts, aouts, step)


# ---- the checks that the host routine (float32) and the kernel (fp64) share; run(steps, alpha0) -> the dict above, dt their arithmetic
def check_no_alpha(run, plain, net, lo, hi, dt):
    """steps = 0 without alpha0: the alpha outputs are the plain pass, bit for bit, alpha is the plain rule; for every T the ten
    existing arrays have the plain entry's bits"""
    r0 = run(0, None)
    assert np.array_equal(r0["a_smax"], r0["smax"]) and np.array_equal(r0["a_A"], r0["A"]) and np.array_equal(r0["a_b0"], r0["b0"])
    assert np.array_equal(r0["alpha"], plain_alpha(net.Ms, lo, hi, dt, r0["smax"].shape[0])) and not r0["best_step"].any()
    for T in STEPS:
        for k, want in zip(KEYS, plain):
            assert np.array_equal(run(T, None)[k], want), (T, k)


def check_never_looser(run):
    """a_smax <= smax exactly for every T, and T = 8 <= T = 3 <= T = 1 (the iterates are a prefix of one another)"""
    for T in STEPS:
        r = run(T, None)
        assert np.all(r["a_smax"] <= r["smax"]), T
        assert np.all((r["best_step"] >= 0) & (r["best_step"] <= T)), T
    assert np.all(run(8, None)["a_smax"] <= run(3, None)["a_smax"]) and np.all(run(3, None)["a_smax"] <= run(1, None)["a_smax"])


def pinned_errors(res, net, lo, hi, Cm, ref_dt):
    """largest |result - R_at(ref_dt, alpha = the returned alpha)| / (1 + |v|) over a_smax, a_A, a_b0, and the largest
    |a_smax - (a_A c + |a_A| r + a_b0)| / (1 + |v|) recomputed in longdouble"""
    ref = R_at(net.Ms, lo, hi, ref_dt, Cm, res["alpha"])
    err = max(rel_err(g, w) for g, w in zip((res["a_smax"], res["a_A"], res["a_b0"]), ref))
    ld = np.longdouble
    c, rad, A = (hi.astype(ld) + lo.astype(ld)) / ld(2), (hi.astype(ld) - lo.astype(ld)) / ld(2), res["a_A"].astype(ld)
    re = np.einsum("iqb,qb->ib", A, c) + np.einsum("iqb,qb->ib", np.abs(A), rad) + res["a_b0"].astype(ld)
    return err, rel_err(res["a_smax"], re)


def check_given_alpha(run, net, lo, hi, Cm, dt, seed):
    """steps = 0 at a seeded uniform alpha0: the returned alpha is alpha0 on the unstable neurons and the plain rule elsewhere, exactly"""
    nlit, acdim, nbox = Cm.shape[0], sum(net.xdims[1:-1]), lo.shape[1]
    a0 = f32_uniform((nlit, acdim, nbox), seed)
    res = run(0, a0)
    uns = unstable_mask(net.Ms, lo, hi, dt)[None, :, :]
    want = np.where(uns, a0, plain_alpha(net.Ms, lo, hi, dt, nlit))
    assert np.array_equal(res["alpha"], want) and not res["best_step"].any()
    return res
