"""Shared by the resident-bounder tests (test_crown_resident_*.py, test_split_resident_gpu.py): `R_tanh`, the numpy restatement of the
Tanh recurrences of csrc/intervals.hpp (tanh_relax, tanh_d_lower / tanh_d_upper, crown_backward with tanh_act) parametrised by
dtype, the Tanh copies of the nets of the ReLU tests, and the float32 figure of the host routine.  Nothing here needs a GPU."""
import numpy as np

import nnsdp_amd as na
import literal_common as lc

_cache = {}


def tanh_copy(net):
    return na.FeedFwdNet(xdims=list(net.xdims), Ms=net.Ms, activ=na.methods.TanhActiv)


class Exact:
    """tanh and cosh as numpy computes them"""
    tanh, cosh = staticmethod(np.tanh), staticmethod(np.cosh)


class Moved:
    """tanh and cosh with every result moved by `ulps` units in the last place, up or down by a seeded draw per element: what a
    library with that error bound may return"""

    def __init__(self, ulps, seed):
        self.ulps, self.rng = ulps, np.random.default_rng(seed)

    def _move(self, y):
        y = np.asarray(y)
        return y + y.dtype.type(self.ulps) * np.spacing(np.abs(y)) * self.rng.choice(np.array([-1, 1], dtype=y.dtype), size=y.shape)

    def tanh(self, x):
        return self._move(np.tanh(x))

    def cosh(self, x):
        return self._move(np.cosh(x))


def _dtanh(x, dt, lib=Exact):
    """dtanh_f: 1 / cosh(x)^2 where |x| < 25, else 0"""
    ok = np.abs(x) < dt(25)
    c = lib.cosh(np.where(ok, x, dt(0)))
    return np.where(ok, dt(1) / (c * c), dt(0))


def _d_lower(upper, dt, lib=Exact):
    """tanh_d_lower, elementwise: the 0.01 grid, the doubling search, then 100 halvings"""
    idx = np.maximum(0, np.trunc(upper / dt(0.01)).astype(np.int64)) + 1
    U = dt(0.01) * idx.astype(dt)
    fU = lib.tanh(U)
    ok = lambda d: _dtanh(d, dt, lib) * (U - d) + lib.tanh(d) <= fU
    l, r = np.full(upper.shape, dt(-1)), np.zeros(upper.shape, dtype=dt)
    go = np.ones(upper.shape, dtype=bool)
    for _ in range(64):
        go &= ~ok(l)
        if not go.any():
            break
        l = np.where(go, l * dt(2), l)
    for _ in range(100):
        m = (l + r) / dt(2)
        good = ok(m)
        l, r = np.where(good, m, l), np.where(good, r, m)
    return l


def _d_upper(lower, dt, lib=Exact):
    """tanh_d_upper, elementwise"""
    idx = np.maximum(0, np.trunc(lower / dt(-0.01)).astype(np.int64)) + 1
    Lw = dt(-0.01) * idx.astype(dt)
    fL = lib.tanh(Lw)
    ok = lambda d: _dtanh(d, dt, lib) * (Lw - d) + lib.tanh(d) >= fL
    l, r = np.zeros(lower.shape, dtype=dt), np.full(lower.shape, dt(1))
    go = np.ones(lower.shape, dtype=bool)
    for _ in range(64):
        go &= ~ok(r)
        if not go.any():
            break
        r = np.where(go, r * dt(2), r)
    for _ in range(100):
        m = (l + r) / dt(2)
        good = ok(m)
        l, r = np.where(good, l, m), np.where(good, m, r)
    return r


def relax(l, u, dt, lib=Exact):
    """tanh_relax line by line on arrays: -> lw, lb, uw, ub with  lw x + lb <= tanh(x) <= uw x + ub  on [l, u], and the regime of
    every neuron (0: u <= 0, 1: l >= 0, 2: crossing)"""
    zero, one = dt(0), dt(1)
    lower, upper = np.maximum(l, dt(-500)), np.minimum(u, dt(500))
    yl, yu = lib.tanh(lower), lib.tanh(upper)
    wd = upper - lower
    kd = np.where(wd < dt(1e-6), _dtanh(upper, dt, lib), (yu - yl) / np.maximum(wd, dt(1e-6)))
    pos = l >= zero
    neg = (u <= zero) & ~pos                    # l = u = 0 takes the l >= 0 regime alone
    m = (lower + upper) / dt(2)
    ym, km = lib.tanh(m), _dtanh(m, dt, lib)
    fpos, fneg = pos.astype(dt), neg.astype(dt)
    fboth = one - fpos - fneg
    line = lambda k, x0, y0: (k, -x0 * k + y0)
    cw, cb = line(kd, lower, yl)          # the chord (or the tangent at `upper` of a thin interval)
    mw, mb = line(km, m, ym)              # the tangent at the midpoint
    lw = fneg * mw + fpos * cw
    lb = fneg * mb + fpos * cb
    uw = fneg * cw + fpos * mw
    ub = fneg * cb + fpos * mb
    both = fboth != zero
    if both.any():
        lo_b, up_b, kd_b, cw_b, cb_b = lower[both], upper[both], kd[both], cw[both], cb[both]
        dl, du = _d_lower(up_b, dt, lib), _d_upper(lo_b, dt, lib)
        tw, tb = line(_dtanh(dl, dt, lib), dl, lib.tanh(dl))
        use = kd_b < _dtanh(lo_b, dt, lib)
        lw[both] += fboth[both] * np.where(use, cw_b, tw)
        lb[both] += fboth[both] * np.where(use, cb_b, tb)
        tw, tb = line(_dtanh(du, dt, lib), du, lib.tanh(du))
        use = kd_b < _dtanh(up_b, dt, lib)
        uw[both] += fboth[both] * np.where(use, cw_b, tw)
        ub[both] += fboth[both] * np.where(use, cb_b, tb)
    over, under = u > dt(500), l < dt(-500)      # an end beyond the clamp: the line the clamped fit would carry past it is a constant
    lw, lb = np.where(over, zero, lw), np.where(over, yl, lb)
    uw, ub = np.where(under, zero, uw), np.where(under, yu, ub)
    return lw, lb, uw, ub, np.where(neg, 0, np.where(pos, 1, 2))


def R_tanh(Ms, lo, hi, dt, C=None, regimes=None, lib=Exact):
    """the Tanh recurrences in dtype dt, all boxes at once: lo / hi are n0 x nbox -> the six arrays, one column per box.  With C (the
    nlit x ny matrix of literal normals) the four literal outputs smin, smax (nlit x nbox, raw), A (nlit x n0 x nbox), b0 (nlit x nbox)
    follow, as in literal_common.R.  regimes (a list): receives the regime array of every hidden layer.  lib: where tanh and cosh come
    from (Exact, or a Moved)."""
    K = len(Ms)
    W = [np.asarray(Mk[:, :-1], dtype=dt) for Mk in Ms]
    b = [np.asarray(Mk[:, -1], dtype=dt) for Mk in Ms]
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)            # nbox x n0
    nbox, zero = lo.shape[0], dt(0)
    rel = []                                                                   # per hidden layer: lw, lb, uw, ub (nbox x d), computed once

    def backward(Ws, bs, full=False):
        lA = np.broadcast_to(Ws[-1], (nbox,) + Ws[-1].shape).copy()
        uA = lA.copy()
        lb = np.broadcast_to(bs[-1], (nbox, len(bs[-1]))).copy()
        ub = lb.copy()
        for j in range(len(Ws) - 2, -1, -1):
            dl, bl, du, bu = rel[j]
            lAp, lAn, uAp, uAn = np.maximum(lA, zero), np.minimum(lA, zero), np.maximum(uA, zero), np.minimum(uA, zero)
            lb = lb + (lAn * bu[:, None, :] + lAp * bl[:, None, :]).sum(axis=2)
            ub = ub + (uAp * bu[:, None, :] + uAn * bl[:, None, :]).sum(axis=2)
            lA = lAp * dl[:, None, :] + lAn * du[:, None, :]
            uA = uAp * du[:, None, :] + uAn * dl[:, None, :]
            lb = lb + lA @ bs[j]
            ub = ub + uA @ bs[j]
            lA, uA = lA @ Ws[j], uA @ Ws[j]
        c, r = (hi + lo) / dt(2), (hi - lo) / dt(2)
        out = (np.einsum("biq,bq->bi", lA, c) - np.einsum("biq,bq->bi", np.abs(lA), r) + lb,
               np.einsum("biq,bq->bi", uA, c) + np.einsum("biq,bq->bi", np.abs(uA), r) + ub)
        return out + (uA, ub) if full else out

    def fix(l, u):
        l = np.minimum(l, u)
        return l, np.maximum(l, u)

    xlo, xhi = [lo], [hi]
    for k in range(1, K + 1):
        l, u = backward(W[:k], b[:k])
        if k < K:
            *r4, regime = relax(l, u, dt, lib)
            rel.append(tuple(r4))
            if regimes is not None:
                regimes.append(regime)
            n = W[k - 1].shape[0]
            l, u = backward(W[:k] + [np.eye(n, dtype=dt)], b[:k] + [np.zeros(n, dtype=dt)])
        l, u = fix(l, u)
        xlo.append(l)
        xhi.append(u)
    plo, phi = [], []
    for k in range(K - 1):
        Wp, Wn = np.maximum(W[k], zero), np.minimum(W[k], zero)
        plo.append(xlo[k] @ Wp.T + xhi[k] @ Wn.T + b[k])
        phi.append(xhi[k] @ Wp.T + xlo[k] @ Wn.T + b[k])
    cat = lambda parts: np.concatenate(parts, axis=1).T
    six = cat(xlo[1:K]), cat(xhi[1:K]), cat(plo), cat(phi), xlo[K].T, xhi[K].T
    if C is None:
        return six
    Cm = np.asarray(C, dtype=dt)
    sl, su, uA, ub = backward(W[:K - 1] + [Cm @ W[K - 1]], b[:K - 1] + [Cm @ b[K - 1]], full=True)
    return six + (sl.T, su.T, uA.transpose(1, 2, 0), ub.T)


def flat(res):
    """the six arrays, then the four of a LiteralBounds if the result ends in one"""
    res = tuple(res)
    return res[:6] + tuple(res[6]) if len(res) == 7 else res


# the two nets of sound_cases / literal_common.sound_nets as Tanh nets, their 64 boxes and 7 literal rows.  The box seeds are chosen on
# the CPU so that the float32 host routine meets the float32 condition (its grid index  (long)(u / 0.01f)  differs from the float64 one
# for a bound within float32 rounding of a multiple of 0.01, and such a box moves the host's bound by a whole grid step): the seeds of
# sound_cases, 31 and 33, do - the figure is 2.5e-5, on the coefficients A of boxes 1e-6 wide, and 5.0e-7 on the bounds.
SOUND_SEEDS = (31, 33)


def sound_tanh():
    """per net: net, lo, hi, C, the host routine's ten arrays and R_tanh(float64)'s"""
    if "sound" not in _cache:
        out = []
        for net, seed in zip((tanh_copy(lc.fixture_net()), tanh_copy(lc.random_net([5, 50, 50, 50, 5], 32))), SOUND_SEEDS):
            rng = np.random.default_rng(seed)
            n0 = net.xdims[0]
            c = 1.0 + 0.5 * rng.uniform(-1, 1, size=(n0, 64))
            hw = np.array([1e-6, 0.05, 0.25, 0.5])[rng.integers(0, 4, size=(n0, 64))]
            hw[:, 0] = 0.0
            lo, hi, C = c - hw, c + hw, lc.literal_rows(net.xdims[-1], 7, seed + 100)
            host = flat(na.makeIntervalsBatch(net, lo, hi, backend="host", normals=C))
            out.append(dict(net=net, lo=lo, hi=hi, C=C, host=host, r64=R_tanh(net.Ms, lo, hi, np.float64, C)))
        _cache["sound"] = out
    return _cache["sound"]


def rel_err(a, ref):
    return float((np.abs(a - ref) / (1.0 + np.abs(ref))).max()) if a.size else 0.0


def host_figure():
    """max |R_tanh(float64) - host| / (1 + |v|) over the ten arrays of both nets"""
    return max(rel_err(h, r) for cs in sound_tanh() for h, r in zip(cs["host"], cs["r64"]))


def assert_hidden_and_output_sound(net, lo, hi, acymin, acymax, ymin, ymax, npts=2000, seed=5):
    """npts points per box: every hidden post-activation lies in [acymin, acymax] and the output in [ymin, ymax], slack 1e-9 (1 + |v|)"""
    rng = np.random.default_rng(seed)
    for bx in range(lo.shape[1]):
        x = lo[:, [bx]] + rng.random((net.xdims[0], npts)) * (hi[:, [bx]] - lo[:, [bx]])
        hid = []
        for Mk in net.Ms[:-1]:
            x = np.tanh(Mk[:, :-1] @ x + Mk[:, -1:])
            hid.append(x)
        y = net.Ms[-1][:, :-1] @ x + net.Ms[-1][:, -1:]
        for v, l, u in ((np.concatenate(hid), acymin[:, [bx]], acymax[:, [bx]]), (y, ymin[:, [bx]], ymax[:, [bx]])):
            slack = 1e-9 * (1.0 + np.abs(v))
            assert np.all(v >= l - slack) and np.all(v <= u + slack), bx
