"""Ground truth for the Tanh bounds (numpy + scipy + mpmath only; nothing of the product, of the oracle package or of the numpy
restatement crown_tanh_common is used).  tests/test_tanh_truth_cpu.py and tests/test_tanh_truth_gpu.py hold the relaxation lines, the
bounds, the reach enclosures and the split verdicts of Tanh networks against it; tests/golden/make_tanh_ranges.py records the
network-level part in tests/golden/tanh_ranges.json.

  line_gap      the exact worst violation of one relaxation line over an interval, in mpmath, from the endpoints and the stationary
                points of  w x + b - tanh(x)  (no sampling)
  attained_max  a value the network attains in the box: a rigorous LOWER bound w of the true maximum, whatever the optimiser did
  enclosed_max  a rigorous UPPER bound v of the true maximum: best-first interval branch and bound in long double, every operation
                widened outward by nextafter, mean-value form with an interval gradient and a monotonicity cut

Rigour of the interval arithmetic: numpy's long double (x87, 64-bit mantissa) rounds +, -, * to nearest, so the exact result lies
within one nextafter of the computed one; tanhl of the C library is not correctly rounded (the glibc manual lists 3 ulp on x86-64), its
results are widened by TANH_ULPS = 4 steps and clipped to [-1, 1].  float64 weights and boxes convert to long double exactly."""
import heapq
import time
from collections import namedtuple

import mpmath
import numpy as np
from scipy.optimize import minimize

LD = np.longdouble
DPS = 60
TANH_ULPS = 4
_INF, _NINF = LD(np.inf), LD(-np.inf)


# ----------------------------------------------------------------------------- one line against tanh
def line_gap(w, b, l, u, side):
    """the largest violation over [l, u] of  w x + b >= tanh(x)  (side "upper") or  w x + b <= tanh(x)  (side "lower"), as an mpmath
    number: positive where the line is violated somewhere, <= 0 where it holds on the whole interval (then minus the smallest distance).
    w, b, l, u are taken exactly as the doubles (or mpmath numbers) given.  g(x) = w x + b - tanh(x) has g' = w - 1 + tanh(x)^2, which
    vanishes only at x = +-atanh(sqrt(1 - w)), 0 < w <= 1: the extrema of g over [l, u] are at l, u and at those points inside."""
    assert side in ("upper", "lower")
    with mpmath.workdps(DPS):
        w, b, l, u = (mpmath.mpf(t) for t in (w, b, l, u))
        assert l <= u
        pts = [l, u]
        if 0 < w <= 1:
            s = mpmath.sqrt(1 - w)
            if s < 1:
                x0 = mpmath.atanh(s)
                pts += [x for x in (x0, -x0) if l <= x <= u]
        g = [w * x + b - mpmath.tanh(x) for x in pts]
        return +(-min(g) if side == "upper" else max(g))


def tangent(x0):
    """slope and intercept of the tangent of tanh at x0, as mpmath numbers at DPS digits"""
    with mpmath.workdps(DPS):
        x0 = mpmath.mpf(x0)
        t = mpmath.tanh(x0)
        k = 1 - t * t
        return +k, +(t - k * x0)


def tanh_mp(x):
    """tanh of a double -> the nearest doubles below and above the true value"""
    with mpmath.workdps(DPS):
        t = mpmath.tanh(mpmath.mpf(x))
        f = float(t)
        lo = f if mpmath.mpf(f) <= t else np.nextafter(f, -np.inf)
        hi = f if mpmath.mpf(f) >= t else np.nextafter(f, np.inf)
        return lo, hi


# ----------------------------------------------------------------------------- the network at one point
def _split(Ms):
    return [np.asarray(Mk, dtype=np.float64)[:, :-1] for Mk in Ms], [np.asarray(Mk, dtype=np.float64)[:, -1] for Mk in Ms]


def forward_ld(Ms, x, hidden=False):
    """long-double forward pass of the Tanh network Ms = [[W_0 b_0], ..] (linear last layer) at one point"""
    h, hid = np.asarray(x, dtype=LD), []
    for Mk in Ms[:-1]:
        Mk = np.asarray(Mk, dtype=LD)
        h = np.tanh(Mk[:, :-1] @ h + Mk[:, -1])
        hid.append(h)
    ML = np.asarray(Ms[-1], dtype=LD)
    y = ML[:, :-1] @ h + ML[:, -1]
    return (y, hid) if hidden else y


def value_mp(Ms, x, c):
    """c' f(x) in mpmath at DPS digits"""
    with mpmath.workdps(DPS):
        h = [mpmath.mpf(float(t)) for t in np.ravel(x)]
        for k, Mk in enumerate(Ms):
            Mk = np.asarray(Mk, dtype=np.float64)
            z = [mpmath.fsum([mpmath.mpf(float(Mk[i, j])) * h[j] for j in range(len(h))] + [mpmath.mpf(float(Mk[i, -1]))]) for i in range(Mk.shape[0])]
            h = [mpmath.tanh(t) for t in z] if k < len(Ms) - 1 else z
        return mpmath.fsum([mpmath.mpf(float(ci)) * hi for ci, hi in zip(np.ravel(c), h)])


def round_down(v):
    """an mpmath number -> the largest double <= it"""
    f = float(v)
    return f if mpmath.mpf(f) <= v else float(np.nextafter(f, -np.inf))


def attained_max(Ms, lo, hi, c, starts=8, seed=0):
    """multi-start L-BFGS-B on -c' f(x) over the box, from the corners (all of them up to 2^4, a seeded choice beyond), the centre and
    `starts` seeded interior points -> (x*, w): w = c' f(x*) in mpmath, rounded down to a double.  x* lies in the box, so w is attained."""
    W, b = _split(Ms)
    lo, hi = np.asarray(lo, dtype=np.float64).ravel(), np.asarray(hi, dtype=np.float64).ravel()
    c = np.asarray(c, dtype=np.float64).ravel()
    n0 = len(lo)

    def fun(x):
        h, acts = x, []
        for Wk, bk in zip(W[:-1], b[:-1]):
            h = np.tanh(Wk @ h + bk)
            acts.append(h)
        val = c @ (W[-1] @ h + b[-1])
        g = c @ W[-1]
        for Wk, a in zip(W[-2::-1], acts[::-1]):
            g = (g * (1.0 - a * a)) @ Wk
        return -val, -g

    rng = np.random.default_rng(seed)
    if n0 <= 4:
        corners = [np.array([(hi if (m >> i) & 1 else lo)[i] for i in range(n0)]) for m in range(1 << n0)]
    else:
        corners = [np.where(rng.random(n0) < 0.5, lo, hi) for _ in range(16)]
    pts = corners + [0.5 * (lo + hi)] + [lo + rng.random(n0) * (hi - lo) for _ in range(starts)]
    best, bx = -np.inf, pts[0]
    for p in pts:
        cand = [p]
        if np.any(hi > lo):
            res = minimize(fun, p, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)), options=dict(maxiter=500, ftol=1e-15, gtol=1e-12))
            cand.append(np.clip(res.x, lo, hi))
        for x in cand:
            f = -fun(x)[0]
            if f > best:
                best, bx = f, x.copy()
    return bx, round_down(value_mp(Ms, bx, c))


# ----------------------------------------------------------------------------- outward-rounded long-double intervals, many boxes at once
def _dn(x, n=1):
    for _ in range(n):
        x = np.nextafter(x, _NINF)
    return x


def _up(x, n=1):
    for _ in range(n):
        x = np.nextafter(x, _INF)
    return x


def _add(a, b):
    return _dn(a[0] + b[0]), _up(a[1] + b[1])


def _scale(k, a):
    """constant (array of exact long doubles) times interval"""
    p, q = k * a[0], k * a[1]
    return _dn(np.minimum(p, q)), _up(np.maximum(p, q))


def _mul(a, b):
    p = (a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1])
    return _dn(np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3]))), _up(np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3])))


def _affine(Wk, bk, a):
    """W a + b for a constant matrix: (nbox x n) interval -> (nbox x m), one widened operation at a time"""
    acc = (np.broadcast_to(bk, (a[0].shape[0], len(bk))).copy(), np.broadcast_to(bk, (a[0].shape[0], len(bk))).copy())
    for j in range(Wk.shape[1]):
        acc = _add(acc, _scale(Wk[None, :, j], (a[0][:, [j]], a[1][:, [j]])))
    return acc


def _tanh_iv(a):
    return np.maximum(_dn(np.tanh(a[0]), TANH_ULPS), LD(-1)), np.minimum(_up(np.tanh(a[1]), TANH_ULPS), LD(1))


def _dtanh_iv(t):
    """1 - t^2 for the interval t of tanh values"""
    lo2 = np.where((t[0] <= 0) & (t[1] >= 0), LD(0), np.minimum(t[0] * t[0], t[1] * t[1]))
    hi2 = np.maximum(t[0] * t[0], t[1] * t[1])
    return np.maximum(_dn(LD(1) - _up(hi2)), LD(0)), np.minimum(_up(LD(1) - np.maximum(_dn(lo2), LD(0))), LD(1))


class _Net:
    def __init__(self, Ms, c):
        W, b = _split(Ms)
        self.W, self.b = [Wk.astype(LD) for Wk in W], [bk.astype(LD) for bk in b]
        self.c = np.asarray(c, dtype=np.float64).ravel().astype(LD)

    def value(self, x, want_d=False):
        """interval of c' f over the boxes x = (lo, hi), nbox x n0 each (natural extension) [, the intervals of tanh' per hidden layer]"""
        h, ds = x, []
        for Wk, bk in zip(self.W[:-1], self.b[:-1]):
            h = _tanh_iv(_affine(Wk, bk, h))
            if want_d:
                ds.append(_dtanh_iv(h))
        y = _affine(self.W[-1], self.b[-1], h)
        out = _affine(self.c[None, :], np.zeros(1, dtype=LD), y)
        out = out[0][:, 0], out[1][:, 0]
        return (out, ds) if want_d else out

    def gradient(self, ds, nbox):
        """interval of the gradient of c' f over the boxes, nbox x n0, from the tanh' intervals of value()"""
        g = _affine(self.W[-1].T, np.zeros(self.W[-1].shape[1], dtype=LD), (np.broadcast_to(self.c, (nbox, len(self.c))).copy(),) * 2)
        for Wk, d in zip(self.W[-2::-1], ds[::-1]):
            g = _affine(Wk.T, np.zeros(Wk.shape[1], dtype=LD), _mul(g, d))
        return g

    def bound(self, lo, hi):
        """upper bounds of max c' f over the boxes (nbox x n0 long doubles) -> (ub, lo, hi): the smaller of the natural extension and the
        mean-value form  f(m) + G (x - m),  G the interval gradient over the box; where a component of G has one sign over the whole box
        the maximum over the box lies on that face, and the returned box is that face (its bound is not recomputed: it stays valid)"""
        nat, ds = self.value((lo, hi), want_d=True)
        G = self.gradient(ds, lo.shape[0])
        m = lo + (hi - lo) / LD(2)
        m = np.minimum(np.maximum(m, lo), hi)
        fm = self.value((m, m))
        dx = _dn(lo - m), _up(hi - m)
        prod = _mul(G, dx)
        mv = fm[1]
        for j in range(lo.shape[1]):
            mv = _up(mv + prod[1][:, j])
        lo2, hi2 = np.where(G[0] > 0, hi, lo), np.where(G[1] < 0, lo, hi)
        return np.minimum(nat[1], mv), lo2, hi2


Enclosed = namedtuple("Enclosed", "v gap boxes")


def enclosed_max(Ms, lo, hi, c, w, gap, batch=256, max_boxes=2_000_000, deadline=None):
    """a rigorous upper bound v of max c' f over the box, by best-first branch and bound: the `batch` boxes with the largest bounds are
    bisected along their widest edge at a time, every box whose bound is <= w (an attained value) is dropped, and v = max(w, the largest
    bound left).  Stops when v - w <= gap (1 + |v|), and otherwise at max_boxes evaluated boxes or past `deadline` (time.monotonic()) ->
    Enclosed(v as a double rounded up, the gap (v - w) / (1 + |v|) reached, boxes evaluated)"""
    net = _Net(Ms, c)
    lo, hi = np.asarray(lo, dtype=np.float64).ravel().astype(LD)[None], np.asarray(hi, dtype=np.float64).ravel().astype(LD)[None]
    wl = LD(w)
    heap, count, tick = [], 0, 0

    def push(lo, hi):
        nonlocal count, tick
        ub, lo2, hi2 = net.bound(lo, hi)
        count += len(ub)
        for _ in range(lo.shape[1] + 1):                           # a box cut down to a face is bounded again, as that face
            cut = np.nonzero((((lo2 != lo) | (hi2 != hi)).any(axis=1)) & (ub > wl))[0]
            if not len(cut):
                break
            lo, hi = lo2.copy(), hi2.copy()
            ub_c, lo2[cut], hi2[cut] = net.bound(lo[cut], hi[cut])
            ub[cut] = np.minimum(ub[cut], ub_c)
            count += len(cut)
        for i in np.nonzero(ub > wl)[0]:
            tick += 1
            heapq.heappush(heap, (-ub[i], tick, lo2[i], hi2[i]))

    def state():
        v = max(wl, -heap[0][0]) if heap else wl
        vf = float(v)
        vf = vf if LD(vf) >= v else float(np.nextafter(vf, np.inf))
        return vf, (vf - w) / (1.0 + abs(vf))

    push(lo, hi)
    while True:
        v, reached = state()
        if reached <= gap or not heap or count >= max_boxes or (deadline is not None and time.monotonic() > deadline):
            return Enclosed(v, max(reached, 0.0), count)
        top = [heapq.heappop(heap) for _ in range(min(batch, len(heap)))]
        blo, bhi = np.stack([t[2] for t in top]), np.stack([t[3] for t in top])
        wide = bhi - blo
        j = np.argmax(wide, axis=1)
        rows = np.arange(len(top))
        thin = wide[rows, j] <= 0                                  # a point: its bound cannot improve, it stays in the heap as it is
        for t in np.nonzero(thin)[0]:
            heapq.heappush(heap, top[t])
        if thin.all():                                             # the largest bounds left are those of points: v is final
            v, reached = state()
            return Enclosed(v, max(reached, 0.0), count)
        keep = ~thin
        blo, bhi, j, rows = blo[keep], bhi[keep], j[keep], np.arange(int(keep.sum()))
        mid = blo[rows, j] + (bhi[rows, j] - blo[rows, j]) / LD(2)
        left_hi, right_lo = bhi.copy(), blo.copy()
        left_hi[rows, j], right_lo[rows, j] = mid, mid
        push(np.concatenate([blo, right_lo]), np.concatenate([left_hi, bhi]))


def enclosed_range(Ms, lo, hi, c, **kw):
    """(w_min, v_min, w_max, v_max) of c' f over the box with gap 1e-9 by default: v_min <= true min <= w_min, w_max <= true max <= v_max"""
    kw.setdefault("gap", 1e-9)
    c = np.asarray(c, dtype=np.float64).ravel()
    _, wmax = attained_max(Ms, lo, hi, c)
    vmax = enclosed_max(Ms, lo, hi, c, wmax, **kw).v
    _, wneg = attained_max(Ms, lo, hi, -c)
    vneg = enclosed_max(Ms, lo, hi, -c, wneg, **kw).v
    return -wneg, -vneg, wmax, vmax
