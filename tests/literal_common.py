"""Shared by the literal-bound tests (test_literal_bounds_*.py, test_split_literals_*.py): the numpy restatement `R` of the recurrences
of csrc/intervals.hpp with a literal head, the net / box recipes of tests/test_crown_batch_gpu.py restated, and the two split
instances.  Nothing here needs a GPU."""
import numpy as np

import helpers
import nnsdp_amd as na

NAMES = ("acymin", "acymax", "acxmin", "acxmax", "ymin", "ymax")
LIT_NAMES = ("smin", "smax", "A", "b0")
HALF_WIDTHS = np.array([0.0, 1e-6, 0.05, 0.5, 3.0])
_cache = {}


def R(Ms, lo, hi, dt, head=None):
    """the recurrences in dtype dt, all boxes at once: lo / hi are n0 x nbox -> the six arrays, one column per box.  With head (the
    nlit x ny matrix C of literal normals): one more backward pass from [C W_{K-1} | C b_{K-1}] over layers K-2 .. 0, and the four
    literal outputs smin, smax (nlit x nbox, raw), A (nlit x n0 x nbox) and b0 (nlit x nbox) of the upper bound A' x + b0 follow."""
    K = len(Ms)
    W = [np.asarray(Mk[:, :-1], dtype=dt) for Mk in Ms]
    b = [np.asarray(Mk[:, -1], dtype=dt) for Mk in Ms]
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)            # nbox x n0
    nbox, zero = lo.shape[0], dt(0)

    def backward(Ws, bs, pre, full=False):
        lA = np.broadcast_to(Ws[-1], (nbox,) + Ws[-1].shape).copy()
        uA = lA.copy()
        lb = np.broadcast_to(bs[-1], (nbox, len(bs[-1]))).copy()
        ub = lb.copy()
        for j in range(len(Ws) - 2, -1, -1):
            l, u = pre[j]                                                    # nbox x d
            lr = np.minimum(l, zero)
            ur = np.maximum(np.maximum(u, zero), lr + dt(1e-8))
            du = ur / (ur - lr)
            dl = (du > dt(0.5)).astype(dt)
            bu = -lr * du
            lAp, lAn, uAp, uAn = np.maximum(lA, zero), np.minimum(lA, zero), np.maximum(uA, zero), np.minimum(uA, zero)
            lb = lb + np.einsum("bit,bt->bi", lAn, bu)
            ub = ub + np.einsum("bit,bt->bi", uAp, bu)
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

    pre, xlo, xhi = [], [lo], [hi]
    for k in range(1, K + 1):
        l, u = backward(W[:k], b[:k], pre)
        if k < K:
            pre.append((l, u))
            n = W[k - 1].shape[0]
            l, u = backward(W[:k] + [np.eye(n, dtype=dt)], b[:k] + [np.zeros(n, dtype=dt)], pre)
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
    if head is None:
        return six
    Cm = np.asarray(head, dtype=dt)
    sl, su, uA, ub = backward(W[:K - 1] + [Cm @ W[K - 1]], b[:K - 1] + [Cm @ b[K - 1]], pre, full=True)
    return six + (sl.T, su.T, uA.transpose(1, 2, 0), ub.T)


def fixture_net():
    d = helpers.load_problem("W10-D5", 0)
    return na.FeedFwdNet(xdims=[int(v) for v in d["xdims"]], Ms=helpers.problem_Ms(d))


def random_net(xdims, seed):
    rng = np.random.default_rng(seed)
    Ms = [rng.normal(0.0, 1.0 / np.sqrt(xdims[k] + 1), size=(xdims[k + 1], xdims[k] + 1)) for k in range(len(xdims) - 1)]   # N(0, 1/(in+1))
    return na.FeedFwdNet(xdims=list(xdims), Ms=Ms)


def boxes(n0, nbox, seed):
    """centre +- half-widths from HALF_WIDTHS: the first five boxes use one half-width for every coordinate (box 0 is a point),
    the others draw one per coordinate"""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n0, nbox))
    hw = HALF_WIDTHS[rng.integers(0, len(HALF_WIDTHS), size=(n0, nbox))]
    for j in range(min(nbox, len(HALF_WIDTHS))):
        hw[:, j] = HALF_WIDTHS[j]
    return c - hw, c + hw


def literal_rows(ny, nlit, seed):
    """e_0 - e_{ny-1}, e_0, -e_0, the zero row, then seeded Gaussian rows: the first nlit of them"""
    C = np.random.default_rng(seed).normal(size=(max(nlit, 64), ny))       # row i does not depend on nlit
    C[:4] = 0.0
    C[0, 0] += 1.0
    C[0, ny - 1] -= 1.0          # ny = 1: e_0 - e_0, a second zero row
    C[1, 0] = 1.0
    C[2, 0] = -1.0
    return C[:nlit].copy()


def sound_nets():
    """the two nets and 64 boxes each of sound_cases in tests/test_crown_batch_gpu.py"""
    if "sound" not in _cache:
        out = []
        for net, seed in ((fixture_net(), 31), (random_net([5, 50, 50, 50, 5], 32), 33)):
            rng = np.random.default_rng(seed)
            n0 = net.xdims[0]
            c = 1.0 + 0.5 * rng.uniform(-1, 1, size=(n0, 64))
            hw = np.array([1e-6, 0.05, 0.25, 0.5])[rng.integers(0, 4, size=(n0, 64))]
            hw[:, 0] = 0.0
            out.append(dict(net=net, lo=c - hw, hi=c + hw, C=literal_rows(net.xdims[-1], 7, seed + 100)))
        _cache["sound"] = out
    return _cache["sound"]


def forward(net, X):
    """numpy forward pass of a ReLU / Tanh net at the columns of X"""
    act = np.tanh if na.methods._activ_code(net.activ) == na.methods.ACTIV_TANH else (lambda v: np.maximum(v, 0.0))
    for Mk in net.Ms[:-1]:
        X = act(Mk[:, :-1] @ X + Mk[:, -1:])
    return net.Ms[-1][:, :-1] @ X + net.Ms[-1][:, -1:]


def assert_literals_sound(net, lo, hi, C, lits, slack_rel, npts=2000, seed=5):
    """npts points per box: smin - slack <= C f(x) <= smax + slack and C f(x) <= A' x + b0 + slack, slack = slack_rel (1 + |v|)"""
    rng = np.random.default_rng(seed)
    for b in range(lo.shape[1]):
        X = lo[:, [b]] + rng.random((net.xdims[0], npts)) * (hi[:, [b]] - lo[:, [b]])
        v = C @ forward(net, X)                                                  # nlit x npts
        slack = slack_rel * (1.0 + np.abs(v))
        assert np.all(v >= lits.smin[:, [b]] - slack) and np.all(v <= lits.smax[:, [b]] + slack), b
        assert np.all(v <= lits.A[:, :, b] @ X + lits.b0[:, [b]] + slack), b


def assert_tiles(leaves, lo, hi):
    """the leaves are dyadic sub-boxes of [lo, hi] whose volumes add up to the root's"""
    vol = sum(float(np.prod(lf.hi - lf.lo)) for lf in leaves)
    assert abs(vol - float(np.prod(hi - lo))) <= 1e-12 * float(np.prod(hi - lo))
    for lf in leaves:
        w = (lf.hi - lf.lo) / (hi - lo)
        k = np.round(-np.log2(w))
        assert np.allclose(w, 2.0 ** -k, rtol=1e-12, atol=0) and int(k.sum()) == lf.depth
        pos = (lf.lo - lo) / (hi - lo) * 2.0 ** k
        assert np.allclose(pos, np.round(pos), rtol=0, atol=1e-9)


def instance(which, backend="host"):
    """the two split instances: net, box, normal, s = max of the literal over lo + default_rng(0).random((n0, 20000)) * (hi - lo), c0 =
    the root box's cheap bound (from the given backend), and the threshold h"""
    key = (which, backend)
    if key not in _cache:
        if which == "holds":
            net, nrm = random_net([3, 17, 33, 4], 14), np.array([1.0, 0.0, 0.0, -1.0])
        else:
            net, nrm = random_net([5, 20, 20, 20, 5], 31), np.array([1.0, 0.0, 0.0, 0.0, -1.0])
        n0 = net.xdims[0]
        lo, hi = -np.ones(n0), np.ones(n0)
        X = lo[:, None] + np.random.default_rng(0).random((n0, 20000)) * (hi - lo)[:, None]
        s = float((nrm @ forward(net, X)).max())
        iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend=backend)
        c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
        assert c0 > s
        h = s + 0.05 * (c0 - s) if which == "holds" else s - 0.1 * abs(s)
        _cache[key] = dict(net=net, lo=lo, hi=hi, normal=nrm, s=s, c0=c0, h=h)
    return _cache[key]
