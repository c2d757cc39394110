"""Batched CROWN-sliced bounds on the GPU (nnsdp_make_intervals_batch, csrc/crown_batch.hpp; frontend.makeIntervalsBatch) against a
numpy restatement `R` of the recurrences of csrc/intervals.hpp (make_intervals / crown_backward), parametrised by dtype:
R(longdouble) is the oracle, |R(float64) - R(longdouble)| the yardstick of the tolerance, R(float64) against the float32 host routine
the yardstick of the agreement with nnsdp_make_intervals."""
import ctypes as C

import numpy as np
import pytest

import helpers
import nnsdp_amd as na
from nnsdp_amd import _lib

NAMES = ("acymin", "acymax", "acxmin", "acxmax", "ymin", "ymax")
HALF_WIDTHS = np.array([0.0, 1e-6, 0.05, 0.5, 3.0])
NBOX = 257
_cache = {}


def R(Ms, lo, hi, dt):
    """the recurrences in dtype dt, all boxes at once: lo / hi are n0 x nbox -> the six arrays, one column per box"""
    K = len(Ms)
    W = [np.asarray(Mk[:, :-1], dtype=dt) for Mk in Ms]
    b = [np.asarray(Mk[:, -1], dtype=dt) for Mk in Ms]
    lo, hi = np.asarray(lo.T, dtype=dt), np.asarray(hi.T, dtype=dt)            # nbox x n0
    nbox, zero = lo.shape[0], dt(0)

    def backward(Ws, bs, pre):
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
        return (np.einsum("biq,bq->bi", lA, c) - np.einsum("biq,bq->bi", np.abs(lA), r) + lb,
                np.einsum("biq,bq->bi", uA, c) + np.einsum("biq,bq->bi", np.abs(uA), r) + ub)

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
    return cat(xlo[1:K]), cat(xhi[1:K]), cat(plo), cat(phi), xlo[K].T, xhi[K].T


def fixture_net():
    d = helpers.load_problem("W10-D5", 0)
    return na.FeedFwdNet(xdims=[int(v) for v in d["xdims"]], Ms=helpers.problem_Ms(d))


def random_net(xdims, seed, dead_first_layer=False):
    rng = np.random.default_rng(seed)
    Ms = [rng.normal(0.0, 1.0 / np.sqrt(xdims[k] + 1), size=(xdims[k + 1], xdims[k] + 1)) for k in range(len(xdims) - 1)]   # N(0, 1/(in+1))
    if dead_first_layer:
        Ms[0][:, -1] = -10.0
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


CASES = {
    "1-1-1": lambda: random_net([1, 1, 1], 11),
    "2-15-2": lambda: random_net([2, 15, 2], 12),
    "2-16-16-2": lambda: random_net([2, 16, 16, 2], 13),
    "3-17-33-4": lambda: random_net([3, 17, 33, 4], 14),
    "5-63-64-5": lambda: random_net([5, 63, 64, 5], 15),
    "64-64-64-64": lambda: random_net([64, 64, 64, 64], 16),
    "2-10x5-2": lambda: random_net([2, 10, 10, 10, 10, 10, 2], 17),
    "W10-D5": fixture_net,
    "3-17-33-4-dead": lambda: random_net([3, 17, 33, 4], 18, dead_first_layer=True),
}


def case(name):
    """net, boxes, R(float64), R(longdouble) and the 257-box GPU result of a case: computed once, shared, never modified"""
    if name not in _cache:
        net = CASES[name]()
        lo, hi = boxes(net.xdims[0], NBOX, seed=sum(map(ord, name)))
        r64 = R(net.Ms, lo, hi, np.float64)
        rld = R(net.Ms, lo, hi, np.longdouble)
        *gpu, ms = na.makeIntervalsBatch(net, lo, hi, backend="gpu", return_ms=True)
        _cache[name] = dict(net=net, lo=lo, hi=hi, r64=r64, rld=rld, gpu=gpu, ms=ms)
    return _cache[name]


@pytest.mark.gpu
@pytest.mark.parametrize("nbox", [1, 2, 257])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_numpy_recurrences(name, nbox):
    """|GPU - R(longdouble)| <= max(8 r, 64 * 2^-52 * s) for every output array, r = max |R(float64) - R(longdouble)| and s = max |bound|
    of that array over the boxes of the call.  The test prints err / max(r, 8 * 2^-52 s) per array (8 is the limit)."""
    cs = case(name)
    got = cs["gpu"] if nbox == NBOX else na.makeIntervalsBatch(cs["net"], cs["lo"][:, :nbox], cs["hi"][:, :nbox], backend="gpu")
    worst = 0.0
    for nm, g, a64, ald in zip(NAMES, got, cs["r64"], cs["rld"]):
        assert g.shape == (a64.shape[0], nbox), nm
        a64, ald = a64[:, :nbox], ald[:, :nbox]
        r = float(np.abs(a64 - ald).max()) if a64.size else 0.0
        s = float(np.abs(ald).max()) if ald.size else 0.0
        err = float(np.abs(g - ald).max()) if g.size else 0.0
        tol = max(8.0 * r, 64.0 * 2.0 ** -52 * s)
        ratio = err / max(r, 8.0 * 2.0 ** -52 * s) if max(r, s) > 0 else 0.0
        worst = max(worst, ratio)
        print(f"{name} nbox={nbox} {nm}: err {err:.3e}  r {r:.3e}  s {s:.3e}  tol {tol:.3e}  err / max(r, floor / 8) = {ratio:.3f}")
        assert np.all(np.isfinite(g)), nm
        assert err <= tol, (name, nbox, nm, err, tol)
    print(f"{name} nbox={nbox}: largest ratio {worst:.3f} (8 allowed)")



def sound_cases():
    if "sound" not in _cache:
        out = []
        for net, seed in ((fixture_net(), 31), (random_net([5, 50, 50, 50, 5], 32), 33)):
            rng = np.random.default_rng(seed)
            n0 = net.xdims[0]
            c = 1.0 + 0.5 * rng.uniform(-1, 1, size=(n0, 64))
            hw = np.array([1e-6, 0.05, 0.25, 0.5])[rng.integers(0, 4, size=(n0, 64))]
            hw[:, 0] = 0.0
            lo, hi = c - hw, c + hw
            out.append(dict(net=net, lo=lo, hi=hi, gpu=na.makeIntervalsBatch(net, lo, hi, backend="gpu"),
                            host=na.makeIntervalsBatch(net, lo, hi, backend="host"), r64=R(net.Ms, lo, hi, np.float64)))
        _cache["sound"] = out
    return _cache["sound"]


@pytest.mark.gpu
def test_bounds_are_sound_on_sampled_points():
    """2000 points per box: every hidden post-activation lies in [acymin, acymax] and the output in [ymin, ymax] (numpy forward pass)"""
    for cs in sound_cases():
        net, (acymin, acymax, _, _, ymin, ymax) = cs["net"], cs["gpu"]
        rng = np.random.default_rng(5)
        for b in range(cs["lo"].shape[1]):
            x = cs["lo"][:, [b]] + rng.random((net.xdims[0], 2000)) * (cs["hi"][:, [b]] - cs["lo"][:, [b]])
            hid = []
            for Mk in net.Ms[:-1]:
                x = np.maximum(Mk[:, :-1] @ x + Mk[:, -1:], 0.0)
                hid.append(x)
            y = net.Ms[-1][:, :-1] @ x + net.Ms[-1][:, -1:]
            for v, l, u in ((np.concatenate(hid), acymin[:, [b]], acymax[:, [b]]), (y, ymin[:, [b]], ymax[:, [b]])):
                slack = 1e-9 * (1.0 + np.abs(v))
                assert np.all(v >= l - slack) and np.all(v <= u + slack), b


@pytest.mark.gpu
def test_agrees_with_the_float32_host_routine():
    """nnsdp_make_intervals computes in float32 by design: the figure max |R(float64) - host| / (1 + |v|) is measured here on the CPU
    (HOST_FLOAT32_FIGURE is what it was when this test was written); the GPU stays within twice that figure of the
    host routine."""
    rel = lambda a, ref: float((np.abs(a - ref) / (1.0 + np.abs(ref))).max())
    figure = max(rel(h, r) for cs in sound_cases() for h, r in zip(cs["host"], cs["r64"]))
    gpu = max(rel(g, h) for cs in sound_cases() for g, h in zip(cs["gpu"], cs["host"]))
    print(f"max |R(float64) - host| / (1 + |v|) = {figure:.3e} (recorded {HOST_FLOAT32_FIGURE:.3e});  max |GPU - host| / (1 + |v|) = {gpu:.3e}")
    assert 0.0 < figure < 1e-4, "the host routine is float32: the figure is of float32 size"
    assert gpu <= 2.0 * figure


HOST_FLOAT32_FIGURE = 3.14e-7


@pytest.mark.gpu
def test_a_box_has_the_same_bits_wherever_it_stands():
    for name in ("3-17-33-4", "64-64-64-64", "W10-D5"):
        cs = case(name)
        for j in (0, 1, 130, 256):
            one = na.makeIntervalsBatch(cs["net"], cs["lo"][:, [j]], cs["hi"][:, [j]], backend="gpu")
            for nm, a, g in zip(NAMES, one, cs["gpu"]):
                assert np.array_equal(a[:, 0], g[:, j]), (name, j, nm)


@pytest.mark.gpu
def test_kernel_time_is_reported():
    assert case("W10-D5")["ms"] > 0.0


def _raw(xdims, M, activ, nbox, lo, hi):
    lib = _lib.load()
    xd = np.asarray(xdims, dtype=np.int32)
    dp = _lib.c_double_p
    p = lambda a: None if a is None else a.ctypes.data_as(dp)
    rc = lib.nnsdp_make_intervals_batch(len(xdims) - 1, xd.ctypes.data_as(_lib.c_int32_p), p(M), activ, nbox, p(lo), p(hi),
                                        None, None, None, None, None, None, None)
    return rc, lib.nnsdp_last_error().decode()


def _refusals():
    M3 = np.zeros(3 * 3 + 2 * 4)                      # a 2-3-2 network: [W0 b0] 3 x 3, [W1 b1] 2 x 4
    lo, hi = np.zeros((4, 2)), np.ones((4, 2))        # 4 boxes: n0 x nbox column-major is one row of this array per box
    rc, msg = _raw([2, 3, 2], M3, 1, 4, lo, hi)
    assert rc < 0 and "Tanh" in msg
    M65 = np.zeros(65 * 3 + 2 * 66)
    rc, msg = _raw([2, 65, 2], M65, 0, 4, lo, hi)
    assert rc < 0 and "65" in msg and "64" in msg
    bad = hi.copy()
    bad[2, 1] = -1.0
    rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, bad)
    assert rc < 0 and "box 2" in msg and "x1min" in msg
    nan = hi.copy()
    nan[3, 0] = np.nan
    rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, nan)
    assert rc < 0 and "box 3" in msg and "NaN" in msg
    inf = hi.copy()
    inf[1, 1] = np.inf
    rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, inf)
    assert rc < 0 and "box 1" in msg and "finite" in msg
    rc, msg = _raw([2, 3, 2], None, 0, 4, lo, hi)
    assert rc < 0 and "network" in msg
    rc, msg = _raw([2, 3, 2], M3, 0, -1, lo, hi)
    assert rc < 0 and "nbox" in msg
    assert _raw([2, 3, 2], M3, 0, 0, None, None)[0] == 0          # nbox = 0: nothing to do


def test_batch_intervals_entry_rejects_bad_arguments_without_a_gpu():
    _refusals()


@pytest.mark.gpu
def test_refusals_name_the_fact():
    _refusals()
    net = random_net([2, 3, 2], 1)
    lo, hi = np.zeros((2, 3)), np.ones((2, 3))
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    with pytest.raises(_lib.NnsdpError, match="Tanh"):
        na.makeIntervalsBatch(tanh, lo, hi, backend="gpu")
    with pytest.raises(_lib.NnsdpError, match="65"):
        na.makeIntervalsBatch(random_net([2, 65, 2], 1), lo, hi, backend="gpu")
    hi[1, 2] = -1.0
    with pytest.raises(_lib.NnsdpError, match="box 2"):
        na.makeIntervalsBatch(net, lo, hi, backend="gpu")
    assert all(a.shape[1] == 0 for a in na.makeIntervalsBatch(net, lo[:, :0], hi[:, :0], backend="gpu"))
