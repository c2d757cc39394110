"""Optimised ReLU slopes (alpha-CROWN) without a GPU: the numpy yardstick of tests/crown_alpha_common.py pinned on its own, the float32
host routine nnsdp_make_intervals_lits_alpha against it, and the split driver with alpha_steps on the host backend."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import crown_alpha_common as ca
import literal_common as lc

# max |host - R_at(float64, alpha = the host's alpha)| / (1 + |v|) over a_smax, a_A, a_b0, every case and T below, measured on the CPU:
# 3.7e-7 (the plain host literal pass gave 4.1e-7 on its own boxes); the assertion allows twice the figure
HOST_FIGURE = 3.7e-7
_cache = {}


# ----------------------------------------------------------------------------- the yardstick, no product code
def test_the_gradient_is_the_derivative_of_R_at():
    """grad against central finite differences of R_at at alpha = 0.5 on 3-17-33-4, the cube of half-width 1: 1e-7 absolute"""
    net, lo, hi, Cm = ca.table_case(1.0)
    acdim = sum(net.xdims[1:-1])
    a = np.full((1, acdim, 1), 0.5)
    g = ca.grad(net.Ms, lo, hi, np.float64, Cm, a)
    uns = ca.unstable_mask(net.Ms, lo, hi, np.float64)[:, 0]
    assert uns.sum() > 10 and not g[0, ~uns, 0].any()
    fd, e = np.zeros(acdim), 1e-6
    for k in range(acdim):
        ap, am = a.copy(), a.copy()
        ap[0, k, 0] += e
        am[0, k, 0] -= e
        fd[k] = (ca.R_at(net.Ms, lo, hi, np.float64, Cm, ap)[0][0, 0] - ca.R_at(net.Ms, lo, hi, np.float64, Cm, am)[0][0, 0]) / (2 * e)
    err = float(np.abs(fd - g[0, :, 0]).max())
    print(f"max |grad - finite differences| = {err:.3e}, max |grad| = {float(np.abs(g).max()):.3e}")
    assert np.abs(g).max() > 0.1 and err <= 1e-7


@pytest.mark.parametrize("hw, want", [(1.0, (2.748, 2.582, 2.530, 2.470)), (0.25, (0.4436, 0.4295, 0.4203, 0.4122))])
def test_R_alpha_reproduces_the_prototype(hw, want):
    """plain, 4, 8 and 16 steps of the literal y_0 - y_3 on 3-17-33-4 to 4 decimals (3 after the point on the cube of half-width 1, as
    the prototype's table prints them); the running minimum never rises; R_at at the plain rule is literal_common.R"""
    net, lo, hi, Cm = ca.table_case(hw)
    tr = ca.R_alpha(net.Ms, lo, hi, np.float64, Cm, 16)["trace"][:, 0, 0]
    run = np.minimum.accumulate(tr)
    assert np.all(np.diff(run) <= 0.0)
    got = (run[0], run[4], run[8], run[16])
    print(hw, got)
    assert [round(float(v), 3 if hw == 1.0 else 4) for v in got] == list(want)
    for T in (4, 8):
        r = ca.R_alpha(net.Ms, lo, hi, np.float64, Cm, T)
        assert r["smax"][0, 0] == run[T] and r["best_step"][0, 0] == int(np.argmin(tr[:T + 1]))
    plain = lc.R(net.Ms, lo, hi, np.float64, head=Cm)
    at = ca.R_at(net.Ms, lo, hi, np.float64, Cm, ca.plain_alpha(net.Ms, lo, hi, np.float64, 1))
    assert all(np.array_equal(a, b) for a, b in zip(at, plain[7:]))


# ----------------------------------------------------------------------------- the host routine
def host(n, T, a0=None):
    """the raw outputs of case n at T steps; a0: None, or "u" for the seeded uniform alpha0"""
    key = (n, T, a0)
    if key not in _cache:
        net, lo, hi, Cm = ca.cases()[n]
        alpha0 = None if a0 is None else ca.f32_uniform((Cm.shape[0], sum(net.xdims[1:-1]), lo.shape[1]), 77 + n)
        _cache[key] = ca.raw_host(net, lo, hi, Cm, T, alpha0=alpha0)
    return _cache[key]


def plain_host(n):
    net, lo, hi, Cm = ca.cases()[n]
    *six, lits = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=Cm, workers=1)
    return tuple(six) + tuple(lits)


@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_host_without_alpha_is_the_plain_pass(n):
    net, lo, hi, _ = ca.cases()[n]
    ca.check_no_alpha(lambda T, a0: host(n, T), plain_host(n), net, lo, hi, np.float32)


@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_host_is_never_looser(n):
    ca.check_never_looser(lambda T, a0: host(n, T))


@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_host_result_is_the_bound_of_the_alpha_it_reports(n):
    """|host - R_at(float64, alpha = the returned alpha)| / (1 + |v|) <= 2 HOST_FIGURE for every T and at the seeded alpha0, and
    a_smax = a_A c + |a_A| r + a_b0 to the same bound (float32 sums)"""
    net, lo, hi, Cm = ca.cases()[n]
    for T, a0 in [(T, None) for T in ca.STEPS] + [(0, "u")]:
        err, re = ca.pinned_errors(host(n, T, a0), net, lo, hi, Cm, np.float64)
        print(f"case {n} T={T} alpha0={a0}: |host - R_at(float64)| / (1 + |v|) = {err:.3e}, smax against its linear form {re:.3e}")
        assert err <= 2.0 * HOST_FIGURE and re <= 2.0 * HOST_FIGURE


@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_host_evaluates_at_a_given_alpha(n):
    net, lo, hi, Cm = ca.cases()[n]
    ca.check_given_alpha(lambda T, a0: host(n, T, "u"), net, lo, hi, Cm, np.float32, 77 + n)


def test_host_alpha_bounds_are_sound_on_sampled_points():
    """2000 points per box, the slack of the host literal pass's own test (tests/test_literal_bounds_cpu.py)"""
    import test_literal_bounds_cpu as lbc
    for cs in lc.sound_nets():
        lo, hi = cs["lo"][:, :8], cs["hi"][:, :8]
        for T in (3, 8):
            r = ca.raw_host(cs["net"], lo, hi, cs["C"], T)
            lc.assert_literals_sound(cs["net"], lo, hi, cs["C"], na.LiteralBounds(r["smin"], r["a_smax"], r["a_A"], r["a_b0"]), lbc.SLACK)


def test_host_refusals_arrive_as_messages():
    net, lo, hi, Cm = ca.cases()[0]
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    bad = np.full((Cm.shape[0], sum(net.xdims[1:-1]), lo.shape[1]), 0.5)
    bad[0, 3, 0] = np.nan
    for kw, word in ((dict(steps=-1), "steps"), (dict(steps=65), "steps"), (dict(steps=1, eta0=0.0), "eta0"), (dict(steps=1, eta0=np.inf), "eta0"),
                     (dict(steps=1, decay=0.0), "decay"), (dict(steps=1, decay=1.5), "decay"), (dict(steps=1, alpha0=bad), "alpha0")):
        rc, msg = ca.raw_host(net, lo, hi, Cm, check=False, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    rc, msg = ca.raw_host(tanh, lo, hi, Cm, 1, check=False)
    assert rc == -1 and "Tanh" in msg
    rc, msg = ca.raw_host(net, lo, hi, Cm[:0], 1, check=False)
    assert rc == -1 and "nlit" in msg


def test_the_python_route_keeps_the_smaller_bound():
    """makeIntervalsBatch(backend="host", alpha_steps=...): smax / A / b0 of whichever is smaller, the new fields beside them; without
    alpha the result is today's; backend="gpu" points to the resident bounder"""
    net, lo, hi, Cm = ca.cases()[1]
    *six, lits = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=Cm, alpha_steps=3)
    r, plain = host(1, 3), plain_host(1)
    assert all(np.array_equal(a, b) for a, b in zip(six, plain[:6])) and np.array_equal(lits.smin, plain[6])
    assert np.array_equal(lits.smax_plain, plain[7]) and np.array_equal(lits.smax, np.minimum(r["a_smax"], plain[7]))
    assert np.array_equal(lits.alpha, r["alpha"]) and np.array_equal(lits.best_step, r["best_step"])
    take = r["a_smax"] < plain[7]
    assert take.any() and np.array_equal(lits.A.transpose(0, 2, 1)[take], r["a_A"].transpose(0, 2, 1)[take]) and np.array_equal(lits.b0[~take], plain[9][~take])
    *_, today = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=Cm)
    assert type(today) is na.LiteralBounds and len(today) == 4 and today.alpha is None
    with pytest.raises(ValueError, match="resident"):
        na.makeIntervalsBatch(net, lo, hi, backend="gpu", normals=Cm, alpha_steps=3)


# ----------------------------------------------------------------------------- the driver
def driver_instance():
    """random_net([4, 24, 24, 24, 3], 7) on [-1, 1]^4, the literal y_0 - y_2 <= h = s + 0.1 (c0 - s): s the sampled maximum, c0 the root's
    plain literal smax"""
    if "driver" not in _cache:
        net, nrm = lc.random_net([4, 24, 24, 24, 3], 7), np.array([1.0, 0.0, -1.0])
        lo, hi = -np.ones(4), np.ones(4)
        X = lo[:, None] + np.random.default_rng(0).random((4, 20000)) * (hi - lo)[:, None]
        s = float((nrm @ lc.forward(net, X)).max())
        *_, lits = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="host", normals=nrm[None])
        c0 = float(lits.smax[0, 0])
        assert c0 > s
        _cache["driver"] = dict(net=net, lo=lo, hi=hi, normal=nrm, h=s + 0.1 * (c0 - s))
    return _cache["driver"]


def drive(backend="host", **kw):
    it = driver_instance()
    opts = na.split.SplitOptions(sdp_per_level=0, literal_bounds=True, crown_backend=backend, **kw)
    res = na.split.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, na.AdmmSdpOptions(), opts)
    assert res.verdict == "holds" and all(lf.proved_by == "crown" and lf.bound <= it["h"] for lf in res.leaves)
    lc.assert_tiles(res.leaves, it["lo"], it["hi"])
    return res.visited


def test_the_driver_visits_fewer_boxes():
    """boxes(alpha_steps = 4) <= 0.85 boxes(alpha_steps = 0); the numpy prototype gave 69 against 93"""
    plain, four, inherit = drive(), drive(alpha_steps=4), drive(alpha_steps=4, alpha_inherit=True)
    print(f"boxes: plain {plain}, alpha_steps=4 {four}, with alpha_inherit {inherit}")
    assert four <= 0.85 * plain


def test_option_errors():
    it = driver_instance()
    lit, o = [(it["normal"], it["h"])], na.AdmmSdpOptions()
    S = na.split.SplitOptions
    with pytest.raises(ValueError, match="literal_bounds"):
        na.split.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, o, S(sdp_per_level=0, alpha_steps=4))
    with pytest.raises(ValueError, match="crown_backend"):
        na.split.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, o, S(sdp_per_level=0, alpha_steps=4, literal_bounds=True, crown_backend="gpu"))
    tanh = na.FeedFwdNet(xdims=it["net"].xdims, Ms=it["net"].Ms, activ=na.methods.TanhActiv)
    with pytest.raises(ValueError, match="ReLU"):
        na.split.verifySplit(tanh, it["lo"], it["hi"], lit, 0, o, S(sdp_per_level=0, alpha_steps=4, literal_bounds=True))
