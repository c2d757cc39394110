"""The resident CROWN bounder (nnsdp_crown, csrc/crown_batch.hpp k_crown_resident; frontend.CrownBounder) on the GPU: the ReLU instance
has the bits of the one-shot entry, the Tanh instance is held against the numpy restatement R_tanh of tests/crown_tanh_common.py
(R_tanh(longdouble) the oracle, |R_tanh(float64) - R_tanh(longdouble)| the yardstick, as tests/test_crown_batch_gpu.py does for ReLU),
against sampled points and against the float32 host routine; the handle keeps its buffers, and two handles do not disturb each other."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import crown_tanh_common as tc
import literal_common as lc
import test_crown_batch_gpu as cb
import test_literal_bounds_gpu as lb

ALL = lc.NAMES + lc.LIT_NAMES
EPS = 2.0 ** -52
NBOX = 257
# the device library's fp64 tanh and cosh are documented to stay within 1 ulp of the correctly rounded result (HIP math API reference,
# double precision functions); numpy's are the C library's.  The yardstick r of the Tanh tests therefore also holds the float64
# restatement run with every tanh / cosh result moved by that one ulp in a seeded direction - computed without the kernel
DEVICE_ULPS = 1.0
TANH_CASES = ("2-15-2", "2-16-16-2", "3-17-33-4", "5-63-64-5", "64-64-64-64", "2-10x5-2", "W10-D5", "1-1-1")
_cache = {}


def same(a, b, what):
    a, b = tc.flat(a), tc.flat(b)
    assert len(a) == len(b), what
    for nm, x, y in zip(ALL, a, b):
        assert x.shape == y.shape and np.array_equal(x, y), (what, nm)


# ----------------------------------------------------------------------------- ReLU: the bits of the one-shot entry
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cb.CASES))
def test_relu_has_the_bits_of_the_one_shot_entry(name):
    """nbox 257, 2, 1, 257 on one bounder (stale buffer contents would show), 1 then 257 on a second (growth)"""
    cs = cb.case(name)
    want = {NBOX: cs["gpu"]}
    for nbox in (1, 2):
        want[nbox] = na.makeIntervalsBatch(cs["net"], cs["lo"][:, :nbox], cs["hi"][:, :nbox], backend="gpu")
    for order in ((NBOX, 2, 1, NBOX), (1, NBOX)):
        with na.CrownBounder(cs["net"]) as bd:
            for nbox in order:
                same(bd.bound(cs["lo"][:, :nbox], cs["hi"][:, :nbox]), want[nbox], (name, order, nbox))


@pytest.mark.gpu
@pytest.mark.parametrize("nlit", [1, 17, 64])
@pytest.mark.parametrize("name", list(lb.CASES))
def test_relu_literals_have_the_bits_of_the_one_shot_entry(name, nlit):
    cs = lb.case(name)
    want = {NBOX: lb.gpu(name, nlit)[:2]}
    for nbox in (1, 2):
        *six, lits = na.makeIntervalsBatch(cs["net"], cs["lo"][:, :nbox], cs["hi"][:, :nbox], backend="gpu", normals=cs["C"][:nlit])
        want[nbox] = (six, lits)
    for order in ((NBOX, 2, 1, NBOX), (1, NBOX)):
        with na.CrownBounder(cs["net"], cs["C"][:nlit]) as bd:
            for nbox in order:
                six, lits = want[nbox]
                same(bd.bound(cs["lo"][:, :nbox], cs["hi"][:, :nbox]), tuple(six) + (lits,), (name, nlit, order, nbox))


# ----------------------------------------------------------------------------- Tanh against the oracle
def tanh_case(name):
    """Tanh copy of a net of tests/test_crown_batch_gpu.py, its 257 boxes, 17 literal rows, R_tanh(float64) and R_tanh(longdouble) of all
    ten arrays, R_tanh(float64) with tanh / cosh moved by DEVICE_ULPS, the regimes of the hidden neurons, and the 257-box GPU result:
    computed once, shared, never modified"""
    key = ("tanh", name)
    if key not in _cache:
        net = tc.tanh_copy(cb.CASES[name]())
        lo, hi = cb.boxes(net.xdims[0], NBOX, seed=sum(map(ord, name)))
        Cm = lc.literal_rows(net.xdims[-1], 17, seed=1000 + sum(map(ord, name)))
        regimes = []
        r64 = tc.R_tanh(net.Ms, lo, hi, np.float64, Cm, regimes=regimes)
        rld = tc.R_tanh(net.Ms, lo, hi, np.longdouble, Cm)
        rmv = tc.R_tanh(net.Ms, lo, hi, np.float64, Cm, lib=tc.Moved(DEVICE_ULPS, seed=sum(map(ord, name))))
        with na.CrownBounder(net, Cm) as bd:
            gpu = tc.flat(bd.bound(lo, hi))
        _cache[key] = dict(net=net, lo=lo, hi=hi, C=Cm, r64=r64, rld=rld, rmv=rmv, regimes=np.concatenate(regimes, axis=1), gpu=gpu)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("nlit", [1, 17])
@pytest.mark.parametrize("nbox", [1, 2, 257])
@pytest.mark.parametrize("name", TANH_CASES)
def test_tanh_against_the_numpy_recurrences(name, nbox, nlit):
    """|GPU - R_tanh(longdouble)| <= max(8 r, 64 * 2^-52 * s) for each of the ten arrays, s = max |value| of that array over the call: the
    formula and margin of tests/test_crown_batch_gpu.py.  r = max |R_tanh(float64) - R_tanh(longdouble)| + max |R_tanh(float64 with tanh
    and cosh moved by DEVICE_ULPS) - R_tanh(longdouble)|.  The second term is there because the first alone was exceeded on the GPU by
    one array of one case, and reading gave the reason: on a box 1e-6 wide the chord slope (tanh u - tanh l) / (u - l) of a
    pre-activation interval about 1e-5 wide multiplies the rounding of the two tanh values by 1e5, so the coefficients A and the
    constant b0 (not the bounds, where the two cancel) carry that library's rounding at 1e-12, and at nbox = 2, nlit = 1 the first
    term is one draw of numpy's own rounding (b0 of 64-64-64-64: err 4.2e-12 against r 3.7e-13 without the second term, ratio 11.5;
    every other array of the 26 cases run before it stayed below 3.7).  The test prints err / max(r, 8 * 2^-52 s) per array (8 is the
    limit).  Every regime of the relaxation (u <= 0, l >= 0, crossing) occurs in the 257 boxes of every case with more than one hidden
    neuron."""
    cs = tanh_case(name)
    if name != "1-1-1":
        assert all((cs["regimes"] == k).any() for k in (0, 1, 2)), "a regime of the relaxation does not occur"
    if nbox == NBOX and nlit == 17:
        got = cs["gpu"]
    else:
        with na.CrownBounder(cs["net"], cs["C"][:nlit]) as bd:
            got = tc.flat(bd.bound(cs["lo"][:, :nbox], cs["hi"][:, :nbox]))
    worst = 0.0
    for i, (nm, g, a64, ald, amv) in enumerate(zip(ALL, got, cs["r64"], cs["rld"], cs["rmv"])):
        cut = (lambda a: a[..., :nbox]) if i < 6 else (lambda a: a[:nlit, ..., :nbox])
        a64, ald, amv = cut(a64), cut(ald), cut(amv)
        assert g.shape == a64.shape, nm
        r = float(np.abs(a64 - ald).max() + np.abs(amv - ald).max()) if a64.size else 0.0
        s = float(np.abs(ald).max()) if ald.size else 0.0
        err = float(np.abs(g - ald).max()) if g.size else 0.0
        tol = max(8.0 * r, 64.0 * EPS * s)
        ratio = err / max(r, 8.0 * EPS * s) if max(r, s) > 0 else 0.0
        worst = max(worst, ratio)
        print(f"tanh {name} nbox={nbox} nlit={nlit} {nm}: err {err:.3e}  r {r:.3e}  s {s:.3e}  tol {tol:.3e}  err / max(r, floor / 8) = {ratio:.3f}")
        assert np.all(np.isfinite(g)), nm
        assert err <= tol, (name, nbox, nlit, nm, err, tol)
    print(f"tanh {name} nbox={nbox} nlit={nlit}: largest ratio {worst:.3f} (8 allowed)")


def sound_gpu():
    if "sound" not in _cache:
        out = []
        for cs in tc.sound_tanh():
            with na.CrownBounder(cs["net"], cs["C"]) as bd:
                out.append(tc.flat(bd.bound(cs["lo"], cs["hi"])))
        _cache["sound"] = out
    return _cache["sound"]


@pytest.mark.gpu
def test_tanh_bounds_are_sound_on_sampled_points():
    """2000 points per box: hidden post-activations and outputs inside their intervals, smin <= normal' f(x) <= smax and
    normal' f(x) <= A' x + b0, slack 1e-9 (1 + |v|)"""
    for cs, g in zip(tc.sound_tanh(), sound_gpu()):
        tc.assert_hidden_and_output_sound(cs["net"], cs["lo"], cs["hi"], g[0], g[1], g[4], g[5])
        lc.assert_literals_sound(cs["net"], cs["lo"], cs["hi"], cs["C"], na.LiteralBounds(*g[6:]), 1e-9)


@pytest.mark.gpu
def test_tanh_agrees_with_the_float32_host_routine():
    """the host routine computes in float32 by design: max |GPU - host| / (1 + |v|) stays within twice the figure
    max |R_tanh(float64) - host| / (1 + |v|), measured on the CPU (tests/test_crown_resident_cpu.py) and recomputed here"""
    figure = tc.host_figure()
    gpu = max(tc.rel_err(g, h) for cs, got in zip(tc.sound_tanh(), sound_gpu()) for g, h in zip(got, cs["host"]))
    print(f"max |R_tanh(float64) - host| / (1 + |v|) = {figure:.3e};  max |GPU - host| / (1 + |v|) = {gpu:.3e}")
    assert 0.0 < figure < 1e-4
    assert gpu <= 2.0 * figure


# ----------------------------------------------------------------------------- position and company
@pytest.mark.gpu
def test_a_tanh_box_has_the_same_bits_wherever_it_stands():
    for name in ("3-17-33-4", "64-64-64-64", "W10-D5"):
        cs = tanh_case(name)
        with na.CrownBounder(cs["net"], cs["C"]) as bd:
            for j in (0, 1, 130, 256):
                one = tc.flat(bd.bound(cs["lo"][:, [j]], cs["hi"][:, [j]]))
                for nm, a, g in zip(ALL, one, cs["gpu"]):
                    assert np.array_equal(a[..., 0], g[..., j]), (name, j, nm)


@pytest.mark.gpu
def test_a_tanh_literal_has_the_same_bits_alone_and_among_others():
    for name in ("3-17-33-4", "64-64-64-64"):
        cs = tanh_case(name)
        for i in (0, 1, 5, 16):
            with na.CrownBounder(cs["net"], cs["C"][[i]]) as bd:
                alone = tc.flat(bd.bound(cs["lo"], cs["hi"]))
            for nm, a, g in zip(ALL[:6], alone, cs["gpu"]):
                assert np.array_equal(a, g), (name, i, nm)
            for nm, a, g in zip(lc.LIT_NAMES, alone[6:], cs["gpu"][6:]):
                assert np.array_equal(a[0], g[i]), (name, i, nm)


# ----------------------------------------------------------------------------- residency
@pytest.mark.gpu
def test_the_network_is_uploaded_once_and_the_buffers_are_kept():
    cs = tanh_case("3-17-33-4")
    with na.CrownBounder(cs["net"], cs["C"]) as bd:
        i0 = bd.info()
        assert i0["network_uploads"] == 1 and i0["bound_calls"] == 0 and i0["box_capacity"] == 0 and i0["device_allocations"] > 0
        first = tc.flat(bd.bound(cs["lo"][:, :40], cs["hi"][:, :40]))
        i1 = bd.info()
        assert i1["box_capacity"] >= 40 and i1["device_allocations"] > i0["device_allocations"] and i1["device_bytes"] > i0["device_bytes"]
        for nbox in (40, 1, 17, 2):
            bd.bound(cs["lo"][:, :nbox], cs["hi"][:, :nbox])
        i2 = bd.info()
        assert i2["bound_calls"] == 5
        assert (i2["device_allocations"], i2["network_uploads"], i2["box_capacity"], i2["device_bytes"]) == \
               (i1["device_allocations"], 1, i1["box_capacity"], i1["device_bytes"])
        big = tc.flat(bd.bound(cs["lo"], cs["hi"]))                    # 257 boxes: above the capacity
        i3 = bd.info()
        assert i3["box_capacity"] >= NBOX > i1["box_capacity"] and i3["device_allocations"] > i2["device_allocations"]
        assert i3["network_uploads"] == 1
        same(big, cs["gpu"], "after growth")
        same(bd.bound(cs["lo"][:, :40], cs["hi"][:, :40]), first, "a repeat of an earlier call")
        assert bd.info()["sample_capacity"] == 0
        bd.eval(cs["lo"][:, :5])
        assert bd.info()["sample_capacity"] >= 5 and bd.info()["network_uploads"] == 1
    with pytest.raises(ValueError, match="closed"):
        bd.info()


@pytest.mark.gpu
@pytest.mark.parametrize("activ", ["relu", "tanh"])
def test_eval_has_the_bits_of_the_one_shot_forward_pass(activ):
    net = cb.CASES["5-63-64-5"]()
    if activ == "tanh":
        net = tc.tanh_copy(net)
    X = np.random.default_rng(7).normal(size=(5, 1000))
    with na.CrownBounder(net) as bd:
        for N in (1, 16, 17, 1000, 16):
            Y, ms = bd.eval(X[:, :N], return_ms=True)
            assert Y.shape == (5, N) and ms > 0.0
            assert np.array_equal(Y, na.evalFeedFwdNetBatch(net, X[:, :N])), N
        assert bd.eval(X[:, :0]).shape == (5, 0)


@pytest.mark.gpu
def test_two_bounders_alive_at_once():
    a, b = cb.case("5-63-64-5"), tanh_case("3-17-33-4")
    with na.CrownBounder(a["net"]) as ba, na.CrownBounder(b["net"], b["C"]) as bb:
        for nbox in (NBOX, 3, NBOX):
            ga = ba.bound(a["lo"][:, :nbox], a["hi"][:, :nbox])
            gb = bb.bound(b["lo"][:, :nbox], b["hi"][:, :nbox])
            same(ga, tuple(x[:, :nbox] for x in a["gpu"]), ("relu", nbox))
            same(gb, tuple(x[..., :nbox] for x in b["gpu"]), ("tanh", nbox))


# ----------------------------------------------------------------------------- refusals through the handle
@pytest.mark.gpu
def test_a_bad_box_is_refused_with_the_one_shot_messages():
    net = tc.tanh_copy(lc.random_net([2, 3, 2], 1))
    lo, hi = np.zeros((2, 4)), np.ones((2, 4))
    with na.CrownBounder(net, np.ones((3, 2))) as bd:
        bad = hi.copy()
        bad[1, 2] = -1.0
        with pytest.raises(_lib.NnsdpError, match="box 2.*x1min must be <= x1max"):
            bd.bound(lo, bad)
        bad[1, 2] = np.nan
        with pytest.raises(_lib.NnsdpError, match="box 2.*NaN"):
            bd.bound(lo, bad)
        bad[1, 2], bad[0, 1] = 1.0, np.inf
        with pytest.raises(_lib.NnsdpError, match="box 1.*finite"):
            bd.bound(lo, bad)
        with pytest.raises(ValueError):
            bd.bound(lo[:1], hi[:1])
        *six, lits = bd.bound(lo[:, :0], hi[:, :0])
        assert all(x.shape[1] == 0 for x in six) and lits.smax.shape == (3, 0) and lits.A.shape == (3, 2, 0)
        assert bd.info()["bound_calls"] == 0
        assert len(bd.bound(lo, hi)) == 7 and bd.info()["bound_calls"] == 1
    with pytest.raises(_lib.NnsdpError, match="65"):
        na.CrownBounder(lc.random_net([2, 65, 2], 1))
