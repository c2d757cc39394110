"""Optimised ReLU slopes (alpha-CROWN) on the GPU: nnsdp_crown_bound_alpha (csrc/crown_alpha.hpp, k_crown_alpha behind the resident
bounder's kernel) against the numpy yardstick of tests/crown_alpha_common.py, and the split driver with crown_backend="resident"."""
import numpy as np
import pytest

import nnsdp_amd as na
import crown_alpha_common as ca
import literal_common as lc
import test_crown_alpha_cpu as cpu

_cache = {}


def gpu(n, T, a0=None):
    """the raw outputs of case n at T steps (a0: None, "u" the seeded uniform alpha0, "h" alpha0 = 0.5 with eta0 = 1e-3), each on a
    bounder of its own; computed once, shared, never modified"""
    key = (n, T, a0)
    if key not in _cache:
        net, lo, hi, Cm = ca.cases()[n]
        shape = (Cm.shape[0], sum(net.xdims[1:-1]), lo.shape[1])
        alpha0 = {None: None, "u": ca.f32_uniform(shape, 77 + n), "h": np.full(shape, 0.5)}[a0]
        with na.CrownBounder(net, Cm) as bd:
            _cache[key] = ca.raw_gpu(bd, lo, hi, T, eta0=1e-3 if a0 == "h" else 0.5, alpha0=alpha0)
    return _cache[key]


def plain_gpu(n):
    key = ("plain", n)
    if key not in _cache:
        net, lo, hi, Cm = ca.cases()[n]
        with na.CrownBounder(net, Cm) as bd:
            *six, lits = bd.bound(lo, hi)
        _cache[key] = tuple(six) + tuple(lits)
    return _cache[key]


def pinned(res, n):
    """test 3's check of one result: within 8 r of R_at(longdouble) at the returned alpha, r = max |R_at(float64) - R_at(longdouble)| /
    (1 + |v|) at that alpha (the 8 r of tests/test_literal_bounds_gpu.py; the largest err / r measured on the MI355X was 3.0), and
    a_smax = a_A c + |a_A| r + a_b0 to 1e-12 (1 + |v|)"""
    net, lo, hi, Cm = ca.cases()[n]
    r64, rld = ca.R_at(net.Ms, lo, hi, np.float64, Cm, res["alpha"]), ca.R_at(net.Ms, lo, hi, np.longdouble, Cm, res["alpha"])
    r = max(ca.rel_err(a, b) for a, b in zip(r64, rld))
    err, re = ca.pinned_errors(res, net, lo, hi, Cm, np.longdouble)
    tol = 8.0 * r
    print(f"case {n}: err {err:.3e}  r {r:.3e}  tol {tol:.3e}  err / r = {err / r if r > 0 else 0.0:.3f} (8 allowed);  smax against its linear form {re:.3e}")
    assert all(np.all(np.isfinite(res[k])) for k in ca.A_KEYS)
    assert err <= tol and re <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_without_alpha_it_is_the_plain_pass(n):
    net, lo, hi, _ = ca.cases()[n]
    ca.check_no_alpha(lambda T, a0: gpu(n, T), plain_gpu(n), net, lo, hi, np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_never_looser(n):
    ca.check_never_looser(lambda T, a0: gpu(n, T))


@pytest.mark.gpu
@pytest.mark.parametrize("T", ca.STEPS)
@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_the_result_is_the_bound_of_the_alpha_it_reports(n, T):
    pinned(gpu(n, T), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_evaluation_at_a_given_alpha(n):
    net, lo, hi, Cm = ca.cases()[n]
    pinned(ca.check_given_alpha(lambda T, a0: gpu(n, T, "u"), net, lo, hi, Cm, np.float64, 77 + n), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(ca.cases())))
def test_the_gradient(n):
    """alpha0 = 0.5, one step with eta0 = 1e-3 on the boxes of half-width >= 0.05: best_step == 1 wherever the yardstick's max|g| > 0,
    and the returned alpha is clip(0.5 - 1e-3 g / max|g|, 0, 1) with the yardstick's g to 1e-10 absolute"""
    net, lo, hi, Cm = ca.cases()[n]
    wide = np.flatnonzero((hi - lo).min(axis=0) >= 0.1 - 1e-12)
    assert len(wide) == (3 if lo.shape[1] == 5 else 1)
    res = gpu(n, 1, "h")
    a0 = np.full(res["alpha"].shape, 0.5)
    g = ca.grad(net.Ms, lo, hi, np.float64, Cm, a0)
    gmax = np.abs(g).max(axis=1)                                             # nlit x nbox
    uns = np.broadcast_to(ca.unstable_mask(net.Ms, lo, hi, np.float64)[None], g.shape)
    moved = np.clip(0.5 - 1e-3 * g / np.where(gmax > 0, gmax, 1.0)[:, None, :], 0.0, 1.0)
    want = np.where(uns, moved, ca.plain_alpha(net.Ms, lo, hi, np.float64, Cm.shape[0]))
    live = gmax[:, wide] > 0
    err = float(np.abs(res["alpha"] - want)[:, :, wide].max())
    print(f"case {n}: {int(live.sum())} of {live.size} literals move, max |alpha - yardstick| = {err:.3e}")
    assert live.any() and np.all(res["best_step"][:, wide][live] == 1) and not res["best_step"][:, wide][~live].any()
    assert err <= 1e-10


@pytest.mark.gpu
def test_alpha_bounds_are_sound_on_sampled_points():
    """2000 points per box, 8 boxes of each net of sound_nets, slack 1e-9 (1 + |v|) as tests/test_literal_bounds_gpu.py"""
    for cs in lc.sound_nets():
        lo, hi = cs["lo"][:, :8], cs["hi"][:, :8]
        with na.CrownBounder(cs["net"], cs["C"]) as bd:
            for T in (3, 8):
                r = ca.raw_gpu(bd, lo, hi, T)
                lc.assert_literals_sound(cs["net"], lo, hi, cs["C"], na.LiteralBounds(r["smin"], r["a_smax"], r["a_A"], r["a_b0"]), 1e-9)


@pytest.mark.gpu
def test_independence():
    """a literal alone has its bits among 17; a box alone has its bits among 5; a second call on the handle repeats the first"""
    for n17 in (2, 6):
        net, lo, hi, C17 = ca.cases()[n17]
        for T, a0 in ((8, None), (3, "u")):
            together = gpu(n17, T, a0)
            alpha0 = None if a0 is None else ca.f32_uniform(together["alpha"].shape, 77 + n17)
            for i in (0, 5, 16):
                with na.CrownBounder(net, C17[[i]]) as bd:
                    alone = ca.raw_gpu(bd, lo, hi, T, alpha0=None if alpha0 is None else alpha0[[i]])
                for k in lc.LIT_NAMES + ca.A_KEYS:
                    assert np.array_equal(alone[k][0], together[k][i]), (n17, T, i, k)
            with na.CrownBounder(net, C17) as bd:
                for j in range(lo.shape[1]):
                    one = ca.raw_gpu(bd, lo[:, [j]], hi[:, [j]], T, alpha0=None if alpha0 is None else alpha0[:, :, [j]])
                    for k in ca.KEYS + ca.A_KEYS:
                        assert np.array_equal(one[k][..., 0], together[k][..., j]), (n17, T, j, k)
                again = ca.raw_gpu(bd, lo, hi, T, alpha0=alpha0)
                for k in ca.KEYS + ca.A_KEYS:
                    assert np.array_equal(again[k], together[k]), (n17, T, k)


@pytest.mark.gpu
def test_the_handle():
    """a bounder that only calls bound holds what it held before there was an alpha entry (the sums of nnsdp_crown's buffers: the widths,
    the offsets, the network with the head, and per box of capacity the boxes, the scratch and the ten outputs); the alpha buffers come
    with the first alpha call and stay; the refusals arrive as messages"""
    net, lo, hi, Cm = ca.cases()[2]
    K, xd, nlit = net.K, net.xdims, Cm.shape[0]
    n0, ny, acdim = xd[0], xd[-1], sum(xd[1:-1])
    fixed = 4 * (K + 1) + 4 * K + 8 * (K + 1) + 8 * (sum(xd[k + 1] * (xd[k] + 1) for k in range(K)) + nlit * (xd[K - 1] + 1))
    per_box = 8 * (2 * n0 + 2 * acdim + 4 * acdim + 2 * ny + 3 * nlit + nlit * n0)
    with na.CrownBounder(net, Cm) as bd:
        assert (bd.info()["device_allocations"], bd.info()["device_bytes"]) == (4, fixed)
        bd.bound(lo, hi)
        i1 = bd.info()
        assert (i1["device_allocations"], i1["device_bytes"], i1["box_capacity"]) == (7, fixed + 5 * per_box, 5)
        first = ca.raw_gpu(bd, lo, hi, 3)
        i2 = bd.info()
        assert i2["device_allocations"] == 10 and i2["device_bytes"] > i1["device_bytes"] and i2["network_uploads"] == 1
        for nbox, T in ((5, 8), (1, 0), (3, 3), (5, 3)):
            last = ca.raw_gpu(bd, lo[:, :nbox], hi[:, :nbox], T)
        i3 = bd.info()
        assert (i3["device_allocations"], i3["network_uploads"], i3["device_bytes"]) == (10, 1, i2["device_bytes"]) and i3["bound_calls"] == 6
        assert all(np.array_equal(first[k], last[k]) for k in ca.KEYS + ca.A_KEYS)
        # the Python route: the smaller of the two, the new fields beside it
        *six, lits = bd.bound(lo, hi, alpha_steps=3)
        plain = plain_gpu(2)
        assert isinstance(lits, na.LiteralBounds) and np.array_equal(lits.smax_plain, plain[7]) and np.array_equal(lits.smax, first["a_smax"])
        take = first["a_smax"] < plain[7]
        assert take.any() and np.array_equal(lits.A.transpose(0, 2, 1)[take], first["a_A"].transpose(0, 2, 1)[take])
        assert np.array_equal(lits.b0[~take], plain[9][~take]) and np.array_equal(lits.alpha, first["alpha"])
        assert np.array_equal(lits.best_step, first["best_step"])
        # refusals
        bad = np.full(first["alpha"].shape, 0.5)
        bad[1, 2, 3] = np.inf
        for kw, word in ((dict(steps=-1), "steps"), (dict(steps=65), "steps"), (dict(steps=1, eta0=-1.0), "eta0"), (dict(steps=1, eta0=np.nan), "eta0"),
                         (dict(steps=1, decay=0.0), "decay"), (dict(steps=1, decay=1.01), "decay"), (dict(steps=1, alpha0=bad), "alpha0")):
            rc, msg = ca.raw_gpu(bd, lo, hi, check=False, **kw)
            assert rc == -1 and word in msg, (kw, msg)
        assert bd.info()["bound_calls"] == 7
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    with na.CrownBounder(tanh, Cm) as bd:
        rc, msg = ca.raw_gpu(bd, lo, hi, 1, check=False)
        assert rc == -1 and "Tanh" in msg
    with na.CrownBounder(net) as bd:
        rc, msg = ca.raw_gpu(bd, lo, hi, 1, check=False)
        assert rc == -1 and "literals" in msg
        assert bd.info()["device_allocations"] == 4


@pytest.mark.gpu
def test_it_tightens():
    """3-17-33-4, the cube of half-width 1, the literal y_0 - y_3: 8 steps gain at least half of what the yardstick gains in float64
    (2.748 to 2.530 there; a kink crossed in another order may change the path, not the order of magnitude)"""
    net, lo, hi, Cm = ca.table_case(1.0)
    y = ca.R_alpha(net.Ms, lo, hi, np.float64, Cm, 8)
    with na.CrownBounder(net, Cm) as bd:
        r = ca.raw_gpu(bd, lo, hi, 8)
    want, got = float(y["trace"][0, 0, 0] - y["smax"][0, 0]), float(r["smax"][0, 0] - r["a_smax"][0, 0])
    print(f"plain {r['smax'][0, 0]:.6f}, 8 steps {r['a_smax'][0, 0]:.6f} (best step {r['best_step'][0, 0]}): gain {got:.6f}, yardstick's gain {want:.6f}")
    assert want > 0.2 and got >= 0.5 * want


@pytest.mark.gpu
def test_the_driver_on_the_resident_bounder():
    """the instance of the CPU driver test, alpha_steps = 4: "holds" with tiling leaves, the box count within 2 of the host backend's"""
    res, host = cpu.drive("resident", alpha_steps=4), cpu.drive(alpha_steps=4)
    inherit = cpu.drive("resident", alpha_steps=4, alpha_inherit=True)
    print(f"boxes: resident {res}, host {host}, resident with alpha_inherit {inherit}")
    assert abs(res - host) <= 2
