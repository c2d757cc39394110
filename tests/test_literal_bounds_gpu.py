"""The literal pass of the batched CROWN kernel (nnsdp_make_intervals_batch_lits, csrc/crown_batch.hpp; makeIntervalsBatch with
normals, backend="gpu") against the numpy restatement R of literal_common with a head: R(longdouble) is the oracle,
|R(float64) - R(longdouble)| the yardstick of the tolerance, as in tests/test_crown_batch_gpu.py."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
from literal_common import LIT_NAMES, NAMES, R, assert_literals_sound, boxes, literal_rows, random_net, sound_nets

NBOX = 257
EPS = 2.0 ** -52
CASES = {
    "1-1-1": lambda: random_net([1, 1, 1], 11),
    "2-16-16-2": lambda: random_net([2, 16, 16, 2], 13),
    "3-17-33-4": lambda: random_net([3, 17, 33, 4], 14),
    "5-63-64-5": lambda: random_net([5, 63, 64, 5], 15),
    "64-64-64-64": lambda: random_net([64, 64, 64, 64], 16),
    "2-10x5-2": lambda: random_net([2, 10, 10, 10, 10, 10, 2], 17),
}
_cache = {}


def case(name):
    """net, 257 boxes, the 64 literal rows, R(float64) and R(longdouble) with all 64 rows: computed once, shared, never modified.  Row i
    of the literal outputs of R does not depend on the other rows beyond the rounding that r measures."""
    if name not in _cache:
        net = CASES[name]()
        lo, hi = boxes(net.xdims[0], NBOX, seed=sum(map(ord, name)))
        Cm = literal_rows(net.xdims[-1], 64, seed=1000 + sum(map(ord, name)))
        _cache[name] = dict(net=net, lo=lo, hi=hi, C=Cm, r64=R(net.Ms, lo, hi, np.float64, head=Cm), rld=R(net.Ms, lo, hi, np.longdouble, head=Cm))
    return _cache[name]


def gpu(name, nlit, nbox=NBOX):
    """(six arrays, LiteralBounds, kernel ms) of the first nbox boxes with the first nlit literal rows"""
    key = (name, nlit, nbox)
    if key not in _cache:
        cs = case(name)
        *six, lits, ms = na.makeIntervalsBatch(cs["net"], cs["lo"][:, :nbox], cs["hi"][:, :nbox], backend="gpu", normals=cs["C"][:nlit], return_ms=True)
        _cache[key] = (six, lits, ms)
    return _cache[key]


def tol_of(a64, ald):
    r = float(np.abs(a64 - ald).max()) if a64.size else 0.0
    s = float(np.abs(ald).max()) if ald.size else 0.0
    return r, s, max(8.0 * r, 64.0 * EPS * s)


@pytest.mark.gpu
@pytest.mark.parametrize("nlit", [1, 16, 17, 64])
@pytest.mark.parametrize("nbox", [1, 2, 257])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_numpy_recurrences(name, nbox, nlit):
    """|GPU - R(longdouble)| <= max(8 r, 64 * 2^-52 * s) for smin, smax, A and b0, r = max |R(float64) - R(longdouble)| and s = max |value|
    of that array over the call.  The test prints err / max(r, 8 * 2^-52 s) per array (8 is the limit).  Beside it: the zero row is
    exactly zero, the rows e_0 and -e_0 repeat the raw output pass, and smax is the returned linear bound over the box."""
    cs = case(name)
    six, lits, _ = gpu(name, nlit, nbox)
    n0, ny = cs["net"].xdims[0], cs["net"].xdims[-1]
    assert lits.smin.shape == lits.smax.shape == lits.b0.shape == (nlit, nbox) and lits.A.shape == (nlit, n0, nbox)
    tols, worst = {}, 0.0
    for nm, g, a64, ald in zip(LIT_NAMES, lits, cs["r64"][6:], cs["rld"][6:]):
        a64, ald = a64[:nlit, ..., :nbox], ald[:nlit, ..., :nbox]
        r, s, tol = tol_of(a64, ald)
        tols[nm] = tol
        err = float(np.abs(g - ald).max())
        ratio = err / max(r, 8.0 * EPS * s) if max(r, s) > 0 else 0.0
        worst = max(worst, ratio)
        print(f"{name} nbox={nbox} nlit={nlit} {nm}: err {err:.3e}  r {r:.3e}  s {s:.3e}  tol {tol:.3e}  err / max(r, floor / 8) = {ratio:.3f}")
        assert np.all(np.isfinite(g)), nm
        assert err <= tol, (name, nbox, nlit, nm, err, tol)
    print(f"{name} nbox={nbox} nlit={nlit}: largest ratio {worst:.3f} (8 allowed)")
    # the zero row (row 3; with one output row 0 = e_0 - e_0 as well)
    for i in [3] * (nlit > 3) + [0] * (ny == 1):
        assert not lits.smin[i].any() and not lits.smax[i].any() and not lits.b0[i].any() and not lits.A[i].any(), i
    # e_0 and -e_0 against the output pass, where its post-fix did not act (it acted only where it left ymin == ymax)
    if nlit > 2:
        ymin, ymax = six[4][0], six[5][0]
        raw = ymin < ymax
        for nm, got, want, k in (("smax(e_0)", lits.smax[1], ymax, 5), ("smin(e_0)", lits.smin[1], ymin, 4),
                                 ("smax(-e_0)", lits.smax[2], -ymin, 4), ("smin(-e_0)", lits.smin[2], -ymax, 5)):
            _, _, tol = tol_of(cs["r64"][k][:, :nbox], cs["rld"][k][:, :nbox])
            err = float(np.abs(got - want)[raw].max()) if raw.any() else 0.0
            print(f"{name} nbox={nbox} nlit={nlit} {nm} against the output pass: err {err:.3e}  tol {tol:.3e}  ({int(raw.sum())} boxes)")
            assert err <= tol, nm
    # smax = A c + |A| r + b0, recomputed in longdouble from the returned A and b0
    ld = np.longdouble
    lo, hi = cs["lo"][:, :nbox].astype(ld), cs["hi"][:, :nbox].astype(ld)
    c, rad = (hi + lo) / ld(2), (hi - lo) / ld(2)
    A = lits.A.astype(ld)
    re = np.einsum("iqb,qb->ib", A, c) + np.einsum("iqb,qb->ib", np.abs(A), rad) + lits.b0.astype(ld)
    err = float(np.abs(re - lits.smax).max())
    print(f"{name} nbox={nbox} nlit={nlit} smax - (A c + |A| r + b0): {err:.3e}  tol {tols['smax']:.3e}")
    assert err <= tols["smax"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_never_looser_than_the_per_output_bound(name):
    """smax <= cheap + max(8 r, 64 * 2^-52 * s) per literal and box: cheap = sum_j max(n_j ymin_j, n_j ymax_j) from the same call,
    s = sum_j |n_j| max(|ymin_j|, |ymax_j|), r the larger fp64-against-longdouble difference of the two sides over the call.  (In exact
    arithmetic the literal bound is never above cheap; an fp64 emulation measured 3.3e-16 relative.)"""
    cs = case(name)
    six, lits, _ = gpu(name, 64)
    cheap = lambda ymin, ymax: np.stack([np.maximum(n[:, None] * ymin, n[:, None] * ymax).sum(axis=0) for n in cs["C"].astype(ymin.dtype)])
    c64, cld = cheap(cs["r64"][4], cs["r64"][5]), cheap(cs["rld"][4], cs["rld"][5])
    r = max(float(np.abs(c64 - cld).max()), float(np.abs(cs["r64"][7] - cs["rld"][7]).max()))
    s = np.abs(cs["C"]) @ np.maximum(np.abs(six[4]), np.abs(six[5]))
    over = lits.smax - cheap(six[4], six[5])
    tol = np.maximum(8.0 * r, 64.0 * EPS * s)
    print(f"{name}: max (smax - cheap) / max(1, |cheap|) = {float((over / np.maximum(1.0, np.abs(cheap(six[4], six[5])))).max()):.3e}, "
          f"r {r:.3e}, largest over / tol {float((over / np.where(tol > 0, tol, 1.0)).max()):.3f}")
    assert np.all(over <= tol)


@pytest.mark.gpu
def test_literal_bounds_are_sound_on_sampled_points():
    """2000 points per box: smin - slack <= C f(x) <= smax + slack and C f(x) <= A x + b0 + slack, slack = 1e-9 (1 + |v|)"""
    for cs in sound_nets():
        *_, lits = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="gpu", normals=cs["C"])
        assert_literals_sound(cs["net"], cs["lo"], cs["hi"], cs["C"], lits, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_six_arrays_keep_their_bits(name):
    cs = case(name)
    plain = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="gpu")
    for nlit in (1, 17, 64):
        for nm, a, b in zip(NAMES, plain, gpu(name, nlit)[0]):
            assert np.array_equal(a, b), (nlit, nm)


@pytest.mark.gpu
def test_a_box_has_the_same_literal_bits_wherever_it_stands():
    for name in ("3-17-33-4", "64-64-64-64", "2-10x5-2"):
        cs = case(name)
        _, all_boxes, _ = gpu(name, 17)
        for j in (0, 1, 130, 256):
            *_, one = na.makeIntervalsBatch(cs["net"], cs["lo"][:, [j]], cs["hi"][:, [j]], backend="gpu", normals=cs["C"][:17])
            for nm, a, g in zip(LIT_NAMES, one, all_boxes):
                assert np.array_equal(a[..., 0], g[..., j]), (name, j, nm)


@pytest.mark.gpu
def test_a_literal_has_the_same_bits_alone_and_among_others():
    for name in ("3-17-33-4", "64-64-64-64"):
        cs = case(name)
        _, together, _ = gpu(name, 17)
        for i in range(17):
            *_, alone = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="gpu", normals=cs["C"][[i]])
            for nm, a, g in zip(LIT_NAMES, alone, together):
                assert np.array_equal(a[0], g[i]), (name, i, nm)


@pytest.mark.gpu
def test_kernel_time_is_reported():
    assert gpu("3-17-33-4", 17)[2] > 0.0


def _raw(xdims, M, activ, nbox, lo, hi, nlit, normals, one_box=False):
    lib = _lib.load()
    xd = np.asarray(xdims, dtype=np.int32)
    dp = _lib.c_double_p
    p = lambda a: None if a is None else a.ctypes.data_as(dp)
    if one_box:
        rc = lib.nnsdp_make_intervals_lits(len(xdims) - 1, xd.ctypes.data_as(_lib.c_int32_p), p(M), activ, p(lo), p(hi),
                                           None, None, None, None, None, None, None, None, nlit, p(normals), None, None, None, None)
    else:
        rc = lib.nnsdp_make_intervals_batch_lits(len(xdims) - 1, xd.ctypes.data_as(_lib.c_int32_p), p(M), activ, nbox, p(lo), p(hi),
                                                 None, None, None, None, None, None, nlit, p(normals), None, None, None, None, None)
    return rc, lib.nnsdp_last_error().decode()


def _refusals():
    M3 = np.zeros(3 * 3 + 2 * 4)                      # a 2-3-2 network: [W0 b0] 3 x 3, [W1 b1] 2 x 4
    lo, hi = np.zeros((4, 2)), np.ones((4, 2))        # 4 boxes: n0 x nbox column-major is one row of this array per box
    nrm = np.ones((3, 2))                             # 3 literals: ny x nlit column-major is one row per literal
    for one_box in (False, True):
        rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, hi, -1, nrm, one_box)
        assert rc < 0 and "nlit" in msg
        rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, hi, 65, np.ones((65, 2)), one_box)
        assert rc < 0 and "nlit" in msg and "64" in msg
        rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, hi, 3, None, one_box)
        assert rc < 0 and "normals" in msg
        for bad in (np.nan, np.inf):
            nb = nrm.copy()
            nb[2, 1] = bad
            rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, hi, 3, nb, one_box)
            assert rc < 0 and "literal 2" in msg and "finite" in msg
    # as today: Tanh and a width above 64 (batch entry), and the bad box is still named with literals present
    rc, msg = _raw([2, 3, 2], M3, 1, 4, lo, hi, 3, nrm)
    assert rc < 0 and "Tanh" in msg
    rc, msg = _raw([2, 65, 2], np.zeros(65 * 3 + 2 * 66), 0, 4, lo, hi, 3, nrm)
    assert rc < 0 and "65" in msg and "64" in msg
    for widths in ([2, 0, 2], [0, 65, 2]):             # an empty layer; the first bad width is the one named
        rc, msg = _raw(widths, M3, 0, 4, lo, hi, 3, nrm)
        assert rc < 0 and "layer widths must be >= 1" in msg
    bad = hi.copy()
    bad[2, 1] = -1.0
    rc, msg = _raw([2, 3, 2], M3, 0, 4, lo, bad, 3, nrm)
    assert rc < 0 and "box 2" in msg
    assert _raw([2, 3, 2], M3, 0, 0, None, None, 3, nrm)[0] == 0          # nbox = 0: nothing to do
    # the one-box entry needs no GPU: it runs
    assert _raw([2, 3, 2], M3, 0, 1, lo[0], hi[0], 3, nrm, one_box=True)[0] == 0
    assert _raw([2, 3, 2], M3, 0, 1, lo[0], hi[0], 0, None, one_box=True)[0] == 0


def test_literal_entries_reject_bad_arguments_without_a_gpu():
    _refusals()


@pytest.mark.gpu
def test_refusals_name_the_fact():
    _refusals()
    net = random_net([2, 3, 2], 1)
    lo, hi = np.zeros((2, 3)), np.ones((2, 3))
    with pytest.raises(ValueError):
        na.makeIntervalsBatch(net, lo, hi, backend="gpu", normals=np.ones((2, 3)))
    with pytest.raises(_lib.NnsdpError, match="nlit"):
        na.makeIntervalsBatch(net, lo, hi, backend="gpu", normals=np.ones((65, 2)))
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    with pytest.raises(_lib.NnsdpError, match="Tanh"):
        na.makeIntervalsBatch(tanh, lo, hi, backend="gpu", normals=np.ones((1, 2)))
    *six, lits = na.makeIntervalsBatch(net, lo[:, :0], hi[:, :0], backend="gpu", normals=np.ones((2, 2)))
    assert lits.smax.shape == (2, 0) and lits.A.shape == (2, 2, 0)
