"""The wide resident CROWN bounder (CrownBounder(max_width=128), csrc/crown_wide.hpp k_crown_wide) on the GPU: on a network of widths
<= 64 it has the bits of the narrow instance; on hidden layers up to 128 wide it is held against the numpy recurrences (R(longdouble)
the oracle, |R(float64) - R(longdouble)| the yardstick, the formula and margin of tests/test_crown_batch_gpu.py and, for Tanh, of
tests/test_crown_resident_gpu.py), against the float32 host routine and against sampled points; a box's bits depend neither on its
position nor on its company; both frontiers of the split driver walk the same tree on it; the handle keeps its buffers."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import crown_tanh_common as tc
import crown_wide_common as wc
import literal_common as lc
import reach_common as rc
from test_split_resident_gpu import assert_same_tree

pytestmark = pytest.mark.gpu
ALL = lc.NAMES + lc.LIT_NAMES
EPS = 2.0 ** -52
OPTS = na.AdmmSdpOptions()
_cache = {}


def wide(name, activ, nbox, nlit):
    """the wide bounder's arrays on the first nbox boxes and nlit literal rows of a case; the full call of a case is made once"""
    key = (name, activ, nbox, nlit)
    if key not in _cache:
        cs = wc.case(name, activ)
        with na.CrownBounder(cs["net"], cs["C"][:nlit] if nlit else None, max_width=128) as bd:
            assert bd.max_width == 128
            _cache[key] = tc.flat(bd.bound(cs["lo"][:, :nbox], cs["hi"][:, :nbox]))
    return _cache[key]


# ----------------------------------------------------------------------------- 1. the bits of the narrow instance
@pytest.mark.parametrize("nlit", [0, 7, 64])
@pytest.mark.parametrize("activ", ["relu", "tanh"])
@pytest.mark.parametrize("name", ["3-64-64-3", "W10-D5"])
def test_a_narrow_network_gets_the_bits_of_the_narrow_instance(name, activ, nlit):
    if name == "W10-D5":
        net = lc.fixture_net()
        lo, hi = lc.boxes(net.xdims[0], wc.NBOX, 77)
        Cm = lc.literal_rows(net.xdims[-1], 64, 78)
    else:
        cs = wc.case(name)
        net, lo, hi, Cm = cs["net"], cs["lo"], cs["hi"], cs["C"]
    if activ == "tanh":
        net = tc.tanh_copy(net)
    Cn = Cm[:nlit] if nlit else None
    X = np.random.default_rng(9).normal(size=(net.xdims[0], 37))
    with na.CrownBounder(net, Cn) as narrow, na.CrownBounder(net, Cn, max_width=128) as wd:
        assert (narrow.max_width, wd.max_width) == (64, 128)
        for nbox in (wc.NBOX, 1, 3):
            a, b = tc.flat(narrow.bound(lo[:, :nbox], hi[:, :nbox])), tc.flat(wd.bound(lo[:, :nbox], hi[:, :nbox]))
            assert len(a) == len(b) == (10 if nlit else 6)
            for nm, x, y in zip(ALL, a, b):
                assert x.shape == y.shape and np.array_equal(x, y), (name, activ, nlit, nbox, nm)
        assert np.array_equal(narrow.eval(X), wd.eval(X))


# ----------------------------------------------------------------------------- 2. accuracy against the numpy recurrences
@pytest.mark.parametrize("nlit", [0, 1, 7, 64])
@pytest.mark.parametrize("nbox", [1, 3, 6])
@pytest.mark.parametrize("name", list(wc.SHAPES))
def test_relu_against_the_numpy_recurrences(name, nbox, nlit):
    """|GPU - R(longdouble)| <= max(8 r, 64 * 2^-52 * s) per array, r = max |R(float64) - R(longdouble)| and s = max |value| of that array
    over the call: the formula and margin of tests/test_crown_batch_gpu.py.  Prints err / max(r, 8 * 2^-52 s) per array (8 is the limit)."""
    cs = wc.case(name)
    got = wide(name, "relu", nbox, nlit)
    assert len(got) == (10 if nlit else 6)
    for nm, g, a64, ald in zip(ALL, got, wc.cut(cs["r64"], nbox, nlit), wc.cut(cs["rld"], nbox, nlit)):
        assert g.shape == a64.shape, nm
        r, s, err = float(np.abs(a64 - ald).max()), float(np.abs(ald).max()), float(np.abs(g - ald).max())
        tol = max(8.0 * r, 64.0 * EPS * s)
        ratio = err / max(r, 8.0 * EPS * s) if max(r, s) > 0 else 0.0
        print(f"relu {name} nbox={nbox} nlit={nlit} {nm}: err {err:.3e}  r {r:.3e}  s {s:.3e}  tol {tol:.3e}  ratio {ratio:.3f}")
        assert np.all(np.isfinite(g)), nm
        assert err <= tol, (name, nbox, nlit, nm, err, tol)


@pytest.mark.parametrize("nlit", [0, 1, 7, 64])
@pytest.mark.parametrize("nbox", [1, 3, 6])
@pytest.mark.parametrize("name", wc.TANH)
def test_tanh_against_the_numpy_recurrences(name, nbox, nlit):
    """as above with R_tanh and the two-term yardstick of tests/test_crown_resident_gpu.py: r = max |R_tanh(float64) - R_tanh(longdouble)|
    + max |R_tanh(float64, tanh and cosh moved by one ulp) - R_tanh(longdouble)|"""
    cs = wc.case(name, "tanh")
    got = wide(name, "tanh", nbox, nlit)
    assert len(got) == (10 if nlit else 6)
    for nm, g, a64, ald, amv in zip(ALL, got, wc.cut(cs["r64"], nbox, nlit), wc.cut(cs["rld"], nbox, nlit), wc.cut(cs["rmv"], nbox, nlit)):
        assert g.shape == a64.shape, nm
        r = float(np.abs(a64 - ald).max() + np.abs(amv - ald).max())
        s, err = float(np.abs(ald).max()), float(np.abs(g - ald).max())
        tol = max(8.0 * r, 64.0 * EPS * s)
        ratio = err / max(r, 8.0 * EPS * s) if max(r, s) > 0 else 0.0
        print(f"tanh {name} nbox={nbox} nlit={nlit} {nm}: err {err:.3e}  r {r:.3e}  s {s:.3e}  tol {tol:.3e}  ratio {ratio:.3f}")
        assert np.all(np.isfinite(g)), nm
        assert err <= tol, (name, nbox, nlit, nm, err, tol)


# ----------------------------------------------------------------------------- 3. the float32 host routine
def test_agrees_with_the_float32_host_routine():
    """the host routine computes in float32 by design and takes any width: max |GPU - host| / (1 + |v|) over the wide ReLU nets stays
    within twice the figure max |R(float64) - host| / (1 + |v|), measured without the kernel (tests/test_crown_wide_cpu.py) and
    recomputed here - the margin of the narrow tests, with the figure of these nets (the float32 sums of a 128-wide layer are longer).
    ReLU only: on these boxes the float32 tangent grid of the host's Tanh routine moves its bounds by a whole grid step (3e-2 against
    R_tanh(float64), the effect tests/crown_tanh_common.py describes), which is no yardstick for an fp64 kernel"""
    figure = wc.host_figure()
    gpu = max(tc.rel_err(g, h) for name in wc.WIDE for g, h in zip(wide(name, "relu", wc.NBOX, 7), wc.host(name)))
    print(f"max |R(float64) - host| / (1 + |v|) = {figure:.3e} (recorded {wc.HOST_FLOAT32_FIGURE_WIDE:.3e});  max |GPU - host| / (1 + |v|) = {gpu:.3e}")
    assert 0.0 < figure < 1e-4
    assert gpu <= 2.0 * figure


# ----------------------------------------------------------------------------- 4. soundness
@pytest.mark.parametrize("activ", ["relu", "tanh"])
def test_literal_bounds_are_sound_on_sampled_points(activ):
    cs = wc.case("3-65-128-66-4", activ)
    got = wide("3-65-128-66-4", activ, wc.NBOX, 7)
    lc.assert_literals_sound(cs["net"], cs["lo"], cs["hi"], cs["C"][:7], na.LiteralBounds(*got[6:]), 1e-9)


# ----------------------------------------------------------------------------- 5. position and company
@pytest.mark.parametrize("activ", ["relu", "tanh"])
def test_a_box_has_the_same_bits_alone_elsewhere_and_among_other_literals(activ):
    name = "3-65-128-66-4"
    cs, full = wc.case(name, activ), wide(name, activ, wc.NBOX, 7)
    with na.CrownBounder(cs["net"], cs["C"][:7], max_width=128) as bd:
        for j in (0, 1, 5):
            one = tc.flat(bd.bound(cs["lo"][:, [j]], cs["hi"][:, [j]]))                     # alone
            for nm, a, g in zip(ALL, one, full):
                assert np.array_equal(a[..., 0], g[..., j]), (activ, j, nm)
        order = np.array([4, 2, 5, 0, 1, 3])
        moved = tc.flat(bd.bound(cs["lo"][:, order], cs["hi"][:, order]))                   # at another position
        for nm, a, g in zip(ALL, moved, full):
            assert np.array_equal(a, g[..., order]), (activ, nm)
    for i in (0, 3, 6):
        with na.CrownBounder(cs["net"], cs["C"][[i]], max_width=128) as bd:                # without the other literals
            alone = tc.flat(bd.bound(cs["lo"], cs["hi"]))
        for nm, a, g in zip(ALL[:6], alone, full):
            assert np.array_equal(a, g), (activ, i, nm)
        for nm, a, g in zip(lc.LIT_NAMES, alone[6:], full[6:]):
            assert np.array_equal(a[0], g[i]), (activ, i, nm)
    among = wide(name, activ, wc.NBOX, 64)                                                  # among 64
    for nm, a, g in zip(ALL, among, full):
        assert np.array_equal(a[:7] if nm in lc.LIT_NAMES else a, g), (activ, nm)


# ----------------------------------------------------------------------------- 6. the two frontiers
@pytest.mark.parametrize("threshold", list(wc.THRESHOLDS))
@pytest.mark.parametrize("name", list(wc.INSTANCES))
def test_verify_split_walks_the_same_tree_on_both_frontiers(name, threshold):
    it = wc.instance(name)
    rule, verdict = wc.THRESHOLDS[threshold]
    lits = [(it["normal"], rule(it["s"], it["c0"]))]
    opt = dict(sdp_per_level=0, literal_bounds=True, max_boxes=512)
    run = lambda **kw: na.verifySplit(it["net"], it["lo"], it["hi"], lits, 0, OPTS, na.SplitOptions(**opt, **kw))
    host = run(crown_backend="resident", crown_max_width=128)
    dev = run(crown_backend="resident", crown_max_width=128, frontier="device")
    f32 = run(crown_backend="host")
    print(f"{name} {threshold}: {host.verdict} after {host.visited} boxes (float32 host routine: {f32.verdict} after {f32.visited})")
    assert host.verdict == dev.verdict == f32.verdict == verdict
    assert_same_tree(host, dev)
    lc.assert_tiles(dev.leaves, it["lo"], it["hi"])


@pytest.mark.parametrize("name", list(wc.INSTANCES))
def test_reach_split_walks_the_same_tree_on_both_frontiers(name):
    it = wc.instance(name)
    Cn, tol = it["normal"][None], 0.25 * (it["c0"] - it["s"])
    opt = dict(crown_backend="resident", crown_max_width=128, sdp_per_level=0, max_boxes=512)
    host = na.reachSplit(it["net"], it["lo"], it["hi"], Cn, tol, split=na.SplitOptions(**opt))
    dev = na.reachSplit(it["net"], it["lo"], it["hi"], Cn, tol, split=na.SplitOptions(frontier="device", **opt))
    print(f"{name}: {host.status} after {host.visited} boxes, [{host.lower[0]:.6f}, {host.upper[0]:.6f}], sampled maximum {it['s']:.6f}")
    rc.assert_same_reach(host, dev)
    assert host.visited > 1 and host.lower[0] <= host.upper[0] and host.upper[0] >= it["s"] - 1e-9 * (1.0 + abs(it["s"]))


# ----------------------------------------------------------------------------- 7. housekeeping
def test_a_wide_handle_keeps_its_buffers_and_its_bits_across_entries():
    it = wc.instance("2-100-100-2")
    h = it["s"] + 0.1 * (it["c0"] - it["s"])
    lo, hi = np.stack([it["lo"], 0.5 * it["lo"]], axis=1), np.stack([it["hi"], 0.25 * it["hi"]], axis=1)
    skw = dict(literal_bounds=True, max_boxes=64)
    rkw = dict(max_boxes=64)
    with na.CrownBounder(it["net"], it["normal"][None], max_width=128) as bd:
        i0 = bd.info()
        assert i0["network_uploads"] == 1 and i0["bound_calls"] == 0
        b0 = tc.flat(bd.bound(lo, hi))
        s0 = bd.search(it["lo"], it["hi"], np.array([h]), **skw)
        r0 = bd.reach(it["lo"], it["hi"], 0.5 * (it["c0"] - it["s"]), **rkw)
        i1 = bd.info()
        r1 = bd.reach(it["lo"], it["hi"], 0.5 * (it["c0"] - it["s"]), **rkw)
        b1 = tc.flat(bd.bound(lo, hi))
        s1 = bd.search(it["lo"], it["hi"], np.array([h]), **skw)
        b2 = tc.flat(bd.bound(lo, hi))
        i2 = bd.info()
        assert (i2["device_allocations"], i2["network_uploads"], i2["device_bytes"], i2["box_capacity"]) == \
               (i1["device_allocations"], 1, i1["device_bytes"], i1["box_capacity"])
        assert bd.max_width == 128
        for a, b, c in zip(b0, b1, b2):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert (s0["verdict"], s0["visited"], s0["depth"]) == (s1["verdict"], s1["visited"], s1["depth"])
        for k in ("lo", "hi", "leaf_depth", "proved", "literal", "bound"):
            assert np.array_equal(s0[k], s1[k]), k
        assert (r0["status"], r0["visited"]) == (r1["status"], r1["visited"])
        for k in ("lo", "hi", "leaf_depth", "closed", "bound", "incumbent", "witnesses"):
            assert np.array_equal(r0[k], r1[k]), k
        # optimised slopes: refused by the frontend before the library, and by the library with its message
        with pytest.raises(ValueError, match="wide bounder"):
            bd.bound(lo, hi, alpha_steps=2)
        dp = _lib.c_double_p
        loc, hic = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)
        code = bd._lib.nnsdp_crown_bound_alpha(bd._handle(), 2, loc.ctypes.data_as(dp), hic.ctypes.data_as(dp), *[None] * 11, 2, 0.5, 0.9,
                                              *[None] * 6)
        assert code == -1 and "wide bounder" in bd._lib.nnsdp_last_error().decode()
        assert bd.info()["device_allocations"] == i2["device_allocations"]
        for a, b in zip(b0, tc.flat(bd.bound(lo, hi))):
            assert np.array_equal(a, b)
