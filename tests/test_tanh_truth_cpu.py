"""The Tanh relaxation against tests/tanh_truth.py, without a GPU: the reference checks itself, then the float32 host routine and the
numpy restatement (crown_tanh_common.relax / R_tanh, which restates the kernel's arithmetic in float64) are held to it on the one-neuron
interval set and on the two network-level cases of tests/tanh_truth_common.py, and the fixture tests/golden/tanh_ranges.json is
checked against its generator.  The GPU kernels meet the same checks in tests/test_tanh_truth_gpu.py."""
import importlib.util
import os

import mpmath
import numpy as np

import crown_tanh_common as tc
import exact_common as ec
import helpers
import nnsdp_amd as na
import tanh_truth as tt
import tanh_truth_common as th


# ----------------------------------------------------------------------------- 1. the reference checks itself
def test_the_enclosure_brackets_a_grid_maximum_on_a_1_4_1_net():
    rng = np.random.default_rng(11)
    Ms = [rng.normal(size=(4, 2)) * np.array([3.0, 1.0]), rng.normal(size=(1, 5))]
    lo, hi, c = np.array([-1.0]), np.array([1.0]), np.array([1.0])
    ld = np.longdouble
    x = np.arange(-1000000, 1000001).astype(ld) / ld(1000000)
    h = np.tanh(Ms[0][:, :1].astype(ld) * x[None, :] + Ms[0][:, 1:].astype(ld))
    y = (Ms[1][:, :-1].astype(ld) @ h)[0] + ld(Ms[1][0, -1])
    for sign in (1.0, -1.0):
        grid = float((sign * y).max())
        xs, w = tt.attained_max(Ms, lo, hi, sign * c)
        e = tt.enclosed_max(Ms, lo, hi, sign * c, w, 1e-6)
        print(f"1-4-1 sign {sign:+.0f}: grid maximum {grid:.12f}, w {w:.12f} at {xs}, v {e.v:.12f}, gap {e.gap:.3e}, {e.boxes} boxes")
        assert lo[0] <= xs[0] <= hi[0] and e.gap <= 1e-6
        assert w <= e.v and grid <= e.v + 1e-15 and w >= grid - 1e-6 * (1.0 + abs(e.v))
        tight = tt.enclosed_max(Ms, lo, hi, sign * c, w, 1e-12)
        assert tight.gap <= 1e-12 and w <= tight.v <= e.v and grid <= tight.v + 1e-15


def test_line_gap_of_a_tangent_is_zero_and_of_a_wrong_line_is_positive():
    for x0, l, u in ((0.3, 0.0, 2.0), (1.7, 0.5, 40.0), (-0.4, -3.0, 0.0), (-2.0, -600.0, -1.0), (0.0, 0.0, 0.0)):
        k, c = tt.tangent(x0)
        g = tt.line_gap(k, c, l, u, "upper" if x0 >= 0 else "lower")      # concave on x >= 0: the tangent is an upper line there
        assert abs(g) <= mpmath.mpf(10) ** -30, (x0, g)
    # a chord of the concave side is a lower line; shifted up by 1e-9 it is violated by exactly that at both ends
    with mpmath.workdps(tt.DPS):
        l, u = mpmath.mpf("0.25"), mpmath.mpf("1.5")
        k = (mpmath.tanh(u) - mpmath.tanh(l)) / (u - l)
        c = mpmath.tanh(l) - k * l
        assert abs(tt.line_gap(k, c, l, u, "lower")) <= mpmath.mpf(10) ** -30
        assert abs(tt.line_gap(k, c + mpmath.mpf("1e-9"), l, u, "lower") - mpmath.mpf("1e-9")) <= mpmath.mpf(10) ** -30
        assert tt.line_gap(k, c, l, u, "upper") > mpmath.mpf("0.01")          # the chord is no upper line: violated inside, at the stationary point
    # the library's l = u = 0 lines and its clamped lower line on [-600, 600], as doubles
    assert tt.line_gap(1.00002, 8.333e-8, 0.0, 0.0, "lower") > 8e-8 and tt.line_gap(1.00002, -8.333e-8, 0.0, 0.0, "upper") > 8e-8
    assert tt.line_gap(0.0039685, -0.98430, -600.0, 600.0, "lower") > 0.39
    assert tt.line_gap(0.0, -1.0, -600.0, 600.0, "lower") <= 0 and tt.line_gap(0.0, 1.0, -600.0, 600.0, "upper") <= 0


# ----------------------------------------------------------------------------- 2. the host routine on the interval set
def host_box(l, u):
    """the float32 host routine takes the box as float32, where +-1e300 is not finite: that one interval is given as +-1e38, the largest
    decade whose width float32 still holds; every other interval is the set's, and the lines are checked on the caller's doubles"""
    big = np.abs(l) > 1e38
    return np.where(big, np.sign(l) * 1e38, l), np.where(np.abs(u) > 1e38, np.sign(u) * 1e38, u)


def test_the_host_routine_on_the_interval_set():
    """slack 64 * 2^-23 (1 + |w| max(|l|, |u|)): the project's margin of 64 roundings, for float32"""
    l, u, names = th.interval_set()
    l, u = host_box(l, u)
    net, C = th.one_neuron()
    res = na.makeIntervalsBatch(net, l[None, :], u[None, :], backend="host", normals=C)
    th.check_ends("host", (("acy", res[0][0], res[1][0]), ("y", res[4][0], res[5][0])), l, u, th.EPS32)
    th.check_lines("host", *th.lines_of(res), l, u, names, th.EPS32)


# ----------------------------------------------------------------------------- 3. the numpy restatement
def test_the_numpy_restatement_on_the_interval_set():
    l, u, names = th.interval_set()
    lw, lb, uw, ub, _ = tc.relax(l.copy(), u.copy(), np.float64)
    th.check_lines("relax(float64)", lw, lb, uw, ub, l, u, names, th.EPS64)
    net, C = th.one_neuron()
    r = tc.R_tanh(net.Ms, l[None, :], u[None, :], np.float64, C)
    th.check_ends("R_tanh(float64)", (("acy", r[0][0], r[1][0]), ("y", r[4][0], r[5][0])), l, u, th.EPS64)
    th.check_lines("R_tanh(float64)", -r[8][1, 0], -r[9][1], r[8][0, 0], r[9][0], l, u, names, th.EPS64)


# ----------------------------------------------------------------------------- 4. the two network-level cases
def restated(net, lo, hi):
    r = tc.R_tanh(net.Ms, lo[:, None], hi[:, None], np.float64, th.NORMALS_1)
    return r[:6] + (na.LiteralBounds(*r[6:]),)


def entries(net, lo, hi):
    return (("host", na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="host", normals=th.NORMALS_1), th.EPS32),
            ("R_tanh(float64)", restated(net, lo, hi), th.EPS64))


def test_a_neuron_with_a_zero_weight_row_and_bias():
    net, lo, hi = th.dead_neuron()
    for label, res, eps in entries(net, lo, hi):
        th.check_contains(f"dead neuron, {label}", net, res, np.linspace(-1.0, 1.0, 9)[None, :], eps)


def test_a_point_box_at_the_origin_of_a_bias_free_net():
    net, lo, hi = th.origin_point()
    for label, res, eps in entries(net, lo, hi):
        th.check_contains(f"origin, {label}", net, res, np.zeros((1, 1)), eps)


def test_pre_activations_beyond_the_clamp():
    net, lo, hi = th.clamp_net()
    for label, res, eps in entries(net, lo, hi):
        th.check_clamp(f"clamp, {label}", res, eps)


# ----------------------------------------------------------------------------- the fixture and its generator
def test_the_thresholds_of_the_verdict_tests_are_decidable():
    """the numpy restatement of the driver on R_tanh decides h = v + d and h = w - d (tests/test_tanh_truth_gpu.py: thresholds) within
    the 1 024 boxes those tests allow: 25 and 1 boxes on 2-8-8-2, 113 and 79 on 3-10-10-3; d is at least ten recorded gaps"""
    for name in ec.SMALL:
        cs = th.fixture_case(name)
        root = cs["boxes"][0]
        v, w, gap = float(root["v"][0]), float(root["w"][0]), float(root["gap"][0])
        d = max(1e-4, 10.0 * gap * (1.0 + abs(v)))
        up = th.decide(cs["net"], root["lo"], root["hi"], cs["C"][0], v + d)
        down = th.decide(cs["net"], root["lo"], root["hi"], cs["C"][0], w - d)
        print(f"{name}: d {d:.3e}: h = v + d {up}, h = w - d {down}")
        assert up[0] == "holds" and down[0] == "violated" and max(up[1], down[1]) <= 1024 and d >= 10.0 * gap * (1.0 + abs(v))


def generator():
    spec = importlib.util.spec_from_file_location("make_tanh_ranges", os.path.join(helpers.GOLDEN, "make_tanh_ranges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_is_what_its_generator_writes():
    """the generator's restated recipes are the product's nets and rows bit for bit; every row has w <= v, its x inside the box, its w
    the long-double value at x to 1e-15 and its gap as recorded; the point boxes and one root row regenerate to 1e-12"""
    gen = generator()
    for name in ec.SMALL:
        cs = th.fixture_case(name)
        assert all(np.array_equal(a, b) for a, b in zip(gen.net_Ms(name), cs["net"].Ms)) and np.array_equal(gen.rows(name), cs["C"])
        have = {bx["name"]: bx for bx in ec.case(name)["boxes"]}
        for bx in cs["boxes"]:
            assert np.array_equal(bx["lo"], have[bx["name"]]["lo"]) and np.array_equal(bx["hi"], have[bx["name"]]["hi"])
            assert bx["w"].shape == bx["v"].shape == bx["gap"].shape == (len(cs["C"]),) and np.all(bx["w"] <= bx["v"])
            assert np.all(bx["x"] >= bx["lo"]) and np.all(bx["x"] <= bx["hi"])
            assert np.all(bx["gap"] <= 1e-6) and np.allclose(bx["gap"], (bx["v"] - bx["w"]) / (1.0 + np.abs(bx["v"])), rtol=0, atol=1e-15)
            for c, x, w in zip(cs["C"], bx["x"], bx["w"]):
                assert abs(float(c.astype(np.longdouble) @ tt.forward_ld(cs["net"].Ms, x)) - w) <= 1e-15
            rows = range(len(cs["C"])) if bx["name"] == "point" else ((0,) if bx["name"] == "root" else ())
            for i in rows:
                x, w = tt.attained_max(cs["net"].Ms, bx["lo"], bx["hi"], cs["C"][i])
                e = tt.enclosed_max(cs["net"].Ms, bx["lo"], bx["hi"], cs["C"][i], w, gen.GAP)
                assert abs(w - bx["w"][i]) <= 1e-12 and abs(e.v - bx["v"][i]) <= 1e-12, (name, bx["name"], i)
