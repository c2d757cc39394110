"""The Tanh instances of the CROWN kernels (k_crown_resident and k_crown_wide with kCbTanh, cb_tanh_relax of csrc/crown_batch.hpp) and
the searches on top of them against tests/tanh_truth.py, which owes nothing to the product's arithmetic.

One neuron per box: on the 1-1-1 net y = tanh(x) the box is the neuron's interval and the literal outputs are the relaxation's two
lines; tanh_truth.line_gap gives their exact worst violation over the caller's box, and the interval set of tests/tanh_truth_common.py
holds the smallest cases at which this code can go wrong.  Then the two network-level cases (a neuron whose interval is [0, 0],
pre-activations beyond +-500) and the enclosed maxima of tests/golden/tanh_ranges.json under bound, reachSplit, verifySplit and
search_many."""
import numpy as np
import pytest

import nnsdp_amd as na
import exact_common as ec
import reach_common as rc
import tanh_truth as tt
import tanh_truth_common as th

pytestmark = pytest.mark.gpu
WIDTHS = (64, 128)
_cache = {}


def bound(net, C, lo, hi, max_width):
    with na.CrownBounder(net, C, max_width=max_width) as bd:
        return bd.bound(lo, hi)


def same_bits(a, b, what):
    a, b = tuple(a[:6]) + tuple(a[6]), tuple(b[:6]) + tuple(b[6])
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


# ----------------------------------------------------------------------------- one neuron per box
def one_neuron_result(max_width):
    if max_width not in _cache:
        l, u, _ = th.interval_set()
        net, C = th.one_neuron()
        _cache[max_width] = bound(net, C, l[None, :], u[None, :], max_width)
    return _cache[max_width]


def test_both_lines_hold_on_every_interval_of_the_set():
    """line_gap <= 64 * 2^-52 (1 + |w| max(|l|, |u|)) for both lines, on the caller's box [l, u]; acymin <= tanh(l), acymax >= tanh(u)
    and the same for ymin / ymax.  All 2 300 intervals are one bound call."""
    l, u, names = th.interval_set()
    res = one_neuron_result(64)
    th.check_ends("resident", (("acy", res[0][0], res[1][0]), ("y", res[4][0], res[5][0])), l, u, th.EPS64)
    th.check_lines("resident", *th.lines_of(res), l, u, names, th.EPS64)


def test_the_wide_kernel_gives_the_same_bits_on_one_neuron():
    same_bits(one_neuron_result(64), one_neuron_result(128), "1-1-1, max_width 128 against 64")


def test_rows_beyond_the_first_slab_of_the_wide_kernel():
    """the 1-100-64 selection net: 100 intervals of the set from one box, 64 of their lines exposed, rows of 64 and above among them"""
    net, C, sel, _ = th.selection_net()
    assert (sel >= 64).any()
    res = bound(net, C, -np.ones((1, 1)), np.ones((1, 1)), 128)
    th.check_selection("wide, 1-100-64", res)


@pytest.mark.parametrize("max_width", WIDTHS)
def test_a_neuron_with_a_zero_weight_row_and_bias(max_width):
    net, lo, hi = th.dead_neuron()
    res = bound(net, th.NORMALS_1, lo[:, None], hi[:, None], max_width)
    th.check_contains(f"dead neuron, max_width {max_width}", net, res, np.linspace(-1.0, 1.0, 9)[None, :], th.EPS64)


@pytest.mark.parametrize("max_width", WIDTHS)
def test_a_point_box_at_the_origin_of_a_bias_free_net(max_width):
    net, lo, hi = th.origin_point()
    res = bound(net, th.NORMALS_1, lo[:, None], hi[:, None], max_width)
    th.check_contains(f"origin, max_width {max_width}", net, res, np.zeros((1, 1)), th.EPS64)


@pytest.mark.parametrize("max_width", WIDTHS)
def test_pre_activations_beyond_the_clamp(max_width):
    net, lo, hi = th.clamp_net()
    th.check_clamp(f"clamp, max_width {max_width}", bound(net, th.NORMALS_1, lo[:, None], hi[:, None], max_width), th.EPS64)


# ----------------------------------------------------------------------------- the fixture: bound
NAMES = tuple(ec.SMALL)


def stacked(cs, key):
    return np.stack([bx[key] for bx in cs["boxes"]], axis=-1)


@pytest.mark.parametrize("max_width", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_bound_respects_every_attained_value(name, max_width):
    """per box and row: smax >= w - slack and A' x* + b0 >= w - slack (the upper line at the point where w is attained), smin <= w +
    slack; the hidden and output intervals contain the long-double forward pass at every x*.  slack = 8 r + 64 * 2^-52 s per array
    (tanh_truth_common.fixture_slack, from two CPU runs); for A' x* + b0 it is slack_A |x*|_1 + slack_b0."""
    cs = th.fixture_case(name)
    lo, hi = stacked(cs, "lo"), stacked(cs, "hi")
    w, X = stacked(cs, "w"), stacked(cs, "x")                     # nrow x nbox, nrow x n0 x nbox
    slack = th.fixture_slack(cs, lo, hi)
    acymin, acymax, _, _, ymin, ymax, lits = bound(cs["net"], cs["C"], lo, hi, max_width)
    line = np.einsum("iqb,iqb->ib", lits.A, X) + lits.b0
    line_slack = slack["A"] * np.abs(X).sum(axis=1) + slack["b0"]
    print(f"{name} max_width {max_width}: worst (w - smax) / slack {np.max((w - lits.smax) / slack['smax']):+.3e}, "
          f"worst (w - line) / slack {np.max((w - line) / line_slack):+.3e}, smallest smax - w {np.min(lits.smax - w):.3e}; "
          f"slack of smax per box {slack['smax']}")
    assert np.all(lits.smax >= w - slack["smax"]) and np.all(lits.smin <= w + slack["smin"])
    assert np.all(line >= w - line_slack)
    for b in range(lo.shape[1]):
        for x in X[:, :, b]:
            y, hid = tt.forward_ld(cs["net"].Ms, x, hidden=True)
            h = np.concatenate(hid)
            assert np.all(acymin[:, b] <= h + slack["acymin"][b]) and np.all(acymax[:, b] >= h - slack["acymax"][b]), (name, b)
            assert np.all(ymin[:, b] <= y + slack["ymin"][b]) and np.all(ymax[:, b] >= y - slack["ymax"][b]), (name, b)


# ----------------------------------------------------------------------------- the fixture: reach
def root_of(name):
    cs = th.fixture_case(name)
    root = cs["boxes"][0]
    assert root["name"] == "root"
    slack = th.fixture_slack(cs, root["lo"][:, None], root["hi"][:, None])
    return cs, root, float(max(slack["smax"][0], slack["ymax"][0]))


@pytest.mark.parametrize("name", NAMES)
def test_both_frontiers_enclose_the_maxima(name):
    """upper >= w - slack, lower <= v + slack, and once converged upper <= v + tol + slack; the device frontier gives the host
    frontier's result bit for bit.  (With the float32 host backend the two trees converge after 103 and 341 boxes.)"""
    cs, root, slack = root_of(name)
    opt = dict(crown_backend="resident", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP, max_depth=64)
    host = na.reachSplit(cs["net"], root["lo"], root["hi"], cs["C"], rc.TOL, split=na.SplitOptions(**opt))
    dev = na.reachSplit(cs["net"], root["lo"], root["hi"], cs["C"], rc.TOL, split=na.SplitOptions(frontier="device", **opt))
    for label, res in (("host", host), ("device", dev)):
        rc.check_enclosure(f"tanh {name} {label}", res, root["w"], root["v"], slack, rc.TOL, root["lo"], root["hi"])
        assert res.status == "converged" and np.all(res.upper <= root["v"] + rc.TOL + slack)
    rc.assert_same_reach(host, dev)


# ----------------------------------------------------------------------------- the fixture: verdicts
# The literal is row 0 of the stored rows, y_0 - y_last, on the root box.  d = max(1e-4, 10 gap (1 + |v|)) with the row's recorded gap.
# The numpy restatement of the driver on R_tanh (tanh_truth_common.decide) answers  h = v + d  with "holds" after 25 boxes (2-8-8-2) and
# 113 boxes (3-10-10-3), and  h = w - d  with "violated" after 1 and 79 boxes; tests/test_tanh_truth_cpu.py holds it to max_boxes.
MAX_BOXES = 1024


def thresholds(root, i=0):
    v, w, gap = float(root["v"][i]), float(root["w"][i]), float(root["gap"][i])
    d = max(1e-4, 10.0 * gap * (1.0 + abs(v)))
    return w - d, v + d, d


def check_verdict(label, res_verdict, witness, cs, root, h, truth):
    print(f"{label}: h {h:.10f}: {res_verdict}")
    assert res_verdict != ("holds" if truth == "violated" else "violated"), (label, "a false verdict")
    if res_verdict == "violated":
        assert np.all(witness >= root["lo"]) and np.all(witness <= root["hi"])
        assert tt.value_mp(cs["net"].Ms, witness, cs["C"][0]) > h


@pytest.mark.parametrize("frontier", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_verdicts_on_either_side_of_the_maximum(name, frontier):
    """h = w - d: never "holds", and "violated" with corner_points; h = v + d: never "violated", and "holds" within max_boxes"""
    cs, root, _ = root_of(name)
    below, above, _ = thresholds(root)
    for h, truth, corner_points in ((below, "violated", True), (below, "violated", False), (above, "holds", True), (above, "holds", False)):
        res = na.verifySplit(cs["net"], root["lo"], root["hi"], [(cs["C"][0], h)], 0, na.AdmmSdpOptions(),
                             na.SplitOptions(sdp_per_level=0, max_boxes=MAX_BOXES, max_depth=64, crown_backend="resident", literal_bounds=True,
                                             corner_points=corner_points, frontier=frontier))
        label = f"tanh {name} {frontier} corner_points={corner_points}"
        check_verdict(label, res.verdict, res.witness, cs, root, h, truth)
        print(f"{label}: visited {res.visited}")
        if corner_points or truth == "holds":
            assert res.verdict == truth, (label, h, res.verdict, res.visited)
        if res.verdict == "holds":
            assert all(lf.proved_by == "crown" and lf.bound <= h for lf in res.leaves)


@pytest.mark.parametrize("name", NAMES)
def test_search_many_gives_the_same_verdicts(name):
    """four roots, the root box each time: the two thresholds above and two more at ten times the distance"""
    cs, root, _ = root_of(name)
    below, above, d = thresholds(root)
    hs = np.array([[below, below - 9.0 * d, above, above + 9.0 * d]])
    lo, hi = np.tile(root["lo"][:, None], (1, 4)), np.tile(root["hi"][:, None], (1, 4))
    with na.CrownBounder(cs["net"], cs["C"][:1]) as cb:
        got = cb.search_many(lo, hi, hs, literal_bounds=True, corner_points=True, max_boxes=MAX_BOXES, max_depth=64)
    print(f"tanh {name}: verdicts {list(got['verdict'])}, visited {got['visited'].tolist()}")
    for r, truth in enumerate(("violated", "violated", "holds", "holds")):
        check_verdict(f"tanh {name} root {r}", got["verdict"][r], got["witness"][r], cs, root, float(hs[0, r]), truth)
        assert got["verdict"][r] == truth
