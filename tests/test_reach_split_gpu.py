"""reachSplit on the GPU.  The specification of frontier = "device" (CrownBounder.reach, csrc/crown_reach.hpp) is the Python loop: with
crown_backend = "resident" the two frontiers give the same result bit for bit (reach_common.assert_same_reach).  Then the enclosure of the
exact maxima of tests/golden/exact_ranges.json for both frontiers, the handle shared with bound and search, and the SDP stage."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import vnnlib as vl
import crown_tanh_common as tc
import exact_common as ec
import literal_common as lc
import reach_common as rc
from test_split_cpu import NORMAL
from test_split_gpu import SDP_BETA, SDP_BOX, SDP_NET

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)
_state = {}


def both(net, lo, hi, C, tol=rc.TOL, **options):
    """the host frontier's result (computed once per case) and the device frontier's, both on the resident bounder, bounds only"""
    chunk = options.pop("chunk", 4096)
    opt = dict(crown_backend="resident", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP, max_depth=64)
    opt.update(options)
    key = (id(net), lo.tobytes(), hi.tobytes(), C.tobytes(), np.asarray(tol).tobytes(), tuple(sorted(opt.items())))
    if key not in _state:
        _state[key] = (net, na.reachSplit(net, lo, hi, C, tol, split=na.SplitOptions(**opt)))
    dev = na.reachSplit(net, lo, hi, C, tol, split=na.SplitOptions(frontier="device", chunk=chunk, **opt))
    return _state[key][1], dev


def forward_tol(net, C, X):
    """|c' f(x) in one float64 summation order - the same in another| <= 2 n eps * (|c|' g(|x|)), g the network with |W|, |b| and the
    identity for the activation (ReLU and tanh are 1-Lipschitz and |act(z)| <= |z|), n = the operations on the longest path: per layer
    its fan-in products and sums and the bias, 8 more per hidden layer for a tanh of a few ulps, then the ny terms of c' y.  Per row of
    C and column of X"""
    a = np.abs(X)
    for Mk in net.Ms:
        a = np.abs(Mk[:, :-1]) @ a + np.abs(Mk[:, -1:])
    n = sum(2 * d + 1 for d in net.xdims[:-1]) + 8 * (net.K - 1) + 2 * net.xdims[-1]
    return 2.0 * n * ec.EPS * (np.abs(C) @ a)


def check_lower_against_incumbent(label, net, C, res):
    t = np.diag(forward_tol(net, C, res.witnesses.T))
    d = np.abs(res.lower - res.incumbent)
    print(f"{label}: worst |lower - incumbent| / tol {np.max(d / np.maximum(t, np.finfo(float).tiny)):.3e} (|lower - incumbent| {d.max():.3e})")
    assert np.all(d <= t)


def fixture_case(case, box):
    fb = rc.fixture_box(case, box)
    tols = ec.fp64_tols(ec.case(case), fb["lo"][:, None], fb["hi"][:, None])
    fb["slack"] = max(tols["smax"], tols["ymax"])
    return fb


@pytest.mark.parametrize("case,box,options", [("2-8-8-2", "root", {}), ("3-10-10-3", "root", {}), ("3-10-10-3", "root", dict(chunk=4)),
                                              ("3-10-10-3", "root", dict(max_boxes=50)), ("3-10-10-3", "root", dict(max_boxes=1)),
                                              ("3-10-10-3", "root", dict(max_depth=3)), ("2-8-8-2", "root", dict(corner_points=False)),
                                              ("3-10-10-3", "edge0", {}), ("2-8-8-2", "point", {}), ("3-10-10-3", "stable", {})])
def test_both_frontiers_give_the_same_enclosure_of_the_exact_maxima(case, box, options):
    """2-8-8-2: 11 rows, ny < 8 (the plain sum of the cheap bound).  3-10-10-3: 13 rows; a level of 22 boxes has 308 points, more than the
    256 threads of the incumbent kernel's workgroup"""
    fb = fixture_case(case, box)
    host, dev = both(fb["net"], fb["lo"], fb["hi"], fb["C"], **options)
    label = f"{case} {box} {options}"
    print(f"{label}: seconds host {host.seconds['total']:.4f} device {dev.seconds['total']:.4f} (kernels {dev.seconds['kernel']:.4f})")
    for name, res in (("host", host), ("device", dev)):
        rc.check_enclosure(f"{label} {name}", res, fb["w"], fb["v"], fb["slack"], rc.TOL, fb["lo"], fb["hi"])
        check_lower_against_incumbent(f"{label} {name}", fb["net"], fb["C"], res)
    rc.assert_same_reach(host, dev)
    budget = "max_boxes" in options or "max_depth" in options
    assert host.status == ("budget" if budget else "converged") and host.visited <= options.get("max_boxes", ec.MAX_BOXES_CAP)
    if case == "3-10-10-3" and box == "root" and not budget:
        sizes = np.bincount([lf.depth for lf in host.leaves]).astype(float)
        for d in range(len(sizes) - 2, -1, -1):
            sizes[d] += sizes[d + 1] / 2
        assert sizes.max() * (1 + len(fb["C"])) > 256, sizes       # a level with more points than one pass of the workgroup


def test_a_level_longer_than_a_scan_tile():
    """levels of more than 256 boxes: k_search_scan carries its offset over tiles, k_reach_scatter runs in workgroups after the first and
    k_reach_incumbent walks the points with a stride.  The numpy restatement (reach_common.reference) converges after 3 937 boxes at depth
    21 with four levels above 256, the largest 534"""
    net = _state.setdefault("long", lc.random_net([4, 24, 24, 3], 3))
    C = np.vstack([np.eye(3), -np.eye(3)])
    lo, hi = -np.ones(4), np.ones(4)
    host, dev = both(net, lo, hi, C, tol=2e-2, corner_points=False, max_boxes=4096)
    sizes = np.bincount([lf.depth for lf in host.leaves]).astype(float)      # (level_sizes of test_split_frontier_gpu.py)
    for d in range(len(sizes) - 2, -1, -1):
        sizes[d] += sizes[d + 1] / 2
    print(f"long level: {host.status} after {host.visited} boxes, depth {host.depth}; levels {sizes.astype(int).tolist()}")
    rc.assert_same_reach(host, dev)
    assert sizes.max() > 256, sizes


def test_ten_outputs_take_the_pairwise_sum():
    net = _state.setdefault("wide", lc.random_net([3, 16, 16, 10], 110))
    C = lc.literal_rows(10, 9, 7)
    host, dev = both(net, -np.ones(3), np.ones(3), C, tol=1e-2)
    print(f"ny 10: {host.status} after {host.visited} boxes, depth {host.depth}")
    assert host.status == "converged" and host.visited > 1
    rc.assert_same_reach(host, dev)
    check_lower_against_incumbent("ny 10", net, C, dev)


def test_sixty_four_directions():
    fb = rc.fixture_box("2-8-8-2", "small-a")
    C = lc.literal_rows(2, 64, 11)
    tol = np.where(np.arange(64) % 2 == 0, 1e-3, 0.0)         # (the box is small: only the zero tolerances can make it split)
    # max_depth 12: six cuts per coordinate keep a width of 0.1 * 2^-6 on a box near 0.9 dyadic to the 1e-12 that assert_tiles asks for
    host, dev = both(fb["net"], fb["lo"], fb["hi"], C, tol=tol, max_boxes=128, max_depth=12)
    print(f"nlit 64: {host.status} after {host.visited} boxes, depth {host.depth}")
    rc.assert_same_reach(host, dev)
    rc.assert_tiles_root(dev.leaves, fb["lo"], fb["hi"])
    X = fb["lo"][:, None] + np.random.default_rng(3).random((2, 2000)) * (fb["hi"] - fb["lo"])[:, None]
    s = (C @ lc.forward(fb["net"], X)).max(axis=1)
    slack = forward_tol(fb["net"], C, X).max(axis=1) + 64 * ec.EPS * (1.0 + np.abs(dev.upper))
    assert np.all(dev.upper >= s - slack) and np.all(dev.lower <= dev.upper + slack)


def test_one_direction():
    fb = fixture_case("3-10-10-3", "root")
    host, dev = both(fb["net"], fb["lo"], fb["hi"], fb["C"][:1])
    rc.check_enclosure("nlit 1", dev, fb["w"][:1], fb["v"][:1], fb["slack"], rc.TOL, fb["lo"], fb["hi"])
    assert host.status == "converged" and host.visited > 1
    rc.assert_same_reach(host, dev)


def test_a_tanh_network():
    """no exact maximum for tanh: the same tree, and upper + tol above a sampled maximum"""
    tanh = _state.setdefault("tanh", tc.tanh_copy(lc.random_net([3, 17, 33, 4], 14)))
    C = np.array([[1.0, 0.0, 0.0, -1.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]])
    lo, hi = -np.ones(3), np.ones(3)
    host, dev = both(tanh, lo, hi, C, tol=1e-2, max_boxes=512)
    print(f"tanh: {host.status} after {host.visited} boxes, depth {host.depth}; upper {dev.upper}, lower {dev.lower}")
    rc.assert_same_reach(host, dev)
    rc.assert_tiles_root(dev.leaves, lo, hi)
    X = lo[:, None] + np.random.default_rng(0).random((3, 20000)) * (hi - lo)[:, None]
    s = (C @ lc.forward(tanh, X)).max(axis=1)
    assert np.all(dev.upper + 1e-2 >= s) and np.all(dev.lower <= dev.upper + 1e-2)
    if dev.status == "converged":
        assert np.all(dev.upper <= dev.incumbent + 1e-2)
    check_lower_against_incumbent("tanh", tanh, C, dev)


def test_one_handle_for_bound_search_and_reach():
    fb = rc.fixture_box("3-10-10-3", "root")
    net, C, rlo, rhi = fb["net"], fb["C"], fb["lo"], fb["hi"]
    lo, hi = np.stack([rlo, 0.5 * rlo], axis=1), np.stack([rhi, 0.25 * rhi], axis=1)
    hs = fb["v"] - 0.05         # every literal false somewhere: the search has to split
    tol = np.full(len(C), rc.TOL)
    with na.CrownBounder(net, C) as cb:
        before = cb.bound(lo, hi)
        skw = dict(literal_bounds=True, corner_points=True, max_boxes=100, max_depth=24, chunk=16)
        s_before = cb.search(rlo, rhi, hs, **skw)
        kw = dict(corner_points=True, max_boxes=300, max_depth=64, chunk=16)
        info0 = cb.info()
        first = cb.reach(rlo, rhi, tol, **kw)
        info1 = cb.info()
        second = cb.reach(rlo, rhi, tol, **kw)
        info2 = cb.info()
        assert info1["device_allocations"] > info0["device_allocations"] and info1["device_bytes"] > info0["device_bytes"]
        assert (info2["device_allocations"], info2["network_uploads"], info2["device_bytes"]) == \
               (info1["device_allocations"], info1["network_uploads"], info1["device_bytes"])
        assert (info0["reach_calls"], info1["reach_calls"], info2["reach_calls"]) == (0, 1, 2) and info2["network_uploads"] == 1
        assert first["status"] == "converged" and first["visited"] == second["visited"] > 1
        for k in ("lo", "hi", "leaf_depth", "closed", "bound", "incumbent", "witnesses"):
            assert np.array_equal(first[k], second[k]), k
        after = cb.bound(lo, hi)
        for a, b in zip(before[:6] + tuple(before[6]), after[:6] + tuple(after[6])):
            assert np.array_equal(a, b)
        s_after = cb.search(rlo, rhi, hs, **skw)
        assert (s_before["verdict"], s_before["visited"], s_before["depth"]) == (s_after["verdict"], s_after["visited"], s_after["depth"])
        for k in ("lo", "hi", "leaf_depth", "proved", "literal", "bound"):
            assert np.array_equal(s_before[k], s_after[k]), k
        third = cb.reach(rlo, rhi, tol, **kw)
        for k in ("lo", "hi", "leaf_depth", "closed", "bound", "incumbent", "witnesses"):
            assert np.array_equal(first[k], third[k]), k
        # the refusals that need a handle: nothing is allocated by a refused call
        info3 = cb.info()
        bad_tol = tol.copy()
        bad_tol[2] = np.nan
        neg_tol = tol.copy()
        neg_tol[1] = -1e-3
        for bad, msg in ((dict(tol=bad_tol), "tol"), (dict(tol=neg_tol), "tol"), (dict(lo=np.array([0.0, np.nan, 0.0])), "finite"),
                         (dict(hi=np.array([1.0, np.inf, 1.0])), "finite"), (dict(lo=2.0 * rhi), "x1min must be <= x1max"),
                         (dict(max_boxes=2 ** 25), "2\\^31"), (dict(max_boxes=0), "max_boxes"), (dict(chunk=0), "chunk"), (dict(max_depth=-1), "max_depth")):
            args = dict(lo=rlo, hi=rhi, tol=tol, **kw)
            args.update(bad)
            with pytest.raises(na._lib.NnsdpError, match=msg):
                cb.reach(args.pop("lo"), args.pop("hi"), args.pop("tol"), **args)
        assert cb.info() == info3
    with na.CrownBounder(net) as plain:
        with pytest.raises(na._lib.NnsdpError, match="without normals"):
            plain.reach(rlo, rhi, 1e-3, max_boxes=4)
        assert plain.info()["box_capacity"] == 0 and plain.info()["reach_calls"] == 0


def test_the_sdp_stage_closes_what_the_bounds_cannot():
    """the instance of test_only_the_sdp_can_prove_it (tests/test_split_gpu.py) with one box: the threshold L + tol halfway between the
    root's SDP bound rho and its bound c0 from the bound kernel"""
    wide = na.randomNetwork(SDP_NET["xdims"], sigma=SDP_NET["sigma"], seed=SDP_NET["seed"])
    lo, hi = SDP_BOX
    C = NORMAL[None]
    with na.CrownBounder(wide, C) as cb:
        iv = cb.bound(lo[:, None], hi[:, None])
    ymin, ymax = iv[4][:, 0], iv[5][:, 0]
    cheap = float(np.maximum(NORMAL * ymin, NORMAL * ymax).sum())
    c0 = min(cheap, float(iv[6].smax[0, 0]))
    sq = na.SafetyQuery(ffnet=wide, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_safety=na.QcSafety(S=vl.hplaneS(NORMAL, c0, wide)),
                        qc_activs=na.makeQcActivs(wide, lo, hi, SDP_BETA))
    rq, _, h0 = vl.reachForm(sq, ybounds=(ymin, ymax))
    plain = na.runQuery(rq, OPTS)
    rho = plain.objective_value + h0
    assert vl.isSolutionGood(plain) and rho < c0 - 1e-3 * (1.0 + abs(c0))
    one = dict(crown_backend="resident", corner_points=True, max_boxes=1)
    bounds = na.reachSplit(wide, lo, hi, C, 0.0, SDP_BETA, OPTS, na.SplitOptions(sdp_per_level=0, **one))
    L = float(bounds.incumbent[0])
    tol = 0.5 * (rho + c0) - L
    assert bounds.status == "budget" and L <= rho and tol > 0
    for frontier in ("host", "device"):
        no = na.reachSplit(wide, lo, hi, C, tol, SDP_BETA, OPTS, na.SplitOptions(sdp_per_level=0, frontier=frontier, **one))
        assert no.status == "budget" and no.visited == 1 and no.sdp_solves == 0 and len(no.leaves) == 1 and no.leaves[0].closed_by is None
        assert no.upper[0] == c0 and no.incumbent[0] == L
    yes = na.reachSplit(wide, lo, hi, C, tol, SDP_BETA, OPTS, na.SplitOptions(sdp_per_level=1, **one))
    assert yes.status == "converged" and yes.visited == 1 and yes.sdp_solves == 1
    (lf,) = yes.leaves
    assert lf.closed_by == "sdp" and yes.upper[0] == lf.bound[0] and yes.upper[0] <= L + tol and yes.upper[0] < c0
    assert yes.seconds["solve"] > 0 and yes.seconds["setup"] > 0
