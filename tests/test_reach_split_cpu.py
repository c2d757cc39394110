"""reachSplit without a GPU (crown_backend = "host", the float32 host routine): the enclosure of the exact maxima of
tests/golden/exact_ranges.json, the budget, one joint tree against separate trees, the float64 numpy reference of reach_common, and the
refusals of reachSplit and of nnsdp_crown_reach that need no handle."""
import ctypes as C

import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import exact_common as ec
import literal_common as lc
import reach_common as rc

_state = {}


def host(case, box, **kw):
    fb = rc.fixture_box(case, box)
    key = (case, box, tuple(sorted(kw.items())))
    if key not in _state:
        opt = dict(crown_backend="host", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP, max_depth=64)      # (run_split's depth)
        opt.update(kw)
        _state[key] = na.reachSplit(fb["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL, split=na.SplitOptions(**opt))
    return fb, _state[key]


def enclosed(label, fb, res):
    rc.check_enclosure(label, res, fb["w"], fb["v"], ec.HOST_SLACK * (1.0 + np.abs(fb["w"])), rc.TOL, fb["lo"], fb["hi"])


@pytest.mark.parametrize("box", rc.BOXES)
@pytest.mark.parametrize("case", sorted(ec.SMALL))
def test_the_exact_maxima_are_enclosed(case, box):
    fb, res = host(case, box)
    enclosed(f"{case} {box}", fb, res)
    assert res.status == "converged" and res.visited < ec.MAX_BOXES_CAP and res.sdp_solves == 0
    if box in ("point", "stable"):
        assert res.visited == 1 and len(res.leaves) == 1 and res.depth == 0


@pytest.mark.parametrize("case", sorted(ec.SMALL))
def test_the_roots_converge_without_corner_points(case):
    fb, res = host(case, "root", corner_points=False)
    enclosed(f"{case} root, centres only", fb, res)
    assert res.status == "converged" and res.visited < ec.MAX_BOXES_CAP


def test_a_budget_of_five_boxes():
    fb, res = host("3-10-10-3", "root", max_boxes=5)
    enclosed("3-10-10-3 root, max_boxes 5", fb, res)
    assert res.status == "budget" and res.visited <= 5
    assert all(lf.bound is not None and lf.bound.shape == (len(fb["C"]),) for lf in res.leaves)


@pytest.mark.parametrize("max_boxes,visited", [(1, 1), (2, 1), (3, 3)])
def test_a_level_is_created_only_when_the_budget_holds_all_of_it(max_boxes, visited):
    fb, res = host("3-10-10-3", "root", max_boxes=max_boxes)
    enclosed(f"3-10-10-3 root, max_boxes {max_boxes}", fb, res)
    assert res.status == "budget" and res.visited == visited


def test_max_depth_ends_in_budget():
    fb, res = host("3-10-10-3", "root", max_depth=2)
    enclosed("3-10-10-3 root, max_depth 2", fb, res)
    assert res.status == "budget" and res.depth == 2 and max(lf.depth for lf in res.leaves) == 2


def test_one_joint_tree_visits_no_more_than_the_separate_trees_together():
    fb, joint = host("3-10-10-3", "root")
    opt = na.SplitOptions(crown_backend="host", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP)
    separate = [na.reachSplit(fb["net"], fb["lo"], fb["hi"], fb["C"][i:i + 1], rc.TOL, split=opt) for i in range(len(fb["C"]))]
    total = sum(r.visited for r in separate)
    print(f"joint tree {joint.visited} boxes; {len(separate)} separate trees {total} boxes ({[r.visited for r in separate]})")
    assert all(r.status == "converged" for r in separate)
    assert joint.visited <= total


def test_a_vector_of_tolerances():
    fb = rc.fixture_box("2-8-8-2", "half-a")
    tol = np.where(np.arange(len(fb["C"])) % 2 == 0, 1e-2, 1e-4)
    res = na.reachSplit(fb["net"], fb["lo"], fb["hi"], fb["C"], tol,
                        split=na.SplitOptions(crown_backend="host", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP))
    rc.check_enclosure("2-8-8-2 half-a, tol per row", res, fb["w"], fb["v"], ec.HOST_SLACK * (1.0 + np.abs(fb["w"])), tol, fb["lo"], fb["hi"])
    assert res.status == "converged"


def test_alpha_steps_pass_through_on_the_host_frontier():
    fb = rc.fixture_box("2-8-8-2", "root")
    opt = dict(crown_backend="host", sdp_per_level=0, corner_points=True, max_boxes=ec.MAX_BOXES_CAP)
    res = na.reachSplit(fb["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL, split=na.SplitOptions(alpha_steps=4, alpha_inherit=True, **opt))
    enclosed("2-8-8-2 root, alpha_steps 4", fb, res)
    assert res.status == "converged"


@pytest.mark.parametrize("case", sorted(ec.SMALL))
def test_the_tree_of_the_reference_on_the_point_box(case):
    """a point box: one box, no comparison that float32 against float64 could flip"""
    fb, res = host(case, "point")
    ref = rc.reference(fb["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL)
    assert (res.status, res.visited, res.depth, len(res.leaves)) == (ref.status, ref.visited, ref.depth, len(ref.leaves)) == ("converged", 1, 0, 1)
    for p, q in zip(res.leaves, ref.leaves):
        assert np.array_equal(p.lo, q.lo) and np.array_equal(p.hi, q.hi) and p.depth == q.depth and p.closed_by == q.closed_by
        assert np.all(np.abs(p.bound - q.bound) <= ec.HOST_SLACK * (1.0 + np.abs(q.bound)))
    assert np.array_equal(res.witnesses, ref.witnesses)
    assert np.all(np.abs(res.incumbent - ref.incumbent) <= 64 * ec.EPS * (1.0 + np.abs(ref.incumbent)))


@pytest.mark.parametrize("case", sorted(ec.SMALL))
def test_the_reference_encloses_the_roots_as_the_driver_does(case):
    fb, res = host(case, "root")
    ref = _state.setdefault(("ref", case), rc.reference(fb["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL))
    rc.check_enclosure(f"{case} root, float64 reference", ref, fb["w"], fb["v"], ec.HOST_SLACK * (1.0 + np.abs(fb["w"])), rc.TOL, fb["lo"], fb["hi"])
    print(f"{case} root: driver {res.visited} boxes, reference {ref.visited} boxes")
    assert res.status == ref.status == "converged" and ref.visited <= 195


def test_the_polytope_by_splitting():
    net = ec.case_net("2-8-8-2")
    lo, hi = -np.ones(2), np.ones(2)
    hplanes, res = na.findReach2DpolySplit(net, lo, hi, 1e-3, num_hplanes=6, split=na.SplitOptions(corner_points=True, sdp_per_level=0, max_boxes=ec.MAX_BOXES_CAP))
    assert res.status == "converged" and len(hplanes) == 6
    Y = lc.forward(net, lo[:, None] + np.random.default_rng(0).random((2, 5000)) * (hi - lo)[:, None])
    for k, (nrm, up) in enumerate(hplanes):
        assert np.allclose(nrm, [np.cos(2 * np.pi * k / 6), np.sin(2 * np.pi * k / 6)]) and up == res.upper[k]
        assert np.all(nrm @ Y <= up + ec.HOST_SLACK * (1.0 + abs(up)))


# ---- refusals
def _reach(split=None, normals=np.array([[1.0, 0.0]]), tol=1e-3, lo=(0.0, 0.0), hi=(1.0, 1.0)):
    return na.reachSplit(lc.random_net([2, 3, 2], 1), lo, hi, normals, tol, split=split)


@pytest.mark.parametrize("options,field", [(dict(samples=2), "samples"), (dict(crown_backend="cpu"), "crown_backend"), (dict(frontier="gpu"), "frontier"),
                                           (dict(alpha_steps=-1), "alpha_steps"), (dict(alpha_steps=2, crown_backend="gpu"), "crown_backend"),
                                           (dict(max_boxes=0), "max_boxes"),
                                           (dict(frontier="device", crown_backend="host"), "crown_backend"),
                                           (dict(frontier="device", crown_backend="gpu"), "crown_backend"),
                                           (dict(frontier="device", crown_backend="resident", samples=1), "samples"),
                                           (dict(frontier="device", crown_backend="resident", alpha_steps=2), "alpha_steps"),
                                           (dict(frontier="device", crown_backend="resident", sdp_per_level=1), "sdp_per_level")])
def test_reach_split_names_the_option_it_cannot_take(options, field):
    opt = dict(sdp_per_level=0)
    opt.update(options)
    with pytest.raises(ValueError, match=field):
        _reach(na.SplitOptions(**opt))


def test_alpha_steps_are_for_relu_networks():
    import crown_tanh_common as tc
    with pytest.raises(ValueError, match="ReLU"):
        na.reachSplit(tc.tanh_copy(lc.random_net([2, 3, 2], 1)), [0.0, 0.0], [1.0, 1.0], np.array([[1.0, 0.0]]), 1e-3,
                      split=na.SplitOptions(sdp_per_level=0, alpha_steps=2))


@pytest.mark.parametrize("kw,field", [(dict(tol=-1e-3), "tol"), (dict(tol=np.nan), "tol"), (dict(tol=np.inf), "tol"), (dict(tol=[1e-3, 1e-3]), "tol"),
                                      (dict(normals=np.zeros((0, 2))), "normals"), (dict(normals=np.zeros((65, 2))), "normals"),
                                      (dict(normals=np.zeros((1, 3))), "normals"), (dict(normals=np.zeros(2)), "normals"),
                                      (dict(lo=(2.0, 0.0)), "x1min"), (dict(lo=(0.0,)), "x1min")])
def test_reach_split_refuses_bad_arguments(kw, field):
    with pytest.raises(ValueError, match=field):
        _reach(na.SplitOptions(sdp_per_level=0), **kw)


def test_the_device_frontier_asks_for_its_bounder_past_the_option_check(monkeypatch):
    class Stop(Exception):
        pass

    def fake(net_, normals=None):
        raise Stop

    monkeypatch.setattr(na.frontend, "CrownBounder", fake)
    with pytest.raises(Stop):
        _reach(na.SplitOptions(sdp_per_level=0, frontier="device", crown_backend="resident"))


def _c_reach(h=None, max_boxes=8, max_depth=4, chunk=4):
    lib = _lib.load()
    dp, ip = _lib.c_double_p, _lib.c_int32_p
    lo, hi, tol, inc, wit = np.zeros(2), np.ones(2), np.full(1, 1e-3), np.zeros(1), np.zeros(2)
    out = (C.c_int32 * 4)()
    code = lib.nnsdp_crown_reach(h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 1, tol.ctypes.data_as(dp), 1, max_boxes, max_depth, chunk,
                                 *[C.cast(C.byref(out, 4 * k), ip) for k in range(4)], inc.ctypes.data_as(dp), wit.ctypes.data_as(dp), None)
    return code, lib.nnsdp_last_error().decode()


def test_the_c_entry_refuses_bad_arguments_before_the_gpu():
    code, msg = _c_reach(max_boxes=0)
    assert code == -1 and "max_boxes must be >= 1, got 0" in msg
    code, msg = _c_reach(chunk=0)
    assert code == -1 and "chunk must be >= 1, got 0" in msg
    code, msg = _c_reach(max_depth=-1)
    assert code == -1 and "max_depth must be >= 0, got -1" in msg
    code, msg = _c_reach()
    assert code == -1 and "null handle" in msg
    lib = _lib.load()
    assert lib.nnsdp_crown_reach_leaves(None, None, None, None, None, None) == -1 and "null handle" in lib.nnsdp_last_error().decode()


def test_the_package_exports_the_names():
    assert all(hasattr(na, n) for n in ("reachSplit", "ReachSplitResult", "ReachLeaf", "findReach2DpolySplit"))
    assert {"nnsdp_crown_reach", "nnsdp_crown_reach_leaves"} <= {s[0] for s in _lib.SYMBOLS}
