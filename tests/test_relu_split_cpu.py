"""Branching on unstable ReLUs without a GPU: the float32 host routine (nnsdp_make_intervals_nodes, makeIntervalsNodes) against
affine ground truth, sampled points, an LP and the numpy restatement of tests/relu_split_common.py; the driver verifyReluSplit with
crown_backend="host"; the refusals of both C entries and of the driver."""
import ctypes as C

import numpy as np
import pytest

import nnsdp_amd as na
import exact_common as xc
import literal_common as lc
import relu_split_common as rs
from nnsdp_amd import _lib


def host(net, lo, hi, assign, Cm, steps):
    return na.makeIntervalsNodes(net, lo, hi, assign, Cm, steps=steps)


def test_the_yardstick_on_the_toy():
    """R itself, without product code: beta = 0 gives 2, eight steps end within [1, 1.5], the iterates are 2, 1.5, 1.05, 1.355, ..."""
    net, lo, hi, s, Cm = rs.toy()
    r0, r8 = rs.R(net.Ms, lo[:, 0], hi[:, 0], s[:, 0], Cm, 0), rs.R(net.Ms, lo[:, 0], hi[:, 0], s[:, 0], Cm, 8)
    assert r0["smax"][0] == 2.0 and r8["smax_plain"][0] == 2.0 and 1.0 <= r8["smax"][0] <= 1.5
    assert rs.R(net.Ms, lo[:, 0], hi[:, 0], s[:, 0], Cm, 1)["smax"][0] == 1.5
    assert abs(rs.R(net.Ms, lo[:, 0], hi[:, 0], s[:, 0], Cm, 2)["smax"][0] - 1.05) <= 1e-15
    assert abs(r8["beta"][0, 0] - 1.0) <= 0.05 and r8["beta"][0, 1] == 0.0


def test_all_zero_assignment_is_the_plain_literal_pass():
    """no forced neuron: smin / smax / A / b0 agree with nnsdp_make_intervals_lits to HOST_SLACK, smax == smax_plain, best_step == 0"""
    for cs in rs.kernel_cases():
        net, Cm, lo, hi = cs["net"], cs["C"], cs["lo"], cs["hi"]
        *_, lits = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=Cm)
        for T in (0, 8):
            nb = host(net, lo, hi, np.zeros_like(cs["assign"]), Cm, T)
            assert np.array_equal(nb.smax, nb.smax_plain) and not nb.best_step.any() and not nb.infeasible.any()
            for got, want in ((nb.smin, lits.smin), (nb.smax, lits.smax), (nb.A, lits.A), (nb.b0, lits.b0)):
                assert np.all(np.abs(got - want) <= xc.HOST_SLACK * (1.0 + np.abs(want)))


def test_fully_forced_nodes_are_affine():
    rs.check_fully_forced(host, True)


def test_partial_nodes_are_sound():
    rs.check_partial(host, True)


def test_forced_infeasibility():
    rs.check_forced_infeasible(host)


def test_multipliers_do_their_job():
    rs.check_toy(host, True)


def test_lp_truth():
    rs.check_lp_truth(host, True)


def test_the_host_routine_follows_the_yardstick():
    """float32 against R(float64) on the kernel cases at 0 and 3 steps: smax_plain, smin and the clipped bounds to HOST_SLACK; smax never
    above smax_plain; the branching neuron equal wherever the two best scores differ by more than HOST_SLACK"""
    for cs in rs.kernel_cases():
        net, Cm, lo, hi, s = cs["net"], cs["C"], cs["lo"], cs["hi"], cs["assign"]
        nb = host(net, lo, hi, s, Cm, 3)
        for b in range(lo.shape[1]):
            r = rs.R(net.Ms, lo[:, b], hi[:, b], s[:, b], Cm, 3)
            for got, want in ((nb.smax_plain[:, b], r["smax_plain"]), (nb.smin[:, b], r["smin"]), (nb.pre_lo[:, b], r["pre_lo"]), (nb.pre_hi[:, b], r["pre_hi"])):
                assert np.all(np.abs(got - want) <= xc.HOST_SLACK * (1.0 + np.abs(want))), (net.xdims, b)
            clear = r["gap"] > xc.HOST_SLACK * (1.0 + np.abs(r["smax_plain"]))
            assert np.array_equal(nb.branch[clear, b], r["branch"][clear]), (net.xdims, b)
            assert np.all(nb.smax[:, b] <= nb.smax_plain[:, b])


@pytest.mark.parametrize("name", list(xc.SMALL))
def test_the_driver_on_the_fixture_nets(name):
    rs.check_driver_small("host", name)


def test_the_driver_on_sixteen_inputs():
    rs.check_driver_16("host")


def test_the_driver_reports_budget_and_exhaustion():
    st = xc.verdict_setting("3-10-10-3")
    h = rs.literal_threshold(st, 1e-4)
    res = na.verifyReluSplit(st["net"], st["lo"], st["hi"], [(st["normal"], h)], na.ReluSplitOptions(max_nodes=9))
    assert res.verdict == "unknown" and res.reason == "budget" and res.visited <= 9 and res.open
    rs.check_tree(res, 20)
    res = na.verifyReluSplit(st["net"], st["lo"], st["hi"], [(st["normal"], h)], na.ReluSplitOptions(max_depth=2))
    assert res.verdict == "unknown" and res.reason == "budget" and res.depth == 2
    # clipping alone (steps = 0) leaves fully split nodes open on 2-8-8-2: "exhausted", with every open node's free neurons stable
    st = xc.verdict_setting("2-8-8-2")
    res = na.verifyReluSplit(st["net"], st["lo"], st["hi"], [(st["normal"], rs.literal_threshold(st, 1e-4))], na.ReluSplitOptions(steps=0))
    print(f"2-8-8-2 without multipliers: {res.verdict} ({res.reason}), visited {res.visited}, {len(res.open)} open")
    assert res.verdict in ("holds", "unknown") and (res.verdict == "holds" or res.reason in ("exhausted", "budget"))


def _raw_host(net, lo, hi, assign, Cm, steps=0, eta0=0.5, decay=0.9, activ=None):
    lib, dp, ip = _lib.load(), _lib.c_double_p, _lib.c_int32_p
    xd = np.asarray(net.xdims, dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    nrm = None if Cm is None else np.ascontiguousarray(Cm, dtype=np.float64)
    asg = np.ascontiguousarray(assign, dtype=np.int8)
    rc = lib.nnsdp_make_intervals_nodes(net.K, xd.ctypes.data_as(ip), Mp.ctypes.data_as(dp), na.methods._activ_code(net.activ) if activ is None else activ,
                                        np.ascontiguousarray(lo).ctypes.data_as(dp), np.ascontiguousarray(hi).ctypes.data_as(dp),
                                        asg.ctypes.data_as(C.POINTER(C.c_int8)), 0 if nrm is None else nrm.shape[0],
                                        None if nrm is None else nrm.ctypes.data_as(dp), int(steps), float(eta0), float(decay), *([None] * 10))
    return rc, lib.nnsdp_last_error().decode()


def test_refusals():
    """every refusal of the issue's scope, with its message: the host entry; the handle entry's options on a null handle (they are
    checked before the handle, so that no GPU is needed); the Python layers"""
    net, lo, hi, s, Cm = rs.toy()
    lo, hi, s = lo[:, 0], hi[:, 0], s[:, 0]
    assert _raw_host(net, lo, hi, s, Cm)[0] == 0
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    bad = s.copy()
    bad[1] = 2
    for args, kw, word in (((tanh, lo, hi, s, Cm), {}, "Tanh"), ((net, lo, hi, s, None), {}, "literals"), ((net, lo, hi, bad, Cm), {}, "assign"),
                           ((net, lo, hi, s, Cm), dict(steps=-1), "steps"), ((net, lo, hi, s, Cm), dict(steps=65), "steps"),
                           ((net, lo, hi, s, Cm), dict(eta0=0.0), "eta0"), ((net, lo, hi, s, Cm), dict(eta0=np.inf), "eta0"),
                           ((net, lo, hi, s, Cm), dict(decay=0.0), "decay"), ((net, lo, hi, s, Cm), dict(decay=1.5), "decay")):
        rc, msg = _raw_host(*args, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    lib = _lib.load()
    for opt, word in (((65, 0.5, 0.9), "steps"), ((1, -1.0, 0.9), "eta0"), ((1, 0.5, 1.01), "decay"), ((1, 0.5, 0.9), "null handle")):
        rc = lib.nnsdp_crown_bound_nodes(None, 1, None, None, None, *opt, *([None] * 11))
        assert rc == -1 and word in lib.nnsdp_last_error().decode(), (opt, lib.nnsdp_last_error().decode())
    # the Python layers refuse before any library call
    with pytest.raises(ValueError, match="-1, 0 or \\+1"):
        na.makeIntervalsNodes(net, lo[:, None], hi[:, None], bad[:, None], Cm)
    with pytest.raises(ValueError, match="acdim x nnode"):
        na.makeIntervalsNodes(net, lo[:, None], hi[:, None], s[:1, None], Cm)
    lit = [(np.array([1.0]), 1.5)]
    wide = lc.random_net([2, 80, 2], 3)
    for a, kw, word in (((tanh, lo, hi, lit), {}, "Tanh"), ((net, lo, hi, []), {}, "literals"), ((net, lo, hi, lit), dict(steps=65), "steps"),
                        ((net, lo, hi, lit), dict(eta0=-1.0), "eta0"), ((net, lo, hi, lit), dict(decay=0.0), "decay"),
                        ((net, lo, hi, lit), dict(crown_backend="gpu"), "crown_backend"),
                        ((wide, np.zeros(2), np.ones(2), [(np.array([1.0, -1.0]), 0.0)]), dict(crown_backend="resident"), "widths up to 64")):
        with pytest.raises(ValueError, match=word):
            na.verifyReluSplit(*a, na.ReluSplitOptions(**kw))
