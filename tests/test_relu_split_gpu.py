"""Branching on unstable ReLUs on the GPU: nnsdp_crown_bound_nodes (csrc/crown_relu_split.hpp: k_crown_nodes and k_crown_beta on the
resident bounder's stream) against the plain bounder, affine ground truth, sampled points, an LP and the numpy restatement `R` of
tests/relu_split_common.py; the driver verifyReluSplit with crown_backend="resident"."""
import numpy as np
import pytest

import nnsdp_amd as na
import crown_alpha_common as ca
import exact_common as xc
import literal_common as lc
import relu_split_common as rs

_cache = {}


def gpu(net, lo, hi, assign, Cm, steps):
    with na.CrownBounder(net, Cm) as bd:
        return bd.bound_nodes(lo, hi, assign, steps=steps)


def case(n, T):
    """the kernel case n at T steps; computed once, shared, never modified"""
    if (n, T) not in _cache:
        cs = rs.kernel_cases()[n]
        _cache[(n, T)] = gpu(cs["net"], cs["lo"], cs["hi"], cs["assign"], cs["C"], T)
    return _cache[(n, T)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(rs.NETS)))
def test_all_zero_assignment_has_the_bits_of_bound(n):
    cs = rs.kernel_cases()[n]
    with na.CrownBounder(cs["net"], cs["C"]) as bd:
        *_, lits = bd.bound(cs["lo"], cs["hi"])
        for T in (0, 1, 16):
            nb = bd.bound_nodes(cs["lo"], cs["hi"], np.zeros_like(cs["assign"]), steps=T)
            for got, want in ((nb.smin, lits.smin), (nb.smax, lits.smax), (nb.A, lits.A), (nb.b0, lits.b0), (nb.smax_plain, lits.smax)):
                assert np.array_equal(got, want), T
            assert not nb.best_step.any() and not nb.infeasible.any()


@pytest.mark.gpu
def test_fully_forced_nodes_are_affine():
    rs.check_fully_forced(gpu, False)


@pytest.mark.gpu
def test_partial_nodes_are_sound():
    rs.check_partial(gpu, False)


@pytest.mark.gpu
def test_forced_infeasibility():
    rs.check_forced_infeasible(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("T", rs.STEPS)
@pytest.mark.parametrize("n", range(len(rs.NETS)))
def test_against_the_yardstick(n, T):
    """smax, uA, ub0 within 8 r of R(long double), best_step equal; branch equal wherever the two best scores differ by more than that"""
    rs.check_yardstick(rs.kernel_cases()[n], case(n, T), T)


@pytest.mark.gpu
@pytest.mark.parametrize("n, nlit", ((0, 17), (1, 64)))
def test_more_literals_than_one_tile(n, nlit):
    """17 and 64 literals (two and four 16-row tiles of the products), T = 3, against the yardstick as above; a literal alone has the
    bits it has among the others"""
    cs = dict(rs.kernel_cases()[n])
    cs["C"] = lc.literal_rows(cs["net"].xdims[-1], nlit, 700 + n)
    nb = gpu(cs["net"], cs["lo"], cs["hi"], cs["assign"], cs["C"], 3)
    for b in range(cs["lo"].shape[1]):
        ref, tol = rs.r_tolerance(cs, b, 3)
        errs = [ca.rel_err(got, ref[k]) for got, k in ((nb.smax[:, b], "smax"), (nb.A[:, :, b], "A"), (nb.b0[:, b], "b0"))]
        assert max(errs) <= tol and np.array_equal(nb.best_step[:, b], ref["best_step"]), (b, errs, tol)
    for i in (0, 16, nlit - 1):
        alone = gpu(cs["net"], cs["lo"], cs["hi"], cs["assign"], cs["C"][[i]], 3)
        for name in ("smin", "smax_plain", "smax", "A", "b0", "best_step", "branch"):
            assert np.array_equal(getattr(alone, name)[0], getattr(nb, name)[i]), (i, name)
        assert np.array_equal(alone.pre_lo, nb.pre_lo) and np.array_equal(alone.infeasible, nb.infeasible)


@pytest.mark.gpu
def test_multipliers_do_their_job():
    rs.check_toy(gpu, False)


@pytest.mark.gpu
def test_lp_truth():
    rs.check_lp_truth(gpu, False)


@pytest.mark.gpu
def test_independence():
    """one node alone, and the same node at positions 0, 137 and 299 of 300 different nodes, return identical bits; so does a second
    call on the same handle"""
    cs = rs.kernel_cases()[0]
    net, Cm, rng = cs["net"], cs["C"], np.random.default_rng(8)
    ctr = rng.uniform(-0.5, 0.5, (3, 300))
    lo, hi = ctr - 0.4, ctr + 0.4
    s = np.stack([rs.node_from_point(net, lo[:, b], hi[:, b], rng, 0.3)[1] for b in range(300)], 1)
    mine = (lo[:, 5].copy(), hi[:, 5].copy(), s[:, 5].copy())
    with na.CrownBounder(net, Cm) as bd:
        alone = bd.bound_nodes(mine[0][:, None], mine[1][:, None], mine[2][:, None], steps=8)
        for pos in (0, 137, 299):
            l2, h2, s2 = lo.copy(), hi.copy(), s.copy()
            l2[:, pos], h2[:, pos], s2[:, pos] = mine
            many = bd.bound_nodes(l2, h2, s2, steps=8)
            for name in na.NodeBounds._fields:
                assert np.array_equal(getattr(alone, name)[..., 0], getattr(many, name)[..., pos]), (pos, name)
        again = bd.bound_nodes(mine[0][:, None], mine[1][:, None], mine[2][:, None], steps=8)
        assert all(np.array_equal(getattr(alone, name), getattr(again, name)) for name in na.NodeBounds._fields)
        assert (alone.best_step > 0).any()


@pytest.mark.gpu
def test_the_handle():
    """the node buffers come with the first node call, are counted by info() and stay; a bounder that never calls bound_nodes holds what
    it held; the refusals that need a handle arrive as messages before anything is launched"""
    cs = rs.kernel_cases()[2]
    net, Cm = cs["net"], cs["C"]
    with na.CrownBounder(net, Cm) as bd:
        i0 = bd.info()
        bd.bound_nodes(cs["lo"], cs["hi"], cs["assign"], steps=3)
        i1 = bd.info()
        assert i1["device_allocations"] == i0["device_allocations"] + 3 and i1["device_bytes"] > i0["device_bytes"] and i1["bound_calls"] == 1
        bd.bound_nodes(cs["lo"][:, :2], cs["hi"][:, :2], cs["assign"][:, :2], steps=0)
        i2 = bd.info()
        assert (i2["device_allocations"], i2["device_bytes"], i2["network_uploads"]) == (i1["device_allocations"], i1["device_bytes"], 1)
        for kw, word in ((dict(steps=65), "steps"), (dict(eta0=0.0), "eta0"), (dict(decay=2.0), "decay")):
            with pytest.raises(na._lib.NnsdpError, match=word):
                bd.bound_nodes(cs["lo"], cs["hi"], cs["assign"], **kw)
        assert bd.info()["bound_calls"] == 2
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    for make, word in ((lambda: na.CrownBounder(tanh, Cm), "Tanh"), (lambda: na.CrownBounder(net), "literals"),
                       (lambda: na.CrownBounder(net, Cm, max_width=128), "wide")):
        with make() as bd:
            before = bd.info()
            with pytest.raises(na._lib.NnsdpError, match=word):
                bd.bound_nodes(cs["lo"], cs["hi"], cs["assign"], steps=1)
            assert bd.info() == before


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(xc.SMALL))
def test_the_driver_on_the_fixture_nets(name):
    rs.check_driver_small("resident", name)


@pytest.mark.gpu
def test_the_driver_on_sixteen_inputs():
    rs.check_driver_16("resident")
