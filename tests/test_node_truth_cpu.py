"""Exact ranges over the nodes of a ReLU split as ground truth, without a GPU: tests/node_truth.py checked on its own; the float32 host
routine (nnsdp_make_intervals_nodes, makeIntervalsNodes) against tests/golden/node_ranges.json on every group of
tests/node_truth_common.py; the driver verifyReluSplit with crown_backend="host" on two-literal clauses, with every closed leaf checked
by enumeration of its node.

The measured slacks, the flagged empty nodes and the driver's node counts are in DESIGN.md section 5, "Node truth"."""
import numpy as np
import pytest

import nnsdp_amd as na
import exact_common as xc
import exact_range as er
import literal_common as lc
import node_truth as nt
import node_truth_common as nc
import relu_split_common as rs

_cache = {}


def host(net, lo, hi, assign, Cm, steps):
    return na.makeIntervalsNodes(net, lo, hi, assign, Cm, steps=steps)


# ---- the truth module itself
def test_the_toys_node_maximum_is_one():
    """x <= 0 forced: max relu(x + 1) = 1 at x = 0 (2 over the box); node_depth = 1 at x = -1; the same with the forced neuron deeper"""
    net, lo, hi, s, Cm = rs.toy()
    toys = [(net, s[:, 0])] + list(nc.deep_toys().values())
    for net, s in toys:
        srch = nt.node_regions(net.Ms, lo[:, 0], hi[:, 0], s)
        top, bot = nt.node_range(srch, Cm)
        assert abs(top.v[0] - 1.0) <= 1e-12 and abs(top.w[0] - 1.0) <= 1e-12 and abs(bot.v[0]) <= 1e-12
        assert abs(er.exact_max(net.Ms, lo[:, 0], hi[:, 0], Cm[0]).v - 2.0) <= 1e-12
        d = nt.node_depth(srch)
        assert abs(d.v - 1.0) <= 1e-12 and abs(d.x[0] + 1.0) <= 1e-12
        assert abs(nt.clause_max(srch, Cm, [0.25]).v - 0.75) <= 1e-12
        flipped = -np.asarray(s)                      # x >= 0: the maximum is the box's
        assert abs(nt.node_max(nt.node_regions(net.Ms, lo[:, 0], hi[:, 0], flipped), Cm).v[0] - 2.0) <= 1e-12


def test_an_all_zero_assignment_gives_the_regions_of_the_box():
    """node_regions without forced neurons returns the leaves of exact_range.regions, and node_depth is +inf"""
    for name in xc.SMALL:
        st = xc.verdict_setting(name)
        lo, hi = 0.5 * st["lo"], 0.5 * st["hi"]
        a, b = er.regions(st["net"].Ms, lo, hi), nt.node_regions(st["net"].Ms, lo, hi, np.zeros(sum(st["net"].xdims[1:-1])))
        assert len(a.leaves) == len(b.leaves) > 1 and a.lps == b.lps
        for la, lb in zip(a.leaves, b.leaves):
            assert all(np.array_equal(u, v) for u, v in zip(la, lb))
        assert nt.node_depth(b).v == np.inf


def test_node_maxima_against_a_dense_grid():
    """2-8-8-2, three nodes of the root box with 30 % forced.  The truth is not too low: over the 401 x 401 grid points inside the node,
    the grid maximum of every literal, of every pre-activation, of min_i (c_i' f - h_i) and of min_n s_n z_n is <= the truth + 1e-9.  It
    is not too high: every maximum is attained, |v - w| <= V_W_BOUND (1 + |v|), at a point that is in the node up to 1e-6 (1 + max |z|).
    The grid also comes within 0.05 of every literal's maximum, so the first check has teeth"""
    st = xc.verdict_setting("2-8-8-2")
    net, lo, hi = st["net"], st["lo"], st["hi"]
    Cm, rng = lc.literal_rows(2, 3, 7), np.random.default_rng(3)
    g = np.linspace(lo[0], hi[0], 401)
    X = np.stack([a.ravel() for a in np.meshgrid(g, g)])
    Z, Y = rs.hidden64(net, X), Cm @ lc.forward(net, X)
    for _ in range(3):
        _, s = rs.node_from_point(net, lo, hi, rng, 0.3)
        inside = np.all((Z * s[:, None])[s != 0] >= 0.0, axis=0)
        assert inside.sum() > 100
        srch = nt.node_regions(net.Ms, lo, hi, s)
        top, bot = nt.node_range(srch, Cm)
        ztop, zbot = nt.node_pre_range(srch)
        h = 0.5 * top.v
        cm, d = nt.clause_max(srch, Cm, h), nt.node_depth(srch)
        pairs = ((Y[:, inside].max(1), top), (-Y[:, inside].min(1), bot._replace(v=-bot.v, w=-bot.w)), (Z[:, inside].max(1), ztop),
                 (-Z[:, inside].min(1), zbot._replace(v=-zbot.v, w=-zbot.w)), ((Y[:, inside] - h[:, None]).min(0).max(), cm),
                 ((Z * s[:, None])[s != 0][:, inside].min(0).max(), d))
        zmax = max(np.abs(ztop.v).max(), np.abs(zbot.v).max())
        for grid, m in pairs:
            assert np.all(grid <= m.v + 1e-9), (grid, m.v)
            assert np.all(np.abs(m.v - m.w) <= nt.V_W_BOUND * (1.0 + np.abs(m.v))) and np.all(m.member >= -1e-6 * (1.0 + zmax))
        assert np.all(Y[:, inside].max(1) >= top.v - 0.05) and cm.v <= (top.v - h).min() + 1e-9


def test_the_file_holds_every_case():
    """every group and node of the recipes is in the file, attained to V_W_BOUND; sibling nodes are mostly empty; the point boxes
    enumerate to what a forward pass gives"""
    fx = nc.fixture()
    assert set(fx["groups"]) == set(nc.groups()) and set(fx["driver"]) == set(nc.DRIVER)
    assert fx["header"]["worst_v_minus_w"] <= nt.V_W_BOUND
    assert sum(len(nc.truth(g)) for g in nc.names("a")) == 18
    empties = sum(t["empty"] for g in nc.names("c") for t in nc.truth(g))
    assert 12 <= empties < 48
    for gname in nc.names("abe"):
        assert not any(t["empty"] for t in nc.truth(gname)) and all(t["depth"] >= 0.0 for t in nc.truth(gname))
    for gname in nc.names("d"):
        g, (full, flipped) = nc.groups()[gname], nc.truth(gname)
        assert flipped["empty"] and not full["empty"] and full["regions"] == 1
        z, y = rs.hidden64(g["net"], g["x0"][:, 0]), g["C"] @ xc.forward64(g["net"], g["x0"][:, 0])
        for got, want in ((full["vmax"], y), (full["vmin"], y), (full["zmax"], z), (full["zmin"], z)):
            assert np.all(np.abs(got - want) <= 1e-12 * (1.0 + np.abs(want)))
        assert abs(full["depth"] - np.abs(z).min()) <= 1e-12


# ---- the host routine against the file
@pytest.mark.parametrize("gname", nc.names("ab"))
def test_bounds_enclose_the_exact_ranges(gname):
    slack, *_ = nc.check_ranges(host, True, gname, _cache)
    assert slack >= -1.0


def test_sibling_nodes_and_the_infeasible_flag():
    """c: no non-empty node (beyond the margin) is flagged, a flagged node is empty (up to the margin), and the check is not vacuous"""
    empties = flagged = 0
    for gname in nc.names("c"):
        _, e, f, _ = nc.check_ranges(host, True, gname, _cache)
        empties, flagged = empties + e, flagged + f
    print(f"host: {flagged} of {empties} truly empty nodes flagged")
    assert flagged >= 1


@pytest.mark.parametrize("gname", nc.names("d"))
def test_point_boxes(gname):
    nc.check_points(host, True, gname)


def test_multipliers_of_deeper_layers():
    nc.check_deep_toys(host, True)


def test_the_yardstick_on_the_deep_toys():
    """R itself in fp64: the iterates of the toy, 2, 1.5, 1.05 and 1.00327 at 8 steps, wherever the forced neuron sits"""
    for gname in nc.names("e"):
        g = nc.groups()[gname]
        r = lambda T: rs.R(g["net"].Ms, g["lo"][:, 0], g["hi"][:, 0], g["assign"][:, 0], g["C"], T)
        assert r(0)["smax"][0] == 2.0 and abs(r(1)["smax"][0] - 1.5) <= 1e-12 and abs(r(2)["smax"][0] - 1.05) <= 1e-12
        assert abs(r(8)["smax"][0] - 1.00327) <= 1e-5 and r(8)["smax_plain"][0] == 2.0


def test_full_size_and_deep_nets_follow_the_yardstick():
    """b, d and the full-size nodes: float32 against R(float64) at 3 steps, as test_the_host_routine_follows_the_yardstick: smax_plain,
    smin and the clipped bounds to HOST_SLACK, smax never above smax_plain, the infeasible flag equal; full size is sound at x0"""
    nc.check_full_size_sound(host, True)
    for g in [nc.groups()[n] for n in nc.names("bd")] + [nc.full_size()]:
        nb = host(g["net"], g["lo"], g["hi"], g["assign"], g["C"], 3)
        for b in range(g["lo"].shape[1]):
            r = rs.R(g["net"].Ms, g["lo"][:, b], g["hi"][:, b], g["assign"][:, b], g["C"], 3)
            for got, want in ((nb.smax_plain[:, b], r["smax_plain"]), (nb.smin[:, b], r["smin"]), (nb.pre_lo[:, b], r["pre_lo"]), (nb.pre_hi[:, b], r["pre_hi"])):
                assert np.all(np.abs(got - want) <= xc.HOST_SLACK * (1.0 + np.abs(want))), (g["net"].xdims, b)
            assert np.all(nb.smax[:, b] <= nb.smax_plain[:, b]) and bool(nb.infeasible[b]) == r["infeasible"]


# ---- the driver against truth
@pytest.mark.parametrize("name", list(nc.DRIVER))
def test_the_driver_on_two_literals(name):
    checked, _, worst = nc.check_driver("host", name)
    assert checked >= 1 and worst <= xc.HOST_SLACK
