"""Exact ranges over the nodes of a ReLU split as ground truth, on the GPU: nnsdp_crown_bound_nodes (csrc/crown_relu_split.hpp:
k_crown_nodes, k_crown_beta) against tests/golden/node_ranges.json on every group of tests/node_truth_common.py (nets with three and
four hidden layers, forced neurons in every layer, sibling nodes that are mostly empty, point boxes), against the yardstick `R` on the
deep nets and at full size (64-64-16-64, 64 literals: n0 = 64), and the driver verifyReluSplit with crown_backend="resident" on
two-literal clauses with its closed leaves checked by enumeration of their nodes.  The truth is read from the file; a call takes at
most 12 nodes."""
import numpy as np
import pytest

import nnsdp_amd as na
import node_truth_common as nc
import relu_split_common as rs

_cache = {}


def gpu(net, lo, hi, assign, Cm, steps):
    with na.CrownBounder(net, Cm) as bd:
        return bd.bound_nodes(lo, hi, assign, steps=steps)


@pytest.mark.gpu
@pytest.mark.parametrize("gname", nc.names("ab"))
def test_bounds_enclose_the_exact_ranges(gname):
    slack, *_ = nc.check_ranges(gpu, False, gname, _cache)
    assert slack >= -1.0


@pytest.mark.gpu
def test_sibling_nodes_and_the_infeasible_flag():
    """c: no non-empty node (beyond the margin) is flagged, a flagged node is empty (up to the margin), and the check is not vacuous"""
    empties = flagged = 0
    for gname in nc.names("c"):
        _, e, f, _ = nc.check_ranges(gpu, False, gname, _cache)
        empties, flagged = empties + e, flagged + f
    print(f"resident: {flagged} of {empties} truly empty nodes flagged")
    assert flagged >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("gname", nc.names("d"))
def test_point_boxes(gname):
    nc.check_points(gpu, False, gname)


@pytest.mark.gpu
def test_multipliers_of_deeper_layers():
    nc.check_deep_toys(gpu, False)


@pytest.mark.gpu
@pytest.mark.parametrize("T", nc.STEPS)
@pytest.mark.parametrize("gname", nc.names("bd"))
def test_deep_nets_against_the_yardstick(gname, T):
    """smax, uA, ub0 within 8 r of R(long double), best_step, the clear branching neurons and the infeasible flag equal"""
    rs.check_yardstick(nc.groups()[gname], nc.run_group(gpu, gname, T, _cache), T)


@pytest.mark.gpu
def test_full_size_against_the_yardstick():
    """64-64-16-64 with 64 literals, T = 3: every dimension loop of both kernels at its maximum, the input staging and the four-tile
    input product at n0 = 64; sound at x0 as well"""
    nb = nc.check_full_size_sound(gpu, False)
    rs.check_yardstick(nc.full_size(), nb, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nc.DRIVER))
def test_the_driver_on_two_literals(name):
    """the closed leaves are enumerated when the test runs: a seeded third of the "bound" leaves and every "infeasible" one, to keep the
    test at a few seconds; tests/test_node_truth_cpu.py checks every leaf of the host backend's trees"""
    checked, _, worst = nc.check_driver("resident", name, leaf_share=3)
    assert checked >= 1 and worst <= 1e-6
