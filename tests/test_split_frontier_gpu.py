"""The split driver with frontier = "device" (CrownBounder.search, csrc/crown_search.hpp): the level loop of a bounds-only verifySplit on
the GPU with the frontier in device memory.  The specification is the Python loop: every comparison is between frontier = "host" and
frontier = "device", both with crown_backend = "resident" and sdp_per_level = 0, and asks for the same tree exactly and in order
(assert_same_tree of tests/test_split_resident_gpu.py)."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import vnnlib as vl
import crown_tanh_common as tc
from literal_common import assert_tiles, forward, instance, random_net
from test_split_cpu import NORMAL
from test_split_gpu import SDP_BETA, SDP_BOX, SDP_NET
from test_split_resident_gpu import TANH_H, assert_same_tree

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)
_state = {}


def both(net, lo, hi, literals, **options):
    """the host frontier's result (computed once per case) and the device frontier's"""
    chunk = options.pop("chunk", 4096)
    key = (id(net), lo.tobytes(), hi.tobytes(), tuple((n.tobytes(), float(h)) for n, h in literals), tuple(sorted(options.items())))
    if key not in _state:
        _state[key] = (net, na.verifySplit(net, lo, hi, literals, 0, OPTS, na.SplitOptions(crown_backend="resident", sdp_per_level=0, **options)))
    dev = na.verifySplit(net, lo, hi, literals, 0, OPTS,
                         na.SplitOptions(crown_backend="resident", sdp_per_level=0, frontier="device", chunk=chunk, **options))
    return _state[key][1], dev


def net2():
    """instance 2: the 5-20-20-20-5 net with the literal y_0 - y_4 <= s + 0.05 (c0 - s), which holds (513 boxes with literal bounds)"""
    it = instance("violated", "gpu")
    return it, it["s"] + 0.05 * (it["c0"] - it["s"])


def level_sizes(leaves):
    """boxes per level of a complete bisection tree from its leaves: the leaves of the level plus half the level below"""
    n = np.bincount([lf.depth for lf in leaves]).astype(float)
    for d in range(len(n) - 2, -1, -1):
        n[d] += n[d + 1] / 2
    return n


@pytest.mark.parametrize("which", ["holds", "violated"])
@pytest.mark.parametrize("options", [dict(), dict(literal_bounds=True), dict(literal_bounds=True, corner_points=True)])
def test_the_instances_walk_the_tree_of_the_host_frontier(which, options):
    it = instance(which, "gpu")
    host, dev = both(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], **options)
    print(f"{which} {options}: {host.verdict} after {host.visited} boxes; seconds host {host.seconds['total']:.4f} device {dev.seconds['total']:.4f}")
    if which == "holds" or options.get("corner_points"):
        assert host.verdict == which
    assert_same_tree(host, dev)


@pytest.mark.parametrize("chunk", [1, 7, 64, 4096])
def test_the_tree_does_not_depend_on_the_chunk(chunk):
    it, h = net2()
    host, dev = both(it["net"], it["lo"], it["hi"], [(it["normal"], h)], literal_bounds=True, max_boxes=1024, chunk=chunk)
    assert host.verdict == "holds" and host.visited > 256
    assert_same_tree(host, dev)


# The scan over a level longer than its tiles.  With the factor 0.005 the frontier never exceeds about 400 boxes on this net (the per-output
# bounds prove half of every level from depth 9 on), and no factor gives a level with more than 1 024 boxes still open after its proof
# test within max_boxes = 4096; a numpy prototype of the driver has, at the factor -0.025 (h below the sampled maximum: a centre refutes
# the clause at depth 13), levels of 612, 574, 774 and 1 090 boxes, all of them bounded: the scan then walks five tiles of 256 with a
# carried offset.  A level "holds" the open boxes that are its frontier; the condition below is on that number.
SCAN_FACTOR = -0.025


def test_a_level_longer_than_the_scan_tiles():
    it = instance("violated", "gpu")
    h = it["s"] + SCAN_FACTOR * (it["c0"] - it["s"])
    host, dev = both(it["net"], it["lo"], it["hi"], [(it["normal"], h)], max_boxes=4096, max_depth=24)
    sizes = level_sizes(dev.leaves)
    print(f"{dev.verdict} after {dev.visited} boxes; boxes per level {sizes.astype(int).tolist()}")
    assert dev.visited < 4096          # no box was kept from being bounded: the whole level went through the scan
    assert sizes.max() > 1024
    assert_same_tree(host, dev)


@pytest.mark.parametrize("ny,max_boxes", [(10, 1), (10, 2), (10, 200), (17, 1), (17, 200), (8, 200)])
def test_the_proof_test_sums_in_numpys_order_from_eight_outputs_on(ny, max_boxes):
    """numpy reduces the ny terms of a box's cheap bound pairwise (the terms are contiguous in memory: the bounder returns transposes): a
    plain ascending sum below 8 terms, eight interleaved partial sums from 8 on, a tail from 9 on and a second round from 16 on.  Dense
    normals and per-output bounds only, so that this sum is what decides and what Leaf.bound holds; max_boxes 1 and 2: the root as a leaf"""
    net = _state.setdefault(("wide", ny), random_net([3, 16, 16, ny], 100 + ny))
    nrm = np.random.default_rng(ny).normal(size=ny)
    lo, hi = -np.ones(3), np.ones(3)
    X = lo[:, None] + np.random.default_rng(0).random((3, 5000)) * (hi - lo)[:, None]
    s = float((nrm @ forward(net, X)).max())
    iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="gpu")
    c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
    host, dev = both(net, lo, hi, [(nrm, s + 0.3 * (c0 - s))], max_boxes=max_boxes)
    print(f"ny {ny}, max_boxes {max_boxes}: {host.verdict} after {host.visited} boxes, {len(host.leaves)} leaves")
    assert host.visited > 1 or max_boxes == 1
    assert_same_tree(host, dev)


@pytest.mark.parametrize("max_boxes", [1, 2, 3, 100, 101])
def test_the_budget_ends_in_the_middle_of_a_level(max_boxes):
    it, h = net2()
    host, dev = both(it["net"], it["lo"], it["hi"], [(it["normal"], h)], literal_bounds=True, max_boxes=max_boxes)
    assert dev.verdict == "unknown" and dev.visited == max_boxes
    assert_same_tree(host, dev)
    never = [lf for lf in dev.leaves if lf.proved_by is None and lf.literal is None]
    assert all(lf.bound is None for lf in never) and (len(never) > 0) == (max_boxes in (2, 100, 101))
    assert_tiles(dev.leaves, it["lo"], it["hi"])


@pytest.mark.parametrize("max_depth", [0, 3])
def test_max_depth_ends_the_search(max_depth):
    it, h = net2()
    host, dev = both(it["net"], it["lo"], it["hi"], [(it["normal"], h)], literal_bounds=True, max_depth=max_depth)
    assert dev.verdict == "unknown" and max(lf.depth for lf in dev.leaves) == max_depth
    assert_same_tree(host, dev)


def test_coordinates_that_cannot_be_split():
    it = instance("holds", "gpu")
    lo, hi = it["lo"].copy(), it["hi"].copy()
    lo[1] = hi[1] = 0.3
    host, dev = both(it["net"], lo, hi, [(it["normal"], it["h"])], literal_bounds=True)
    assert host.visited > 1
    assert_same_tree(host, dev)
    assert all(lf.lo[1] == 0.3 and lf.hi[1] == 0.3 for lf in dev.leaves)
    for x in (np.zeros(3), np.array([1.0, -1.0, 1.0])):
        host, dev = both(it["net"], x, x.copy(), [(it["normal"], it["h"])], literal_bounds=True, corner_points=True)
        assert dev.visited == 1 and dev.verdict == host.verdict
        assert_same_tree(host, dev)


# three literals on the 5-20-20-20-5 net: the 0.9 quantiles of y_0 - y_4, y_1 and -y_2 over 20 000 uniform points of the box; in the numpy
# prototype of the driver 9, 24 and 18 leaves are proved by the three literals within 1 024 boxes
CLAUSE = [(np.array([1.0, 0.0, 0.0, 0.0, -1.0]), 0.78786939), (np.array([0.0, 1.0, 0.0, 0.0, 0.0]), -0.30105643),
          (np.array([0.0, 0.0, -1.0, 0.0, 0.0]), 0.37880483)]


def test_a_clause_of_three_literals():
    it = instance("violated", "gpu")
    host, dev = both(it["net"], it["lo"], it["hi"], CLAUSE, literal_bounds=True, max_boxes=1024)
    by = np.bincount([lf.literal for lf in host.leaves if lf.proved_by == "crown"], minlength=3)
    print(f"{host.verdict} after {host.visited} boxes; leaves proved per literal {by.tolist()}")
    assert np.count_nonzero(by) >= 2
    assert_same_tree(host, dev)


@pytest.mark.parametrize("which", ["holds", "violated"])
def test_a_tanh_network(which):
    tanh = _state.setdefault("tanh", tc.tanh_copy(random_net([3, 17, 33, 4], 14)))
    host, dev = both(tanh, -np.ones(3), np.ones(3), [(np.array([1.0, 0.0, 0.0, -1.0]), TANH_H[which])], literal_bounds=True, corner_points=True,
                     max_boxes=128)
    assert host.verdict == which
    assert_same_tree(host, dev)


def test_a_second_search_allocates_nothing_and_bound_keeps_its_bits():
    it, h = net2()
    lo, hi = np.stack([it["lo"], 0.5 * it["lo"]], axis=1), np.stack([it["hi"], 0.25 * it["hi"]], axis=1)
    with na.CrownBounder(it["net"], it["normal"][None]) as cb:
        before = cb.bound(lo, hi)
        kw = dict(literal_bounds=True, corner_points=True, max_boxes=300, max_depth=24, chunk=64)
        first = cb.search(it["lo"], it["hi"], [h], **kw)
        info1 = cb.info()
        second = cb.search(it["lo"], it["hi"], [h], **kw)
        info2 = cb.info()
        after = cb.bound(lo, hi)
        assert (info2["device_allocations"], info2["network_uploads"], info2["device_bytes"]) == \
               (info1["device_allocations"], info1["network_uploads"], info1["device_bytes"])
        assert info1["network_uploads"] == 1 and info1["box_capacity"] == 64
        assert first["visited"] == second["visited"] == 300 and first["verdict"] == "unknown"
        for k in ("lo", "hi", "leaf_depth", "proved", "literal", "bound"):
            assert np.array_equal(first[k], second[k]), k
        for a, b in zip(before[:6] + tuple(before[6]), after[:6] + tuple(after[6])):
            assert np.array_equal(a, b)
        # the refusals that need a handle: nothing is allocated by a refused search
        for bad, msg in ((dict(lo=np.array([0.0, np.nan, 0, 0, 0])), "finite"), (dict(lo=2.0 * it["hi"]), "x1min must be <= x1max"),
                         (dict(hs=[np.inf]), "threshold"), (dict(max_boxes=2 ** 23), "2\\^31"), (dict(normals=it["normal"][None]), "normals")):
            args = dict(lo=it["lo"], hi=it["hi"], hs=[h], **kw)
            args.update(bad)
            with pytest.raises(na._lib.NnsdpError, match=msg):
                cb.search(args.pop("lo"), args.pop("hi"), args.pop("hs"), **args)
        assert cb.info() == dict(info2, bound_calls=info2["bound_calls"] + 1)
    with na.CrownBounder(it["net"]) as plain:
        for flag in ("literal_bounds", "corner_points"):
            with pytest.raises(na._lib.NnsdpError, match=flag):
                plain.search(it["lo"], it["hi"], [h], normals=it["normal"][None], max_boxes=4, **{flag: True})
        assert plain.info()["box_capacity"] == 0
        r = plain.search(it["lo"], it["hi"], [h], normals=it["normal"][None], max_boxes=4)
        assert r["visited"] == 4 and r["verdict"] == "unknown"


def test_the_final_sdp_stage():
    """the instance of test_only_the_sdp_can_prove_it (tests/test_split_gpu.py): h halfway between the root's SDP bound and its cheap bound"""
    wide = na.randomNetwork(SDP_NET["xdims"], sigma=SDP_NET["sigma"], seed=SDP_NET["seed"])
    lo, hi = SDP_BOX
    iv = na.makeIntervalsBatch(wide, lo[:, None], hi[:, None], backend="gpu")
    ymin, ymax = iv[4][:, 0], iv[5][:, 0]
    c0 = float(np.maximum(NORMAL * ymin, NORMAL * ymax).sum())
    sq = na.SafetyQuery(ffnet=wide, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_safety=na.QcSafety(S=vl.hplaneS(NORMAL, c0, wide)),
                        qc_activs=na.makeQcActivs(wide, lo, hi, SDP_BETA))
    rq, _, h0 = vl.reachForm(sq, ybounds=(ymin, ymax))
    plain = na.runQuery(rq, OPTS)
    rho = plain.objective_value + h0
    assert vl.isSolutionGood(plain) and rho < c0 - 1e-3 * (1.0 + abs(c0))
    h = 0.5 * (rho + c0)
    dev = dict(crown_backend="resident", frontier="device", max_boxes=1)
    no = na.verifySplit(wide, lo, hi, [(NORMAL, h)], SDP_BETA, OPTS, na.SplitOptions(sdp_per_level=0, **dev))
    assert no.verdict == "unknown" and no.sdp_solves == 0 and len(no.leaves) == 1 and no.leaves[0].proved_by is None
    assert no.leaves[0].literal == 0 and no.leaves[0].bound == c0
    yes = na.verifySplit(wide, lo, hi, [(NORMAL, h)], SDP_BETA, OPTS, na.SplitOptions(sdp_per_level=1, **dev))
    assert yes.verdict == "holds" and yes.visited == 1 and yes.sdp_solves == 1
    (lf,) = yes.leaves
    assert lf.proved_by == "sdp" and lf.literal == 0 and lf.bound <= h
    assert lf.soln.termination_status == "TARGET_CERTIFIED" and lf.soln.summary["lambda_max"] <= 1e-6
    assert yes.seconds["solve"] > 0 and yes.seconds["setup"] > 0
