"""The split driver with crown_backend="resident": one CrownBounder (network kept on the GPU) for the bound and refutation steps of a
whole verifySplit.  On ReLU networks it is crown_backend="gpu" bit for bit; on a Tanh network, which "gpu" refuses, it walks the tree
of the float32 host backend when no decision of that tree is within float32 reach of the threshold."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import split as sp
import crown_tanh_common as tc
from literal_common import instance, random_net
from test_split_cpu import HI, LO, NORMAL, net, setting

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)


def assert_same_tree(a, b):
    assert (a.verdict, a.visited, a.sdp_solves, len(a.leaves)) == (b.verdict, b.visited, b.sdp_solves, len(b.leaves))
    assert (a.witness is None) == (b.witness is None) and (a.witness is None or np.array_equal(a.witness, b.witness))
    for la, lb in zip(a.leaves, b.leaves):
        assert np.array_equal(la.lo, lb.lo) and np.array_equal(la.hi, lb.hi) and la.depth == lb.depth
        assert (la.proved_by, la.literal, la.bound) == (lb.proved_by, lb.literal, lb.bound)


@pytest.mark.parametrize("which", ["holds", "violated"])
@pytest.mark.parametrize("options", [dict(), dict(literal_bounds=True, corner_points=True), dict(samples=4)])
def test_relu_instances_walk_the_tree_of_the_gpu_backend(which, options):
    it = instance(which, "gpu")
    runs = [na.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, OPTS,
                           na.SplitOptions(crown_backend=backend, sdp_per_level=0, **options)) for backend in ("gpu", "resident")]
    print(f"{which} {options}: {runs[0].verdict} after {runs[0].visited} boxes; crown seconds gpu {runs[0].seconds['crown']:.4f} "
          f"resident {runs[1].seconds['crown']:.4f}")
    if which == "holds" or options.get("corner_points"):      # (the centres alone may not find the violation within max_boxes)
        assert runs[0].verdict == which
    assert_same_tree(*runs)


def test_relu_instance_with_the_sdp_stage():
    s, c0 = setting()
    h = s + 0.25 * (c0 - s)
    runs = [na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, OPTS, na.SplitOptions(crown_backend=backend, sdp_per_level=2, literal_bounds=True))
            for backend in ("gpu", "resident")]
    print(f"{runs[0].verdict} after {runs[0].visited} boxes and {runs[0].sdp_solves} SDPs")
    assert runs[0].verdict == "holds" and runs[0].sdp_solves > 0
    assert_same_tree(*runs)


# Tanh copy of the 3-17-33-4 net of literal_common on [-1, 1]^3, literal y_0 - y_3 <= h.  The maximum of the literal is 0.02267, at a
# corner of the box.  The thresholds were chosen on the CPU with the host backend so that no box it visits has a bound within
# 1e-4 (1 + |h|) of h, float32 against fp64 then cannot change the tree: the smallest |bound - h| over the visited boxes was 5.675e-3 at
# h = 0.11 ("holds", 37 boxes) and 1.156 at h = 0.02 ("violated" at the first box's corner, which exceeds h by 2.7e-3).
TANH_H = {"holds": 0.11, "violated": 0.02}


@pytest.mark.parametrize("which", ["holds", "violated"])
def test_a_tanh_network_walks_the_tree_of_the_host_backend(which, monkeypatch):
    tanh = tc.tanh_copy(random_net([3, 17, 33, 4], 14))
    nrm, h = np.array([1.0, 0.0, 0.0, -1.0]), TANH_H[which]
    lo, hi = -np.ones(3), np.ones(3)
    both = dict(sdp_per_level=0, literal_bounds=True, corner_points=True, max_boxes=128)
    with pytest.raises(na._lib.NnsdpError, match="Tanh"):
        na.verifySplit(tanh, lo, hi, [(nrm, h)], 0, OPTS, na.SplitOptions(crown_backend="gpu", **both))
    bounds, orig = [], na.frontend.makeIntervalsBatch

    def recording(net_, lo_, hi_, **kw):
        r = orig(net_, lo_, hi_, **kw)
        bounds.append(np.minimum(np.maximum(nrm[:, None] * r[4], nrm[:, None] * r[5]).sum(axis=0), r[6].smax[0]))
        return r

    monkeypatch.setattr(na.frontend, "makeIntervalsBatch", recording)
    host = na.verifySplit(tanh, lo, hi, [(nrm, h)], 0, OPTS, na.SplitOptions(crown_backend="host", **both))
    gap = float(np.abs(np.concatenate(bounds) - h).min())
    res = na.verifySplit(tanh, lo, hi, [(nrm, h)], 0, OPTS, na.SplitOptions(crown_backend="resident", **both))
    print(f"{which}: host {host.verdict} after {host.visited} boxes, resident {res.verdict} after {res.visited}; smallest |bound - h| {gap:.3e}")
    assert gap >= 1e-4 * (1.0 + abs(h)), "the instance no longer keeps its decisions away from the threshold"
    assert host.verdict == which and host.visited <= 128
    assert (res.verdict, res.visited) == (host.verdict, host.visited)
    if which == "violated":
        assert float(nrm @ na.evalFeedFwdNet(tanh, res.witness)) > h


def test_the_bounder_is_closed_on_every_way_out(monkeypatch):
    live = []

    class Counted(na.CrownBounder):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            live.append(self)

    monkeypatch.setattr(na.frontend, "CrownBounder", Counted)
    it = instance("violated", "gpu")
    res = na.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, OPTS, na.SplitOptions(crown_backend="resident", sdp_per_level=0, corner_points=True))
    assert res.verdict == "violated" and len(live) == 1 and live[0]._h is None

    def failing(*a, **kw):
        raise RuntimeError("the SDP stage failed")

    monkeypatch.setattr(sp, "_solve_boxes", failing)
    it = instance("holds", "gpu")
    with pytest.raises(RuntimeError, match="SDP stage"):
        na.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, OPTS, na.SplitOptions(crown_backend="resident", sdp_per_level=2))
    assert len(live) == 2 and live[1]._h is None
    with pytest.raises(ValueError, match="closed"):
        live[1].bound(it["lo"][:, None], it["hi"][:, None])
