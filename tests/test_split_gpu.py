"""The split driver (nnsdp_amd/split.py) on the GPU: batched CROWN bounds from csrc/crown_batch.hpp, centre evaluation through
nnsdp_eval_network, and the SDP stage (reach form with a target, decided early, one solver family per box).  The instance of
tests/test_split_cpu.py: W10-D5 fixture, box [0.5, 1.5]^2, literal y_0 <= h with h from the sampled maximum s and the root cheap bound c0."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import vnnlib as vl
from test_split_cpu import HI, HOST, LO, NORMAL, assert_tiles, net, setting

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)
_state = {}


def h_holds():
    s, c0 = setting()
    return s + 0.25 * (c0 - s)


def crown_only():
    if "crown" not in _state:
        _state["crown"] = na.verifySplit(net(), LO, HI, [(NORMAL, h_holds())], 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=0))
    return _state["crown"]


def test_holds_with_the_gpu_bounds():
    """the fp64 bounds of the kernel are not the float32 ones of the host routine: a box at the threshold may flip, hence +-2"""
    res = crown_only()
    host = na.verifySplit(net(), LO, HI, [(NORMAL, h_holds())], 0, OPTS, na.SplitOptions(**HOST))
    print(f"visited: gpu {res.visited}, host {host.visited}; seconds {res.seconds}")
    assert res.verdict == "holds" and host.verdict == "holds"
    assert_tiles(res.leaves)
    assert all(lf.proved_by == "crown" for lf in res.leaves)
    assert abs(res.visited - host.visited) <= 2


def test_sdp_stage_proves_boxes_the_bounds_leave_open():
    h = h_holds()
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=26))
    by = [lf.proved_by for lf in res.leaves]
    print(f"visited {res.visited} (bounds alone: {crown_only().visited}), {res.sdp_solves} SDPs, leaves by crown {by.count('crown')} by sdp {by.count('sdp')}, "
          f"seconds {res.seconds}")
    assert res.verdict == "holds" and res.sdp_solves > 0
    assert_tiles(res.leaves)
    assert res.visited <= crown_only().visited
    rng = np.random.default_rng(7)
    for lf in res.leaves:
        assert lf.proved_by in ("crown", "sdp") and lf.bound <= h
        if lf.proved_by == "sdp":
            s = lf.soln
            assert s.termination_status == "TARGET_CERTIFIED" and s.summary["lambda_max"] <= 1e-6
            assert all(np.all(s.values[k] >= 0.0) for k in ("γin", "γout", "γac1", "γac2"))
            X = lf.lo[:, None] + rng.random((2, 2000)) * (lf.hi - lf.lo)[:, None]
            assert np.all(NORMAL @ na.evalFeedFwdNet(net(), X) <= h)


# an instance on which the relaxation over the whole box is far tighter than the CROWN bound: the fp64 interior-point oracle
# (oracle/ipm.py) has the root SDP bound at 0.893, the root cheap bound is 4.76, the sampled maximum 0.535
SDP_NET = dict(xdims=[2, 6, 6, 2], sigma=1.0, seed=1)
SDP_BOX = (-np.ones(2), np.ones(2))
SDP_BETA = 0


def test_only_the_sdp_can_prove_it():
    """h between the root box's converged SDP bound (one plain solve made here) and its cheap bound c0: the bounds alone leave the root
    open, one SDP on it proves it - the two stages are wired to each other"""
    wide = na.randomNetwork(SDP_NET["xdims"], sigma=SDP_NET["sigma"], seed=SDP_NET["seed"])
    lo, hi = SDP_BOX
    iv = na.makeIntervalsBatch(wide, lo[:, None], hi[:, None], backend="gpu")
    ymin, ymax = iv[4][:, 0], iv[5][:, 0]
    c0 = float(np.maximum(NORMAL * ymin, NORMAL * ymax).sum())
    qa = na.makeQcActivs(wide, lo, hi, SDP_BETA)
    sq = na.SafetyQuery(ffnet=wide, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_safety=na.QcSafety(S=vl.hplaneS(NORMAL, c0, wide)), qc_activs=qa)
    rq, _, h0 = vl.reachForm(sq, ybounds=(ymin, ymax))
    plain = na.runQuery(rq, OPTS)
    rho = plain.objective_value + h0
    print(f"root box: SDP bound {rho:.6f} ({plain.termination_status}), cheap bound {c0:.6f}")
    assert vl.isSolutionGood(plain) and rho < c0 - 1e-3 * (1.0 + abs(c0)), "the instance needs an SDP bound below the CROWN bound"
    h = 0.5 * (rho + c0)
    no = na.verifySplit(wide, lo, hi, [(NORMAL, h)], SDP_BETA, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=0, max_boxes=1))
    assert no.verdict == "unknown" and no.sdp_solves == 0 and no.leaves[0].proved_by is None
    yes = na.verifySplit(wide, lo, hi, [(NORMAL, h)], SDP_BETA, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=1, max_boxes=1))
    assert yes.verdict == "holds" and yes.visited == 1 and yes.sdp_solves == 1
    (lf,) = yes.leaves
    X = lo[:, None] + np.random.default_rng(3).random((2, 20000)) * (hi - lo)[:, None]
    assert lf.proved_by == "sdp" and lf.literal == 0 and float((NORMAL @ na.evalFeedFwdNet(wide, X)).max()) <= lf.bound <= h
    assert lf.soln.termination_status == "TARGET_CERTIFIED" and yes.seconds["solve"] > 0 and yes.seconds["setup"] > 0
    # the certificate of an "sdp" leaf, on a leaf that is known to exist (on the W10-D5 instance above the SDP stage may prove nothing:
    # its root SDP bound is the CROWN bound to seven digits)
    assert lf.soln.summary["lambda_max"] <= 1e-6
    assert all(np.all(lf.soln.values[k] >= 0.0) for k in ("γin", "γout", "γac1", "γac2"))
    assert np.all(NORMAL @ na.evalFeedFwdNet(wide, X[:, :2000]) <= h)


def test_violated_through_the_gpu_centre_evaluation():
    s, _ = setting()
    h = s - 0.1 * abs(s)
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=0))
    assert res.verdict == "violated" and np.all(res.witness >= LO) and np.all(res.witness <= HI)
    assert NORMAL @ na.evalFeedFwdNet(net(), res.witness) > h
    more = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=0, samples=8))
    assert more.verdict == "violated" and NORMAL @ na.evalFeedFwdNet(net(), more.witness) > h


def test_vnnlib_spec_decided_only_by_splitting():
    """unsafe set y_0 >= c with the literal's offset c - 1e-4 at h = s + 0.25 (c0 - s): not certified on the whole box (the spec ends
    "unsafe" as before), decided by the bisection"""
    c = h_holds() + vl.SPEC_EPS
    spec = f"(assert (>= X_0 0.5))(assert (<= X_0 1.5))(assert (>= X_1 0.5))(assert (<= X_1 1.5))(assert (>= Y_0 {c!r}))"
    opts = na.AdmmSdpOptions(max_iters=3000, eps_rel=1e-5)
    solns, nq, whole = vl.verifyAcasSpec(net(), spec, 0, opts, via_reach=True, decide_early=True)
    assert (nq, len(solns), whole) == (1, 1, "unsafe") and type(whole) is str
    solns, nq, status = vl.verifyAcasSpec(net(), spec, 0, opts, via_reach=True, decide_early=True, split=na.SplitOptions(max_boxes=64, crown_backend="gpu"))
    print(f"split: {status.splits[0].verdict} after {status.splits[0].visited} boxes, {status.splits[0].sdp_solves} SDPs")
    assert status == "safe" and status.witness is None and [r.verdict for r in status.splits] == ["holds"]
    assert 1 < status.splits[0].visited <= 64
