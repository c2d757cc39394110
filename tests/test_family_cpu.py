"""Solver families, the part that needs no GPU: which queries may share one set-up (same_family), and the premise of sharing pinned
on the CPU oracle - two SDPs that differ in the output QC (and the last affine layer) only have the same scaled operator A, kept
set, cost, column scales and cost scale BIT FOR BIT; only z0 (and its norm) differs.  A later change of the normalisation that
breaks this makes sharing wrong, and fails here first."""
import copy

import numpy as np
import pytest

import helpers
import nnsdp_amd as na
import oracle_state as ost
from oracle import admm as oadmm, operator as oop


def _hplane(d, ang):
    return helpers.product_query(d, "hplane", normal=(np.cos(ang), np.sin(ang)))


def safety_S(n, off):
    """5 x 5 hyperplane safety set of a 2-in 2-out network: normal' y <= off"""
    S = np.zeros((5, 5))
    S[2:4, 4] = S[4, 2:4] = n
    S[4, 4] = -2.0 * off
    return S


def shifted_bias(q, shift):
    """q on a copy of its network whose output bias is shifted (what vnnlib.reachForm does per literal)"""
    Ms = [np.array(M, copy=True) for M in q.ffnet.Ms]
    Ms[-1][:, -1] += np.asarray(shift, dtype=float)
    q2 = copy.copy(q)
    q2.ffnet = na.FeedFwdNet(xdims=list(q.ffnet.xdims), Ms=Ms, activ=q.ffnet.activ)
    return q2


def test_same_family_accepts_output_only_variants():
    d = helpers.load_problem("W10-D5", 3)
    assert na.same_family(_hplane(d, 0.0), _hplane(d, 1.0))
    assert na.same_family(helpers.product_query(d, "safety", S=safety_S((1, 0), 50)), helpers.product_query(d, "safety", S=safety_S((0, 1), 80)))
    assert na.same_family(helpers.product_query(d, "circle"), helpers.product_query(d, "circle"))
    assert na.same_family(_hplane(d, 0.0), shifted_bias(_hplane(d, 1.0), (0.5, -0.25)))      # the last affine layer enters z0 only


def test_same_family_circle_and_ellipsoid_are_one_kind():
    """circle and ellipsoid give the gout generator the same coefficient (-0.5), the hyperplane -1"""
    d = helpers.load_problem("W10-D5", 3)
    assert na.same_family(helpers.product_query(d, "circle"), helpers.product_query(d, "ellipsoid"))


def test_same_family_rejects_anything_that_enters_the_generators():
    d = helpers.load_problem("W10-D5", 3)
    q0 = _hplane(d, 0.0)
    assert not na.same_family(q0, _hplane(helpers.load_problem("W10-D5", 0), 1.0))          # beta
    d2 = dict(d)
    d2["acymax"] = d["acymax"].copy()
    d2["acymax"][7] += 1e-9
    assert not na.same_family(q0, _hplane(d2, 1.0))                                           # one interval bound
    d3 = dict(d)
    d3["M1"] = np.array(d["M1"], copy=True)
    d3["M1"][2, 3] += 1e-12
    assert not na.same_family(q0, _hplane(d3, 1.0))                                           # one weight of a hidden layer
    d4 = dict(d)
    d4["x1min"] = d["x1min"] - 1e-3
    assert not na.same_family(q0, _hplane(d4, 1.0))                                           # the input box
    assert not na.same_family(q0, helpers.product_query(d, "ellipsoid"))                      # out_kind hyperplane vs ellipsoid
    assert not na.same_family(q0, helpers.product_query(d, "safety", S=safety_S((1, 0), 50)))  # query kind
    qt = copy.copy(q0)
    qt.ffnet = na.FeedFwdNet(xdims=list(q0.ffnet.xdims), Ms=q0.ffnet.Ms, activ=na.methods.TanhActiv)
    assert not na.same_family(q0, qt)                                                         # activation


def _scaled(q, mode):
    return oadmm.ScaledProblem(oop.build_operator(ost.mirror_query(q), mode, normalize=True, merge_identical=True))


def _premise_cases():
    d40 = helpers.load_problem("W40-D20", 0)
    d5 = helpers.load_problem("W10-D5", 3)
    h0 = _hplane(d40, 0.0)
    return {
        "W40-D20-b0-single-hplanes": ("single", [h0, _hplane(d40, 2 * np.pi / 6), shifted_bias(_hplane(d40, 4 * np.pi / 6), (0.3, -0.7))]),
        "W10-D5-b3-single-safety": ("single", [helpers.product_query(d5, "safety", S=safety_S((1, 0), 50)),
                                               helpers.product_query(d5, "safety", S=safety_S((0, 1), 80))]),
        "W40-D20-b0-single-ellipsoid-circle": ("single", [helpers.product_query(d40, "ellipsoid"), helpers.product_query(d40, "circle")]),
        "W20-D10-b0-path-hplanes": ("path", [_hplane(helpers.load_problem("W20-D10", 0), a) for a in (0.0, 2.0)]),
        "W10-D10-b7-single-hplanes": ("single", [ost.net_hplane_query("W10-D10", 7, n) for n in ((0.6, 0.8), (-0.8, 0.6))]),
    }


@pytest.mark.parametrize("case", sorted(_premise_cases()))
def test_family_members_have_one_scaled_operator_on_the_oracle(case):
    mode, qs = _premise_cases()[case]
    assert all(na.same_family(qs[0], q) for q in qs[1:])
    P0 = _scaled(qs[0], mode)
    for q in qs[1:]:
        P = _scaled(q, mode)
        assert np.array_equal(P.keep, P0.keep)
        assert (P.A != P0.A).nnz == 0 and np.array_equal(P.A.indptr, P0.A.indptr) and np.array_equal(P.A.data, P0.A.data)
        assert np.array_equal(P.c, P0.c) and np.array_equal(P.ecol, P0.ecol) and P.cscale == P0.cscale
        assert P.z0.shape == P0.z0.shape and not np.array_equal(P.z0, P0.z0)
