"""The MFMA chains of the ping-pong projection kernel where one wave owns several tiles - V update, E~^2 product, reconstruction - bit
for bit against digests recorded with tools/stage_interleave_bits.py (tests/golden/stage_interleave_bits_parent.json) on the build
whose waves run those chains in turn.  The gate of any change that only reorders independent instructions of one wave (running the
chains side by side was measured against this record, gave the same bytes and was slower: DESIGN.md section 5): a tile's
accumulator sees the same products in the same order, so W, V, the outcome counts and the state words are the same bytes.
What tests/test_stage_shadow_bits.py does not pin: 1, 2 and 3 chains per wave in the V update (n = 41 / 49, 65, 85 / 96) against
reconstructions of 0, 1, 3, 4, 5 and about n / 2 selected eigenpairs from either side of the spectrum, all five sizes in one launch,
each with no helper workgroup and with five, and two solvers in lockstep.  The record is not the only witness: every projection is
also held to LAPACK (numpy.linalg.eigh through the oracle) at the level tests/test_refine_projection.py uses - 30 x tol |A| for a
block that took the step, tol |A| otherwise."""
import json
import os
import sys

import numpy as np
import pytest

import helpers  # noqa: F401
from oracle import admm as oadmm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stage_interleave_bits as sib  # noqa: E402

pytestmark = pytest.mark.gpu

with open(sib.GOLDEN) as _f:
    _GOLDEN = json.load(_f)
_CASES = sib.cases()
_RUNS = [(c, s) for c in _CASES for s in sib.SPLITS]
_REF = {}


def _lapack(cid, visit, mats):
    """LAPACK's projections of a launch's matrices, computed once per case (the launches with and without helpers share them)"""
    key = (cid, visit)
    if key not in _REF:
        _REF[key] = [oadmm.project_psd(A) for A in mats]
    return _REF[key]


def test_every_case_has_a_recorded_digest():
    assert sorted([f"{c[0]}-split{s}" for c, s in _RUNS] + ["lockstep"]) == sorted(_GOLDEN)
    assert len(_CASES) == 5 * 6 * 2 + 2


def test_the_cases_reach_the_chains():
    """(of the record and the case list) every block of every launch took the unchecked step - V update, E~^2 and reconstruction all
    ran - the second launch without the Gram product; the selected counts are the ones the issue names, on the smaller side"""
    for key, v in _GOLDEN.items():
        if key == "lockstep":
            continue
        assert all(r["counts"][1] == sum(r["counts"]) for r in v), key
        assert all(g == 3 for g in v[0]["gram_credit"]) and all(g == 2 for g in v[1]["gram_credit"]), key
    for n in sib.SIZES:
        assert [sib.nsel_of(n, k, "pos")[0] for k in sib.SELECT] == [0, 1, 3, 4, 5, n // 2]
        for k in sib.SELECT:
            sel, p, q = sib.nsel_of(n, k, "pos")
            assert sel == p <= q and p + q == n
            sel, p, q = sib.nsel_of(n, k, "neg")
            assert sel == q < p and p + q == n
    tiles = [((n + 15) // 16) ** 2 for n in sib.SIZES]
    assert [(t + 15) // 16 for t in tiles] == [1, 1, 2, 3, 3]                              # chains per wave in the V update
    assert [((n + 15) // 16) * ((n + 15) // 16 + 1) // 2 for n in sib.SIZES] == [6, 10, 15, 21, 21]      # lower tiles


@pytest.mark.parametrize("case,split", _RUNS, ids=[f"{c[0]}-split{s}" for c, s in _RUNS])
def test_interleaved_chains_match_the_parent_and_lapack(case, split):
    want = _GOLDEN[f"{case[0]}-split{split}"]           # (a case without a record is an error, never a skip)
    kept = []
    got = sib.run_case(case, split, keep=kept)
    assert len(got) == len(want) == 2
    for visit, (g, w) in enumerate(zip(got, want)):
        assert g["counts"] == w["counts"], (case[0], visit, g["counts"], w["counts"])
        for key in ("W", "V", "outcome", "state"):
            assert g[key] == w[key], (case[0], visit, key)
    for visit, (mats, W, oc) in enumerate(kept):
        stepped = oc[1] + oc[4] > 0
        for A, Wk, Wx in zip(mats, W, _lapack(case[0], visit, mats)):
            err = np.linalg.norm(Wk - Wx) / np.linalg.norm(A)
            assert err <= (30 * sib.TOL if stepped else sib.TOL), (case[0], visit, len(A), err)


def test_two_solvers_in_lockstep_match_the_parent_and_the_single_solver():
    """a two-member SolverBatch (the batch form of the kernel) after 60 plain iterations of the smallest fixture: the members carry
    the same query, so the same bytes; they and the single solver reproduce the parent's bytes"""
    members, single = sib.run_lockstep()
    assert np.array_equal(members[0], members[1])
    got = sib.lockstep_digests(members, single)
    assert got == _GOLDEN["lockstep"]
    # The batch handle sums the same products in another order in its M^-1 and sparse products, so a member is not the single solver
    # bit for bit.  The ADMM map is non-expansive, so the differences of the iterations add: per iteration a few dozen roundings of
    # the largest multiplier at most (64 eps |nu|_max allowed; recorded on the parent: 8.0e-15 of 13.2 after 60 iterations)
    diff, scale = float(np.abs(members[0] - single).max()), float(np.abs(single).max())
    print("largest difference between a member and the single solver:", diff, "of", scale)
    assert diff <= sib.LOCKSTEP[2] * 64 * np.finfo(np.float64).eps * scale
