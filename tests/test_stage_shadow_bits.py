"""The refinement stage of the ping-pong projection kernel, bit for bit against the digests recorded from the commit in front of the
change that moved its scalar phases into the matrix products' shadow (tools/stage_bits.py wrote tests/golden/stage_bits_parent.json
on that build): only the wave that runs a chain or takes a partial sum, and when, changed - every tile, every order of summation and
every decision stayed - so W, V, the outcome counts and the state words are the same bytes.  Cases: every tile count (n = 41 .. 96,
full and ragged edges), mixed sizes in one launch, a converged / a stepping / a rejected move, a visit with and one without the Gram
product (two launches on carried state), one and two workgroups per block, and the exact rotation of one unresolvable pair."""
import json
import os
import sys

import pytest

import helpers  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stage_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(stage_bits.GOLDEN) as _f:
    _GOLDEN = json.load(_f)
_CASES = stage_bits.cases()


def test_every_case_has_a_recorded_digest():
    assert sorted(c[0] for c in _CASES) == sorted(_GOLDEN)
    assert len(_CASES) == 3 * (9 + 3 + 6) + 6 + 3


def test_the_cases_reach_every_path():
    """(of the record itself) the three moves end as intended, and the second launch of a stepping case ran without the Gram product"""
    firsts = {cid: v[0]["counts"] for cid, v in _GOLDEN.items()}
    assert all(c[0] == sum(c) for cid, c in firsts.items() if cid.endswith("-eta0"))
    assert all(c[1] == sum(c) for cid, c in firsts.items() if cid.endswith("-eta1e-06"))
    assert all(c[2] + c[4] == sum(c) for cid, c in firsts.items() if cid.endswith("-eta0.0001"))       # rejected: checked step or sweeps
    assert all(c[2] == sum(c) for cid, c in firsts.items() if "-refine1-" in cid)                        # no checked form: the sweeps
    assert all(c[1] == 1 for cid, c in firsts.items() if cid.startswith("pivot"))
    for cid, v in _GOLDEN.items():
        if cid.endswith("-eta1e-06"):
            assert all(g == 3 for g in v[0]["gram_credit"]) and all(g == 2 for g in v[1]["gram_credit"]), cid


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_stage_bits_match_the_parent(case):
    want = _GOLDEN[case[0]]           # (a case without a record is an error, never a skip)
    got = stage_bits.run_case(case)
    assert len(got) == len(want)
    for visit, (g, w) in enumerate(zip(got, want)):
        assert g["counts"] == w["counts"], (case[0], visit, g["counts"], w["counts"])
        for key in ("W", "V", "outcome", "state"):
            assert g[key] == w[key], (case[0], visit, key)
