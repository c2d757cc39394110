"""The five launches behind the projection (gather, A' product, M^-1 product, A product, multiplier update), bit for bit against the
digests recorded from the commit in front of the change that put the loads of a GEMV row in flight together (tools/tail_bits.py wrote
tests/golden/tail_bits_parent.json on that build, twice, with identical digests): the change keeps every floating-point operation and
its order, so the multipliers after 1, 9 and 60 iterations, the residuals of the check iteration behind them and a batch's objectives
are the same bytes.  The same gate holds for any later change to these launches that claims to move no operation.  Cases: W20-D10 beta 0 (every class of row, column and entry but
columns above 256 nonzeros), W10-D5 beta 3 Double and beta 0 (counts that are no multiple of 128), W10-D10 beta 2 Double (an even count), W40-D20 beta 0 for 9 iterations
(columns above 256 nonzeros, more than one GEMV group), each with eager launches, through the graph and through advance; W10-D5 beta 3
Double on a one-rank clique-sharded handle, eager and through advance (the sharded branch of the iteration: own-source gather, the
exchanged sum in the dual check, the update's element range, the resynchronised multiplier block; recorded on the commit in front of
the change that gave the five launches one argument block; with ONE rank the element range is everything and the exchanged sum is the
rank's own, so the digests equal the unsharded ones where the arithmetic agrees: the cases gate the BINDING of that branch's launches,
they are no coverage of the update's range handling - tests/test_sharded_two_ranks.py has that); and a SolverBatch of three members of different sizes (the batch kernels'
per-member guards)."""
import json
import os
import sys

import pytest

import helpers  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import tail_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(tail_bits.GOLDEN) as _f:
    _GOLDEN = json.load(_f)
_CASES = tail_bits.cases()


def test_every_case_has_a_recorded_digest():
    assert sorted(c[0] for c in _CASES) == sorted(_GOLDEN)
    assert len(_CASES) == 5 * 3 + 2 + 1


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_tail_bits_match_the_parent(case):
    want = _GOLDEN[case[0]]           # (a case without a record is an error, never a skip)
    got = tail_bits.run_case(case)
    assert sorted(got) == sorted(want), case[0]
    for key in sorted(want):
        assert got[key] == want[key], (case[0], key)
