"""The two projected-gradient optimisers of the literal bounds - the slopes (k_crown_alpha, lits_alpha) and the multipliers of a ReLU-split
node (k_crown_beta, make_intervals_nodes) - bit for bit against digests recorded with tools/crown_opt_bits.py
(tests/golden/crown_opt_bits_parent.json) on the build in which each of the four carried its own copy of the loop.  The gate of any
change that only moves their code (csrc/crown_opt.hpp, the helpers of csrc/intervals.hpp): the same operations in the same order, so
the same bytes.  The cases are those of tests/test_crown_alpha_gpu.py and tests/test_relu_split_gpu.py (1, 7, 17 and 64 literals: one, two
and four row tiles with a ragged last one; widths 17, 33, 20 and 64; n0 = 1; K = 2 and 3; a point box and one of half-width 1e-6, where the loop
leaves at once; T = 0) and the all-zero assignment at T = 1, which takes the stationary break.
The host section was recorded on the same build.  Its slopes digests cover what makeIntervalsBatch returns (with smax_plain, alpha and
best_step) and the routine's own fifteen arrays (crown_alpha_common.raw_host), so an iterate that loses to the plain pass is held too.
The library's host code is compiled without -march and without fast-math; the record was made on a machine without a GPU and the
GPU machine reproduces it."""
import json
import os
import sys

import pytest

import helpers  # noqa: F401
import crown_alpha_common as ca
import relu_split_common as rs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import crown_opt_bits as cob  # noqa: E402

with open(cob.GOLDEN) as _f:
    _GOLDEN = json.load(_f)
_got = {}


def _digests(section):
    """every digest of a section, computed once"""
    if section not in _got:
        _got[section] = cob.gpu_digests() if section == "gpu" else cob.host_digests()
    return _got[section]


def test_every_case_has_a_recorded_digest():
    ids = cob.case_ids()
    slopes = [f"slopes-{n}-T{T}{a0}" for n in range(len(ca.cases())) for T in ca.STEPS for a0 in ("", "-alpha0")]
    nodes = [f"nodes-{n}-T{T}" for n in range(len(rs.NETS)) for T in rs.STEPS] + [f"nodes-{n}-free-T1" for n in range(len(rs.NETS))] + \
        ["nodes-0-nlit17-T3", "nodes-1-nlit64-T3"]
    assert sorted(ids) == sorted(slopes + nodes) and len(ids) == len(set(ids)) == 11 * 4 * 2 + 3 * 5 + 3 + 2
    assert sorted(_GOLDEN) == ["gpu", "host"]
    for section in ("gpu", "host"):
        assert sorted(_GOLDEN[section]) == sorted(ids), section


def test_the_cases_hold_the_shapes():
    """(of the case list) the literal counts, widths and step counts that the shared body can go wrong at"""
    shapes = {(tuple(net.xdims), Cm.shape[0], lo.shape[1]) for net, lo, _, Cm in ca.cases()}
    assert {s[1] for s in shapes} == {1, 7, 17, 64} and {s[0] for s in shapes} == {(3, 17, 33, 4), (1, 64, 64, 2), (5, 20, 5)}
    assert ((3, 17, 33, 4), 7, 1) in shapes
    assert 0 in ca.STEPS and 0 in rs.STEPS and max(rs.STEPS) == 16
    lo, hi = ca.cases()[0][1:3]
    assert (hi[:, 0] == lo[:, 0]).all() and float((hi[:, 1] - lo[:, 1]).max()) < 2.1e-6          # half-width 1e-6


@pytest.mark.parametrize("cid", cob.case_ids())
def test_the_host_routines_match_the_parent(cid):
    assert _digests("host")[cid] == _GOLDEN["host"][cid]          # (a case without a record is an error, never a skip)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", cob.case_ids())
def test_the_kernels_match_the_parent(cid):
    assert _digests("gpu")[cid] == _GOLDEN["gpu"][cid]
