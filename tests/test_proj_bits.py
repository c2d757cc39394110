"""Every variant of the projection kernel, bit for bit against the digests recorded from the commit in front of the change that made
proj_body's shared phases functions over a per-block context (tools/proj_bits.py wrote tests/golden/proj_bits_parent.json on that
build): the change moved code between functions - every floating-point operation kept its order, every barrier its place - so W, the
eigenvalues, V, the outcome counts and the state words are the same bytes.  Cases: a cold launch per instantiation plan_projection
reaches under NNSDP_PROJ_ALG unset, 0, 2, 3 and 4 (smallest, largest and an odd size of its range, and a 1 x 1 block); warm launches on
carried bases and state (two visits; a converged, a 1e-6 and a 1e-4 move) of the packed variant with its stage off, on and checked,
of the systolic and of the round-robin variant with V in LDS and in HBM.  The ping-pong stage has tests/test_stage_shadow_bits.py.
Batch cases (recorded on the commit that added them, whose kernels are that record's): the batched form k_proj_jacobi_b through a
two-member SolverBatch of one query in lockstep - W20-D10 and W40-D20 with the planner's choice (ping-pong RPW 5 / 6, 3000
iterations: past the cold sweeps, the stage accepting blocks) and with round robin and the systolic variant forced (200 iterations);
the members' multipliers are the same bytes, and the recorded ones.  tools/proj_bits.py names the batch instantiations out of reach."""
import json
import os
import sys

import pytest

import helpers  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import proj_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(proj_bits.GOLDEN) as _f:
    _GOLDEN = json.load(_f)
_CASES = proj_bits.cases()


def test_every_case_has_a_recorded_digest():
    assert sorted(c[0] for c in _CASES) == sorted(_GOLDEN)
    assert len(_CASES) == (7 + 4 + 6 + 6 + 4) + 3 * (4 * 3 + 6) + (2 + 3)


def test_the_warm_cases_reach_the_stage_and_the_sweeps():
    """(of the record itself) a packed block with the stage on and a converged or slowly moving basis never reaches the sweeps; with
    the stage off, and in the variants without one, no launch reports an outcome of the stage"""
    for cid, v in _GOLDEN.items():
        if cid.startswith("warm-packed") and "-refine0-" not in cid and not cid.endswith("-eta0.0001"):
            assert all(r["counts"][2] == 0 and sum(r["counts"]) == 1 for r in v), cid
        if cid.startswith("warm-") and "-refine0-" in cid:
            assert all(sum(r["counts"]) == 0 for r in v), cid
        if cid.startswith("batch-"):      # refine_blocks: accepted as it arrived / after a step / sent to the sweeps / skipped / checked step
            took_steps = all(m[1] > 0 and m[2] > 0 for m in v[0]["refine_blocks"])
            assert took_steps == cid.endswith("-algNone"), cid        # only the planner's choice (ping-pong) has a stage


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_proj_bits_match_the_parent(case):
    want = _GOLDEN[case[0]]           # (a case without a record is an error, never a skip)
    got = proj_bits.run_case(case)
    assert len(got) == len(want)
    if case[1] == "batch":            # the members carry the same query: the same bytes
        assert got[0]["members"][0] == got[0]["members"][1], case[0]
    for visit, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (case[0], visit)
        for key in sorted(w):
            if key in proj_bits.NOTES:      # (kept beside the digests for the reader: a change of the statistics is no bit failure of the kernel)
                continue
            assert g[key] == w[key], (case[0], visit, key)
