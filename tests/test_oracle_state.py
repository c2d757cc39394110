"""The oracle-state harness (tests/oracle_state.py) on the CPU: it steps exactly the iteration admm_solve runs, reports the
block structure the GPU suite checks the library against, and its check quantities are admm_solve's."""
import numpy as np

import oracle_state as ost
from oracle import admm as oadmm


def test_harness_steps_admm_solve_bit_for_bit():
    key = "W40-D20-b0-single"
    T = ost.Trajectory(ost.case_operator(key))
    r = oadmm.admm_solve(ost.case_operator(key), oadmm.AdmmOptions(max_iters=100, adapt_sigma=False))
    assert r.iters == 100 and [h[0] for h in r.history] == [50, 100]
    # admm_solve's check at iteration k is the step taken from state k - 1
    for it, rp, rd, obj, dobj, sigma in r.history:
        assert T.check(it - 1) == (rp, rd, obj, dobj)
        assert sigma == 0.1
    assert np.array_equal(T.gamma(100), r.gamma)
    # the state a check iteration leaves is the state the plain iteration reaches
    nu100 = T.snaps[100].copy()
    T2 = ost.Trajectory(ost.case_operator(key))
    T2.advance(100)
    assert np.array_equal(T2.nu(100), nu100)
    assert T2.bound_norm(100) == max(T2.norms) and len(T2.norms) == 101


def test_harness_block_structure_w40_d20_single():
    """19 blocks, the largest 85 (after the normalising congruence; SURVEY.md table, test_full_size_solver_invariants_w40_d20)"""
    T = ost.trajectory("W40-D20-b0-single")
    assert T.blocks() == (19, 85)


def test_harness_multiplier_layout():
    T = ost.trajectory("W10-D5-b3-single")
    T.advance(7, keep={6})
    m = T.multipliers(7)
    assert m.shape == (T.P.ng_full,)
    dropped = np.setdiff1d(np.arange(T.P.ng_full), T.P.keep)
    assert len(dropped) > 0 and np.all(m[dropped] == 0.0)
    assert np.array_equal(m[T.P.keep], T.nu(7)[:T.S.ng])
    assert not np.array_equal(T.multipliers(6), m)
    with np.testing.assert_raises(ValueError):
        T.nu(3)                          # passed without being kept


def test_harness_check_is_the_step_it_reports():
    """check(n) leaves state n + 1 of the plain trajectory"""
    T = ost.Trajectory(ost.case_operator("W10-D5-b3-single"))
    T.check(4)
    T2 = ost.Trajectory(ost.case_operator("W10-D5-b3-single"))
    T2.advance(5)
    assert np.array_equal(T.nu(5), T2.nu(5))
