"""Solver families whose M^-1 is structured, on the GPU (run with -m gpu on an MI355X): inside a batch handle the four stages of the
structured form (csrc/minv.hpp) serve all members of a family with one pass over the shared factors per stage (k_minv_*_multi), and
every member's result is bit-identical to the single-solver stage on the same vector.  The options, the tolerance rule and the stall
guard are those of tests/test_family.py; the cases are those of tests/oracle_state.py."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import helpers
import nnsdp_amd as na
import oracle_state as ost
from nnsdp_amd import _lib
from test_family import GUARD_AT, N, _compare_state, _exact_opts, _hplanes, _oracle_step, _state_tolerance, _traj

pytestmark = pytest.mark.gpu

STRUCT_NET, STRUCT_BETA = "W20-D20", 5                  # the smallest structured fixture: at least 3 500 kept multipliers, auto
NORMALS = ((0.6, 0.8), (-0.8, 0.6), (1.0, 0.0))


@functools.lru_cache(maxsize=None)
def _squery(normal):
    return ost.net_hplane_query(STRUCT_NET, STRUCT_BETA, normal)


@functools.lru_cache(maxsize=None)
def _straj(normal):
    """the oracle trajectory of one structured member, advanced once and shared"""
    T = _traj(_squery(normal), "double")
    T.keep |= set(GUARD_AT) | {n - 1 for n in GUARD_AT}
    T.advance(N)
    return T


# ----------------------------------------------------------------------------- 1: the fused apply against an independent solve
APPLY_KEYS = {"W20-D20-b5-double-hplane": dict(minv_mode=0), "W40-D20-b2-double": dict(minv_mode=2), "W40-D40-b0-double": dict(minv_mode=2)}


@pytest.mark.parametrize("key", sorted(APPLY_KEYS))
def test_fused_structured_minv_matches_cholesky_of_the_oracle(key):
    T = ost.trajectory(key)
    s = na.Solver(ost.case_query(key), _exact_opts(ost.CASES[key][1], **APPLY_KEYS[key]))
    rng = np.random.default_rng(83)
    dropped = np.setdiff1d(np.arange(T.P.ng_full), T.P.keep)
    try:
        _, structured, _ = s.apply_minv(np.ones(T.P.ng_full))
        assert structured
        print(f"\n[family-structured] {key}: {int(s.info(10))} chunks, {int(s.info(11))} of them on the scalar-load paths")
        assert s.info(10) >= 2 and 0 <= s.info(11) <= s.info(10)
        worst, outs = 0.0, {}
        Q17 = rng.standard_normal((17, T.P.ng_full))
        for nrhs in (1, 2, 5, 16, 17):
            Q = Q17[:nrhs] if nrhs == 17 else rng.standard_normal((nrhs, T.P.ng_full))
            out, ms = s.apply_minv_structured_multi(Q)
            assert out.shape == Q.shape and np.all(out[:, dropped] == 0.0)
            for j in range(nrhs):
                want = sla.cho_solve(T.S.Mfac, Q[j, T.P.keep])
                worst = max(worst, np.abs(out[j, T.P.keep] - want).max() / np.abs(want).max())
            outs[nrhs] = out
            print(f"[family-structured] fused M^-1 {key} nrhs={nrhs}: four launches {1e3 * ms:.1f} us")
        print(f"[family-structured] fused M^-1 {key}: worst relative error {worst:.3e}  tolerance 1e-10")
        assert worst <= 1e-10
        for j in (0, 3, 15, 16):                        # first, second and third pass: the slot and the company do not matter
            one, _ = s.apply_minv_structured_multi(Q17[j])
            assert np.array_equal(one[0], outs[17][j]), j
            single, _, _ = s.apply_minv(Q17[j])
            assert np.array_equal(single, outs[17][j]), j   # ... and the single-solver stages give the same bits
    finally:
        s.close()


def test_fused_structured_minv_ran_both_load_paths():
    """over the three keys, chunks with an odd clo / w0 (scalar loads) and chunks with even ones (16-byte loads) both occurred"""
    seen = {}
    for key in sorted(APPLY_KEYS):
        s = na.Solver(ost.case_query(key), _exact_opts(ost.CASES[key][1], **APPLY_KEYS[key]))
        try:
            seen[key] = (s.info(10), s.info(11))
        finally:
            s.close()
    print(f"\n[family-structured] (chunks, scalar-path chunks) per key: {seen}")
    assert any(odd > 0 for _, odd in seen.values())
    assert any(odd < chunks for chunks, odd in seen.values())


def test_large_plan_is_fused_and_goes_through_in_sub_passes():
    """W40-D20 beta = 7 (auto: structured; a separator of about 2 600 and couplings above 1 024, so eight members' vectors do not
    fit in a CU's LDS at once and the Schur stage takes the members in sub-passes): the family is fused, and eight vectors in one
    pass give the bits of the single form"""
    qs = [ost.net_hplane_query("W40-D20", 7, n) for n in NORMALS[:2]]
    fam = na.SolverFamily(qs, na.AdmmSdpOptions(decomp_mode=ost.decomp("double"), max_iters=10 ** 8, minv_mode=0))
    try:
        s = fam.solvers[1]
        assert s.info(10) >= 2
        assert (fam.batch_info(3), fam.batch_info(4)) == (1, 2)
        Q = np.random.default_rng(89).standard_normal((8, s.cp.ngamma))
        out, ms = s.apply_minv_structured_multi(Q)
        print(f"\n[family-structured] W40-D20 beta=7: {int(s.info(10))} chunks, 8 vectors in {1e3 * ms:.1f} us")
        for j in (0, 5, 7):
            single, structured, _ = s.apply_minv(Q[j])
            assert structured and np.array_equal(single, out[j]), j
        fam.iterate(16)
        assert all(m.info(3) == 16 for m in fam.solvers)
    finally:
        fam.close()


# ----------------------------------------------------------------------------- 2: refusal
def test_fused_structured_minv_refuses_a_dense_handle():
    key = "W40-D20-b0-single"
    s = na.Solver(ost.case_query(key), _exact_opts("single", minv_mode=1))
    try:
        with pytest.raises(_lib.NnsdpError) as e:
            s.apply_minv_structured_multi(np.ones((2, s.cp.ngamma)))
        assert e.value.code < 0 and "dense" in str(e.value)
    finally:
        s.close()


# ----------------------------------------------------------------------------- 3: grouping
def test_structured_family_members_are_grouped():
    qs = [_squery(n) for n in NORMALS[:2]]
    fam = na.SolverFamily(qs, _exact_opts("double", minv_mode=0))
    try:
        assert (fam.batch_info(3), fam.batch_info(4)) == (1, 2)
        assert fam.batch_info(1) == 0 and fam.batch_info(2) == 0
    finally:
        fam.close()
    plain = na.SolverBatch(qs, _exact_opts("double", minv_mode=0))
    try:
        assert (plain.batch_info(3), plain.batch_info(4)) == (0, 0)
    finally:
        plain.close()
    dense = na.SolverFamily(_hplanes(helpers.load_problem("W10-D5", 3), 3), _exact_opts("single"))
    try:
        assert dense.batch_info(3) == 0 and dense.batch_info(4) == 0 and dense.batch_info(1) == 1
    finally:
        dense.close()


# ----------------------------------------------------------------------------- 4: composition invariance in the loop
def test_structured_member_bits_do_not_depend_on_the_group():
    qs = [_squery(NORMALS[0]), _squery(NORMALS[1]), _squery(NORMALS[0]), _squery(NORMALS[1])]
    parent = na.Solver(qs[0], _exact_opts("double", minv_mode=0))
    solvers = [parent] + [parent.sibling(q) for q in qs[1:]]
    batches = []
    try:
        X = na.SolverBatch.from_solvers(solvers[:2]); batches.append(X)      # fused: one group of two
        Y = na.SolverBatch.from_solvers(solvers[2:3]); batches.append(Y)     # alone: the member's own four launches
        Z = na.SolverBatch.from_solvers(solvers[3:4]); batches.append(Z)
        assert (X.batch_info(3), X.batch_info(4)) == (1, 2)
        assert (Y.batch_info(3), Y.batch_info(4)) == (0, 0) and (Z.batch_info(3), Z.batch_info(4)) == (0, 0)
        for b in batches:
            b.iterate(N)
        got = [s.raw_multipliers() for s in solvers]
        assert np.abs(got[0]).max() > 0 and not np.array_equal(got[0], got[1])
        assert np.array_equal(got[2], got[0]) and np.array_equal(got[3], got[1])
    finally:
        for b in batches:
            b.close()
        for s in solvers:
            s.close()


# ----------------------------------------------------------------------------- 5: a mixed batch against the oracles
def test_mixed_batch_members_track_their_own_oracles():
    """a structured family of two, an independently created structured solver and a dense solver in one batch handle"""
    d5 = helpers.load_problem("W10-D5", 3)
    q5 = _hplanes(d5, 3)[1]
    T5 = _traj(q5, "single")
    T5.keep |= set(GUARD_AT) | {n - 1 for n in GUARD_AT}
    T5.advance(N)
    trajs = [_straj(n) for n in NORMALS] + [T5]
    n_guard = next((n for n in GUARD_AT if all(_oracle_step(T, n) >= 100 * _state_tolerance(T, n)[0] for T in trajs)), None)
    assert n_guard is not None, "the oracles' trajectories do not move at any guarded iteration"
    parent = na.Solver(_squery(NORMALS[0]), _exact_opts("double", minv_mode=0))
    solvers = [parent, parent.sibling(_squery(NORMALS[1])), na.Solver(_squery(NORMALS[2]), _exact_opts("double", minv_mode=0)),
               na.Solver(q5, _exact_opts("single"))]
    sb = na.SolverBatch.from_solvers(solvers, own=True)
    try:
        assert (sb.batch_info(3), sb.batch_info(4)) == (1, 2) and sb.batch_info(1) == 0
        assert solvers[0].info(7) == solvers[1].info(7) != 0 and solvers[2].info(7) == 0 and solvers[3].info(7) == 0
        assert solvers[2].info(10) > 0 and solvers[3].info(10) == 0
        if n_guard < N:
            sb.iterate(n_guard)
            for i, (T, s) in enumerate(zip(trajs, solvers)):
                _compare_state(f"mixed batch member {i} at {n_guard} (guarded)", T, n_guard, s.raw_multipliers())
        sb.iterate(N - n_guard if n_guard < N else N)
        for i, (T, s) in enumerate(zip(trajs, solvers)):
            assert s.info(3) == N and s.info(0) > 0                          # graph replay ran
            _compare_state(f"mixed batch member {i}", T, N, s.raw_multipliers(), stall_guard=n_guard == N)
    finally:
        sb.close()


# ----------------------------------------------------------------------------- 6: a batch that shrinks
def _crown_hplanes(normals):
    """the structured net's hyperplane queries with the intervals findReach2Dpoly makes (frontend.makeQcActivs on [0.5, 1.5]^2)"""
    from nnsdp_amd import frontend as F
    net = ost.golden_net(STRUCT_NET)
    lo, hi = np.full(2, 0.5), np.full(2, 1.5)
    qa = F.makeQcActivs(net, lo, hi, STRUCT_BETA)
    return [na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_reach=na.QcReachHplane(normal=np.asarray(n, dtype=float)),
                          qc_activs=qa) for n in normals]


def test_shrinking_structured_family_batch_matches_members_solved_alone():
    """Three hyperplanes of the structured net (W20-D20 beta = 5) as one family batch and alone on siblings, eps_rel = 1e-4, no polish.

    The intervals are those findReach2Dpoly makes (the sliced bounds of frontend.makeQcActivs), not the plain interval arithmetic of
    oracle_state.net_hplane_query: with the latter the SDPs (objectives of 3e4 .. 6e4) do not converge in a test's time - measured,
    batched and alone alike: 62 550 / 52 550 / 79 300 iterations, two of the three directions ending SLOW_PROGRESS, 33 s; twelve
    directions run to 30 000 iterations reached OPTIMAL in none.  The tighter intervals fix more neurons, so fewer than 3 500
    multipliers are kept and the structured form is asked for (minv_mode = 2, as for the other forced fixtures of this file):
    3 chunks.  Measured: 3 700 / 50 / 3 100 iterations, all OPTIMAL, under 3 s."""
    qs = _crown_hplanes(NORMALS) * 2
    eps = 1e-4
    opts = na.AdmmSdpOptions(decomp_mode=ost.decomp("double"), eps_rel=eps, max_iters=100000, polish=False, minv_mode=2)
    parent = na.Solver(qs[0], opts)
    solvers = [parent] + [parent.sibling(q) for q in qs[1:]]
    try:
        assert parent.info(10) > 0
        A = na.SolverBatch.from_solvers(solvers[:3])
        try:
            assert (A.batch_info(3), A.batch_info(4)) == (1, 3)
            ra = A.run()
            assert A.batch_info(0) == 0
        finally:
            A.close()
        alone = []
        for s in solvers[3:]:
            b = na.SolverBatch.from_solvers([s])
            try:
                assert (b.batch_info(3), b.batch_info(4)) == (0, 0)
                alone.append(b.run()[0])
            finally:
                b.close()
        iters = [r.summary["iters"] for r in ra]
        print(f"\n[family-structured] shrinking batch: iterations {iters}; alone {[r.summary['iters'] for r in alone]}; "
              f"objectives {[r.objective_value for r in ra]} / {[r.objective_value for r in alone]}")
        for a, b in zip(ra, alone):
            assert a.termination_status == b.termination_status == "OPTIMAL"
            oa, ob = a.objective_value, b.objective_value
            assert (oa == 0.0 and ob == 0.0) or abs(oa - ob) <= 2 * eps * max(abs(oa), abs(ob)), (oa, ob)
        assert len(set(iters)) >= 2, iters                                   # a member left while others went on: the group was rebuilt
    finally:
        for s in solvers:
            s.close()
