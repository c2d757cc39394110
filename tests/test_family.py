"""Solver families on the GPU (run with -m gpu on an MI355X): solvers that differ in the output QC only share ONE set-up - operator,
tables, M^-1 - by reference count (Solver.sibling, SolverFamily), and inside a batch handle one pass over the common dense M^-1
serves all of them (k_minv_family).  Everything goes through the public Python API; every member is compared with its OWN oracle
trajectory (tests/oracle_state.py), by the tolerance rule of tests/test_state_parity.py, restated here."""
import os

import numpy as np
import pytest
import scipy.linalg as sla

import helpers
import nnsdp_amd as na
import oracle_state as ost
from nnsdp_amd import _lib, vnnlib as vl
from oracle import operator as oop
from test_family_cpu import safety_S, shifted_bias

pytestmark = pytest.mark.gpu

N = 300
TOL = 1e-12


def _exact_opts(mode, **kw):
    """exact sweeps, fixed penalty, raw iterate (test_state_parity._exact_opts)"""
    o = dict(decomp_mode=ost.decomp(mode), max_iters=10 ** 8, proj_tol=TOL, adapt_every=0, polish=False, proj_refine=0)
    o.update(kw)
    return na.AdmmSdpOptions(**o)


def _traj(q, mode):
    return ost.Trajectory(oop.build_operator(ost.mirror_query(q), mode, normalize=True, merge_identical=True))


def _state_tolerance(T, n):
    """1e-9 max(1, max|nu|), never above the rigorous bound 5 N tol B (test_state_parity._state_tolerance)"""
    bound = ost.rigorous_bound(n, TOL, T.bound_norm(n))
    return min(1e-9 * max(1.0, np.abs(T.nu(n)).max()), bound), bound


def _oracle_step(T, n):
    return np.abs(T.multipliers(n) - T.multipliers(n - 1)).max()


def _compare_state(what, T, n, got, stall_guard=True):
    T.keep |= {n - 1, n}
    T.advance(n)
    want = T.multipliers(n)
    tol, bound = _state_tolerance(T, n)
    dropped = np.setdiff1d(np.arange(len(want)), T.P.keep)
    assert np.all(got[dropped] == 0.0), (what, "dropped multipliers must be exactly 0")
    dev = np.abs(got - want).max()
    print(f"\n[family] {what}: deviation {dev:.3e}  tolerance {tol:.3e}  rigorous bound {bound:.3e}")
    assert dev <= tol, (what, n, dev, tol)
    if stall_guard:
        step = _oracle_step(T, n)
        assert step >= 100 * tol, (what, step, tol)                # a stalled or one-step-off state fails


def _hplanes(d, k=6):
    return [helpers.product_query(d, "hplane", normal=(np.cos(2 * np.pi * i / k), np.sin(2 * np.pi * i / k))) for i in range(k)]


def _acas_queries():
    """the network and box of helpers.acas_shaped_query with the normals e_1 and e_2"""
    from nnsdp_amd import frontend as F
    net = na.randomNetwork([5] + [50] * 6 + [5], seed=1234)
    lo, hi = np.full(5, 0.25), np.full(5, 0.35)
    xi, acx = F.intervalsWorstCase(lo, hi, net)
    qa = F.makeQcActivsIntvs(net, xi, acx, 0)
    return [na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_reach=na.QcReachHplane(normal=np.eye(5)[i]), qc_activs=qa)
            for i in range(2)]


def _family_cases():
    d5 = helpers.load_problem("W10-D5", 3)
    h5 = _hplanes(d5, 3)
    return {
        "W40-D20-b0-single-6-hplanes": (lambda: _hplanes(helpers.load_problem("W40-D20", 0)), "single", {}, 1),
        "W10-D5-b3-single-2-safety-sets": (lambda: [helpers.product_query(d5, "safety", S=safety_S((1, 0), 50)),
                                                    helpers.product_query(d5, "safety", S=safety_S((0, 1), 80))], "single", {}, 1),
        "W10-D5-b3-single-hplanes-one-shifted-output-bias": (lambda: [h5[0], h5[1], shifted_bias(h5[2], (0.5, -0.25))], "single", {}, 1),
        "acas50-path-e1-e2": (_acas_queries, "path", {}, 1),
        "W20-D20-b5-double-structured": (lambda: [ost.net_hplane_query("W20-D20", 5, n) for n in ((0.6, 0.8), (-0.8, 0.6))], "double",
                                         dict(minv_mode=0), 0),
    }


# ----------------------------------------------------------------------------- 4: every member against its own oracle
GUARD_AT = (N, 150, 100, 50, 25, 10)


@pytest.mark.parametrize("case", sorted(_family_cases()))
def test_family_members_track_their_own_oracles(case):
    """State N of every member against its own oracle trajectory, with the "a stalled state fails" guard (the oracle's own last step
    is at least 100 x the tolerance, so a state that stopped moving or is one step off cannot pass).  The guard is a property of the
    ORACLE's trajectory alone, and some members' oracles have converged long before iteration 300: the two W10-D5 beta 3 safety sets
    (step from state 299 to 300: 8.6e-11, tolerance 1e-9) and the W40-D20 directions 0, 4 and 5, whose optimum is 0 (step 2e-15; the
    directions 1, 2, 3 still move by 0.44).  Where a member's oracle stands still at 300, the guarded comparison of ALL members is
    made at the latest iteration of GUARD_AT at which every member's oracle still moves by 100 x the tolerance (W40-D20: 25), and
    state 300 is compared as well, with the same tolerance rule and the oracle's own steps printed beside it."""
    make, mode, kw, groups = _family_cases()[case]
    qs = make()
    trajs = [_traj(q, mode) for q in qs]
    for T in trajs:
        T.keep |= set(GUARD_AT) | {n - 1 for n in GUARD_AT}
        T.advance(N)
    n_guard = next((n for n in GUARD_AT if all(_oracle_step(T, n) >= 100 * _state_tolerance(T, n)[0] for T in trajs)), None)
    assert n_guard is not None, (case, "the oracle's trajectory does not move at any guarded iteration")
    fam = na.SolverFamily(qs, _exact_opts(mode, **kw))
    try:
        assert fam.batch_info(0) == len(qs)
        assert fam.batch_info(1) == groups and fam.batch_info(2) == (len(qs) if groups else 0)
        ids = {s.info(7) for s in fam.solvers}
        assert len(ids) == 1 and ids.pop() != 0
        if not groups:
            out, structured, _ = fam.solvers[1].apply_minv(np.ones(fam.solvers[1].cp.ngamma))
            assert structured                                       # ng >= 3500: the shared structured factors
        if n_guard < N:
            fam.iterate(n_guard)
            for i, (T, s) in enumerate(zip(trajs, fam.solvers)):
                _compare_state(f"{case} member {i} at {n_guard} (guarded)", T, n_guard, s.raw_multipliers())
            print(f"[family] {case}: oracle steps at {N}: {[float(_oracle_step(T, N)) for T in trajs]}")
        fam.iterate(N - n_guard if n_guard < N else N)
        for i, (T, s) in enumerate(zip(trajs, fam.solvers)):
            assert s.info(3) == N and s.info(0) > 0                 # graph replay ran
            _compare_state(f"{case} member {i}", T, N, s.raw_multipliers(), stall_guard=n_guard == N)
    finally:
        fam.close()


def test_sibling_iterated_outside_the_batch_uses_the_single_solver_stage():
    """nnsdp_solver_iterate on a member: the single-solver loop (k_gemv_sym on the shared inverse, its own graph), same trajectory"""
    d = helpers.load_problem("W10-D5", 3)
    qs = _hplanes(d, 2)
    fam = na.SolverFamily(qs, _exact_opts("single"))
    try:
        fam.iterate(N)
        s = fam.solvers[1]
        g0 = s.info(0)
        s.iterate(64)
        assert s.info(0) > g0 and s.info(3) == N + 64
        _compare_state("sibling iterated alone after the batch", _traj(qs[1], "single"), N + 64, s.raw_multipliers())
    finally:
        fam.close()


# ----------------------------------------------------------------------------- 5: composition invariance
def test_member_bits_do_not_depend_on_the_group():
    d = helpers.load_problem("W40-D20", 0)
    qs = _hplanes(d) + _hplanes(d)
    parent = na.Solver(qs[0], _exact_opts("single"))
    solvers = [parent] + [parent.sibling(q) for q in qs[1:]]
    batches = []
    try:
        X = na.SolverBatch.from_solvers(solvers[:6]); batches.append(X)
        Y = na.SolverBatch.from_solvers(solvers[6:8]); batches.append(Y)
        Z = na.SolverBatch.from_solvers(solvers[8:9]); batches.append(Z)
        assert (X.batch_info(1), X.batch_info(2)) == (1, 6)
        assert (Y.batch_info(1), Y.batch_info(2)) == (1, 2)
        assert (Z.batch_info(1), Z.batch_info(2)) == (1, 1)       # a group of one still takes the fused pass
        for b in batches:
            b.iterate(N)
        got = [s.raw_multipliers() for s in solvers[:9]]
        assert np.abs(got[0]).max() > 0 and not np.array_equal(got[0], got[1])
        assert np.array_equal(got[6], got[0]) and np.array_equal(got[7], got[1]) and np.array_equal(got[8], got[2])
    finally:
        for b in batches:
            b.close()
        for s in solvers:
            s.close()


def test_shrinking_family_batch_matches_members_solved_alone():
    d = helpers.load_problem("W10-D5", 0)
    qs = _hplanes(d) + _hplanes(d)
    opts = na.AdmmSdpOptions(eps_rel=1e-6, max_iters=100000, polish=False)
    parent = na.Solver(qs[0], opts)
    solvers = [parent] + [parent.sibling(q) for q in qs[1:]]
    try:
        A = na.SolverBatch.from_solvers(solvers[:6])
        try:
            assert (A.batch_info(1), A.batch_info(2)) == (1, 6)
            ra = A.run()
            assert A.batch_info(0) == 0
        finally:
            A.close()
        alone = []
        for s in solvers[6:]:
            b = na.SolverBatch.from_solvers([s])
            try:
                assert (b.batch_info(1), b.batch_info(2)) == (1, 1)
                alone.append(b.run()[0])
            finally:
                b.close()
        iters = [r.summary["iters"] for r in ra]
        print(f"\n[family] shrinking batch: iterations {iters}; alone {[r.summary['iters'] for r in alone]}; "
              f"objectives {[r.objective_value for r in ra]} / {[r.objective_value for r in alone]}")
        for a, b in zip(ra, alone):
            assert a.termination_status == b.termination_status == "OPTIMAL"
            oa, ob = a.objective_value, b.objective_value
            assert (oa == 0.0 and ob == 0.0) or abs(oa - ob) <= 2e-6 * max(abs(oa), abs(ob)), (oa, ob)
        assert len(set(iters)) >= 3, iters                         # members left while others went on: the group was rebuilt under them
    finally:
        for s in solvers:
            s.close()


# ----------------------------------------------------------------------------- 6: the fused product against an independent solve
@pytest.mark.parametrize("key", ["W40-D20-b0-single", "W40-D40-b0-double"])
def test_fused_minv_matches_cholesky_of_the_oracle(key):
    T = ost.trajectory(key)
    s = na.Solver(ost.case_query(key), _exact_opts(ost.CASES[key][1], minv_mode=1))
    rng = np.random.default_rng(79)
    dropped = np.setdiff1d(np.arange(T.P.ng_full), T.P.keep)
    try:
        worst, outs = 0.0, {}
        Q17 = rng.standard_normal((17, T.P.ng_full))
        for nrhs in (1, 2, 5, 16, 17):
            Q = Q17[:nrhs] if nrhs == 17 else rng.standard_normal((nrhs, T.P.ng_full))
            out, ms = s.apply_minv_multi(Q)
            assert out.shape == Q.shape and np.all(out[:, dropped] == 0.0)
            for j in range(nrhs):
                want = sla.cho_solve(T.S.Mfac, Q[j, T.P.keep])
                worst = max(worst, np.abs(out[j, T.P.keep] - want).max() / np.abs(want).max())
            outs[nrhs] = out
            print(f"\n[family] fused M^-1 {key} nrhs={nrhs}: kernel {1e3 * ms:.1f} us")
        print(f"[family] fused M^-1 {key}: worst relative error {worst:.3e}  tolerance 1e-10")
        assert worst <= 1e-10
        for j in (0, 3, 15, 16):                                    # first pass, second pass: the slot and the company do not matter
            one, _ = s.apply_minv_multi(Q17[j])
            assert np.array_equal(one[0], outs[17][j]), j
    finally:
        s.close()


def test_fused_minv_refuses_a_structured_handle():
    key = "W40-D40-b0-double"
    s = na.Solver(ost.case_query(key), _exact_opts("double", minv_mode=2))
    try:
        with pytest.raises(_lib.NnsdpError) as e:
            s.apply_minv_multi(np.ones((2, s.cp.ngamma)))
        assert e.value.code < 0 and "structured" in str(e.value)
    finally:
        s.close()


# ----------------------------------------------------------------------------- 7: sharing is real
def test_family_shares_one_inverse_and_survives_its_parent():
    d = helpers.load_problem("W40-D20", 0)
    qs = _hplanes(d)
    T1 = _traj(qs[1], "single")
    ng = len(T1.P.keep)
    ldm = (ng + 1) & ~1
    alone = na.Solver(qs[0], _exact_opts("single"))
    try:
        assert alone.info(7) == 0 and alone.info(9) == 0
        alone_total = alone.info(8) + alone.info(9)
    finally:
        alone.close()
    parent = na.Solver(qs[0], _exact_opts("single"))
    sibs = [parent.sibling(q) for q in qs[1:]]
    try:
        shared = parent.info(9)
        assert shared >= 8 * ng * ldm
        for s in sibs:
            assert s.info(9) == shared and s.info(8) < s.info(9)
        fam_total = sum(s.info(8) for s in [parent] + sibs) + shared
        print(f"\n[family] device bytes: family of six {fam_total / 1e6:.1f} MB, six stand-alone solvers {6 * alone_total / 1e6:.1f} MB "
              f"(one inverse {8 * ng * ldm / 1e6:.1f} MB)")
        assert fam_total <= 6 * alone_total - 5 * 8 * ng * ldm
        b = na.SolverBatch.from_solvers([parent] + sibs)
        try:
            b.iterate(N)
        finally:
            b.close()
        parent.close()                                              # the parent goes first
        assert all(s.info(9) == shared for s in sibs)               # the siblings keep the set-up alive between them
        b = na.SolverBatch.from_solvers(sibs)
        try:
            assert (b.batch_info(1), b.batch_info(2)) == (1, 5)
            b.iterate(50)
        finally:
            b.close()
        _compare_state("sibling 1 after its parent was destroyed", T1, N + 50, sibs[0].raw_multipliers())
    finally:
        parent.close()
        for s in sibs:
            s.close()


# ----------------------------------------------------------------------------- 8: refusals
def test_sibling_refusals_name_the_reason():
    d = helpers.load_problem("W10-D5", 3)
    q0 = helpers.product_query(d, "hplane", normal=(1.0, 0.0))
    parent = na.Solver(q0, _exact_opts("single"))
    try:
        def refused(q, word, p=parent):
            with pytest.raises(_lib.NnsdpError) as e:
                p.sibling(q).close()
            assert e.value.code < 0 and word in str(e.value), str(e.value)

        d_beta = dict(d); d_beta["beta"] = np.int64(0)
        refused(helpers.product_query(d_beta, "hplane", normal=(0.0, 1.0)), "beta")
        d_box = dict(d); d_box["x1min"] = d["x1min"] - 1e-3
        refused(helpers.product_query(d_box, "hplane", normal=(0.0, 1.0)), "x1min")
        refused(helpers.product_query(d, "ellipsoid"), "out_kind")
        parent.iterate(20)
        assert parent.info(3) == 20
        # a PATH parent and a safety set that couples x_1 with y
        ppath = na.Solver(helpers.product_query(d, "safety", S=safety_S((1, 0), 50)), _exact_opts("path"))
        try:
            S12 = safety_S((0, 1), 80)
            S12[0, 2] = S12[2, 0] = 1.0
            refused(helpers.product_query(d, "safety", S=S12), "S12", p=ppath)
            ok = ppath.sibling(helpers.product_query(d, "safety", S=safety_S((0, 1), 80)))
            ok.close()
            ppath.iterate(20)
            assert ppath.info(3) == 20
        finally:
            ppath.close()
        # a parent that has been given a communicator
        pc = na.Solver(q0, _exact_opts("single"))
        try:
            pc.set_comm_callback(1, 0, lambda a: None)
            refused(helpers.product_query(d, "hplane", normal=(0.0, 1.0)), "communicator", p=pc)
            pc.iterate(20)
            assert pc.info(3) == 20
        finally:
            pc.close()
        # ... and a family member cannot be given one
        sib = parent.sibling(helpers.product_query(d, "hplane", normal=(0.0, 1.0)))
        try:
            with pytest.raises(_lib.NnsdpError) as e:
                sib.set_comm_callback(1, 0, lambda a: None)
            assert e.value.code < 0 and "family" in str(e.value)
        finally:
            sib.close()
    finally:
        parent.close()


# ----------------------------------------------------------------------------- 9: end to end
def _w10d5_net():
    d = helpers.load_problem("W10-D5", 0)
    return d, na.FeedFwdNet(xdims=[int(v) for v in d["xdims"]], Ms=helpers.problem_Ms(d))


def test_find_reach_2d_poly_with_a_shared_setup():
    d, net = _w10d5_net()
    opts = na.AdmmSdpOptions(max_iters=100000, eps_rel=1e-6)
    hf, sf = na.findReach2Dpoly(net, d["x1min"], d["x1max"], 1, opts, share_setup=True)
    hb, sb = na.findReach2Dpoly(net, d["x1min"], d["x1max"], 1, opts)
    assert len(hf) == 6 and all(s.termination_status == "OPTIMAL" for s in sf + sb)
    for (nf, of), (nb, ob) in zip(hf, hb):
        assert np.array_equal(nf, nb) and abs(of - ob) <= 1e-5 * max(1.0, abs(ob)), (of, ob)
    for s in sf:
        assert s.summary["lambda_max"] <= 1e-6
        assert all(np.all(s.values[k] >= 0) for k in ("γin", "γout", "γac1", "γac2"))
    # a sibling reports its own small set-up; the first member's holds the factorisation
    print(f"\n[family] findReach2Dpoly set-up seconds, shared: {[round(s.setup_time, 4) for s in sf]}; unshared: {[round(s.setup_time, 4) for s in sb]}")
    rng = np.random.default_rng(0)
    X = d["x1min"][:, None] + (d["x1max"] - d["x1min"])[:, None] * rng.random((2, 5000))
    Y = na.evalFeedFwdNet(net, X)
    for nrm, off in hf:
        assert np.all(nrm @ Y <= off + 1e-6)


def test_clause_driver_with_a_shared_setup():
    d, net = _w10d5_net()
    spec = """
    (assert (>= X_0 0.5)) (assert (<= X_0 1.5)) (assert (>= X_1 0.5)) (assert (<= X_1 1.5))
    (assert (or (and (<= Y_0 10.0) (>= Y_1 20.0)) (and (>= Y_0 15.0) (>= Y_1 -50.0))))
    """
    opts = na.AdmmSdpOptions(max_iters=4000, eps_rel=1e-5)
    s1, nq1, st1 = vl.verifyAcasSpec(net, spec, 1, opts, batch_clause=True)
    s2, nq2, st2 = vl.verifyAcasSpec(net, spec, 1, opts, batch_clause=True, share_setup=True)
    assert (nq1, st1, len(s1)) == (nq2, st2, len(s2)) == (4, "safe", 4)
    assert [vl.isSolutionGood(s) for s in s1] == [vl.isSolutionGood(s) for s in s2]
    # the reach form shifts the output bias per literal: still one family
    ropts = na.AdmmSdpOptions(max_iters=100000, eps_rel=1e-6, cert_tol=1e-3)
    r1, _, rt1 = vl.verifyAcasSpec(net, spec, 1, ropts, batch_clause=True, via_reach=True)
    r2, _, rt2 = vl.verifyAcasSpec(net, spec, 1, ropts, batch_clause=True, via_reach=True, share_setup=True)
    assert rt1 == rt2 and len(r1) == len(r2) == 4
    assert [s.termination_status for s in r1] == [s.termination_status for s in r2]
    for path in ("prop_bound.vnnlib", "prop_or_inputs.vnnlib"):
        full = os.path.join(helpers.GOLDEN, "vnnlib", path)
        a = vl.verifyPairs([("W10-D5", net, path, full)], 1, na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5), batch_clause=True)[0]
        b = vl.verifyPairs([("W10-D5", net, path, full)], 1, na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5), batch_clause=True, share_setup=True)[0]
        assert a[0][2:5] == b[0][2:5], (path, a, b)


def test_mixed_queries_with_a_shared_setup():
    d = helpers.load_problem("W10-D5", 0)
    qs = [helpers.product_query(d, "hplane", normal=(1.0, 0.0)), helpers.product_query(d, "ellipsoid"),
          helpers.product_query(d, "hplane", normal=(0.0, 1.0))]
    opts = na.AdmmSdpOptions(max_iters=100000, eps_rel=1e-6)
    solvers = na.methods._shared_solvers(qs, [opts] * 3)
    sb = na.SolverBatch.from_solvers(solvers, own=True)
    try:
        assert (sb.batch_info(1), sb.batch_info(2)) == (1, 2)      # one fused group of two, the ellipsoid a loner beside it
        assert solvers[0].info(7) == solvers[2].info(7) != 0 and solvers[1].info(7) == 0
    finally:
        sb.close()
    shared = na.runQueries(qs, opts, share_setup=True)
    plain = na.runQueries(qs, opts)
    for a, b in zip(shared, plain):
        assert a.termination_status == b.termination_status == "OPTIMAL"
        assert abs(a.objective_value - b.objective_value) <= 2e-6 * abs(b.objective_value), (a.objective_value, b.objective_value)
