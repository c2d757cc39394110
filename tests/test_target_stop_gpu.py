"""Deciding a target instead of converging (run with -m gpu on an MI355X): nnsdp_solver_certified_bound - the rigorous bound of any
iterate through the sparse Cholesky of -Z - and the target rule of nnsdp_solver_set_target built on it, through the public Python API.

Workload: the W10-D5 beta = 0 ellipsoid query.  Reference optimum: the independent interior point's bracket in
tests/golden/ipm_optimum.json (lower 0.0911531391 <= optimum <= rho 0.0911531401)."""
import json
import os

import numpy as np
import pytest

import helpers
import nnsdp_amd as na
from nnsdp_amd import _lib, vnnlib as vl

pytestmark = pytest.mark.gpu

SPEC = os.path.join(helpers.GOLDEN, "vnnlib")
IPM = json.load(open(os.path.join(helpers.GOLDEN, "ipm_optimum.json")))["W10-D5_b0"]
LOWER, RHO = IPM["lower"], IPM["rho"]
CHECKPOINTS = (200, 1000, 5000)
# sparse bound against the dense polish of the same iterate, sparse / dense - 1 measured on the MI355X: +2.83e-6, +1.4e-9, +1.4e-9 at the
# three iterates below and +1.53e-4, +2.05e-4, +3.1e-6 at the W40-D20 (Single) iterates 1000 / 3000 / 6000 of tools/decision_timing.py
# (profiles/decision_timing_*.json); asserted at three times the largest
R_MEASURED = 2.06e-4
_state = {}


def query():
    if "q" not in _state:
        _state["d"] = helpers.load_problem("W10-D5", 0)
        _state["q"] = helpers.product_query(_state["d"])
    return _state["q"]


def bounds_at_checkpoints():
    """three solvers advanced through the same calls: `s` asks for the sparse bound at every checkpoint, `twin` never does, `dense`
    finishes (dense polish + dsyevd) there.  Computed once, shared by the tests below."""
    if "cp" not in _state:
        q = query()
        opts = na.AdmmSdpOptions(max_iters=10 ** 8)
        s, twin, dense = na.Solver(q, opts), na.Solver(q, opts), na.Solver(q, opts)
        rows, done = [], 0
        for it in CHECKPOINTS:
            for sv in (s, twin, dense):
                sv.advance(it - done)
            obj, gam, ok, ms = s.certified_bound()
            fin = dense.finish()
            for sv in (s, twin):
                sv.advance(100)
            dense.advance(100)
            done = it + 100
            rows.append(dict(it=it, obj=obj, gam=gam, ok=ok, ms=ms, dense=fin.objective_value, dense_lmax=fin.summary["lambda_max"],
                             same=np.array_equal(s.raw_multipliers(), twin.raw_multipliers()), iters=(s.info(3), twin.info(3))))
        _state["cp"] = rows
        _state["calls"] = s.info(12), twin.info(12), s.info(13)
        for sv in (s, twin, dense):
            sv.close()
    return _state["cp"]


def test_certified_bound_is_feasible_and_rigorous():
    q = query()
    for r in bounds_at_checkpoints():
        assert r["ok"] and np.all(r["gam"] >= 0.0)
        Z = na.makeZ(q, r["gam"])
        ev = np.linalg.eigvalsh(0.5 * (Z + Z.T))
        print(f"it {r['it']}: sparse bound {r['obj']:.10f} ({r['ms']:.2f} ms)  eigmax {ev[-1]:.3e}  |Z|_2 {max(abs(ev[0]), abs(ev[-1])):.3e}  lower {LOWER:.10f}")
        assert ev[-1] <= 1e-9 * max(abs(ev[0]), abs(ev[-1]))
        assert r["obj"] >= LOWER
        assert r["obj"] == pytest.approx(r["gam"][q.ffnet.xdims[0]], rel=1e-12), "the objective of a reach query is gamma_out"
    assert _state["calls"] == (len(CHECKPOINTS), 0, 1)


def test_certified_bound_leaves_the_iteration_alone():
    for r in bounds_at_checkpoints():
        assert r["iters"] == (r["it"] + 100, r["it"] + 100)
        assert r["same"], f"the 100 iterates after the bound at {r['it']} differ from the twin's"


def test_sparse_bound_agrees_with_the_dense_polish():
    worst = 0.0
    for r in bounds_at_checkpoints():
        rel = r["obj"] / r["dense"] - 1.0
        worst = max(worst, rel)
        print(f"it {r['it']}: sparse {r['obj']:.12f} dense {r['dense']:.12f} (lambda_max {r['dense_lmax']:.2e})  sparse / dense - 1 = {rel:+.3e}")
    for r in bounds_at_checkpoints():
        assert r["obj"] >= r["dense"] * (1 - 1e-9)
        assert r["obj"] <= r["dense"] * (1 + 3 * R_MEASURED)
    print(f"largest excess {worst:.3e}, asserted {3 * R_MEASURED:.1e}")


def _run(**kw):
    sv = na.Solver(query(), na.AdmmSdpOptions(max_iters=100000, **kw))
    try:
        return sv.run()
    finally:
        sv.close()


def test_reachable_target_stops_certified():
    target = 1.05 * RHO
    got = _run(target=target)
    ref = _run(cert_tol=1e-3)
    print(f"target 1.05 rho: {got.termination_status} at {got.summary['iters']} iterations, bound {got.objective_value:.8f} "
          f"({got.summary['sparse_bound_calls']} sparse bounds); cert_tol = 1e-3 without target: {ref.termination_status} at {ref.summary['iters']}")
    assert got.termination_status == "TARGET_CERTIFIED"
    assert got.objective_value <= target and got.summary["lambda_max"] <= 1e-6
    assert got.objective_value >= LOWER
    assert got.summary["iters"] <= ref.summary["iters"]
    assert got.summary["sparse_bound_calls"] >= 1


def test_unreachable_target_stops_early():
    got = _run(target=0.95 * LOWER)
    ref = _run()
    print(f"target 0.95 lower: {got.termination_status} at {got.summary['iters']} iterations; eps_rel = 1e-6: {ref.termination_status} at {ref.summary['iters']}")
    assert got.termination_status == "TARGET_UNREACHABLE"
    assert got.summary["iters"] < ref.summary["iters"]


def test_target_inside_the_band_is_never_declared_unreachable():
    got = _run(target=1.0005 * RHO)
    print(f"target 1.0005 rho: {got.termination_status} at {got.summary['iters']} iterations, bound {got.objective_value:.10f}")
    assert got.termination_status != "TARGET_UNREACHABLE"
    if got.termination_status == "TARGET_CERTIFIED":
        assert LOWER <= got.objective_value <= 1.0005 * RHO and got.summary["lambda_max"] <= 1e-6


def _net():
    d = helpers.load_problem("W10-D5", 0)
    return na.FeedFwdNet(xdims=[int(v) for v in d["xdims"]], Ms=helpers.problem_Ms(d))


def test_safety_form_stops_at_the_first_certificate():
    net = _net()
    spec = os.path.join(SPEC, "prop_bound.vnnlib")
    opts = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)
    solns, nq, status = vl.verifyAcasSpec(net, spec, 1, opts, decide_early=True)
    plain, _, _ = vl.verifyAcasSpec(net, spec, 1, opts)
    print(f"feasibility form, decide_early: {solns[0].termination_status} at {solns[0].summary['iters']} iterations "
          f"(lambda_max {solns[0].summary['lambda_max']:.2e}); without: {plain[0].termination_status} at {plain[0].summary['iters']}")
    assert (nq, len(solns), status) == (1, 1, "safe") and vl.isSolutionGood(solns[0])
    assert solns[0].termination_status == "TARGET_CERTIFIED" and solns[0].summary["iters"] <= plain[0].summary["iters"]
    unsafe = open(spec).read().replace("(assert (>= Y_0 10.0))", "(assert (<= Y_0 10.0))")
    solns, nq, status = vl.verifyAcasSpec(net, unsafe, 1, na.AdmmSdpOptions(max_iters=3000, eps_rel=1e-5), decide_early=True)
    assert status == "unsafe" and not vl.isSolutionGood(solns[0]) and solns[0].termination_status != "TARGET_CERTIFIED"


def test_reach_form_decides_early_with_the_same_verdicts():
    net = _net()
    spec = os.path.join(SPEC, "prop_bound.vnnlib")
    opts = na.AdmmSdpOptions(max_iters=100000, eps_rel=1e-6, cert_tol=1e-3)
    s0, _, st0 = vl.verifyAcasSpec(net, spec, 1, opts, via_reach=True)
    bound = s0[0].summary["reach_bound"]
    box = "(assert (>= X_0 0.5))(assert (<= X_0 1.5))(assert (>= X_1 0.5))(assert (<= X_1 1.5))"
    specs = [spec, box + f"(assert (>= Y_0 {bound + 0.01}))", box + f"(assert (>= Y_0 {bound - 0.02 * max(1.0, abs(bound))}))"]
    want = [vl.verifyAcasSpec(net, sp, 1, opts, via_reach=True) for sp in specs[1:]]
    verdicts = [st0] + [w[2] for w in want]
    assert verdicts == ["safe", "safe", "unsafe"]
    iters = [s0[0].summary["iters"]] + [w[0][0].summary["iters"] for w in want]
    for sp, verdict, it in zip(specs, verdicts, iters):
        s, _, st = vl.verifyAcasSpec(net, sp, 1, opts, via_reach=True, decide_early=True)
        print(f"reach form, decide_early: {st} ({s[0].summary['reach_status']}) at {s[0].summary['iters']} iterations, margin {s[0].summary['margin']:+.4f}; without: {verdict} at {it}")
        assert st == verdict
        if verdict == "safe":
            assert s[0].summary["reach_status"] == "TARGET_CERTIFIED" and vl.isSolutionGood(s[0]) and s[0].summary["margin"] >= 0
            assert s[0].summary["iters"] <= it
        else:
            assert s[0].summary["reach_status"] != "TARGET_CERTIFIED" and s[0].summary["margin"] < 0


def test_family_members_carry_their_own_targets():
    """six findReach2Dpoly directions as one family, three targets reachable and three not: every member decides as it does alone"""
    d = helpers.load_problem("W10-D5", 0)
    net = _net()
    qin = na.QcInputBox(x1min=d["x1min"], x1max=d["x1max"])
    qa = na.makeQcActivs(net, d["x1min"], d["x1max"], 0)
    normals = [np.array([np.cos(2 * np.pi * i / 6), np.sin(2 * np.pi * i / 6)]) for i in range(6)]
    queries = [na.ReachQuery(ffnet=net, qc_input=qin, qc_reach=na.QcReachHplane(normal=nrm), qc_activs=qa) for nrm in normals]
    opts = na.AdmmSdpOptions(max_iters=30000, eps_rel=1e-6)
    base = na.runQueries(queries, na.AdmmSdpOptions(max_iters=30000, eps_rel=1e-6, cert_tol=1e-3), share_setup=True)
    opt = [s.objective_value for s in base]            # certified bounds within 1e-3 of the optima
    span = max(max(opt) - min(opt), 0.1)
    targets = [o + 0.05 * span if i % 2 == 0 else o - 0.05 * span for i, o in enumerate(opt)]
    fam = na.SolverFamily(queries, opts, targets=targets)
    try:
        got = fam.run()
    finally:
        fam.close()
    for i, (q, tg, g) in enumerate(zip(queries, targets, got)):
        sv = na.Solver(q, na.AdmmSdpOptions(max_iters=30000, eps_rel=1e-6, target=tg))
        try:
            alone = sv.run()
        finally:
            sv.close()
        print(f"direction {i}: optimum ~{opt[i]:.6f} target {tg:.6f}: family {g.termination_status} at {g.summary['iters']}, alone {alone.termination_status} at {alone.summary['iters']}")
        assert g.termination_status == alone.termination_status
        assert g.termination_status == ("TARGET_CERTIFIED" if i % 2 == 0 else "TARGET_UNREACHABLE")
        if g.termination_status == "TARGET_CERTIFIED":
            assert g.summary["iters"] == alone.summary["iters"]
            assert g.objective_value <= tg and g.summary["lambda_max"] <= 1e-6


def test_sharded_handle_refuses_a_target():
    sv = na.Solver(query(), na.AdmmSdpOptions(max_iters=100))
    try:
        sv.set_comm_callback(1, 0, lambda a: None)
        assert sv.info(2) == 1.0
        with pytest.raises(_lib.NnsdpError) as e:
            sv.set_target(na.TARGET_OBJECTIVE, 1.0)
        assert e.value.code == -1
    finally:
        sv.close()
    safety = na.Solver(vl.loadReluQueriesCnf(_net(), os.path.join(SPEC, "prop_bound.vnnlib"), 1)[0][0], na.AdmmSdpOptions(max_iters=100))
    try:
        with pytest.raises(_lib.NnsdpError):
            safety.set_target(na.TARGET_OBJECTIVE, 1.0)      # (an objective target needs a reach query)
        safety.set_target(na.TARGET_FEASIBLE)
    finally:
        safety.close()
