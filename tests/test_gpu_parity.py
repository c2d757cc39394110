"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the C ABI
(nn-sdp_amd/nnsdp_amd -> libnnsdp_hip.so); the oracle is only the checker.

Tolerances: fp64 throughout.  Assembly / adjoint: 1e-12 relative (different summation order only).
PSD projection: 1e-10 * |A| (Jacobi vs LAPACK).  Solver: the HIP ADMM and the oracle ADMM run the
same iteration, so objectives agree to 1e-6 relative after the same number of iterations; against the
reference's published MOSEK objective the tolerance is 1e-3 relative."""
import os

import numpy as np
import pytest

import helpers
import nnsdp_amd as na
from oracle import admm as oadmm, operator as oop, qc

pytestmark = pytest.mark.gpu


def _sym(rng, n, scale=1.0):
    A = rng.standard_normal((n, n)) * scale
    return 0.5 * (A + A.T)


def _ref_proj(A):
    return oadmm.project_psd(A)


# ----------------------------------------------------------------------------- K3: PSD projection
def test_projection_matches_lapack_ragged_batch():
    rng = np.random.default_rng(0)
    mats = [_sym(rng, n) for n in (1, 2, 3, 5, 16, 23, 31, 40, 41, 64, 83, 85, 97, 98, 99, 121, 127, 128)]
    res, evs, ms = na.project_psd_batched(mats)
    assert ms > 0
    for A, P, ev in zip(mats, res, evs):
        nrm = max(1.0, np.abs(A).max())
        assert np.abs(P - _ref_proj(A)).max() <= 1e-10 * nrm
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-10 * nrm
        assert np.abs(P - P.T).max() <= 1e-12 * nrm


def test_projection_above_128_goes_through_the_library_path():
    """matrices above 128 (the reference's 151-wide cliques, dense cones) in one call with small ones: LAPACK agreement"""
    rng = np.random.default_rng(3)
    mats = [_sym(rng, n) for n in (130, 64, 151, 203, 31, 129)]
    res, evs, ms = na.project_psd_batched(mats)
    for A, P, ev in zip(mats, res, evs):
        nrm = max(1.0, np.abs(A).max())
        assert np.abs(P - _ref_proj(A)).max() <= 1e-10 * nrm, A.shape
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-10 * nrm
        assert np.abs(P - P.T).max() <= 1e-11 * nrm
    res, _, _ = na.project_psd_batched([mats[3]])          # big matrices only
    assert np.abs(res[0] - _ref_proj(mats[3])).max() <= 1e-10 * np.abs(mats[3]).max()


def test_projection_edge_cases():
    rng = np.random.default_rng(1)
    n = 37
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    psd = (Q * np.linspace(0.1, 3, n)) @ Q.T
    nsd = -psd
    rank1 = np.outer(Q[:, 0], Q[:, 0]) * 2.5
    repeated = (Q * np.repeat([2.0, -1.0, 0.0], [12, 12, 13])) @ Q.T
    tiny = _sym(rng, n, 1e-150)
    huge = _sym(rng, n, 1e120)
    cases = [np.zeros((n, n)), np.eye(n), -np.eye(n), psd, nsd, rank1, repeated, np.diag(np.arange(n) - 18.0), tiny, huge,
             np.array([[0.0]]), np.array([[-3.0]]), np.array([[0.0, 1.0], [1.0, 0.0]])]
    res, _, _ = na.project_psd_batched(cases)
    for A, P in zip(cases, res):
        nrm = max(np.abs(A).max(), 1e-300)
        assert np.all(np.isfinite(P))
        assert np.abs(P - _ref_proj(A)).max() <= 1e-10 * nrm
    assert np.array_equal(res[0], np.zeros((n, n)))
    assert na.project_psd_batched([]) == ([], [], 0.0)        # empty batch
    # a non-symmetric input is symmetrised, as LinearAlgebra.Symmetric does in the reference
    B = rng.standard_normal((9, 9))
    P, _, _ = na.project_psd_batched([B])
    assert np.abs(P[0] - _ref_proj(0.5 * (B + B.T))).max() <= 1e-10


@pytest.mark.parametrize("alg", [0, 2, 3])
@pytest.mark.parametrize("n", [49, 61, 90, 91, 96])
def test_projection_variants_edge_cases(alg, n, monkeypatch):
    """every sweep variant of the projection kernel (round robin in LDS, register-resident systolic, ping-pong odd-even
    with scaled rotations; NNSDP_PROJ_ALG) on the hard inputs: zero / identity / definite / rank-1 / repeated and
    clustered eigenvalues, odd sizes (a padded index travels through the positions), 1e-150 and 1e120 scales."""
    monkeypatch.setenv("NNSDP_PROJ_ALG", str(alg))
    rng = np.random.default_rng(100 * alg + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    k = n // 3
    cases = [np.zeros((n, n)), np.eye(n), -np.eye(n), (Q * np.linspace(0.1, 3, n)) @ Q.T, -(Q * np.linspace(0.1, 3, n)) @ Q.T,
             np.outer(Q[:, 0], Q[:, 0]) * 2.5, (Q * np.repeat([2.0, -1.0, 0.0], [k, k, n - 2 * k])) @ Q.T,
             (Q * np.concatenate([1.0 + 1e-9 * np.arange(k), -1.0 - 1e-7 * np.arange(k), 1e-8 * (np.arange(n - 2 * k) - 3.0)])) @ Q.T,
             np.diag(np.arange(n) - n / 2.0), _sym(rng, n, 1e-150), _sym(rng, n, 1e120), _sym(rng, n)]
    cases = [0.5 * (A + A.T) for A in cases]
    res, evs, _ = na.project_psd_batched(cases)
    for A, P, ev in zip(cases, res, evs):
        nrm = max(np.abs(A).max(), 1e-300)
        assert np.all(np.isfinite(P))
        assert np.abs(P - _ref_proj(A)).max() <= 1e-10 * nrm
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-10 * nrm
    assert np.array_equal(res[0], np.zeros((n, n)))


def test_projection_width50_path_cliques():
    """blocks of 97..110 (the 2W+1 = 101 path cliques of width-50 nets) take the 7-slot systolic instantiation."""
    rng = np.random.default_rng(11)
    mats = [_sym(rng, n) for n in (97, 101, 103, 110)]
    res, evs, _ = na.project_psd_batched(mats)
    for A, P, ev in zip(mats, res, evs):
        nrm = np.abs(A).max()
        assert np.abs(P - _ref_proj(A)).max() <= 1e-10 * nrm
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-10 * nrm


def test_projection_properties_at_full_size():
    """size-independent properties on a batch that fills the chip: 256 blocks of n = 121 (the nominal
    W40 clique) and n = 85 (the largest block the normalised W40-D20 solve sees)."""
    rng = np.random.default_rng(2)
    for n in (121, 85):
        mats = [_sym(rng, n) for _ in range(256)]
        P, _, _ = na.project_psd_batched(mats)
        Nn, _, _ = na.project_psd_batched([-A for A in mats])
        PP, _, _ = na.project_psd_batched(P[:32])
        for i, A in enumerate(mats):
            assert np.abs(P[i] - Nn[i] - A).max() <= 1e-10           # Moreau: A = P(A) - P(-A)
            assert abs(np.sum(P[i] * Nn[i])) <= 1e-8                 # complementary parts
        for i in range(32):
            assert np.abs(PP[i] - P[i]).max() <= 1e-10               # idempotence
        assert np.linalg.eigvalsh(P[7]).min() >= -1e-10


# ----------------------------------------------------------------------------- K1 / K2: assembly and adjoint
@pytest.mark.parametrize("name,beta", [("W10-D5", 0), ("W10-D5", 3), ("W10-D10", 2)])
def test_makeZ_and_adjoint_match_golden(name, beta):
    d = helpers.load_problem(name, beta)
    g = helpers.load_golden(name, beta)
    q = helpers.product_query(d)
    for gam, Z in zip(g["gammas"], g["Zs"]):
        assert np.abs(na.makeZ(q, gam) - Z).max() <= 1e-12 * np.abs(Z).max()
    for X, adj in zip(g["Xs"], g["adj"]):
        assert np.abs(na.adjoint(q, X) - adj).max() <= 1e-11 * max(1.0, np.abs(adj).max())


@pytest.mark.parametrize("out", ["hplane", "circle", "safety"])
def test_makeZ_other_output_qcs(out):
    d = helpers.load_problem("W10-D5", 3)
    qo0 = helpers.oracle_query(d)
    kw = {}
    if out == "hplane":
        kw["normal"] = [np.cos(0.7), np.sin(0.7)]
    if out == "safety":
        kw["S"] = qc.hplane_S([1.0, -2.0], 0.3, qo0.net) + 0.1 * np.eye(5)
    q, qo = helpers.product_query(d, out=out, **kw), helpers.oracle_query(d, out=out, **kw)
    gam = np.random.default_rng(4).random(qo.ngamma)
    Z = qc.assemble_Z_literal(qo, gam)
    assert np.abs(na.makeZ(q, gam) - Z).max() <= 1e-12 * np.abs(Z).max()


def test_assembly_linearity_and_adjoint_identity_full_size():
    """BASELINE sizes (W40-D20 beta=2, W40-D40 beta=0): affinity of gamma -> Z and <Z(g)-Z(0), X> = g'adj(X)."""
    rng = np.random.default_rng(5)
    for name, beta in (("W40-D20", 2), ("W40-D40", 0)):
        d = helpers.load_problem(name, beta)
        q = helpers.product_query(d)
        ng = na.methods._CProblem(q).ngamma
        g1, g2 = rng.random(ng), rng.random(ng)
        Z0, Z1, Z2 = na.makeZ(q, np.zeros(ng)), na.makeZ(q, g1), na.makeZ(q, g2)
        Z12 = na.makeZ(q, 0.3 * g1 + 1.7 * g2)
        scale = np.abs(Z12).max()
        assert np.abs((Z12 - Z0) - 0.3 * (Z1 - Z0) - 1.7 * (Z2 - Z0)).max() <= 1e-11 * scale
        assert np.abs(Z1 - Z1.T).max() == 0.0
        n = Z0.shape[0]
        X = _sym(rng, n)
        lhs = np.sum((Z1 - Z0) * X)
        rhs = g1 @ na.adjoint(q, X)
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))
        # support inside the union of clique blocks (chordal_sdp.jl:150 makes everything else 0 == 0)
        mask = np.zeros((n, n), dtype=bool)
        for c in na.makeCliques(d["xdims"], beta, na.SingleDecomp):
            mask[np.ix_(c, c)] = True
        assert np.abs(Z1[~mask]).max() == 0.0


def _high_beta_query(name, beta, out, activ="relu"):
    """a published net (tests/golden/nets) on [0.5, 1.5]^2 with plain interval arithmetic, the given output QC and activation"""
    import oracle_state as ost
    from nnsdp_amd import frontend as F
    net = ost.golden_net(name)
    if activ == "tanh":
        net = na.FeedFwdNet(xdims=list(net.xdims), Ms=net.Ms, activ=na.methods.TanhActiv)
    lo, hi = np.full(2, 0.5), np.full(2, 1.5)
    xi, acx = F.intervalsWorstCase(lo, hi, net)
    qa = F.makeQcActivsIntvs(net, xi, acx, beta)
    yc = F.evalFeedFwdNet(net, 0.5 * (lo + hi))
    rng = np.random.default_rng(10 * beta + len(net.xdims))
    qin = na.QcInputBox(x1min=lo, x1max=hi)
    if out == "ellipsoid":
        B = rng.standard_normal((2, 2))
        invP = np.linalg.inv(B @ B.T + np.eye(2))
        q = na.ReachQuery(ffnet=net, qc_input=qin, qc_reach=na.QcReachEllipsoid(invP=0.5 * (invP + invP.T), yc=yc), qc_activs=qa)
    elif out == "hplane":
        q = na.ReachQuery(ffnet=net, qc_input=qin, qc_reach=na.QcReachHplane(normal=rng.standard_normal(2)), qc_activs=qa)
    else:
        nrm = rng.standard_normal(2)
        onet = ost.mirror_query(na.ReachQuery(ffnet=net, qc_input=qin, qc_reach=na.QcReachHplane(normal=nrm), qc_activs=qa)).net
        q = na.SafetyQuery(ffnet=net, qc_input=qin, qc_safety=na.QcSafety(S=qc.hplane_S(nrm, float(nrm @ yc) + 3.0, onet)), qc_activs=qa)
    return q, ost.mirror_query(q)


HIGH_BETA = [(name, beta, out, "relu") for name in ("W10-D10", "W20-D10") for beta in (5, 6, 7)
             for out in ("ellipsoid", "hplane", "safety")] + [("W10-D10", 5, "hplane", "tanh")]


@pytest.mark.parametrize("name,beta,out,activ", HIGH_BETA)
def test_makeZ_and_adjoint_high_beta(name, beta, out, activ):
    """beta = 5..7 (the published rows' largest repeated-nonlinearity coupling) against the literal restatement: Z at 1e-12, the
    adjoint entry by entry at 1e-10"""
    q, qo = _high_beta_query(name, beta, out, activ)
    rng = np.random.default_rng(1000 + 10 * beta + len(out))
    g = rng.random(qo.ngamma)
    Zo = qc.assemble_Z_literal(qo, g)
    assert np.abs(na.makeZ(q, g) - Zo).max() <= 1e-12 * max(1.0, np.abs(Zo).max())
    X = rng.standard_normal(Zo.shape)
    X = 0.5 * (X + X.T)
    adj = na.adjoint(q, X)
    Z0 = qc.assemble_Z_literal(qo, np.zeros(qo.ngamma))
    nin, nout, n1, n2 = qo.gamma_dims()
    # every block of gamma, the sector multipliers of the beta coupling (the tail of gac2) among them
    picks = np.unique(np.concatenate([rng.choice(qo.ngamma, 8, replace=False), [0, nin, nin + nout, nin + nout + n1, qo.ngamma - 1]]))
    for i in picks:
        if i >= qo.ngamma:
            continue
        e = np.zeros(qo.ngamma)
        e[i] = 1.0
        assert abs(adj[i] - np.sum((qc.assemble_Z_literal(qo, e) - Z0) * X)) <= 1e-10 * max(1.0, np.abs(X).max() * np.abs(Zo).max()), i


def test_makeZ_matches_oracle_structured_w40_d20():
    d = helpers.load_problem("W40-D20", 0)
    q, qo = helpers.product_query(d), helpers.oracle_query(d)
    L = oop.build_operator(qo, "single")
    gam = np.random.default_rng(6).random(qo.ngamma)
    Z = L.Z_dense(gam)
    assert np.abs(na.makeZ(q, gam) - Z).max() <= 1e-12 * np.abs(Z).max()


# ----------------------------------------------------------------------------- solver
def _oracle_solve(d, mode, iters, **kw):
    qo = helpers.oracle_query(d, **kw)
    return oadmm.admm_solve(oop.build_operator(qo, mode, normalize=True), oadmm.AdmmOptions(max_iters=iters))


@pytest.mark.parametrize("name,beta,iters", [("W10-D5", 0, 1500), ("W10-D5", 3, 800), ("W10-D10", 0, 1000)])
def test_admm_tracks_oracle_iteration_for_iteration(name, beta, iters):
    d = helpers.load_problem(name, beta)
    s = na.runQuery(helpers.product_query(d), na.AdmmSdpOptions(max_iters=iters, proj_tol=1e-12, polish=False))   # exact projections, raw iterate
    r = _oracle_solve(d, "single", iters)
    assert s.summary["iters"] == r.iters
    assert s.termination_status == r.status
    assert abs(s.objective_value - r.objective) <= 1e-6 * abs(r.objective) + 1e-12
    # the residual kernels against the oracle's formulas (test_state_parity.py leg B holds them to 1e-8 from one state)
    print(f"\n{name} beta={beta}: pres / dres relative deviation {abs(s.summary['pres'] - r.pres) / r.pres:.2e} / "
          f"{abs(s.summary['dres'] - r.dres) / r.dres:.2e}")
    assert abs(s.summary["pres"] - r.pres) <= 1e-5 * r.pres + 1e-12
    assert abs(s.summary["dres"] - r.dres) <= 1e-5 * r.dres + 1e-12
    gam = np.concatenate([s.values["γin"], s.values["γout"], s.values["γac1"], s.values["γac2"]])
    assert gam.min() >= 0.0
    # values[:Z] is Z(gamma) in the reference's coordinates (Methods.jl:86)
    Zo = oop.build_operator(helpers.oracle_query(d), "dense").Z_dense(gam)
    assert np.abs(s.values["Z"] - Zo).max() <= 1e-9 * max(1.0, np.abs(Zo).max())
    assert abs(np.linalg.eigvalsh(s.values["Z"]).max() - s.summary["lambda_max"]) <= 1e-8 * max(1.0, np.abs(Zo).max())


def test_decomposition_modes_agree():
    d = helpers.load_problem("W10-D5", 0)
    q = helpers.product_query(d)
    rho = {}
    for mode in (na.SingleDecomp(), na.DoubleDecomp(), na.DenseCone(), na.PathDecomp()):
        s = na.runQuery(q, na.AdmmSdpOptions(max_iters=4000, decomp_mode=mode))
        assert s.termination_status == "OPTIMAL"
        rho[type(mode).__name__] = s.objective_value
    # reference: the three methods agree to ~1e-4 relative on every OPTIMAL row
    assert abs(rho["SingleDecomp"] - rho["DenseCone"]) <= 2e-4 * rho["DenseCone"]
    assert abs(rho["DoubleDecomp"] - rho["DenseCone"]) <= 1e-3 * rho["DenseCone"]
    assert abs(rho["PathDecomp"] - rho["DenseCone"]) <= 2e-4 * rho["DenseCone"]     # exact decomposition (extension)


@pytest.mark.parametrize("out", ["hplane", "circle", "safety"])
def test_other_queries_track_oracle(out):
    d = helpers.load_problem("W10-D5", 0)
    kw = {}
    if out == "hplane":
        kw["normal"] = [1.0, 0.0]
    if out == "safety":
        net = helpers.oracle_query(d).net
        kw["S"] = qc.hplane_S([1.0, 0.0], 10.0, net)          # y_1 <= 10: comfortably safe
    # compared at convergence: mid-trajectory iterates of these tiny-objective problems are sensitive to
    # the (deliberately inexact, 1e-10) projection tolerance of the HIP kernel
    s = na.runQuery(helpers.product_query(d, out=out, **kw), na.AdmmSdpOptions(max_iters=8000, polish=False))
    r = _oracle_solve(d, "single", 8000, out=out, **kw)
    assert s.termination_status == "OPTIMAL" and r.status == "OPTIMAL"
    assert abs(s.objective_value - r.objective) <= 1e-4 * abs(r.objective) + 1e-9
    assert ("γout" in s.values) == (out != "safety")


def _unscaled_oracle_rho(qo, mode, iters, sigma=1.0):
    """oracle ADMM in the reference's coordinates verbatim: nonzero generators only, no column / objective scaling
    (what the library runs with normalize = 0, fixed penalty); returns rho of the iterate after `iters` iterations"""
    L = oop.build_operator(qo, mode, normalize=False)
    P = oadmm.ScaledProblem.__new__(oadmm.ScaledProblem)
    A = L.A.tocsc()
    cn = np.sqrt(np.asarray(A.multiply(A).sum(axis=0)).ravel())
    P.keep = np.nonzero(cn > 1e-150)[0]
    P.ecol = np.ones(len(P.keep)); P.A = A[:, P.keep]; P.c = L.c[P.keep]; P.z0 = L.z0
    P.zscale = P.cscale = 1.0; P.pat = L.pat; P.ng_full = L.ng
    S = oadmm.AdmmState(P, sigma, 1.6)
    for _ in range(iters):
        S.step()
    y = S.sigma * (S.nu - S.proj(S.nu))
    return max(-y[list(P.keep).index(2)], 0.0)


def test_unnormalised_solver_tracks_oracle():
    """normalize=0 runs the ADMM in the reference's own coordinates (blocks up to the nominal clique size)."""
    d = helpers.load_problem("W10-D5", 0)
    s = na.runQuery(helpers.product_query(d), na.AdmmSdpOptions(max_iters=300, normalize=False, sigma=1.0, adapt_every=0, proj_tol=1e-12, polish=False))
    rho = _unscaled_oracle_rho(helpers.oracle_query(d), "single", 300)
    assert abs(s.objective_value - rho) <= 1e-6 * abs(rho) + 1e-12
    assert s.summary["max_clique"] == 31


def test_published_objective_w10_d10():
    """the reference's own golden values: dump/scale/*-scale-I2-O2-W10-D10.nnet.csv beta=0 (3 methods)."""
    pub = helpers.published_rho("W10-D10", 0)
    s = na.runQuery(helpers.product_query(helpers.load_problem("W10-D10", 0)), na.AdmmSdpOptions(max_iters=12000))
    assert min(abs(s.objective_value - p) / p for p in pub) <= 1e-3, (s.objective_value, pub)
    assert s.summary["pres"] <= 1e-5 and s.summary["dres"] <= 1e-5


@pytest.mark.parametrize("name,beta,iters", [("W10-D5", 0, 3000), ("W10-D10", 0, 12000), ("W20-D10", 0, 12000)])
def test_polished_certificate_is_feasible(name, beta, iters):
    """the returned (gamma, Z) is a certificate in the reference's sense (Methods.jl:116, acas.jl:76-79):
    gamma >= 0 and eigmax(Z(gamma)) <= tolerance in the reference's coordinates, and the polish costs
    less than 1e-3 of the objective once ADMM has converged."""
    d = helpers.load_problem(name, beta)
    s = na.runQuery(helpers.product_query(d), na.AdmmSdpOptions(max_iters=iters))
    gam = np.concatenate([s.values["γin"], s.values["γout"], s.values["γac1"], s.values["γac2"]])
    assert gam.min() >= 0.0
    Z = s.values["Z"]
    scale = np.abs(Z).max()
    lmax = np.linalg.eigvalsh(Z).max()
    assert lmax <= 1e-6, lmax                                  # the reference's OPTIMAL rows sit at 1e-7 ... 5e-6
    assert abs(lmax - s.summary["lambda_max"]) <= 1e-9 * max(1.0, scale)
    assert s.summary["polish_shift"] >= 0.0
    # a feasible point bounds the optimum from above; it must stay close to the ADMM value
    ra = s.summary["objective_admm"]
    assert s.objective_value >= ra * (1 - 1e-6) - 1e-12
    assert s.objective_value - ra <= 2e-3 * abs(ra), (s.objective_value, ra)


@pytest.mark.parametrize("name,beta,mode", [("W10-D10", 0, "double"), ("W40-D20", 0, "double"), ("W40-D20", 0, "path"), ("W40-D20", 2, "path")])
def test_certified_gap_stopping_rule(name, beta, mode):
    """cert_tol: stop as soon as the polished, exactly feasible objective is within 1e-3 of the ADMM estimates, those being trusted
    once the residuals are below a tenth of cert_tol.  The result is a valid certificate whose objective upper-bounds the
    converged optimum (oracle fixture where there is one) by <= 1e-3 - the epsilon of SURVEY section 8d."""
    import json, os
    q = helpers.product_query(helpers.load_problem(name, beta))
    dm = na.DoubleDecomp() if mode == "double" else na.PathDecomp()
    fast = na.runQuery(q, na.AdmmSdpOptions(max_iters=400000, decomp_mode=dm, cert_tol=1e-3, max_time=100))
    key = f"{name}_b{beta}"
    fixture = json.load(open(os.path.join(helpers.GOLDEN, "oracle_optimum.json")))
    if key in fixture:
        opt = fixture[key]["rho"]
    else:
        full = na.runQuery(q, na.AdmmSdpOptions(max_iters=400000, decomp_mode=dm, max_time=100))
        assert fast.summary["iters"] < full.summary["iters"]
        opt = full.summary["objective_admm"]
    assert fast.termination_status == "OPTIMAL"
    assert fast.summary["lambda_max"] <= 1e-6 and min(np.min(fast.values[k]) for k in ("γin", "γout", "γac1", "γac2")) >= 0.0
    assert fast.objective_value >= opt * (1 - 1e-4)
    # SURVEY section 8d's epsilon; the residual sums are added in a fixed order (k_acc_reduce), so the stopping iteration is reproducible
    assert fast.objective_value - opt <= 1e-3 * opt, (fast.objective_value, opt, fast.summary["iters"])


def test_solve_is_reproducible_run_to_run():
    """no atomics on the way to a stopping / penalty decision: two runs of one solve stop at the same iteration with the same bits"""
    q = helpers.product_query(helpers.load_problem("W40-D20", 0))
    o = na.AdmmSdpOptions(max_iters=400000, decomp_mode=na.DoubleDecomp(), cert_tol=1e-3, max_time=100)
    a, b = na.runQuery(q, o), na.runQuery(q, o)
    assert a.summary["iters"] == b.summary["iters"] and a.termination_status == b.termination_status
    for k in ("γin", "γout", "γac1", "γac2"):
        assert np.array_equal(a.values[k], b.values[k]), k
    assert a.summary["pres"] == b.summary["pres"] and a.summary["dres"] == b.summary["dres"]


def test_full_size_solver_invariants_w40_d20():
    """BASELINE configs[2] at full size: residuals decrease, gamma >= 0, Z symmetric and on the pattern."""
    d = helpers.load_problem("W40-D20", 0)
    sv = na.Solver(helpers.product_query(d), na.AdmmSdpOptions(max_iters=10 ** 8))
    sv.iterate(200)
    p1, d1, _, _ = sv.residuals()
    sv.iterate(1500)
    p2, d2, pobj, dobj = sv.residuals()
    assert np.isfinite([p2, d2, pobj, dobj]).all()
    assert p2 < p1 and max(p2, d2) < 0.5 * max(p1, d1)
    s = sv.finish()
    sv.close()
    assert s.summary["n_cliques"] == 19 and s.summary["max_clique"] <= 121
    gam = np.concatenate([s.values["γin"], s.values["γout"], s.values["γac1"], s.values["γac2"]])
    assert gam.min() >= 0.0 and len(gam) == 3203
    Z = s.values["Z"]
    assert Z.shape == (803, 803) and np.abs(Z - Z.T).max() == 0.0


def test_w40_d40_double_decomposition_runs_to_certificate():
    """BASELINE configs[3] shape (W=40, D=40: Zdim 1603, 6403 multipliers) on one GPU, Double decomposition,
    certified-gap rule: a valid certificate (gamma >= 0, eigmax(Z) <= 1e-6) whose objective matches the ADMM
    primal/dual estimates to 1e-3."""
    d = helpers.load_problem("W40-D40", 0)
    s = na.runQuery(helpers.product_query(d), na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp(), max_iters=60000, cert_tol=1e-3, max_time=120))
    assert s.values["Z"].shape == (1603, 1603)
    gam = np.concatenate([s.values["γin"], s.values["γout"], s.values["γac1"], s.values["γac2"]])
    assert len(gam) == 6403 and gam.min() >= 0.0
    assert s.termination_status == "OPTIMAL", (s.termination_status, s.summary)
    assert s.summary["lambda_max"] <= 1e-6
    assert abs(s.objective_value - s.summary["objective_admm"]) <= 2e-3 * abs(s.objective_value)


def test_acas_shaped_safety_query_tracks_oracle():
    """BASELINE configs[4] kind of query: no ACAS file is in the reference checkout, so a synthetic 5-40x6-5 ReLU
    net (scripts/make_networks.jl distribution), box of half-width 0.05, hyperplane safety S (Utils/qc.jl:27-37),
    objective sum(gamma) (deep_sdp.jl:25).  GPU ADMM vs oracle ADMM after the same number of iterations.
    (The real ACAS width of 50 gives 151-wide cliques: see the blocks-above-128 tests below.)"""
    from oracle import nnet_io, qc as oqc
    net = nnet_io.random_net([5] + [40] * 6 + [5], seed=1234)
    x0 = np.full(5, 0.3)
    lo, hi = x0 - 0.05, x0 + 0.05
    y0 = nnet_io.eval_net(net, x0)
    normal = np.zeros(5); normal[0] = 1.0
    S = oqc.hplane_S(normal, float(y0[0]) + 5.0, net)               # y_1 <= y_1(x0) + 5
    qo = oqc.make_safety_query(net, lo, hi, 1, S)
    qb = na.QcActivBounded(acymin=qo.qc_bounded.acymin, acymax=qo.qc_bounded.acymax)
    qs = na.QcActivSector(acxdim=240, beta=1, smin=qo.qc_sector.smin, smax=qo.qc_sector.smax)
    q = na.SafetyQuery(ffnet=na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms), qc_input=na.QcInputBox(x1min=lo, x1max=hi),
                       qc_safety=na.QcSafety(S=S), qc_activs=[qb, qs])
    assert [len(c) for c in na.makeCliques([5] + [50] * 6 + [5], 0, na.SingleDecomp)] == [106, 151, 151, 151, 151]
    acas = na.SafetyQuery(ffnet=na.FeedFwdNet(xdims=[5] + [50] * 6 + [5], Ms=nnet_io.random_net([5] + [50] * 6 + [5], seed=1).Ms),
                          qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_safety=na.QcSafety(S=S),
                          qc_activs=[na.QcActivBounded(acymin=np.zeros(300), acymax=np.ones(300)),
                                     na.QcActivSector(acxdim=300, beta=0, smin=np.zeros(300), smax=np.ones(300))])
    # (blocks above 128 run through the library path: test_blocks_above_128_width_50_safety_query_in_the_reference_cliques)
    # the path decomposition (extension, exact for hyperplane safety sets: S12 = 0) keeps width-50 blocks at 2W+1 = 101
    sp = na.runQuery(acas, na.AdmmSdpOptions(max_iters=60, decomp_mode=na.PathDecomp()))
    assert sp.summary["max_clique"] <= 103 and np.isfinite(sp.objective_value)
    # ... and is refused when the safety set couples x_1 with the output
    Sc = S.copy(); Sc[0, 5] = Sc[5, 0] = 1.0
    acas2 = na.SafetyQuery(ffnet=acas.ffnet, qc_input=acas.qc_input, qc_safety=na.QcSafety(S=Sc), qc_activs=acas.qc_activs)
    with pytest.raises(na._lib.NnsdpError) as ei2:
        na.runQuery(acas2, na.AdmmSdpOptions(max_iters=10, decomp_mode=na.PathDecomp()))
    assert "S12" in str(ei2.value)
    # AutoDecomp (nnsdp.h: NNSDP_DECOMP_AUTO) takes the path cliques where the query allows them and the Double ones where not
    sa = na.runQuery(acas, na.AdmmSdpOptions(max_iters=60, decomp_mode=na.AutoDecomp()))
    assert (sa.summary["n_cliques"], sa.summary["max_clique"]) == (sp.summary["n_cliques"], sp.summary["max_clique"])
    assert sa.objective_value == sp.objective_value
    sd2 = na.runQuery(acas2, na.AdmmSdpOptions(max_iters=60, decomp_mode=na.DoubleDecomp()))
    sa2 = na.runQuery(acas2, na.AdmmSdpOptions(max_iters=60, decomp_mode=na.AutoDecomp()))
    assert (sa2.summary["n_cliques"], sa2.summary["max_clique"]) == (sd2.summary["n_cliques"], sd2.summary["max_clique"])
    assert sa2.objective_value == sd2.objective_value
    iters = 400
    s = na.runQuery(q, na.AdmmSdpOptions(max_iters=iters, proj_tol=1e-12, polish=False))
    r = oadmm.admm_solve(oop.build_operator(qo, "single", normalize=True), oadmm.AdmmOptions(max_iters=iters))
    assert s.summary["iters"] == r.iters
    assert abs(s.objective_value - r.objective) <= 1e-5 * abs(r.objective) + 1e-9
    assert "γout" not in s.values and len(s.values["γac2"]) == qs.vardim
    Zo = oop.build_operator(qo, "dense").Z_dense(np.concatenate([s.values["γin"], s.values["γac1"], s.values["γac2"]]))
    assert np.abs(s.values["Z"] - Zo).max() <= 1e-9 * max(1.0, np.abs(Zo).max())


def test_solver_batch_matches_single_solves():
    """independent SDPs advanced in lockstep by the batch handle (one launch per stage for all of them, mixed sizes)
    give exactly the iterates of the same problems solved one after the other; so does the one-stream-per-SDP form."""
    ds = [helpers.load_problem("W10-D5", 0), helpers.load_problem("W10-D5", 3), helpers.load_problem("W10-D10", 0)]
    qs = [helpers.product_query(d) for d in ds]
    opts = na.AdmmSdpOptions(max_iters=10 ** 8, proj_tol=1e-12)
    sb = na.SolverBatch(qs, opts)
    sb.iterate(300)
    rb = sb.residuals()
    sb.close()
    ss = na.SolverBatch(qs, opts)
    ss.iterate_streams(300)
    rs = ss.residuals()
    ss.close()
    for q, r, r2 in zip(qs, rb, rs):
        sv = na.Solver(q, opts)
        sv.iterate(300)
        r1 = sv.residuals()
        sv.close()
        assert np.allclose(r, r1, rtol=1e-9, atol=1e-14)
        assert np.allclose(r2, r1, rtol=1e-9, atol=1e-14)


def test_run_queries_batched_matches_run_query():
    """full solves through the batch handle: per-SDP stopping (the three problems need different iteration counts, so
    the batch shrinks twice), certificate polish and result packaging as in runQuery."""
    ds = [helpers.load_problem("W10-D5", 0), helpers.load_problem("W10-D10", 2), helpers.load_problem("W10-D5", 3)]
    qs = [helpers.product_query(d) for d in ds]
    opts = na.AdmmSdpOptions(max_iters=200000, eps_rel=1e-6)
    sols = na.runQueries(qs, opts)
    its = []
    for q, sb in zip(qs, sols):
        s1 = na.runQuery(q, opts)
        assert sb.termination_status == s1.termination_status == "OPTIMAL"
        assert abs(sb.objective_value - s1.objective_value) <= 2e-6 * abs(s1.objective_value)
        assert sb.summary["lambda_max"] <= 1e-6 and all(np.all(sb.values[k] >= 0) for k in ("γin", "γac1", "γac2", "γout"))
        assert sb.summary["iters"] == s1.summary["iters"]      # same stopping rule on the same iterates
        its.append(sb.summary["iters"])
    assert len(set(its)) > 1
    with pytest.raises(na._lib.NnsdpError):
        na.SolverBatch([], opts)


def test_batch_handle_limits_and_errors():
    """per-SDP options in a batch: one SDP runs into its iteration limit while the other converges; argument errors."""
    q0 = helpers.product_query(helpers.load_problem("W10-D5", 0))
    q1 = helpers.product_query(helpers.load_problem("W10-D5", 3))
    sols = na.runQueries([q0, q1], [na.AdmmSdpOptions(max_iters=200), na.AdmmSdpOptions(max_iters=200000, eps_rel=1e-6)])
    assert sols[0].termination_status == "ITERATION_LIMIT" and sols[0].summary["iters"] == 200
    assert sols[1].termination_status == "OPTIMAL" and sols[1].summary["iters"] > 200
    ref = na.runQuery(q1, na.AdmmSdpOptions(max_iters=200000, eps_rel=1e-6))
    assert abs(sols[1].objective_value - ref.objective_value) <= 2e-6 * abs(ref.objective_value)
    with pytest.raises(ValueError):
        na.SolverBatch([q0, q1], [na.AdmmSdpOptions()])
    with pytest.raises(na._lib.NnsdpError) as ei:
        na.SolverBatch([q0, q1], [na.AdmmSdpOptions(check_every=50), na.AdmmSdpOptions(check_every=25)])
    assert "check_every" in str(ei.value)
    sb = na.SolverBatch([q0], na.AdmmSdpOptions())
    with pytest.raises(na._lib.NnsdpError):
        sb.iterate(-1)
    sb.iterate(0)
    sb.close()


def test_clique_sharded_mode_single_rank_rccl():
    """the clique-sharded code path (own-clique projection, RCCL all-reduce of the consensus sum, replicated
    operator kernels) with a one-rank communicator must reproduce the unsharded iteration.  Multi-rank logic is
    covered on CPU by tests/test_distributed_cpu.py (gloo, world size 2)."""
    d = helpers.load_problem("W10-D10", 0)
    q = helpers.product_query(d)
    opts = na.AdmmSdpOptions(max_iters=10 ** 8, proj_tol=1e-12)
    a = na.Solver(q, opts)
    a.iterate(250)
    ra = a.residuals()
    a.close()
    b = na.Solver(q, opts)
    b.set_comm(1, 0, na.comm_unique_id())
    b.iterate(250)
    graphs = b.info(0), b.info(1)
    rb = b.residuals()
    sb = b.finish()
    b.close()
    assert np.allclose(ra, rb, rtol=1e-8, atol=1e-13), (ra, rb)
    assert np.isfinite(sb.objective_value)
    # the sharded iteration replays a hipGraph with the ncclAllReduce inside it when this ROCm's RCCL can be captured (probed at set_comm)
    print("RCCL all-reduce capturable into a hipGraph:", bool(graphs[1]), "- graph launches in 250 iterations:", int(graphs[0]))
    assert (graphs[0] > 0) == bool(graphs[1])
    import json, time
    os.makedirs(os.path.join(helpers.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(helpers.ROOT, "gpurun_out", "rccl_one_rank_graph.json"), "w") as fh:      # (a silently eager fall-back shows here)
        json.dump({"rccl_allreduce_capturable": bool(graphs[1]), "graph_launches_in_250_iterations": int(graphs[0])}, fh)
    for capture in ("1", "0"):       # control-flow cost of the sharded iteration on one card: eager vs graph replay vs unsharded
        os.environ["NNSDP_NO_RCCL_GRAPH"] = "0" if capture == "1" else "1"
        e = na.Solver(helpers.product_query(helpers.load_problem("W40-D20", 0)), na.AdmmSdpOptions(max_iters=10 ** 8))
        e.set_comm(1, 0, na.comm_unique_id())
        e.iterate(600)
        t0 = time.perf_counter(); e.iterate(800); dt = time.perf_counter() - t0
        print(f"W40-D20 one-rank RCCL sharded iteration, all-reduce in hipGraph {capture}: {1e6 * dt / 800:.1f} us/iteration (graph launches {int(e.info(0))})")
        e.close()
    os.environ.pop("NNSDP_NO_RCCL_GRAPH", None)
    c = na.Solver(q, opts)
    c.iterate(5)
    with pytest.raises(na._lib.NnsdpError):
        c.set_comm(1, 0, na.comm_unique_id())                # only before the first iteration
    c.close()


def test_solver_argument_errors():
    d = helpers.load_problem("W10-D5", 0)
    q = helpers.product_query(d)
    for bad in (dict(max_iters=0), dict(alpha=2.5), dict(sigma=-1.0), dict(decomp_mode=7)):
        with pytest.raises(na._lib.NnsdpError) as ei:
            na.runQuery(q, na.AdmmSdpOptions(**bad))
        assert ei.value.code < 0
    with pytest.raises(ValueError):
        na.makeZ(q, np.zeros(5))
    for bad in (dict(interval_guard=-1.0), dict(interval_guard=0.5)):
        with pytest.raises(na._lib.NnsdpError):
            na.runQuery(q, na.AdmmSdpOptions(**bad))


def test_blocks_above_128_dense_cone_w10_d20_tracks_oracle():
    """DeepSdpOptions' single cone (src/Methods/deep_sdp.jl:57) on W10-D20: Zdim 203 > 128, so the block goes through the
    library path (rocSOLVER dsyevd + rocBLAS dgemm) instead of the LDS-resident Jacobi kernel.  Same iterates as the oracle
    ADMM on the dense cone, and the same optimum as the Double decomposition of the same problem."""
    d = helpers.load_problem("W10-D20", 0)
    q, qo = helpers.product_query(d), helpers.oracle_query(d)
    iters = 300
    # the solver's normalisation drops the 97 fixed neurons: one cone of 106, still the LDS kernel
    s = na.runQuery(q, na.AdmmSdpOptions(decomp_mode=na.DenseCone(), max_iters=iters, polish=False))
    assert s.summary["n_cliques"] == 1 and s.summary["max_clique"] == 106
    r = oadmm.admm_solve(oop.build_operator(qo, "dense", normalize=True), oadmm.AdmmOptions(max_iters=iters))
    assert s.summary["iters"] == r.iters
    assert abs(s.objective_value - r.objective) <= 1e-6 * abs(r.objective) + 1e-9
    # the reference's coordinates verbatim: one 203 x 203 cone through the library path
    s0 = na.runQuery(q, na.AdmmSdpOptions(decomp_mode=na.DenseCone(), normalize=False, max_iters=iters, sigma=1.0, adapt_every=0, polish=False))
    assert s0.summary["n_cliques"] == 1 and s0.summary["max_clique"] == 203 and s0.summary["iters"] == iters
    rho0 = _unscaled_oracle_rho(qo, "dense", iters)
    assert abs(s0.objective_value - rho0) <= 1e-6 * abs(rho0) + 1e-12


@pytest.mark.parametrize("n", [129, 151, 160])
def test_packed_variant_blocks_129_to_160_warm_and_cold_against_lapack(n):
    """blocks 129 .. 160 (the reference's 151-wide cliques) in the LDS-resident kernel's packed-triangle variant: cold start through
    nnsdp_project_psd_batched and the warm form a solve uses (basis of the previous projection, HBM scratch for the congruence)"""
    rng = np.random.default_rng(n)
    spec = np.concatenate([np.linspace(0.05, 2.0, n - n // 3), -np.linspace(0.05, 1.0, n // 3)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A0 = (Q * spec) @ Q.T
    P, ev, _ = na.project_psd_batched([A0, A0[:57, :57]])
    for Pk, Ak in zip(P, (A0, A0[:57, :57])):
        w, U = np.linalg.eigh(Ak)
        assert np.abs(Pk - (U * np.maximum(w, 0)) @ U.T).max() <= 1e-10 * np.abs(Ak).max()
    assert np.abs(np.sort(ev[0]) - spec[np.argsort(spec)]).max() <= 1e-10
    for eta, tol in ((1e-3, 1e-6), (1e-6, 1e-9)):
        D = rng.standard_normal((n, n)); D = 0.5 * (D + D.T)
        A1 = A0 + eta * np.linalg.norm(A0) / np.linalg.norm(D) * D
        W, V, oc, _ = na.project_psd_warm([A1], [Q], tol, refine=False)      # (the packed sweeps alone; the stage in its packed form: tests/test_refine_projection.py)
        w, U = np.linalg.eigh(A1)
        assert np.linalg.norm(W[0] - (U * np.maximum(w, 0)) @ U.T) <= tol * np.linalg.norm(A1)
        assert np.linalg.norm(V[0].T @ V[0] - np.eye(n)) <= 1e-10
        assert oc == [0, 0, 0, 0, 0]


def test_blocks_above_128_width_50_safety_query_in_the_reference_cliques():
    """the 5-50x6-5 (ACAS-Xu shaped) safety query in the reference's OWN Single / Double cliques (106, 151 x 4;
    chordal_cliques.jl:33-36) - blocks of 151 > 128: library path for those, LDS kernel for the rest - against the oracle."""
    from oracle import nnet_io, qc as oqc
    net = nnet_io.random_net([5] + [50] * 6 + [5], seed=1)
    x0 = np.full(5, 0.3)
    lo, hi = x0 - 0.05, x0 + 0.05
    y0 = nnet_io.eval_net(net, x0)
    normal = np.zeros(5); normal[0] = 1.0
    S = oqc.hplane_S(normal, float(y0[0]) + 5.0, net)
    qo = oqc.make_safety_query(net, lo, hi, 0, S)
    q = na.SafetyQuery(ffnet=na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms), qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_safety=na.QcSafety(S=S),
                       qc_activs=[na.QcActivBounded(acymin=qo.qc_bounded.acymin, acymax=qo.qc_bounded.acymax),
                                  na.QcActivSector(acxdim=300, beta=0, smin=qo.qc_sector.smin, smax=qo.qc_sector.smax)])
    iters = 150
    # fixed penalty and exact projections: this transient is sensitive (the objective is a sum of ~1200 multipliers of size
    # 1e2 .. 1e3; one flipped penalty decision changes it by a factor), so the comparison is iterate for iterate
    s = na.runQuery(q, na.AdmmSdpOptions(max_iters=iters, decomp_mode=na.SingleDecomp(), proj_tol=1e-12, adapt_every=0, polish=False))
    r = oadmm.admm_solve(oop.build_operator(qo, "single", normalize=True), oadmm.AdmmOptions(max_iters=iters, adapt_sigma=False))
    assert s.summary["iters"] == r.iters and s.summary["max_clique"] == 151 and s.summary["n_cliques"] == 5
    assert abs(s.objective_value - r.objective) <= 1e-8 * abs(r.objective), (s.objective_value, r.objective)
    # Double: the last clique (151) is not split by the reference either; identical index sets are merged by the library, so the
    # iteration differs from the oracle's - same optimum (test_decomposition_modes_agree); here: it runs and stays finite
    sd = na.runQuery(q, na.AdmmSdpOptions(max_iters=iters, decomp_mode=na.DoubleDecomp(), polish=False))
    assert sd.summary["max_clique"] == 151 and np.isfinite(sd.objective_value)
    # the same query through the batch handle (two copies in lockstep: the 106-block of both in ONE launch of the LDS kernel, their
    # 151-blocks through the library path on the batch's stream) and through the clique-sharded mode (one-rank RCCL): the iterates of
    # the plain solve.  BASELINE config 5's shape in the reference's own decomposition, batched and sharded.
    o = na.AdmmSdpOptions(max_iters=10 ** 8, decomp_mode=na.SingleDecomp(), proj_tol=1e-12, adapt_every=0, proj_refine=0)
    ref = na.Solver(q, o)
    ref.iterate(120)
    r_ref = ref.residuals()
    ref.close()
    sb = na.SolverBatch([q, q], o)
    sb.iterate(120)
    for rr in sb.residuals():      # (the batch applies M^-1 through its tiled symmetric form: other rounding, and this transient amplifies it)
        assert np.allclose(rr, r_ref, rtol=1e-6, atol=1e-9), (rr, r_ref)
    sb.close()
    sh = na.Solver(q, o)
    sh.set_comm(1, 0, na.comm_unique_id())
    sh.iterate(120)
    r_sh = sh.residuals()
    sh.close()
    assert np.allclose(r_sh, r_ref, rtol=1e-6, atol=1e-9), (r_sh, r_ref)
    bn, st = na.shardPlan(q, o, 2)
    assert bn == [106, 151, 151, 151, 151] and st == [0, 3, 5]      # load-balanced by n^3: 106 + 151 + 151 | 151 + 151


def _oracle_optimum():
    import json, os
    p = os.path.join(helpers.GOLDEN, "oracle_optimum.json")
    return json.load(open(p)) if os.path.exists(p) else {}


@pytest.mark.parametrize("key", sorted(_oracle_optimum()))
def test_baseline_configs_match_the_oracle_optimum(key):
    """BASELINE.json's own configs have no published value: the converged optimum of the CPU oracle (numpy ADMM to 1e-6
    residuals, tests/golden/make_oracle_optimum.py, run in the build container) is the pin.  The HIP solver's converged rho,
    through BOTH chordal decompositions, within SURVEY section 8d's epsilon-certificate tolerance: 1e-3 |rho| + 1e-9 (measured
    agreement of the raw iterates: 1e-6 .. 3e-5)."""
    g = _oracle_optimum()[key]
    q = helpers.product_query(helpers.load_problem(g["net"], g["beta"]))
    # every pin is a run to OPTIMAL at residuals 1e-6 (W40-D40: 273 600 iterations of the C++ port of the oracle's loop,
    # tests/golden/make_oracle_optimum_c.py; the numpy loop of round 2 had stopped at its 200 000-iteration cap with 1.3e-6)
    assert g["status"] == "OPTIMAL" and max(g["pres"], g["dres"]) <= 1e-6 and g["gamma_min"] >= 0.0
    # W40-D40 through Single creeps over the last 10 % of the way to 1e-6 and trips the 50 000-iteration stall detector first
    # (SLOW_PROGRESS at 1.2e-6): that config is held to the pin through the decomposition the pin was made with
    modes = (na.DoubleDecomp(),) if g["net"] == "W40-D40" else (na.DoubleDecomp(), na.SingleDecomp())
    for mode in modes:
        s = na.runQuery(q, na.AdmmSdpOptions(decomp_mode=mode, max_iters=400000, eps_rel=1e-6, max_time=150))
        assert s.termination_status == "OPTIMAL" and max(s.summary["pres"], s.summary["dres"]) <= 1e-6, \
            (key, type(mode).__name__, s.termination_status, s.summary)
        tol = 1e-3 * abs(g["rho"]) + 1e-9
        assert abs(s.objective_value - g["rho"]) <= tol, (key, type(mode).__name__, s.objective_value, g["rho"])
        assert abs(s.summary["objective_admm"] - g["rho"]) <= 0.1 * tol          # the raw iterates agree much more closely
        assert s.summary["lambda_max"] <= 1e-6 and min(np.min(s.values[k]) for k in ("γin", "γout", "γac1", "γac2")) >= 0.0


def test_structured_minv_matches_the_dense_inverse():
    """the Woodbury core M^-1 (M = I + A'D^-1A over the kept multipliers) in its structured form - block-banded by network layer
    plus the low-rank term of the affine-affine entry, two-level domain decomposition, three launches (csrc/minv.hpp) - against
    the dense inverse: same vector to 1e-10, a fraction of the bytes, and the same ADMM iterates."""
    rng = np.random.default_rng(11)
    for name, beta in (("W40-D20", 2), ("W40-D40", 0)):
        q = helpers.product_query(helpers.load_problem(name, beta))
        # (proj_refine=0: exact sweeps in both, so that the iterates differ by the two forms of M^-1 alone - the refinement stage
        # takes accept / reject decisions at thresholds, which amplify a 1e-10 difference into different, equally valid, iterates)
        sd = na.Solver(q, na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp(), minv_mode=1, proj_refine=0))
        ss = na.Solver(q, na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp(), minv_mode=2, proj_refine=0))
        for _ in range(3):
            v = rng.standard_normal(sd.cp.ngamma)
            a, stra, ba = sd.apply_minv(v)
            b, strb, bb = ss.apply_minv(v)
            assert not stra and strb
            assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max(), (name, np.abs(a - b).max(), np.abs(a).max())
        assert bb <= 0.5 * ba, (name, bb, ba)
        sd.advance(1500); ss.advance(1500)
        rd, rs = sd.finish(), ss.finish()
        assert abs(rd.summary["objective_admm"] - rs.summary["objective_admm"]) <= 1e-7 * abs(rd.summary["objective_admm"])
        sd.close(); ss.close()
    # auto mode on a big multiplier count: W20-D100 beta = 7 (22 013 multipliers; dense inverse ~1 GB)
    d = np.load(__import__("os").path.join(helpers.GOLDEN, "nets", "scale-I2-O2-W20-D100.npz"))
    xd = [int(v) for v in d["xdims"]]
    net = na.FeedFwdNet(xdims=xd, Ms=[np.array(d[f"M{k}"]) for k in range(len(xd) - 1)])
    qq, _, _ = na.ellipsoidQuery(net, [0.5, 0.5], [1.5, 1.5], 7)
    sa = na.Solver(qq, na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp()))
    out, structured, nbytes = sa.apply_minv(rng.standard_normal(sa.cp.ngamma))
    assert structured and nbytes <= 300e6 and np.all(np.isfinite(out))        # measured 269 MB; the dense inverse would be ~1 GB
    sa.close()
    with pytest.raises(na._lib.NnsdpError):          # a 5-layer net has too few layers to cut: structured mode is refused, not faked
        na.Solver(helpers.product_query(helpers.load_problem("W10-D5", 0)), na.AdmmSdpOptions(minv_mode=2))


def test_degenerate_input_box_is_certified():
    """an input coordinate with x1min == x1max is eliminated by the normalisation like a fixed neuron; its cost-free multiplier
    gin_i is raised in the returned certificate (it used to stay 0 and the result was never certifiable)."""
    d = helpers.load_problem("W10-D5", 0)
    xd = [int(v) for v in d["xdims"]]
    net = na.FeedFwdNet(xdims=xd, Ms=helpers.problem_Ms(d))
    lo, hi = np.array([0.5, 1.0]), np.array([1.5, 1.0])
    normal = np.array([1.0, 0.0])
    q = na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_reach=na.QcReachHplane(normal=normal),
                      qc_activs=na.makeQcActivs(net, lo, hi, 0))
    s = na.runQuery(q, na.AdmmSdpOptions(max_iters=200000, eps_rel=1e-6))
    assert s.termination_status == "OPTIMAL"
    assert s.summary["lambda_max"] <= 1e-6 and min(np.min(s.values[k]) for k in ("γin", "γout", "γac1", "γac2")) >= 0.0
    X = np.stack([0.5 + np.random.default_rng(0).random(5000), np.ones(5000)])
    assert np.max(normal @ na.evalFeedFwdNet(net, X)) <= s.objective_value + 1e-9          # a sound bound on the slice
    assert s.values["γin"][1] > 0.0                                                          # the eliminated coordinate's multiplier


def test_woodbury_core_does_not_depend_on_the_host_thread_count(monkeypatch):
    """M = I + A'D^-1A is assembled by host threads that own disjoint column ranges (round 4): every entry is accumulated by one thread
    in the row order of A, so M^-1 q must come out bit for bit the same with 1, 3 and 4 threads"""
    import hashlib
    q = helpers.product_query(helpers.load_problem("W40-D20", 0))
    dig = []
    for t in ("1", "3", "4"):
        monkeypatch.setenv("NNSDP_HOST_THREADS", t)
        s = na.Solver(q, na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp(), minv_mode=1))
        v = np.cos(np.arange(s.cp.ngamma) * 0.37)
        dig.append(hashlib.sha256(s.apply_minv(v)[0].tobytes()).hexdigest())
        s.close()
    assert dig[0] == dig[1] == dig[2]
