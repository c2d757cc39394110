"""The HIP solver's bound against exact ranges and against the independent interior point (run with -m gpu on an MI355X).  The table, the
two interval sources and the fixture are those of tests/sdp_truth_common.py; tests/test_sdp_truth_cpu.py holds the oracle to the same truth.

Every solve is held to two statements, neither of which reads anything the HIP solver computed:
  soundness   rho >= w - max(0, lambda_max(Z)) |z|^2 - 1e-12 (1 + |w|), Z = makeZ(q, gamma) and z lifted at the stored witness of the
              attained value w (the statement of tests/test_exact_soundness_gpu.py), every multiplier >= 0, gamma_out among them;
  two-sided   lower - 1e-9 <= rho <= upper (1 + 1e-3) + 1e-9 with [lower, upper] the interior point's bracket in
              tests/golden/sdp_truth.json (the rule of cert_tol and of test_baseline_configs_match_the_oracle_optimum); the bracket is
              taken over four runs of the interior point, because one run's residuals do not bracket these optima
              (sdp_truth_common.ipm_bracket), and with "product" intervals it is the bracket of the product's own QCs.
The upper side is asserted on every solve, the degenerate boxes (stable, point) and the solves that end at the iteration limit included;
only a solve that was told to stop at a target above the optimum is held to its target instead.  Default AdmmSdpOptions() (max_iters = 20 000) unless a test says otherwise."""
import numpy as np
import pytest

import nnsdp_amd as na
import oracle_state as ost
import sdp_truth_common as sc
from nnsdp_amd import vnnlib as vl
from oracle import ipm, qc

pytestmark = pytest.mark.gpu

MODES = {"double": na.DoubleDecomp, "path": na.PathDecomp, "dense": na.DenseCone, "auto": na.AutoDecomp}


def gamma_of(s):
    v = s.values
    return np.concatenate([v["γin"], v["γout"], v["γac1"], v["γac2"]])


def held(cs, q, s, label="", upper=True):
    """the two statements of the module docstring for one solution of the case -> True where the upper side was asserted.  upper=False:
    a solve that was told to stop at a target above the optimum; its caller asserts objective <= target instead"""
    g, val = sc.stored(cs), s.values
    Z = na.makeZ(q, gamma_of(s))
    lam = float(np.linalg.eigvalsh(0.5 * (Z + Z.T))[-1])
    z = sc.lifted(cs, np.array(g["x"]))
    w, rho = float(g["w"]), float(s.objective_value)
    room = max(0.0, lam) * float(z @ z)
    upper_cap = g["upper"] * (1.0 + 1e-3) + 1e-9
    print(f"{sc.key(cs)} {label}: rho {rho:.10f} w {w:.10f} (rho - w {rho - w:+.3e}) ipm [{g['lower']:.10f}, {g['upper']:.10f}] (rho - rho_ipm {rho - g['upper']:+.3e}) "
          f"{s.termination_status} at {s.summary['iters']}, lambda_max(Z) {lam:+.2e}, room {room:.2e}")
    assert s.termination_status != "NUMERICAL_ERROR" and np.isfinite(rho)
    assert rho == float(val["γout"][0])
    assert min(val["γin"].min(), val["γout"].min(), val["γac1"].min(), val["γac2"].min()) >= 0.0
    assert rho >= w - room - 1e-12 * (1.0 + abs(w)), (sc.key(cs), label, rho - w, room)
    assert rho >= g["lower"] - 1e-9, (sc.key(cs), label, rho - g["lower"])
    if not upper:
        return False
    assert rho <= upper_cap, (sc.key(cs), label, s.termination_status, rho - upper_cap)
    return True


def solve(cs, **opts):
    q = sc.product_query(cs)
    return q, na.runQuery(q, na.AdmmSdpOptions(**opts))


# ----------------------------------------------------------------------------- ReLU hyperplane, Single decomposition
@pytest.mark.parametrize("cs", sc.relu_hplane_cases("exact") + sc.relu_hplane_cases("product"), ids=sc.key)
def test_relu_hyperplane_bound_is_sound_and_in_the_bracket(cs):
    """both nets; "exact" intervals on root, half-a, small-a, edge0, stable, point and "product" intervals on root, half-a, edge0; the
    largest direction and the largest literal direction; beta 0 and 2.  With "product" the product's own float32 routine builds the QCs,
    for the solve and for the interior point's bracket alike"""
    q, s = solve(cs)
    assert held(cs, q, s)


# ----------------------------------------------------------------------------- the other decompositions
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cs", [sc.make(n, "relu", b, "hplane", "top", beta, "exact") for n in sc.NETS for b in ("root", "half-a") for beta in sc.BETAS], ids=sc.key)
def test_every_decomposition_lands_in_the_same_bracket(cs, mode):
    """Double, Path, Dense and Auto: a chordal decomposition does not move the optimum, so the bracket of the dense interior point holds"""
    q, s = solve(cs, decomp_mode=MODES[mode]())
    assert held(cs, q, s, mode)


# ----------------------------------------------------------------------------- the optimum that is exactly 0
@pytest.mark.parametrize("cs", sc.negative_cases(), ids=sc.key)
def test_a_negative_maximum_gives_exactly_zero(cs):
    """a direction whose exact maximum on half-a is negative (-0.42, -0.59): gamma_out >= 0 makes the optimum exactly 0, so soundness
    says nothing here and the expectation is |rho| <= 1e-9, a finite status and multipliers >= 0"""
    q, s = solve(cs)
    g, val = sc.stored(cs), s.values
    print(f"{sc.key(cs)}: rho {s.objective_value:+.3e} (w {g['w']:+.6f}, rho_ipm {g['rho_ipm']:+.3e}) {s.termination_status} at {s.summary['iters']}")
    assert g["w"] <= -sc.W_MIN and s.termination_status != "NUMERICAL_ERROR"
    assert abs(s.objective_value) <= 1e-9
    assert min(val["γin"].min(), val["γout"].min(), val["γac1"].min(), val["γac2"].min()) >= 0.0


# ----------------------------------------------------------------------------- circle and ellipsoid
@pytest.mark.parametrize("cs", sc.quad_cases(), ids=sc.key)
def test_circle_and_ellipsoid_bounds(cs):
    """yc = f(centre), invP seeded SPD; root and small-a, beta 0 and 2.  w is the largest value of the form attained over the stored
    witnesses, the corners and 2 000 seeded samples: the truth is known from inside only, which is the side soundness needs; the upper
    side comes from the interior point's bracket"""
    q, s = solve(cs)
    assert held(cs, q, s)


# ----------------------------------------------------------------------------- safety
@pytest.mark.parametrize("cs", [sc.make(n, "relu", b, "hplane", "top", 0, "exact") for n in sc.NETS for b in ("root", "half-a")], ids=sc.key)
def test_safety_verdicts_follow_the_truth(cs):
    """hplaneS(c, h): at h = w - 1e-3 (1 + |w|) the property is false (the network attains w > h), so no certificate may be good; at
    h = upper + 1e-2 (1 + |upper|) the interior point's optimum is below h and the certificate must be found"""
    g, c = sc.stored(cs), sc.normal(cs)
    for h, want in ((g["w"] - 1e-3 * (1.0 + abs(g["w"])), False), (g["upper"] + 1e-2 * (1.0 + abs(g["upper"])), True)):
        q = sc.product_query(cs, S=qc.hplane_S(c, h, sc.oracle_net(cs)))
        s = na.runQuery(q, na.AdmmSdpOptions())
        print(f"{sc.key(cs)} h {h:.8f} (w {g['w']:.8f}, upper {g['upper']:.8f}): {s.termination_status} at {s.summary['iters']}, "
              f"lambda_max {s.summary['lambda_max']:+.3e}, good {vl.isSolutionGood(s)}")
        assert vl.isSolutionGood(s) == want, (sc.key(cs), h, s.termination_status, s.summary["lambda_max"])


# ----------------------------------------------------------------------------- Tanh
@pytest.mark.parametrize("cs", sc.tanh_cases(), ids=sc.key)
def test_tanh_bound_is_sound_and_in_the_bracket(cs):
    """both nets on root, small-a, stable, point, beta 0 and 2, the product's own intervals, against the attained value of
    tests/golden/tanh_ranges.json and the interior point's bracket.  Where the set-up refuses the activation QCs (3-10-10-3 root, small-a,
    stable: the reference's lexicographic `smin <= smax`, pinned in tests/test_sdp_truth_cpu.py) there is no query and no bound: that
    refusal is what is asserted"""
    if sc.tanh_refusal(cs) is not None:
        with pytest.raises(AssertionError):
            sc.product_query(cs)
        return
    q = sc.product_query(cs)
    assert held(cs, q, na.runQuery(q, na.AdmmSdpOptions()))


# ----------------------------------------------------------------------------- deciding a target
@pytest.mark.parametrize("net", sc.NETS)
def test_targets_are_decided_truthfully_with_the_coupling(net):
    """half-a, beta = 2, DoubleDecomp: the sparse Cholesky fronts of the certificate include the beta coupling.  A target below the
    optimum (lower - 1e-3 |lower|) is never certified; 1.05 upper is, with w - room <= objective <= target; certified_bound() of the
    iterates 200 and 2 000 is a feasible point of the LMI and therefore >= lower - 1e-9"""
    cs = sc.make(net, "relu", "half-a", "hplane", "top", 2, "exact")
    g, q = sc.stored(cs), sc.product_query(cs)
    opts = dict(decomp_mode=na.DoubleDecomp(), max_iters=20000)
    low = na.runQuery(q, na.AdmmSdpOptions(target=g["lower"] - 1e-3 * abs(g["lower"]), **opts))
    print(f"{sc.key(cs)} target below the optimum: {low.termination_status} at {low.summary['iters']}")
    assert low.termination_status != "TARGET_CERTIFIED"
    target = 1.05 * g["upper"]
    hi = na.runQuery(q, na.AdmmSdpOptions(target=target, **opts))
    assert hi.termination_status == "TARGET_CERTIFIED" and hi.objective_value <= target
    held(cs, q, hi, "target 1.05 upper", upper=False)
    sv = na.Solver(q, na.AdmmSdpOptions(**opts))
    try:
        done = 0
        for it in (200, 2000):
            sv.advance(it - done)
            done = it
            obj, gam, ok, ms = sv.certified_bound()
            print(f"{sc.key(cs)} certified_bound at {it}: {obj:.10f} certified {ok} ({ms:.2f} ms), lower {g['lower']:.10f}")
            assert ok and np.all(gam >= 0.0) and obj >= g["lower"] - 1e-9
            Z = na.makeZ(q, gam)
            z = sc.lifted(cs, np.array(g["x"]))
            assert obj >= g["w"] - max(0.0, float(np.linalg.eigvalsh(0.5 * (Z + Z.T))[-1])) * float(z @ z) - 1e-12 * (1.0 + abs(g["w"]))
    finally:
        sv.close()


# ----------------------------------------------------------------------------- a family
@pytest.mark.parametrize("net", sc.NETS)
def test_every_member_of_a_family_is_held_to_its_own_truth(net):
    """every qualifying direction of the root box (10 and 12) as one runQueries(..., share_setup=True): each member against its own w
    and its own bracket"""
    cases = sc.family_cases(net)
    assert len(cases) >= 10
    queries = [sc.product_query(cs) for cs in cases]
    for cs, q, s in zip(cases, queries, na.runQueries(queries, na.AdmmSdpOptions(), share_setup=True)):
        assert held(cs, q, s, "family")


# ----------------------------------------------------------------------------- assembly, generator by generator
@pytest.mark.parametrize("cs", [sc.make("3-10-10-3", "relu", "half-a", "hplane", "top", 3, "product"),
                                sc.make("2-8-8-2", "tanh", "small-a", "hplane", "top", 2, "product")], ids=sc.key)
def test_makeZ_generators_match_the_literal_ones(cs):
    """makeZ(q, e_i) - makeZ(q, 0) against G_i of the literal assembly of the same QCs, every multiplier, at 1e-12 max(1, |G_i|_max):
    with the generators pinned one by one, what tests/test_sdp_truth_cpu.py shows of the literal ones on the graph of the network holds
    for the product's"""
    q = sc.product_query(cs)
    qo = ost.mirror_query(q)
    Z0o, G = ipm.literal_generators(qo)
    Z0 = na.makeZ(q, np.zeros(qo.ngamma))
    assert np.abs(0.5 * (Z0 + Z0.T) - Z0o).max() <= 1e-12 * max(1.0, np.abs(Z0o).max())
    for i in range(qo.ngamma):
        e = np.zeros(qo.ngamma)
        e[i] = 1.0
        Gi = na.makeZ(q, e) - Z0
        assert np.abs(0.5 * (Gi + Gi.T) - G[i]).max() <= 1e-12 * max(1.0, np.abs(G[i]).max()), (sc.key(cs), i)
