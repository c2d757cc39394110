"""The kernels' claims against exact ReLU ranges (tests/exact_range.py, recorded in tests/golden/exact_ranges.json): every bound of
makeIntervalsBatch(backend="gpu") and of the resident CrownBounder, plain and with optimised slopes, respects values the network attains at
the exact extrema; the linear upper bound holds on the whole box; the split driver's verdicts on every GPU backend are the true ones for
thresholds placed just above and just below the exact maximum; the certified SDP bound respects the exact maximum up to what its
lambda_max allows; and the Tanh kernel respects the maxima of a fine grid.  The tolerances are those the arithmetic tests already derive
(max(8 r, 64 * 2^-52 * s) with r = |R(float64) - R(long double)| on the same boxes); the margins printed are measured, none is assumed.
tests/test_exact_range_cpu.py holds the host routine and the host driver against the same fixture."""
import numpy as np
import pytest

import crown_alpha_common as ca
import crown_tanh_common as tc
import exact_common as ec
import exact_range as er
import literal_common as lc
import nnsdp_amd as na

_cache = {}
ENTRIES = ("gpu", "gpu, no literals", "resident", "resident alpha 3", "resident alpha 8", "resident alpha0 a", "resident alpha0 b")


def setting(name):
    """the case, its boxes as arrays, and the fp64 tolerances of the ten arrays on these boxes: computed once, shared, never modified"""
    if name not in _cache:
        cs = ec.case(name)
        lo, hi = ec.box_arrays(cs)
        _cache[name] = dict(cs=cs, lo=lo, hi=hi, tol=ec.fp64_tols(cs, lo, hi))
    return _cache[name]


def alpha_tols(st, lits):
    """the tolerances of smax, A, b0 of an alpha result: the plain ones, or where larger 8 r (1 + |value|) with r = max |R_at(float64) -
    R_at(long double)| / (1 + |v|) at the returned slopes (the 8 r of tests/test_crown_alpha_gpu.py)"""
    Ms, C = st["cs"]["net"].Ms, st["cs"]["C"]
    r64, rld = ca.R_at(Ms, st["lo"], st["hi"], np.float64, C, lits.alpha), ca.R_at(Ms, st["lo"], st["hi"], np.longdouble, C, lits.alpha)
    r = max(ca.rel_err(a, b) for a, b in zip(r64, rld))
    tol = dict(st["tol"])
    for nm, got in (("smax", lits.smax), ("A", lits.A), ("b0", lits.b0)):
        tol[nm] = np.maximum(tol[nm], 8.0 * r * (1.0 + np.abs(got)))
    return tol


def run_entry(st, entry):
    """-> (result of the entry, its tolerances)"""
    cs, lo, hi = st["cs"], st["lo"], st["hi"]
    if entry == "gpu":
        return na.makeIntervalsBatch(cs["net"], lo, hi, backend="gpu", normals=cs["C"]), st["tol"]
    if entry == "gpu, no literals":
        return na.makeIntervalsBatch(cs["net"], lo, hi, backend="gpu"), st["tol"]
    with na.CrownBounder(cs["net"], cs["C"]) as bd:
        if entry == "resident":
            return bd.bound(lo, hi), st["tol"]
        if entry.startswith("resident alpha0"):
            shape = (len(cs["C"]), sum(cs["net"].xdims[1:-1]), lo.shape[1])
            res = bd.bound(lo, hi, alpha_steps=0, alpha0=ca.f32_uniform(shape, 900 + ord(entry[-1])))
        else:
            res = bd.bound(lo, hi, alpha_steps=int(entry.split()[-1]))
    return res, alpha_tols(st, res[6])


# ----------------------------------------------------------------------------- b. soundness at the witnesses
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_bounds_respect_the_exact_extrema(name, entry):
    """every fixture box of the case in one call (8 boxes): lower <= w_min + tol and upper >= w_max - tol for the six arrays and, where
    the entry returns them, the literal bounds; |bound - v| <= tol on the point box and (CROWN arrays) on the all-stable box.  "alpha0":
    alpha_steps = 0 at seeded uniform slopes in [0, 1]: any slope is sound, so the bound of every one of them must hold.  Prints the
    worst (w - bound) / tol of every array and of the entry with the box it occurred on (1 is the limit; negative: the bound has room)"""
    st = setting(name)
    res, tol = run_entry(st, entry)
    if entry.startswith("resident alpha"):
        assert np.all(res[6].smax <= res[6].smax_plain)
    worst, nm, box = ec.check_sound(f"{name} {entry}", st["cs"], ec.entry_arrays(res), tol)
    print(f"{name} {entry}: worst (w - bound) / tol of the entry = {worst:+.3e} ({nm}, box {box})")


# ----------------------------------------------------------------------------- c. the linear form on the whole box
@pytest.mark.gpu
def test_the_linear_form_is_sound_on_the_whole_box():
    """2-8-8-2, the root and one box of half-width 0.5, the resident bounder plain and with alpha_steps = 8: the oracle's maximum over
    the box of C_i f(x) - A_i' x, minus b0_i, is <= tol_A * sum_q max |x_q| + tol_b0 (the arithmetic tolerances of A and b0: the form is
    an upper bound in exact arithmetic, and A, b0 carry their rounding).  2 boxes x 2 entries x 11 literals = 44 maxima on two
    enumerations (43 and 11 regions), about 3 s of LPs"""
    st = setting("2-8-8-2")
    cs = st["cs"]
    with na.CrownBounder(cs["net"], cs["C"]) as bd:
        results = {T: bd.bound(st["lo"], st["hi"], **(dict(alpha_steps=T) if T else {}))[6] for T in (0, 8)}
    for j in (0, 1):
        bx = cs["boxes"][j]
        s = er.regions(cs["net"].Ms, bx["lo"], bx["hi"])
        for T, lits in results.items():
            tol = alpha_tols(st, lits) if T else st["tol"]
            tA, tb = np.broadcast_to(tol["A"], lits.A.shape)[:, :, j].max(axis=1), np.broadcast_to(tol["b0"], lits.b0.shape)[:, j]
            bound = tA * np.maximum(np.abs(bx["lo"]), np.abs(bx["hi"])).sum() + tb
            r = er.exact_max(cs["net"].Ms, bx["lo"], bx["hi"], cs["C"], a=lits.A[:, :, j], search=s)
            excess = r.v - lits.b0[:, j]
            i = int(np.argmax(excess / bound))
            print(f"{bx['name']} alpha {T}: worst (max(C f - A x) - b0) / tol = {excess[i] / bound[i]:+.3e} (literal {i}, excess {excess[i]:+.3e}, tol {bound[i]:.3e})")
            assert np.all(excess <= bound), (bx["name"], T, i, float(excess[i]), float(bound[i]))


# ----------------------------------------------------------------------------- d. verdicts are true
LB, CP = dict(literal_bounds=True), dict(corner_points=True)
CONFIGS = {
    "gpu": (dict(crown_backend="gpu"), {}),
    "gpu literal_bounds": (dict(crown_backend="gpu", **LB), LB),
    "gpu corner_points": (dict(crown_backend="gpu", **CP), CP),
    "resident": (dict(crown_backend="resident"), {}),
    "resident literal_bounds": (dict(crown_backend="resident", **LB), LB),
    "resident corner_points": (dict(crown_backend="resident", **CP), CP),
    "device": (dict(crown_backend="resident", frontier="device"), {}),
    "device literal_bounds": (dict(crown_backend="resident", frontier="device", **LB), LB),
    "device corner_points": (dict(crown_backend="resident", frontier="device", **CP), CP),
    "resident alpha 4": (dict(crown_backend="resident", alpha_steps=4, **LB), dict(alpha_steps=4, **LB)),
    "resident alpha 4 corner_points": (dict(crown_backend="resident", alpha_steps=4, **LB, **CP), dict(alpha_steps=4, **LB, **CP)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_verdicts_are_true(name, config):
    """the literal y_0 - y_last on the root box, h = v + rel (c0 - v) for rel in {+1e-2, +1e-4, -1e-4, -1e-2}, v the exact maximum:
    rel > 0 never gives "violated", rel < 0 never "holds"; a witness is inside the box and violates by a numpy forward pass; a "holds" tree
    tiles the box with every leaf bound <= h; and the verdict is the true one within max_boxes = min(4 096, 4 x the visited count of the
    host backend with the same options, computed here): the factor covers the different trees of float32 and fp64 bounds"""
    st = ec.verdict_setting(name)
    gpu_opts, host_opts = CONFIGS[config]
    for rel in ec.RELS:
        _, host = ec.run_split(st, rel, crown_backend="host", **host_opts)
        assert host.verdict == ("holds" if rel > 0 else "violated")
        budget = min(ec.MAX_BOXES_CAP, 4 * host.visited)
        h, res = ec.run_split(st, rel, max_boxes=budget, **gpu_opts)
        print(f"{name} {config} rel {rel:+.0e}: host visited {host.visited}, budget {budget}")
        ec.check_verdict(f"{name} {config}", st, rel, h, res)


# ----------------------------------------------------------------------------- e. the certified SDP bound
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_the_certified_sdp_bound_respects_the_exact_maximum(name):
    """reach-hyperplane query of +-(y_0 - y_last) on the root box, beta = 0, default options (certificate polish on).  With the returned
    multipliers Z = makeZ(q, gamma) and z = (x*, hidden activations, 1) at the exact argmax, the S-procedure gives
    c' f(x*) - rho <= lambda_max(Z) |z|^2 for multipliers >= 0 (tests/test_exact_range_cpu.py checks the identity with the oracle's
    assembly, where the sharper factor 1 / 2 holds as well), so  rho >= w - max(0, lambda_max(Z)) |z|^2 - 1e-12 (1 + |w|).
    Every multiplier is >= 0, gamma_out (which is rho itself) among them: the model has gamma >= 0 throughout, so a direction whose
    exact maximum is negative has the optimum exactly 0 and the statement above would hold of any solver.  The sign of the row is
    therefore the one with w >= 1e-2 (3-10-10-3: max (y_0 - y_last) = -0.114, so the row is negated and w = 0.769); tests/test_sdp_truth_gpu.py
    holds the bound to many more boxes, QCs and decompositions"""
    cs = ec.case(name)
    root, net = cs["boxes"][0], cs["net"]
    sign = 1.0 if root["lit"]["wmax"][0] >= 1e-2 else -1.0
    nrm = sign * cs["C"][0]
    w, xstar = (float(root["lit"]["wmax"][0]), root["lit"]["xmax"][0]) if sign > 0 else (-float(root["lit"]["wmin"][0]), root["lit"]["xmin"][0])
    assert w >= 1e-2
    q = na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=root["lo"], x1max=root["hi"]), qc_reach=na.QcReachHplane(normal=nrm),
                      qc_activs=na.makeQcActivs(net, root["lo"], root["hi"], 0))
    s = na.runQuery(q, na.AdmmSdpOptions())
    val = s.values
    gamma = np.concatenate([val["γin"], val["γout"], val["γac1"], val["γac2"]])
    Z = na.makeZ(q, gamma)
    lam = float(np.linalg.eigvalsh(0.5 * (Z + Z.T))[-1])
    z = er.lifted(net.Ms, xstar)
    rho = float(s.objective_value)
    room = max(0.0, lam) * float(z @ z)
    print(f"{name}: rho {rho:.10f}, exact max {w:.10f} (gap {rho - w:+.3e}), status {s.termination_status}, lambda_max(Z) {lam:+.3e}, |z|^2 {z @ z:.4f}, "
          f"allowed shortfall {room:.3e}, smallest multiplier {min(val['γin'].min(), val['γac1'].min(), val['γac2'].min()):+.3e}")
    assert rho == float(val["γout"][0])
    assert val["γin"].min() >= 0.0 and val["γout"].min() >= 0.0 and val["γac1"].min() >= 0.0 and val["γac2"].min() >= 0.0
    assert rho >= w - room - 1e-12 * (1.0 + abs(w))


# ----------------------------------------------------------------------------- f. Tanh
@pytest.mark.gpu
def test_the_tanh_kernel_respects_grid_extrema():
    """the 2-8-8-2 net as a Tanh net on the fixture's boxes: ymin / ymax and the literal bounds of the resident kernel against the extrema
    over a 1001 x 1001 grid per box (values the network attains), within max(8 r, 64 * 2^-52 * s) with the r of
    tests/test_crown_resident_gpu.py (|R_tanh(float64) - R_tanh(long double)| plus the same with tanh / cosh moved by one ulp), taken per
    box and not over the call: on the box whose first-layer upper bound is exactly 0 the float64 and the long-double restatement fall
    into different regimes of the relaxation and r is 1e-4 to 6e-4 there (both bounds are sound; the yardstick is discontinuous at
    u = 0), which must not loosen the other seven boxes, where the tolerance is of order 1e-15"""
    st = setting("2-8-8-2")
    cs, lo, hi = st["cs"], st["lo"], st["hi"]
    net = tc.tanh_copy(cs["net"])
    r64, rld = tc.R_tanh(net.Ms, lo, hi, np.float64, cs["C"]), tc.R_tanh(net.Ms, lo, hi, np.longdouble, cs["C"])
    rmv = tc.R_tanh(net.Ms, lo, hi, np.float64, cs["C"], lib=tc.Moved(1.0, seed=7))
    with na.CrownBounder(net, cs["C"]) as bd:
        got = tc.flat(bd.bound(lo, hi))
    names = lc.NAMES + lc.LIT_NAMES
    gmin, gmax = [], []
    for b in range(lo.shape[1]):
        g0, g1 = np.meshgrid(np.linspace(lo[0, b], hi[0, b], 1001), np.linspace(lo[1, b], hi[1, b], 1001))
        Y = lc.forward(net, np.stack([g0.ravel(), g1.ravel()]))
        rows = np.vstack([Y, cs["C"] @ Y])
        gmin.append(rows.min(axis=1))
        gmax.append(rows.max(axis=1))
    gmin, gmax, ny = np.stack(gmin, axis=1), np.stack(gmax, axis=1), net.xdims[-1]
    for nm, wit in (("ymin", gmin[:ny]), ("ymax", gmax[:ny]), ("smin", gmin[ny:]), ("smax", gmax[ny:])):
        i = names.index(nm)
        r = np.abs(r64[i] - rld[i]).max(axis=0) + np.abs(rmv[i] - rld[i]).max(axis=0)
        tol = np.maximum(8.0 * r, 64.0 * ec.EPS * np.abs(rld[i]).max(axis=0)).astype(np.float64)[None, :]
        excess = (got[i] - wit) if nm.endswith("min") else (wit - got[i])
        k, b = np.unravel_index(np.argmax(excess / tol), excess.shape)
        print(f"tanh {nm}: worst (w - bound) / tol = {excess[k, b] / tol[0, b]:+.3e} (row {k}, box {cs['boxes'][b]['name']}, excess {excess[k, b]:+.3e}, "
              f"tol {tol[0, b]:.3e}); tol per box {np.array2string(tol[0], precision=1)}")
        assert np.all(np.isfinite(got[i])) and np.all(excess <= tol), (nm, cs["boxes"][b]["name"], float(excess[k, b]), float(tol[0, b]))
