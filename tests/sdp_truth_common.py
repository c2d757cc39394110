"""Shared by tests/test_sdp_truth_cpu.py, tests/test_sdp_truth_gpu.py and tests/golden/make_sdp_truth.py: the table of SDP queries whose
true optimum side is known (exact ReLU ranges of tests/golden/exact_ranges.json, attained Tanh values of tests/golden/tanh_ranges.json),
the two sources of the activation intervals, both statements of every query (product and oracle) and the reader of
tests/golden/sdp_truth.json, which holds the bracket of an independent interior point (oracle/ipm.py) per case.  Nothing here needs a GPU.

A case is a dict: net, activ ("relu" | "tanh"), box, out ("hplane" | "circle" | "ellipsoid"), dir ("top" | "lit" | "neg" | "row<k><+|->"),
beta, source ("exact" | "product").  Its direction comes from the stored rows and their negations: c = C[k] with w = wmax[k], or c = -C[k]
with w = -wmin[k] (Tanh: the stored rows only; that fixture records maxima).  "top" is the largest w of the box, "lit" the largest among
the literal rows 0..6 and their negations whose normal is not that of "top" (on 3-10-10-3 the largest of all is a literal row, and the
rows e_0, -e_0 are stored twice), "neg" the smallest.

Interval sources:
  "exact"    the fixture's pre / post ranges (LP value and attained value, whichever lies further out), widened outward by
             1e-9 (1 + |v|), acymin clipped at 0, through makeQcActivsIntvs on both sides.  ReLU only.
  "product"  na.makeQcActivs (the float32 host routine) on the product side, oracle.qc.make_qc_activs on the oracle side."""
import json
import os

import numpy as np

import exact_common as ec
import exact_range as er
import helpers
import nnsdp_amd as na
import tanh_truth as tt
import tanh_truth_common as ttc
from nnsdp_amd import frontend as F
from oracle import intervals as oiv, nnet_io, qc

FIXTURE = os.path.join(helpers.GOLDEN, "sdp_truth.json")
NETS = tuple(ec.SMALL)
W_MIN = 1e-2                       # a case that claims soundness has an exact maximum of at least this: rho >= 0 alone does not pass it
WIDEN = 1e-9                       # the LP values are the true ranges within 1e-9 (1 + |v|) (exact_range.V_W_BOUND)
EPS = 2.0 ** -52
GPU_BOXES = ("root", "half-a", "small-a", "edge0", "stable", "point")
PRODUCT_BOXES = ("root", "half-a", "edge0")
TIGHT = ("half-a", "half-b", "edge0")          # 2-8-8-2 with "exact" intervals: the relaxation is tight to the IPM's own gap
DEGENERATE = ("stable", "point")
TANH_BOXES = ("root", "small-a", "stable", "point")
QUAD_BOXES = ("root", "small-a")
BETAS = (0, 2)
NSAMPLES_QUAD = 2000
_cache = {}


# ----------------------------------------------------------------------------- nets, boxes, directions
def setting(net, activ):
    return ec.case(net) if activ == "relu" else ttc.fixture_case(net)


def box_of(net, activ, box):
    return next(bx for bx in setting(net, activ)["boxes"] if bx["name"] == box)


def candidates(net, activ, box):
    """every direction the fixture knows on the box: (row, sign, w, x), w attained at x"""
    bx = box_of(net, activ, box)
    if activ == "tanh":
        return [(k, 1, float(bx["w"][k]), bx["x"][k]) for k in range(len(bx["w"]))]
    lit = bx["lit"]
    return [(k, 1, float(lit["wmax"][k]), lit["xmax"][k]) for k in range(len(lit["wmax"]))] + \
           [(k, -1, -float(lit["wmin"][k]), lit["xmin"][k]) for k in range(len(lit["wmin"]))]


def direction(net, activ, box, name):
    """-> (row, sign, w, x) of "top", "lit", "neg" or "row<k>+" / "row<k>-" """
    cand = candidates(net, activ, box)
    if name.startswith("row"):
        k, s = int(name[3:-1]), 1 if name[-1] == "+" else -1
        return next(c for c in cand if (c[0], c[1]) == (k, s))
    top = max(cand, key=lambda c: c[2])
    if name == "top":
        return top
    if name == "lit":
        C = setting(net, activ)["C"]
        return max((c for c in cand if c[0] < 7 and not np.array_equal(c[1] * C[c[0]], top[1] * C[top[0]])), key=lambda c: c[2])
    if name == "neg":
        return min(cand, key=lambda c: c[2])
    raise KeyError(name)


def qualifying(net, box="root"):
    """the names of every direction of a ReLU box with w >= W_MIN"""
    return [f"row{k}{'+' if s > 0 else '-'}" for k, s, w, _ in candidates(net, "relu", box) if w >= W_MIN]


def normal(cs):
    k, s, _, _ = direction(cs["net"], cs["activ"], cs["box"], cs["dir"])
    return s * setting(cs["net"], cs["activ"])["C"][k]


def key(cs):
    return "|".join(str(cs[k]) for k in ("net", "activ", "box", "out", "dir", "beta", "source"))


def make(net, activ, box, out, dirn, beta, source):
    return dict(net=net, activ=activ, box=box, out=out, dir=dirn, beta=int(beta), source=source)


# ----------------------------------------------------------------------------- the table
def relu_hplane_cases(source):
    boxes = GPU_BOXES if source == "exact" else PRODUCT_BOXES
    return [make(n, "relu", b, "hplane", d, beta, source) for n in NETS for b in boxes for d in ("top", "lit") for beta in BETAS]


def tight_cases(source):
    """2-8-8-2, beta = 0, the boxes on which the relaxation with "exact" intervals is tight"""
    return [make("2-8-8-2", "relu", b, "hplane", "top", 0, source) for b in TIGHT]


def negative_cases():
    return [make(n, "relu", "half-a", "hplane", "neg", 0, "exact") for n in NETS]


def quad_cases():
    return [make(n, "relu", b, out, "top", beta, "exact") for n in NETS for b in QUAD_BOXES for out in ("circle", "ellipsoid") for beta in BETAS]


def tanh_cases():
    return [make(n, "tanh", b, "hplane", "top", beta, "product") for n in NETS for b in TANH_BOXES for beta in BETAS]


def family_cases(net):
    return [make(net, "relu", "root", "hplane", d, 0, "exact") for d in qualifying(net)]


def all_cases():
    """every case the fixture holds, each once"""
    out, seen = [], set()
    for cs in (relu_hplane_cases("exact") + relu_hplane_cases("product") + tight_cases("exact") + tight_cases("product") + negative_cases()
               + quad_cases() + tanh_cases() + [c for n in NETS for c in family_cases(n)]):
        if key(cs) not in seen:
            seen.add(key(cs))
            out.append(cs)
    return out


def claims_soundness(cs):
    return cs["dir"] != "neg"


# ----------------------------------------------------------------------------- lifting and attained values
def lifted(cs, x):
    """(x, hidden activations, 1) from the long-double forward pass of the case's own activation"""
    Ms = setting(cs["net"], cs["activ"])["net"].Ms
    if cs["activ"] == "relu":
        return er.lifted(Ms, x)
    _, hid = tt.forward_ld(Ms, x, hidden=True)
    return np.concatenate([np.asarray(x, dtype=np.float64)] + [np.asarray(h, dtype=np.float64) for h in hid] + [np.ones(1)])


def output_ld(cs, x):
    Ms = setting(cs["net"], cs["activ"])["net"].Ms
    return (er.forward_ld if cs["activ"] == "relu" else tt.forward_ld)(Ms, x)


def quad_data(cs):
    """circle / ellipsoid: yc = f(centre of the box) and a seeded SPD invP (the seed depends on the net and the box only)"""
    bx = box_of(cs["net"], cs["activ"], cs["box"])
    yc = np.asarray(output_ld(cs, 0.5 * (bx["lo"] + bx["hi"])), dtype=np.float64)
    m = len(yc)
    rng = np.random.default_rng(7000 + 10 * NETS.index(cs["net"]) + GPU_BOXES.index(cs["box"]))
    B = rng.standard_normal((m, m))
    invP = np.linalg.inv(B @ B.T + np.eye(m))
    return yc, 0.5 * (invP + invP.T)


def form_value(cs, x):
    """what gamma_out bounds at the point x, from the long-double forward pass: c' f(x), |f(x) - yc|^2, or |invP f(x) - yc|^2 (the
    reference's ellipsoid form as oracle/qc.py make_S keeps it, S33 = yc' yc - gamma_out)"""
    ld = np.longdouble
    y = output_ld(cs, x)
    if cs["out"] == "hplane":
        return float(normal(cs).astype(ld) @ y)
    yc, invP = quad_data(cs)
    r = (y if cs["out"] == "circle" else invP.astype(ld) @ y) - yc.astype(ld)
    return float(r @ r)


def stored_points(cs):
    """every stored witness of the box (lit, pre, post, both ends; Tanh: the rows' argmaxima) and its corners"""
    bx = box_of(cs["net"], cs["activ"], cs["box"])
    n0 = len(bx["lo"])
    corners = np.array([[bx["hi"][q] if (m >> q) & 1 else bx["lo"][q] for q in range(n0)] for m in range(2 ** n0)])
    if cs["activ"] == "tanh":
        return np.vstack([bx["x"], corners])
    return np.vstack([bx[blk][k] for blk in ("lit", "pre", "post") for k in ("xmax", "xmin")] + [corners])


def samples(cs, n, seed):
    bx = box_of(cs["net"], cs["activ"], cs["box"])
    return bx["lo"] + np.random.default_rng(seed).random((n, len(bx["lo"]))) * (bx["hi"] - bx["lo"])


def truth(cs):
    """-> (w, x): the value the bound must respect and the point that attains it.  hplane: the fixture's exact maximum (ReLU) or
    attained value (Tanh).  circle / ellipsoid: the largest value of the form over the stored witnesses, the corners and 2 000 seeded
    samples - the truth is known from inside only, which is the side soundness needs"""
    if cs["out"] == "hplane":
        _, _, w, x = direction(cs["net"], cs["activ"], cs["box"], cs["dir"])
        return w, np.asarray(x, dtype=np.float64)
    k = key(dict(cs, beta=0))
    if k not in _cache:
        pts = np.vstack([stored_points(cs), samples(cs, NSAMPLES_QUAD, 11)])
        vals = np.array([form_value(cs, x) for x in pts])
        _cache[k] = (float(vals.max()), pts[int(np.argmax(vals))])
    return _cache[k]


# ----------------------------------------------------------------------------- intervals and queries
def exact_intervals(net, box):
    """(x_intvs, acx_intvs) of makeQcActivsIntvs from the fixture's neuron rows: per end the LP value or the attained value, whichever
    lies further out, moved outward by WIDEN (1 + |v|); the post-activation lower ends clipped at 0"""
    cs, bx = ec.case(net), box_of(net, "relu", box)
    out = {}
    for blk in ("pre", "post"):
        lo, hi = np.minimum(bx[blk]["vmin"], bx[blk]["wmin"]), np.maximum(bx[blk]["vmax"], bx[blk]["wmax"])
        out[blk] = (lo - WIDEN * (1.0 + np.abs(lo)), hi + WIDEN * (1.0 + np.abs(hi)))
    out["post"] = (np.maximum(out["post"][0], 0.0), out["post"][1])
    x_intvs, acx, o = [(bx["lo"], bx["hi"])], [], 0
    for n in cs["net"].xdims[1:-1]:
        x_intvs.append((out["post"][0][o:o + n], out["post"][1][o:o + n]))
        acx.append((out["pre"][0][o:o + n], out["pre"][1][o:o + n]))
        o += n
    ny = cs["net"].xdims[-1]
    x_intvs.append((bx["lit"]["vmin"][7:7 + ny], bx["lit"]["vmax"][7:7 + ny]))        # the output interval: no QC reads it
    return x_intvs, acx


def oracle_net(cs):
    net = setting(cs["net"], cs["activ"])["net"]
    return nnet_io.FeedFwdNet(xdims=list(net.xdims), Ms=[np.array(M, dtype=np.float64) for M in net.Ms])


def product_activs(cs):
    """the product's activation QCs of the case (host code only)"""
    net, bx = setting(cs["net"], cs["activ"])["net"], box_of(cs["net"], cs["activ"], cs["box"])
    if cs["source"] == "exact":
        assert cs["activ"] == "relu"
        return F.makeQcActivsIntvs(net, *exact_intervals(cs["net"], cs["box"]), cs["beta"])
    return na.makeQcActivs(net, bx["lo"], bx["hi"], cs["beta"])


def oracle_activs(cs):
    bx = box_of(cs["net"], cs["activ"], cs["box"])
    if cs["source"] == "exact":
        assert cs["activ"] == "relu"
        return qc.make_qc_activs(oracle_net(cs), bx["lo"], bx["hi"], cs["beta"], intv=oiv.IntervalsInfo(*exact_intervals(cs["net"], cs["box"])))
    return qc.make_qc_activs(oracle_net(cs), bx["lo"], bx["hi"], cs["beta"], activ=cs["activ"])


def product_query(cs, S=None):
    """the product's query of the case; with S a safety query of the same box and activation QCs"""
    net, bx = setting(cs["net"], cs["activ"])["net"], box_of(cs["net"], cs["activ"], cs["box"])
    qin, qa = na.QcInputBox(x1min=bx["lo"], x1max=bx["hi"]), product_activs(cs)
    if S is not None:
        return na.SafetyQuery(ffnet=net, qc_input=qin, qc_safety=na.QcSafety(S=np.asarray(S, dtype=np.float64)), qc_activs=qa)
    if cs["out"] == "hplane":
        out = na.QcReachHplane(normal=normal(cs))
    else:
        yc, invP = quad_data(cs)
        out = na.QcReachCircle(yc=yc) if cs["out"] == "circle" else na.QcReachEllipsoid(invP=invP, yc=yc)
    return na.ReachQuery(ffnet=net, qc_input=qin, qc_reach=out, qc_activs=qa)


def oracle_query(cs, S=None):
    bx = box_of(cs["net"], cs["activ"], cs["box"])
    qb, qs = oracle_activs(cs)
    if S is not None:
        out = qc.QcSafety(S=np.asarray(S, dtype=np.float64))
    elif cs["out"] == "hplane":
        out = qc.QcReachHplane(normal=normal(cs))
    else:
        yc, invP = quad_data(cs)
        out = qc.QcReachCircle(yc=yc) if cs["out"] == "circle" else qc.QcReachEllipsoid(invP=invP, yc=yc)
    return qc.Query(net=oracle_net(cs), qc_input=qc.QcInputBox(bx["lo"], bx["hi"]), qc_out=out, qc_bounded=qb, qc_sector=qs)


# ----------------------------------------------------------------------------- the fixture
# The interior point is run with four settings of its step fraction and tolerances.  One run's residuals do not bracket the optimum of
# these LMIs: a neuron that is dead or fixed on the box has an "exact" interval 1e-9 wide, its multiplier runs to 1e5 .. 1e8, and the
# objective error of a run is its primal residual times such multipliers.  On 3-10-10-3 small-a (top, beta 0, "exact") the default run ends
# OPTIMAL at 0.7212503340 with gap 4.9e-10, and the run with step_frac = 0.8 ends OPTIMAL at the feasible point 0.7212498996, 4.3e-7
# below the first run's lower end.  A feasible point (gamma >= 0, lambda_max(Z) <= 0: _feasible) is an upper bound whatever the run's state, so
# `upper` is the smallest feasible objective of the four; `lower` is the smallest lower end of the converged runs.
IPM_RUNS = (dict(), dict(step_frac=0.9, max_iters=400), dict(step_frac=0.995, max_iters=400, tol_gap=1e-11, tol_feas=1e-11),
            dict(step_frac=0.8, max_iters=600, tol_gap=1e-10, tol_feas=1e-10))


def bracket(r):
    """one run's bracket of the optimum from its IpmResult -> (lower, upper)"""
    return min(r.objective, r.dual_objective) - (r.gap + r.pinf + r.dinf) * (1.0 + abs(r.objective)), r.objective


def _feasible(Z0, G, r, strict):
    """gamma >= 0 and lambda_max(Z) <= 0 (strict), or <= 1e-9 |Z|_2, the rule of tests/test_target_stop_gpu.py.  The multipliers of the
    narrow intervals put |Z|_2 at 1e5 .. 1e8, so the second rule admits a lambda_max of 1e-4 .. 1e-1 and a point that may lie below the
    optimum by about lambda_max |z|^2: it is the fallback for a case none of whose runs passes the first"""
    ev = np.linalg.eigvalsh(Z0 + np.tensordot(r.gamma, G, axes=1))
    return bool(np.all(r.gamma >= 0.0) and ev[-1] <= (0.0 if strict else 1e-9 * max(abs(ev[0]), abs(ev[-1]))))


def ipm_bracket(cs, w):
    """-> (best run, lower, upper, the four runs).  On the degenerate boxes (no interior, no Slater point: every run may stall) `lower`
    is capped by the attained value w: the QCs hold on the graph of the network, so the optimum is >= w, and that is the one lower
    bound that is a proof there"""
    from oracle import ipm
    q = fixture_query(cs)
    Z0, G = ipm.literal_generators(q)
    runs = [ipm.solve_lmi(Z0, G, q.cost(), ipm.IpmOptions(**kw)) for kw in IPM_RUNS]
    ok = [r for r in runs if _feasible(Z0, G, r, True)] or [r for r in runs if _feasible(Z0, G, r, False)]
    best = min(ok, key=lambda r: r.objective)
    lower = min(bracket(r)[0] for r in runs if r is best or r.status in ("OPTIMAL", "NEAR_OPTIMAL"))
    if cs["box"] in DEGENERATE:
        lower = min(lower, w)
    return best, lower, best.objective, runs


def fixture_query(cs):
    """the oracle's statement of the problem the fixture solves.  "exact": oracle_query.  "product": the QCs of the product's own float32
    host routine, mirrored - the two float32 routines differ in the last bits of an interval end, which moves the optimum by up to 1e-6
    on a tight box, and the bracket is held to 1e-9; where the product refuses the Tanh QCs (no query exists) the oracle's routine"""
    import oracle_state as ost
    if cs["source"] == "exact":
        return oracle_query(cs)
    try:
        return ost.mirror_query(product_query(cs))
    except AssertionError:
        assert cs["activ"] == "tanh"
        return oracle_query(cs)


def tanh_refusal(cs):
    """None where the product builds the Tanh case's activation QCs, else the reason it refuses them: "nan" (a pre-activation end that
    is exactly 0.0 makes the slope 0 / 0) or "order" (the reference's `@assert smin <= smax` compares the vectors lexicographically, and
    its Tanh branch returns smin > smax on a negative interval: refused where the first differing neuron has one).  Read from the
    product's intervals, not from an exception"""
    bx, net = box_of(cs["net"], "tanh", cs["box"]), setting(cs["net"], "tanh")["net"]
    _, acx = F.makeIntervalsInfo(bx["lo"], bx["hi"], net)
    lo, hi = np.concatenate([a for a, _ in acx]), np.concatenate([b for _, b in acx])
    if np.any(lo == 0.0) or np.any(hi == 0.0):
        return "nan"
    t = lambda v: np.tanh(v) / v
    smin, smax = np.where(lo * hi >= 0, t(hi), np.minimum(t(lo), t(hi))), np.where(lo * hi >= 0, t(lo), 1.0)
    return None if smin.tolist() <= smax.tolist() else "order"


def slope_range(lo, hi):
    """the range of tanh(x) / x over [lo, hi] in mpmath, rounded to doubles -> (inf, sup): tanh(x) / x is even and decreases in |x|, so
    the infimum is at the end farther from 0 and the supremum at the nearer one, or 1 (at x = 0) on an interval that crosses 0.  Written
    from the function, not from makeSectorMinMax"""
    import mpmath
    with mpmath.workdps(40):
        t = lambda v: float(mpmath.tanh(mpmath.mpf(float(v))) / mpmath.mpf(float(v)))
        far, near = (lo, hi) if abs(lo) >= abs(hi) else (hi, lo)
        return t(far), (1.0 if lo < 0.0 < hi else t(near))


def fixture():
    """the JSON as written; a missing file or case is an error, never a skip"""
    if "fixture" not in _cache:
        with open(FIXTURE) as fh:
            _cache["fixture"] = json.load(fh)
    return _cache["fixture"]


def stored(cs):
    return fixture()["cases"][key(cs)]
