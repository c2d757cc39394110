"""The SDP side against exact ranges, without a GPU (the table and both interval sources: tests/sdp_truth_common.py).

a. Every multiplier's generator G_i = Z(e_i) - Z(0), i != out, of the oracle's literal assembly is a quadratic constraint of its own:
   z' G_i z >= 0 at every z = (x, hidden activations, 1) of the true network.  A QC misread in oracle/qc.py fails here whatever the
   kernels do, because the points come from the network and not from the assembly.
b. The out generator is the form the docstrings claim (hyperplane, circle, ellipsoid, hyperplane safety set).
c. The oracle's interior point against the truth: sound everywhere, tight where the relaxation is tight, exactly 0 where the true
   maximum is negative; the stored fixture against a live solve.
d. The Tanh queries the set-up refuses are refused, with the exception pinned.

Tolerances are derived, none is measured:
  rounding        64 * 2^-52 * |z|' |G_i| |z|  (test_crown_batch_gpu.py: 64 roundings) for every generator;
  "exact"         nothing else: the intervals contain the true ranges by construction (LP value and attained value, widened by 1e-9);
  "product"       the float32 intervals are sound to HOST_SLACK (1 + |v|) per end (tests/test_literal_bounds_cpu.py); a bounded generator is
                  2 (y - lo)(hi - y), so moving lo, hi outward by d_lo, d_hi changes it by 2 ((y - lo) d_hi + (hi - y) d_lo + d_lo d_hi); a
                  Tanh-sector generator is -2 smin smax x^2 + 2 (smin + smax) x y, and moving the pre-activation ends outward changes it
                  by 2 x^2 (smin' smax' - smin smax) - 2 x y (smin' + smax' - smin - smax) with smin', smax' from the moved ends.  The
                  generator of the moved intervals is >= 0 on the graph, so the product's is >= minus that change.  The input, ReLU-sector
                  (slopes 0 / 1 decided at 1e-4, far above the slack) and beta-coupling generators read no float32 quantity."""
import numpy as np
import pytest

import exact_common as ec
import nnsdp_amd as na
import sdp_truth_common as sc
from oracle import intervals as oiv, ipm, qc

MARGIN = 64.0 * sc.EPS


def generator_kinds(q):
    """kind of every multiplier, its neuron (bounded, sector, eta, nu) or -1"""
    nin, nout, n1, n2 = q.gamma_dims()
    n, npairs = q.qc_sector.acxdim, len(q.qc_sector.pairs()) if q.beta > 0 else 0
    kinds = [("in", -1)] * nin + [("out", -1)] * nout + [("bounded", j) for j in range(n1)] + [("sector", j) for j in range(n)] + [("coupling", -1)] * npairs
    if q.qc_sector.activ == "relu":
        kinds += [("eta", j) for j in range(n)] + [("nu", j) for j in range(n)]
    assert len(kinds) == q.ngamma
    return kinds


def points_of(cs):
    """every stored witness, the corners and 50 seeded samples of the case's box, lifted -> npts x Zdim"""
    pts = np.vstack([sc.stored_points(cs), sc.samples(cs, 50, 5)])
    return np.array([sc.lifted(cs, x) for x in pts])


def moved(intv):
    """the oracle's float32 intervals with every end moved outward by HOST_SLACK (1 + |v|)"""
    out = lambda lo, hi: (lo - ec.HOST_SLACK * (1.0 + np.abs(lo)), hi + ec.HOST_SLACK * (1.0 + np.abs(hi)))
    return oiv.IntervalsInfo([out(*iv) for iv in intv.x_intvs], [out(*iv) for iv in intv.acx_intvs])


def slack_of(cs, q, Rz):
    """the float32 allowance of the bounded and Tanh-sector generators at the lifted points (docstring); None with "exact" intervals.
    Rz: npts x (2 n + 1), the rows of make_R applied to the points: pre-activations, post-activations, 1"""
    if cs["source"] == "exact":
        return None
    bx, n = sc.box_of(cs["net"], cs["activ"], cs["box"]), q.qc_sector.acxdim
    intv = oiv.intervals_crown_sliced(q.net, bx["lo"], bx["hi"], activ=cs["activ"])
    with np.errstate(invalid="ignore", divide="ignore"):
        qb0, qs0 = qc.make_qc_activs(q.net, bx["lo"], bx["hi"], cs["beta"], intv=intv, activ=cs["activ"])
    assert np.array_equal(qb0.acymin, q.qc_bounded.acymin) and np.array_equal(qs0.smin, q.qc_sector.smin, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        qb1, qs1 = qc.make_qc_activs(q.net, bx["lo"], bx["hi"], cs["beta"], intv=moved(intv), activ=cs["activ"])
    x, y = Rz[:, :n], Rz[:, n:2 * n]
    dlo, dhi = qb0.acymin - qb1.acymin, qb1.acymax - qb0.acymax
    assert np.all(dlo >= 0) and np.all(dhi >= 0)
    out = dict(bounded=2.0 * (np.abs(y - qb0.acymin) * dhi + np.abs(qb0.acymax - y) * dlo + dlo * dhi))
    if cs["activ"] == "tanh":
        out["sector"] = 2.0 * np.abs(x * x * (qs1.smin * qs1.smax - qs0.smin * qs0.smax)) + \
                        2.0 * np.abs(x * y * (qs1.smin + qs1.smax - qs0.smin - qs0.smax))
    return out


GRAPH = [sc.make(n, "relu", b, "hplane", "top", beta, src) for n in sc.NETS for b in ec.BOX_NAMES for beta in (0, 1, 3) for src in ("exact", "product")] + \
        [sc.make(n, "tanh", b, "hplane", "top", beta, "product") for n in sc.NETS for b in ("root", "edge0", "stable", "point", "small-a") for beta in (0, 2)]


# ----------------------------------------------------------------------------- a. the generators on the graph of the network
@pytest.mark.parametrize("cs", GRAPH, ids=sc.key)
def test_every_generator_is_nonnegative_on_the_graph(cs):
    """z' G_i z >= -(64 * 2^-52 |z|' |G_i| |z| + the float32 allowance of the generator's kind) at every stored witness, corner and
    sample.  With "exact" intervals the bounded generator of post-activation j is also 0 at that neuron's stored argmax and argmin, up
    to 2 (hi - lo) * 2e-9 (1 + |end|): the end lies within 1e-9 (1 + |v|) of the LP value, which lies within 1e-9 (1 + |v|) of the
    attained one (a swapped or shifted end fails this).  A Tanh neuron whose oracle interval has an end at exactly 0.0 has NaN slopes
    (the quirk kept from the reference, test d): only on edge0, and its sector generator is left out there.  Prints the most negative
    value per QC kind (DESIGN section 7 quotes the worst over the cases)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sc.oracle_query(cs)
    kinds = generator_kinds(q)
    nan = np.isnan(q.qc_sector.smin) | np.isnan(q.qc_sector.smax)
    assert not nan.any() or (cs["activ"] == "tanh" and cs["box"] == "edge0" and nan.sum() == 1)
    Z = points_of(cs)
    slack = slack_of(cs, q, Z @ qc.make_R(q.net).T)
    if nan.any():
        q.qc_sector.smin, q.qc_sector.smax = np.where(nan, 0.0, q.qc_sector.smin), np.where(nan, 0.0, q.qc_sector.smax)
    _, G = ipm.literal_generators(q)
    vals = np.einsum("pa,iab,pb->ip", Z, G, Z)
    rnd = MARGIN * np.einsum("pa,iab,pb->ip", np.abs(Z), np.abs(G), np.abs(Z))
    worst = {}
    for i, (kind, j) in enumerate(kinds):
        if kind == "out" or (kind == "sector" and j >= 0 and nan[j]):
            continue
        tol = rnd[i] + (slack[kind][:, j] if slack is not None and kind in slack else 0.0)
        p = int(np.argmin(vals[i] + tol))
        worst[kind] = min(worst.get(kind, 0.0), float(vals[i].min()))
        assert np.all(vals[i] >= -tol), (sc.key(cs), kind, j, float(vals[i, p]), float(np.broadcast_to(tol, vals[i].shape)[p]))
    print(f"{sc.key(cs)}: most negative generator value per kind " + ", ".join(f"{k} {v:+.3e}" for k, v in sorted(worst.items())))
    if cs["source"] == "exact":
        bx, n = sc.box_of(cs["net"], "relu", cs["box"]), q.qc_sector.acxdim
        first = q.gamma_dims()[0] + 1
        for side in ("xmax", "xmin"):
            for j in range(n):
                z = sc.lifted(cs, bx["post"][side][j])
                lo, hi = q.qc_bounded.acymin[j], q.qc_bounded.acymax[j]
                cap = 2.0 * (hi - lo) * 2.0 * sc.WIDEN * (1.0 + max(abs(lo), abs(hi))) + MARGIN * float(np.abs(z) @ np.abs(G[first + j]) @ np.abs(z))
                assert abs(float(z @ G[first + j] @ z)) <= cap, (sc.key(cs), side, j, float(z @ G[first + j] @ z), cap)


# ----------------------------------------------------------------------------- b. the out generator
@pytest.mark.parametrize("net", sc.NETS)
def test_the_out_generator_is_the_documented_form(net):
    """with every other multiplier 0: z' Z(g e_out) z = 2 (c' f(x) - g) (hyperplane), |f(x) - yc|^2 - g (circle), |invP f(x) - yc|^2 - g
    (ellipsoid: the reference's S33 = yc' yc - g), and z' Z z = 2 (c' f(x) - h) for the safety set hplane_S(c, h), at 1e-12 (1 + |value|)"""
    rng = np.random.default_rng(4)
    for box in sc.QUAD_BOXES:
        for out in ("hplane", "circle", "ellipsoid"):
            cs = sc.make(net, "relu", box, out, "top", 0, "exact")
            q = sc.oracle_query(cs)
            nin = q.gamma_dims()[0]
            for x in np.vstack([sc.truth(cs)[1], sc.samples(cs, 10, 6)]):
                g = float(rng.normal())
                gamma = np.zeros(q.ngamma)
                gamma[nin] = g
                z, f = sc.lifted(cs, x), sc.form_value(cs, x)
                got, want = float(z @ qc.assemble_Z_literal(q, gamma) @ z), (2.0 * (f - g) if out == "hplane" else f - g)
                assert abs(got - want) <= 1e-12 * (1.0 + abs(want)), (net, box, out, got, want)
        cs = sc.make(net, "relu", box, "hplane", "top", 0, "exact")
        c, h = sc.normal(cs), float(rng.normal())
        q = sc.oracle_query(cs, S=qc.hplane_S(c, h, sc.oracle_net(cs)))
        for x in sc.samples(cs, 10, 7):
            z, f = sc.lifted(cs, x), sc.form_value(cs, x)
            got = float(z @ qc.assemble_Z_literal(q, np.zeros(q.ngamma)) @ z)
            assert abs(got - 2.0 * (f - h)) <= 1e-12 * (1.0 + abs(f - h)), (net, box, "safety", got, 2.0 * (f - h))


# ----------------------------------------------------------------------------- c. the oracle's SDP against the truth
def test_the_table_is_not_vacuous():
    """every direction that claims soundness has w >= 1e-2 (rho >= 0 alone would not pass it); the negative directions are negative; 10
    of 22 directions (2-8-8-2) and 12 of 26 (3-10-10-3) qualify on the root box; the fixture holds every case of the table.  A circle or
    ellipsoid bounds a squared distance from f(centre), which is small on a small box (3.6e-5 on 2-8-8-2 small-a): there w > 0 is all
    that can be asked, and the bracket of the interior point carries the case"""
    for cs in sc.all_cases():
        g = sc.stored(cs)
        w, x = sc.truth(cs)
        assert g["w"] == w and np.array_equal(np.array(g["x"]), x), sc.key(cs)
        if cs["out"] != "hplane":
            assert w > 0.0 and g["lower"] > 0.0, (sc.key(cs), w)
        elif sc.claims_soundness(cs):
            assert w >= sc.W_MIN, (sc.key(cs), w)
        else:
            assert w <= -sc.W_MIN, (sc.key(cs), w)
        if cs["out"] == "hplane":
            assert abs(sc.form_value(cs, x) - w) <= 1e-12 * (1.0 + abs(w))
    assert [len(sc.qualifying(n)) for n in sc.NETS] == [10, 12]
    assert sorted(sc.fixture()["cases"]) == sorted(sc.key(cs) for cs in sc.all_cases())
    for cs in sc.relu_hplane_cases("exact"):
        top, lit = (sc.normal(dict(cs, dir=d)) for d in ("top", "lit"))
        assert not np.array_equal(top, lit)


def test_the_interior_point_respects_the_truth():
    """rho_ipm >= w - (gap + pinf) (1 + |w|) on every case that claims soundness, both interval sources (with "product" on the tight
    box edge0 the float32 intervals' excess of about 1e-7 would show here if it reached rho); |rho_ipm| <= 1e-8 on the negative
    directions; and with "exact" intervals on 2-8-8-2 half-a, half-b, edge0: rho_ipm - w <= 1e-7 (1 + |w|), ten times the interior
    point's tol_gap - the relaxation is tight there, so the truth is two-sided and an unsound QC cannot hide behind slack"""
    for cs in sc.all_cases():
        g = sc.stored(cs)
        if sc.claims_soundness(cs):
            assert g["rho_ipm"] >= g["w"] - (g["gap"] + g["pinf"]) * (1.0 + abs(g["w"])), (sc.key(cs), g["rho_ipm"] - g["w"])
            assert g["lower"] <= g["upper"]
        else:
            assert abs(g["rho_ipm"]) <= 1e-8, (sc.key(cs), g["rho_ipm"])
    for cs in sc.tight_cases("exact"):
        g = sc.stored(cs)
        print(f"{sc.key(cs)}: rho_ipm - w = {g['rho_ipm'] - g['w']:+.3e}")
        assert g["rho_ipm"] - g["w"] <= 1e-7 * (1.0 + abs(g["w"])), (sc.key(cs), g["rho_ipm"] - g["w"])
    for cs in sc.tight_cases("product"):
        g = sc.stored(cs)
        print(f"{sc.key(cs)}: rho_ipm - w = {g['rho_ipm'] - g['w']:+.3e}")


LIVE = [sc.make("2-8-8-2", "relu", "half-a", "hplane", "top", 0, "exact"), sc.make("3-10-10-3", "relu", "small-a", "hplane", "lit", 2, "exact"),
        sc.make("2-8-8-2", "tanh", "small-a", "hplane", "top", 2, "product"), sc.make("3-10-10-3", "tanh", "root", "hplane", "top", 0, "product"),
        sc.make("2-8-8-2", "tanh", "root", "hplane", "top", 2, "product"), sc.make("2-8-8-2", "relu", "half-a", "hplane", "neg", 0, "exact")]


@pytest.mark.parametrize("cs", LIVE, ids=sc.key)
def test_a_live_solve_reproduces_the_fixture(cs):
    """one case per net and activation solved again by the fixture's own procedure (the four runs of sdp_truth_common.ipm_bracket):
    rho_ipm within its stored gap.  Also 2-8-8-2 Tanh root at beta 2, where 10 neurons cross 0 and the coupling makes the optimum move
    with smax (6.4e-4 for smax = tanh(u) / u), and a negative direction, where the live solve itself must return |rho| <= 1e-8: an
    interior point that left gamma_out free would return the negative value"""
    g = sc.stored(cs)
    r, lower, upper, _ = sc.ipm_bracket(cs, g["w"])
    assert abs(upper - g["rho_ipm"]) <= g["gap"] * (1.0 + abs(g["rho_ipm"])), (sc.key(cs), upper, g["rho_ipm"], g["gap"])
    assert lower <= upper
    if not sc.claims_soundness(cs):
        assert abs(upper) <= 1e-8 and np.all(r.gamma >= 0.0), (sc.key(cs), upper)


TANH_SLOPES = [sc.make(n, "tanh", b, "hplane", "top", 2, "product") for n in sc.NETS for b in ("root", "edge0", "stable", "point", "small-a")]


@pytest.mark.parametrize("cs", TANH_SLOPES, ids=sc.key)
def test_tanh_sector_slopes_are_the_range_of_the_slope(cs):
    """{smin_j, smax_j} of the product's host routine (nnsdp_make_intervals_activ behind makeQcActivs) and of oracle/qc.py
    make_sector_min_max, each on its own pre-activation intervals, against the range of tanh(x) / x over that interval from
    sdp_truth_common.slope_range (mpmath): 4 * 2^-52 relative (one division and two library tanh).  As a set, because the reference
    returns the two in the other order on a negative interval.  A neuron with an end at exactly 0.0 has the NaN the reference has.
    At least one case has crossing intervals (10 on 2-8-8-2 root): there the upper end must be 1"""
    bx, net = sc.box_of(cs["net"], "tanh", cs["box"]), sc.setting(cs["net"], "tanh")["net"]
    out = na.frontend._intervals_native(bx["lo"], bx["hi"], net)
    with np.errstate(invalid="ignore", divide="ignore"):
        qo = sc.oracle_query(cs)
        intv = oiv.intervals_crown_sliced(qo.net, bx["lo"], bx["hi"], activ="tanh")
    olo, ohi = np.concatenate([a for a, _ in intv.acx_intvs]), np.concatenate([b for _, b in intv.acx_intvs])
    crossing = 0
    for label, lo, hi, smin, smax in (("product", out[2], out[3], out[4], out[5]), ("oracle", olo, ohi, qo.qc_sector.smin, qo.qc_sector.smax)):
        for j in range(len(lo)):
            if lo[j] == 0.0 or hi[j] == 0.0:
                assert np.isnan(smin[j]) or np.isnan(smax[j]), (sc.key(cs), label, j)
                continue
            inf, sup = sc.slope_range(lo[j], hi[j])
            crossing += bool(lo[j] < 0.0 < hi[j])
            got = sorted([float(smin[j]), float(smax[j])])
            assert abs(got[0] - inf) <= 4.0 * sc.EPS * inf and abs(got[1] - sup) <= 4.0 * sc.EPS * sup, (sc.key(cs), label, j, lo[j], hi[j], got, inf, sup)
    assert crossing >= 10 or (cs["net"], cs["box"]) != ("2-8-8-2", "root")


# ----------------------------------------------------------------------------- d. the refused Tanh queries
TANH_ALL = [sc.make(n, "tanh", b, "hplane", "top", 0, "product") for n in sc.NETS for b in ("root", "edge0", "stable", "point", "small-a")]


@pytest.mark.parametrize("cs", TANH_ALL, ids=sc.key)
def test_refused_tanh_queries_raise_and_return_no_bound(cs):
    """makeQcActivs on a refused box raises AssertionError from QcActivSector (methods.py: "smin / smax contain NaN", or the bare
    lexicographic assertion) before any query, Solver or runQuery exists, so no bound can come back; the same slopes handed to
    QcActivSector directly are refused the same way.  On every other box the QCs are built and finite.  3-10-10-3 edge0 (an upper
    pre-activation end of exactly 0.0) is the NaN case the issue names; it must be among the refused"""
    why = sc.tanh_refusal(cs)
    bx, net = sc.box_of(cs["net"], "tanh", cs["box"]), sc.setting(cs["net"], "tanh")["net"]
    if why is None:
        qb, qs = na.makeQcActivs(net, bx["lo"], bx["hi"], 0)
        assert np.all(np.isfinite(qs.smin)) and np.all(np.isfinite(qs.smax)) and np.all(qb.acymin <= qb.acymax)
        return
    with pytest.raises(AssertionError, match="NaN" if why == "nan" else None):
        na.makeQcActivs(net, bx["lo"], bx["hi"], 0)
    with pytest.raises(AssertionError):
        sc.product_query(cs)
    if why == "nan":
        with pytest.raises(AssertionError, match="NaN"):
            na.QcActivSector(acxdim=2, beta=0, smin=np.array([0.5, np.nan]), smax=np.array([1.0, 1.0]), activ=na.methods.TanhActiv)


def test_the_nan_case_exists():
    refused = {sc.key(cs): sc.tanh_refusal(cs) for cs in TANH_ALL}
    assert refused[sc.key(sc.make("3-10-10-3", "tanh", "edge0", "hplane", "top", 0, "product"))] == "nan"
    print({k: v for k, v in refused.items() if v})
