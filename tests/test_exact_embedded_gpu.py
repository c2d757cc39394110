"""The kernels against exact ReLU ranges beyond one MFMA tile.  tests/embed_common.py embeds the two small nets of
tests/golden/exact_ranges.json in nets of width 17 to 128 without changing their function (tests/test_exact_embedded_cpu.py checks that,
and that the yardstick below is usable, without a GPU), so the stored extrema, witnesses and thresholds are ground truth for the second
to eighth column tile and the k tail of crown_pass and k_crown_alpha and for all of k_crown_wide: slabs, both column tiles of a wave, the
skip of tile w + 4.  Tolerances are the project's own on the embedded net and the boxes of the call: ec.fp64_tols, max(8 r, 64 * 2^-52 * s)
with r = |R(float64) - R(long double)|, and alpha_tols of tests/test_exact_soundness_gpu.py at returned slopes.  Every test prints the
worst (w - bound) / tol with its array and box; 1 is the limit."""
import numpy as np
import pytest

import crown_tanh_common as tc
import embed_common as em_
import exact_common as ec
import literal_common as lc
import nnsdp_amd as na
import reach_common as rc
from test_exact_soundness_gpu import ENTRIES, alpha_tols, run_entry
from test_split_resident_gpu import assert_same_tree

pytestmark = pytest.mark.gpu
WIDE, NARROW = em_.combos(em_.WIDE), em_.combos(em_.NARROW)
ids = lambda cases: [em_.label(*c[:3]) + "".join(f" {x}" for x in c[3:]) for c in cases]
TEN = lc.NAMES + lc.LIT_NAMES
_cache = {}


def wide_bound(e):
    """the wide bounder's result on the embedded net and the 8 fixture boxes: one call per case"""
    if "wide" not in e:
        with na.CrownBounder(e["net"], e["C"], max_width=128) as bd:
            assert bd.max_width == 128
            e["wide"] = bd.bound(e["lo"], e["hi"])
    return e["wide"]


# ----------------------------------------------------------------------------- a. the wide bounder at the witnesses
@pytest.mark.parametrize("name,widths,kind", WIDE, ids=ids(WIDE))
def test_the_wide_bounder_respects_the_exact_extrema(name, widths, kind):
    """ec.check_sound at the live rows on the 8 fixture boxes; tight on the point box, and on the all-stable box where the filler is
    stable too.  And the linear form at the stored argmax of every literal and box, a value it must dominate:
    A' xmax + b0 >= C f(xmax) - (tol_A sum_q |xmax_q| + tol_b0)"""
    e = em_.case(name, widths, kind)
    tol, res = em_.tols(e), wide_bound(e)
    worst, nm, box = ec.check_sound(f"{e['label']} wide", e["small"], em_.cut(e, ec.entry_arrays(res)), tol, tight=em_.tight_boxes(e, kind))
    print(f"{e['label']} wide: worst (w - bound) / tol of the entry = {worst:+.3e} ({nm}, box {box})")
    xmax, wmax = ec.stacked(e["small"], "xmax"), ec.stacked(e["small"], "wmax")              # nlit x nbox x n0, nlit x nbox
    lits = res[6]
    form = np.einsum("iqb,ibq->ib", lits.A, xmax) + lits.b0
    t = tol["A"] * np.abs(xmax).sum(axis=2) + tol["b0"]
    ratio = (wmax - form) / t
    i, b = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{e['label']} wide: worst (C f(xmax) - A' xmax - b0) / tol = {ratio[i, b]:+.3e} (literal {i}, box {ec.BOX_NAMES[b]}, tol {t[i, b]:.3e})")
    assert np.all(np.isfinite(form)) and np.all(wmax - form <= t), (e["label"], i, ec.BOX_NAMES[b], float((wmax - form)[i, b]), float(t[i, b]))


# ----------------------------------------------------------------------------- b. wide against narrow
NOT_CANCEL = [c for c in WIDE if c[2] != "cancel"]


@pytest.mark.parametrize("name,widths,kind", NOT_CANCEL, ids=ids(NOT_CANCEL))
def test_the_wide_bounder_agrees_with_the_narrow_one_on_the_small_net(name, widths, kind):
    """"scatter" and "split" leave every CROWN bound of a live neuron, of the outputs and of the literals unchanged in exact arithmetic:
    all ten arrays of the wide bounder on the embedded net, at the live rows, against CrownBounder(small_net, C) on the same boxes,
    within tol_wide + tol_small - the wide kernel pinned to the narrow one at widths 65 to 128 without the numpy restatement.  Copies
    of one neuron have the same acxmin / acxmax bit for bit (interval arithmetic over identical rows: the same operations in the same
    order); their acy* agree within twice the tolerance of the array (each copy is within one of the recurrences)"""
    e = em_.case(name, widths, kind)
    tw, ts = em_.tols(e), em_.small_tols(name)
    got = tc.flat(wide_bound(e))
    if ("narrow", name) not in _cache:
        with na.CrownBounder(e["small"]["net"], e["C"]) as bd:
            _cache[("narrow", name)] = tc.flat(bd.bound(e["lo"], e["hi"]))
    worst = (-np.inf, None)
    for nm, a, b in zip(TEN, got, _cache[("narrow", name)]):
        a = a[e["rows"]] if nm.startswith("ac") else a
        assert a.shape == b.shape and np.all(np.isfinite(a)), nm
        d = np.abs(a - b).reshape(-1, a.shape[-1]).max(axis=0)
        j = int(np.argmax(d))
        print(f"{e['label']} {nm}: |wide - narrow| / tol = {d[j] / (tw[nm] + ts[nm]):.3e} (box {ec.BOX_NAMES[j]}, {d[j]:.3e}, tol {tw[nm] + ts[nm]:.3e})")
        worst = max(worst, (float(d[j] / (tw[nm] + ts[nm])), nm))
        assert d[j] <= tw[nm] + ts[nm], (e["label"], nm, ec.BOX_NAMES[j], float(d[j]))
    print(f"{e['label']}: worst |wide - narrow| / tol = {worst[0]:.3e} ({worst[1]})")
    off = np.concatenate([[0], np.cumsum(e["net"].xdims[1:-1])])
    ncopy = 0
    for k, cp in enumerate(e["info"]["copies"]):
        for c in cp:
            for p in c[1:]:
                ncopy += 1
                for i in (2, 3):
                    assert np.array_equal(got[i][off[k] + p], got[i][off[k] + c[0]]), (e["label"], TEN[i], k, p)
                for i in (0, 1):
                    assert np.all(np.abs(got[i][off[k] + p] - got[i][off[k] + c[0]]) <= 2.0 * tw[TEN[i]]), (e["label"], TEN[i], k, p)
    assert (ncopy > 0) == (kind == "split")


# ----------------------------------------------------------------------------- c. the narrow kernels beyond one tile
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,widths,kind", NARROW, ids=ids(NARROW))
def test_the_narrow_kernels_respect_the_exact_extrema_beyond_one_tile(name, widths, kind, entry):
    """every entry of tests/test_exact_soundness_gpu.py on the narrow layouts (hidden widths 17 to 64: up to four column tiles, k
    tails of 1 and 0).  On "cancel" the optimiser moves the slopes of filler neurons as well: any slope is sound, so the exact maxima
    still hold, and smax <= smax_plain"""
    e = em_.case(name, widths, kind)
    st = dict(cs=e["cs"], lo=e["lo"], hi=e["hi"], tol=em_.tols(e))
    res, tol = run_entry(st, entry)
    if entry.startswith("resident alpha"):
        assert np.all(res[6].smax <= res[6].smax_plain)
    worst, nm, box = ec.check_sound(f"{e['label']} {entry}", e["small"], em_.cut(e, ec.entry_arrays(res)), tol, tight=em_.tight_boxes(e, kind))
    print(f"{e['label']} {entry}: worst (w - bound) / tol of the entry = {worst:+.3e} ({nm}, box {box})")


# ----------------------------------------------------------------------------- d. true verdicts on the wide bounder
OPTION_SETS = {"plain": {}, "literal_bounds": dict(literal_bounds=True), "corner_points": dict(corner_points=True)}
VERDICTS = [c + (o,) for c in WIDE if c[2] != "scatter" for o in OPTION_SETS]


@pytest.mark.parametrize("name,widths,kind,opts", VERDICTS, ids=ids(VERDICTS))
def test_verdicts_on_the_wide_bounder_are_true(name, widths, kind, opts):
    """the literal y_0 - y_last on the root box, h = v + rel (c0 - v) at the four ec.RELS, v the fixture's exact maximum and c0 the
    embedded net's root bound: the true verdict on both frontiers within min(4 096, 4 x the visited count of the host backend with the
    same options), and the two frontiers walk the same tree"""
    e = em_.case(name, widths, kind)
    st = em_.verdict_setting(e)
    for rel in ec.RELS:
        _, host = ec.run_split(st, rel, crown_backend="host", **OPTION_SETS[opts])
        assert host.verdict == ("holds" if rel > 0 else "violated")
        budget = min(ec.MAX_BOXES_CAP, 4 * host.visited)
        runs = {}
        for frontier in ("host", "device"):
            h, runs[frontier] = ec.run_split(st, rel, max_boxes=budget, crown_backend="resident", crown_max_width=128, frontier=frontier, **OPTION_SETS[opts])
            print(f"{e['label']} {opts} {frontier} rel {rel:+.0e}: host backend visited {host.visited}, budget {budget}")
            ec.check_verdict(f"{e['label']} {opts} {frontier}", st, rel, h, runs[frontier])
        assert_same_tree(runs["host"], runs["device"])


# ----------------------------------------------------------------------------- e. reach on the wide bounder
REACH = [c + (cp,) for c in WIDE for cp in ("corner_points", "centres") if c[2] == "scatter" or (c[2] == "cancel" and cp == "corner_points")]


@pytest.mark.parametrize("name,widths,kind,points", REACH, ids=ids(REACH))
def test_reach_on_the_wide_bounder_encloses_the_exact_maxima(name, widths, kind, points):
    """reachSplit at rc.TOL on the root box, every stored row, both frontiers: rc.check_enclosure against the fixture's w, v with the
    slack of tests/test_reach_split_gpu.py (max of the fp64 tolerances of smax and ymax) on the embedded net; the same result bit for bit"""
    e = em_.case(name, widths, kind)
    fb = rc.fixture_box(name, "root")
    tols = ec.fp64_tols(e["cs"], fb["lo"][:, None], fb["hi"][:, None])
    slack = max(tols["smax"], tols["ymax"])
    opt = dict(crown_backend="resident", crown_max_width=128, sdp_per_level=0, corner_points=points == "corner_points", max_boxes=ec.MAX_BOXES_CAP,
               max_depth=64)
    res = {f: na.reachSplit(e["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL, split=na.SplitOptions(frontier=f, **opt)) for f in ("host", "device")}
    for f, r in res.items():
        rc.check_enclosure(f"{e['label']} {points} {f}", r, fb["w"], fb["v"], slack, rc.TOL, fb["lo"], fb["hi"])
        assert r.status == "converged" and r.visited < ec.MAX_BOXES_CAP
    rc.assert_same_reach(res["host"], res["device"])


# ----------------------------------------------------------------------------- f. Tanh
def tanh_grid():
    """the extrema of the outputs and of the stored rows over a 1001 x 1001 grid per fixture box of the 2-8-8-2 net as a Tanh net: values
    the network attains, computed once on the small net (the embedded nets have the same function)"""
    if "grid" not in _cache:
        cs = ec.case("2-8-8-2")
        net = tc.tanh_copy(cs["net"])
        lo, hi = ec.box_arrays(cs)
        gmin, gmax = [], []
        for b in range(lo.shape[1]):
            g0, g1 = np.meshgrid(np.linspace(lo[0, b], hi[0, b], 1001), np.linspace(lo[1, b], hi[1, b], 1001))
            Y = lc.forward(net, np.stack([g0.ravel(), g1.ravel()]))
            rows = np.vstack([Y, cs["C"] @ Y])
            gmin.append(rows.min(axis=1))
            gmax.append(rows.max(axis=1))
        _cache["grid"] = np.stack(gmin, axis=1), np.stack(gmax, axis=1)
    return _cache["grid"]


TANH = [("2-8-8-2", w, kind) for w in ((127, 65), (17, 64)) for kind in em_.KINDS]


@pytest.mark.parametrize("name,widths,kind", TANH, ids=ids(TANH))
def test_the_tanh_kernels_respect_grid_extrema_on_the_embedded_nets(name, widths, kind):
    """the 2-8-8-2 net as a Tanh net, embedded at 127-65 (the wide bounder) and at 17-64 (the resident bounder): ymin / ymax and the
    literal bounds against the grid extrema, within the per-box two-term tolerance of test_the_tanh_kernel_respects_grid_extrema taken
    on the embedded net (R_tanh float64 against long double, plus float64 with tanh / cosh moved by one ulp)"""
    e = em_.case(name, widths, kind, tanh=True)
    net, lo, hi, C = e["net"], e["lo"], e["hi"], e["C"]
    r64, rld = tc.R_tanh(net.Ms, lo, hi, np.float64, C), tc.R_tanh(net.Ms, lo, hi, np.longdouble, C)
    rmv = tc.R_tanh(net.Ms, lo, hi, np.float64, C, lib=tc.Moved(1.0, seed=7))
    with na.CrownBounder(net, C, **(dict(max_width=128) if max(widths) > 64 else {})) as bd:
        got = tc.flat(bd.bound(lo, hi))
    gmin, gmax = tanh_grid()
    ny = net.xdims[-1]
    for nm, wit in (("ymin", gmin[:ny]), ("ymax", gmax[:ny]), ("smin", gmin[ny:]), ("smax", gmax[ny:])):
        i = TEN.index(nm)
        r = np.abs(r64[i] - rld[i]).max(axis=0) + np.abs(rmv[i] - rld[i]).max(axis=0)
        tol = np.maximum(8.0 * r, 64.0 * ec.EPS * np.abs(rld[i]).max(axis=0)).astype(np.float64)[None, :]
        excess = (got[i] - wit) if nm.endswith("min") else (wit - got[i])
        k, b = np.unravel_index(np.argmax(excess / tol), excess.shape)
        print(f"tanh {e['label']} {nm}: worst (w - bound) / tol = {excess[k, b] / tol[0, b]:+.3e} (row {k}, box {ec.BOX_NAMES[b]}, excess {excess[k, b]:+.3e}, "
              f"tol {tol[0, b]:.3e}); tol per box {np.array2string(tol[0], precision=1)}")
        assert np.all(np.isfinite(got[i])) and np.all(excess <= tol), (e["label"], nm, ec.BOX_NAMES[b], float(excess[k, b]), float(tol[0, b]))
