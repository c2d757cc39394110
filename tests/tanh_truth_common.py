"""Shared by tests/test_tanh_truth_cpu.py and tests/test_tanh_truth_gpu.py: the set of one-neuron intervals at which a Tanh relaxation
can go wrong, the 1-1-1 net that turns a box into that neuron's interval and its literal outputs into the relaxation's two lines, the
two network-level cases (a neuron whose interval is [0, 0], pre-activations beyond +-500), the reader of tests/golden/tanh_ranges.json
and the checks both files make against tests/tanh_truth.py.  Nothing here needs a GPU."""
import json
import os

import mpmath
import numpy as np

import crown_tanh_common as tc
import exact_common as ec
import helpers
import nnsdp_amd as na
import tanh_truth as tt

EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
MARGIN = 64.0                 # tests/test_crown_batch_gpu.py: 64 roundings
FIXTURE = os.path.join(helpers.GOLDEN, "tanh_ranges.json")
BOXES = ("root", "edge0", "stable", "point", "small-a")
GRID_K = (1, 2, 7, 29, 100, 2499)
_cache = {}


def tanh_net(Ms):
    return na.FeedFwdNet(xdims=[Ms[0].shape[1] - 1] + [Mk.shape[0] for Mk in Ms], Ms=[np.asarray(Mk, dtype=np.float64) for Mk in Ms],
                         activ=na.methods.TanhActiv)


# ----------------------------------------------------------------------------- one neuron per box
def one_neuron():
    """y = tanh(x): the box [l, u] is the neuron's interval; with the normals [[1], [-1]] the literal outputs are the two lines: row 0
    gives A = uw, b0 = ub, row 1 gives A = -lw, b0 = -lb"""
    return tanh_net([np.array([[1.0, 0.0]]), np.array([[1.0, 0.0]])]), np.array([[1.0], [-1.0]])


def _chord_condition():
    """crossing intervals at the switch between the chord and the tangent: float64 bisection on l (u fixed) to where the chord's slope
    kd = (tanh u - tanh l) / (u - l) meets tanh'(l), and on u (l fixed) to where it meets tanh'(u); both ends of the last bracket are
    kept, so kd lies within a few ulps (far below 1e-9 relative) of the derivative, once on each side"""
    d = lambda x: 1.0 / np.cosh(x) ** 2
    kd = lambda l, u: (np.tanh(u) - np.tanh(l)) / (u - l)
    out = []
    for t in (0.05, 0.3, 1.0, 2.5, 7.0):
        a, b = -64.0, -1e-9 * t                      # kd - tanh'(l): > 0 at a, < 0 at b
        for _ in range(200):
            m = 0.5 * (a + b)
            a, b = (m, b) if kd(m, t) - d(m) > 0 else (a, m)
        out += [(a, t), (b, t)]
        a, b = 1e-9 * t, 64.0                        # kd - tanh'(u): < 0 at a, > 0 at b
        for _ in range(200):
            m = 0.5 * (a + b)
            a, b = (a, m) if kd(-t, m) - d(m) > 0 else (m, b)
        out += [(-t, a), (-t, b)]
    for l, u in out:
        k = kd(l, u)
        assert l < 0 < u and min(abs(k - d(l)), abs(k - d(u))) <= 1e-9 * k
    return out


def interval_set():
    """-> l, u (float64 arrays) and the name of every interval's group"""
    if "set" in _cache:
        return _cache["set"]
    S = []
    add = lambda name, *pairs: S.extend((name, float(l), float(u)) for l, u in pairs)
    add("zero", (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.3, 0.3), (-0.3, -0.3))
    for t in (1e-300, 1e-7, 1.0, 30.0):
        add("end at zero", (-t, 0.0), (0.0, t))
    for wd in (9.9e-7, 1e-6, 1.1e-6):
        add("width switch", (0.5, 0.5 + wd), (0.0, wd), (-0.5 - wd, -0.5), (-wd, 0.0), (-0.25 * wd, 0.75 * wd), (-0.75 * wd, 0.25 * wd))
    for k in GRID_K:
        for g in {k * 0.01, k / 100.0}:
            for e in (np.nextafter(g, -np.inf), g, np.nextafter(g, np.inf)):
                add("grid", (-1.5, e), (-0.004, e), (-e, 1.5), (-e, 0.004), (-e, e))
    for e in (24.999, 25.0, 25.001):
        add("derivative mask", (e, e + 1.0), (e - 1.0, e), (-e - 1.0, -e), (-e, -e + 1.0), (-1.0, e), (-e, 1.0), (-e, e), (e, e), (-e, -e))
    add("wide", (-30.0, 40.0), (-499.0, 499.5))
    add("clamp", (-500.0, 500.0), (-501.0, 3.0), (-3.0, 501.0), (-600.0, 600.0), (400.0, 1e4), (-1e4, -400.0), (-1e300, 1e300),
        (600.0, 700.0), (-700.0, -600.0), (499.0, 501.0), (-501.0, -499.0), (0.0, 600.0), (-600.0, 0.0))
    add("chord condition", *_chord_condition())
    rng = np.random.default_rng(20)
    wd, c = 10.0 ** rng.uniform(-9.0, 3.0, size=2048), rng.uniform(-30.0, 30.0, size=2048)
    add("sweep", *zip(c - 0.5 * wd, c + 0.5 * wd))
    names = [s[0] for s in S]
    l, u = np.array([s[1] for s in S]), np.array([s[2] for s in S])
    assert np.all(l <= u) and sum(n == "chord condition" for n in names) >= 10 and sum(n == "sweep" for n in names) == 2048
    _cache["set"] = (l, u, names)
    return _cache["set"]


def check_lines(label, lw, lb, uw, ub, l, u, names, eps):
    """line_gap <= 64 eps (1 + |w| max(|l|, |u|)) for both lines of every interval; prints the worst ratio per group"""
    worst, bad = {}, []
    for i in range(len(l)):
        m = max(abs(l[i]), abs(u[i]))
        for side, w, b in (("lower", lw[i], lb[i]), ("upper", uw[i], ub[i])):
            assert np.isfinite(w) and np.isfinite(b), (label, names[i], l[i], u[i], side, w, b)
            gap = tt.line_gap(float(w), float(b), float(l[i]), float(u[i]), side)
            slack = MARGIN * eps * (1.0 + abs(float(w)) * m)
            ratio = float(gap / mpmath.mpf(slack))
            if ratio > worst.get(names[i], (-np.inf,))[0]:
                worst[names[i]] = (ratio, float(l[i]), float(u[i]), side, float(gap))
            if gap > slack:
                bad.append((names[i], float(l[i]), float(u[i]), side, float(w), float(b), float(gap), slack))
    for nm, (ratio, a, b, side, gap) in worst.items():
        print(f"{label} {nm}: worst line_gap / slack = {ratio:+.3e} ({side} line on [{a!r}, {b!r}], gap {gap:+.3e})")
    assert not bad, (label, len(bad), bad[:6])


def check_ends(label, arrays, l, u, eps):
    """the interval of tanh over the box: lower <= tanh(l) and upper >= tanh(u), slack 64 eps (tanh is at most 1)"""
    t = np.array([[tt.tanh_mp(x)[1] for x in l], [tt.tanh_mp(x)[0] for x in u]])
    for nm, lo_arr, hi_arr in arrays:
        over = np.maximum(lo_arr - t[0], t[1] - hi_arr)
        i = int(np.argmax(over))
        print(f"{label} {nm}: worst excess over [tanh l, tanh u] = {over[i]:+.3e} on [{l[i]!r}, {u[i]!r}]")
        assert np.all(np.isfinite(lo_arr)) and np.all(np.isfinite(hi_arr)) and np.all(over <= MARGIN * eps), (label, nm, l[i], u[i], over[i])


def lines_of(res):
    """the result of a bound call on one_neuron() -> lw, lb, uw, ub, one entry per box"""
    lits = res[6]
    return -lits.A[1, 0], -lits.b0[1], lits.A[0, 0], lits.b0[0]


# ----------------------------------------------------------------------------- 100 intervals from one box, beyond the first slab
def selection_net(seed=3):
    """a 1-100-64 Tanh net: hidden neuron i has its own (w_i, b_i) that carries the box [-1, 1] onto interval i of a seeded choice of
    100 intervals of the set, one of every group among them (w_i the half-width and b_i the centre, so the pre-activation interval
    b_i -+ w_i is the set's up to the rounding of the two; the checks take the exact image of the box); the
    output layer selects 64 hidden neurons by a seeded permutation with rows below and above 64.  The normals are e_j for even j and
    -e_j for odd j (64 literals is the most a bounder takes), so literal row j gives the upper line of neuron i = sel[j] in terms of x
    (A = uw w_i, b0 = uw b_i + ub) for even j and its lower line, negated, for odd j.
    -> net, normals, sel, M0 (column 0: w_i, column 1: b_i; the interval of neuron i is b_i -+ w_i)"""
    L, U, names = interval_set()
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero((np.abs(L) < 1e100) & (np.abs(U) < 1e100))
    first = [names.index(g) for g in ("zero", "end at zero", "width switch", "grid", "derivative mask", "wide", "clamp", "chord condition")]
    pick = np.array(first + list(rng.choice(np.setdiff1d(ok, first), size=100 - len(first), replace=False)))
    pick = pick[rng.permutation(100)]
    w, b = 0.5 * (U[pick] - L[pick]), 0.5 * (U[pick] + L[pick])
    M0 = np.stack([w, b], axis=1)
    sel = rng.permutation(100)[:64]
    assert (sel >= 64).sum() >= 8 and (sel < 64).sum() >= 8
    M1 = np.zeros((64, 101))
    M1[np.arange(64), sel] = 1.0
    return tanh_net([M0, M1]), np.diag(np.where(np.arange(64) % 2 == 0, 1.0, -1.0)), sel, M0


def check_selection(label, res, eps=EPS64):
    """the 64 exposed lines of selection_net() and the intervals of all 100 neurons, on the exact image b_i -+ w_i of the box [-1, 1]:
    in z = w_i x + b_i the literal row is the line (A / w_i) z + (b0 - A b_i / w_i), taken in mpmath; w_i = 0 leaves the constant b0"""
    _, _, sel, M0 = selection_net()
    acymin, acymax, lits = res[0][:, 0], res[1][:, 0], res[6]
    mp = mpmath.mpf
    worst = (-np.inf,)
    with mpmath.workdps(tt.DPS):
        for i in range(100):
            w, b = mp(float(M0[i, 0])), mp(float(M0[i, 1]))
            tl, tu = mpmath.tanh(b - w), mpmath.tanh(b + w)
            assert mp(float(acymin[i])) <= tl + MARGIN * eps and mp(float(acymax[i])) >= tu - MARGIN * eps, (label, i, acymin[i], acymax[i])
        for j, i in enumerate(sel):
            w, b = mp(float(M0[i, 0])), mp(float(M0[i, 1]))
            sign = 1 if j % 2 == 0 else -1
            A, b0 = sign * mp(float(lits.A[j, 0, 0])), sign * mp(float(lits.b0[j, 0]))
            k, c = (A / w, b0 - A * b / w) if w > 0 else (mp(0), b0)
            gap = tt.line_gap(k, c, b - w, b + w, "upper" if sign > 0 else "lower")
            slack = MARGIN * eps * (1 + abs(k) * max(abs(b - w), abs(b + w)))
            if gap / slack > worst[0]:
                worst = (float(gap / slack), int(i), j, float(b - w), float(b + w))
            assert gap <= slack, (label, j, int(i), float(b - w), float(b + w), float(gap), float(slack))
    print(f"{label}: worst line_gap / slack = {worst[0]:+.3e} (neuron {worst[1]}, literal {worst[2]}, interval [{worst[3]!r}, {worst[4]!r}])")


# ----------------------------------------------------------------------------- the two network-level cases
def dead_neuron():
    """h = tanh([x + 0.3; 0 x]), y = h_0 + h_1 on [-1, 1]: the second neuron's interval is [0, 0] on every box"""
    return tanh_net([np.array([[1.0, 0.3], [0.0, 0.0]]), np.array([[1.0, 1.0, 0.0]])]), np.array([-1.0]), np.array([1.0])


def origin_point():
    """bias-free, point box at the origin: every hidden interval is [0, 0] and the network's value is exactly 0"""
    return tanh_net([np.array([[1.0, 0.0], [2.0, 0.0]]), np.array([[1.0, 5.0, 0.0]])]), np.array([0.0]), np.array([0.0])


def clamp_net():
    """y = tanh(x) - (0.00397 / 1e-6) tanh(1e-6 x) on [-600, 600]: the first pre-activation passes +-500"""
    return tanh_net([np.array([[1.0, 0.0], [1e-6, 0.0]]), np.array([[1.0, -0.00397 / 1e-6, 0.0]])]), np.array([-600.0]), np.array([600.0])


NORMALS_1 = np.array([[1.0], [-1.0]])


def check_contains(label, net, res, X, eps):
    """every reported interval (acymin / acymax, ymin / ymax, smin / smax for the normals +-1) contains the long-double value of the
    network at the columns of X, slack 64 eps (1 + |v|)"""
    acymin, acymax, _, _, ymin, ymax, lits = res
    print(f"{label}: acy [{acymin[:, 0]}, {acymax[:, 0]}], y [{ymin[:, 0]}, {ymax[:, 0]}], s [{lits.smin[:, 0]}, {lits.smax[:, 0]}]")
    for x in np.atleast_2d(X).T:
        y, hid = tt.forward_ld(net.Ms, x, hidden=True)
        h = np.concatenate(hid)
        for nm, lo_arr, hi_arr, v in (("acy", acymin[:, 0], acymax[:, 0], h), ("y", ymin[:, 0], ymax[:, 0], y),
                                      ("s", lits.smin[:, 0], lits.smax[:, 0], np.array([y[0], -y[0]]))):
            slack = (MARGIN * eps * (1.0 + np.abs(v))).astype(np.float64)
            lo_x, hi_x = (lo_arr - v).astype(np.float64), (v - hi_arr).astype(np.float64)
            assert np.all(np.isfinite(lo_arr)) and np.all(np.isfinite(hi_arr)), (label, nm)
            assert np.all(lo_x <= slack) and np.all(hi_x <= slack), (label, nm, x, lo_arr, hi_arr, v.astype(np.float64))


def clamp_truth():
    """(w_min, v_min, w_max, v_max) of the clamp net's output on its box, by tanh_truth"""
    if "clamp" not in _cache:
        net, lo, hi = clamp_net()
        _cache["clamp"] = tt.enclosed_range(net.Ms, lo, hi, np.array([1.0]), gap=1e-9)
    return _cache["clamp"]


def check_clamp(label, res, eps):
    """ymin <= the true minimum and ymax >= the true maximum of the clamp net: the attained values w bound them from inside, and the
    enclosure v says how near (1e-9) they are"""
    wmin, vmin, wmax, vmax = clamp_truth()
    assert vmin <= wmin <= wmax <= vmax and wmin - vmin <= 1e-8 and vmax - wmax <= 1e-8
    ymin, ymax, lits = res[4][0, 0], res[5][0, 0], res[6]
    slack = MARGIN * eps * (1.0 + max(abs(vmin), abs(vmax)))
    print(f"{label}: ymin {ymin:.6f} (true minimum in [{vmin:.6f}, {wmin:.6f}]), ymax {ymax:.6f} (true maximum in [{wmax:.6f}, {vmax:.6f}]); "
          f"smin {lits.smin[:, 0]}, smax {lits.smax[:, 0]}")
    assert ymin <= wmin + slack and ymax >= wmax - slack, (label, ymin, wmin, ymax, wmax)
    assert lits.smax[0, 0] >= wmax - slack and lits.smin[0, 0] <= wmin + slack
    assert lits.smax[1, 0] >= -wmin - slack and lits.smin[1, 0] <= -wmax + slack


# ----------------------------------------------------------------------------- the fixture
def decide(net, root_lo, root_hi, c, h, max_boxes=1024, max_depth=64):
    """the level loop of verifySplit for one literal c' f(x) <= h in float64 numpy on R_tanh, bounds only, with literal_bounds and
    corner_points (no library call) -> (verdict, boxes bounded).  It chooses the thresholds of the verdict tests; it is no oracle."""
    import literal_common as lc
    C = np.asarray(c, dtype=np.float64)[None]
    lo, hi = np.array(root_lo, dtype=np.float64)[:, None], np.array(root_hi, dtype=np.float64)[:, None]
    cuts = np.zeros_like(lo, dtype=np.int64)
    splittable = root_hi > root_lo
    visited = depth = 0
    while lo.shape[1]:
        room = max_boxes - visited
        if room <= 0:
            return "unknown", visited
        budget_cut = lo.shape[1] > room
        lo, hi, cuts = lo[:, :room], hi[:, :room], cuts[:, :room]
        visited += lo.shape[1]
        out = tc.R_tanh(net.Ms, lo, hi, np.float64, C)
        ub = np.minimum(np.maximum(C[0][:, None] * out[4], C[0][:, None] * out[5]).sum(axis=0), out[7][0])
        ids = np.flatnonzero(ub > h)
        if ids.size:
            X = np.concatenate([0.5 * (lo[:, ids] + hi[:, ids]), np.where(out[8][0][:, ids] >= 0.0, hi[:, ids], lo[:, ids])], axis=1)
            if np.any(C @ lc.forward(net, X) > h):
                return "violated", visited
        if budget_cut or (ids.size and (visited >= max_boxes or depth >= max_depth or not np.any(splittable))):
            return "unknown", visited
        nlo, nhi, ncuts = [], [], []
        for b in ids:
            j = int(np.argmin(np.where(splittable, cuts[:, b], np.iinfo(np.int64).max)))
            mid = 0.5 * (lo[j, b] + hi[j, b])
            cc, lh, rl = cuts[:, b].copy(), hi[:, b].copy(), lo[:, b].copy()
            cc[j] += 1
            lh[j] = rl[j] = mid
            nlo += [lo[:, b], rl]
            nhi += [lh, hi[:, b]]
            ncuts += [cc, cc]
        if not nlo:
            return "holds", visited
        lo, hi, cuts = np.stack(nlo, axis=1), np.stack(nhi, axis=1), np.stack(ncuts, axis=1)
        depth += 1
    return "holds", visited


def fixture_case(name):
    """net (the Tanh copy of exact_common.case_net), C, and per stored box lo, hi, x (nrow x n0), w, v, gap (nrow)"""
    key = ("case", name)
    if key not in _cache:
        with open(FIXTURE) as fh:
            raw = json.load(fh)["cases"][name]
        boxes = [{k: (np.array(v) if k != "name" else v) for k, v in bx.items()} for bx in raw["boxes"]]
        assert [bx["name"] for bx in boxes] == [b for b in BOXES if b in ec.BOX_NAMES]
        _cache[key] = dict(net=tc.tanh_copy(ec.case_net(name)), C=ec.case_rows(name), boxes=boxes)
    return _cache[key]


def fixture_slack(cs, lo, hi):
    """8 r + 64 * 2^-52 * s per array and box (the form of tests/test_crown_resident_gpu.py), r = max |R_tanh(float64) - R_tanh(long
    double)| on that box and s = max |R_tanh(long double)| of the array over the call: two CPU runs, nothing of the GPU -> dict over the
    ten array names, one value per box.  r is about 1e-15 except on edge0, the box built so that an upper pre-activation bound is
    exactly 0.0 in float64: in long double that bound is not 0, the neuron changes regime, and r is the distance between two
    relaxations (up to 0.03 on the bounds and 0.3 on A) - on that box the checks only hold what such a change leaves."""
    import literal_common as lc
    r64 = tc.R_tanh(cs["net"].Ms, lo, hi, np.float64, cs["C"])
    rld = tc.R_tanh(cs["net"].Ms, lo, hi, np.longdouble, cs["C"])
    per_box = lambda a: np.abs(a).reshape(-1, a.shape[-1]).max(axis=0).astype(np.float64)
    return {nm: 8.0 * per_box(a - b) + MARGIN * EPS64 * float(np.abs(b).max()) for nm, a, b in zip(lc.NAMES + lc.LIT_NAMES, r64, rld)}
