"""Shared by the exact-range tests (test_exact_range_cpu.py, test_exact_soundness_gpu.py) and by tests/golden/make_exact_ranges.py: the
recipes of the fixture's cases, its stored rows, and the reader of tests/golden/exact_ranges.json.  Nothing here needs a GPU."""
import json
import os

import numpy as np

import helpers
import literal_common as lc

FIXTURE = os.path.join(helpers.GOLDEN, "exact_ranges.json")
SMALL = {"2-8-8-2": ([2, 8, 8, 2], 1), "3-10-10-3": ([3, 10, 10, 3], 2)}          # name -> (xdims, seed) of literal_common.random_net
BOX_NAMES = ("root", "half-a", "half-b", "small-a", "small-b", "stable", "point", "edge0")
BLOCK_KEYS = ("vmax", "wmax", "xmax", "vmin", "wmin", "xmin")
_cache = {}


def stored_rows(ny, seed):
    """the literal rows of a small case: literal_rows(ny, 7, seed + 100), then e_j and -e_j for every output"""
    return np.vstack([lc.literal_rows(ny, 7, seed + 100), np.eye(ny), -np.eye(ny)])


def case_net(name):
    if name in SMALL:
        return lc.random_net(*SMALL[name])
    if name == "holds":
        return lc.random_net([3, 17, 33, 4], 14)
    if name == "violated":
        return lc.random_net([5, 20, 20, 20, 5], 31)
    if name == "W10-D5":
        return lc.fixture_net()
    raise KeyError(name)


def case_rows(name):
    if name in SMALL:
        xdims, seed = SMALL[name]
        return stored_rows(xdims[-1], seed)
    return {"holds": np.array([[1.0, 0.0, 0.0, -1.0]]), "violated": np.array([[1.0, 0.0, 0.0, 0.0, -1.0]]), "W10-D5": np.array([[1.0, 0.0]])}[name]


def fixture():
    """the JSON as written; a missing file or case is an error, never a skip"""
    if "fixture" not in _cache:
        with open(FIXTURE) as fh:
            _cache["fixture"] = json.load(fh)
    return _cache["fixture"]


def case(name):
    """dict(net, C, boxes): boxes is a list of dicts with lo, hi (vectors) and the blocks lit / pre / post as arrays (pre and post only
    on the small nets): vmax, wmax (nrow), xmax (nrow x n0), vmin, wmin, xmin"""
    key = ("case", name)
    if key not in _cache:
        raw = fixture()["cases"][name]
        boxes = []
        for bx in raw["boxes"]:
            out = dict(name=bx["name"], lo=np.array(bx["lo"]), hi=np.array(bx["hi"]), regions=bx["regions"], lps=bx["lps"])
            for blk in ("lit", "pre", "post"):
                if blk in bx:
                    out[blk] = {k: np.array(bx[blk][k]) for k in BLOCK_KEYS}
            boxes.append(out)
        _cache[key] = dict(net=case_net(name), C=case_rows(name), boxes=boxes)
    return _cache[key]


def stacked(cs, key, blk="lit"):
    """one array of a block over the boxes of a case: nrow x nbox (x n0 for the argmax / argmin)"""
    return np.stack([bx[blk][key] for bx in cs["boxes"]], axis=1)


def box_arrays(cs):
    """lo, hi as n0 x nbox"""
    return np.stack([bx["lo"] for bx in cs["boxes"]], axis=1), np.stack([bx["hi"] for bx in cs["boxes"]], axis=1)


# ---- what the soundness tests of both files share
EPS = 2.0 ** -52
HOST_SLACK = 1e-5          # tests/test_literal_bounds_cpu.py SLACK: the float32 host routine, relative to 1 + |v|
RELS = (1e-2, 1e-4, -1e-4, -1e-2)
MAX_BOXES_CAP = 4096
ARRAYS = lc.NAMES + ("smin", "smax")


def witnesses(cs):
    """per array of ARRAYS: (w, v), each rows x nbox: the attained value (long-double forward pass at the argmin / argmax) that the bound
    must respect, and the LP value.  acy* are the post-activations, acx* the pre-activations, y* the rows e_j of the literal block"""
    ny = cs["net"].xdims[-1]
    pick = lambda blk, side, rows=slice(None): (stacked(cs, "w" + side, blk)[rows], stacked(cs, "v" + side, blk)[rows])
    out = pick("lit", "min", slice(7, 7 + ny)), pick("lit", "max", slice(7, 7 + ny))
    return dict(zip(ARRAYS, (pick("post", "min"), pick("post", "max"), pick("pre", "min"), pick("pre", "max")) + out + (pick("lit", "min"), pick("lit", "max"))))


def fp64_tols(cs, lo, hi):
    """the tolerance tests/test_crown_batch_gpu.py derives for an fp64 kernel's array: max(8 r, 64 * 2^-52 * s), r = max |R(float64) -
    R(long double)| and s = max |R(long double)| over the boxes of the call -> dict over ARRAYS + A, b0"""
    r64, rld = lc.R(cs["net"].Ms, lo, hi, np.float64, head=cs["C"]), lc.R(cs["net"].Ms, lo, hi, np.longdouble, head=cs["C"])
    tol = {}
    for nm, a64, ald in zip(lc.NAMES + lc.LIT_NAMES, r64, rld):
        tol[nm] = max(8.0 * float(np.abs(a64 - ald).max()), 64.0 * EPS * float(np.abs(ald).max()))
    return tol


def host_tols(cs):
    """the float32 host routine: HOST_SLACK (1 + |w|) per value"""
    return {nm: HOST_SLACK * (1.0 + np.abs(w)) for nm, (w, _) in witnesses(cs).items()}


def check_sound(label, cs, arrays, tol, report=None, tight=("point", "stable")):
    """arrays: dict over (a subset of) ARRAYS -> rows x nbox.  lower <= w_min + tol and upper >= w_max - tol at every witness; on the
    point box every array, and on the all-stable box every CROWN array (acy*, y*, s*: the relaxation of a stable neuron is the neuron),
    is also tight: |bound - v| <= tol.  tight: the boxes of that second check; the default is for the fixture's own nets, and a net that
    has further neurons which are unstable on the "stable" box (tests/embed_common.py, "cancel") passes ("point",).  Prints the worst
    (w - bound) / tol per array with its box -> the worst of the entry"""
    wit, names = witnesses(cs), [bx["name"] for bx in cs["boxes"]]
    worst_all = (-np.inf, None, None)
    for nm, got in arrays.items():
        w, v = wit[nm]
        assert got.shape == w.shape, (label, nm, got.shape, w.shape)
        assert np.all(np.isfinite(got)), (label, nm)
        t = np.broadcast_to(tol[nm], w.shape)
        excess = (got - w) if nm.endswith("min") else (w - got)
        ratio = excess / t
        i, b = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{label} {nm}: worst (w - bound) / tol = {ratio[i, b]:+.3e} (row {i}, box {names[b]}, excess {excess[i, b]:+.3e}, tol {t[i, b]:.3e})")
        if ratio[i, b] > worst_all[0]:
            worst_all = (float(ratio[i, b]), nm, names[b])
        assert np.all(excess <= t), (label, nm, names[b], float(excess[i, b]), float(t[i, b]))
        for bname in tight:
            if bname == "stable" and nm.startswith("acx"):
                continue                       # plain interval arithmetic of the pre-activations: sound, not exact on a box with a width
            j = names.index(bname)
            gap = np.abs(got[:, j] - v[:, j])
            assert np.all(gap <= t[:, j]), (label, nm, bname, float(gap.max()), float(np.max(t[:, j])))
    if report is not None:
        report[label] = worst_all
    return worst_all


def entry_arrays(res):
    """the result of makeIntervalsBatch / CrownBounder.bound -> dict over ARRAYS (the literal arrays only where the entry returned them)"""
    out = dict(zip(lc.NAMES, res[:6]))
    if len(res) > 6:
        out.update(smin=res[6].smin, smax=res[6].smax)
    return out


def forward64(net, x):
    for Mk in net.Ms[:-1]:
        x = np.maximum(Mk[:, :-1] @ x + Mk[:, -1], 0.0)
    return net.Ms[-1][:, :-1] @ x + net.Ms[-1][:, -1]


def verdict_setting(name):
    """the literal y_0 - y_last on the root box of a small case: net, lo, hi, normal, v (the exact maximum, from the fixture), c0 (the
    root's cheap bound from the host routine, which needs no GPU)"""
    import nnsdp_amd as na
    key = ("verdict", name)
    if key not in _cache:
        cs = case(name)
        root = cs["boxes"][0]
        assert root["name"] == "root"
        nrm, v = cs["C"][0], float(root["lit"]["vmax"][0])
        iv = na.makeIntervalsBatch(cs["net"], root["lo"][:, None], root["hi"][:, None], backend="host")
        c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
        assert c0 > v
        _cache[key] = dict(net=cs["net"], lo=root["lo"], hi=root["hi"], normal=nrm, v=v, c0=c0)
    return _cache[key]


def run_split(st, rel, max_boxes=MAX_BOXES_CAP, **opts):
    import nnsdp_amd as na
    h = st["v"] + rel * (st["c0"] - st["v"])
    res = na.verifySplit(st["net"], st["lo"], st["hi"], [(st["normal"], h)], 0, na.AdmmSdpOptions(),
                         na.SplitOptions(sdp_per_level=0, max_boxes=int(max_boxes), max_depth=64, **opts))
    return h, res


def check_verdict(label, st, rel, h, res):
    """rel > 0: the clause is true (h > v), rel < 0: false.  The verdict is the true one, never "unknown"; "violated" carries a witness
    inside the box with c' f(x) > h by a numpy forward pass; a "holds" tree tiles the box and every leaf bound is <= h"""
    truth = "holds" if rel > 0 else "violated"
    print(f"{label} rel {rel:+.0e}: h {h:.10f} (v {st['v']:.10f}, c0 {st['c0']:.6f}): {res.verdict}, visited {res.visited}, "
          f"depth {max(lf.depth for lf in res.leaves)}")
    assert res.verdict != ("violated" if rel > 0 else "holds"), (label, rel, "a false verdict")
    if res.verdict == "violated":
        x = res.witness
        assert x is not None and np.all(x >= st["lo"]) and np.all(x <= st["hi"])
        assert st["normal"] @ forward64(st["net"], x) > h
    if res.verdict == "holds":
        assert res.witness is None
        lc.assert_tiles(res.leaves, st["lo"], st["hi"])
        assert all(lf.proved_by == "crown" and lf.bound <= h for lf in res.leaves)
    assert res.verdict == truth, (label, rel, res.verdict, res.visited)
