"""Shared by the reach-split tests (test_reach_split_cpu.py, test_reach_split_gpu.py): `reference`, a float64 numpy restatement of the
level loop of nnsdp_amd.split.reachSplit on the recurrences `R` of literal_common (no library call), and the checks that both files make.
Nothing here needs a GPU."""
import types

import numpy as np

import exact_common as ec
import literal_common as lc
import nnsdp_amd as na

TOL = 1e-3
BOXES = ("root", "half-a", "small-a", "stable", "point", "edge0")
_cache = {}


def support_values(C, Y):
    """s[i, p] = c_i[0] Y[0, p], then + c_i[j] Y[j, p] for j ascending: every product and every sum rounded on its own"""
    s = C[:, 0:1] * Y[0:1, :]
    for j in range(1, C.shape[1]):
        s = s + C[:, j:j + 1] * Y[j:j + 1, :]
    return s


def reference(net, root_lo, root_hi, C, tol, corner_points=True, max_boxes=ec.MAX_BOXES_CAP, max_depth=24):
    """the loop of the issue in float64 numpy, bounds only -> namespace(status, lower, upper, incumbent, witnesses, leaves, visited, depth)"""
    C = np.asarray(C, dtype=np.float64)
    nlit, n0 = C.shape[0], len(root_lo)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (nlit,))
    lo, hi = np.array(root_lo, dtype=np.float64)[:, None], np.array(root_hi, dtype=np.float64)[:, None]
    cuts = np.zeros((n0, 1), dtype=np.int64)
    splittable = root_hi > root_lo
    L, W = np.full(nlit, -np.inf), np.zeros((nlit, n0))
    leaves, visited, depth = [], 1, 0
    while True:
        out = lc.R(net.Ms, lo, hi, np.float64, head=C)
        ymin, ymax, smax, A = out[4], out[5], out[7], out[8]
        cheap = np.stack([np.maximum(nrm[:, None] * ymin, nrm[:, None] * ymax).sum(axis=0) for nrm in C])
        ub = np.minimum(cheap, smax)
        pts = [0.5 * (lo + hi)]
        if corner_points:
            pts += [np.where(A[i] >= 0.0, hi, lo) for i in range(nlit)]
        X = np.concatenate(pts, axis=1)
        s = support_values(C, lc.forward(net, X))
        for i in range(nlit):
            p = int(np.argmax(s[i]))
            if s[i, p] > L[i]:
                L[i], W[i] = s[i, p], X[:, p]
        thr = L + tol
        is_open = np.any(ub > thr[:, None], axis=0)
        for b in np.flatnonzero(~is_open):
            leaves.append(na.ReachLeaf(lo[:, b].copy(), hi[:, b].copy(), depth, "crown", ub[:, b].copy()))
        ids = np.flatnonzero(is_open)
        status = None
        if ids.size == 0:
            status = "converged"
        elif depth >= max_depth or not np.any(splittable) or visited + 2 * ids.size > max_boxes:
            status = "budget"
            for b in ids:
                leaves.append(na.ReachLeaf(lo[:, b].copy(), hi[:, b].copy(), depth, None, ub[:, b].copy()))
        if status is not None:
            lower = np.array([float(C[i] @ lc.forward(net, W[i][:, None])[:, 0]) for i in range(nlit)])
            upper = np.max(np.stack([lf.bound for lf in leaves], axis=1), axis=1)
            return types.SimpleNamespace(status=status, lower=lower, upper=upper, incumbent=L, witnesses=W, leaves=leaves, visited=visited,
                                         depth=depth)
        nlo, nhi, ncuts = [], [], []
        for b in ids:
            j = int(np.argmin(np.where(splittable, cuts[:, b], np.iinfo(np.int64).max)))
            mid = 0.5 * (lo[j, b] + hi[j, b])
            c = cuts[:, b].copy()
            c[j] += 1
            lh, rl = hi[:, b].copy(), lo[:, b].copy()
            lh[j] = mid
            rl[j] = mid
            nlo += [lo[:, b], rl]
            nhi += [lh, hi[:, b]]
            ncuts += [c, c]
        lo, hi, cuts = np.stack(nlo, axis=1), np.stack(nhi, axis=1), np.stack(ncuts, axis=1)
        visited += lo.shape[1]
        depth += 1


def fixture_box(case, box):
    """net, C (the case's stored rows), lo, hi, and per row w (the attained maximum) and v (the exact maximum) of a stored box"""
    cs = ec.case(case)
    bx = next(b for b in cs["boxes"] if b["name"] == box)
    return dict(net=cs["net"], C=cs["C"], lo=bx["lo"], hi=bx["hi"], w=bx["lit"]["wmax"], v=bx["lit"]["vmax"])


def assert_tiles_root(leaves, lo, hi):
    """lc.assert_tiles on the coordinates of the root that have a width; the others are the root's on every leaf"""
    wide = hi > lo
    for lf in leaves:
        assert np.array_equal(lf.lo[~wide], lo[~wide]) and np.array_equal(lf.hi[~wide], hi[~wide])
        assert np.all(lf.lo >= lo) and np.all(lf.hi <= hi)
    lc.assert_tiles([types.SimpleNamespace(lo=lf.lo[wide], hi=lf.hi[wide], depth=lf.depth) for lf in leaves], lo[wide], hi[wide])


def check_enclosure(label, res, w, v, slack, tol, lo, hi):
    """upper >= w - slack, lower <= v + slack, (converged) upper <= incumbent + tol as floats; the leaves tile the root, every leaf has
    its bounds and upper is their maximum; the witnesses lie in the root box"""
    nlit = len(w)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (nlit,))
    gap = res.upper - res.lower
    print(f"{label}: {res.status}, visited {res.visited}, depth {res.depth}, {len(res.leaves)} leaves; worst upper - lower {gap.max():.3e}; "
          f"worst (w - upper) / slack {np.max((w - res.upper) / slack):+.3e}, worst (lower - v) / slack {np.max((res.lower - v) / slack):+.3e}")
    assert res.upper.shape == res.lower.shape == res.incumbent.shape == (nlit,) and res.witnesses.shape == (nlit, len(lo))
    assert np.all(np.isfinite(res.upper)) and np.all(np.isfinite(res.lower)) and np.all(np.isfinite(res.incumbent))
    assert np.all(res.upper >= w - slack), (label, "upper below the attained maximum")
    assert np.all(res.lower <= v + slack), (label, "lower above the exact maximum")
    if res.status == "converged":
        assert np.all(res.upper <= res.incumbent + tol), (label, "converged, but upper > incumbent + tol")
        assert all(lf.closed_by in ("crown", "sdp") for lf in res.leaves)
    else:
        assert res.status == "budget" and any(lf.closed_by is None for lf in res.leaves)
    assert all(lf.bound.shape == (nlit,) and np.all(np.isfinite(lf.bound)) for lf in res.leaves)
    assert np.array_equal(res.upper, np.max(np.stack([lf.bound for lf in res.leaves], axis=1), axis=1))
    assert np.all(res.witnesses >= lo) and np.all(res.witnesses <= hi)
    assert_tiles_root(res.leaves, lo, hi)


def assert_same_reach(a, b):
    """the same result bit for bit: status, visited, depth, incumbent, witnesses and every leaf's lo / hi / depth / closed_by / bound in order"""
    assert (a.status, a.visited, a.depth, len(a.leaves)) == (b.status, b.visited, b.depth, len(b.leaves))
    assert np.array_equal(a.incumbent, b.incumbent) and np.array_equal(a.witnesses, b.witnesses)
    for k, (p, q) in enumerate(zip(a.leaves, b.leaves)):
        assert p.depth == q.depth and p.closed_by == q.closed_by, k
        assert np.array_equal(p.lo, q.lo) and np.array_equal(p.hi, q.hi) and np.array_equal(p.bound, q.bound), k
