"""The forest search (CrownBounder.search_many, csrc/crown_forest.hpp; verifySplitMany with frontier = "device"): many root boxes
decided by one level loop on the GPU.  The specification is CrownBounder.search on one root: every comparison below is np.array_equal,
per root and per field, against single searches on a bounder of their own (split_many_common.assert_same_result).  The last test but
one is ground truth instead: the exact maxima of tests/golden/exact_ranges.json."""
import numpy as np
import pytest

import nnsdp_amd as na
import crown_tanh_common as tc
import crown_wide_common as cw
import exact_common as ec
import literal_common as lc
import split_many_common as sm
from test_split_resident_gpu import TANH_H

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions()
KW = dict(max_boxes=sm.MAX_BOXES, max_depth=sm.MAX_DEPTH)
_singles = {}


def singles(net, normals, lo, hi, hs, confirm=None, max_width=64, **kw):
    """CrownBounder.search on every root, on a bounder of its own; computed once per setting when there is no callback"""
    key = (id(net), normals.tobytes(), lo.tobytes(), hi.tobytes(), hs.tobytes(), max_width, tuple(sorted(kw.items())))
    if confirm is None and key in _singles:
        return _singles[key][1]
    with na.CrownBounder(net, normals, max_width=max_width) as cb:
        out = [cb.search(lo[:, r], hi[:, r], hs[:, r], confirm=None if confirm is None else (lambda x, r=r: confirm(r, x)), **kw)
               for r in range(lo.shape[1])]
    if confirm is None:
        _singles[key] = (net, out)
    return out


def many(net, normals, lo, hi, hs, max_width=64, **kw):
    with na.CrownBounder(net, normals, max_width=max_width) as cb:
        return cb.search_many(lo, hi, hs, **kw)


def compare(label, net, normals, lo, hi, hs, confirm=None, max_width=64, group=0, **kw):
    one = singles(net, normals, lo, hi, hs, confirm=confirm, max_width=max_width, **kw)
    got = many(net, normals, lo, hi, hs, max_width=max_width, confirm=confirm, group=group, **kw)
    for r in range(lo.shape[1]):
        sm.assert_same_result(label, got, r, one[r])
    return got, one


# ----------------------------------------------------------------------------- 1. the instance
@pytest.mark.parametrize("literal_bounds,corner_points", [(False, False), (True, False), (False, True), (True, True)])
def test_the_instance_equals_the_single_searches(literal_bounds, corner_points):
    it = sm.instance()
    got, one = compare("instance", it["net"], it["normal"][None], it["lo"], it["hi"], it["hs"], literal_bounds=literal_bounds,
                       corner_points=corner_points, **KW)
    print([(r["verdict"], r["visited"], r["depth"]) for r in one])
    if literal_bounds and not corner_points:       # the setting of tests/test_split_many_cpu.py: its coverage, on the fp64 kernel
        assert set(got["verdict"]) == {"holds", "violated", "unknown"}
        held = [r for r in one if r["verdict"] == "holds"]
        assert any(r["visited"] == 1 for r in held) and any(r["depth"] >= 2 for r in held)


def test_a_clause_of_three_literals_with_thresholds_per_root():
    it = sm.instance()
    normals, hs = sm.second_literal()
    got, one = compare("three literals", it["net"], normals, it["lo"], it["hi"], hs, literal_bounds=True, corner_points=True, **KW)
    by = np.bincount(np.concatenate([r["literal"][r["proved"] == 1] for r in one]), minlength=3)
    print(f"leaves proved per literal {by.tolist()}; verdicts {list(got['verdict'])}")
    assert np.count_nonzero(by) >= 2
    assert any(len(set(r["literal"][r["literal"] >= 0].tolist())) >= 2 for r in one)       # within one root, more than one best literal


def test_verify_split_many_builds_the_results_of_verify_split():
    """the Python layer: frontier "device" (one search_many) against verifySplit with frontier "device" root by root, and against the
    host frontier on one shared resident bounder"""
    it = sm.instance()
    opts = dict(crown_backend="resident", sdp_per_level=0, literal_bounds=True, corner_points=True, **KW)
    lits = [(it["normal"], 0.0)]
    dev = na.verifySplitMany(it["net"], it["lo"], it["hi"], lits, 0, OPTS, na.SplitOptions(frontier="device", **opts), hs=it["hs"])
    host = na.verifySplitMany(it["net"], it["lo"], it["hi"], lits, 0, OPTS, na.SplitOptions(frontier="host", **opts), hs=it["hs"])
    assert len(dev) == len(host) == 8
    for r in range(8):
        one = na.verifySplit(it["net"], it["lo"][:, r], it["hi"][:, r], [(it["normal"], float(it["hs"][0, r]))], 0, OPTS,
                             na.SplitOptions(frontier="device", **opts))
        sm.assert_same_split(dev[r], one)
        sm.assert_same_split(dev[r], host[r])
        assert dev[r].seconds["kernel"] > 0.0 and dev[r].seconds["total"] >= dev[r].seconds["crown"] > 0.0


# ----------------------------------------------------------------------------- 2. budget and depth
@pytest.mark.parametrize("max_boxes", [1, 2, 7, 16])
def test_the_budget_is_per_root(max_boxes):
    it = sm.instance()
    got, one = compare("budget", it["net"], it["normal"][None], it["lo"], it["hi"], it["hs"], literal_bounds=True, max_boxes=max_boxes,
                       max_depth=sm.MAX_DEPTH)
    assert np.all(got["visited"] <= max_boxes)
    never = [int(np.count_nonzero(r["literal"] < 0)) for r in one]
    ends = sorted({r["depth"] for r, n in zip(one, never) if n > 0})
    print(f"max_boxes {max_boxes}: never bounded per root {never}, on levels {ends}")
    if max_boxes in (2, 16):       # (7 = 1 + 2 + 4 ends a complete tree with a level; only a root that proved a box before gets cut there)
        assert sum(n > 0 for n in never) >= 1
    if max_boxes == 16:
        assert len(ends) >= 2       # the budget ends in the middle of different levels for different roots


@pytest.mark.parametrize("max_depth", [0, 1, 3])
def test_max_depth_is_per_root(max_depth):
    it = sm.instance()
    got, _ = compare("depth", it["net"], it["normal"][None], it["lo"], it["hi"], it["hs"], literal_bounds=True, max_boxes=sm.MAX_BOXES,
                     max_depth=max_depth)
    assert int(got["depth"].max()) == max_depth and int(got["leaf_depth"].max()) == max_depth


# ----------------------------------------------------------------------------- 3. degenerate roots
def degenerate_roots():
    """a point box, a box flat in two of three coordinates, a root proved at level 0 (octant 0 with its threshold), a root whose centre
    violates (octant 6, h below the literal at its centre) -> lo, hi (3 x 4), hs (1 x 4)"""
    it = sm.instance()
    lo, hi, hs = [], [], []
    p = np.array([0.25, -0.5, 0.75])
    lo.append(p); hi.append(p.copy()); hs.append(float(it["hs"][0, 3]))
    lo.append(np.array([-1.0, 0.3, -0.2])); hi.append(np.array([0.0, 0.3, -0.2])); hs.append(float(it["hs"][0, 1]))
    lo.append(it["lo"][:, 0]); hi.append(it["hi"][:, 0]); hs.append(float(it["hs"][0, 0]))
    c = 0.5 * (it["lo"][:, 6] + it["hi"][:, 6])
    lo.append(it["lo"][:, 6]); hi.append(it["hi"][:, 6]); hs.append(float(it["normal"] @ lc.forward(it["net"], c[:, None])[:, 0]) - 1e-3)
    return np.stack(lo, axis=1), np.stack(hi, axis=1), np.array([hs])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_degenerate_roots_among_ordinary_ones(where):
    it = sm.instance()
    dlo, dhi, dhs = degenerate_roots()
    keep = [1, 4, 5, 7]
    olo, ohi, ohs = it["lo"][:, keep], it["hi"][:, keep], it["hs"][:, keep]
    at = dict(first=0, middle=2, last=4)[where]
    cat = lambda o, d: np.concatenate([o[:, :at], d, o[:, at:]], axis=1)
    lo, hi, hs = cat(olo, dlo), cat(ohi, dhi), cat(ohs, dhs)
    opts = dict(literal_bounds=True, corner_points=True, **KW)
    got, one = compare(f"degenerate {where}", it["net"], it["normal"][None], lo, hi, hs, **opts)
    d = [one[at + k] for k in range(4)]
    assert d[0]["visited"] == 1 and d[0]["depth"] == 0                                   # nothing to split
    assert all(np.array_equal(x[1:], dlo[1:, 1]) for x in d[1]["lo"]) and (d[1]["visited"] > 1 or d[1]["verdict"] == "holds")
    assert (d[2]["verdict"], d[2]["visited"]) == ("holds", 1)
    assert (d[3]["verdict"], d[3]["visited"]) == ("violated", 1)
    # the ordinary roots' results are those they have without the degenerate ones
    alone = many(it["net"], it["normal"][None], olo, ohi, ohs, **opts)
    others = [k for k in range(8) if not at <= k < at + 4]
    for j, k in enumerate(others):
        a, b = int(alone["leaf_start"][j]), int(alone["leaf_start"][j + 1])
        sm.assert_same_result(f"ordinary {where}", got, k, dict(verdict=str(alone["verdict"][j]), visited=int(alone["visited"][j]),
                              depth=int(alone["depth"][j]), witness=None if np.all(np.isnan(alone["witness"][j])) else alone["witness"][j],
                              **{key: alone[key][a:b] for key in sm.LEAF_KEYS}))


# ----------------------------------------------------------------------------- 4. permutations, one root, a second call
def test_permuting_the_roots_permutes_the_results():
    it = sm.instance()
    perm = np.random.default_rng(3).permutation(8)
    compare("permuted", it["net"], it["normal"][None], it["lo"][:, perm], it["hi"][:, perm], it["hs"][:, perm], literal_bounds=True, **KW)
    got = many(it["net"], it["normal"][None], it["lo"][:, perm], it["hi"][:, perm], it["hs"][:, perm], literal_bounds=True, **KW)
    one = singles(it["net"], it["normal"][None], it["lo"], it["hi"], it["hs"], literal_bounds=True, **KW)
    for k, r in enumerate(perm):
        sm.assert_same_result("permuted", got, k, one[int(r)])


def test_one_root_is_a_search_and_a_second_call_allocates_nothing():
    it = sm.instance()
    kw = dict(literal_bounds=True, corner_points=True, chunk=64, **KW)
    with na.CrownBounder(it["net"], it["normal"][None]) as cb:
        for r in (1, 6):
            single = cb.search(it["lo"][:, r], it["hi"][:, r], it["hs"][:, r], **kw)
            sm.assert_same_result("one root", cb.search_many(it["lo"][:, [r]], it["hi"][:, [r]], it["hs"][:, [r]], **kw), 0, single)
        first = cb.search_many(it["lo"], it["hi"], it["hs"], **kw)
        info1 = cb.info()
        second = cb.search_many(it["lo"], it["hi"], it["hs"], **kw)
        info2 = cb.info()
        for k in ("device_allocations", "network_uploads", "device_bytes", "box_capacity"):
            assert info1[k] == info2[k], k
        assert info2["network_uploads"] == 1 and info2["box_capacity"] <= 64
        assert info2["bound_calls"] - info1["bound_calls"] > 0
        for k in ("verdict", "visited", "depth", "leaf_start") + sm.LEAF_KEYS:
            assert np.array_equal(first[k], second[k]), k
        assert np.array_equal(first["witness"], second["witness"], equal_nan=True)
        none = cb.search_many(np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((1, 0)), **kw)
        assert len(none["verdict"]) == 0 and none["leaf_start"].tolist() == [0] and cb.info() == info2
        # the refusals that need a handle name the root
        bad_hs = it["hs"].copy()
        bad_hs[0, 5] = np.inf
        with pytest.raises(na._lib.NnsdpError, match="root 5, literal 0"):
            cb.search_many(it["lo"], it["hi"], bad_hs, **kw)
        bad_lo = it["lo"].copy()
        bad_lo[1, 2] = 7.0
        with pytest.raises(na._lib.NnsdpError, match="root 2"):
            cb.search_many(bad_lo, it["hi"], it["hs"], **kw)
        with pytest.raises(na._lib.NnsdpError, match=r"2\^31"):
            cb.search_many(it["lo"], it["hi"], it["hs"], **dict(kw, max_boxes=2 ** 23))
        assert cb.info() == info2


# ----------------------------------------------------------------------------- 5. chunks and groups
@pytest.mark.parametrize("chunk", [1, 3, 4096])
def test_chunks_cross_root_boundaries(chunk):
    it = sm.instance()
    compare("chunk", it["net"], it["normal"][None], it["lo"], it["hi"], it["hs"], literal_bounds=True, corner_points=True, chunk=chunk, **KW)


@pytest.mark.parametrize("group", [1, 2, 3])
def test_the_result_does_not_depend_on_the_grouping(group):
    it = sm.instance()
    sel = [1, 6, 0, 2, 5]
    lo, hi, hs = it["lo"][:, sel], it["hi"][:, sel], it["hs"][:, sel]
    kw = dict(literal_bounds=True, **KW)
    whole = many(it["net"], it["normal"][None], lo, hi, hs, group=0, **kw)
    got, _ = compare("group", it["net"], it["normal"][None], lo, hi, hs, group=group, **kw)
    for k in ("verdict", "visited", "depth", "leaf_start") + sm.LEAF_KEYS:
        assert np.array_equal(whole[k], got[k]), k
    assert np.array_equal(whole["witness"], got["witness"], equal_nan=True)


def test_one_bound_launch_per_level_of_the_deepest_root():
    it = sm.instance()
    kw = dict(literal_bounds=True, chunk=4096, **KW)
    with na.CrownBounder(it["net"], it["normal"][None]) as cb:
        before = cb.info()["bound_calls"]
        got = cb.search_many(it["lo"], it["hi"], it["hs"], **kw)
        after = cb.info()["bound_calls"]
    assert int(got["visited"].sum()) <= 4096 and len(set(got["depth"].tolist())) >= 2
    assert after - before == int(got["depth"].max()) + 1          # levels 0 .. depth of the deepest root, not the sum over roots


# ----------------------------------------------------------------------------- 6. the children of a violated root
def corner_setting():
    """root 0: octant 4 with h just below the sampled maximum, which a corner point refutes on level 1 (the host routine says so; the test
    asserts it of the single search); then octants 1, 3, 5 with the instance's thresholds, which go on to level 5 or 6; then octant 1
    with h below its maximum (a corner on level 2)"""
    it = sm.instance()
    sel = [4, 1, 3, 5, 1]
    lo, hi, hs = it["lo"][:, sel], it["hi"][:, sel], it["hs"][:, sel].copy()
    hs[0, 0] = it["s"][4] - 0.03 * abs(it["s"][4])
    hs[0, 4] = it["s"][1] - 0.03 * abs(it["s"][1])
    return it, lo, hi, hs


def is_centre_of_a_leaf(res):
    d = res["depth"]
    return any(np.array_equal(0.5 * (l + u), res["witness"]) for l, u, dd in zip(res["lo"], res["hi"], res["leaf_depth"]) if dd == d)


def test_the_children_of_a_violated_root_are_discarded():
    it, lo, hi, hs = corner_setting()
    got, one = compare("violated children", it["net"], it["normal"][None], lo, hi, hs, literal_bounds=True, corner_points=True, **KW)
    print([(r["verdict"], r["visited"], r["depth"]) for r in one])
    d = one[0]["depth"]
    assert one[0]["verdict"] == "violated" and d >= 1 and not is_centre_of_a_leaf(one[0])
    assert all(one[k]["depth"] >= d + 2 for k in (1, 2, 3))
    assert one[4]["verdict"] == "violated" and one[4]["depth"] > d


def test_a_rejecting_confirm_walks_the_single_searchs_path():
    it, lo, hi, hs = corner_setting()
    normals = it["normal"][None]

    def rejecting(target):
        seen = []

        def confirm(r, x):
            seen.append((r, x.copy()))
            if r == target:
                return sum(1 for q, _ in seen if q == target) > 1          # the first flagged point of this root is rejected
            return bool(normals[0] @ ec.forward64(it["net"], x) > hs[0, r])
        return confirm, seen

    kw = dict(literal_bounds=True, corner_points=True, **KW)
    c1, seen1 = rejecting(0)
    one = singles(it["net"], normals, lo, hi, hs, confirm=c1, **kw)
    c2, seen2 = rejecting(0)
    got = many(it["net"], normals, lo, hi, hs, confirm=c2, **kw)
    for r in range(lo.shape[1]):
        sm.assert_same_result("rejecting confirm", got, r, one[r])
    for r in range(lo.shape[1]):       # per root the same points in the same order
        a, b = [x for q, x in seen1 if q == r], [x for q, x in seen2 if q == r]
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), r
    assert sum(1 for q, _ in seen2 if q == 0) >= 2
    plain = singles(it["net"], normals, lo, hi, hs, **kw)
    assert one[0]["visited"] > plain[0]["visited"] or not np.array_equal(one[0]["witness"], plain[0]["witness"])


# ----------------------------------------------------------------------------- 7. scan sizes
SCAN_BLOCK = 256          # kForestScanBlock of csrc/crown_forest.hpp (kScanTile of csrc/crown_frontier.hpp)


@pytest.mark.parametrize("R", [200, 33000])
def test_levels_longer_than_the_scan_blocks(R):
    """every root is open on level 0 (h halfway between the literal at the centre and the root's bound) and max_depth = 1, so level 1 has
    2 R boxes: 400, more than one scan block, and 66 000, more than one block (256) of block totals, which the second step of the scan
    walks with a carried offset"""
    net = lc.random_net(*ec.SMALL["2-8-8-2"])
    nrm = np.array([[1.0, -1.0]])
    rng = np.random.default_rng(R)
    c = rng.uniform(-1.0, 1.0, size=(2, R))
    lo, hi = c - 0.5, c + 0.5
    assert 2 * R > SCAN_BLOCK and (R == 200 or 2 * R > SCAN_BLOCK * SCAN_BLOCK)
    kw = dict(max_boxes=8, max_depth=1, chunk=1 << 17)
    with na.CrownBounder(net, nrm) as cb:
        iv = cb.bound(lo, hi)
        c0 = np.maximum(nrm[0][:, None] * iv[4], nrm[0][:, None] * iv[5]).sum(axis=0)
        vc = nrm[0] @ lc.forward(net, c)
        hs = (0.5 * (vc + c0))[None]
        got = cb.search_many(lo, hi, hs, **kw)
        sample = np.random.default_rng(7).choice(R, size=16, replace=False)
        for r in sample:
            sm.assert_same_result(f"scan R={R}", got, int(r), cb.search(lo[:, r], hi[:, r], hs[:, r], **kw))
    assert np.all(got["visited"] == 3) and int(got["visited"].sum()) == 3 * R and np.all(got["depth"] == 1)
    assert int(got["leaf_start"][-1]) == 2 * R and np.all(np.diff(got["leaf_start"]) == 2)


# ----------------------------------------------------------------------------- 8. ground truth
def in_the_unit_cube(res, lo, hi):
    """The leaves of a result as boxes of the unit cube, exactly.  check_verdict's tiling test (literal_common.assert_tiles) compares a
    leaf's width with 2^-k of the root's to 1e-12; the stored boxes have corners that are no dyadic numbers, every midpoint 0.5 (lo + hi)
    is rounded to about 2^-54, and from 13 cuts of a coordinate of width 0.1 on that is more than 1e-12 of the leaf's width (depth 38
    occurs below).  So the tree is rebuilt here from the root with the driver's own rule (the least-cut splittable coordinate, the
    midpoint 0.5 (lo + hi)): every leaf must be met with its bits at its depth, exactly once, and no node may go deeper than the leaves
    do, which is a complete bisection tree and asks more than the volumes do.  Each leaf then gets the dyadic box of its node in
    [0, 1]^n0, where the tiling test is exact"""
    want = {}
    for k, lf in enumerate(res.leaves):
        key = (lf.lo.tobytes(), lf.hi.tobytes(), lf.depth)
        assert key not in want, "a leaf occurs twice"
        want[key] = k
    deepest, n0, splittable = max(lf.depth for lf in res.leaves), len(lo), hi > lo
    unit = [None] * len(res.leaves)
    stack = [(lo.copy(), hi.copy(), np.zeros(n0, dtype=np.int64), 0, np.zeros(n0), np.ones(n0))]
    while stack:
        blo, bhi, cuts, depth, ulo, uhi = stack.pop()
        key = (blo.tobytes(), bhi.tobytes(), depth)
        if key in want:
            k = want.pop(key)
            lf = res.leaves[k]
            unit[k] = na.Leaf(ulo, uhi, lf.depth, lf.proved_by, lf.literal, lf.bound)
            continue
        assert depth < deepest and np.any(splittable), "a node of the bisection tree is no leaf and has none below it"
        j = int(np.argmin(np.where(splittable, cuts, np.iinfo(np.int64).max)))
        mid, umid = 0.5 * (blo[j] + bhi[j]), 0.5 * (ulo[j] + uhi[j])
        c = cuts.copy()
        c[j] += 1
        lhi, rlo, ulhi, urlo = bhi.copy(), blo.copy(), uhi.copy(), ulo.copy()
        lhi[j], rlo[j], ulhi[j], urlo[j] = mid, mid, umid, umid
        stack.append((rlo, bhi, c, depth + 1, urlo, uhi))
        stack.append((blo, lhi, c, depth + 1, ulo, ulhi))
    assert not want, "leaves that no node of the bisection tree is"
    return na.SplitResult(res.verdict, unit, res.witness, res.visited, res.sdp_solves, res.seconds)


@pytest.mark.parametrize("name", list(ec.SMALL))
def test_verdicts_are_true_on_the_stored_boxes(name):
    """roots: the eight stored boxes of the case; literal row 0 (y_0 - y_last); h_r = vmax_r + rel (c0_r - vmax_r), vmax_r the exact
    maximum on root r (the fixture), c0_r the root's per-output bound from the host routine; all roots of a case in one call per rel.
    A root is degenerate when c0_r - vmax_r is within the float32 host routine's own error, exact_common.HOST_SLACK (1 + |vmax_r|): the
    point box always, and a box on which the per-output bound is exact up to rounding, where h no longer lies on the side of vmax_r that
    rel names.  Every other root gets the true verdict within 4 096 boxes (exact_common.check_verdict, a "holds" tree through
    in_the_unit_cube).  A degenerate root is judged by
    forward passes: never a false verdict against the exact maximum, a witness violates by a numpy forward pass, and the point box is
    decided by the pass at its point"""
    cs = ec.case(name)
    assert tuple(bx["name"] for bx in cs["boxes"]) == ec.BOX_NAMES
    lo, hi = ec.box_arrays(cs)
    nrm = cs["C"][0]
    v = np.array([float(bx["lit"]["vmax"][0]) for bx in cs["boxes"]])
    c0 = sm.cheap_host(cs["net"], nrm, lo, hi)
    degenerate = c0 - v <= ec.HOST_SLACK * (1.0 + np.abs(v))
    print(f"{name}: degenerate roots {[b for b, d in zip(ec.BOX_NAMES, degenerate) if d]}")
    assert degenerate[ec.BOX_NAMES.index("point")] and not degenerate[0] and np.count_nonzero(~degenerate) >= 5
    split = na.SplitOptions(sdp_per_level=0, crown_backend="resident", frontier="device", literal_bounds=True, corner_points=True,
                            max_boxes=ec.MAX_BOXES_CAP, max_depth=64)
    for rel in ec.RELS:
        hs = (v + rel * (c0 - v))[None]
        res = na.verifySplitMany(cs["net"], lo, hi, [(nrm, 0.0)], 0, OPTS, split, hs=hs)
        for r, bname in enumerate(ec.BOX_NAMES):
            h = float(hs[0, r])
            if not degenerate[r]:
                st = dict(net=cs["net"], lo=lo[:, r], hi=hi[:, r], normal=nrm, v=v[r], c0=c0[r])
                unit = in_the_unit_cube(res[r], lo[:, r], hi[:, r])
                if res[r].verdict == "holds":
                    st.update(lo=np.zeros(lo.shape[0]), hi=np.ones(lo.shape[0]))
                ec.check_verdict(f"{name} {bname}", st, rel, h, unit if res[r].verdict == "holds" else res[r])
                continue
            print(f"{name} {bname} (degenerate) rel {rel:+.0e}: v {v[r]:.12f}, h {h:.12f}: {res[r].verdict} after {res[r].visited}")
            assert res[r].verdict != ("violated" if h >= v[r] else "holds")
            if res[r].verdict == "violated":
                x = res[r].witness
                assert np.all(x >= lo[:, r]) and np.all(x <= hi[:, r]) and nrm @ ec.forward64(cs["net"], x) > h
            if bname == "point":
                y = float(nrm @ ec.forward64(cs["net"], lo[:, r]))
                assert res[r].visited == 1 and res[r].verdict != ("holds" if y > h else "violated")


# ----------------------------------------------------------------------------- 9. the wide instance and Tanh
def test_the_wide_bounder():
    it = cw.instance("3-80-70-3")
    lo = np.array([[-1.0, -1.0, -1.0], [0.0, -1.0, -1.0], [-1.0, 0.0, -1.0], [0.0, 0.0, -1.0]]).T
    hi = lo + np.array([1.0, 1.0, 2.0])[:, None]
    hq, hb = cw.THRESHOLDS["quarter"][0](it["s"], it["c0"]), cw.THRESHOLDS["below"][0](it["s"], it["c0"])
    hs = np.array([[hq, hb, hq, 0.5 * (hq + hb)]])
    got, one = compare("wide", it["net"], it["normal"][None], lo, hi, hs, max_width=128, literal_bounds=True, corner_points=True, max_boxes=128,
                       max_depth=12)
    print([(r["verdict"], r["visited"], r["depth"]) for r in one])
    assert int(got["visited"].sum()) > 4


def test_a_tanh_network():
    tanh = tc.tanh_copy(lc.random_net([3, 17, 33, 4], 14))
    lo, hi = sm.octants()
    hs = np.array([[TANH_H["holds"] if r % 2 == 0 else TANH_H["violated"] for r in range(8)]])
    got, one = compare("tanh", tanh, sm.NORMAL[None], lo, hi, hs, literal_bounds=True, corner_points=True, max_boxes=128, max_depth=8)
    print([(r["verdict"], r["visited"], r["depth"]) for r in one])
    assert int(got["visited"].sum()) > 8
