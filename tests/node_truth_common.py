"""Shared by the node-truth tests (test_node_truth_cpu.py, test_node_truth_gpu.py) and by tests/golden/make_node_ranges.py: the recipes of
the nodes, the reader of tests/golden/node_ranges.json (exact ranges over every node by tests/node_truth.py) and the checks that the
float32 host routine (makeIntervalsNodes) and the kernels (CrownBounder.bound_nodes) share.  Nothing here needs a GPU, and no check
runs a long enumeration: the truth of the fixed nodes comes from the file; only the leaves of a driver run, which no file can know
beforehand, are enumerated when the test runs (a fraction of a second each).

Groups of nodes (each: net, C, lo / hi n0 x nnode, assign acdim x nnode, x0):
  a/<net>   the 18 nodes of relu_split_common.kernel_cases(), unchanged
  b/<net>   deep nets (K = 4, 5), six nodes each: hw 0.3, three with 20 % and three with 50 % of the neurons forced, three literals
  c/<net>   sibling nodes: 12 nodes with 40 % forced, hw 0.3, then the sign of one forced neuron flipped: most of them are empty
  d/<net>   point boxes lo == hi == x0 on the nets of b: the full pattern of x0, and that pattern with one neuron flipped
  e/<toy>   relu_split_common.toy() with the forced neuron in hidden layer 1 and in hidden layer 2
Full size (`full_size`, 64-64-16-64 with 64 literals) has no enumeration: it is held to the yardstick R and to x0 alone.

Tolerances come from the project, not from the code under test: an fp64 kernel has 1e-6 (1 + |v|) (relu_split_common.check_lp_truth:
HiGHS stops at a primal feasibility of 1e-7), the float32 host routine exact_common.HOST_SLACK (1 + |v|); the margin of the
infeasibility checks is the same number relative to 1 + max |z| over the node."""
import json
import os

import numpy as np

import exact_common as xc
import helpers
import literal_common as lc
import relu_split_common as rs
import nnsdp_amd as na

FIXTURE = os.path.join(helpers.GOLDEN, "node_ranges.json")
DEEP = (([3, 6, 6, 6, 3], 4), ([2, 5, 5, 5, 5, 2], 9), ([4, 12, 12, 12, 2], 3), ([2, 17, 16, 15, 2], 11), ([1, 64, 64, 64, 2], 12))
SIBLINGS = (([3, 6, 6, 6, 3], 4), ([2, 5, 5, 5, 5, 2], 9), ([2, 8, 8, 2], 1), ([4, 12, 12, 12, 2], 3))
DRIVER = {"3-6-6-6-3": ([3, 6, 6, 6, 3], 4, 0.5), "3-10-10-3": ([3, 10, 10, 3], 2, 0.5), "4-8-8-8-2": ([4, 8, 8, 8, 2], 3, 0.4),
          "2-5-5-5-5-2": ([2, 5, 5, 5, 5, 2], 9, 1.0)}
# the cells of the issue's table that the host backend decides with default options and max_nodes = 8192; both backends must decide them
DECIDED = {"3-6-6-6-3": {1e-2: "holds", 1e-4: "holds", -1e-4: "violated", -1e-2: "violated"},
           "3-10-10-3": {1e-2: "holds", -1e-4: "violated", -1e-2: "violated"},
           "4-8-8-8-2": {1e-2: "holds", -1e-2: "violated"},
           "2-5-5-5-5-2": {-1e-2: "violated"}}
STEPS = (0, 16)
_cache = {}


def name_of(xdims):
    return "-".join(str(d) for d in xdims)


def rel_tol(host):
    return xc.HOST_SLACK if host else 1e-6


# ---- the recipes
def _stack(net, C, nodes):
    """nodes: list of (lo, hi, assign, x0)"""
    return dict(net=net, C=C, lo=np.stack([n[0] for n in nodes], 1), hi=np.stack([n[1] for n in nodes], 1),
                assign=np.stack([n[2] for n in nodes], 1).astype(np.int8), x0=np.stack([n[3] for n in nodes], 1))


def _deep(xdims, seed):
    net, rng = lc.random_net(xdims, seed), np.random.default_rng(seed + 900)
    nodes = []
    for frac in (0.2, 0.5, 0.2, 0.5, 0.2, 0.5):
        ctr = rng.uniform(-0.5, 0.5, xdims[0])
        x0, s = rs.node_from_point(net, ctr - 0.3, ctr + 0.3, rng, frac)
        nodes.append((ctr - 0.3, ctr + 0.3, s, x0))
    return _stack(net, lc.literal_rows(xdims[-1], 3, seed + 100), nodes)


def _siblings(xdims, seed):
    net, rng = lc.random_net(xdims, seed), np.random.default_rng(seed + 77)
    nodes = []
    while len(nodes) < 12:
        ctr = rng.uniform(-0.5, 0.5, xdims[0])
        x0, s = rs.node_from_point(net, ctr - 0.3, ctr + 0.3, rng, 0.4)
        forced = np.flatnonzero(s)
        if not len(forced):
            continue
        n = forced[rng.integers(len(forced))]
        s[n] = -s[n]
        nodes.append((ctr - 0.3, ctr + 0.3, s, x0))            # x0 is a point of the sibling, not of this node
    return _stack(net, lc.literal_rows(xdims[-1], 3, seed + 100), nodes)


def _points(xdims, seed):
    net, rng = lc.random_net(xdims, seed), np.random.default_rng(seed + 55)
    x0 = rng.uniform(-0.5, 0.5, xdims[0])
    z = rs.hidden64(net, x0)
    s = np.where(z >= 0.0, 1, -1).astype(np.int8)
    clear = np.flatnonzero(np.abs(z) > 1e-3)
    flipped = s.copy()
    n = clear[rng.integers(len(clear))]
    flipped[n] = -flipped[n]
    return _stack(net, lc.literal_rows(xdims[-1], 3, seed + 100), [(x0, x0, s, x0), (x0, x0, flipped, x0)])


def deep_toys():
    """the toy of relu_split_common (z = (x, x + 1) behind layers that pass x + 2 through, output relu(z_2), box [-1, 1], x <= 0
    forced): the forced neuron in hidden layer 1 of [1, 1, 2, 1] and in hidden layer 2 of [1, 1, 1, 2, 1]"""
    a = lambda *rows: np.array(rows, dtype=np.float64)
    t1 = na.FeedFwdNet(xdims=[1, 1, 2, 1], Ms=[a([1, 2]), a([1, -2], [1, -1]), a([0, 1, 0])])
    t2 = na.FeedFwdNet(xdims=[1, 1, 1, 2, 1], Ms=[a([1, 2]), a([1, 1]), a([1, -3], [1, -2]), a([0, 1, 0])])
    return {"1-1-2-1": (t1, (0, -1, 0)), "1-1-1-2-1": (t2, (0, 0, -1, 0))}


def groups():
    """name -> group, in the order of the module's docstring; built once, never modified"""
    if "groups" not in _cache:
        out = {}
        for cs in rs.kernel_cases():
            out["a/" + name_of(cs["net"].xdims)] = cs
        for xdims, seed in DEEP:
            out["b/" + name_of(xdims)] = _deep(xdims, seed)
        for xdims, seed in SIBLINGS:
            out["c/" + name_of(xdims)] = _siblings(xdims, seed)
        for xdims, seed in DEEP:
            out["d/" + name_of(xdims)] = _points(xdims, seed)
        one = np.ones(1)
        for nm, (net, s) in deep_toys().items():
            out["e/" + nm] = _stack(net, np.array([[1.0]]), [(-one, one, np.array(s, dtype=np.int8), -one)])
        _cache["groups"] = out
    return _cache["groups"]


def names(prefixes):
    return [g for g in groups() if g[0] in prefixes]


def full_size():
    """64-64-16-64 (seed 21) with 64 literals, two nodes of half-width 0.05 with 30 % forced: every dimension loop of both kernels at its
    maximum with n0 = 64"""
    if "full" not in _cache:
        xdims, seed = [64, 64, 16, 64], 21
        net, rng = lc.random_net(xdims, seed), np.random.default_rng(seed + 900)
        nodes = []
        for _ in range(2):
            ctr = rng.uniform(-0.5, 0.5, 64)
            x0, s = rs.node_from_point(net, ctr - 0.05, ctr + 0.05, rng, 0.3)
            nodes.append((ctr - 0.05, ctr + 0.05, s, x0))
        _cache["full"] = _stack(net, lc.literal_rows(64, 64, seed + 100), nodes)
    return _cache["full"]


def driver_setting(name):
    """net, lo, hi of the root box [-hw, hw]^n0, C: two literals"""
    xdims, seed, hw = DRIVER[name]
    return dict(net=lc.random_net(xdims, seed), lo=-hw * np.ones(xdims[0]), hi=hw * np.ones(xdims[0]), C=lc.literal_rows(xdims[-1], 2, seed + 100))


# ---- the file
def fixture():
    """the JSON as written; a missing file, group or node is an error, never a skip"""
    if "fixture" not in _cache:
        with open(FIXTURE) as fh:
            _cache["fixture"] = json.load(fh)
    return _cache["fixture"]


def _num(v):
    return np.array([np.nan if x is None else x for x in v], dtype=np.float64)


def truth(gname):
    """per node of the group: dict(empty, depth, regions, and on a non-empty node vmax, vmin (nlit), zmax, zmin (acdim), margin_z =
    1 + max |z| over the node).  The recipe must reproduce the stored node: lo, hi and assign are compared"""
    key = ("truth", gname)
    if key not in _cache:
        g, raw = groups()[gname], fixture()["groups"][gname]["nodes"]
        assert len(raw) == g["lo"].shape[1], gname
        out = []
        for b, nd in enumerate(raw):
            assert np.array_equal(nd["lo"], g["lo"][:, b]) and np.array_equal(nd["hi"], g["hi"][:, b]), (gname, b, "the recipe moved")
            assert np.array_equal(nd["assign"], g["assign"][:, b]), (gname, b, "the recipe moved")
            t = dict(empty=bool(nd["empty"]), depth=-np.inf if nd["empty"] else (np.inf if nd["depth"] is None else float(nd["depth"])),
                     regions=int(nd["regions"]))
            if not t["empty"]:
                t.update({k: _num(nd[k]) for k in ("vmax", "vmin", "zmax", "zmin")})
                t["margin_z"] = 1.0 + max(float(np.abs(t["zmax"]).max()), float(np.abs(t["zmin"]).max()))
            out.append(t)
        _cache[key] = out
    return _cache[key]


def driver_truth(name):
    """top (the exact maxima of the two rows over the root box), h0 = 0.5 top, v = clause_max(root, C, h0)"""
    raw = fixture()["driver"][name]
    return dict(top=np.array(raw["top"]), h0=np.array(raw["h0"]), v=float(raw["v"]))


# ---- the checks that both routes share; run(net, lo, hi, assign, C, steps) -> na.NodeBounds
def run_group(run, gname, T, cache):
    """the group at T steps, at most 12 nodes per call; computed once per cache, shared, never modified"""
    if (gname, T) not in cache:
        g = groups()[gname]
        assert g["lo"].shape[1] <= 12
        cache[(gname, T)] = run(g["net"], g["lo"], g["hi"], g["assign"], g["C"], T)
    return cache[(gname, T)]


def check_ranges(run, host, gname, cache):
    """a, b and the non-empty nodes of c: per literal smax >= v_max - tol and smin <= v_min + tol; per hidden neuron pre_lo <= zmin + tol
    and pre_hi >= zmax - tol against the range over the node; not infeasible where node_depth >= margin; smax <= smax_plain.
    c: a flagged node has node_depth <= margin (empty: -inf) -> (the smallest slack in units of tol, truly empty nodes, flagged ones
    among them, the largest node_depth of a flagged node)"""
    g, tr, rel = groups()[gname], truth(gname), rel_tol(host)
    tol = lambda v: rel * (1.0 + np.abs(v))
    slack, empties, flagged, deepest = np.inf, 0, 0, -np.inf
    for T in STEPS:
        nb = run_group(run, gname, T, cache)
        assert np.all(nb.smax <= nb.smax_plain), (gname, T)
        for b, t in enumerate(tr):
            margin = rel * t["margin_z"] if not t["empty"] else 0.0
            if nb.infeasible[b]:
                assert t["depth"] <= margin, (gname, T, b, "flagged, but non-empty by", t["depth"])
                deepest = max(deepest, t["depth"])
            if t["empty"]:
                empties, flagged = empties + (T == STEPS[0]), flagged + int(T == STEPS[0] and nb.infeasible[b])
                continue
            assert t["depth"] < margin or not nb.infeasible[b], (gname, T, b, t["depth"])
            if nb.infeasible[b]:
                continue                               # non-empty by less than the margin: the flag is allowed, the bounds mean nothing
            for got, want, up in ((nb.smax[:, b], t["vmax"], True), (nb.smin[:, b], t["vmin"], False),
                                  (nb.pre_hi[:, b], t["zmax"], True), (nb.pre_lo[:, b], t["zmin"], False)):
                room = (got - want if up else want - got) / tol(want)
                slack = min(slack, float(room.min()))
                assert np.all(room >= -1.0), (gname, T, b, "upper" if up else "lower", int(np.argmin(room)), float(room.min()))
    print(f"{gname}: smallest slack {slack:+.3e} tol; {empties} empty nodes, {flagged} of them flagged; deepest flagged node {deepest:.3e}")
    return slack, empties, flagged, deepest


def check_points(run, host, gname):
    """d: on the pattern node smax, smin, pre_lo, pre_hi equal the fp64 forward values to tol and the node is not infeasible; on the
    flipped node infeasible is true (on a point box l = u = z exactly)"""
    g, rel = groups()[gname], rel_tol(host)
    x0 = g["x0"][:, 0]
    z, y = rs.hidden64(g["net"], x0), g["C"] @ xc.forward64(g["net"], x0)
    for T in STEPS:
        nb = run(g["net"], g["lo"], g["hi"], g["assign"], g["C"], T)
        assert not nb.infeasible[0] and nb.infeasible[1], (gname, T, nb.infeasible)
        for got, want in ((nb.smax[:, 0], y), (nb.smin[:, 0], y), (nb.pre_lo[:, 0], z), (nb.pre_hi[:, 0], z)):
            assert np.all(np.abs(got - want) <= rel * (1.0 + np.abs(want))), (gname, T, float(np.abs(got - want).max()))


def check_deep_toys(run, host):
    """e: smax_plain = 2 and 1 - tol <= smax <= 1.5 at 8 steps (check_toy); the iterates 1 and 2 are 1.5 and 1.05: to 1e-12 in fp64"""
    tol = xc.HOST_SLACK * 2.0 if host else 1e-12
    for gname in names("e"):
        g = groups()[gname]
        args = (g["net"], g["lo"], g["hi"], g["assign"], g["C"])
        nb = run(*args, 8)
        print(f"{gname}: smax_plain {nb.smax_plain[0, 0]:.6f}, smax {nb.smax[0, 0]:.6f} at step {nb.best_step[0, 0]}")
        assert abs(nb.smax_plain[0, 0] - 2.0) <= tol and not nb.infeasible[0], gname
        assert 1.0 - tol <= nb.smax[0, 0] <= 1.5, gname
        for T, want in ((1, 1.5), (2, 1.05)):
            nb = run(*args, T)
            assert abs(nb.smax[0, 0] - want) <= tol * (1.0 + want) and nb.best_step[0, 0] == T, (gname, T, nb.smax[0, 0])


def check_full_size_sound(run, host, T=3):
    """f: no enumeration at this size: the bounds hold at x0, smax <= smax_plain, and a node built from a point is not infeasible"""
    g, rel = full_size(), rel_tol(host)
    nb = run(g["net"], g["lo"], g["hi"], g["assign"], g["C"], T)
    assert not nb.infeasible.any() and np.all(nb.smax <= nb.smax_plain)
    Z, Y = rs.hidden64(g["net"], g["x0"]), g["C"] @ lc.forward(g["net"], g["x0"])
    tz, ty = rel * (1.0 + np.abs(Z)), rel * (1.0 + np.abs(Y))
    assert np.all(nb.pre_lo <= Z + tz) and np.all(nb.pre_hi >= Z - tz) and np.all(nb.smax >= Y - ty) and np.all(nb.smin <= Y + ty)
    return nb


# ---- the driver against truth
def driver_thresholds(name, rel):
    t = driver_truth(name)
    return t["h0"] + t["v"] + rel * (1.0 + abs(t["v"]))


def check_driver(backend, name, leaf_share=1):
    """two literals on the root box, h = h0 + v + rel (1 + |v|): the clause holds iff rel > 0.  No run returns the opposite of the truth;
    the cells of DECIDED are decided; every "violated" has a witness in the box that violates every literal in fp64; check_tree passes;
    of every run, also the "unknown" ones, every closed leaf is right by enumeration of its node: an "infeasible" leaf has node_depth <=
    margin, a "bound" leaf clause_max(node, C, h) <= tol.  leaf_share = 3 checks a seeded third of the "bound" leaves (and every
    "infeasible" one) -> the number of leaves checked, the infeasible ones among them, the largest clause_max of a "bound" leaf"""
    import node_truth as nt
    st, host = driver_setting(name), backend == "host"
    net, lo, hi, Cm = st["net"], st["lo"], st["hi"], st["C"]
    acdim, tol = sum(net.xdims[1:-1]), rel_tol(host)
    rng = np.random.default_rng(5)
    checked, infeasible, worst = 0, 0, -np.inf
    for rel in xc.RELS:
        h = driver_thresholds(name, rel)
        res = na.verifyReluSplit(net, lo, hi, [(Cm[i], h[i]) for i in range(2)], na.ReluSplitOptions(max_nodes=8192, crown_backend=backend))
        print(f"{name} {backend} rel {rel:+.0e}: {res.verdict} ({res.reason}), visited {res.visited}, depth {res.depth}, "
              f"{len(res.leaves)} leaves, {len(res.open)} open")
        assert res.verdict != ("violated" if rel > 0 else "holds"), (name, rel, "a false verdict")
        if res.verdict == "violated":
            x = res.witness
            assert x is not None and np.all(x >= lo) and np.all(x <= hi)
            assert np.all(Cm @ xc.forward64(net, x) > h)
        if res.verdict == "holds":
            assert res.witness is None and not res.open
        rs.check_tree(res, acdim)
        if rel in DECIDED[name]:
            assert res.verdict == DECIDED[name][rel], (name, rel, res.verdict, res.reason, res.visited)
        for lf in res.leaves:
            if lf.closed_by == "bound" and leaf_share > 1 and rng.integers(leaf_share) != 0:
                continue
            s = nt.node_regions(net.Ms, lo, hi, lf.assign)
            checked += 1
            if lf.closed_by == "infeasible":
                infeasible += 1
                if s.leaves:
                    top, bot = nt.node_pre_range(s)
                    margin = tol * (1.0 + max(float(np.abs(top.v).max()), float(np.abs(bot.v).max())))
                    assert nt.node_depth(s).v <= margin, (name, rel, lf.assign.tolist(), nt.node_depth(s).v)
            else:
                assert lf.closed_by == "bound"
                v = nt.clause_max(s, Cm, h).v
                worst = max(worst, v)
                assert v <= tol, (name, rel, lf.assign.tolist(), v)
    print(f"{name} {backend}: {checked} closed leaves checked by enumeration, {infeasible} infeasible, largest clause_max of a bound leaf {worst:+.3e}")
    return checked, infeasible, worst
