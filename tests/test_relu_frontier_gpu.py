"""The device-resident node frontier of the ReLU split (ReluSplitOptions(frontier="device"), CrownBounder.search_nodes,
csrc/crown_node_search.hpp): every case runs the host loop and the device loop on crown_backend="resident" and holds the two results
equal field by field, the bits of `bound` and `witness` included; one net's closed leaves are also checked by enumeration, without the
host loop; info() shows what crosses the bus."""
import numpy as np
import pytest

import nnsdp_amd as na
import exact_common as xc
import literal_common as lc
import node_truth_common as nc
import relu_split_common as rs

CHUNKS = (1, 7, 4096)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint8)


def assert_same(host, dev):
    """two ReluSplitResults, field by field; `bound` and `witness` by their bytes, so NaN equals NaN.  Only `seconds` may differ"""
    assert (dev.verdict, dev.reason, dev.visited, dev.depth) == (host.verdict, host.reason, host.visited, host.depth)
    assert (host.witness is None) == (dev.witness is None)
    if host.witness is not None:
        assert dev.witness.dtype == np.float64 and np.array_equal(_bits(host.witness), _bits(dev.witness))
    for name in ("leaves", "open"):
        a, b = getattr(host, name), getattr(dev, name)
        assert len(a) == len(b), (name, len(a), len(b))
        for k, (x, y) in enumerate(zip(a, b)):
            assert y.assign.dtype == np.int8 and np.array_equal(x.assign, y.assign), (name, k)
            assert (x.depth, x.closed_by) == (y.depth, y.closed_by), (name, k)
            assert np.array_equal(_bits(x.bound), _bits(y.bound)), (name, k, x.bound, y.bound)
    assert "kernel" in dev.seconds and dev.seconds["kernel"] > 0.0


def both(net, lo, hi, literals, chunks=CHUNKS, **kw):
    """the host frontier once, the device frontier per chunk, compared -> the host result"""
    host = na.verifyReluSplit(net, lo, hi, literals, na.ReluSplitOptions(crown_backend="resident", **kw))
    for chunk in chunks:
        dev = na.verifyReluSplit(net, lo, hi, literals, na.ReluSplitOptions(crown_backend="resident", frontier="device", chunk=chunk, **kw))
        assert_same(host, dev)
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(xc.SMALL))
def test_the_fixture_nets_for_every_chunk(name):
    """levels longer than the chunk and no multiple of it; the refuted cases end at the root (2-8-8-2, after 1 node) and below it
    through a corner point (3-10-10-3, after 7)"""
    st = xc.verdict_setting(name)
    seen = {}
    for rel in xc.RELS:
        res = both(st["net"], st["lo"], st["hi"], [(st["normal"], rs.literal_threshold(st, rel))])
        print(f"{name} rel {rel:+.0e}: {res.verdict} ({res.reason}), visited {res.visited}, depth {res.depth}")
        assert res.verdict == ("holds" if rel > 0 else "violated")
        seen[rel] = res.visited
    assert seen[1e-2] > 7 and seen[-1e-2] == (1 if name == "2-8-8-2" else 7)


@pytest.mark.gpu
def test_stuck_nodes_and_the_order_of_open():
    """clipping alone on 2-8-8-2 at rel = 1e-4: "exhausted" with 46 stuck nodes after 135, collected over several levels"""
    st = xc.verdict_setting("2-8-8-2")
    res = both(st["net"], st["lo"], st["hi"], [(st["normal"], rs.literal_threshold(st, 1e-4))], steps=0)
    assert (res.verdict, res.reason, res.visited, len(res.open)) == ("unknown", "exhausted", 135, 46)
    assert len({lf.depth for lf in res.open}) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw, visited", ((dict(max_nodes=20), 15), (dict(max_depth=3), 15), (dict(max_nodes=1), 1)))
def test_budgets(kw, visited):
    st = xc.verdict_setting("3-10-10-3")
    res = both(st["net"], st["lo"], st["hi"], [(st["normal"], rs.literal_threshold(st, 1e-2))], **kw)
    assert (res.verdict, res.reason, res.visited) == ("unknown", "budget", visited) and res.open and not any(lf.closed_by for lf in res.open)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nc.DRIVER))
def test_two_literal_clauses(name):
    st = nc.driver_setting(name)
    for rel in xc.RELS:
        h = nc.driver_thresholds(name, rel)
        res = both(st["net"], st["lo"], st["hi"], [(st["C"][i], h[i]) for i in range(2)], chunks=(7, 4096), max_nodes=2048)
        print(f"{name} rel {rel:+.0e}: {res.verdict} ({res.reason}), visited {res.visited}, {len(res.leaves)} leaves, {len(res.open)} open")


def seven_literals(f):
    """3-17-33-4 (acdim 50: no multiple of 8 or of a 16-row tile) on the box of half-width 1 of rs.kernel_cases() with its 7 literals:
    h_i = a sampled maximum plus f times the root's slack, from the host routine (no GPU); row 3 of C is zero, so h_3 = -1 keeps
    that literal false everywhere"""
    cs = rs.kernel_cases()[0]
    net, C, lo, hi = cs["net"], cs["C"], cs["lo"][:, 4], cs["hi"][:, 4]
    root = na.makeIntervalsNodes(net, lo[:, None], hi[:, None], np.zeros((50, 1), dtype=np.int8), C, steps=16)
    X = lo[:, None] + np.random.default_rng(0).random((3, 20000)) * (hi - lo)[:, None]
    top = (C @ lc.forward(net, X)).max(axis=1)
    hs = top + f * (root.smax[:, 0] - top)
    hs[3] = -1.0
    return net, lo, hi, [(C[i], hs[i]) for i in range(7)]


@pytest.mark.gpu
@pytest.mark.parametrize("f, kw, want", ((0.1, {}, "holds"), (-0.05, dict(max_nodes=600), "unknown")))
def test_seven_literals_on_fifty_neurons(f, kw, want):
    assert sum(rs.kernel_cases()[0]["net"].xdims[1:-1]) == 50
    res = both(*seven_literals(f), chunks=(7, 4096), **kw)
    print(f"3-17-33-4 f {f}: {res.verdict} ({res.reason}), visited {res.visited}, depth {res.depth}, {len(res.leaves)} leaves, {len(res.open)} open")
    assert res.verdict == want and res.visited > 100
    assert any(lf.assign[:17].any() for lf in res.leaves) and any(lf.assign[17:].any() for lf in res.leaves)      # both hidden layers branch


@pytest.mark.gpu
def test_without_corner_points():
    st = xc.verdict_setting("3-10-10-3")
    for rel in (1e-2, -1e-2):
        res = both(st["net"], st["lo"], st["hi"], [(st["normal"], rs.literal_threshold(st, rel))], chunks=(7,), corner_points=False, max_nodes=512)
        print(f"no corner points, rel {rel:+.0e}: {res.verdict} ({res.reason}), visited {res.visited}")


@pytest.mark.gpu
@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_several_candidates_on_one_level(sign):
    """thresholds below the root's smin: every point of the box violates every literal, so the centre and the corners are all flagged
    at the root and all confirm; the witness is the first of them in the order of np.unique(axis=1), in both frontiers.  The second
    case negates the normals, which moves the corners"""
    st = nc.driver_setting("3-10-10-3")
    net, lo, hi, C = st["net"], st["lo"], st["hi"], sign * st["C"]
    with na.CrownBounder(net, C) as bd:
        root = bd.bound_nodes(lo[:, None], hi[:, None], np.zeros((20, 1), dtype=np.int8), steps=16)
    hs = root.smin[:, 0] - 0.1
    literals = [(C[i], hs[i]) for i in range(2)]
    c, r = 0.5 * (lo + hi), 0.5 * (hi - lo)
    X = np.unique(np.concatenate([c[:, None], (c[None, :] + np.sign(root.A[:, :, 0]) * r[None, :]).T], axis=1), axis=1)
    confirmed = [k for k in range(X.shape[1]) if np.all(C @ xc.forward64(net, X[:, k]) > hs)]
    host = na.verifyReluSplit(net, lo, hi, literals, na.ReluSplitOptions(crown_backend="resident"))
    assert len(confirmed) >= 2 and host.verdict == "violated" and host.visited == 1
    assert np.array_equal(_bits(host.witness), _bits(X[:, confirmed[0]]))
    print(f"sign {sign:+.0f}: {X.shape[1]} distinct points, {len(confirmed)} confirm, witness {host.witness.tolist()}")
    both(net, lo, hi, literals, chunks=(4096,))


@pytest.mark.gpu
def test_sixteen_inputs_hold_in_101_nodes():
    net = lc.random_net([16, 16, 16, 2], 7)
    lo, hi = -0.5 * np.ones(16), 0.5 * np.ones(16)
    lit = [(np.array([1.0, -1.0]), 0.95)]
    host = both(net, lo, hi, lit, chunks=(7, 4096))
    dev = na.verifyReluSplit(net, lo, hi, lit, na.ReluSplitOptions(crown_backend="resident", frontier="device"))
    assert (dev.verdict, dev.visited, host.visited) == ("holds", 101, 101) and not dev.open
    rs.check_tree(dev, 32)


@pytest.mark.gpu
def test_the_closed_leaves_by_enumeration():
    """independent of the host loop: every closed leaf of the device frontier's trees on 3-6-6-6-3 is right by enumeration of its node,
    with the tolerances of node_truth_common.rel_tol(False) (what node_truth_common.check_driver holds the host loop to)"""
    import node_truth as nt
    name = "3-6-6-6-3"
    st, tol = nc.driver_setting(name), nc.rel_tol(False)
    net, lo, hi, Cm = st["net"], st["lo"], st["hi"], st["C"]
    checked = infeasible = 0
    for rel in xc.RELS:
        h = nc.driver_thresholds(name, rel)
        res = na.verifyReluSplit(net, lo, hi, [(Cm[i], h[i]) for i in range(2)],
                                 na.ReluSplitOptions(max_nodes=8192, crown_backend="resident", frontier="device", chunk=5))
        assert res.verdict == nc.DECIDED[name][rel]
        if res.verdict == "violated":
            assert np.all(res.witness >= lo) and np.all(res.witness <= hi) and np.all(Cm @ xc.forward64(net, res.witness) > h)
        rs.check_tree(res, sum(net.xdims[1:-1]))
        for lf in res.leaves:
            s = nt.node_regions(net.Ms, lo, hi, lf.assign)
            checked += 1
            if lf.closed_by == "infeasible":
                infeasible += 1
                assert np.isnan(lf.bound)
                if s.leaves:
                    top, bot = nt.node_pre_range(s)
                    margin = tol * (1.0 + max(float(np.abs(top.v).max()), float(np.abs(bot.v).max())))
                    assert nt.node_depth(s).v <= margin, (rel, lf.assign.tolist())
            else:
                assert lf.closed_by == "bound" and nt.clause_max(s, Cm, h).v <= tol, (rel, lf.assign.tolist())
    print(f"{name}: {checked} closed leaves of the device frontier checked by enumeration, {infeasible} infeasible")
    assert checked >= 20 and infeasible >= 1


@pytest.mark.gpu
def test_what_crosses_the_bus():
    """a "holds" search reads one status record per level and downloads no points; a refuted one downloads the points of its last level
    alone; the buffers of a second identical search are the first one's"""
    st = xc.verdict_setting("3-10-10-3")
    net, lo, hi = st["net"], st["lo"], st["hi"]
    with na.CrownBounder(net, st["normal"][None, :]) as bd:
        i0 = bd.info()
        assert (i0["node_searches"], i0["node_search_levels"], i0["node_point_downloads"]) == (0, 0, 0)
        r = bd.search_nodes(lo, hi, [rs.literal_threshold(st, 1e-2)], chunk=64)
        i1 = bd.info()
        assert r["verdict"] == "holds" and r["visited"] == 313 and r["kernel_ms"] > 0.0
        assert (i1["node_searches"], i1["node_search_levels"], i1["node_point_downloads"]) == (1, r["depth"] + 1, 0)
        assert i1["device_bytes"] > i0["device_bytes"] and i1["network_uploads"] == 1
        again = bd.search_nodes(lo, hi, [rs.literal_threshold(st, 1e-2)], chunk=64)
        i2 = bd.info()
        assert (i2["device_allocations"], i2["device_bytes"]) == (i1["device_allocations"], i1["device_bytes"])
        assert all(np.array_equal(_bits(r[k]), _bits(again[k])) for k in ("bound",)) and np.array_equal(r["assign"], again["assign"])
        v = bd.search_nodes(lo, hi, [rs.literal_threshold(st, -1e-2)])
        i3 = bd.info()
        assert v["verdict"] == "violated" and v["visited"] == 7
        assert (i3["node_search_levels"] - i2["node_search_levels"], i3["node_point_downloads"]) == (v["depth"] + 1, 1)
        # confirm decides: a search whose every candidate is turned down goes on
        none = bd.search_nodes(lo, hi, [rs.literal_threshold(st, -1e-2)], max_nodes=64, confirm=lambda x: False)
        assert none["verdict"] != "violated" and none["witness"] is None and none["visited"] > 7


@pytest.mark.gpu
def test_the_refusals_on_a_live_handle():
    cs = rs.kernel_cases()[2]
    net, Cm = cs["net"], cs["C"]
    lo, hi, hs = cs["lo"][:, 0], cs["hi"][:, 0], np.zeros(len(Cm))
    tanh = na.FeedFwdNet(xdims=net.xdims, Ms=net.Ms, activ=na.methods.TanhActiv)
    for make, word in ((lambda: na.CrownBounder(tanh, Cm), "Tanh"), (lambda: na.CrownBounder(net), "literals"),
                       (lambda: na.CrownBounder(net, Cm, max_width=128), "wide")):
        with make() as bd:
            before = bd.info()
            with pytest.raises(na._lib.NnsdpError, match=word):
                bd.search_nodes(lo, hi, hs)
            assert bd.info() == before
    with na.CrownBounder(net, Cm) as bd:
        before = bd.info()
        for kw, word in ((dict(max_nodes=0), "max_nodes"), (dict(chunk=0), "chunk"), (dict(max_depth=-1), "max_depth"), (dict(steps=65), "steps"),
                         (dict(eta0=0.0), "eta0"), (dict(decay=2.0), "decay"), (dict(max_nodes=2 ** 31 - 1), "2\\^31")):
            with pytest.raises(na._lib.NnsdpError, match=word):
                bd.search_nodes(lo, hi, hs, **kw)
        for args, word in (((lo, hi, hs[:3]), "nlit"), ((hi + 1.0, lo, hs), "x1min"), ((lo, hi, np.full(len(Cm), np.nan)), "not finite")):
            with pytest.raises(na._lib.NnsdpError, match=word):
                bd.search_nodes(*args)
        assert bd.info() == before
