"""The split driver's literal options (SplitOptions.literal_bounds / corner_points, nnsdp_amd/split.py) without a GPU:
crown_backend="host", sdp_per_level=0.  Two instances (literal_common.instance): s = the maximum of the literal over
lo + default_rng(0).random((n0, 20000)) * (hi - lo), c0 = the root box's cheap bound."""
import numpy as np

import nnsdp_amd as na
from literal_common import assert_tiles, forward, instance
from test_split_cpu import HI, LO, NORMAL, net, samples, setting

HOST = dict(crown_backend="host", sdp_per_level=0)
OPTS = na.AdmmSdpOptions()
_runs = {}


def run(which, **kw):
    key = (which,) + tuple(sorted(kw.items()))
    if key not in _runs:
        it = instance(which)
        _runs[key] = na.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, OPTS, na.SplitOptions(**HOST, **kw))
    return _runs[key]


def w10d5(**kw):
    """the "holds" instance of tests/test_split_cpu.py"""
    key = ("w10d5",) + tuple(sorted(kw.items()))
    if key not in _runs:
        s, c0 = setting()
        _runs[key] = na.verifySplit(net(), LO, HI, [(NORMAL, s + 0.25 * (c0 - s))], 0, OPTS, na.SplitOptions(**HOST, **kw))
    return _runs[key]


def test_defaults_are_off():
    so = na.SplitOptions()
    assert so.literal_bounds is False and so.corner_points is False


def test_holds_with_a_quarter_of_the_boxes():
    """net 3-17-33-4 seed 14, box [-1, 1]^3, y_0 - y_3 <= s + 0.05 (c0 - s).  Measured with the float32 host bounds: visited 59 with the
    per-output bound, 15 with the literal bound (the fp64 emulation: 59 and 15)."""
    it = instance("holds")
    plain, lits = run("holds"), run("holds", literal_bounds=True)
    print(f"s {it['s']:.8f} c0 {it['c0']:.8f} h {it['h']:.8f}: visited plain {plain.visited}, literal_bounds {lits.visited}")
    for res in (plain, lits):
        assert res.verdict == "holds" and res.witness is None and res.sdp_solves == 0
        assert_tiles(res.leaves, it["lo"], it["hi"])
        assert all(lf.proved_by == "crown" and lf.literal == 0 for lf in res.leaves)
    assert all(lf.bound <= it["h"] for lf in lits.leaves)
    assert lits.visited < plain.visited
    assert 2 * lits.visited <= plain.visited


def test_violated_at_a_corner():
    """net 5-20-20-20-5 seed 31, box [-1, 1]^5, y_0 - y_4 <= s - 0.1 |s|.  Measured with the host bounds: corner_points visits 3 boxes,
    the plain run ends "unknown" at 512 (the fp64 emulation: 3 and 512)."""
    it = instance("violated")
    res, plain = run("violated", corner_points=True), run("violated")
    print(f"s {it['s']:.8f} h {it['h']:.8f}: corner_points {res.verdict} after {res.visited}, plain {plain.verdict} after {plain.visited}")
    assert res.verdict == "violated" and res.witness is not None
    assert np.all(res.witness >= it["lo"]) and np.all(res.witness <= it["hi"])
    assert float(it["normal"] @ forward(it["net"], res.witness[:, None])[:, 0]) > it["h"]
    assert res.visited <= 64
    assert plain.visited > res.visited
    assert plain.verdict in ("violated", "unknown")


def test_violated_on_the_first_net_too():
    """net 3-17-33-4 seed 14 with the threshold s - 0.1 |s| (the emulation: 163 boxes with centres only, 7 with corners)"""
    it = instance("holds")
    h = it["s"] - 0.1 * abs(it["s"])
    lit = [(it["normal"], h)]
    plain = na.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, OPTS, na.SplitOptions(**HOST))
    res = na.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, OPTS, na.SplitOptions(corner_points=True, **HOST))
    print(f"visited: centres only {plain.visited} ({plain.verdict}), with corners {res.visited} ({res.verdict})")
    assert res.verdict == "violated" and float(it["normal"] @ forward(it["net"], res.witness[:, None])[:, 0]) > h
    assert res.visited <= plain.visited


def test_options_off_change_nothing():
    """both options off, spelled out, against a run that never mentions them: leaf for leaf"""
    a, b = w10d5(), w10d5(literal_bounds=False, corner_points=False)
    assert a.verdict == b.verdict == "holds" and a.visited == b.visited and len(a.leaves) == len(b.leaves)
    for x, y in zip(a.leaves, b.leaves):
        assert np.array_equal(x.lo, y.lo) and np.array_equal(x.hi, y.hi)
        assert (x.depth, x.proved_by, x.literal, x.bound) == (y.depth, y.proved_by, y.literal, y.bound)


def test_the_leaf_names_the_literal_that_was_proved():
    """y_0 - y_3 <= s - 1 (false somewhere: not provable)  OR  y_0 - y_3 <= h (the "holds" threshold): every leaf is proved by literal 1,
    and its bound is literal 1's"""
    it = instance("holds")
    lits = [(it["normal"], it["s"] - 1.0), (it["normal"], it["h"])]
    res = na.verifySplit(it["net"], it["lo"], it["hi"], lits, 0, OPTS, na.SplitOptions(literal_bounds=True, **HOST))
    assert res.verdict == "holds" and res.visited == run("holds", literal_bounds=True).visited
    for lf in res.leaves:
        assert lf.proved_by == "crown" and lf.literal == 1 and it["s"] - 1.0 < lf.bound <= it["h"]
    # two different normals: y_1 <= (its sampled minimum - 1), false everywhere sampled, OR the provable literal
    other = np.array([0.0, 1.0, 0.0, 0.0])
    X = it["lo"][:, None] + np.random.default_rng(1).random((3, 20000)) * (it["hi"] - it["lo"])[:, None]
    lits = [(other, float((other @ forward(it["net"], X)).min()) - 1.0), (it["normal"], it["h"])]
    res = na.verifySplit(it["net"], it["lo"], it["hi"], lits, 0, OPTS, na.SplitOptions(literal_bounds=True, **HOST))
    assert res.verdict == "holds"
    for lf in res.leaves:
        assert lf.literal == 1 and lf.bound <= it["h"]
        Xl = lf.lo[:, None] + np.random.default_rng(2).random((3, 500)) * (lf.hi - lf.lo)[:, None]
        assert np.all(it["normal"] @ forward(it["net"], Xl) <= lf.bound + 1e-5 * (1.0 + abs(lf.bound)))


def test_literal_bounds_never_visit_more():
    pairs = [(run("holds").visited, run("holds", literal_bounds=True).visited),
             (run("violated").visited, run("violated", literal_bounds=True).visited),
             (w10d5().visited, w10d5(literal_bounds=True).visited)]
    print("visited (plain, literal_bounds):", pairs)
    assert all(lit <= plain for plain, lit in pairs)
    assert np.all(NORMAL @ samples(1)[1] <= setting()[0] + 0.25 * (setting()[1] - setting()[0]))
    assert w10d5(literal_bounds=True).verdict == "holds"
