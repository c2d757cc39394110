"""The split driver (nnsdp_amd/split.py) without a GPU: crown_backend="host", sdp_per_level=0.  W10-D5 fixture on the box
[0.5, 1.5]^2, one literal  y_0 <= h  (normal (1, 0)).  s = max of y_0 over 20 000 seeded samples, c0 = the root box's cheap bound;
the thresholds are placed between the two from quantities the tests compute."""
import os

import numpy as np
import pytest

import helpers
import nnsdp_amd as na
from nnsdp_amd import vnnlib as vl

LO, HI = np.array([0.5, 0.5]), np.array([1.5, 1.5])
NORMAL = np.array([1.0, 0.0])
HOST = dict(crown_backend="host", sdp_per_level=0)
_state = {}


def net():
    if "net" not in _state:
        d = helpers.load_problem("W10-D5", 0)
        _state["net"] = na.FeedFwdNet(xdims=[int(v) for v in d["xdims"]], Ms=helpers.problem_Ms(d))
    return _state["net"]


def samples(seed, n=20000):
    X = LO[:, None] + np.random.default_rng(seed).random((2, n)) * (HI - LO)[:, None]
    return X, na.evalFeedFwdNet(net(), X)


def setting():
    """(s, c0) of the literal y_0 <= h on the root box, host bounds"""
    if "s" not in _state:
        _state["s"] = float((NORMAL @ samples(0)[1]).max())
        iv = na.makeIntervalsBatch(net(), LO[:, None], HI[:, None], backend="host")
        _state["c0"] = float(np.maximum(NORMAL * iv[4][:, 0], NORMAL * iv[5][:, 0]).sum())
        assert _state["c0"] > _state["s"]
    return _state["s"], _state["c0"]


def assert_tiles(leaves, lo=LO, hi=HI):
    """the leaves are dyadic sub-boxes of [lo, hi] whose volumes add up to the root's"""
    vol = sum(float(np.prod(lf.hi - lf.lo)) for lf in leaves)
    assert abs(vol - float(np.prod(hi - lo))) <= 1e-12
    for lf in leaves:
        w = (lf.hi - lf.lo) / (hi - lo)
        k = np.round(-np.log2(w))
        assert np.allclose(w, 2.0 ** -k, rtol=1e-12, atol=0) and int(k.sum()) == lf.depth
        pos = (lf.lo - lo) / (hi - lo) * 2.0 ** k
        assert np.allclose(pos, np.round(pos), rtol=0, atol=1e-9)


def test_holds_by_bounds_alone():
    """h = s + 0.25 (c0 - s): the fraction the issue starts from; visited is 19 with the host bounds (the cap is 512)."""
    s, c0 = setting()
    h = s + 0.25 * (c0 - s)
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    print(f"s {s:.8f} c0 {c0:.8f} h {h:.8f}: {res.verdict}, visited {res.visited}, {len(res.leaves)} leaves, seconds {res.seconds}")
    assert res.verdict == "holds" and res.witness is None and res.sdp_solves == 0
    assert res.visited <= 512
    assert_tiles(res.leaves)
    assert all(lf.proved_by == "crown" and lf.literal == 0 and lf.bound <= h for lf in res.leaves)
    assert len(res.leaves) > 1, "the root box alone must not be enough: the instance would not exercise the splitting"
    assert np.all(NORMAL @ samples(1)[1] <= h)
    assert set(res.seconds) == {"crown", "setup", "solve", "finish", "total"} and res.seconds["total"] >= res.seconds["crown"] > 0
    again = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    assert again.visited == res.visited and all(np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi) and a.bound == b.bound
                                               for a, b in zip(again.leaves, res.leaves)), "the driver is deterministic"


def test_violated_with_a_witness():
    s, _ = setting()
    h = s - 0.1 * abs(s)
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    assert res.verdict == "violated" and res.witness is not None
    assert np.all(res.witness >= LO) and np.all(res.witness <= HI)
    x = res.witness
    for Mk in net().Ms[:-1]:
        x = np.maximum(Mk[:, :-1] @ x + Mk[:, -1], 0.0)
    y = net().Ms[-1][:, :-1] @ x + net().Ms[-1][:, -1]
    assert NORMAL @ y > h


def test_unknown_when_the_box_budget_ends():
    s, c0 = setting()
    h = s + 0.25 * (c0 - s)
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(max_boxes=1, **HOST))
    assert res.verdict == "unknown" and res.visited == 1 and res.witness is None
    (lf,) = res.leaves
    assert lf.proved_by is None and lf.depth == 0 and np.array_equal(lf.lo, LO) and np.array_equal(lf.hi, HI)
    deep = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(max_depth=2, **HOST))
    assert deep.verdict == "unknown" and max(lf.depth for lf in deep.leaves) == 2
    assert_tiles(deep.leaves)
    assert any(lf.proved_by is None for lf in deep.leaves)


def test_holds_is_never_returned_with_an_open_leaf():
    """every box budget from 1 to what the instance needs: a budget that ends inside a level leaves boxes unbounded, and the verdict
    is then "unknown" even if every bounded box of that level was proved"""
    s, c0 = setting()
    h = s + 0.25 * (c0 - s)
    need = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST)).visited
    verdicts = []
    for cap in range(1, need + 2):
        res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(max_boxes=cap, **HOST))
        verdicts.append(res.verdict)
        assert res.visited <= cap
        assert_tiles(res.leaves)
        assert (res.verdict == "holds") == all(lf.proved_by is not None for lf in res.leaves), cap
        assert res.verdict in ("holds", "unknown")
    assert verdicts[:need - 1] == ["unknown"] * (need - 1) and verdicts[need - 1:] == ["holds", "holds"]


def test_clause_of_two_literals():
    """y_0 <= a  OR  y_0 >= b  with b < a the 40 % and 60 % quantiles of y_0 on the box: each literal is false on a part of the box and
    true on the rest, the clause holds everywhere"""
    y0 = samples(0)[1][0]
    b, a = np.quantile(y0, 0.4), np.quantile(y0, 0.6)
    lits = [(NORMAL, float(a)), (-NORMAL, float(-b))]
    assert (y0 > a).any() and (y0 < b).any()
    res = na.verifySplit(net(), LO, HI, lits, 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    print(f"a {a:.6f} b {b:.6f}: {res.verdict}, visited {res.visited}, {len(res.leaves)} leaves")
    assert res.verdict == "holds" and res.visited <= 512
    assert_tiles(res.leaves)
    assert {lf.literal for lf in res.leaves} == {0, 1}
    Y = samples(2)[1]
    assert np.all((NORMAL @ Y <= a) | (-NORMAL @ Y <= -b))
    for lf in res.leaves:
        assert lf.proved_by == "crown" and lf.bound <= lits[lf.literal][1]


def test_options_are_checked():
    with pytest.raises(ValueError):
        na.verifySplit(net(), LO, HI, [], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    with pytest.raises(ValueError):
        na.verifySplit(net(), LO, HI, [(np.ones(3), 0.0)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    with pytest.raises(ValueError):
        na.verifySplit(net(), HI, LO, [(NORMAL, 0.0)], 0, na.AdmmSdpOptions(), na.SplitOptions(**HOST))
    with pytest.raises(ValueError):
        na.verifySplit(net(), LO, HI, [(NORMAL, 0.0)], 0, na.AdmmSdpOptions(), na.SplitOptions(crown_backend="cpu"))


def test_host_backend_of_the_batched_intervals_is_the_host_routine():
    rng = np.random.default_rng(4)
    lo = 0.5 + 0.5 * rng.random((2, 40))
    hi = lo + 0.3 * rng.random((2, 40))
    got = na.makeIntervalsBatch(net(), lo, hi, backend="host")
    one = na.makeIntervalsBatch(net(), lo, hi, backend="host", workers=1)
    assert all(np.array_equal(a, b) for a, b in zip(got, one))
    for j in (0, 17, 39):
        xi, acx = na.makeIntervalsInfo(lo[:, j], hi[:, j], net())
        assert np.array_equal(got[0][:, j], np.concatenate([v[0] for v in xi[1:-1]]))
        assert np.array_equal(got[3][:, j], np.concatenate([v[1] for v in acx]))
        assert np.array_equal(got[5][:, j], xi[-1][1])


class _Never:
    """stands in for runQuery: certifies nothing"""

    def __init__(self):
        self.calls = 0

    def __call__(self, query, opts):
        self.calls += 1
        return na.QuerySolution(objective_value=0.0, values={}, termination_status="ITERATION_LIMIT", total_time=0.5, setup_time=0.1,
                                solve_time=0.4, summary={"lambda_max": 0.3})


class _Listed(_Never):
    """certifies the literals whose last S column is listed"""

    def __init__(self, good):
        super().__init__()
        self.good = set(good)

    def __call__(self, query, opts):
        s = super().__call__(query, opts)
        if tuple(float(v) for v in query.qc_safety.S[:, -1]) in self.good:
            s.termination_status, s.summary = "OPTIMAL", {"lambda_max": 1e-9}
        return s


def test_spec_driver_without_split_is_unchanged():
    """verifyAcasSpec(split=None) on tests/golden/vnnlib/prop_or_outputs.vnnlib with a stub solver: the statuses and the number of solves
    of tests/test_vnnlib.py::test_driver_early_exit_semantics, a plain str as the status"""
    from oracle import nnet_io
    n = nnet_io.random_net([2, 6, 6, 3], seed=3)
    small = na.FeedFwdNet(xdims=list(n.xdims), Ms=n.Ms)
    spec = os.path.join(helpers.GOLDEN, "vnnlib", "prop_or_outputs.vnnlib")
    cnf = vl.loadReluQueriesCnf(small, spec, 0)
    key = lambda c, i: tuple(float(v) for v in cnf[c][i].qc_safety.S[:, -1])
    for good, want in (({key(0, 1), key(1, 0)}, (5, 3, "safe")), ({key(1, 0)}, (5, 2, "unsafe"))):
        for kw in ({}, {"split": None}):
            stub = _Listed(good)
            solns, nq, status = vl.verifyAcasSpec(small, spec, 0, na.AdmmSdpOptions(), solve=stub, **kw)
            assert (nq, len(solns), status) == want and type(status) is str and stub.calls == want[1]


def test_spec_driver_hands_an_undecided_clause_to_the_split():
    s, c0 = setting()
    box = "(assert (>= X_0 0.5))(assert (<= X_0 1.5))(assert (>= X_1 0.5))(assert (<= X_1 1.5))"
    split = na.SplitOptions(max_boxes=64, **HOST)
    # unsafe set y_0 >= c: the literal is y_0 <= c - 1e-4
    c = s + 0.25 * (c0 - s) + vl.SPEC_EPS
    stub = _Never()
    solns, nq, status = vl.verifyAcasSpec(net(), box + f"(assert (>= Y_0 {c!r}))", 0, na.AdmmSdpOptions(), solve=stub, split=split)
    assert (nq, stub.calls, status) == (1, 1, "safe") and status.witness is None
    assert [r.verdict for r in status.splits] == ["holds"] and 1 < status.splits[0].visited <= 64
    assert vl.verifyAcasSpec(net(), box + f"(assert (>= Y_0 {c!r}))", 0, na.AdmmSdpOptions(), solve=_Never())[2] == "unsafe"
    c = s - 0.1 * abs(s)
    solns, nq, status = vl.verifyAcasSpec(net(), box + f"(assert (>= Y_0 {c!r}))", 0, na.AdmmSdpOptions(), solve=_Never(), split=split)
    assert status == "violated" and status != "unknown" and na.evalFeedFwdNet(net(), status.witness)[0] >= c
    tight = na.SplitOptions(max_boxes=1, **HOST)
    c = s + 0.25 * (c0 - s) + vl.SPEC_EPS
    solns, nq, status = vl.verifyAcasSpec(net(), box + f"(assert (>= Y_0 {c!r}))", 0, na.AdmmSdpOptions(), solve=_Never(), split=tight)
    assert status == "unknown" and status.witness is None
