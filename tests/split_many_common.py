"""Shared by tests/test_split_many_cpu.py and tests/test_split_many_gpu.py: the instance of the forest search (verifySplitMany,
CrownBounder.search_many) and the comparison of a search_many result with single searches.  Nothing here needs a GPU."""
import itertools

import numpy as np

import nnsdp_amd as na
import literal_common as lc

NORMAL = np.array([1.0, 0.0, 0.0, -1.0])
FRACTIONS = (0.25, 0.05, None, 0.02)          # h_r = s + f (c0 - s); None: s - 0.1 |s|, below the sampled maximum
MAX_BOXES, MAX_DEPTH = 64, 6
LEAF_KEYS = ("lo", "hi", "leaf_depth", "proved", "literal", "bound")
_cache = {}


def octants():
    """the eight octants of [-1, 1]^3 -> lo, hi (3 x 8)"""
    lo = np.array(list(itertools.product((-1.0, 0.0), repeat=3))).T
    return lo, lo + 1.0


def cheap_host(net, normal, lo, hi):
    """per root the per-output bound of the literal from the host routine"""
    iv = na.makeIntervalsBatch(net, lo, hi, backend="host")
    return np.maximum(normal[:, None] * iv[4], normal[:, None] * iv[5]).sum(axis=0)


def sampled_max(net, normal, lo, hi, n=20000):
    """per root the literal's maximum over lo + default_rng(r).random((n0, n)) * (hi - lo)"""
    out = []
    for r in range(lo.shape[1]):
        X = lo[:, [r]] + np.random.default_rng(r).random((lo.shape[0], n)) * (hi[:, [r]] - lo[:, [r]])
        out.append(float((normal @ lc.forward(net, X)).max()))
    return np.array(out)


def instance():
    """net 3-17-33-4 (seed 14), the literal y_0 - y_3, the eight octants as roots; s, c0 (8 each) and hs (1 x 8): the thresholds of
    FRACTIONS in turn"""
    if "instance" not in _cache:
        net = lc.random_net([3, 17, 33, 4], 14)
        lo, hi = octants()
        s, c0 = sampled_max(net, NORMAL, lo, hi), cheap_host(net, NORMAL, lo, hi)
        assert np.all(c0 > s)
        hs = np.array([[s[r] - 0.1 * abs(s[r]) if FRACTIONS[r % 4] is None else s[r] + FRACTIONS[r % 4] * (c0[r] - s[r]) for r in range(8)]])
        _cache["instance"] = dict(net=net, lo=lo, hi=hi, normal=NORMAL, s=s, c0=c0, hs=hs)
    return _cache["instance"]


def second_literal():
    """a second literal, -y_1, with thresholds of its own per root (odd roots: 2 % of its sampled range above its sampled maximum; even
    roots: its 0.9 quantile), and a third, y_2 <= its median.  With the host routine every one of the three is the best literal of some
    leaf, and in five roots more than one is -> normals (3 x 4), hs (3 x 8)"""
    if "second" not in _cache:
        it = instance()
        n2, n3 = np.array([0.0, -1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0])
        h2, h3 = [], []
        for r in range(8):
            X = it["lo"][:, [r]] + np.random.default_rng(100 + r).random((3, 5000)) * (it["hi"][:, [r]] - it["lo"][:, [r]])
            Y = lc.forward(it["net"], X)
            v2 = n2 @ Y
            h2.append(float(v2.max() + 0.02 * (v2.max() - v2.min())) if r % 2 else float(np.quantile(v2, 0.9)))
            h3.append(float(np.quantile(n3 @ Y, 0.5)))
        _cache["second"] = (np.stack([NORMAL, n2, n3]), np.vstack([it["hs"], np.array([h2]), np.array([h3])]))
    return _cache["second"]


def assert_same_result(label, many, r, single):
    """root r of a search_many result against the dict of CrownBounder.search on that root: every field, bit for bit and in order"""
    a, b = int(many["leaf_start"][r]), int(many["leaf_start"][r + 1])
    assert str(many["verdict"][r]) == single["verdict"], (label, r, str(many["verdict"][r]), single["verdict"])
    assert int(many["visited"][r]) == single["visited"], (label, r, int(many["visited"][r]), single["visited"])
    assert int(many["depth"][r]) == single["depth"], (label, r, int(many["depth"][r]), single["depth"])
    if single["witness"] is None:
        assert np.all(np.isnan(many["witness"][r])), (label, r)
    else:
        assert np.array_equal(many["witness"][r], single["witness"]), (label, r)
    assert b - a == len(single["proved"]), (label, r, b - a, len(single["proved"]))
    for k in LEAF_KEYS:
        assert np.array_equal(many[k][a:b], single[k]), (label, r, k)


def assert_same_split(a, b):
    """two SplitResults: the same verdict, witness, visited and leaves, field for field and in order"""
    assert (a.verdict, a.visited, a.sdp_solves, len(a.leaves)) == (b.verdict, b.visited, b.sdp_solves, len(b.leaves))
    assert (a.witness is None) == (b.witness is None) and (a.witness is None or np.array_equal(a.witness, b.witness))
    for la, lb in zip(a.leaves, b.leaves):
        assert np.array_equal(la.lo, lb.lo) and np.array_equal(la.hi, lb.hi)
        assert (la.depth, la.proved_by, la.literal, la.bound) == (lb.depth, lb.proved_by, lb.literal, lb.bound)
