"""verifySplitMany and the forest search without a GPU: the host frontier against the list of verifySplit results, the coverage of the
instance that tests/test_split_many_gpu.py runs on the device, the refusals that are made before the GPU is touched, and the grouping
rule of nnsdp_crown_search_many (nnsdp_crown_forest_plan)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import literal_common as lc
import split_many_common as sm

OPTS = na.AdmmSdpOptions()
CAP = 2 ** 31
_state = {}


def host_options(**kw):
    return na.SplitOptions(frontier="host", crown_backend="host", sdp_per_level=0, literal_bounds=True, max_boxes=sm.MAX_BOXES,
                           max_depth=sm.MAX_DEPTH, **kw)


def host_results():
    if "many" not in _state:
        it = sm.instance()
        _state["many"] = na.verifySplitMany(it["net"], it["lo"], it["hi"], [(it["normal"], 0.0)], 0, OPTS, host_options(), hs=it["hs"])
    return _state["many"]


def test_the_host_frontier_is_the_list_of_single_results():
    it, many = sm.instance(), host_results()
    assert len(many) == 8
    for r, res in enumerate(many):
        one = na.verifySplit(it["net"], it["lo"][:, r], it["hi"][:, r], [(it["normal"], float(it["hs"][0, r]))], 0, OPTS, host_options())
        sm.assert_same_split(res, one)
        lc.assert_tiles(res.leaves, it["lo"][:, r], it["hi"][:, r])


def test_without_hs_the_literals_thresholds_hold_for_every_root():
    it = sm.instance()
    h = float(it["hs"][0, 1])
    (got,) = na.verifySplitMany(it["net"], it["lo"][:, [1]], it["hi"][:, [1]], [(it["normal"], h)], 0, OPTS, host_options())
    sm.assert_same_split(got, na.verifySplit(it["net"], it["lo"][:, 1], it["hi"][:, 1], [(it["normal"], h)], 0, OPTS, host_options()))
    sm.assert_same_split(got, host_results()[1])


def test_no_roots_no_results():
    it = sm.instance()
    assert na.verifySplitMany(it["net"], np.zeros((3, 0)), np.zeros((3, 0)), [(it["normal"], 0.0)], 0, OPTS, host_options()) == []
    assert na.verifySplitMany(it["net"], np.zeros((3, 0)), np.zeros((3, 0)), [(it["normal"], 0.0)], 0, OPTS, host_options(),
                              hs=np.zeros((1, 0))) == []


def test_the_instance_covers_every_verdict():
    """what the GPU test relies on: all three verdicts, "holds" at level 0 and after at least two bisections.  An fp64 emulation of the
    driver gave: holds after 1, 7, 17 and 29 boxes, one violated after 33, three unknown"""
    many = host_results()
    for r, res in enumerate(many):
        print(f"root {r}: {res.verdict} after {res.visited} boxes, depth {max(lf.depth for lf in res.leaves)}, {len(res.leaves)} leaves")
    assert {res.verdict for res in many} == {"holds", "violated", "unknown"}
    holds = [res for res in many if res.verdict == "holds"]
    assert any(res.visited == 1 for res in holds)
    assert any(max(lf.depth for lf in res.leaves) >= 2 for res in holds)


def _many(**kw):
    net = lc.random_net([2, 3, 2], 1)
    split = dict(sdp_per_level=0)
    split.update(kw)
    return na.verifySplitMany(net, np.zeros((2, 2)), np.ones((2, 2)), [(np.array([1.0, 0.0]), 0.0)], 0, OPTS, na.SplitOptions(**split))


@pytest.mark.parametrize("options,word", [(dict(sdp_per_level=3), "sdp_per_level"),
                                          (dict(frontier="device", crown_backend="resident", sdp_per_level=3), "sdp_per_level"),
                                          (dict(frontier="device", crown_backend="host"), "crown_backend"),
                                          (dict(frontier="device", crown_backend="gpu"), "crown_backend"),
                                          (dict(frontier="device", crown_backend="resident", samples=2), "samples"),
                                          (dict(frontier="device", crown_backend="resident", literal_bounds=True, alpha_steps=3), "alpha_steps"),
                                          (dict(frontier="gpu"), "frontier")])
def test_verify_split_many_names_the_option_it_cannot_take(options, word):
    with pytest.raises(ValueError, match=word):
        _many(**options)


def test_verify_split_many_checks_its_arrays():
    net = lc.random_net([2, 3, 2], 1)
    lit = [(np.array([1.0, 0.0]), 0.0)]
    with pytest.raises(ValueError, match="xdims"):
        na.verifySplitMany(net, np.zeros(2), np.ones(2), lit, 0, OPTS, na.SplitOptions(sdp_per_level=0))
    with pytest.raises(ValueError, match="hs"):
        na.verifySplitMany(net, np.zeros((2, 3)), np.ones((2, 3)), lit, 0, OPTS, na.SplitOptions(sdp_per_level=0), hs=np.zeros((1, 2)))


def _search_many(h=None, nroot=2, max_boxes=8, max_depth=4, chunk=4, group=0):
    lib = _lib.load()
    dp, ip = _lib.c_double_p, _lib.c_int32_p
    n = max(nroot, 1)
    lo, hi, nrm, hs, wit = np.zeros(2 * n), np.ones(2 * n), np.array([1.0, 0.0]), np.zeros(n), np.zeros(2 * n)
    out = [np.zeros(n, dtype=np.int32) for _ in range(4)]
    rc = lib.nnsdp_crown_search_many(h, nroot, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 1, nrm.ctypes.data_as(dp), hs.ctypes.data_as(dp),
                                     0, 0, max_boxes, max_depth, chunk, group, None, None, *[o.ctypes.data_as(ip) for o in out],
                                     wit.ctypes.data_as(dp), None)
    return rc, lib.nnsdp_last_error().decode()


def test_search_many_refuses_bad_arguments_before_the_gpu():
    for kw, word in ((dict(max_boxes=0), "max_boxes"), (dict(chunk=0), "chunk"), (dict(max_depth=-1), "max_depth"), (dict(group=-1), "group"),
                     (dict(nroot=-1), "nroot")):
        rc, msg = _search_many(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    rc, msg = _search_many()
    assert rc == -1 and "null handle" in msg
    assert _search_many(nroot=0)[0] == 0            # no roots: returns at once, whatever the handle
    lib = _lib.load()
    assert lib.nnsdp_crown_search_many_leaves(None, 0, None, None, None, None, None, None) == -1
    assert "null handle" in lib.nnsdp_last_error().decode()


@pytest.mark.parametrize("n0,nlit,max_boxes,corner", list(itertools.product((1, 5, 64), (1, 64), (1, 512, 2 ** 20), (False, True))))
def test_the_grouping_rule_keeps_every_buffer_within_the_cap(n0, nlit, max_boxes, corner):
    """restated from the buffers' contents (csrc/crown_forest.hpp, ForestPlan): per root 2 max_boxes boxes per frontier"""
    ny, nroot = 5, 10 ** 6

    def sizes(g):
        cap = 2 * max_boxes * g
        npts = (2 if corner else 1) * cap
        logw = 2 * n0 + 4
        frontier = 2 * cap * (n0 * (8 + 8 + 4) + 4)
        doubles = 8 * (g + nlit * g + nlit * ny + cap + npts * n0 + npts * ny + max_boxes * g * logw + cap * logw)
        ints = 4 * (5 * g + 5 * g + 3 * g + 3 * cap + npts + 5 * cap + 5 * (-(-cap // 256) + 1))
        return cap, frontier, doubles, ints

    one = sizes(1)
    if max(one[1:]) > CAP:
        with pytest.raises(_lib.NnsdpError, match=str(max(b for b in one[1:] if b > CAP)) if sum(b > CAP for b in one[1:]) == 1 else "bytes"):
            na.frontend.forestPlan(n0, ny, nlit, max_boxes, corner, nroot)
        return
    plan = na.frontend.forestPlan(n0, ny, nlit, max_boxes, corner, nroot)
    g = plan["group"]
    assert 1 <= g <= nroot
    assert (plan["level_capacity"], plan["frontier_bytes"], plan["point_log_bytes"], plan["record_bytes"]) == sizes(g)
    assert max(sizes(g)[1:]) <= CAP and plan["level_capacity"] <= 2 ** 26
    assert g == nroot or max(sizes(g + 1)[1:]) > CAP or sizes(g + 1)[0] > 2 ** 26          # and no larger group would fit
    forced = na.frontend.forestPlan(n0, ny, nlit, max_boxes, corner, nroot, group=3)
    assert forced["group"] == min(3, g)
    assert na.frontend.forestPlan(n0, ny, nlit, max_boxes, corner, 2)["group"] == min(2, g)


def test_the_plan_refuses_with_the_byte_count_as_search_does():
    with pytest.raises(_lib.NnsdpError, match=r"max_boxes = 8388608 needs \d+ bytes of frontier buffers for one root, above the cap of 2\^31"):
        na.frontend.forestPlan(5, 5, 1, 2 ** 23, False, 4)
