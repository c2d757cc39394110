"""Shared by the tests of the wide resident CROWN bounder (test_crown_wide_*.py): the nets at which the slab, tile and k-tail indexing
of csrc/crown_wide.hpp can go wrong, their boxes and literal rows, the numpy recurrences of all ten arrays in float64 and longdouble
(computed once per net, on 6 boxes and 64 literal rows, and cut by the tests: row i of literal_rows does not depend on nlit), the
float32 host routine's result on them, and the two split instances.  Nothing here needs a GPU."""
import numpy as np

import crown_tanh_common as tc
import literal_common as lc
import nnsdp_amd as na

NBOX, NLIT = 6, 64
# narrow with one slab; a second slab of one row, a second column tile of one column and a k tail of one; 127; slabs and tiles that
# change from layer to layer; everything full
SHAPES = {"3-64-64-3": [3, 64, 64, 3], "2-65-2": [2, 65, 2], "4-127-4": [4, 127, 4], "3-65-128-66-4": [3, 65, 128, 66, 4],
          "5-128x3-5": [5, 128, 128, 128, 5]}
WIDE = ("2-65-2", "4-127-4", "3-65-128-66-4", "5-128x3-5")
TANH = ("4-127-4", "3-65-128-66-4")
DEVICE_ULPS = 1.0      # as in tests/test_crown_resident_gpu.py: the device library's tanh / cosh stay within 1 ulp
# max |R(float64) - host| / (1 + |v|) over the ten arrays of the four WIDE ReLU nets as it was when these tests were written
# (test_crown_wide_cpu.py measures it again); the narrow nets' figure is 3.1e-7
HOST_FLOAT32_FIGURE_WIDE = 4.37e-7
_cache = {}


def seed_of(name):
    return sum(map(ord, name))


def case(name, activ="relu"):
    """net, lo, hi (6 boxes: the point box, half-widths 1e-6, 0.05, 0.5, 3, one mixed), C (64 rows), r64 / rld (the ten arrays of the
    numpy recurrences in float64 / longdouble; Tanh: also rmv, float64 with tanh and cosh moved by DEVICE_ULPS): computed once, shared,
    never modified"""
    key = (name, activ)
    if key not in _cache:
        net = lc.random_net(SHAPES[name], seed_of(name))
        lo, hi = lc.boxes(net.xdims[0], NBOX, seed_of(name) + 1)
        Cm = lc.literal_rows(net.xdims[-1], NLIT, seed_of(name) + 2)
        cs = dict(lo=lo, hi=hi, C=Cm)
        if activ == "tanh":
            net = tc.tanh_copy(net)
            cs.update(r64=tc.R_tanh(net.Ms, lo, hi, np.float64, Cm), rld=tc.R_tanh(net.Ms, lo, hi, np.longdouble, Cm),
                      rmv=tc.R_tanh(net.Ms, lo, hi, np.float64, Cm, lib=tc.Moved(DEVICE_ULPS, seed=seed_of(name))))
        else:
            cs.update(r64=lc.R(net.Ms, lo, hi, np.float64, Cm), rld=lc.R(net.Ms, lo, hi, np.longdouble, Cm))
        cs["net"] = net
        _cache[key] = cs
    return _cache[key]


def cut(arrays, nbox, nlit):
    """the ten arrays of `case` as a call with the first nbox boxes and the first nlit literal rows returns them (nlit = 0: six)"""
    six = tuple(a[..., :nbox] for a in arrays[:6])
    return six + tuple(a[:nlit, ..., :nbox] for a in arrays[6:]) if nlit > 0 else six


def host(name):
    """the float32 host routine's ten arrays on the case's boxes with 7 literal rows"""
    key = ("host", name)
    if key not in _cache:
        cs = case(name)
        _cache[key] = tc.flat(na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="host", normals=cs["C"][:7]))
    return _cache[key]


def host_figure():
    """max |R(float64) - host| / (1 + |v|) over the ten arrays of the WIDE nets: measured without the kernel"""
    return max(tc.rel_err(h, r) for name in WIDE for h, r in zip(host(name), cut(case(name)["r64"], NBOX, 7)))


# the two split instances: on [-1, 1]^n0, one literal, max_boxes 512
INSTANCES = {"3-80-70-3": ([3, 80, 70, 3], 5, np.array([1.0, 0.0, -1.0])), "2-100-100-2": ([2, 100, 100, 2], 6, np.array([1.0, -1.0]))}
# the thresholds between the sampled maximum s and the root's per-output bound c0, and the verdict of each (an fp64 emulation with
# literal bounds and centre points visits 13 / 35 / 229 boxes on the first instance and 7 / 11 / 83 on the second)
THRESHOLDS = {"quarter": (lambda s, c0: s + 0.25 * (c0 - s), "holds"), "tenth": (lambda s, c0: s + 0.1 * (c0 - s), "holds"),
              "below": (lambda s, c0: s - 0.1 * abs(s), "violated")}


def instance(name):
    """as literal_common.instance: net, box, normal, s = the literal's maximum over lo + default_rng(0).random((n0, 20000)) * (hi - lo),
    c0 = the root's per-output bound (the host routine takes any width)"""
    key = ("instance", name)
    if key not in _cache:
        xdims, seed, nrm = INSTANCES[name]
        net = lc.random_net(xdims, seed)
        n0 = xdims[0]
        lo, hi = -np.ones(n0), np.ones(n0)
        X = lo[:, None] + np.random.default_rng(0).random((n0, 20000)) * (hi - lo)[:, None]
        s = float((nrm @ lc.forward(net, X)).max())
        iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="host")
        c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
        assert c0 > s
        _cache[key] = dict(net=net, lo=lo, hi=hi, normal=nrm, s=s, c0=c0)
    return _cache[key]
