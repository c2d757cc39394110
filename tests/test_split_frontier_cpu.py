"""frontier = "device" of the split driver without a GPU: the option check of verifySplit and the refusals of nnsdp_crown_search that
need no handle (all made before the GPU is touched; those that need one are in tests/test_split_frontier_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import literal_common as lc


def _verify(**kw):
    net = lc.random_net([2, 3, 2], 1)
    return na.verifySplit(net, [0.0, 0.0], [1.0, 1.0], [(np.array([1.0, 0.0]), 0.0)], 0, na.AdmmSdpOptions(), na.SplitOptions(sdp_per_level=0, **kw))


def test_the_default_frontier_is_the_host():
    assert na.SplitOptions().frontier == "host" and na.SplitOptions().chunk == 4096


@pytest.mark.parametrize("options,field", [(dict(crown_backend="host"), "crown_backend"), (dict(crown_backend="gpu"), "crown_backend"),
                                           (dict(crown_backend="resident", samples=2), "samples"),
                                           (dict(crown_backend="resident", literal_bounds=True, alpha_steps=3), "alpha_steps")])
def test_the_device_frontier_names_the_option_it_cannot_take(options, field):
    with pytest.raises(ValueError, match=field):
        _verify(frontier="device", **options)


def test_an_unknown_frontier_is_refused():
    with pytest.raises(ValueError, match="frontier"):
        _verify(frontier="gpu")


def test_the_device_frontier_asks_for_its_bounder_past_the_option_check(monkeypatch):
    class Stop(Exception):
        pass

    def fake(net_, normals=None):
        raise Stop

    monkeypatch.setattr(na.frontend, "CrownBounder", fake)
    with pytest.raises(Stop):
        _verify(frontier="device", crown_backend="resident")


def _search(h=None, max_boxes=8, max_depth=4, chunk=4):
    lib = _lib.load()
    dp, ip = _lib.c_double_p, _lib.c_int32_p
    lo, hi, nrm, hs, wit = np.zeros(2), np.ones(2), np.array([1.0, 0.0]), np.zeros(1), np.zeros(2)
    out = (C.c_int32 * 4)()
    rc = lib.nnsdp_crown_search(h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 1, nrm.ctypes.data_as(dp), hs.ctypes.data_as(dp), 0, 0,
                                max_boxes, max_depth, chunk, None, None, *[C.cast(C.byref(out, 4 * k), ip) for k in range(4)],
                                wit.ctypes.data_as(dp), None)
    return rc, lib.nnsdp_last_error().decode()


def test_search_refuses_bad_arguments_before_the_gpu():
    rc, msg = _search(max_boxes=0)
    assert rc == -1 and "max_boxes" in msg and "0" in msg
    rc, msg = _search(chunk=0)
    assert rc == -1 and "chunk" in msg
    rc, msg = _search(max_depth=-1)
    assert rc == -1 and "max_depth" in msg
    rc, msg = _search()
    assert rc == -1 and "null handle" in msg
    lib = _lib.load()
    assert lib.nnsdp_crown_search_leaves(None, None, None, None, None, None, None) == -1 and "null handle" in lib.nnsdp_last_error().decode()
