"""The device-resident node frontier of the ReLU split without a GPU: the options of ReluSplitOptions (frontier, chunk) and the
refusals of nnsdp_crown_search_nodes that come before the handle is used."""
import numpy as np
import pytest

import nnsdp_amd as na
import relu_split_common as rs
from nnsdp_amd import _lib


def test_the_defaults_are_the_host_loop():
    opt = na.ReluSplitOptions()
    assert (opt.frontier, opt.chunk, opt.crown_backend) == ("host", 4096, "host")


def test_the_options_are_refused_before_any_library_call():
    net, lo, hi, _, _ = rs.toy()
    lit = [(np.array([1.0]), 2.5)]          # the toy's output is relu(x + 1) <= 2 on [-1, 1]
    for kw, word in ((dict(frontier="gpu"), "frontier must be"), (dict(frontier="device"), "needs crown_backend 'resident'"),
                     (dict(frontier="device", crown_backend="host"), "needs crown_backend 'resident'"),
                     (dict(chunk=0), "chunk"), (dict(frontier="device", crown_backend="resident", chunk=-3), "chunk")):
        with pytest.raises(ValueError, match=word):
            na.verifyReluSplit(net, lo[:, 0], hi[:, 0], lit, na.ReluSplitOptions(**kw))
    # the host loop still runs with the new fields at their defaults and with a chunk it never reads
    res = na.verifyReluSplit(net, lo[:, 0], hi[:, 0], lit, na.ReluSplitOptions(chunk=7))
    assert res.verdict == "holds" and "kernel" not in res.seconds


def _raw(steps=16, eta0=0.5, decay=0.9, max_nodes=64, max_depth=8, chunk=16):
    lib = _lib.load()
    rc = lib.nnsdp_crown_search_nodes(None, None, None, 1, None, steps, eta0, decay, 1, max_nodes, max_depth, chunk, None, None,
                                      *([None] * 8))
    return rc, lib.nnsdp_last_error().decode()


def test_the_scalar_options_come_before_the_null_handle():
    for kw, word in ((dict(max_nodes=0), "max_nodes"), (dict(chunk=0), "chunk"), (dict(max_depth=-1), "max_depth"), (dict(steps=65), "steps"),
                     (dict(steps=-1), "steps"), (dict(eta0=0.0), "eta0"), (dict(decay=1.5), "decay"), ({}, "null handle")):
        rc, msg = _raw(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # the budget's message names max_nodes, not the bisection searches' max_boxes
    assert "max_boxes" not in _raw(max_nodes=0)[1]
    lib = _lib.load()
    assert lib.nnsdp_crown_search_nodes_leaves(None, None, None, None, None) == -1 and "null handle" in lib.nnsdp_last_error().decode()
