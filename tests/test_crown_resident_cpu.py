"""The resident CROWN bounder without a GPU: the refusals of nnsdp_crown_create (all made before the GPU is touched), the option check
of the split driver, and the numpy restatement R_tanh (tests/crown_tanh_common.py) pinned to the float32 host routine and to sampled
forward passes before any GPU is involved."""
import ctypes as C

import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import _lib
import crown_tanh_common as tc
import literal_common as lc


def _create(xdims, M, activ, nlit=0, normals=None):
    lib = _lib.load()
    xd = np.asarray(xdims, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)
    h = C.c_void_p()
    rc = lib.nnsdp_crown_create(len(xdims) - 1, xd.ctypes.data_as(_lib.c_int32_p), p(M), activ, nlit, p(normals), C.byref(h))
    assert h.value is None or rc == 0
    if h.value is not None:                      # (a GPU is present and the arguments were good: not what these tests look at)
        lib.nnsdp_crown_destroy(h)
    return rc, lib.nnsdp_last_error().decode()


def test_create_refuses_bad_arguments_before_the_gpu():
    M3 = np.zeros(3 * 3 + 2 * 4)                      # a 2-3-2 network: [W0 b0] 3 x 3, [W1 b1] 2 x 4
    rc, msg = _create([2, 3, 2], None, 0)
    assert rc == -1 and "network" in msg
    rc, msg = _create([2, 3], np.zeros(9), 0)
    assert rc == -1 and "K >= 2" in msg
    rc, msg = _create([2, 65, 2], np.zeros(65 * 3 + 2 * 66), 1)
    assert rc == -1 and "65" in msg and "64" in msg
    for widths in ([2, 0, 2], [0, 65, 2]):             # an empty layer; the first bad width is the one named
        rc, msg = _create(widths, M3, 0)
        assert rc == -1 and "layer widths must be >= 1" in msg
    rc, msg = _create([2, 3, 2], M3, 7)
    assert rc == -1 and "activation" in msg
    rc, msg = _create([2, 3, 2], M3, 1, 65, np.zeros((65, 2)))
    assert rc == -1 and "nlit" in msg and "65" in msg
    rc, msg = _create([2, 3, 2], M3, 1, 2, None)
    assert rc == -1 and "normals" in msg and "null" in msg
    nrm = np.ones((3, 2))
    nrm[2, 1] = np.nan
    rc, msg = _create([2, 3, 2], M3, 0, 3, nrm)
    assert rc == -1 and "literal 2" in msg and "NaN" in msg


def test_destroy_of_null_is_a_no_op():
    assert _lib.load().nnsdp_crown_destroy(None) == 0


def test_split_option_accepts_resident_and_still_refuses_others(monkeypatch):
    net = lc.random_net([2, 3, 2], 1)
    lits = [(np.array([1.0, 0.0]), 0.0)]
    seen = []

    class Stop(Exception):
        pass

    def fake(net_, normals=None):
        seen.append(normals)
        raise Stop

    monkeypatch.setattr(na.frontend, "CrownBounder", fake)      # past the option check the driver asks for its bounder
    with pytest.raises(Stop):
        na.verifySplit(net, [0.0, 0.0], [1.0, 1.0], lits, 0, na.AdmmSdpOptions(), na.SplitOptions(crown_backend="resident", sdp_per_level=0))
    assert seen == [None]
    with pytest.raises(Stop):
        na.verifySplit(net, [0.0, 0.0], [1.0, 1.0], lits, 0, na.AdmmSdpOptions(),
                       na.SplitOptions(crown_backend="resident", sdp_per_level=0, corner_points=True))
    assert seen[1].shape == (1, 2)
    with pytest.raises(ValueError, match="crown_backend"):
        na.verifySplit(net, [0.0, 0.0], [1.0, 1.0], lits, 0, na.AdmmSdpOptions(), na.SplitOptions(crown_backend="cpu", sdp_per_level=0))


def test_the_restatement_agrees_with_the_float32_host_routine():
    """max |R_tanh(float64) - host| / (1 + |v|) over the ten arrays (six intervals, four literal outputs) of 64 boxes each of the Tanh
    W10-D5 fixture and a Tanh 5-50-50-50-5 net, with and without normals: positive (the host is float32) and below 1e-4."""
    worst = 0.0
    for cs in tc.sound_tanh():
        for nm, h, r in zip(lc.NAMES + lc.LIT_NAMES, cs["host"], cs["r64"]):
            assert h.shape == r.shape, nm
            f = tc.rel_err(h, r)
            worst = max(worst, f)
            print(f"{cs['net'].xdims} {nm}: max |R_tanh(float64) - host| / (1 + |v|) = {f:.3e}")
        plain = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="host")
        for nm, h, r in zip(lc.NAMES, plain, tc.R_tanh(cs["net"].Ms, cs["lo"], cs["hi"], np.float64)):
            f = tc.rel_err(h, r)
            worst = max(worst, f)
            print(f"{cs['net'].xdims} {nm} (no normals): {f:.3e}")
    print(f"largest figure {worst:.3e};  host_figure() = {tc.host_figure():.3e}")
    assert 0.0 < worst < 1e-4
    assert 0.0 < tc.host_figure() <= worst


def test_the_restatement_is_sound_on_sampled_points():
    for cs in tc.sound_tanh():
        acymin, acymax, _, _, ymin, ymax, smin, smax, A, b0 = cs["r64"]
        tc.assert_hidden_and_output_sound(cs["net"], cs["lo"], cs["hi"], acymin, acymax, ymin, ymax)
        lc.assert_literals_sound(cs["net"], cs["lo"], cs["hi"], cs["C"], na.LiteralBounds(smin, smax, A, b0), 1e-9)
