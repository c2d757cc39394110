"""Bounds of literals  normal' f(x)  from the host routine (nnsdp_make_intervals_lits, csrc/intervals.hpp; makeIntervalsBatch with
normals, backend="host") against the numpy restatement R of literal_common with a head.  The host routine is float32 by design."""
import numpy as np

import nnsdp_amd as na
from literal_common import R, assert_literals_sound, literal_rows, random_net, sound_nets

# max |host - R(float64)| / (1 + |v|) over the literal outputs of the sound_nets boxes, as measured when this test was written; beside
# it the figure of the six interval arrays recorded in tests/test_crown_batch_gpu.py
HOST_FLOAT32_FIGURE = 3.14e-7
HOST_FLOAT32_LITERAL_FIGURE = 4.07e-7
# soundness slack, relative to 1 + |v|: the host bounds carry the float32 error of the figure above (a few 1e-7), so a sampled value may
# pass a bound by that much; 1e-5 covers the figure more than ten times over
SLACK = 1e-5
_cache = {}


def host_cases():
    if "host" not in _cache:
        out = []
        for cs in sound_nets():
            *six, lits = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="host", normals=cs["C"])
            out.append(dict(cs, six=six, lits=lits, r64=R(cs["net"].Ms, cs["lo"], cs["hi"], np.float64, head=cs["C"])))
        _cache["host"] = out
    return _cache["host"]


def test_host_literals_agree_with_the_recurrences_to_float32():
    rel = lambda a, ref: float((np.abs(a - ref) / (1.0 + np.abs(ref))).max())
    figure = max(rel(h, r) for cs in host_cases() for h, r in zip(cs["lits"], cs["r64"][6:]))
    print(f"max |host - R(float64)| / (1 + |v|) over smin, smax, A, b0 = {figure:.3e} (recorded {HOST_FLOAT32_LITERAL_FIGURE:.3e}; "
          f"the six interval arrays: {HOST_FLOAT32_FIGURE:.3e})")
    assert 0.0 < figure < 1e-4, "the host routine is float32: the figure is of float32 size"
    assert figure <= SLACK, "the soundness slack must cover the float32 figure"
    for cs in host_cases():
        n0, nbox, nlit = cs["net"].xdims[0], cs["lo"].shape[1], len(cs["C"])
        assert cs["lits"].smin.shape == cs["lits"].smax.shape == cs["lits"].b0.shape == (nlit, nbox) and cs["lits"].A.shape == (nlit, n0, nbox)


def test_host_literals_are_sound_on_sampled_points():
    for cs in host_cases():
        assert_literals_sound(cs["net"], cs["lo"], cs["hi"], cs["C"], cs["lits"], SLACK)


def test_smax_is_the_linear_bound_over_the_box():
    """smax = A c + |A| r + b0 to float32 level, and the zero row gives exact zeros"""
    for cs in host_cases():
        L = cs["lits"]
        c, r = 0.5 * (cs["hi"] + cs["lo"]), 0.5 * (cs["hi"] - cs["lo"])
        re = np.einsum("iqb,qb->ib", L.A, c) + np.einsum("iqb,qb->ib", np.abs(L.A), r) + L.b0
        assert np.all(np.abs(re - L.smax) <= 1e-4 * (1.0 + np.abs(L.smax)))
        assert not L.smin[3].any() and not L.smax[3].any() and not L.b0[3].any() and not L.A[3].any()


def test_tanh_and_wide_nets_on_the_host():
    base = random_net([2, 8, 8, 2], 41)
    tanh = na.FeedFwdNet(xdims=base.xdims, Ms=base.Ms, activ=na.methods.TanhActiv)
    wide = random_net([2, 65, 2], 42)
    rng = np.random.default_rng(43)
    c = rng.normal(size=(2, 12))
    hw = np.array([0.0, 1e-3, 0.1, 0.5])[rng.integers(0, 4, size=(2, 12))]
    lo, hi = c - hw, c + hw
    C = literal_rows(2, 6, 44)
    for net in (tanh, wide):
        *six, lits = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=C)
        assert all(np.all(np.isfinite(a)) for a in lits)
        assert_literals_sound(net, lo, hi, C, lits, SLACK)
        assert np.all(lits.smin <= lits.smax + SLACK * (1.0 + np.abs(lits.smax)))


def test_the_six_arrays_keep_their_bits():
    for cs in host_cases():
        plain = na.makeIntervalsBatch(cs["net"], cs["lo"], cs["hi"], backend="host")
        assert len(plain) == 6 and all(np.array_equal(a, b) for a, b in zip(plain, cs["six"]))
    cs = host_cases()[0]
    *six, lits, ms = na.makeIntervalsBatch(cs["net"], cs["lo"][:, :3], cs["hi"][:, :3], backend="host", normals=cs["C"], return_ms=True, workers=1)
    assert isinstance(lits, na.LiteralBounds) and isinstance(ms, float)
    assert all(np.array_equal(a, b[..., :3]) for a, b in zip(lits, cs["lits"]))
