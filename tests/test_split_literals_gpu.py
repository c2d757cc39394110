"""The split driver's literal options on the GPU: the literal pass of csrc/crown_batch.hpp in the bound step, the corners through
nnsdp_eval_network in the refutation step.  The two instances of tests/test_split_literals_cpu.py with crown_backend="gpu", and the
W10-D5 instance of tests/test_split_gpu.py with the SDP stage."""
import numpy as np
import pytest

import nnsdp_amd as na
from nnsdp_amd import vnnlib as vl
from literal_common import assert_tiles, forward, instance
from test_split_cpu import HI, LO, NORMAL, net, setting

pytestmark = pytest.mark.gpu
OPTS = na.AdmmSdpOptions(max_iters=20000, eps_rel=1e-5)
BOTH = dict(crown_backend="gpu", literal_bounds=True, corner_points=True)


def test_holds_with_both_options():
    """net 3-17-33-4 seed 14: "holds" within half the boxes of the plain run (the host runs: 15 against 59)"""
    it = instance("holds", "gpu")
    lit = [(it["normal"], it["h"])]
    plain = na.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=0))
    res = na.verifySplit(it["net"], it["lo"], it["hi"], lit, 0, OPTS, na.SplitOptions(sdp_per_level=0, **BOTH))
    print(f"h {it['h']:.8f}: visited plain {plain.visited}, both options {res.visited}; seconds {res.seconds}")
    assert plain.verdict == "holds" and res.verdict == "holds" and res.witness is None
    assert_tiles(res.leaves, it["lo"], it["hi"])
    assert res.visited < plain.visited and 2 * res.visited <= plain.visited
    rng = np.random.default_rng(7)
    for lf in res.leaves:
        assert lf.proved_by == "crown" and lf.literal == 0 and lf.bound <= it["h"]
        X = lf.lo[:, None] + rng.random((3, 2000)) * (lf.hi - lf.lo)[:, None]
        assert np.all(it["normal"] @ forward(it["net"], X) <= lf.bound + 1e-9 * (1.0 + abs(lf.bound)))


def test_violated_with_both_options():
    """net 5-20-20-20-5 seed 31: "violated" at a corner within 64 boxes (the host run: 3), the witness confirmed by a numpy forward pass"""
    it = instance("violated", "gpu")
    res = na.verifySplit(it["net"], it["lo"], it["hi"], [(it["normal"], it["h"])], 0, OPTS, na.SplitOptions(sdp_per_level=0, **BOTH))
    print(f"h {it['h']:.8f}: {res.verdict} after {res.visited} boxes")
    assert res.verdict == "violated" and res.visited <= 64
    assert np.all(res.witness >= it["lo"]) and np.all(res.witness <= it["hi"])
    assert float(it["normal"] @ forward(it["net"], res.witness[:, None])[:, 0]) > it["h"]
    rng = np.random.default_rng(8)
    for lf in res.leaves:
        if lf.proved_by is not None:
            X = lf.lo[:, None] + rng.random((5, 2000)) * (lf.hi - lf.lo)[:, None]
            assert np.all(it["normal"] @ forward(it["net"], X) <= lf.bound + 1e-9 * (1.0 + abs(lf.bound)))


def test_sdp_stage_with_literal_bounds():
    s, c0 = setting()
    h = s + 0.25 * (c0 - s)
    res = na.verifySplit(net(), LO, HI, [(NORMAL, h)], 0, OPTS, na.SplitOptions(crown_backend="gpu", sdp_per_level=2, literal_bounds=True))
    by = [lf.proved_by for lf in res.leaves]
    print(f"visited {res.visited}, {res.sdp_solves} SDPs, leaves by crown {by.count('crown')} by sdp {by.count('sdp')}")
    assert res.verdict == "holds"
    assert_tiles(res.leaves, LO, HI)
    for lf in res.leaves:
        assert lf.proved_by in ("crown", "sdp") and lf.bound <= h
        if lf.proved_by == "sdp":
            assert vl.isSolutionGood(lf.soln)
