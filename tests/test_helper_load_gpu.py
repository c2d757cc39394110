"""The helper workgroups' own load (csrc/kernels.hip, proj_helper_load): a helper reads all of nu_k but of V_k only the tile columns
from its lowest owned one upwards, symmetrises flat over its threads, sums no norm, and reads its share of the deal from the launch's
arguments.  None of that may show in a result: H = 1, 3, 5 and 7 helpers per block against H = 0 of the same build, through the warm
test entry (NNSDP_SPLIT_WARM) - W, V, the outcome counts and the per-block state words bit for bit.

Anchors: n = 41 (odd n^2: the last 16-byte piece is moved back by one element; 3 tile columns), 48 (no padding at all), 57, 85, 96
(full tiles, even n^2).  Each runs alone and once in a launch with riders of 1 (first: the one-element piece), 15, 16, 17, 33 and 2
(last) - n = 17 and 33 give a helper whose lowest strip holds a single valid column.  H = 3 at six tile columns (85, 96) is the helper
with the non-adjacent columns {2, 5}."""
import numpy as np
import pytest

import helpers  # noqa: F401  (puts the package on the path)
import nnsdp_amd as na

pytestmark = pytest.mark.gpu

SETTINGS = ((1e-6, 3e-7, True), (0.0, 1e-7, True), (3e-2, 1e-6, True), (1e-6, 3e-7, False))      # a step, a converged block, sweeps, the stage off
COUNTS = ("1", "3", "5", "7")
ANCHORS = (41, 48, 57, 85, 96)
RIDERS_FRONT, RIDERS_BACK = (1, 15, 16, 17, 33), (2,)


def _sym(rng, n):
    spec = np.concatenate([np.linspace(0.2, 2.0, n - n // 3), -np.linspace(0.1, 1.5, n // 3)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * spec) @ Q.T, Q


def _check(sizes, seed, monkeypatch):
    rng = np.random.default_rng(seed)
    base = [_sym(rng, n) for n in sizes]
    for eta, tol, refine in SETTINGS:
        mats = []
        for A, _ in base:
            D = rng.standard_normal(A.shape); D = 0.5 * (D + D.T)
            mats.append(A + eta * np.linalg.norm(A) / max(np.linalg.norm(D), 1e-300) * D)
        out = {}
        for H in ("0",) + COUNTS:
            monkeypatch.setenv("NNSDP_SPLIT_WARM", H)
            state = np.zeros(4 * len(sizes), dtype=np.int32)
            W, V, oc, _ = na.project_psd_warm(mats, [Q for _, Q in base], tol, refine=refine, state=state)
            out[H] = (W, V, list(oc), state)
        W0, V0, oc0, st0 = out["0"]
        for H in COUNTS:
            W, V, oc, st = out[H]
            for b, n in enumerate(sizes):
                assert np.array_equal(W0[b], W[b]), ("W", H, eta, refine, b, n)
                assert np.array_equal(V0[b], V[b]), ("V", H, eta, refine, b, n)
            assert oc0 == oc, ("outcome", H, eta, refine)
            assert np.array_equal(st0, st), ("state", H, eta, refine)


@pytest.mark.parametrize("n", ANCHORS)
def test_anchor_alone(n, monkeypatch):
    _check((n,), n, monkeypatch)


@pytest.mark.parametrize("n", ANCHORS)
def test_anchor_among_riders(n, monkeypatch):
    _check(RIDERS_FRONT + (n,) + RIDERS_BACK, 1000 + n, monkeypatch)
