"""Several helper workgroups per block for the warm-start congruence (ProjArgs::split = H, csrc/split_deal.hpp): every tile keeps its
own chain, so W, V and the outcome words must be the bits of the one-workgroup launch - for single sizes of 3, 4 and 6 tile columns,
for one launch that mixes sizes (ids past the last block in every helper band, helpers without a share), and through a solver's
launches (counters carried across launches, visits with and without the Gram product, replayed graphs)."""
import hashlib

import numpy as np
import pytest

import helpers
import nnsdp_amd as na

pytestmark = pytest.mark.gpu

SETTINGS = ((1e-6, 3e-7, True), (0.0, 1e-7, True), (3e-2, 1e-6, True), (1e-6, 3e-7, False))      # a step, a converged block, sweeps, the stage off


def _sym(rng, n):
    spec = np.concatenate([np.linspace(0.2, 2.0, n - n // 3), -np.linspace(0.1, 1.5, n // 3)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * spec) @ Q.T, Q


def _same_bits_for_every_helper_count(rng, base, counts, monkeypatch):
    for eta, tol, refine in SETTINGS:
        mats = []
        for A, _ in base:
            D = rng.standard_normal(A.shape); D = 0.5 * (D + D.T)
            mats.append(A + eta * np.linalg.norm(A) / np.linalg.norm(D) * D)
        out = {}
        for H in ("0",) + counts:
            monkeypatch.setenv("NNSDP_SPLIT_WARM", H)
            out[H] = na.project_psd_warm(mats, [Q for _, Q in base], tol, refine=refine)
        for H in counts:
            for a, b in zip(out["0"][0] + out["0"][1], out[H][0] + out[H][1]):
                assert np.array_equal(a, b), (H, eta, refine)
            assert list(out["0"][2]) == list(out[H][2]), (H, eta, refine)


@pytest.mark.parametrize("n", [41, 57, 85, 96])
def test_helper_counts_give_identical_bits(n, monkeypatch):
    """batches of 7 blocks of one size (3, 4, 6 and 6 tile columns); 7 helpers are clamped to the columns there are"""
    rng = np.random.default_rng(n)
    _same_bits_for_every_helper_count(rng, [_sym(rng, n) for _ in range(7)], ("2", "3", "5", "7"), monkeypatch)


def test_mixed_launch_gives_identical_bits(monkeypatch):
    """9 blocks of 3 to 6 tile columns in one launch: bands of 16 ids with 7 past the last block each, helpers 3 .. 5 of the small blocks
    without a share"""
    rng = np.random.default_rng(9)
    _same_bits_for_every_helper_count(rng, [_sym(rng, n) for n in (96, 41, 85, 57, 64, 80, 48, 85, 96)], ("3", "5"), monkeypatch)


def test_solver_iterates_do_not_depend_on_the_helper_count(monkeypatch):
    """W40-D20 Single (19 blocks up to 85): 1 500 iterations of the solve loop, then 64 plain ones, leave the same multiplier bits and
    residuals with 0, 3 and 5 helpers per block"""
    q = helpers.product_query(helpers.load_problem("W40-D20", 0))
    dig = []
    for H in ("0", "3", "5"):
        monkeypatch.setenv("NNSDP_SPLIT", H)
        s = na.Solver(q, na.AdmmSdpOptions(decomp_mode=na.SingleDecomp(), max_iters=10 ** 9))
        s.advance(1500)
        s.iterate(64)
        res = s.residuals()
        dig.append((hashlib.sha256(s.raw_multipliers().tobytes()).hexdigest(), res))
        s.close()
    assert dig[0] == dig[1] == dig[2]
