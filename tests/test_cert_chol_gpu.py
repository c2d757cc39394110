"""The sparse NSD check on the GPU (nnsdp_sparse_nsd: csrc/cert_plan.hpp + csrc/cert_chol.hpp; run with -m gpu on an MI355X): a
multifrontal Cholesky of -M on the clique pattern, one workgroup per candidate, against numpy's dense fp64 Cholesky.

Test matrices: M = -(sum_k E_k' G_k G_k' E_k + eps I) with thin random G_k (the sum is rank-deficient, so eps alone sets the smallest
eigenvalue) and eps chosen for kappa_2(-M_xx) = 1e2, 1e6, 1e10 exactly (from the eigenvalues of the sum).

Tolerance of the Schur complement: the backward error of a Cholesky solve is bounded by c n u kappa_2 relative to the terms that make
up the result, |M_aa| + z' (-M_xx)^-1 z; numpy's own reference carries an error of the same order, hence 50 n 2^-52 kappa_2."""
import numpy as np
import pytest
import scipy.linalg as sla

import nnsdp_amd as na
from nnsdp_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
W10 = [2] + [10] * 5 + [2]
PATTERNS = {
    "w10_b0_single": (W10, 0, na.SingleDecomp),
    "w10_b0_double": (W10, 0, na.DoubleDecomp),
    "w10_b3_single": (W10, 3, na.SingleDecomp),
    "w10_b3_double": (W10, 3, na.DoubleDecomp),
    "odd_widths_b2": ([3, 7, 9, 8, 6, 7, 2], 2, na.SingleDecomp),
    "exact_tiles": ([2, 16, 16, 16, 2], 0, na.SingleDecomp),
    "front_128": ([2, 40, 40, 40, 40, 2], 7, na.SingleDecomp),
    "front_102_path": ([5, 50, 50, 50, 5], 1, na.PathDecomp),
    "one_clique": ([2, 12, 2], 0, na.SingleDecomp),
    "dense_53": None,
    "forest": None,
}
_cache = {}


def pattern(name):
    if name == "dense_53":
        return 53, [list(range(53))]
    if name == "forest":
        return 5, [[0, 1, 4], [2, 3, 4]]
    xdims, beta, mode = PATTERNS[name]
    return sum(xdims[:-1]) + 1, na.makeCliques(xdims, beta, mode())


def base(name):
    """(n, cliques, S, lam): S = sum_k E_k' G_k G_k' E_k (PSD, rank-deficient), lam = eigenvalues of S_xx; computed once per pattern"""
    if name not in _cache:
        n, cl = pattern(name)
        rng = np.random.default_rng(sum(map(ord, name)))
        S = np.zeros((n, n))
        for c in cl:
            G = rng.standard_normal((len(c), 1 if len(c) <= 4 else 2))
            S[np.ix_(c, c)] += G @ G.T
        lam = np.linalg.eigvalsh(S[:-1, :-1])
        assert lam[0] <= 1e-12 * lam[-1], "the sum of thin Gram matrices is expected to be rank-deficient"
        _cache[name] = (n, cl, S, lam)
    return _cache[name]


def matrix(name, kappa):
    """M with kappa_2(-M_xx) = kappa, and the smallest eigenvalue of -M_xx"""
    n, cl, S, lam = base(name)
    eps = lam[-1] / (kappa - 1.0)        # (lam_max + eps) / (0 + eps) = kappa
    return -(S + eps * np.eye(n)), eps + max(lam[0], 0.0)


def reference(M):
    n = M.shape[0]
    L = np.linalg.cholesky(-M[:-1, :-1])
    y = sla.solve_triangular(L, M[:-1, -1], lower=True)
    q = float(y @ y)
    return M[-1, -1] + q, abs(M[-1, -1]) + q


@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_schur_complement_matches_numpy(name, kappa):
    n, cl, _, _ = base(name)
    M, _ = matrix(name, kappa)
    ok, minp, schur, ms = na.sparse_nsd(n, cl, [M])
    ref, mag = reference(M)
    tol = 50 * n * U * kappa * mag
    print(f"{name} kappa {kappa:.0e}: n {n} ok {ok[0]} min pivot {minp[0]:.3e} schur {schur[0]:.12e} ref {ref:.12e} "
          f"err {abs(schur[0] - ref):.2e} tol {tol:.2e} kernel {ms:.3f} ms")
    assert ok[0] == 1
    assert minp[0] > 0
    assert abs(schur[0] - ref) <= tol


@pytest.mark.parametrize("kappa", [1e2, 1e6])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_decisions_at_the_boundary(name, kappa):
    n, cl, _, _ = base(name)
    M, lmin = matrix(name, kappa)
    Ixx = np.eye(n)
    Ixx[-1, -1] = 0.0
    inside, outside = M + (1 - 1e-3) * lmin * Ixx, M + (1 + 1e-3) * lmin * Ixx
    ok, minp, schur, _ = na.sparse_nsd(n, cl, [inside, outside])
    print(f"{name} kappa {kappa:.0e}: ok {ok.tolist()} min pivots {minp.tolist()} failing column {schur[1]}")
    assert ok[0] == 1 and minp[0] > 0
    assert ok[1] == 0
    assert schur[1] == int(schur[1]) and 0 <= schur[1] < n - 1, "a failing column is reported"


@pytest.mark.parametrize("name", ["w10_b3_double", "front_128", "forest"])
def test_bits_do_not_depend_on_batch_size_or_position(name):
    n, cl, _, _ = base(name)
    M2, l2 = matrix(name, 1e2)
    M6, _ = matrix(name, 1e6)
    M10, _ = matrix(name, 1e10)
    Ixx = np.eye(n)
    Ixx[-1, -1] = 0.0
    pool = [M2, M6, M10, M2 + 1.001 * l2 * Ixx, M2 + 0.5 * l2 * Ixx]      # (the fourth one fails)
    seen = {}
    for size in (1, 3, 65):
        which = [(3 * size + 2 * j) % len(pool) for j in range(size)]
        ok, minp, schur, _ = na.sparse_nsd(n, cl, [pool[w] for w in which])
        for j, w in enumerate(which):
            bits = (int(ok[j]), minp[j].tobytes(), schur[j].tobytes())
            assert seen.setdefault(w, bits) == bits, (size, j, w)
    assert len(seen) == len(pool)
    assert [seen[w][0] for w in range(len(pool))] == [1, 1, 1, 0, 1]


def test_entry_outside_the_pattern_is_refused():
    n, cl, _, _ = base("w10_b0_single")
    M, _ = matrix("w10_b0_single", 1e2)
    inpat = np.zeros((n, n), dtype=bool)
    for c in cl:
        inpat[np.ix_(c, c)] = True
    i, j = np.argwhere(~inpat)[0]
    M = M.copy()
    M[i, j] = M[j, i] = 0.5
    with pytest.raises(_lib.NnsdpError) as e:
        na.sparse_nsd(n, cl, [M])
    assert e.value.code == -1


def test_front_above_the_limit_is_refused_before_any_launch():
    xdims = [5] + [50] * 6 + [5]
    n = sum(xdims[:-1]) + 1
    cl = na.makeCliques(xdims, 1, na.SingleDecomp())
    with pytest.raises(_lib.NnsdpError) as e:
        na.sparse_nsd(n, cl, [-np.eye(n)])
    assert e.value.code == -2 and "152" in str(e.value)
