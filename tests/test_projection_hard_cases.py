"""The PSD projection (k_proj_jacobi, csrc/kernels.hip) on degenerate spectra in ragged launches, one test id per launch.

plan_projection picks the code path of a launch from its LARGEST block (the anchor); every other block of the launch - however
small - goes through that path.  Each launch here holds every hard family at the anchor size plus small riders (n = 1, 2, 3, 15, 16,
17, 33) with hard spectra of their own, a 1 x 1 block first and a 2 x 2 block last, through the public entries project_psd_batched
(cold) and project_psd_warm (the kernel as a solve runs it from its second iteration on).

Reference: oracle.admm.project_psd (numpy eigh), itself checked on the CPU against the projection each family is CONSTRUCTED with,
Q max(s, 0) Q' (test_reference_matches_the_constructed_projection: 1e-13 max|A|, three orders below what the GPU gets).
Tolerances: 1e-10 max|A| cold (K3, tests/test_gpu_parity.py), tol |A|_F warm, 30 tol |A|_F (+ 1e-12 on blocks of order one) with the
refinement stage on (include/nnsdp.h, proj_refine)."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import helpers  # noqa: F401
import nnsdp_amd as na
from oracle import admm as oadmm

RIDER_SIZES = (1, 2, 3, 15, 16, 17, 33)
RIDER_FAMILIES = ("zero", "minus_identity", "repeated", "clustered", "scaled_1e120", "gaussian")
SCALED = ("scaled_1e-150", "scaled_1e120")          # blocks far from order one: relative bounds only, no absolute floor

# (anchor, NNSDP_PROJ_ALG or None) of the cold launches through the LDS-resident kernel
COLD_LAUNCHES = [(a, None) for a in (40, 41, 74, 75, 90, 91, 97, 110, 111, 127, 128, 129, 144, 145, 160)] \
    + [(41, 0), (97, 0), (128, 0), (49, 2), (97, 4), (112, 4), (128, 4)]
LIBRARY_ANCHORS = (161, 203)
WARM_ANCHORS = (40, 85, 96, 101, 128, 151, 160)
ALL_SIZES = sorted(set(RIDER_SIZES) | {a for a, _ in COLD_LAUNCHES} | set(LIBRARY_ANCHORS) | set(WARM_ANCHORS))

Family = namedtuple("Family", "name A P Q")
Block = namedtuple("Block", "name n A ref ev Q Qrand Qnear")


def _sym(M):
    return 0.5 * (M + M.T)


def _psd_part_by_sign_iteration(A):
    """max(A, 0) = (A + sign(A) A) / 2 with the matrix sign function from the scaled Newton iteration X <- (mu X + (mu X)^-1) / 2:
    a projection of a matrix without a constructed spectrum that owes nothing to an eigensolver."""
    X = A.copy()
    for _ in range(60):
        Xi = np.linalg.inv(X)
        mu = np.sqrt(np.linalg.norm(Xi) / np.linalg.norm(X))
        Xn = _sym(0.5 * (mu * X + Xi / mu))
        done = np.linalg.norm(Xn - X) <= 1e-14 * np.linalg.norm(Xn)
        X = Xn
        if done:
            break
    return _sym(0.5 * (A + X @ A))


def families(n, rng):
    """The hard inputs at size n: for each family the matrix A and the projection it is constructed with, Q max(s, 0) Q' (Q from a QR
    of a Gaussian matrix), both symmetrised, and Q.  k = n // 3; below n = 3 the families that degenerate (k = 0) are dropped."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    k = n // 3
    i = np.arange(n, dtype=float)
    spectra = [("zero", np.zeros(n)), ("identity", np.ones(n)), ("minus_identity", -np.ones(n)),
               ("graded_definite", np.linspace(0.1, 3.0, n)), ("graded_negative", -np.linspace(0.1, 3.0, n)),
               ("rank_one", np.concatenate([[2.5], np.zeros(n - 1)]))]
    if k > 0:
        spectra.append(("repeated", np.repeat([2.0, -1.0, 0.0], [k, k, n - 2 * k])))
        spectra.append(("clustered", np.concatenate([1.0 + 1e-9 * np.arange(k), -1.0 - 1e-7 * np.arange(k), 1e-8 * (np.arange(n - 2 * k) - 3.0)])))
    spectra.append(("alternating_geometric", np.where(i % 2 == 0, 1.0, -1.0) * np.logspace(0.0, -12.0, n)))
    spectra.append(("scaled_1e-150", np.linspace(-1.0, 2.0, n) * 1e-150))
    spectra.append(("scaled_1e120", np.linspace(-1.0, 2.0, n) * 1e120))
    out = [Family(name, _sym((Q * s) @ Q.T), _sym((Q * np.maximum(s, 0.0)) @ Q.T), Q) for name, s in spectra]
    d = i - n / 2.0
    out.append(Family("diagonal_integers", np.diag(d), np.diag(np.maximum(d, 0.0)), np.eye(n)))
    G = _sym(rng.standard_normal((n, n)))
    out.append(Family("gaussian", G, _psd_part_by_sign_iteration(G), np.linalg.eigh(G)[1]))
    return out


@functools.lru_cache(maxsize=None)
def _blocks(n):
    """every family at size n with its reference and its starting bases, computed once and shared read-only by all tests"""
    rng = np.random.default_rng(7000 + n)
    out = []
    for f in families(n, rng):
        D = _sym(rng.standard_normal((n, n)))
        near = f.A + 1e-6 * np.linalg.norm(f.A) / np.linalg.norm(D) * D
        Qrand, _ = np.linalg.qr(rng.standard_normal((n, n)))
        b = Block(f.name, n, f.A, oadmm.project_psd(f.A), np.linalg.eigvalsh(f.A), f.Q, Qrand, np.linalg.eigh(near)[1])
        for arr in b[2:]:
            arr.setflags(write=False)
        out.append(b)
    return tuple(out)


def _riders(sizes, below):
    return [b for n in sizes if n < below for b in _blocks(n) if b.name in RIDER_FAMILIES]


def _launch(anchor, riders=True):
    """all families at the anchor size; riders of size 1 in front, of sizes 3 .. 33 behind, of size 2 last"""
    if not riders:
        return list(_blocks(anchor))
    return _riders((1,), anchor) + list(_blocks(anchor)) + _riders(RIDER_SIZES[2:], anchor) + _riders((2,), anchor)


def planned_variant(anchor, alg=None, warm_refine=False):
    """the instantiation plan_projection chooses for a launch whose largest block is `anchor` (csrc/kernels.hip)"""
    if anchor > 160:
        return "library path (rocSOLVER dsyevd + dgemm)"
    if anchor > 128 or (warm_refine and anchor > 96 and alg is None) or (alg == 4 and anchor > 96):
        return "packed triangle, 1024 threads, V in HBM"
    if alg is None:
        alg = 3 if 40 < anchor <= 96 else 2 if anchor > 96 else 0
    if alg == 3 and 40 < anchor <= 96:
        return "ping-pong, RPW %d" % (5 if anchor <= 74 else 6 if anchor <= 90 else 7)
    if alg == 2 and 49 <= anchor <= 128:
        return "systolic, 6 slots, V in LDS" if anchor <= 96 else "systolic, %d slots, V in HBM" % (7 if anchor <= 110 else 8)
    if anchor <= 40:
        return "round robin, 256 threads, V in LDS"
    return "round robin, 1024 threads, V in %s" % ("LDS" if anchor <= 96 else "HBM")


# ----------------------------------------------------------------------------- the reference itself (CPU)
def test_reference_matches_the_constructed_projection():
    """numpy's eigh-based projection against the projection every family is constructed with, at every size the GPU tests use"""
    worst = 0.0
    for n in ALL_SIZES:
        fams = families(n, np.random.default_rng(7000 + n))
        assert len(fams) == (13 if n >= 3 else 11)
        for f in fams:
            assert np.array_equal(f.A, f.A.T) and np.array_equal(f.P, f.P.T)
            err, scale = np.abs(oadmm.project_psd(f.A) - f.P).max(), np.abs(f.A).max()
            assert err <= 1e-13 * scale, (n, f.name, err, scale)
            if scale > 0.0:
                worst = max(worst, err / scale)
    print("reference against the constructed projections, sizes %s: worst error / max|A| = %.2e" % (ALL_SIZES, worst))


def test_every_path_of_the_plan_is_on_the_launch_list():
    cold = {planned_variant(a, alg) for a, alg in COLD_LAUNCHES} | {planned_variant(a) for a in LIBRARY_ANCHORS}
    warm = {planned_variant(a, None, r) for a in WARM_ANCHORS for r in (False, True)}
    want = {"round robin, 256 threads, V in LDS", "ping-pong, RPW 5", "ping-pong, RPW 6", "ping-pong, RPW 7", "systolic, 7 slots, V in HBM",
            "systolic, 8 slots, V in HBM", "packed triangle, 1024 threads, V in HBM", "library path (rocSOLVER dsyevd + dgemm)",
            "round robin, 1024 threads, V in LDS", "round robin, 1024 threads, V in HBM", "systolic, 6 slots, V in LDS"}
    assert cold == want
    assert warm == want - {"library path (rocSOLVER dsyevd + dgemm)", "round robin, 1024 threads, V in LDS", "round robin, 1024 threads, V in HBM",
                           "systolic, 6 slots, V in LDS", "ping-pong, RPW 5"}
    # a launch with riders: 1 x 1 first, 2 x 2 last, every rider size below the anchor, the anchor's own families complete
    blocks = _launch(160)
    assert blocks[0].n == 1 and blocks[-1].n == 2 and {b.n for b in blocks} == set(RIDER_SIZES) | {160}
    assert sum(b.n == 160 for b in blocks) == 13 and sum(b.n != 160 for b in blocks) == 38


# ----------------------------------------------------------------------------- cold leg
def _check_cold(blocks, label):
    mats = [b.A for b in blocks]
    P, evs, _ = na.project_psd_batched(mats)
    N, _, _ = na.project_psd_batched([-A for A in mats])
    worst = {"P": (0.0, ""), "ev": (0.0, ""), "sym": (0.0, ""), "moreau": (0.0, "")}
    bad = []

    def note(key, val, lim, b):
        if val > worst[key][0]:
            worst[key] = (val, "%s n=%d" % (b.name, b.n))
        if not val <= lim:
            bad.append((key, b.name, b.n, val, lim))

    for b, Pk, Nk, ev in zip(blocks, P, N, evs):
        nrm = max(np.abs(b.A).max(), 1e-300)
        if not (np.all(np.isfinite(Pk)) and np.all(np.isfinite(Nk)) and np.all(np.isfinite(ev))):
            bad.append(("finite", b.name, b.n, np.nan, 0.0))
            continue
        note("P", np.abs(Pk - b.ref).max() / nrm, 1e-10, b)
        note("ev", np.abs(np.sort(ev) - b.ev).max() / nrm, 1e-10, b)
        note("sym", np.abs(Pk - Pk.T).max() / nrm, 1e-11 if b.n > 160 else 1e-12, b)
        note("moreau", np.abs(Pk - Nk - b.A).max() / nrm, 1e-10, b)       # A = P(A) - P(-A): no oracle involved
        if b.name == "zero" and not (np.array_equal(Pk, np.zeros_like(Pk)) and np.array_equal(Nk, np.zeros_like(Nk))):
            bad.append(("zero block is not exactly zero", b.name, b.n, np.abs(Pk).max(), 0.0))
    print("[projection hard cases] cold %s: %d blocks; worst / max|A|: |P - ref| %.2e (%s), eigenvalues %.2e (%s), |P - P'| %.2e (%s), Moreau %.2e (%s)"
          % (label, len(blocks), *worst["P"], *worst["ev"], *worst["sym"], *worst["moreau"]))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("anchor,alg", COLD_LAUNCHES)
def test_cold_launch_of_hard_blocks_with_riders(anchor, alg, monkeypatch):
    """every family at the anchor size (the size that picks the instantiation) and the small riders in ONE launch"""
    if alg is None:
        monkeypatch.delenv("NNSDP_PROJ_ALG", raising=False)
    else:
        monkeypatch.setenv("NNSDP_PROJ_ALG", str(alg))
    _check_cold(_launch(anchor), "anchor %d, NNSDP_PROJ_ALG %s -> %s" % (anchor, alg, planned_variant(anchor, alg)))


@pytest.mark.gpu
@pytest.mark.parametrize("riders", [False, True], ids=["alone", "with_small_blocks"])
@pytest.mark.parametrize("anchor", LIBRARY_ANCHORS)
def test_cold_library_path_on_hard_blocks(anchor, riders, monkeypatch):
    """blocks above 160 (rocSOLVER dsyevd + dgemm) in a call of their own, and with blocks of n <= 160 in the same call: the kernel
    then runs over the compacted list of the small ones (nnsdp_project_psd_batched)"""
    monkeypatch.delenv("NNSDP_PROJ_ALG", raising=False)
    _check_cold(_launch(anchor, riders), "anchor %d -> %s%s" % (anchor, planned_variant(anchor),
                                                              ", riders through " + planned_variant(33) if riders else ""))


# ----------------------------------------------------------------------------- warm leg
WARM_TOL = 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [False, True], ids=["sweeps", "refine"])
@pytest.mark.parametrize("anchor", WARM_ANCHORS)
def test_warm_launch_of_hard_blocks_with_riders(anchor, refine, monkeypatch):
    """the warm entry on the same launches, once per starting basis: the identity, the exact eigenbasis, an unrelated orthogonal matrix,
    the eigenbasis of a matrix a relative 1e-6 away.  refine = False: the sweeps of the planned variant; refine = True: the refinement
    stage in front of them where the variant has one (ping-pong, packed - which then also takes 97 .. 128)."""
    monkeypatch.delenv("NNSDP_PROJ_ALG", raising=False)
    blocks = _launch(anchor)
    mats = [b.A for b in blocks]
    variant = planned_variant(anchor, None, refine)
    has_stage = refine and (variant.startswith("ping-pong") or variant.startswith("packed"))
    bad = []
    for kind in ("identity", "exact", "random", "near"):
        bases = [np.eye(b.n) if kind == "identity" else b.Q if kind == "exact" else b.Qrand if kind == "random" else b.Qnear for b in blocks]
        W, V, oc, _ = na.project_psd_warm(mats, bases, WARM_TOL, refine=refine)
        worst, worst_at, worst_orth = 0.0, "", 0.0
        for b, Wk, Vk in zip(blocks, W, V):
            if not (np.all(np.isfinite(Wk)) and np.all(np.isfinite(Vk))):
                bad.append((kind, "finite", b.name, b.n))
                continue
            fro = np.linalg.norm(b.A)
            err = np.linalg.norm(Wk - b.ref)
            lim = WARM_TOL * fro if not refine else 30.0 * WARM_TOL * fro + (0.0 if b.name in SCALED else 1e-12)
            if not err <= lim:
                bad.append((kind, "|W - ref|_F", b.name, b.n, err, lim))
            if fro > 0.0 and err / fro > worst:
                worst, worst_at = err / fro, "%s n=%d" % (b.name, b.n)
            orth = np.linalg.norm(Vk.T @ Vk - np.eye(b.n))
            worst_orth = max(worst_orth, orth)
            if not orth <= (1e-3 if refine else 1e-9):
                bad.append((kind, "|V'V - I|_F", b.name, b.n, orth))
            if b.name == "zero" and not np.array_equal(Wk, np.zeros_like(Wk)):
                bad.append((kind, "zero block is not exactly zero", b.name, b.n, np.abs(Wk).max()))
        # every block that meets the stage is counted in exactly one outcome; a launch without the stage counts nothing
        if sum(oc) != (len(blocks) if has_stage else 0):
            bad.append((kind, "outcome counts", oc, len(blocks)))
        print("[projection hard cases] warm anchor %d, refine %s -> %s, basis %s: %d blocks, outcomes %s; worst |W - ref|_F / |A|_F %.2e (%s), worst |V'V - I|_F %.2e"
              % (anchor, refine, variant, kind, len(blocks), oc, worst, worst_at, worst_orth))
    assert not bad, bad
