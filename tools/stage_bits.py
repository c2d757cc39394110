"""Digests of what the projection kernel's refinement stage returns, case by case: the gate of changes that only move work between
waves of the ping-pong variant (same chains, same reductions, same bits).  Every case is two (one family: three) warm launches of at most three
blocks through nnsdp_project_psd_warm_state; a case's digests are the SHA-256 of the bytes of W, V, the outcome vector and the returned
state words after each launch.
usage: python tools/stage_bits.py [out.json]     (default tests/golden/stage_bits_parent.json; run on a build of the commit to compare against)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nn-sdp_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_bits_parent.json")
SIZES = (41, 48, 49, 64, 65, 80, 81, 85, 96)        # 3 .. 6 tile rows: 6, 10, 15, 21 lower tiles, full and ragged edge tiles
MIXED = ((57, 85, 64), (41, 96, 65), (81, 48, 80))
# (relative move, tolerance, AdmmSdpOptions.proj_refine): converged as it arrives / one unchecked step / a move whose prediction misses the
# accepted level (30 x tol |A|: the products of two first-order terms of size 1e-4 stand against 3e-9), which ends in the checked step
# or in the sweeps
MOVES = ((0.0, 1e-7, 1), (1e-6, 3e-7, 1), (1e-4, 1e-10, 2))
# the same rejected move without the checked form, a near miss for it, and a move far outside first order (back-off word): n = 64, 85
EXTRA = ((1e-4, 1e-10, 1), (1e-4, 1e-8, 2), (3e-2, 1e-6, 1))


def _sym(rng, n):
    spec = np.concatenate([np.linspace(0.2, 2.0, n - n // 3), -np.linspace(0.1, 1.5, n // 3)])       # two thirds positive
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * spec) @ Q.T, Q


def _perturb(rng, A, eta):
    if eta == 0.0:
        return A
    D = rng.standard_normal(A.shape)
    D = 0.5 * (D + D.T)
    return A + eta * np.linalg.norm(A) / np.linalg.norm(D) * D


def cases():
    """(id, sizes, eta, tol, split or None, pivot, refine)"""
    out = []
    for eta, tol, refine in MOVES:
        for n in SIZES:
            out.append((f"n{n}-eta{eta:g}", (n,), eta, tol, None, False, refine))
        for ns in MIXED:
            out.append((f"mixed{'_'.join(map(str, ns))}-eta{eta:g}", ns, eta, tol, None, False, refine))
        for n in (81, 85, 96):
            for split in ("0", "1"):
                out.append((f"n{n}_57_64-split{split}-eta{eta:g}", (n, 57, 64), eta, tol, split, False, refine))
    for eta, tol, refine in EXTRA:
        for split in (None, "1"):
            out.append((f"extra64_85-eta{eta:g}-tol{tol:g}-refine{refine}-split{split}", (64, 85), eta, tol, split, False, refine))
    out.append(("pivot-n85", (85,), 0.0, 1e-7, None, True, 1))
    for split in ("0", "1"):
        out.append((f"pivot-n85-split{split}", (85,), 0.0, 1e-7, split, True, 1))
    return out


def _pivot_input(n):
    """one pair of eigenvalues on either side of zero, coupled far above its gap: the stage rotates it exactly, then steps"""
    rng = np.random.default_rng(n)
    h = n // 2
    spec = np.concatenate([np.linspace(0.2, 2.0, h - 1), [1e-4, -1e-4], -np.linspace(0.1, 1.5, n - h - 1)])
    Q0, _ = np.linalg.qr(rng.standard_normal((n, n)))
    E = 1e-7 * rng.standard_normal((n, n))
    E = 0.5 * (E + E.T)
    E[h - 1, h] = E[h, h - 1] = 1e-3
    A1 = Q0 @ (np.diag(spec) + E) @ Q0.T
    return 0.5 * (A1 + A1.T), Q0


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(case):
    """the case's launches on the loaded build: a list with one dict of digests (and the outcome counts, for the reader) per launch.
    Two launches on carried state: the first measures the Gram product (zero state), the second runs on its credit."""
    import nnsdp_amd as na
    cid, ns, eta, tol, split, pivot, refine = case
    seed = int.from_bytes(hashlib.sha256(cid.encode()).digest()[:4], "little")
    rng = np.random.default_rng(seed)
    if pivot:
        pairs = [_pivot_input(n) for n in ns]
    else:
        pairs = [_sym(rng, n) for n in ns]
    mats, bases = [A for A, _ in pairs], [Q for _, Q in pairs]
    state = np.zeros(4 * len(ns), dtype=np.int32)
    old = os.environ.get("NNSDP_SPLIT_WARM")
    if split is not None:
        os.environ["NNSDP_SPLIT_WARM"] = split
    else:
        os.environ.pop("NNSDP_SPLIT_WARM", None)
    try:
        res = []
        for visit in range(3 if eta > 1e-3 else 2):      # (a move far outside first order: the third visit finds the back-off word set and skips the stage)
            if not pivot:
                mats = [_perturb(rng, A, eta) for A in mats]
            W, bases, oc, _ = na.project_psd_warm(mats, bases, tol, refine=refine, state=state)
            res.append({"W": _sha(*W), "V": _sha(*bases), "outcome": _sha(np.asarray(oc, dtype=np.int32)), "state": _sha(state),
                        "counts": [int(v) for v in oc], "gram_credit": [(int(w) >> 24) & 15 for w in state.reshape(-1, 4)[:, 0]]})
        return res
    finally:
        if old is None:
            os.environ.pop("NNSDP_SPLIT_WARM", None)
        else:
            os.environ["NNSDP_SPLIT_WARM"] = old


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = {}
    for c in cases():
        table[c[0]] = run_case(c)
        print(c[0], [r["counts"] for r in table[c[0]]], [r["gram_credit"] for r in table[c[0]]], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} cases -> {path}")
