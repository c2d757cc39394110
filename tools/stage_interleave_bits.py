"""Digests of what the ping-pong projection kernel returns on the cases that pin the chains a wave runs side by side (V update, the
E~^2 product, the reconstruction W): the companion of tools/stage_bits.py for changes that only reorder independent MFMA chains
inside one wave (same sequence of products per accumulator: same bits).
Sizes 41, 49, 65, 85, 96 give 1, 1, 2, 3, 3 chains per wave in the V update (9, 16, 25, 36, 36 tiles over 16 waves) and 6, 10, 15, 21,
21 lower tiles (waves 0 .. 4 hold two from 85 on).  The length of the reconstruction's chains is the number of selected eigenpairs: the
spectra put 0, 1, 3, 4, 5 or about n / 2 eigenvalues on the smaller side of zero, which is the side the stage rebuilds from - the
positive one (W = sum) or the negative one (W = sym(nu) - sum).  Every case is a stepping move (one unchecked step) launched twice on
carried state (with and without the Gram product), with no helper workgroup and with the five a solver's launches take; two launches
mix all five sizes.  A case's digests are the SHA-256 of the bytes of W, V, the outcome vector and the state words after each launch.
The lockstep case is a two-member SolverBatch and a single Solver on the smallest fixture: the members' and the solver's multipliers.
usage: python tools/stage_interleave_bits.py [out.json]   (default tests/golden/stage_interleave_bits_parent.json; run on a build of
the commit to compare against)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_interleave_bits_parent.json")
SIZES = (41, 49, 65, 85, 96)
SELECT = (0, 1, 3, 4, 5, "half")          # eigenvalues on the smaller side of zero = eigenpairs the reconstruction selects
SIDES = ("pos", "neg")
SPLITS = ("0", "5")                        # NNSDP_SPLIT_WARM: helper workgroups per block
ETA, TOL = 1e-6, 3e-7                      # the stepping move of tools/stage_bits.py
LOCKSTEP = ("W10-D5", 0, 60)               # fixture, beta, plain iterations


def nsel_of(n, k, side):
    """(selected, positive, negative) eigenvalue counts: the stage rebuilds from the positive side unless the negative one is smaller"""
    if k == "half":
        k = n // 2 if side == "pos" else (n - 1) // 2        # pos: n // 2 <= n - n // 2; neg: strictly fewer negative ones
    return (k, k, n - k) if side == "pos" else (k, n - k, k)


def spectrum(n, k, side):
    _, p, q = nsel_of(n, k, side)
    return np.concatenate([np.linspace(0.2, 2.0, p), -np.linspace(0.1, 1.5, q)])


def cases():
    """(id, ((n, k), ...), side)"""
    out = [(f"n{n}-{side}{k}", ((n, k),), side) for n in SIZES for k in SELECT for side in SIDES]
    for side in SIDES:      # all five sizes in one launch, a different chain length on each
        out.append((f"mixed-{side}", tuple((n, SELECT[(i + 1) % len(SELECT)]) for i, n in enumerate(SIZES)), side))
    return out


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def inputs(case):
    """the case's two moves: [(matrices, starting bases or None for "what the last launch returned")]"""
    cid, blocks, side = case
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(cid.encode()).digest()[:4], "little"))
    mats, bases = [], []
    for n, k in blocks:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        mats.append((Q * spectrum(n, k, side)) @ Q.T)
        bases.append(Q)
    moves = []
    for _ in range(2):
        nxt = []
        for A in mats:
            D = rng.standard_normal(A.shape)
            D = 0.5 * (D + D.T)
            nxt.append(A + ETA * np.linalg.norm(A) / np.linalg.norm(D) * D)
        mats = nxt
        moves.append(mats)
    return moves, bases


def run_case(case, split, keep=None):
    """the case's two launches on the loaded build with `split` helper workgroups per block: one dict of digests (and the outcome
    counts, for the reader) per launch.  keep: a list that receives (matrices, W, counts) of every launch"""
    import nnsdp_amd as na
    moves, bases = inputs(case)
    state = np.zeros(4 * len(bases), dtype=np.int32)
    old = os.environ.get("NNSDP_SPLIT_WARM")
    os.environ["NNSDP_SPLIT_WARM"] = split
    try:
        res = []
        for mats in moves:
            W, bases, oc, _ = na.project_psd_warm(mats, bases, TOL, refine=1, state=state)
            res.append({"W": _sha(*W), "V": _sha(*bases), "outcome": _sha(np.asarray(oc, dtype=np.int32)), "state": _sha(state),
                        "counts": [int(v) for v in oc], "gram_credit": [(int(w) >> 24) & 15 for w in state.reshape(-1, 4)[:, 0]]})
            if keep is not None:
                keep.append((mats, W, [int(v) for v in oc]))
        return res
    finally:
        if old is None:
            os.environ.pop("NNSDP_SPLIT_WARM", None)
        else:
            os.environ["NNSDP_SPLIT_WARM"] = old


def run_lockstep():
    """two members of one SolverBatch in lockstep and a single Solver, the same query: (members' multipliers, the solver's)"""
    import helpers
    import nnsdp_amd as na
    name, beta, iters = LOCKSTEP
    q = helpers.product_query(helpers.load_problem(name, beta))
    opts = na.AdmmSdpOptions(decomp_mode=na.SingleDecomp(), max_iters=10 ** 9)
    sb = na.SolverBatch([q, q], opts)
    try:
        sb.iterate(iters)
        members = [s.raw_multipliers() for s in sb.solvers]
    finally:
        sb.close()
    s = na.Solver(q, opts)
    try:
        s.iterate(iters)
        single = s.raw_multipliers()
    finally:
        s.close()
    return members, single


def lockstep_digests(members, single):
    return {"members": [_sha(m) for m in members], "single": _sha(single)}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = {}
    for c in cases():
        for split in SPLITS:
            key = f"{c[0]}-split{split}"
            table[key] = run_case(c, split)
            print(key, [r["counts"] for r in table[key]], [r["gram_credit"] for r in table[key]], flush=True)
    members, single = run_lockstep()
    table["lockstep"] = lockstep_digests(members, single)
    print("lockstep: largest difference between a member and the single solver", max(float(np.abs(m - single).max()) for m in members),
          "of", float(np.abs(single).max()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} records -> {path}")
