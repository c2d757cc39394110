"""Digests of what the projection kernel returns in every variant plan_projection can reach, case by case: the gate of changes that
reorganise the kernel's source without moving a floating-point operation (tools/stage_bits.py is the same gate for the ping-pong
variant's refinement stage alone).  A cold case is one launch through nnsdp_project_psd_batched whose blocks are the smallest, the
largest and an odd size of an instantiation's range and a 1 x 1 block; its digests are the SHA-256 of the bytes of W and of the
eigenvalues.  A warm case is two launches of one block on carried bases and state through nnsdp_project_psd_warm_state; its digests
are those of W, V, the outcome vector and the state words after each launch.
A batch case is the batched form of the kernel (k_proj_jacobi_b), which the cases above never launch: a two-member SolverBatch of one
query (SingleDecomp) after a fixed number of plain iterations in lockstep, shaped like tools/stage_interleave_bits.run_lockstep; its
digests are those of both members' raw multipliers.  Instantiations reached (the members' largest block through plan_projection:
W20-D10 has 9 blocks of 28 .. 43, W40-D20 19 blocks of 57 .. 85):
  W20-D10 unset  k_proj_jacobi_b<true, 1024, 3, 1, 5>  (ping-pong, RPW 5)      alg 0  k_proj_jacobi_b<true, 1024, 0, 1, 1>  (round robin, V in LDS)
  W40-D20 unset  k_proj_jacobi_b<true, 1024, 3, 1, 6>  (ping-pong, RPW 6)      alg 0  the same round-robin instantiation
          alg 2  k_proj_jacobi_b<true, 512, 2, 6, 12>  (systolic, V in LDS)
The unset cases run BATCH_ITERS[None] iterations, far past the cold sweeps: the members' refinement statistics (printed when the
record is written, kept as "refine_blocks") show blocks accepted by the stage; the cases with a variant forced have no stage, every
iteration runs the sweeps, and BATCH_ITERS["0"] iterations pin them.  Out of the fixtures' reach in the batched form: the systolic
instantiations with V in HBM, the packed one, ping-pong RPW 7 and round robin with V in HBM (and 256 threads beyond W10-D5 of
tests/test_stage_interleave_bits.py) - those are held by the resource table of the change and by sharing the very functions the
single form is pinned on.
usage: python tools/proj_bits.py [out.json [kind]]     (default tests/golden/proj_bits_parent.json; run on a build of the commit to
compare against; with a kind - cold, warm, batch - only those cases run and the file's other records are kept as they are)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import stage_bits
from stage_bits import _perturb, _sha, _sym

GOLDEN = os.path.join(ROOT, "tests", "golden", "proj_bits_parent.json")
# NNSDP_PROJ_ALG -> (smallest n, largest n, an odd n inside) of every instantiation plan_projection reaches under it, in the order
# of its branches: round robin 256 threads / ping-pong RPW 5, 6, 7 or round robin 1024 threads / systolic / packed
COLD = {
    None: ((1, 40, 23), (41, 74, 57), (75, 90, 83), (91, 96, 93), (97, 110, 103), (111, 128, 119), (129, 160, 151)),
    "0": ((1, 40, 23), (41, 96, 67), (97, 128, 113), (129, 160, 151)),
    "2": ((1, 40, 23), (41, 48, 45), (49, 96, 71), (97, 110, 103), (111, 128, 119), (129, 160, 151)),
    "3": ((1, 40, 23), (41, 74, 57), (75, 90, 83), (91, 96, 93), (97, 128, 113), (129, 160, 151)),
    "4": ((1, 40, 23), (41, 96, 67), (97, 128, 113), (129, 160, 151)),
}
MOVES = stage_bits.MOVES[:2] + ((1e-4, 1e-10, None),)        # (relative move, tolerance): converged / 1e-6 / 1e-4
# (label, NNSDP_PROJ_ALG, n, refine) of the warm launches: the packed variant's own stage and its rotation log (97 under the stage is
# the solver's choice; without it only the diagnostic value reaches it), the systolic and the round-robin variant in both V forms
WARM = [("packed", "4" if n == 97 and r == 0 else None, n, r) for n in (97, 129, 151, 160) for r in (0, 1, 2)] \
    + [("systolic-vlds", "2", 85, 0), ("systolic-7", None, 103, 0), ("systolic-8", None, 128, 0),
       ("rr256", "0", 31, 0), ("rr-vlds", "0", 67, 0), ("rr-vhbm", "0", 113, 0)]
# (fixture, beta, NNSDP_PROJ_ALG) of the batch cases and their plain iterations by NNSDP_PROJ_ALG
BATCH = [("W20-D10", 0, None), ("W20-D10", 0, "0"), ("W40-D20", 0, None), ("W40-D20", 0, "0"), ("W40-D20", 0, "2")]
BATCH_ITERS = {None: 3000, "0": 200, "2": 200}
NOTES = ("refine_blocks", "nmax")      # keys of a batch record that are notes for the reader, not digests


def cases():
    """(id, kind, NNSDP_PROJ_ALG or None, sizes (batch: (fixture, beta, iterations)), eta, tol, refine)"""
    out = []
    for alg, ranges in COLD.items():
        for lo, hi, odd in ranges:
            out.append((f"cold-alg{alg}-n{lo}_{hi}", "cold", alg, (lo, hi, odd, 1), 0.0, 0.0, 0))
    for label, alg, n, refine in WARM:
        for eta, tol, _ in MOVES:
            out.append((f"warm-{label}-n{n}-refine{refine}-eta{eta:g}", "warm", alg, (n,), eta, tol, refine))
    for name, beta, alg in BATCH:
        out.append((f"batch-{name}-b{beta}-alg{alg}", "batch", alg, (name, beta, BATCH_ITERS[alg]), 0.0, 0.0, 0))
    return out


def run_batch(name, beta, iters):
    """two members of one SolverBatch in lockstep, the same query: (members' multipliers, their refinement statistics, largest block)"""
    import helpers
    import nnsdp_amd as na
    q = helpers.product_query(helpers.load_problem(name, beta))
    opts = na.AdmmSdpOptions(decomp_mode=na.SingleDecomp(), max_iters=10 ** 9, polish=False)
    sb = na.SolverBatch([q, q], opts)
    try:
        sb.iterate(iters)
        members = [s.raw_multipliers() for s in sb.solvers]
        nmax = int(sb.solvers[0].info(5))
        stats = [[int(v) for v in r.summary.get("refine_blocks", [])] for r in sb.finish()]
    finally:
        sb.close()
    return members, stats, nmax


def run_case(case):
    """the case's launches on the loaded build: a list with one dict of digests per launch"""
    import nnsdp_amd as na
    cid, kind, alg, ns, eta, tol, refine = case
    seed = int.from_bytes(hashlib.sha256(cid.encode()).digest()[:4], "little")
    rng = np.random.default_rng(seed)
    if kind != "batch":
        pairs = [_sym(rng, n) for n in ns]
        mats, bases = [A for A, _ in pairs], [Q for _, Q in pairs]
    old = os.environ.get("NNSDP_PROJ_ALG")
    if alg is not None:
        os.environ["NNSDP_PROJ_ALG"] = alg
    else:
        os.environ.pop("NNSDP_PROJ_ALG", None)
    try:
        if kind == "batch":
            members, stats, nmax = run_batch(*ns)
            return [{"members": [_sha(m) for m in members], "refine_blocks": stats, "nmax": nmax}]
        if kind == "cold":
            W, ev, _ = na.project_psd_batched(mats)
            return [{"W": _sha(*W), "eig": _sha(*ev)}]
        state = np.zeros(4 * len(ns), dtype=np.int32)
        res = []
        for visit in range(2):
            mats = [_perturb(rng, A, eta) for A in mats]
            W, bases, oc, _ = na.project_psd_warm(mats, bases, tol, refine=refine, state=state)
            res.append({"W": _sha(*W), "V": _sha(*bases), "outcome": _sha(np.asarray(oc, dtype=np.int32)), "state": _sha(state),
                        "counts": [int(v) for v in oc]})
        return res
    finally:
        if old is None:
            os.environ.pop("NNSDP_PROJ_ALG", None)
        else:
            os.environ["NNSDP_PROJ_ALG"] = old


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    only = sys.argv[2] if len(sys.argv) > 2 else None
    table = {}
    if only is not None:
        with open(path) as f:
            table = json.load(f)
    for c in cases():
        if only is not None and c[1] != only:
            continue
        table[c[0]] = run_case(c)
        print(c[0], [r.get("counts", r.get("refine_blocks")) for r in table[c[0]]], [r.get("nmax") for r in table[c[0]]], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + "\n}\n")      # one case per line
    print(f"{len(table)} cases -> {path}")
