"""Digests of what a caller of the solve loop sees, case by case: the gate of changes to the five launches behind the projection
(k_gather_g, k_spmv_At, k_gemv_sym, k_spmv_A_x_all, k_update_nu and their batch forms) that move no floating-point operation.
A solver case is one fixture and one way of driving the handle: `eager` (iterate(n, time_eig=True): one launch per stage), `graph`
(iterate(n): hipGraph replay) or `advance` (the solve loop's check iterations and adaptation inside).  Its digests are the SHA-256 of
the bytes of Solver.raw_multipliers() after 1, 9 and 60 iterations (W40-D20: 1 and 9) and of Solver.residuals() after the last.  The
batch case is a SolverBatch of three problems of different sizes after iterate(24): the members' residuals and finish() objectives.
Every case forces the dense M^-1 (minv_mode = 1): the solver cases then run k_gemv_sym (odd multiplier counts 203, 347, 803, 1 965 and
the even 600 of W10-D10 beta 2, whose rows have no last single element); the batch case runs the tiled product of the batch handle
(k_symv_tiles_b), not that kernel - it gates the batch forms of the sparse launches and the multiplier update.
A sharded case is a solver case on a one-rank clique-sharded handle (set_comm_callback(1, 0, ...): the all-reduce of one rank leaves its
buffer alone), the branch no other case takes: k_gather_h and k_finish_g in place of k_gather_g, k_check_dual reading the exchanged sum,
k_update_nu with the rank's element range and the resynchronisation of the multiplier block.  Such a handle replays no graph.
usage: python tools/tail_bits.py [out.json]     (default tests/golden/tail_bits_parent.json; run on a build of the commit to compare against)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "tail_bits_parent.json")
# (fixture, beta, decomposition, iteration counts at which the multipliers are digested)
FIXTURES = (("W20-D10", 0, "single", (1, 9, 60)),      # every class of row, column and entry except columns above 256 nonzeros
            ("W10-D5", 3, "double", (1, 9, 60)),       # nearly every row medium; NE 230, ng 347
            ("W10-D5", 0, "single", (1, 9, 60)),       # ng 203
            ("W10-D10", 2, "double", (1, 9, 60)),      # ng 600: an even multiplier count
            ("W40-D20", 0, "single", (1, 9)))          # columns above 256 nonzeros, more than one GEMV group
MODES = ("eager", "graph", "advance")
SHARDED = (("W10-D5", 3, "double", (1, 9, 60)),)       # several cliques, NE 230, ng 347
SHARDED_MODES = ("eager", "advance")
BATCH = (("W10-D5", 0, "single"), ("W10-D5", 3, "double"), ("W10-D10", 2, "double"))
BATCH_ITERS = 24


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def cases():
    """(id, kind, ...)"""
    out = [(f"{name}-b{beta}-{dec}-{mode}", "solver", name, beta, dec, counts, mode) for name, beta, dec, counts in FIXTURES for mode in MODES]
    out += [(f"{name}-b{beta}-{dec}-sharded1-{mode}", "sharded", name, beta, dec, counts, mode) for name, beta, dec, counts in SHARDED for mode in SHARDED_MODES]
    out.append(("batch-" + "+".join(f"{n}-b{b}" for n, b, _ in BATCH), "batch"))
    return out


def _solver_args(name, beta, dec):
    import helpers
    import nnsdp_amd as na
    q = helpers.product_query(helpers.load_problem(name, beta))
    mode = na.SingleDecomp() if dec == "single" else na.DoubleDecomp()
    return q, na.AdmmSdpOptions(decomp_mode=mode, max_iters=10 ** 9, minv_mode=1)


def run_case(case):
    """the case on the loaded build: a dict of digests"""
    import nnsdp_amd as na
    if case[1] == "batch":
        qs, os_ = zip(*[_solver_args(*m) for m in BATCH])
        sb = na.SolverBatch(list(qs), list(os_))
        try:
            sb.iterate(BATCH_ITERS)
            res = sb.residuals()
            obj = [s.objective_value for s in sb.finish()]
        finally:
            sb.close()
        out = {f"residuals{i}": _sha(r) for i, r in enumerate(res)}
        out.update({f"objective{i}": _sha([v]) for i, v in enumerate(obj)})
        return out
    _, kind, name, beta, dec, counts, mode = case
    q, o = _solver_args(name, beta, dec)
    s = na.Solver(q, o)
    try:
        if kind == "sharded":
            s.set_comm_callback(1, 0, lambda a: None)
        out, done = {}, 0
        for n in (counts if mode != "advance" else counts[-1:]):      # (advance: one call, so that the check iteration falls where the solve loop puts it)
            if mode == "eager":
                s.iterate(n - done, time_eig=True)
            elif mode == "graph":
                s.iterate(n - done)
            else:
                s.advance(n - done)
            done = n
            out[f"nu{n}"] = _sha(s.raw_multipliers())
        out["residuals"] = _sha(s.residuals())
    finally:
        s.close()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = {}
    for c in cases():
        table[c[0]] = run_case(c)
        print(c[0], table[c[0]][sorted(table[c[0]])[0]][:16], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + "\n}\n")      # one case per line
    print(f"{len(table)} cases -> {path}")
