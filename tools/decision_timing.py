#!/usr/bin/env python3
"""Sparse certified bound against the dense polish, and time to a DECISION against time to a converged bound.
usage: python tools/decision_timing.py [case ...]   cases: W40-D20-single W40-D20-double W20-D100 acas-path W10-D5   (default: all)
Writes profiles/decision_timing_<case>.json (or $DECISION_TIMING_OUT/...).  Per case:
  bound    at a few iterates of one solve: nnsdp_solver_certified_bound through the sparse Cholesky (median of 7 calls on the same
           iterate, first call - plan + buffers - reported apart) and through the dense polish (a twin handle created with
           NNSDP_SPARSE_BOUND=0; median of 3), both wall-clock around a call that ends in a device synchronise, and both objectives
  decide   iterations and wall-clock of a solve with a target at 1.01 x, 1.05 x, 1.5 x and 0.95 x the converged bound, against the
           cert_tol = 1e-3 solve without a target; every solve is run twice and the second (warm) one is reported
Timings are host clocks of whole calls on an otherwise idle stream; the GPU is shared, so expect a few per cent of spread."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-sdp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import helpers, nnsdp_amd as na
from nnsdp_amd import frontend as F


def case(name):
    if name == "W40-D20-single": return helpers.product_query(helpers.load_problem("W40-D20", 0)), na.SingleDecomp(), (1000, 3000, 6000)
    if name == "W40-D20-double": return helpers.product_query(helpers.load_problem("W40-D20", 0)), na.DoubleDecomp(), (1000, 3000, 6000)
    if name == "W10-D5": return helpers.product_query(helpers.load_problem("W10-D5", 0)), na.SingleDecomp(), (200, 1000, 5000)
    if name == "acas-path": return helpers.acas_shaped_query(), na.PathDecomp(), (500, 1500)
    if name == "W20-D100":
        z = np.load(os.path.join(helpers.GOLDEN, "nets", "scale-I2-O2-W20-D100.npz"))
        xdims = [int(v) for v in z["xdims"]]
        net = na.FeedFwdNet(xdims=xdims, Ms=[np.array(z[f"M{k}"], dtype=np.float64) for k in range(len(xdims) - 1)])
        q, _ = F.ellipsoidQuery(net, np.full(2, 0.5), np.full(2, 1.5), 0)
        return q, na.DoubleDecomp(), (1000, 3000)
    raise SystemExit(f"unknown case {name}")


def bound_rows(q, mode, iterates):
    opts = na.AdmmSdpOptions(decomp_mode=mode, max_iters=10 ** 8)
    sp = na.Solver(q, opts)
    os.environ["NNSDP_SPARSE_BOUND"] = "0"
    de = na.Solver(q, opts)
    de.certified_bound()                     # (reads the variable: this handle stays on the dense polish)
    del os.environ["NNSDP_SPARSE_BOUND"]
    rows, done, first = [], 0, None
    for it in iterates:
        sp.advance(it - done); de.advance(it - done); done = it
        t = time.perf_counter(); o0 = sp.certified_bound(); t_first = 1e3 * (time.perf_counter() - t)
        if first is None: first = t_first
        ts = []
        for _ in range(7):
            t = time.perf_counter(); o = sp.certified_bound(); ts.append(1e3 * (time.perf_counter() - t))
            assert o[0] == o0[0], "the sparse bound is deterministic"
        td = []
        for _ in range(3):
            t = time.perf_counter(); od = de.certified_bound(); td.append(1e3 * (time.perf_counter() - t))
        rows.append(dict(iterate=it, sparse_objective=o0[0], sparse_certified=o0[2], sparse_ms_median=statistics.median(ts), sparse_ms_min=min(ts), sparse_ms_max=max(ts),
                         dense_objective=od[0], dense_certified=od[2], dense_ms_median=statistics.median(td), sparse_over_dense_minus_1=o0[0] / od[0] - 1.0 if od[2] and o0[2] else None))
        print(rows[-1], flush=True)
    plan = sp.cert_plan()
    out = dict(rows=rows, first_call_ms=first, supported=bool(sp.info(13)), plan=dict(n=plan["n"], n_super=plan["n_super"], max_front=plan["max_front"], fill=plan["fill"]))
    sp.close(); de.close()
    return out


def solve(q, mode, **kw):
    res = None
    for _ in range(2):
        t = time.perf_counter()
        s = na.runQuery(q, na.AdmmSdpOptions(decomp_mode=mode, max_iters=200000, max_time=120, **kw))
        res = dict(status=s.termination_status, iters=s.summary["iters"], wall_s=time.perf_counter() - t, solve_s=s.solve_time, objective=s.objective_value,
                   lambda_max=s.summary["lambda_max"], sparse_bound_calls=s.summary.get("sparse_bound_calls", 0))
    return res


def main():
    names = sys.argv[1:] or ["W10-D5", "W40-D20-single", "W40-D20-double", "W20-D100", "acas-path"]
    outdir = os.environ.get("DECISION_TIMING_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(outdir, exist_ok=True)
    for name in names:
        q, mode, iterates = case(name)
        rec = dict(case=name, decomp=type(mode).__name__, bound=bound_rows(q, mode, iterates))
        ref = solve(q, mode, eps_rel=1e-6, cert_tol=1e-3)
        rec["cert_tol_1e-3"] = ref
        print(name, "cert_tol 1e-3:", ref, flush=True)
        rec["decide"] = {}
        for f in (1.01, 1.05, 1.5, 0.95):
            rec["decide"][str(f)] = solve(q, mode, eps_rel=1e-6, target=f * ref["objective"])
            print(name, "target", f, rec["decide"][str(f)], flush=True)
        with open(os.path.join(outdir, f"decision_timing_{name}.json"), "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
