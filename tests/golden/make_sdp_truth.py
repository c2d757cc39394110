"""Writes tests/golden/sdp_truth.json: the optimum of every SDP query of tests/sdp_truth_common.py by the independent interior point
(oracle/ipm.solve_query on the literal dense assembly; CPU only, numpy + scipy), next to the true value the query bounds.

    python tests/golden/make_sdp_truth.py              every case of sdp_truth_common.all_cases(), one process per case
    python tests/golden/make_sdp_truth.py --check      nothing is written: the regenerated rho_ipm against the file's, within the gaps

Recipes and numbers only, never weights: a case is its key (net, activation, box, output QC, direction, beta, interval source); the nets
are the recipes of tests/exact_common.py.  Per case: w (the attained value the bound must respect) and its witness x, rho_ipm,
dual_objective, gap, pinf, dinf, status, iterations, and the bracket
    lower = min(rho_ipm, dual_objective) - (gap + pinf + dinf) (1 + |rho_ipm|) per run,   upper = rho_ipm.
The interior point is run with four settings and the bracket taken over them (sdp_truth_common.ipm_bracket says why, with the
figures): upper = rho_ipm = the smallest objective of a feasible end point, lower = the smallest lower end of the converged runs, capped
by w on the degenerate boxes (stable, point).  `runs` keeps every run's objective, status and lambda_max(Z)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

os.environ.setdefault("OMP_NUM_THREADS", "1")          # one process per case: the 19- and 24-row solves gain nothing from threads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sdp_truth_common as sc      # noqa: E402
from oracle import ipm             # noqa: E402


def job(cs):
    t0 = time.time()
    w, x = sc.truth(cs)
    r, lower, upper, runs = sc.ipm_bracket(cs, w)
    row = dict(w=w, x=[float(v) for v in x], rho_ipm=r.objective, dual_objective=r.dual_objective, gap=r.gap, pinf=r.pinf, dinf=r.dinf,
               lower=lower, upper=upper)
    return sc.key(cs), dict({k: (v if k == "x" else float(v)) for k, v in row.items()}, status=r.status, iters=int(r.iters),
                            runs=[[float(t.objective), t.status, float(t.lambda_max)] for t in runs]), cs, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    cases = {}
    with ProcessPoolExecutor(max_workers=args.workers) as pool:
        for k, row, cs, secs in pool.map(job, sc.all_cases()):
            converged = row["status"] in ("OPTIMAL", "NEAR_OPTIMAL")
            assert converged or cs["box"] in sc.DEGENERATE, (k, row)
            cases[k] = row
            print(f"{k}: w {row['w']:+.10f} rho_ipm {row['rho_ipm']:+.10f} (rho - w {row['rho_ipm'] - row['w']:+.3e}) gap {row['gap']:.1e} "
                  f"pinf {row['pinf']:.1e} dinf {row['dinf']:.1e} {row['status']} {row['iters']} it, {secs:.1f} s", flush=True)
    if args.check:
        with open(sc.FIXTURE) as fh:
            old = json.load(fh)["cases"]
        assert sorted(old) == sorted(cases)
        for k, row in cases.items():
            tol = (row["gap"] + old[k]["gap"] + 1e-9) * (1.0 + abs(row["rho_ipm"]))
            assert abs(row["rho_ipm"] - old[k]["rho_ipm"]) <= tol and row["w"] == old[k]["w"], (k, row, old[k])
        print(f"{len(cases)} cases agree with the file within their gaps")
        return
    header = dict(generator="tests/golden/make_sdp_truth.py", solver="oracle/ipm.py solve_lmi, sdp_truth_common.IPM_RUNS",
                  table="tests/sdp_truth_common.py all_cases", w_min=sc.W_MIN, widen=sc.WIDEN)
    with open(sc.FIXTURE, "w") as fh:
        json.dump(dict(header=header, cases={k: cases[k] for k in sorted(cases)}), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {sc.FIXTURE}: {len(cases)} cases")


if __name__ == "__main__":
    main()
