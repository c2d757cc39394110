"""(diagnostic) solver families against the same queries as independently created solvers in a plain SolverBatch: set-up wall time,
time per lockstep iteration, the fused M^-1 kernel per pass, device memory taken.  The two forms alternate in one process, `reps`
times each; medians and the spread (max - min) are reported and written as JSON.

Time per iteration: wall time of the synchronous nnsdp_batch_iterate over `iters` (>= 2 000) warm iterations after advance(2000) -
the call enqueues graph replays of 8 iterations and waits once, so launch and wait latency are below 0.1 % of the figure.  The
per-kernel times of the two forms come from a rocprofv3 --kernel-trace --stats run of `--profile-run B` (family) or
`--profile-run B --plain`.

Structured cases (W40-D20-b7, W20-D100-b7: the published nets, Double decomposition, auto minv_mode, the hyperplane directions and
intervals of findReach2Dpoly on [0.5, 1.5]^2): three forms - "family" (the fused structured stages, k_minv_*_multi), "unfused" (the
same family with NNSDP_FAMILY_STRUCT=0: four launches per member, the path before the fused stages existed) and "plain"
(independently created solvers).  The switch is read once per process, so every measurement is a child process of its own; the forms
alternate, `reps` times each.  Beside the lockstep iteration the family form reports the HIP-event time of the four fused launches
for one pass over B vectors, the bytes of one pass over the factors (operand_bytes of apply_minv: Pinv, H, HT, Scinv, v) and the
rate that gives against the 6.29 TB/s copy rate measured on this device.

usage: python tools/family_timing.py W40-D20 [--B 2,6,13] [--reps 5] [--iters 2000] [--out profiles/family_timing_W40-D20.json]
       python tools/family_timing.py W40-D20 --profile-run 13 [--plain]
       python tools/family_timing.py W40-D20-b7 [--B 2,6] [--forms family,unfused,plain] [--out profiles/family_structured_timing_W40-D20-b7.json]
       python tools/family_timing.py W40-D20-b7 --profile-run 6 [--form unfused]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-sdp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import nnsdp_amd as na
import helpers

CASES = {"W40-D20": ("W40-D20", 0, na.SingleDecomp), "W40-D40": ("W40-D40", 0, na.DoubleDecomp)}
STRUCTURED = {"W40-D20-b7": ("W40-D20", 7), "W20-D100-b7": ("W20-D100", 7)}
COPY_RATE = 6.29e12        # bytes / s, measured device copy rate


def queries(case, B):
    if case in STRUCTURED:
        import oracle_state as ost
        from nnsdp_amd import frontend as F
        name, beta = STRUCTURED[case]
        net = ost.golden_net(name)
        lo, hi = np.full(2, 0.5), np.full(2, 1.5)
        qa = F.makeQcActivs(net, lo, hi, beta)
        return [na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_activs=qa,
                              qc_reach=na.QcReachHplane(normal=np.array([np.cos(2 * np.pi * i / B), np.sin(2 * np.pi * i / B)]))) for i in range(B)]
    name, beta, _ = CASES[case]
    d = helpers.load_problem(name, beta)
    return [helpers.product_query(d, "hplane", normal=(np.cos(2 * np.pi * i / B), np.sin(2 * np.pi * i / B))) for i in range(B)]


def options(case):
    if case in STRUCTURED:
        return na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp(), max_iters=10 ** 8, minv_mode=0)
    return na.AdmmSdpOptions(decomp_mode=CASES[case][2](), max_iters=10 ** 8, minv_mode=1)


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def one(case, B, family, burn, iters, form=None):
    qs, o = queries(case, B), options(case)
    m0 = used_bytes()
    t0 = time.perf_counter()
    sb = na.SolverFamily(qs, o) if family else na.SolverBatch(qs, o)
    t_setup = time.perf_counter() - t0
    mem = used_bytes() - m0
    try:
        sb.advance(burn)
        sb.iterate(64)                        # the cold iteration after the resync and the graph's instantiation stay outside
        t0 = time.perf_counter()
        sb.iterate(iters)
        us = 1e6 * (time.perf_counter() - t0) / iters
        res = dict(setup_s=t_setup, iter_us=us, device_bytes=mem, fused_groups=sb.batch_info(1))
        if case in STRUCTURED:
            s0 = sb.solvers[0]
            Q = np.random.default_rng(0).standard_normal((B, s0.cp.ngamma))
            _, structured, nbytes = s0.apply_minv(Q[0])
            if not structured:
                raise SystemExit("auto minv_mode chose the dense M^-1 for this case (fewer than 3 500 kept multipliers)")
            res.update(fused_groups=sb.batch_info(3), fused_members=sb.batch_info(4), multipliers=int(s0.cp.ngamma), chunks=s0.info(10),
                       scalar_path_chunks=s0.info(11), pass_bytes=int(nbytes), device=torch.cuda.get_device_name(0))
            if form == "family" and res["fused_groups"] < 1:
                raise SystemExit("the family form was not fused (batch_info(3) == 0): it would time the per-member launches")
            if form == "unfused" and res["fused_groups"] != 0:
                raise SystemExit("the unfused form was fused: NNSDP_FAMILY_STRUCT=0 did not reach the library")
            if form == "family":
                us4 = 1e3 * min(s0.apply_minv_structured_multi(Q)[1] for _ in range(5))
                res.update(fused_pass_us=us4, fused_pass_bytes_per_s=nbytes / (1e-6 * us4), fused_pass_share_of_copy_rate=nbytes / (1e-6 * us4) / COPY_RATE)
        elif family:
            ng = sb.solvers[0].cp.ngamma
            Q = np.random.default_rng(0).standard_normal((B, ng))
            res["fused_kernel_us"] = 1e3 * min(sb.solvers[0].apply_minv_multi(Q)[1] for _ in range(5))
        return res
    finally:
        sb.close()


def summary(rows, key):
    v = sorted(r[key] for r in rows)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], spread=v[-1] - v[0])


def child(case, B, form, burn, iters):
    """one measurement in a process of its own (NNSDP_FAMILY_STRUCT is read once)"""
    env = dict(os.environ)
    env.pop("NNSDP_FAMILY_STRUCT", None)
    if form == "unfused":
        env["NNSDP_FAMILY_STRUCT"] = "0"
    cmd = [sys.executable, os.path.abspath(__file__), case, "--profile-run", str(B), "--form", form, "--burn-in", str(burn), "--iters", str(iters)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed with status {r.returncode}:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def structured_main(a):
    forms = a.forms.split(",")
    out = dict(case=a.case, iters=a.iters, burn_in=a.burn_in, reps=a.reps, forms=forms, copy_rate_bytes_per_s=COPY_RATE, sizes={})
    for B in [int(v) for v in a.B.split(",")]:
        rows = {f: [] for f in forms}
        for _ in range(a.reps):               # the forms alternate
            for f in forms:
                rows[f].append(child(a.case, B, f, a.burn_in, a.iters))
        first = rows[forms[0]][0]
        out.update(device=first["device"], multipliers=first["multipliers"], chunks=first["chunks"], scalar_path_chunks=first["scalar_path_chunks"],
                   pass_bytes=first["pass_bytes"])
        row = {f: {k: summary(rows[f], k) for k in ("setup_s", "iter_us", "device_bytes")} for f in forms}
        for f in forms:
            row[f]["fused_groups"] = rows[f][0]["fused_groups"]
        if "family" in forms:
            for k in ("fused_pass_us", "fused_pass_bytes_per_s", "fused_pass_share_of_copy_rate"):
                row["family"][k] = summary(rows["family"], k)
        if "family" in forms and "unfused" in forms:
            fu, un = row["family"]["iter_us"], row["unfused"]["iter_us"]
            row["gain_us"] = un["median"] - fu["median"]
            row["sum_of_spreads_us"] = un["spread"] + fu["spread"]
        out["sizes"][str(B)] = row
        print(f"{a.case} B={B}: " + "; ".join(f"{f} {row[f]['iter_us']['median']:.1f} us (spread {row[f]['iter_us']['spread']:.1f})" for f in forms)
              + (f"; fused pass {row['family']['fused_pass_us']['median']:.1f} us over {out['pass_bytes'] / 1e6:.1f} MB = "
                 f"{row['family']['fused_pass_bytes_per_s']['median'] / 1e12:.2f} TB/s" if "family" in forms else ""), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=sorted(CASES) + sorted(STRUCTURED))
    ap.add_argument("--B", default="2,6,13")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--burn-in", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", type=int, default=0)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--forms", default="family,unfused,plain")
    ap.add_argument("--form", default=None, choices=["family", "unfused", "plain"])
    a = ap.parse_args()
    if a.case in STRUCTURED and not a.profile_run:
        if a.B == "2,6,13":
            a.B = "2,6"
        return structured_main(a)
    if a.case in STRUCTURED:
        if a.form == "unfused" and os.environ.get("NNSDP_FAMILY_STRUCT") != "0":
            raise SystemExit("the unfused form needs NNSDP_FAMILY_STRUCT=0 in the environment (it is read once, at the first batch)")
        form = a.form or "family"
        print(json.dumps(one(a.case, a.profile_run, form != "plain", a.burn_in, a.iters, form)))
        return
    if a.profile_run:
        print(json.dumps(one(a.case, a.profile_run, not a.plain, a.burn_in, a.iters)))
        return
    torch.cuda.init()
    out = dict(case=a.case, iters=a.iters, burn_in=a.burn_in, reps=a.reps, device=torch.cuda.get_device_name(0), sizes={})
    for B in [int(v) for v in a.B.split(",")]:
        fam, plain = [], []
        for _ in range(a.reps):               # the two forms alternate
            fam.append(one(a.case, B, True, a.burn_in, a.iters))
            plain.append(one(a.case, B, False, a.burn_in, a.iters))
        row = dict(family={k: summary(fam, k) for k in ("setup_s", "iter_us", "device_bytes", "fused_kernel_us")},
                   plain={k: summary(plain, k) for k in ("setup_s", "iter_us", "device_bytes")})
        out["sizes"][str(B)] = row
        print(f"{a.case} B={B:2d}: iteration family {row['family']['iter_us']['median']:.1f} us (spread {row['family']['iter_us']['spread']:.1f}) "
              f"plain {row['plain']['iter_us']['median']:.1f} us (spread {row['plain']['iter_us']['spread']:.1f}); set-up family "
              f"{row['family']['setup_s']['median']:.3f} s plain {row['plain']['setup_s']['median']:.3f} s; memory family "
              f"{row['family']['device_bytes']['median'] / 1e6:.0f} MB plain {row['plain']['device_bytes']['median'] / 1e6:.0f} MB; fused kernel "
              f"{row['family']['fused_kernel_us']['median']:.1f} us per pass", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
