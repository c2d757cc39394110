"""(diagnostic) solver families against the same queries as independently created solvers in a plain SolverBatch: set-up wall time,
time per lockstep iteration, the fused M^-1 kernel per pass, device memory taken.  The two forms alternate in one process, `reps`
times each; medians and the spread (max - min) are reported and written as JSON.

Time per iteration: wall time of the synchronous nnsdp_batch_iterate over `iters` (>= 2 000) warm iterations after advance(2000) -
the call enqueues graph replays of 8 iterations and waits once, so launch and wait latency are below 0.1 % of the figure.  The
per-kernel times of the two forms come from a rocprofv3 --kernel-trace --stats run of `--profile-run B` (family) or
`--profile-run B --plain`.

usage: python tools/family_timing.py W40-D20 [--B 2,6,13] [--reps 5] [--iters 2000] [--out profiles/family_timing_W40-D20.json]
       python tools/family_timing.py W40-D20 --profile-run 13 [--plain]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-sdp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import nnsdp_amd as na
import helpers

CASES = {"W40-D20": ("W40-D20", 0, na.SingleDecomp), "W40-D40": ("W40-D40", 0, na.DoubleDecomp)}


def queries(case, B):
    name, beta, _ = CASES[case]
    d = helpers.load_problem(name, beta)
    return [helpers.product_query(d, "hplane", normal=(np.cos(2 * np.pi * i / B), np.sin(2 * np.pi * i / B))) for i in range(B)]


def options(case):
    return na.AdmmSdpOptions(decomp_mode=CASES[case][2](), max_iters=10 ** 8, minv_mode=1)


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def one(case, B, family, burn, iters):
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
        if family:
            ng = sb.solvers[0].cp.ngamma
            Q = np.random.default_rng(0).standard_normal((B, ng))
            res["fused_kernel_us"] = 1e3 * min(sb.solvers[0].apply_minv_multi(Q)[1] for _ in range(5))
        return res
    finally:
        sb.close()


def summary(rows, key):
    v = sorted(r[key] for r in rows)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], spread=v[-1] - v[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=sorted(CASES))
    ap.add_argument("--B", default="2,6,13")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--burn-in", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", type=int, default=0)
    ap.add_argument("--plain", action="store_true")
    a = ap.parse_args()
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
