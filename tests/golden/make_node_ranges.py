"""Writes tests/golden/node_ranges.json: exact ranges over the nodes of a ReLU split by tests/node_truth.py (CPU only, numpy + scipy).

    python tests/golden/make_node_ranges.py                 every group and the driver's root boxes, one process per node
    python tests/golden/make_node_ranges.py --check         nothing is written: the regenerated values against the file's, to 1e-9

Networks and nodes are stored as recipes (tests/node_truth_common.py: groups, driver_setting); per node the file keeps lo, hi and assign,
so that a recipe that moves is noticed, and values only, no regions: empty, depth (node_depth; null: no forced neuron), the region count,
and on a non-empty node vmax / vmin per literal and zmax / zmin per hidden pre-activation, all over the node.  Per driver net: top (the
exact maxima of the two literals over the root box), h0 = 0.5 top and v = clause_max(root, C, h0).

Before anything is written every value must satisfy |v - w| <= 1e-6 (1 + |v|), w the long-double forward value at the clipped argmax
(node_truth.V_W_BOUND: the argmax may sit 1e-7 outside a forced half-space).  The header records the worst |v - w| / (1 + |v|) and the
worst membership residual min_n s_n z_n(x) of an argmax.  No case is left out."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import node_truth as nt            # noqa: E402
import node_truth_common as nc     # noqa: E402


def attained(maxima):
    """the worst |v - w| / (1 + |v|) and the smallest membership residual of some NodeMax; refuses what passes V_W_BOUND"""
    gap, member = 0.0, np.inf
    for m in maxima:
        v, w = np.atleast_1d(m.v), np.atleast_1d(m.w)
        fin = np.isfinite(v)
        err = np.abs(v[fin] - w[fin]) / (1.0 + np.abs(v[fin]))
        assert np.all(err <= nt.V_W_BOUND), (v[fin][err > nt.V_W_BOUND], w[fin][err > nt.V_W_BOUND])
        gap = max(gap, float(err.max(initial=0.0)))
        member = min(member, float(np.min(np.atleast_1d(m.member)[fin], initial=np.inf)))
    return gap, member


def node_job(args):
    gname, b = args
    t0 = time.time()
    g = nc.groups()[gname]
    lo, hi, s = g["lo"][:, b], g["hi"][:, b], g["assign"][:, b]
    srch = nt.node_regions(g["net"].Ms, lo, hi, s)
    depth = nt.node_depth(srch)
    out = dict(lo=lo.tolist(), hi=hi.tolist(), assign=s.tolist(), empty=not srch.leaves, regions=len(srch.leaves),
               depth=None if not np.isfinite(depth.v) else depth.v)
    gap, member = 0.0, np.inf
    if srch.leaves:
        top, bot = nt.node_range(srch, g["C"])
        ztop, zbot = nt.node_pre_range(srch)
        gap, member = attained([top, bot, ztop, zbot] + ([depth] if np.isfinite(depth.v) else []))
        out.update(vmax=top.v.tolist(), vmin=bot.v.tolist(), zmax=ztop.v.tolist(), zmin=zbot.v.tolist())
    return gname, b, out, gap, member, srch.lps, time.time() - t0


def driver_job(name):
    import exact_range as er
    t0 = time.time()
    st = nc.driver_setting(name)
    Ms, lo, hi, C = st["net"].Ms, st["lo"], st["hi"], st["C"]
    root = nt.node_regions(Ms, lo, hi, np.zeros(sum(st["net"].xdims[1:-1]), dtype=np.int8))
    top = er.exact_max(Ms, lo, hi, C, search=root)
    assert np.all(np.abs(top.v - top.w) <= er.V_W_BOUND * (1.0 + np.abs(top.v)))
    h0 = 0.5 * top.v
    cm = nt.clause_max(root, C, h0)
    gap, member = attained([cm])
    return name, dict(top=top.v.tolist(), h0=h0.tolist(), v=cm.v, regions=len(root.leaves)), gap, member, time.time() - t0


def numbers(obj):
    if isinstance(obj, dict):
        return [x for k in sorted(obj) for x in numbers(obj[k])]
    if isinstance(obj, list):
        return [x for v in obj for x in numbers(v)]
    return [float(obj)] if isinstance(obj, (int, float)) else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    jobs = [(gname, b) for gname, g in nc.groups().items() for b in range(g["lo"].shape[1])]
    groups = {gname: dict(nodes=[None] * g["lo"].shape[1]) for gname, g in nc.groups().items()}
    driver, gap, member = {}, 0.0, np.inf
    with ProcessPoolExecutor(max_workers=args.workers) as pool:
        for gname, b, out, gp, mb, lps, secs in pool.map(node_job, jobs):
            groups[gname]["nodes"][b] = out
            gap, member = max(gap, gp), min(member, mb)
            print(f"{gname} node {b}: {'empty' if out['empty'] else out['regions']}, depth {out['depth']}, {lps} LPs, {secs:.1f} s", flush=True)
        for name, out, gp, mb, secs in pool.map(driver_job, list(nc.DRIVER)):
            driver[name] = out
            gap, member = max(gap, gp), min(member, mb)
            print(f"driver {name}: {out}, {secs:.1f} s", flush=True)
    for gname, g in nc.groups().items():
        groups[gname]["xdims"] = list(g["net"].xdims)
    if args.check:
        with open(nc.FIXTURE) as fh:
            old = json.load(fh)
        for key, new in (("groups", groups), ("driver", driver)):
            a, b = np.array(numbers(new)), np.array(numbers(old[key]))
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9, (key, np.abs(a - b).max())
            print(f"{key}: {a.size} numbers equal to the file's to 1e-9")
        return
    header = dict(generator="tests/golden/make_node_ranges.py", oracle="tests/node_truth.py", v_w_bound=nt.V_W_BOUND,
                  worst_v_minus_w=gap, worst_membership=member,
                  note="worst_v_minus_w: max |v - w| / (1 + |v|) over every stored maximum; worst_membership: the smallest "
                       "min_n s_n z_n(x) at an argmax, how far outside its node an LP vertex lies")
    with open(nc.FIXTURE, "w") as fh:
        json.dump(dict(header=header, groups=groups, driver=driver), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {nc.FIXTURE}: {len(jobs)} nodes, worst |v - w| {gap:.3e}, worst membership {member:.3e}")


if __name__ == "__main__":
    main()
