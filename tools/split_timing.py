#!/usr/bin/env python3
"""Batched CROWN bounds: the GPU kernel against the host routine, and where one verifySplit spends its time.
usage: python tools/split_timing.py [--nlit | --resident | --alpha | --frontier | --reach | --wide | --forest | --relu | --relu-frontier] [case ...]   cases: W10-D5 W40-D20 acas-shape   (default: all)
With --relu-frontier only the node-frontier leg runs (it takes no cases) and profiles/split_timing_relu_frontier.json is written:
  search   the two whole-search instances of the --relu leg, verifyReluSplit with crown_backend "resident" and frontier "host" and then
           "device" in this process: verdict, nodes visited, levels, milliseconds (median, min, max of 5 after 1 warm run), and for the
           device frontier the HIP-event time of its kernels
With --relu only the ReLU-split leg runs (cases W10-D5 and W40-D20 by default) and profiles/split_timing_relu.json is written:
  bound    CrownBounder.bound_nodes at 1, 256 and 4096 nodes with 0 and 16 multiplier steps beside CrownBounder.bound on the same boxes in
           the same process: HIP-event time of the launches (median, min, max of 7 after 2 warm calls) and the median wall-clock of the call
  search   verifyReluSplit against verifySplit (both crown_backend "resident", bounds only) on a 16-input and a 12-input net: verdict,
           nodes / boxes visited, milliseconds (median, min, max of 5 after 1 warm run); --no-search leaves it out
With --forest only the forest leg runs (cases W10-D5 and acas-shape by default) and profiles/split_timing_forest_<case>.json is written:
  forest   R = 1, 16, 256, 4096 roots: a regular grid of the case's root box (2^k cells, the halvings dealt to the coordinates in turn);
           per root the literal y_0 - y_last <= s_r + 0.1 (c0_r - s_r), s_r the largest of 256 sampled values in the root, c0_r its
           per-output bound; literal_bounds, max_boxes 512 per root.  On ONE CrownBounder: R sequential search calls against one
           search_many: wall-clock of the whole (median of 3 after 1 warm run; one run at R = 4096), the HIP-event time of the launches,
           levels (sequential: the sum over the roots), bound launches and bounded boxes per launch
With --wide only the wide leg runs (cases W40-D20, acas-shape - the 5-50x6-5 net - and 5-100x4-5 by default) and
profiles/split_timing_wide_<case>.json is written:
  bound    CrownBounder(max_width=128).bound at nbox = 1, 256, 4096: HIP-event time of the launch and wall-clock of the call, median of 7
           after 2 warm calls.  On a net of widths <= 64 beside CrownBounder(max_width=64).bound in the same process - what the slab loop and
           one workgroup per CU instead of two cost; on a wider net beside makeIntervalsBatch(backend="host") with 1 and 16 workers on the
           same boxes, wall-clock, one run (the 1-worker run on at most 256 boxes, scaled to nbox) - the only other route there
With --reach only the reach leg runs and profiles/split_timing_reach_<case>.json is written:
  reach    one bounds-only reachSplit (crown_backend "resident", corner_points, max_boxes 16384, max_depth 64) with frontier "host" and then
           "device" in this process; the directions are findReach2Dpoly's six normals on a two-output net, else e_j and -e_j of every
           output; tol_i = f (upper_i - incumbent_i of the root box alone), f the first of 0.25, 0.1, 0.05, 0.02 at which the host frontier
           visits at least 1 000 boxes, else the one with the most boxes visited.  Median of 5 runs after 1 warm run: total seconds,
           seconds["crown"], and for the device frontier the HIP-event time of its kernels; status, visited, levels, worst upper - lower
With --frontier only the frontier leg runs and profiles/split_timing_frontier_<case>.json is written:
  split    one bounds-only verifySplit (crown_backend "resident", literal_bounds, max_boxes 16384) of the literal
           y_0 - y_last <= s + f (c0 - s) with frontier "host" and then "device" in this process; f is the first of 0.25, 0.1, 0.05, 0.02 at
           which the host frontier visits at least 1 000 boxes, else the one with the most boxes visited.  Median of 5 runs after 1 warm
           run: total seconds, seconds["crown"], and for the device frontier the HIP-event time of its kernels; visited and levels
With --alpha only the optimised-slope leg runs and profiles/split_timing_alpha_<case>.json is written:
  bound    CrownBounder.bound at nbox = 256 with alpha_steps 0, 4 and 8 and 1 and 10 literals: wall-clock of the call and HIP-event time of
           its kernels (the plain one, and k_crown_alpha of csrc/crown_alpha.hpp behind it when alpha_steps > 0), median of 7 after 2 warm calls
  host     makeIntervalsBatch(backend="host", workers=16) on the same boxes with the same settings, wall-clock, one run
  split    one verifySplit (bounds only, literal_bounds, crown_backend "resident", at most 512 boxes) of the literal y_0 - y_last per
           alpha_steps 0, 4, 8 and 4 with alpha_inherit: verdict, visited, `seconds`
  with --no-host only `bound` runs, in the form of the --relu leg, and profiles/split_timing_alpha_bound_<case>.json is written instead:
           nbox = 1, 256 and 4096, one literal, alpha_steps 0 and 4, median, min and max of the HIP-event time over 7 calls after 2 warm
           ones - the rows a change of k_crown_alpha is compared on
With --resident only the resident leg runs and profiles/split_timing_resident_<case>.json is written:
  bound    CrownBounder.bound beside makeIntervalsBatch(backend="gpu") at nbox = 1, 16, 256: wall-clock of the call and HIP-event time
           of the launch, median of 7 after 2 warm calls - what keeping the network on the device saves per level of a split tree
  eval     CrownBounder.eval beside evalFeedFwdNetBatch at N = 1, 16, 256, the same way
  split    one verifySplit (bounds only, at most 256 boxes) with crown_backend "gpu" and with "resident": verdict, visited, `seconds`
With --nlit only the literal leg runs and profiles/split_timing_nlit_<case>.json is written:
  nlit     nnsdp_make_intervals_batch_lits at nbox = 256 with 0, 1 and 10 literals (y_0 - y_last, then seeded Gaussian normals): HIP-event
           time of the launch and wall-clock of the call, median of 7 after 2 warm launches - what the literal pass adds to a launch
Otherwise writes profiles/split_timing_<case>.json (or $SPLIT_TIMING_OUT/...).  Per case:
  crown    nnsdp_make_intervals_batch at nbox = 1, 256, 4096 sub-boxes of the root box: HIP-event time of the launch (median of 7 after 2
           warm launches) and the wall-clock of the whole call with its copies; beside it the host backend (nnsdp_make_intervals_activ per
           box) with 1 and 16 workers on the same boxes, wall-clock, one run (the 1-worker run on at most 256 boxes, scaled to nbox)
  split    one verifySplit of the literal y_0 <= s + 0.25 (c0 - s) (s: sampled maximum, c0: root cheap bound): verdict, visited, SDPs and
           the `seconds` breakdown crown / setup / solve / finish / total
Timings are host clocks of whole calls unless marked kernel; the GPU is shared, so expect a few per cent of spread."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-sdp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import helpers, nnsdp_amd as na


def case(name):
    if name in ("W10-D5", "W40-D20"):
        z = np.load(os.path.join(helpers.GOLDEN, "nets", f"scale-I2-O2-{name}.npz"))
        xdims = [int(v) for v in z["xdims"]]
        return na.FeedFwdNet(xdims=xdims, Ms=[np.array(z[f"M{k}"], dtype=np.float64) for k in range(len(xdims) - 1)]), np.full(2, 0.5), np.full(2, 1.5)
    if name == "5-100x4-5":
        return na.randomNetwork([5] + [100] * 4 + [5], seed=1234), np.full(5, 0.25), np.full(5, 0.35)
    if name == "acas-shape":
        return na.randomNetwork([5] + [50] * 6 + [5], seed=1234), np.full(5, 0.25), np.full(5, 0.35)
    raise SystemExit(f"unknown case {name}")


def sub_boxes(lo, hi, nbox, seed=0):
    rng = np.random.default_rng(seed)
    hw = (hi - lo)[:, None] / 16.0
    c = lo[:, None] + hw + rng.random((len(lo), nbox)) * ((hi - lo)[:, None] - 2 * hw)
    return c - hw, c + hw


def crown_rows(net, lo, hi):
    rows = []
    for nbox in (1, 256, 4096):
        blo, bhi = sub_boxes(lo, hi, nbox)
        ker, wall = [], []
        for i in range(9):
            t = time.perf_counter()
            *_, ms = na.makeIntervalsBatch(net, blo, bhi, backend="gpu", return_ms=True)
            if i >= 2:
                ker.append(ms); wall.append(1e3 * (time.perf_counter() - t))
        n1 = min(nbox, 256)
        t = time.perf_counter(); na.makeIntervalsBatch(net, blo[:, :n1], bhi[:, :n1], backend="host", workers=1); h1 = 1e3 * (time.perf_counter() - t) * nbox / n1
        t = time.perf_counter(); na.makeIntervalsBatch(net, blo, bhi, backend="host", workers=16); h16 = 1e3 * (time.perf_counter() - t)
        rows.append(dict(nbox=nbox, gpu_kernel_ms_median=statistics.median(ker), gpu_kernel_ms_min=min(ker), gpu_kernel_ms_max=max(ker),
                         gpu_call_ms_median=statistics.median(wall), host_1_worker_ms=h1, host_1_worker_boxes_timed=n1, host_16_workers_ms=h16,
                         gpu_call_over_host_16=statistics.median(wall) / h16, gpu_kernel_over_host_16=statistics.median(ker) / h16))
        print(rows[-1], flush=True)
    return rows


def nlit_rows(net, lo, hi, nbox=256):
    blo, bhi = sub_boxes(lo, hi, nbox)
    ny = net.xdims[-1]
    Cm = np.random.default_rng(1).normal(size=(10, ny))
    Cm[0] = 0.0; Cm[0, 0] = 1.0; Cm[0, ny - 1] -= 1.0
    rows = []
    for nlit in (0, 1, 10):
        ker, wall = [], []
        for i in range(9):
            t = time.perf_counter()
            *_, ms = na.makeIntervalsBatch(net, blo, bhi, backend="gpu", return_ms=True, normals=Cm[:nlit] if nlit else None)
            if i >= 2:
                ker.append(ms); wall.append(1e3 * (time.perf_counter() - t))
        rows.append(dict(nbox=nbox, nlit=nlit, gpu_kernel_ms_median=statistics.median(ker), gpu_kernel_ms_min=min(ker), gpu_kernel_ms_max=max(ker),
                         gpu_call_ms_median=statistics.median(wall)))
        rows[-1]["kernel_over_nlit0"] = rows[-1]["gpu_kernel_ms_median"] / rows[0]["gpu_kernel_ms_median"]
        print(rows[-1], flush=True)
    return rows


def _timed(call):
    """call() -> (..., kernel ms): medians of the wall-clock and of the kernel time over 7 calls after 2 warm ones"""
    ker, wall = [], []
    for i in range(9):
        t = time.perf_counter()
        *_, ms = call()
        if i >= 2:
            ker.append(ms); wall.append(1e3 * (time.perf_counter() - t))
    return statistics.median(wall), statistics.median(ker)


def resident_rows(net, lo, hi):
    bound, ev = [], []
    with na.CrownBounder(net) as bd:
        for n in (1, 16, 256):
            blo, bhi = sub_boxes(lo, hi, n)
            ow, ok = _timed(lambda: na.makeIntervalsBatch(net, blo, bhi, backend="gpu", return_ms=True))
            rw, rk = _timed(lambda: bd.bound(blo, bhi, return_ms=True))
            bound.append(dict(nbox=n, one_shot_call_ms_median=ow, one_shot_kernel_ms_median=ok, resident_call_ms_median=rw,
                              resident_kernel_ms_median=rk, resident_call_over_one_shot=rw / ow))
            print(bound[-1], flush=True)
            X = 0.5 * (blo + bhi)
            ow, ok = _timed(lambda: na.evalFeedFwdNetBatch(net, X, return_ms=True))
            rw, rk = _timed(lambda: bd.eval(X, return_ms=True))
            ev.append(dict(N=n, one_shot_call_ms_median=ow, one_shot_kernel_ms_median=ok, resident_call_ms_median=rw,
                           resident_kernel_ms_median=rk, resident_call_over_one_shot=rw / ow))
            print(ev[-1], flush=True)
        info = bd.info()
    nrm = np.zeros(net.xdims[-1]); nrm[0] = 1.0
    X = lo[:, None] + np.random.default_rng(0).random((len(lo), 20000)) * (hi - lo)[:, None]
    s = float((nrm @ na.evalFeedFwdNetBatch(net, X)).max())
    iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="gpu")
    c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
    h = s + 0.25 * (c0 - s)
    split = {}
    for backend in ("gpu", "resident"):
        r = na.verifySplit(net, lo, hi, [(nrm, h)], 0, na.AdmmSdpOptions(), na.SplitOptions(max_boxes=256, sdp_per_level=0, crown_backend=backend))
        split[backend] = dict(verdict=r.verdict, visited=r.visited, leaves=len(r.leaves), seconds=r.seconds)
        print(backend, split[backend], flush=True)
    return dict(bound=bound, eval=ev, handle=info, h=h, split=split)


def wide_rows(net, lo, hi):
    narrow_fits = max(net.xdims) <= 64
    rows = []
    with na.CrownBounder(net, max_width=128) as wd:
        for nbox in (1, 256, 4096):
            blo, bhi = sub_boxes(lo, hi, nbox)
            ww, wk = _timed(lambda: wd.bound(blo, bhi, return_ms=True))
            row = dict(nbox=nbox, wide_call_ms_median=ww, wide_kernel_ms_median=wk)
            if narrow_fits:
                with na.CrownBounder(net) as nr:
                    nw, nk = _timed(lambda: nr.bound(blo, bhi, return_ms=True))
                row.update(narrow_call_ms_median=nw, narrow_kernel_ms_median=nk, wide_kernel_over_narrow=wk / nk)
            else:
                n1 = min(nbox, 256)
                t = time.perf_counter(); na.makeIntervalsBatch(net, blo[:, :n1], bhi[:, :n1], backend="host", workers=1); h1 = 1e3 * (time.perf_counter() - t) * nbox / n1
                t = time.perf_counter(); na.makeIntervalsBatch(net, blo, bhi, backend="host", workers=16); h16 = 1e3 * (time.perf_counter() - t)
                row.update(host_1_worker_ms=h1, host_1_worker_boxes_timed=n1, host_16_workers_ms=h16, wide_call_over_host_16=ww / h16,
                           wide_kernel_over_host_16=wk / h16)
            rows.append(row)
            print(row, flush=True)
    return rows


def alpha_rows(net, lo, hi, nbox=256):
    blo, bhi = sub_boxes(lo, hi, nbox)
    ny = net.xdims[-1]
    Cm = np.random.default_rng(1).normal(size=(10, ny))
    Cm[0] = 0.0; Cm[0, 0] = 1.0; Cm[0, ny - 1] -= 1.0
    bound, host = [], []
    for nlit in (1, 10):
        with na.CrownBounder(net, Cm[:nlit]) as bd:
            for steps in (0, 4, 8):
                w, k = _timed(lambda: bd.bound(blo, bhi, return_ms=True, alpha_steps=steps))
                *_, lits, _ = bd.bound(blo, bhi, return_ms=True, alpha_steps=steps)
                gain = float(np.mean(lits.smax_plain - lits.smax)) if steps else 0.0
                bound.append(dict(nbox=nbox, nlit=nlit, alpha_steps=steps, call_ms_median=w, kernel_ms_median=k, mean_smax_gain=gain,
                                  device_bytes=bd.info()["device_bytes"]))
                print(bound[-1], flush=True)
        for steps in (0, 4, 8):
            t = time.perf_counter()
            na.makeIntervalsBatch(net, blo, bhi, backend="host", workers=16, normals=Cm[:nlit], alpha_steps=steps)
            host.append(dict(nbox=nbox, nlit=nlit, alpha_steps=steps, host_16_workers_ms=1e3 * (time.perf_counter() - t)))
            print(host[-1], flush=True)
    nrm = Cm[0]
    X = lo[:, None] + np.random.default_rng(0).random((len(lo), 20000)) * (hi - lo)[:, None]
    s = float((nrm @ na.evalFeedFwdNetBatch(net, X)).max())
    *_, lits = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="gpu", normals=nrm[None])
    c0 = float(lits.smax[0, 0])
    h = s + 0.25 * (c0 - s)
    split = {}
    for key, kw in (("0", {}), ("4", dict(alpha_steps=4)), ("8", dict(alpha_steps=8)), ("4+inherit", dict(alpha_steps=4, alpha_inherit=True))):
        r = na.verifySplit(net, lo, hi, [(nrm, h)], 0, na.AdmmSdpOptions(),
                           na.SplitOptions(max_boxes=512, sdp_per_level=0, crown_backend="resident", literal_bounds=True, **kw))
        split[key] = dict(verdict=r.verdict, visited=r.visited, leaves=len(r.leaves), seconds=r.seconds)
        print(key, split[key], flush=True)
    return dict(bound=bound, host=host, sampled_max=s, root_plain_smax=c0, h=h, split=split)


def frontier_rows(net, lo, hi, max_boxes=16384):
    nrm = np.zeros(net.xdims[-1]); nrm[0] = 1.0; nrm[-1] -= 1.0
    X = lo[:, None] + np.random.default_rng(0).random((len(lo), 20000)) * (hi - lo)[:, None]
    s = float((nrm @ na.evalFeedFwdNetBatch(net, X)).max())
    iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="gpu")
    c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())

    def run(f, frontier):
        return na.verifySplit(net, lo, hi, [(nrm, s + f * (c0 - s))], 0, na.AdmmSdpOptions(),
                              na.SplitOptions(max_boxes=max_boxes, sdp_per_level=0, crown_backend="resident", literal_bounds=True, frontier=frontier))

    tried = {}
    for f in (0.25, 0.1, 0.05, 0.02):
        tried[f] = run(f, "host").visited
        if tried[f] >= 1000:
            break
    f = f if tried[f] >= 1000 else max(tried, key=tried.get)
    out = dict(sampled_max=s, root_cheap_bound=c0, f=f, h=s + f * (c0 - s), max_boxes=max_boxes, host_visited_per_f={str(k): v for k, v in tried.items()})
    for frontier in ("host", "device"):
        runs = [run(f, frontier) for _ in range(6)][1:]
        r = runs[0]
        row = dict(verdict=r.verdict, visited=r.visited, leaves=len(r.leaves), levels=1 + max(lf.depth for lf in r.leaves),
                   total_s_median=statistics.median(q.seconds["total"] for q in runs), crown_s_median=statistics.median(q.seconds["crown"] for q in runs))
        if frontier == "device":
            row["kernel_s_median"] = statistics.median(q.seconds["kernel"] for q in runs)
        out[frontier] = row
        print(frontier, row, flush=True)
    out["host_over_device_total"] = out["host"]["total_s_median"] / out["device"]["total_s_median"]
    return out


def reach_rows(net, lo, hi, max_boxes=16384):
    ny = net.xdims[-1]
    if ny == 2:
        Cm = np.array([[np.cos(2 * np.pi * i / 6), np.sin(2 * np.pi * i / 6)] for i in range(6)])
    else:
        Cm = np.vstack([np.eye(ny), -np.eye(ny)])

    def run(tol, frontier, mb=max_boxes):
        return na.reachSplit(net, lo, hi, Cm, tol, split=na.SplitOptions(max_boxes=mb, max_depth=64, sdp_per_level=0, crown_backend="resident",
                                                                         corner_points=True, frontier=frontier))

    root = run(0.0, "host", 1)
    gap0 = root.upper - root.incumbent
    tried = {}
    for f in (0.25, 0.1, 0.05, 0.02):
        tried[f] = run(f * gap0, "host").visited
        if tried[f] >= 1000:
            break
    f = f if tried[f] >= 1000 else max(tried, key=tried.get)
    out = dict(nlit=len(Cm), root_upper=root.upper.tolist(), root_incumbent=root.incumbent.tolist(), f=f, tol=(f * gap0).tolist(), max_boxes=max_boxes,
               host_visited_per_f={str(k): v for k, v in tried.items()})
    for frontier in ("host", "device"):
        runs = [run(f * gap0, frontier) for _ in range(6)][1:]
        r = runs[0]
        row = dict(status=r.status, visited=r.visited, leaves=len(r.leaves), levels=1 + r.depth, worst_upper_minus_lower=float(np.max(r.upper - r.lower)),
                   total_s_median=statistics.median(q.seconds["total"] for q in runs), crown_s_median=statistics.median(q.seconds["crown"] for q in runs))
        if frontier == "device":
            row["kernel_s_median"] = statistics.median(q.seconds["kernel"] for q in runs)
        out[frontier] = row
        print(frontier, row, flush=True)
    out["host_over_device_total"] = out["host"]["total_s_median"] / out["device"]["total_s_median"]
    return out


def grid_roots(lo, hi, R):
    """R = 2^k cells of a regular grid of the box: the k halvings go to the coordinates in turn -> lo, hi (n0 x R)"""
    n0, k = len(lo), int(round(np.log2(R)))
    assert 2 ** k == R
    parts = [2 ** ((k + n0 - 1 - t) // n0) for t in range(n0)]
    idx = np.stack(np.meshgrid(*[np.arange(p) for p in parts], indexing="ij"), axis=0).reshape(n0, -1)
    w = (hi - lo) / np.array(parts)
    return lo[:, None] + idx * w[:, None], lo[:, None] + (idx + 1) * w[:, None]


def forest_rows(net, lo, hi, max_boxes=512, f=0.1, nsample=256):
    nrm = np.zeros(net.xdims[-1]); nrm[0] = 1.0; nrm[-1] -= 1.0
    kw = dict(literal_bounds=True, max_boxes=max_boxes, max_depth=24)
    rows = []
    with na.CrownBounder(net, nrm[None]) as cb:
        for R in (1, 16, 256, 4096):
            rlo, rhi = grid_roots(lo, hi, R)
            X = np.repeat(rlo, nsample, axis=1) + np.random.default_rng(0).random((len(lo), R * nsample)) * np.repeat(rhi - rlo, nsample, axis=1)
            s = (nrm @ cb.eval(X)).reshape(R, nsample).max(axis=1)
            iv = cb.bound(rlo, rhi)
            c0 = np.maximum(nrm[:, None] * iv[4], nrm[:, None] * iv[5]).sum(axis=0)
            hs = (s + f * (c0 - s))[None]

            def sequential():
                b0, t = cb.info()["bound_calls"], time.perf_counter()
                res = [cb.search(rlo[:, r], rhi[:, r], hs[:, r], **kw) for r in range(R)]
                wall = time.perf_counter() - t
                return dict(wall_ms=1e3 * wall, kernel_ms=sum(q["kernel_ms"] for q in res), levels=sum(q["depth"] + 1 for q in res),
                            bound_launches=cb.info()["bound_calls"] - b0, visited=sum(q["visited"] for q in res),
                            verdicts=[sum(q["verdict"] == v for q in res) for v in ("holds", "violated", "unknown")])

            def forest():
                b0, t = cb.info()["bound_calls"], time.perf_counter()
                q = cb.search_many(rlo, rhi, hs, **kw)
                wall = time.perf_counter() - t
                return dict(wall_ms=1e3 * wall, kernel_ms=q["kernel_ms"], levels=int(q["depth"].max()) + 1, bound_launches=cb.info()["bound_calls"] - b0,
                            visited=int(q["visited"].sum()), verdicts=[int(np.sum(q["verdict"] == v)) for v in ("holds", "violated", "unknown")])

            row = dict(R=R, max_boxes=max_boxes, f=f)
            for key, call in (("sequential", sequential), ("forest", forest)):
                runs = [call() for _ in range(2 if R == 4096 else 4)][1:]
                r = dict(runs[0], wall_ms=statistics.median(q["wall_ms"] for q in runs), kernel_ms=statistics.median(q["kernel_ms"] for q in runs))
                r["boxes_per_launch"] = r["visited"] / r["bound_launches"]
                row[key] = r
            assert row["sequential"]["visited"] == row["forest"]["visited"] and row["sequential"]["verdicts"] == row["forest"]["verdicts"]
            row["sequential_over_forest_wall"] = row["sequential"]["wall_ms"] / row["forest"]["wall_ms"]
            rows.append(row)
            print(row, flush=True)
        info = cb.info()
    return dict(forest=rows, handle=info)


def split_row(net, lo, hi):
    nrm = np.zeros(net.xdims[-1]); nrm[0] = 1.0
    X = lo[:, None] + np.random.default_rng(0).random((len(lo), 20000)) * (hi - lo)[:, None]
    s = float((nrm @ na.evalFeedFwdNetBatch(net, X)).max())
    iv = na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="gpu")
    c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
    h = s + 0.25 * (c0 - s)
    opts = na.AdmmSdpOptions(max_iters=4000, eps_rel=1e-5)
    so = na.SplitOptions(max_boxes=256, sdp_per_level=13, crown_backend="gpu")
    r = na.verifySplit(net, lo, hi, [(nrm, h)], 0, opts, so)
    by = [lf.proved_by for lf in r.leaves]
    row = dict(sampled_max=s, root_cheap_bound=c0, h=h, verdict=r.verdict, visited=r.visited, sdp_solves=r.sdp_solves, leaves=len(r.leaves),
               by_crown=by.count("crown"), by_sdp=by.count("sdp"), open=by.count(None), max_boxes=so.max_boxes, sdp_per_level=so.sdp_per_level,
               max_iters=opts.max_iters, seconds=r.seconds)
    print(row, flush=True)
    return row


def _spread(call, runs=7, warm=2):
    """call() -> (..., kernel ms): median, min and max of the kernel time and the median wall-clock over `runs` calls after `warm`"""
    ker, wall = [], []
    for i in range(runs + warm):
        t = time.perf_counter()
        *_, ms = call()
        if i >= warm:
            ker.append(ms); wall.append(1e3 * (time.perf_counter() - t))
    return dict(kernel_ms_median=statistics.median(ker), kernel_ms_min=min(ker), kernel_ms_max=max(ker), call_ms_median=statistics.median(wall))


def alpha_bound_rows(net, lo, hi):
    """bound at 1, 256 and 4096 boxes with alpha_steps 0 and 4, one literal y_0 - y_last, on one bounder"""
    ny = net.xdims[-1]
    Cm = np.zeros((1, ny)); Cm[0, 0] = 1.0; Cm[0, ny - 1] -= 1.0
    rows = []
    with na.CrownBounder(net, Cm) as bd:
        for n in (1, 256, 4096):
            blo, bhi = sub_boxes(lo, hi, n)
            rows.append(dict(nbox=n, **{f"alpha_steps{T}": _spread(lambda: bd.bound(blo, bhi, return_ms=True, alpha_steps=T)) for T in (0, 4)}))
            print(rows[-1], flush=True)
    return rows


def relu_bound_rows(net, lo, hi):
    """bound_nodes at 1, 256 and 4096 nodes (sub-boxes of the root, 20 % of the neurons forced to the pattern of a seeded point) with 0 and
    16 multiplier steps, beside CrownBounder.bound on the same boxes in the same process; one literal y_0 - y_last"""
    import relu_split_common as rs
    ny = net.xdims[-1]
    Cm = np.zeros((1, ny)); Cm[0, 0] = 1.0; Cm[0, ny - 1] -= 1.0
    rows = []
    with na.CrownBounder(net, Cm) as bd:
        for n in (1, 256, 4096):
            blo, bhi = sub_boxes(lo, hi, n)
            rng = np.random.default_rng(n)
            asg = np.stack([rs.node_from_point(net, blo[:, b], bhi[:, b], rng, 0.2)[1] for b in range(n)], 1)
            row = dict(nnode=n, bound=_spread(lambda: bd.bound(blo, bhi, return_ms=True)))
            for T in (0, 16):
                row[f"bound_nodes_steps{T}"] = _spread(lambda: bd.bound_nodes(blo, bhi, asg, steps=T, return_ms=True))
                row[f"kernel_over_bound_steps{T}"] = row[f"bound_nodes_steps{T}"]["kernel_ms_median"] / row["bound"]["kernel_ms_median"]
            rows.append(row)
            print(row, flush=True)
    return rows


def relu_search_rows():
    """whole searches: verifyReluSplit (crown_backend "resident", 16 steps) against verifySplit (crown_backend "resident", literal_bounds,
    centre points, bounds only) on the literal y_0 - y_1 <= h over [-0.5, 0.5]^n0 of two seeded nets; L is the largest of 4096 sampled
    values and the centre's, c0 the literal's plain bound on the root; 5 runs each after 1 warm run"""
    import literal_common as lc
    rows = []
    for xdims, seed, f, cap in (([16, 16, 16, 2], 7, 0.5, 16384), ([12, 16, 16, 2], 5, 0.2, 16384)):
        net = lc.random_net(xdims, seed)
        n0 = xdims[0]
        lo, hi, nrm = -0.5 * np.ones(n0), 0.5 * np.ones(n0), np.array([1.0, -1.0])
        X = np.concatenate([np.zeros((n0, 1)), lo[:, None] + np.random.default_rng(0).random((n0, 4096))], axis=1)
        L = float((nrm @ na.evalFeedFwdNet(net, X)).max())
        c0 = float(na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="host", normals=nrm[None, :])[-1].smax[0, 0])
        h = L + f * (c0 - L)
        row = dict(xdims=xdims, seed=seed, L=L, c0=c0, h=h)
        for label, run in (("relu_split", lambda: na.verifyReluSplit(net, lo, hi, [(nrm, h)], na.ReluSplitOptions(max_nodes=cap, crown_backend="resident"))),
                           ("input_split", lambda: na.verifySplit(net, lo, hi, [(nrm, h)], 0, na.AdmmSdpOptions(),
                                                                  na.SplitOptions(sdp_per_level=0, max_boxes=cap, max_depth=64, crown_backend="resident",
                                                                                  literal_bounds=True)))):
            ms, res = [], None
            for i in range(6):
                t = time.perf_counter()
                res = run()
                if i >= 1:
                    ms.append(1e3 * (time.perf_counter() - t))
            row[label] = dict(verdict=res.verdict, visited=int(res.visited), ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))
        rows.append(row)
        print(row, flush=True)
    return rows


def relu_frontier_rows():
    """the two whole-search instances of relu_search_rows, crown_backend "resident", with the host frontier against the device frontier
    (CrownBounder.search_nodes) in one process; 5 runs each after 1 warm run, and the device frontier's HIP-event time"""
    import literal_common as lc
    rows = []
    for xdims, seed, f, cap in (([16, 16, 16, 2], 7, 0.5, 16384), ([12, 16, 16, 2], 5, 0.2, 16384)):
        net = lc.random_net(xdims, seed)
        n0 = xdims[0]
        lo, hi, nrm = -0.5 * np.ones(n0), 0.5 * np.ones(n0), np.array([1.0, -1.0])
        X = np.concatenate([np.zeros((n0, 1)), lo[:, None] + np.random.default_rng(0).random((n0, 4096))], axis=1)
        L = float((nrm @ na.evalFeedFwdNet(net, X)).max())
        c0 = float(na.makeIntervalsBatch(net, lo[:, None], hi[:, None], backend="host", normals=nrm[None, :])[-1].smax[0, 0])
        h = L + f * (c0 - L)
        row = dict(xdims=xdims, seed=seed, L=L, c0=c0, h=h, max_nodes=cap)
        for frontier in ("host", "device"):
            ms, ker, res = [], [], None
            for i in range(6):
                t = time.perf_counter()
                res = na.verifyReluSplit(net, lo, hi, [(nrm, h)], na.ReluSplitOptions(max_nodes=cap, crown_backend="resident", frontier=frontier))
                if i >= 1:
                    ms.append(1e3 * (time.perf_counter() - t)); ker.append(1e3 * res.seconds.get("kernel", 0.0))
            row[frontier] = dict(verdict=res.verdict, visited=int(res.visited), levels=int(res.depth) + 1, ms_median=statistics.median(ms),
                                 ms_min=min(ms), ms_max=max(ms))
            if frontier == "device":
                row[frontier].update(kernel_ms_median=statistics.median(ker), kernel_ms_min=min(ker), kernel_ms_max=max(ker))
        assert (row["host"]["verdict"], row["host"]["visited"]) == (row["device"]["verdict"], row["device"]["visited"])
        row["host_over_device"] = row["host"]["ms_median"] / row["device"]["ms_median"]
        rows.append(row)
        print(row, flush=True)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--relu-frontier" in args:
        # the node-frontier leg: profiles/split_timing_relu_frontier.json
        out_dir = os.environ.get("SPLIT_TIMING_OUT", os.path.join(ROOT, "profiles"))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "split_timing_relu_frontier.json"), "w") as fh:
            json.dump(dict(search=relu_frontier_rows()), fh, indent=1)
        sys.exit(0)
    if "--relu" in args:
        # the ReLU-split leg: profiles/split_timing_relu.json; cases W10-D5 and W40-D20 unless named
        out_dir = os.environ.get("SPLIT_TIMING_OUT", os.path.join(ROOT, "profiles"))
        os.makedirs(out_dir, exist_ok=True)
        names = [a for a in args if not a.startswith("--")] or ["W10-D5", "W40-D20"]
        res = dict(bound={name: relu_bound_rows(*case(name)) for name in names})
        if "--no-search" not in args:
            res["search"] = relu_search_rows()
        with open(os.path.join(out_dir, "split_timing_relu.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        sys.exit(0)
    lit_leg, res_leg, alpha_leg, frontier_leg, reach_leg, wide_leg = ("--nlit" in args, "--resident" in args, "--alpha" in args, "--frontier" in args,
                                                                      "--reach" in args, "--wide" in args)
    forest_leg = "--forest" in args
    names = [a for a in args if not a.startswith("--")] or \
        (["W40-D20", "acas-shape", "5-100x4-5"] if wide_leg else ["W10-D5", "acas-shape"] if forest_leg else ["W10-D5", "W40-D20", "acas-shape"])
    out_dir = os.environ.get("SPLIT_TIMING_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    for name in names:
        net, lo, hi = case(name)
        if forest_leg:
            with open(os.path.join(out_dir, f"split_timing_forest_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, **forest_rows(net, lo, hi)), fh, indent=1)
            continue
        if wide_leg:
            with open(os.path.join(out_dir, f"split_timing_wide_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, bound=wide_rows(net, lo, hi)), fh, indent=1)
            continue
        if reach_leg:
            with open(os.path.join(out_dir, f"split_timing_reach_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, **reach_rows(net, lo, hi)), fh, indent=1)
            continue
        if frontier_leg:
            with open(os.path.join(out_dir, f"split_timing_frontier_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, **frontier_rows(net, lo, hi)), fh, indent=1)
            continue
        if alpha_leg and "--no-host" in args:
            with open(os.path.join(out_dir, f"split_timing_alpha_bound_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, bound=alpha_bound_rows(net, lo, hi)), fh, indent=1)
            continue
        if alpha_leg:
            with open(os.path.join(out_dir, f"split_timing_alpha_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, **alpha_rows(net, lo, hi)), fh, indent=1)
            continue
        if res_leg:
            with open(os.path.join(out_dir, f"split_timing_resident_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, **resident_rows(net, lo, hi)), fh, indent=1)
            continue
        if lit_leg:
            with open(os.path.join(out_dir, f"split_timing_nlit_{name}.json"), "w") as fh:
                json.dump(dict(case=name, xdims=net.xdims, nlit=nlit_rows(net, lo, hi)), fh, indent=1)
            continue
        res = dict(case=name, xdims=net.xdims, crown=crown_rows(net, lo, hi), split=split_row(net, lo, hi))
        with open(os.path.join(out_dir, f"split_timing_{name}.json"), "w") as fh:
            json.dump(res, fh, indent=1)
