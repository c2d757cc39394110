"""Writes tests/golden/exact_ranges.json: exact ranges of small ReLU networks by tests/exact_range.py (CPU only, numpy + scipy).

    python tests/golden/make_exact_ranges.py                 every case, one process per (case, box)
    python tests/golden/make_exact_ranges.py --cases a,b     only these cases; the others are kept as the file has them
    python tests/golden/make_exact_ranges.py --check         nothing is written: the regenerated values against the file's, to 1e-12

Networks are stored as recipes (xdims, seed) of literal_common.random_net, or as the name of the W10-D5 fixture; never as weights.
Per box and stored row: v (the LP value), w (the long-double forward pass at the argmax / argmin) and the argmax / argmin, for the
maximum and the minimum, with the region and LP counts of the enumerations.  The rows are exact_common.case_rows (the literal rows),
and on the two small nets every hidden neuron's pre-activation and post-activation, in the order of acxmin / acymin.

A case whose enumeration passes CAP_SECONDS is left out whole and named in the header; no partial value is written.
Before anything is written every value must satisfy |v - w| <= 1e-9 (1 + |v|)."""
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

import exact_common as ec          # noqa: E402
import exact_range as er           # noqa: E402

CAP_SECONDS = 30 * 60
BIG = {"holds": (-1.0, 1.0), "W10-D5": (0.5, 1.5), "violated": (-1.0, 1.0)}          # root box only


def hidden_pre(Ms, X):
    """pre-activations of every hidden layer at the columns of X"""
    out = []
    for Mk in Ms[:-1]:
        z = Mk[:, :-1] @ X + Mk[:, -1:]
        out.append(z)
        X = np.maximum(z, 0.0)
    return np.concatenate(out)


def edge_box(Ms, rng):
    """a box of half-width 0.25 whose one edge is moved so that the upper bound of a first-layer pre-activation over the box is exactly
    0.0 in float64, both as W c + |W| r + b (the backward pass) and as hi' W+ + lo' W- + b (interval arithmetic) -> lo, hi, neuron"""
    W, b = Ms[0][:, :-1], Ms[0][:, -1]
    for _ in range(2000):
        c = rng.uniform(-0.5, 0.5, size=W.shape[1])
        for i in range(W.shape[0]):
            q = int(np.argmax(np.abs(W[i])))
            lo, hi = c - 0.25, c + 0.25
            edge = hi if W[i, q] > 0 else lo
            rest = float(np.maximum(W[i], 0) @ hi + np.minimum(W[i], 0) @ lo + b[i]) - W[i, q] * edge[q]
            t = -rest / W[i, q]
            if not (lo[q] + 0.05 < t if W[i, q] > 0 else t < hi[q] - 0.05) or abs(t) > 1.0:
                continue
            for _ulp in range(-64, 65):
                edge[q] = t
                for _ in range(abs(_ulp)):
                    edge[q] = np.nextafter(edge[q], np.inf if _ulp > 0 else -np.inf)
                cc, rr = (hi + lo) / 2.0, (hi - lo) / 2.0
                u1 = W[i] @ cc + np.abs(W[i]) @ rr + b[i]
                u2 = hi @ np.maximum(W[i], 0.0) + lo @ np.minimum(W[i], 0.0) + b[i]
                if u1 == 0.0 and u2 == 0.0:
                    return lo.copy(), hi.copy(), i
    raise RuntimeError("no box with an exactly zero upper bound found")


def small_boxes(name):
    """the eight boxes of a small case (exact_common.BOX_NAMES), seeded"""
    xdims, seed = ec.SMALL[name]
    Ms, n0 = ec.case_net(name).Ms, xdims[0]
    rng = np.random.default_rng(seed + 500)
    out = [(-np.ones(n0), np.ones(n0))]
    for hw, span in ((0.5, 0.5), (0.5, 0.5), (0.05, 0.95), (0.05, 0.95)):
        c = rng.uniform(-span, span, size=n0)
        out.append((c - hw, c + hw))
    while True:                                                   # every neuron stable on the box: |z| at the centre far above L * 1e-6
        c = rng.uniform(-1.0, 1.0, size=n0)
        if np.abs(hidden_pre(Ms, c[:, None])).min() >= 1e-3:
            break
    out.append((c - 1e-6, c + 1e-6))
    c = rng.uniform(-1.0, 1.0, size=n0)
    out.append((c.copy(), c.copy()))
    out.append(edge_box(Ms, rng)[:2])
    return out


def block(top, bot):
    return dict(vmax=top.v.tolist(), wmax=top.w.tolist(), xmax=top.x.tolist(), vmin=bot.v.tolist(), wmin=bot.w.tolist(), xmin=bot.x.tolist())


def join(blocks):
    return {k: sum((b[k] for b in blocks), []) for k in ec.BLOCK_KEYS}


def job(args):
    """one (case, box): the dict of the box, or None where the deadline passed"""
    name, bname, lo, hi = args
    t0 = time.time()
    deadline = time.monotonic() + CAP_SECONDS
    Ms, C = ec.case_net(name).Ms, ec.case_rows(name)
    out = dict(name=bname, lo=lo.tolist(), hi=hi.tolist(), regions=[], lps=0)
    try:
        if name in ec.SMALL:
            pre, post = [], []
            for k in range(len(Ms)):                              # depth k: the regions of hidden layers 0 .. k-1
                d = Ms[k].shape[1] - 1
                last = Ms[k] if k == 0 else np.vstack([np.hstack([np.eye(d), np.zeros((d, 1))]), Ms[k]])
                net_k = list(Ms[:k]) + [last]
                s = er.regions(net_k, lo, hi, deadline)
                rows = np.eye(last.shape[0])
                if k == len(Ms) - 1:
                    rows = np.vstack([rows[:d], C @ rows[d:]])
                top, bot = er.exact_range(net_k, lo, hi, rows, search=s)
                cut = lambda r, a, b: er.ExactMax(r.v[a:b], r.x[a:b], r.w[a:b], r.regions, r.lps)
                n = rows.shape[0]
                if k > 0:
                    post.append(block(cut(top, 0, d), cut(bot, 0, d)))
                if k < len(Ms) - 1:
                    pre.append(block(cut(top, d if k else 0, n), cut(bot, d if k else 0, n)))
                else:
                    out["lit"] = block(cut(top, d, n), cut(bot, d, n))
                out["regions"].append(len(s.leaves))
                out["lps"] += s.lps
            out["pre"], out["post"] = join(pre), join(post)
        else:
            s = er.regions(Ms, lo, hi, deadline)
            top, bot = er.exact_range(Ms, lo, hi, C, search=s)
            out["lit"] = block(top, bot)
            out["regions"].append(len(s.leaves))
            out["lps"] += s.lps
    except TimeoutError:
        return name, None, time.time() - t0
    return name, out, time.time() - t0


def check_attained(name, bx):
    for blk in ("lit", "pre", "post"):
        if blk in bx:
            for v, w in ((bx[blk]["vmax"], bx[blk]["wmax"]), (bx[blk]["vmin"], bx[blk]["wmin"])):
                v, w = np.array(v), np.array(w)
                bad = np.abs(v - w) > er.V_W_BOUND * (1.0 + np.abs(v))
                assert not bad.any(), (name, bx["name"], blk, v[bad], w[bad])


def numbers(obj):
    if isinstance(obj, dict):
        return [x for k in sorted(obj) for x in numbers(obj[k])]
    if isinstance(obj, list):
        return [x for v in obj for x in numbers(v)]
    return [float(obj)] if isinstance(obj, (int, float)) else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(ec.SMALL) + list(BIG)))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    names = args.cases.split(",")
    jobs = []
    for name in names:
        if name in ec.SMALL:
            jobs += [(name, bn, lo, hi) for bn, (lo, hi) in zip(ec.BOX_NAMES, small_boxes(name))]
        else:
            n0 = ec.case_net(name).xdims[0]
            jobs.append((name, "root", np.full(n0, BIG[name][0]), np.full(n0, BIG[name][1])))
    cases, left_out, seconds = {}, [], {}
    with ProcessPoolExecutor(max_workers=args.workers) as pool:
        for name, bx, secs in pool.map(job, jobs):
            seconds[name] = seconds.get(name, 0.0) + secs
            if bx is None:
                left_out.append(name)
                continue
            check_attained(name, bx)
            cases.setdefault(name, dict(boxes=[]))["boxes"].append(bx)
            print(f"{name} {bx['name']}: regions {bx['regions']}, {bx['lps']} LPs, {secs:.1f} s", flush=True)
    for name in left_out:
        cases.pop(name, None)
    for name, cs in cases.items():
        cs["recipe"] = dict(xdims=ec.case_net(name).xdims, seed=ec.SMALL[name][1] if name in ec.SMALL else {"holds": 14, "violated": 31}.get(name),
                            net="literal_common.fixture_net" if name == "W10-D5" else "literal_common.random_net", rows="exact_common.case_rows")
        cs["seconds"] = round(seconds[name], 1)
    if os.path.exists(ec.FIXTURE):                                # read only now: the file as it is when this run has finished
        with open(ec.FIXTURE) as fh:
            old = json.load(fh)
    else:
        old = dict(header={}, cases={})
    if args.check:
        for name, cs in cases.items():
            a, b = np.array(numbers(cs["boxes"])), np.array(numbers(old["cases"][name]["boxes"]))
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12, (name, np.abs(a - b).max())
            print(f"{name}: {a.size} numbers equal to the file's to 1e-12")
        return
    merged = {k: v for k, v in old.get("cases", {}).items() if k not in names}
    merged.update(cases)
    gone = sorted((set(old.get("header", {}).get("left_out", [])) - set(cases)) | set(left_out))
    header = dict(generator="tests/golden/make_exact_ranges.py", oracle="tests/exact_range.py", cap_seconds=CAP_SECONDS, left_out=gone,
                  note="a case in left_out passed the cap: nothing of it is stored")
    with open(ec.FIXTURE, "w") as fh:
        json.dump(dict(header=header, cases={k: merged[k] for k in sorted(merged)}), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {ec.FIXTURE}: cases {sorted(merged)}, left out {gone}")


if __name__ == "__main__":
    main()
