"""Writes tests/golden/tanh_ranges.json: enclosed maxima of small Tanh networks by tests/tanh_truth.py (CPU only; numpy, scipy, mpmath).

    python tests/golden/make_tanh_ranges.py            every case, one process per (net, box)
    python tests/golden/make_tanh_ranges.py --check    nothing is written: the regenerated w and v against the file's, to 1e-12

The nets are the Tanh copies of the two small nets of tests/golden/exact_ranges.json (the recipe of literal_common.random_net, restated
here so that nothing of the product is imported; tests/test_tanh_truth_cpu.py holds the restatement to the product's nets bit for bit).
The boxes are that file's root, edge0, stable, point and small-a, read from it; the rows are its stored rows (exact_common.stored_rows,
restated as well).  Per net, box and row: x (a point of the box), w = c' f(x) (mpmath, rounded down: attained, so w <= the true
maximum), v (interval branch and bound, rounded up: v >= the true maximum) and the gap (v - w) / (1 + |v|) reached.  The aim is GAP;
a row that does not get there within CAP_SECONDS keeps the smallest gap reached, and the tests read the gap from the file.
A row with v < w is refused."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tanh_truth as tt          # noqa: E402

FIXTURE = os.path.join(HERE, "tanh_ranges.json")
SOURCE = os.path.join(HERE, "exact_ranges.json")
NETS = {"2-8-8-2": ([2, 8, 8, 2], 1), "3-10-10-3": ([3, 10, 10, 3], 2)}
BOXES = ("root", "edge0", "stable", "point", "small-a")
GAP = 1e-6
CAP_SECONDS = 10 * 60


def net_Ms(name):
    xdims, seed = NETS[name]
    rng = np.random.default_rng(seed)
    return [rng.normal(0.0, 1.0 / np.sqrt(xdims[k] + 1), size=(xdims[k + 1], xdims[k] + 1)) for k in range(len(xdims) - 1)]


def rows(name):
    """literal_common.literal_rows(ny, 7, seed + 100), then e_j and -e_j for every output"""
    xdims, seed = NETS[name]
    ny = xdims[-1]
    C = np.random.default_rng(seed + 100).normal(size=(64, ny))
    C[:4] = 0.0
    C[0, 0] += 1.0
    C[0, ny - 1] -= 1.0
    C[1, 0] = 1.0
    C[2, 0] = -1.0
    return np.vstack([C[:7], np.eye(ny), -np.eye(ny)])


def job(args):
    name, bname, lo, hi = args
    t0 = time.time()
    Ms, C = net_Ms(name), rows(name)
    out = dict(name=bname, lo=lo, hi=hi, x=[], w=[], v=[], gap=[], boxes=[])
    for c in C:
        x, w = tt.attained_max(Ms, lo, hi, c)
        e = tt.enclosed_max(Ms, lo, hi, c, w, GAP, deadline=time.monotonic() + CAP_SECONDS)
        assert e.v >= w, (name, bname, c, e.v, w)
        out["x"].append(x.tolist())
        out["w"].append(w)
        out["v"].append(e.v)
        out["gap"].append(e.gap)
        out["boxes"].append(e.boxes)
    return name, out, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--workers", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    with open(SOURCE) as fh:
        src = json.load(fh)["cases"]
    jobs = []
    for name in NETS:
        have = {bx["name"]: bx for bx in src[name]["boxes"]}
        jobs += [(name, bn, have[bn]["lo"], have[bn]["hi"]) for bn in BOXES if bn in have]
    cases = {}
    with ProcessPoolExecutor(max_workers=args.workers) as pool:
        for name, bx, secs in pool.map(job, jobs):
            cases.setdefault(name, dict(recipe=dict(xdims=NETS[name][0], seed=NETS[name][1], net="literal_common.random_net, as a Tanh net",
                                                    rows="exact_common.stored_rows"), boxes=[]))["boxes"].append(bx)
            print(f"{name} {bx['name']}: worst gap {max(bx['gap']):.3e}, {sum(bx['boxes'])} boxes, {secs:.1f} s", flush=True)
    for name, cs in cases.items():
        for bx in cs["boxes"]:
            assert all(v >= w for v, w in zip(bx["v"], bx["w"])), (name, bx["name"])
    if args.check:
        with open(FIXTURE) as fh:
            old = json.load(fh)["cases"]
        for name, cs in cases.items():
            for bx, ob in zip(cs["boxes"], old[name]["boxes"]):
                assert bx["name"] == ob["name"]
                for k in ("w", "v"):
                    assert np.abs(np.array(bx[k]) - np.array(ob[k])).max() <= 1e-12, (name, bx["name"], k)
            print(f"{name}: w and v equal to the file's to 1e-12")
        return
    header = dict(generator="tests/golden/make_tanh_ranges.py", oracle="tests/tanh_truth.py", gap_aim=GAP, cap_seconds=CAP_SECONDS,
                  note="w <= true maximum <= v per row; gap = (v - w) / (1 + |v|) as reached")
    with open(FIXTURE, "w") as fh:
        json.dump(dict(header=header, cases=cases), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {FIXTURE}")


if __name__ == "__main__":
    main()
