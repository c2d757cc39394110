"""Digests of what the two projected-gradient optimisers of the CROWN bounder return - the slopes (k_crown_alpha, lits_alpha) and the
multipliers of a ReLU-split node (k_crown_beta, make_intervals_nodes) - on the cases of their own test files: the gate of a change
that only moves their code (csrc/crown_opt.hpp, csrc/intervals.hpp), which must return the same bytes.
  gpu   slopes: every case of crown_alpha_common.cases() at every T of its STEPS, without alpha0 and with the seeded uniform alpha0 of
        tests/test_crown_alpha_gpu.py; every array of KEYS + A_KEYS of raw_gpu.  multipliers: every case of
        relu_split_common.kernel_cases() at every T of its STEPS, the 17-literal case on net 0 and the 64-literal case on net 1 of
        test_more_literals_than_one_tile at T = 3, and the all-zero assignment at T = 1 (the stationary break); every field of NodeBounds
  host  the same cases and steps through makeIntervalsBatch(backend="host", normals=C, alpha_steps=T[, alpha0]) (the six arrays, the
        four fields of the literal bounds - the smaller of plain and optimised - and smax_plain, alpha, best_step where it has them),
        then the routine's own outputs (crown_alpha_common.raw_host, every array of KEYS + A_KEYS: the optimised bound also where it
        loses to the plain one, and at T = 0 without alpha0, where makeIntervalsBatch does not call it); makeIntervalsNodes (every
        field of NodeBounds)
A record is the SHA-256 of the arrays' bytes in that order.
usage: python tools/crown_opt_bits.py --record [--host-only] [out.json]   on a build of the commit to compare against (default
           tests/golden/crown_opt_bits_parent.json; --host-only keeps the file's gpu section)
       python tools/crown_opt_bits.py [--host-only]                       compares the loaded build with the record"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import crown_alpha_common as ca
import literal_common as lc
import relu_split_common as rs

GOLDEN = os.path.join(ROOT, "tests", "golden", "crown_opt_bits_parent.json")
MORE_LITERALS = ((0, 17), (1, 64))         # (net, literals) of test_more_literals_than_one_tile, at T = 3


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def slope_cases():
    """(id, case index, T, alpha0 or None)"""
    out = []
    for n, (net, lo, _, Cm) in enumerate(ca.cases()):
        shape = (Cm.shape[0], sum(net.xdims[1:-1]), lo.shape[1])
        for T in ca.STEPS:
            out.append((f"slopes-{n}-T{T}", n, T, None))
            out.append((f"slopes-{n}-T{T}-alpha0", n, T, ca.f32_uniform(shape, 77 + n)))
    return out


def node_cases():
    """(id, net, lo, hi, assign, C, T)"""
    out = []
    for n, cs in enumerate(rs.kernel_cases()):
        out += [(f"nodes-{n}-T{T}", cs["net"], cs["lo"], cs["hi"], cs["assign"], cs["C"], T) for T in rs.STEPS]
        out.append((f"nodes-{n}-free-T1", cs["net"], cs["lo"], cs["hi"], np.zeros_like(cs["assign"]), cs["C"], 1))
    for n, nlit in MORE_LITERALS:
        cs = rs.kernel_cases()[n]
        out.append((f"nodes-{n}-nlit{nlit}-T3", cs["net"], cs["lo"], cs["hi"], cs["assign"], lc.literal_rows(cs["net"].xdims[-1], nlit, 700 + n), 3))
    return out


def case_ids():
    return [c[0] for c in slope_cases()] + [c[0] for c in node_cases()]


def gpu_digests():
    import nnsdp_amd as na
    out = {}
    for cid, n, T, a0 in slope_cases():
        net, lo, hi, Cm = ca.cases()[n]
        with na.CrownBounder(net, Cm) as bd:
            r = ca.raw_gpu(bd, lo, hi, T, alpha0=a0)
        out[cid] = _sha(r[k] for k in ca.KEYS + ca.A_KEYS)
    for cid, net, lo, hi, asg, Cm, T in node_cases():
        with na.CrownBounder(net, Cm) as bd:
            out[cid] = _sha(bd.bound_nodes(lo, hi, asg, steps=T))
    return out


def host_digests():
    import nnsdp_amd as na
    out = {}
    for cid, n, T, a0 in slope_cases():
        net, lo, hi, Cm = ca.cases()[n]
        *six, lits = na.makeIntervalsBatch(net, lo, hi, backend="host", normals=Cm, alpha_steps=T, alpha0=a0)
        extra = [getattr(lits, k, None) for k in ("smax_plain", "alpha", "best_step")]     # (as a tuple it is four fields)
        raw = ca.raw_host(net, lo, hi, Cm, T, alpha0=a0)
        out[cid] = _sha([v for v in six + list(lits) + extra if v is not None] + [raw[k] for k in ca.KEYS + ca.A_KEYS])
    for cid, net, lo, hi, asg, Cm, T in node_cases():
        out[cid] = _sha(na.makeIntervalsNodes(net, lo, hi, asg, Cm, steps=T))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    host_only = "--host-only" in args
    paths = [a for a in args if not a.startswith("--")]
    if "--record" in args:
        path = paths[0] if paths else GOLDEN
        table = {}
        if host_only and os.path.exists(path):
            with open(path) as f:
                table = json.load(f)
        if not host_only:
            table["gpu"] = gpu_digests()
        table["host"] = host_digests()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print({k: len(v) for k, v in table.items()}, "records ->", path)
        sys.exit(0)
    with open(GOLDEN) as f:
        want = json.load(f)
    bad = []
    for section, fn in (("host", host_digests),) + (() if host_only else (("gpu", gpu_digests),)):
        got = fn()
        bad += [(section, k) for k in case_ids() if got[k] != want[section][k]]
    print(f"{len(case_ids())} cases per section, {len(bad)} differ", bad)
    sys.exit(1 if bad else 0)
