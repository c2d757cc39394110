"""Shared by the embedded exact-range tests (test_exact_embedded_cpu.py, test_exact_embedded_gpu.py): `embed` places a small net inside
a wide one without changing its function, so that the exact extrema, witnesses and verdict thresholds of tests/golden/exact_ranges.json
apply to networks of width 17 to 128; the layouts of both files, their seeds, and the cases built on them (computed once, shared, never
modified).  Numpy only; nothing here needs a GPU."""
import numpy as np

import crown_tanh_common as tc
import exact_common as ec
import literal_common as lc
import nnsdp_amd as na

KINDS = ("scatter", "split", "cancel")
# small net -> layouts; a wide layout has a hidden layer above 64 (the wide bounder), a narrow one more than one 16-wide tile and none
# above 64 (k_crown_batch, k_crown_resident, k_crown_alpha)
WIDE = {"2-8-8-2": ([127, 65],), "3-10-10-3": ([65, 128], [128, 128])}
NARROW = {"2-8-8-2": ([17, 64],), "3-10-10-3": ([48, 33],)}
SPLIT_ONLY = ([128, 128],)
# The first and the last row of each 64-row slab, both sides of the 16-column tile boundaries in both column tiles of a wave (tiles w and
# w + 4), and the k tail.  A layer has fewer live neurons than positions named here, so they are taken in this order: the first six as
# far as the layer has them, then the second list rotated by three per hidden layer, so that two wide layers of one net take different ones
FIRST = (0, -1, 63, 64, 15, 16)
SECOND = (79, 80, 65, 112, 111, 126)
_cache = {}


def live_positions(D, n, k, rng):
    """n distinct positions of a layer of width D, hidden layer k (0-based): FIRST and SECOND in order while they last (those the layer
    has), the rest drawn; which neuron gets which position is drawn too"""
    assert n <= D
    want = [D - 1 if p < 0 else p for p in FIRST] + [SECOND[(3 * k + j) % len(SECOND)] for j in range(len(SECOND))]
    pos = []
    for p in want:
        if p < D and p not in pos and len(pos) < n:
            pos.append(p)
    free = np.array([p for p in range(D) if p not in pos], dtype=np.int64)
    pos += list(rng.permutation(free)[:n - len(pos)])
    return np.array(pos, dtype=np.int64)[rng.permutation(n)]


def multiplicities(n, D):
    """"split": every neuron once, then the smallest count (the first of them) doubled while the layer has room"""
    m = np.ones(n, dtype=np.int64)
    while True:
        i = int(np.argmin(m))
        if m.sum() + m[i] > D:
            return m
        m[i] *= 2


def embed(net, widths, kind, seed, full=False):
    """-> (wide_net, live): the net with hidden widths `widths` and the same function; live[k][i] is the position of neuron i of hidden
    layer k (its first copy).  Input and output layers are untouched, `activ` is kept.
    "scatter": the live neurons at chosen positions, every other neuron a zero row (bias included) and a zero outgoing column.
    "split": the free positions are copies of live neurons, m_i of neuron i (a power of two, so the outgoing weights w / m_i are exact);
    positions left over are zero filler.
    "cancel": the free positions in pairs; both members have one seeded incoming row over the live columns and a bias, N(0, 1 / (d_live + 1)),
    and outgoing columns + g and - g into every row of the next layer that is not a zero leftover, g ~ N(0, 1 / (D + 1)).  The function
    is unchanged, the CROWN bounds are not (the relaxations of an unstable pair do not cancel).  Every member of a pair has live inputs:
    a neuron fed by pairs alone would have symmetric bounds (-x, x), an upper slope of 0.5 up to rounding and a lower slope that flips
    between float64 and long double.  An unpaired leftover is a zero row and a zero column.
    full=True: also a dict with, per hidden layer, copies (the positions of every copy of neuron i, the first one first), pairs (P x 2)
    and zero (the zero filler)"""
    assert kind in KINDS
    xd, K = list(net.xdims), len(net.Ms)
    assert len(widths) == K - 1 and all(D >= d for D, d in zip(widths, xd[1:-1]))
    rng = np.random.default_rng(seed)
    copies, pairs, zero = [], [], []
    for k, D in enumerate(widths):
        n = xd[k + 1]
        pos = live_positions(D, n, k, rng)
        free = rng.permutation(np.array([p for p in range(D) if p not in set(pos.tolist())], dtype=np.int64))
        cp, pr = [[int(p)] for p in pos], np.zeros((0, 2), dtype=np.int64)
        if kind == "split":
            m, o = multiplicities(n, D), 0
            for i in range(n):
                cp[i] += [int(p) for p in free[o:o + m[i] - 1]]
                o += m[i] - 1
            free = free[o:]
        elif kind == "cancel":
            npair = len(free) // 2
            pr, free = free[:2 * npair].reshape(npair, 2), free[2 * npair:]
        copies.append(cp)
        pairs.append(pr)
        zero.append(np.sort(free))
    dims = [xd[0]] + list(widths) + [xd[-1]]
    Ms = []
    for k in range(K):
        W, b = net.Ms[k][:, :-1], net.Ms[k][:, -1]
        M = np.zeros((dims[k + 1], dims[k] + 1))
        rows = copies[k] if k < K - 1 else [[i] for i in range(xd[-1])]              # where the rows of W go (every copy)
        cols = copies[k - 1] if k > 0 else [[q] for q in range(xd[0])]               # where its columns go (every copy, weight w / m)
        for i, ri in enumerate(rows):
            for q, cq in enumerate(cols):
                M[np.ix_(ri, cq)] = W[i, q] / len(cq)
            M[ri, -1] = b[i]
        if kind == "cancel":
            first = [c[0] for c in cols]
            if k < K - 1:                                                            # the incoming rows of this layer's pairs
                for p, q in pairs[k]:
                    row = rng.normal(0.0, 1.0 / np.sqrt(len(first) + 1), size=len(first) + 1)
                    M[p, first], M[p, -1] = row[:-1], row[-1]
                    M[q, first], M[q, -1] = row[:-1], row[-1]
            if k > 0:                                                                # the outgoing columns of the pairs below
                fed = np.setdiff1d(np.arange(dims[k + 1]), zero[k]) if k < K - 1 else np.arange(dims[k + 1])
                for p, q in pairs[k - 1]:
                    g = rng.normal(0.0, 1.0 / np.sqrt(dims[k] + 1), size=len(fed))
                    M[fed, p], M[fed, q] = g, -g
        Ms.append(M)
    wide = na.FeedFwdNet(xdims=dims, Ms=Ms, activ=net.activ)
    live = [np.array([c[0] for c in cp], dtype=np.int64) for cp in copies]
    if full:
        return wide, live, dict(copies=copies, pairs=pairs, zero=zero)
    return wide, live


# ----------------------------------------------------------------------------- the cases of both files
def combos(layouts):
    """(name, widths, kind) of every layout of a table and every kind it runs with"""
    return [(name, tuple(w), kind) for name, ws in layouts.items() for w in ws for kind in KINDS if kind == "split" or list(w) not in SPLIT_ONLY]


def label(name, widths, kind):
    return f"{name} in {'-'.join(map(str, widths))} {kind}"


# The seed of a combination: 1000 + (its index in the list below) unless named here, where it is the first of that + 100, + 200, ... which
# meets two conditions on the inputs that test_exact_embedded_cpu.py asserts for every combination, both decided without any kernel:
# the yardstick |R(float64) - R(long double)| of the embedded net is continuous on the fixture's boxes (1e-12 per array and box; no seed
# failed it), and in every hidden layer above 64 that a product reads as columns a live neuron at a position >= 64 is active on the
# point box, where every kind is tight - or a "cancel" net, whose bounds are loose elsewhere, could lose tile w + 4 unnoticed (1005 of
# 3-10-10-3 in 65-128 "cancel" put a neuron that is off there on the layer's only such column; 1105 did the same)
SEEDS = {("3-10-10-3", (65, 128), "cancel", False): 1205}


def seed_of(name, widths, kind, tanh=False):
    order = combos(WIDE) + combos(NARROW)
    return SEEDS.get((name, tuple(widths), kind, tanh), 1000 + order.index((name, tuple(widths), kind)) + (500 if tanh else 0))


def hidden_rows(xdims, live):
    """the rows of an acdim-long array of the wide net that belong to the live neurons, in the small net's order"""
    off = np.concatenate([[0], np.cumsum(xdims[1:-1])])
    return np.concatenate([off[k] + live[k] for k in range(len(live))])


def case(name, widths, kind, tanh=False):
    """dict: small (ec.case(name); its net as a Tanh net for tanh=True), net (the embedded net), live, info, rows (hidden_rows), C, lo,
    hi (the 8 fixture boxes), cs (net, C, boxes: what ec.fp64_tols and the entries of tests/test_exact_soundness_gpu.py read)"""
    key = (name, tuple(widths), kind, tanh)
    if key not in _cache:
        small = ec.case(name)
        snet = tc.tanh_copy(small["net"]) if tanh else small["net"]
        net, live, info = embed(snet, list(widths), kind, seed_of(name, widths, kind, tanh), full=True)
        lo, hi = ec.box_arrays(small)
        _cache[key] = dict(small=small, small_net=snet, net=net, live=live, info=info, rows=hidden_rows(net.xdims, live), C=small["C"], lo=lo, hi=hi,
                           cs=dict(net=net, C=small["C"], boxes=small["boxes"]), label=label(name, widths, kind))
    return _cache[key]


def tols(em):
    """ec.fp64_tols on the embedded net and the fixture's boxes, with the two restatements they come from"""
    if "tol" not in em:
        em["r64"] = lc.R(em["net"].Ms, em["lo"], em["hi"], np.float64, head=em["C"])
        em["rld"] = lc.R(em["net"].Ms, em["lo"], em["hi"], np.longdouble, head=em["C"])
        em["tol"] = {nm: max(8.0 * float(np.abs(a - b).max()), 64.0 * ec.EPS * float(np.abs(b).max()))
                     for nm, a, b in zip(lc.NAMES + lc.LIT_NAMES, em["r64"], em["rld"])}
    return em["tol"]


def small_tols(name):
    key = ("small tol", name)
    if key not in _cache:
        cs = ec.case(name)
        _cache[key] = ec.fp64_tols(cs, *ec.box_arrays(cs))
    return _cache[key]


def cut(em, arrays):
    """a dict over (a subset of) ec.ARRAYS of the embedded net -> the same with the hidden arrays cut to the live rows"""
    return {nm: (a[em["rows"]] if nm.startswith("ac") else a) for nm, a in arrays.items()}


def filler_is_stable(em, box):
    """by R(float64): on this box no neuron of the embedded net outside `live` has l < 0 < u"""
    tols(em)
    j = ec.BOX_NAMES.index(box)
    l, u = em["r64"][2][:, j], em["r64"][3][:, j]
    fill = np.setdiff1d(np.arange(len(l)), em["rows"])
    return not np.any((l[fill] < 0.0) & (u[fill] > 0.0))


def tight_boxes(em, kind):
    """the boxes on which check_sound asks for tightness: "stable" for a "cancel" net only if its filler is stable there as well"""
    return ("point", "stable") if kind != "cancel" or filler_is_stable(em, "stable") else ("point",)


def verdict_setting(em):
    """ec.verdict_setting on the embedded net: v from the fixture, c0 the embedded net's root bound (the host routine)"""
    if "verdict" not in em:
        root = em["small"]["boxes"][0]
        nrm, v = em["C"][0], float(root["lit"]["vmax"][0])
        iv = na.makeIntervalsBatch(em["net"], root["lo"][:, None], root["hi"][:, None], backend="host")
        c0 = float(np.maximum(nrm * iv[4][:, 0], nrm * iv[5][:, 0]).sum())
        assert c0 > v
        em["verdict"] = dict(net=em["net"], lo=root["lo"], hi=root["hi"], normal=nrm, v=v, c0=c0)
    return em["verdict"]
