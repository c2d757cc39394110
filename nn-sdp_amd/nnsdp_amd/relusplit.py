"""Branching on the activation state of unstable ReLUs ("Branching on unstable ReLUs"): verifyReluSplit decides the
clause  OR_i normal_i' f(x) <= h_i  on one input box by splitting a node into the two signs of one pre-activation instead of bisecting
the box, so the tree grows with the number of unstable neurons and not with 2^n0.  The bounds of a node come from
CrownBounder.bound_nodes (crown_backend="resident", csrc/crown_relu_split.hpp) or makeIntervalsNodes (crown_backend="host", float32, no GPU):
exact relaxations of the forced neurons, clipped pre-activation bounds, and per literal a few projected-gradient steps on the Lagrange
multipliers of the forced signs.  The level loop is on the host (frontier="host"), or, with crown_backend="resident" and
frontier="device", on the bounder's stream (CrownBounder.search_nodes, csrc/crown_node_search.hpp): the assignments of a level stay in
device memory, the host reads back five integers per level, the points only on a level where the device flagged a possible
counterexample, and the leaves once at the end; the result is the host loop's on the resident bounder, bit for bit.

Not here: bisecting the box of an exhausted node, SDPs on nodes, verifyAcasSpec, the wide bounder
(max_width 128) and Tanh networks."""
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import frontend as F
from . import methods as M


@dataclass
class ReluSplitOptions:
    max_nodes: int = 4096          # nodes bounded in all; a level that would pass it ends the search "unknown" / "budget"
    max_depth: int = 64            # forced neurons on a path
    steps: int = 16                # multiplier steps per literal and node (0: clipping alone)
    eta0: float = 0.5
    decay: float = 0.9
    crown_backend: str = "host"    # "host": makeIntervalsNodes; "resident": one CrownBounder for the search
    workers: int = 16              # threads of the host routine
    corner_points: bool = True     # try the maximiser of every literal's linear bound besides the box centre
    frontier: str = "host"         # "host": the level loop below; "device": CrownBounder.search_nodes (needs crown_backend "resident")
    chunk: int = 4096              # frontier "device": nodes per launch of the node kernels; the result does not depend on it


@dataclass
class ReluLeaf:
    assign: np.ndarray             # acdim, int8
    depth: int
    closed_by: Optional[str]       # "bound", "infeasible"; None on an open node
    bound: float                   # smax of the literal closest to its threshold (NaN on an infeasible node)


@dataclass
class ReluSplitResult:
    verdict: str                   # "holds", "violated", "unknown"
    witness: Optional[np.ndarray]
    leaves: List[ReluLeaf]         # the closed nodes
    open: List[ReluLeaf]           # the nodes still open at the end ("holds": none)
    visited: int
    depth: int
    reason: Optional[str]          # "unknown" only: "budget" or "exhausted"
    seconds: dict = field(default_factory=dict)


def _check(net, x1min, x1max, literals, split):
    if net.activ is not M.ReluActiv:
        raise ValueError("verifyReluSplit is for ReLU networks, not Tanh")
    if len(literals) < 1:
        raise ValueError("verifyReluSplit needs literals: at least one (normal, h)")
    if split.crown_backend not in ("host", "resident"):
        raise ValueError("crown_backend must be 'host' or 'resident'")
    if split.crown_backend == "resident" and max(net.xdims) > 64:
        raise ValueError("crown_backend 'resident' takes layer widths up to 64: the node kernels have no wide instance")
    if not 0 <= int(split.steps) <= 64:
        raise ValueError("steps must be in 0..64")
    if not (np.isfinite(split.eta0) and split.eta0 > 0.0):
        raise ValueError("eta0 must be positive and finite")
    if not 0.0 < split.decay <= 1.0:
        raise ValueError("decay must be in (0, 1]")
    if split.max_nodes < 1 or split.max_depth < 0:
        raise ValueError("max_nodes must be >= 1 and max_depth >= 0")
    if split.frontier not in ("host", "device"):
        raise ValueError("frontier must be 'host' or 'device'")
    if split.frontier == "device" and split.crown_backend != "resident":
        raise ValueError("frontier 'device' needs crown_backend 'resident': the nodes live beside the resident bounder's network")
    if int(split.chunk) < 1:
        raise ValueError("chunk must be >= 1")
    lo, hi = np.asarray(x1min, dtype=np.float64), np.asarray(x1max, dtype=np.float64)
    if lo.shape != (net.xdims[0],) or hi.shape != lo.shape or not np.all(lo <= hi):
        raise ValueError("x1min / x1max must have xdims[0] entries with x1min <= x1max")
    normals = np.array([np.asarray(nrm, dtype=np.float64) for nrm, _ in literals])
    if normals.shape != (len(literals), net.xdims[-1]):
        raise ValueError("every literal's normal must have xdims[K] entries")
    return lo, hi, normals, np.array([float(h) for _, h in literals])


def verifyReluSplit(net: M.FeedFwdNet, x1min, x1max, literals, split: ReluSplitOptions = None) -> ReluSplitResult:
    """Decide  OR_i normal_i' f(x) <= h_i  for all x in the box; literals: [(normal, h)].  Per level, one bound call for all open nodes:
    a node is closed when it is infeasible or some literal has smax_i <= h_i; otherwise the box centre (and with corner_points every
    literal's maximiser x*) is evaluated, and a point that violates every literal, confirmed in fp64 on the host, ends the search
    "violated"; otherwise the node splits on branch[i] of the literal with the smallest smax_i - h_i into the signs +1 and -1.  A node
    without an unstable free neuron stays open ("unknown" / "exhausted" unless a witness turns up)."""
    split = split or ReluSplitOptions()
    lo, hi, normals, hs = _check(net, x1min, x1max, literals, split)
    t_start = time.perf_counter()
    seconds = dict(bound=0.0, points=0.0)
    bounder = F.CrownBounder(net, normals) if split.crown_backend == "resident" else None
    try:
        if split.frontier == "device":
            return _device_levels(net, lo, hi, normals, hs, split, bounder, t_start)
        return _levels(net, lo, hi, normals, hs, split, bounder, seconds, t_start)
    finally:
        if bounder is not None:
            bounder.close()


def _device_levels(net, lo, hi, normals, hs, split, bounder, t_start):
    """the level loop on the bounder's stream; a flagged point is confirmed in fp64 on the host, as in _levels"""
    def confirm(x):
        return bool(_violates_all(F.evalFeedFwdNet(net, x)[:, None], normals, hs)[0])

    r = bounder.search_nodes(lo, hi, hs, steps=split.steps, eta0=split.eta0, decay=split.decay, corner_points=split.corner_points,
                             max_nodes=split.max_nodes, max_depth=split.max_depth, chunk=split.chunk, confirm=confirm)
    by = {0: "infeasible", 1: "bound", -1: None}
    nodes = [ReluLeaf(r["assign"][k].copy(), int(r["leaf_depth"][k]), by[int(r["closed_by"][k])],
                      float("nan") if r["closed_by"][k] == 0 else float(r["bound"][k])) for k in range(len(r["bound"]))]
    seconds = dict(kernel=r["kernel_ms"] * 1e-3, total=time.perf_counter() - t_start)
    return ReluSplitResult(r["verdict"], r["witness"], nodes[:r["nleaves"]], nodes[r["nleaves"]:], r["visited"], r["depth"], r["reason"], seconds)


def _violates_all(Y, normals, hs):
    return np.all(normals @ Y > hs[:, None], axis=0)


def _levels(net, lo, hi, normals, hs, split, bounder, seconds, t_start):
    n0, acdim, nlit = net.xdims[0], int(sum(net.xdims[1:-1])), len(hs)
    frontier = [np.zeros(acdim, dtype=np.int8)]
    leaves, stuck, visited, depth = [], [], 0, 0

    def done(verdict, witness=None, reason=None, still=()):
        seconds["total"] = time.perf_counter() - t_start
        return ReluSplitResult(verdict, witness, leaves, stuck + list(still), visited, depth, reason, seconds)

    while True:
        nn = len(frontier)
        asg = np.stack(frontier, axis=1)
        blo, bhi = np.repeat(lo[:, None], nn, axis=1), np.repeat(hi[:, None], nn, axis=1)
        t0 = time.perf_counter()
        if bounder is not None:
            nb = bounder.bound_nodes(blo, bhi, asg, steps=split.steps, eta0=split.eta0, decay=split.decay)
        else:
            nb = F.makeIntervalsNodes(net, blo, bhi, asg, normals, steps=split.steps, eta0=split.eta0, decay=split.decay, workers=split.workers)
        seconds["bound"] += time.perf_counter() - t0
        visited += nn
        # 1. close
        excess = nb.smax - hs[:, None]
        best = np.argmin(excess, axis=0)
        open_ids = []
        for b in range(nn):
            if nb.infeasible[b]:
                leaves.append(ReluLeaf(frontier[b], depth, "infeasible", float("nan")))
            elif excess[best[b], b] <= 0.0:
                leaves.append(ReluLeaf(frontier[b], depth, "bound", float(nb.smax[best[b], b])))
            else:
                open_ids.append(b)
        still = [ReluLeaf(frontier[b], depth, None, float(nb.smax[best[b], b])) for b in open_ids]
        if not open_ids:
            if stuck:
                return done("unknown", reason="exhausted")
            return done("holds")
        # 2. refute: the centre, and every literal's maximiser over the box
        t0 = time.perf_counter()
        c, r = 0.5 * (lo + hi), 0.5 * (hi - lo)
        pts = [c[:, None]]
        if split.corner_points:
            for b in open_ids:
                pts.append((c[None, :] + np.sign(nb.A[:, :, b]) * r[None, :]).T)
        X = np.unique(np.concatenate(pts, axis=1), axis=1)
        Y = bounder.eval(X) if bounder is not None else F.evalFeedFwdNet(net, X)
        seconds["points"] += time.perf_counter() - t0
        for k in np.flatnonzero(_violates_all(Y, normals, hs)):
            x = X[:, k].copy()
            if bool(_violates_all(F.evalFeedFwdNet(net, x)[:, None], normals, hs)[0]):      # confirmed in fp64 on the host
                return done("violated", x, still=still)
        # 3. branch
        nxt = []
        for b, leaf in zip(open_ids, still):
            n = int(nb.branch[best[b], b])
            if n < 0:
                stuck.append(leaf)
                continue
            for sign in (1, -1):
                child = frontier[b].copy()
                child[n] = sign
                nxt.append(child)
        if not nxt:
            return done("unknown", reason="exhausted")
        if visited + len(nxt) > split.max_nodes or depth + 1 > split.max_depth:
            return done("unknown", reason="budget", still=[lf for lf, b in zip(still, open_ids) if int(nb.branch[best[b], b]) >= 0])
        frontier, depth = nxt, depth + 1
