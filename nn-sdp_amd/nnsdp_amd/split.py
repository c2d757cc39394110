"""Input splitting: decide a disjunctive clause of hyperplane literals on an input box by bisecting the box.

A relaxation over a whole input box is often too loose to decide a literal, and TARGET_UNREACHABLE / ITERATION_LIMIT are final
answers of a single solve.  verifySplit works level by level on the frontier of open sub-boxes:

  bound    one makeIntervalsBatch call for the whole frontier (csrc/crown_batch.hpp on the GPU, or the host routine per box), or
           with crown_backend = "resident" one call of a CrownBounder that keeps the network on the GPU for the whole verifySplit;
           a literal  normal' f(x) <= h  is proved on a box when  sum_j max(n_j ymin_j, n_j ymax_j) <= h.  With literal_bounds the
           same call also back-propagates every normal folded into the last affine layer (the literal pass of the kernel /
           nnsdp_make_intervals_lits), which keeps the correlation between the outputs; the smaller of the two bounds is used
  refute   the network at the box centres (plus `samples` seeded points per box, plus with corner_points the corner of each box
           that maximises the linear upper bound of its best literal): a point that violates every literal, confirmed by the
           fp64 numpy evaluation, is a witness
  sdp      the boxes closest to a proof get one reach-hyperplane SDP per literal (vnnlib.reachForm) with the target h, decided
           early, in lockstep batches; the literals of a box form one solver family; the activation QCs come from the bounds of
           the first step (no second interval pass)
  split    every box still open is bisected along the coordinate that is widest relative to the root box

The driver is deterministic: no random numbers unless samples > 0, and then seeded from the box index.  With
sdp_per_level = 0 and crown_backend = "host" it needs no GPU.  The reference has no counterpart (it prints :unsafe for a clause
it could not certify on the whole box, experiments/acas.jl:87-137).

reachSplit (below) is the same tree for a reach question: no threshold is given, the threshold of direction i is the incumbent
L_i + tol_i, which moves as better points are found, and the result is an enclosure [lower_i, upper_i] of  max_x c_i' f(x).
"""
from __future__ import annotations

import dataclasses
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import ctypes as C

import numpy as np

from . import _lib
from . import frontend as F
from . import methods as M
from . import vnnlib as V


@dataclass
class SplitOptions:
    max_boxes: int = 512          # boxes bounded (visited) before the driver gives up
    max_depth: int = 24           # bisections of one box before the driver gives up
    sdp_per_level: int = 26       # open boxes per level that get SDPs (0: bounds only)
    batch: int = 13               # SDPs advanced in lockstep in one batch handle
    # makeIntervalsBatch backend and where the refutation points are evaluated: "gpu" (csrc/crown_batch.hpp, fp64), "host", or
    # "resident": one frontend.CrownBounder for the whole call (the network uploaded once; the same bits as "gpu" on a ReLU network,
    # and the only GPU route for a Tanh network).  "host" is the default until the kernel has been timed against 16 host workers
    # (tools/split_timing.py)
    crown_backend: str = "host"
    samples: int = 0              # extra uniform points per open box in the refutation step, seeded from the box index
    # bound the literals themselves in the bound step (makeIntervalsBatch(normals=...)) and use min(that bound, the per-output one)
    # for proving, for Leaf.bound and for the order of the SDP stage: never proves less than without it (a clause of at most 64 literals)
    literal_bounds: bool = False
    # the refutation step also tries, per open box, the corner  where(A >= 0, hi, lo)  of its best literal's linear upper bound
    # A' x + b0 (requests the literal bounds whatever literal_bounds says)
    corner_points: bool = False
    # optimised lower slopes of the unstable ReLUs for the literal bounds (alpha-CROWN): projected-gradient steps
    # per box and literal, their step size and its decay per step; needs literal_bounds and crown_backend "host" or "resident", ReLU.
    # alpha_inherit: a child box starts from its parent's best slopes instead of the plain rule
    alpha_steps: int = 0
    alpha_eta0: float = 0.5
    alpha_decay: float = 0.9
    alpha_inherit: bool = False
    # where the frontier of open boxes lives: "host" (the Python loop below), or "device": the level loop of a bounds-only search runs on
    # the CrownBounder's stream with the boxes, the proof test, the refutation points, the bisection and the leaf log in device memory
    # (CrownBounder.search, csrc/crown_search.hpp); the same SplitResult bit for bit.  Needs crown_backend "resident", samples = 0 and
    # alpha_steps = 0.  With sdp_per_level > 0 the SDPs run once, on the open leaves of a search that ended "unknown".
    # SplitResult.seconds then has one more key, "kernel": the HIP-event time of the search's launches (tools/split_timing.py reads it).
    # reachSplit takes the same option (CrownBounder.reach, csrc/crown_reach.hpp) and then also needs sdp_per_level = 0.
    # verifySplitMany takes it too (CrownBounder.search_many, csrc/crown_forest.hpp: many root boxes in one level loop); it is bounds-only.
    # chunk: boxes per launch of the bound kernel, which bounds the device memory of a level's interval arrays
    frontier: str = "host"
    chunk: int = 4096
    # the widest hidden layer of the CrownBounder of crown_backend "resident": 64, or 128 for the wide instance of the kernel
    # (csrc/crown_wide.hpp: one workgroup per CU instead of two, so it is asked for; xdims[0], xdims[K] and the literals stay at 64).
    # 128 needs crown_backend "resident" and alpha_steps = 0 (the alpha kernel keeps a 64-wide layout); both frontiers take it
    crown_max_width: int = 64


@dataclass
class Leaf:
    lo: np.ndarray
    hi: np.ndarray
    depth: int
    proved_by: Optional[str]      # "crown" | "sdp" | None (open)
    literal: Optional[int]        # index of the literal that was proved
    bound: Optional[float]        # the proved literal's upper bound of normal' f on the box (open: the smallest excess literal's bound)
    soln: Any = None              # the reach-form QuerySolution of an "sdp" leaf


@dataclass
class SplitResult:
    verdict: str                  # "holds" | "violated" | "unknown"
    leaves: List[Leaf]
    witness: Optional[np.ndarray]
    visited: int
    sdp_solves: int
    seconds: Dict[str, float] = field(default_factory=dict)


@dataclass
class _Box:
    lo: np.ndarray
    hi: np.ndarray
    cuts: np.ndarray              # bisections per coordinate: the width is the root's times 2^-cuts, exactly comparable
    index: int = -1
    alpha0: Optional[np.ndarray] = None      # nlit x acdim: the parent's best slopes (alpha_inherit)


def _violates_all(Y, normals, hs) -> np.ndarray:
    """columns of Y (outputs) at which every literal normal' y <= h is false"""
    return np.all(normals @ Y > hs[:, None], axis=0)


def _solve_boxes(net, todo, normals, hs, beta: int, opts: M.AdmmSdpOptions, batch: int, seconds: Dict[str, float]):
    """todo: [(box, intervals of that box)] -> per box the list of (reach solution, h0) of its literals.  Boxes are packed into batch
    handles of at most `batch` SDPs (a box's literals stay together: they are one solver family)."""
    lib = _lib.load()
    out, group, count = [], [], 0

    def flush():
        nonlocal group, count
        if not group:
            return
        queries, optl, h0s = [], [], []
        for box, (acymin, acymax, acxmin, acxmax, ymin, ymax) in group:
            x_intvs, acx, o = [(box.lo, box.hi)], [], 0
            for k in range(1, net.K):
                n = net.xdims[k]
                x_intvs.append((acymin[o:o + n], acymax[o:o + n]))
                acx.append((acxmin[o:o + n], acxmax[o:o + n]))
                o += n
            x_intvs.append((ymin, ymax))
            qin = M.QcInputBox(x1min=box.lo, x1max=box.hi)
            qa = F.makeQcActivsIntvs(net, x_intvs, acx, beta)
            for nrm, h in zip(normals, hs):
                sq = M.SafetyQuery(ffnet=net, qc_input=qin, qc_safety=M.QcSafety(S=V.hplaneS(nrm, h, net)), qc_activs=qa)
                rq, hh, h0 = V.reachForm(sq, ybounds=(ymin, ymax))
                queries.append(rq)
                h0s.append(h0)
                optl.append(dataclasses.replace(opts, target=hh - h0, target_mode=M.TARGET_OBJECTIVE))
        t0 = time.perf_counter()
        sb = M.SolverBatch.from_solvers(M._shared_solvers(queries, optl), own=True)
        try:
            t1 = time.perf_counter()
            st = (C.c_int32 * len(sb.solvers))()
            _lib.check(lib.nnsdp_batch_run(sb.h, st))
            t2 = time.perf_counter()
            solns = []
            for s, code in zip(sb.solvers, st):
                r, bufs = M._alloc_result(s.cp)
                _lib.check(lib.nnsdp_solver_finish_status(s.h, int(code), C.byref(r)))
                solns.append(s._soln(r, bufs))
            t3 = time.perf_counter()
        finally:
            sb.close()
        seconds["setup"] += t1 - t0
        seconds["solve"] += t2 - t1
        seconds["finish"] += t3 - t2
        nl = len(normals)
        for b in range(len(group)):
            out.append(list(zip(solns[b * nl:(b + 1) * nl], h0s[b * nl:(b + 1) * nl])))
        group, count = [], 0

    for item in todo:
        if group and count + len(normals) > max(1, int(batch)):
            flush()
        group.append(item)
        count += len(normals)
    flush()
    return out


def _check_crown_max_width(split: SplitOptions) -> None:
    if split.crown_max_width not in (64, 128):
        raise ValueError("crown_max_width must be 64 or 128")
    if split.crown_max_width == 128:
        if split.crown_backend != "resident":
            raise ValueError("crown_max_width 128 needs crown_backend 'resident'")
        if split.alpha_steps > 0:
            raise ValueError("crown_max_width 128 needs alpha_steps == 0")


def _crown_bounder(net, normals, split: SplitOptions):
    """the CrownBounder of crown_backend "resident": the call of before at the default width, max_width only when it is asked for"""
    if split.crown_max_width == 64:
        return F.CrownBounder(net, normals)
    return F.CrownBounder(net, normals, max_width=split.crown_max_width)


def _check_split_options(net, split: SplitOptions) -> None:
    """the option refusals of verifySplit"""
    if split.crown_backend not in ("gpu", "host", "resident"):
        raise ValueError("crown_backend must be 'gpu', 'host' or 'resident'")
    if split.alpha_steps < 0:
        raise ValueError("alpha_steps must be >= 0")
    if split.alpha_steps > 0:
        if not split.literal_bounds:
            raise ValueError("alpha_steps > 0 tightens the literal bounds: it needs literal_bounds=True")
        if split.crown_backend not in ("host", "resident"):
            raise ValueError("alpha_steps > 0 needs crown_backend 'host' or 'resident'")
        if M._activ_code(net.activ) != M.ACTIV_RELU:
            raise ValueError("alpha_steps > 0 is for ReLU networks")
    if split.frontier not in ("host", "device"):
        raise ValueError("frontier must be 'host' or 'device'")
    if split.frontier == "device":
        if split.crown_backend != "resident":
            raise ValueError("frontier 'device' needs crown_backend 'resident'")
        if split.samples != 0:
            raise ValueError("frontier 'device' needs samples == 0")
        if split.alpha_steps != 0:
            raise ValueError("frontier 'device' needs alpha_steps == 0")
    _check_crown_max_width(split)


def _clause(net, literals):
    """(normals nlit x xdims[K], hs nlit) of a clause"""
    if not literals:
        raise ValueError("a clause needs at least one literal")
    normals = np.array([np.asarray(nrm, dtype=np.float64) for nrm, _ in literals])
    hs = np.array([float(h) for _, h in literals])
    if normals.shape != (len(literals), net.xdims[-1]):
        raise ValueError("every normal must have xdims[K] entries")
    return normals, hs


def verifySplit(net: M.FeedFwdNet, x1min, x1max, literals: Sequence[Tuple[Any, float]], beta: int, opts: M.AdmmSdpOptions,
                split: SplitOptions = None) -> SplitResult:
    """Decide the clause  OR_i normal_i' f(x) <= h_i  on the box [x1min, x1max]: "holds" when every leaf of the bisection tree has
    one literal proved on all of it, "violated" with a witness x at which every literal is false, "unknown" when max_boxes or
    max_depth ends the search (the open leaves are returned as they are)."""
    split = split or SplitOptions()
    _check_split_options(net, split)
    return _verify_split(net, x1min, x1max, literals, beta, opts, split, None)


def _verify_split(net, x1min, x1max, literals, beta, opts, split, shared) -> SplitResult:
    """verifySplit behind its option checks; shared: a CrownBounder of crown_backend "resident" that the caller owns (verifySplitMany),
    or None: the call makes and closes its own"""
    t_start = time.perf_counter()
    root_lo, root_hi = np.array(x1min, dtype=np.float64), np.array(x1max, dtype=np.float64)
    n0 = net.xdims[0]
    if root_lo.shape != (n0,) or root_hi.shape != (n0,) or not np.all(root_lo <= root_hi):
        raise ValueError("x1min / x1max must have xdims[0] entries with x1min <= x1max")
    normals, hs = _clause(net, literals)
    seconds = {"crown": 0.0, "setup": 0.0, "solve": 0.0, "finish": 0.0, "total": 0.0}
    frontier = [_Box(root_lo, root_hi, np.zeros(n0, dtype=np.int64))]
    want_lits = split.literal_bounds or split.corner_points
    bounder = shared
    if shared is None and split.crown_backend == "resident":
        bounder = _crown_bounder(net, normals if want_lits else None, split)
    try:
        if split.frontier == "device":
            return _split_device(net, root_lo, root_hi, normals, hs, beta, opts, split, bounder, want_lits, seconds, t_start)
        return _split_levels(net, frontier, root_lo, root_hi, normals, hs, beta, opts, split, bounder, seconds, t_start)
    finally:
        if bounder is not None and shared is None:
            bounder.close()


def verifySplitMany(net: M.FeedFwdNet, x1min, x1max, literals: Sequence[Tuple[Any, float]], beta: int, opts: M.AdmmSdpOptions,
                    split: SplitOptions = None, hs=None) -> List[SplitResult]:
    """verifySplit for the R root boxes x1min / x1max (xdims[0] x R), bounds only: the clause of `literals` on every root, with the
    thresholds of root r replaced by hs[:, r] when hs (nlit x R) is given.  max_boxes and max_depth apply to every root alone, and
    result r is what verifySplit returns for root r with its thresholds (the timings apart).  sdp_per_level must be 0.
    frontier = "host": the loop over verifySplit, on one CrownBounder when crown_backend is "resident".  frontier = "device" (needs what
    it needs in verifySplit): one CrownBounder.search_many (csrc/crown_forest.hpp), which runs level d of every undecided root as one
    frontier on the GPU, so a level's launches and its synchronisation are paid once for all roots; seconds["crown"], ["kernel"] and
    ["total"] of every result are then the whole call's."""
    split = split or SplitOptions()
    _check_split_options(net, split)
    if split.sdp_per_level != 0:
        raise ValueError("verifySplitMany is bounds-only: it needs sdp_per_level == 0")
    t_start = time.perf_counter()
    lo, hi = np.array(x1min, dtype=np.float64), np.array(x1max, dtype=np.float64)
    n0 = net.xdims[0]
    if lo.ndim != 2 or lo.shape[0] != n0 or hi.shape != lo.shape or not np.all(lo <= hi):
        raise ValueError("x1min / x1max must be xdims[0] x R with x1min <= x1max")
    R = lo.shape[1]
    normals, h0 = _clause(net, literals)
    H = np.repeat(h0[:, None], R, axis=1) if hs is None else np.array(hs, dtype=np.float64)
    if H.shape != (len(h0), R):
        raise ValueError("hs must be nlit x R: one threshold per literal and root")
    if R == 0:
        return []
    want_lits = split.literal_bounds or split.corner_points
    bounder = _crown_bounder(net, normals if want_lits else None, split) if split.crown_backend == "resident" else None
    try:
        if split.frontier == "host":
            return [_verify_split(net, lo[:, r], hi[:, r], [(normals[i], H[i, r]) for i in range(len(h0))], beta, opts, split, bounder)
                    for r in range(R)]
        t0 = time.perf_counter()
        res = bounder.search_many(lo, hi, H, normals=None if want_lits else normals, literal_bounds=split.literal_bounds,
                                  corner_points=split.corner_points, max_boxes=int(split.max_boxes), max_depth=int(split.max_depth),
                                  chunk=int(split.chunk),
                                  confirm=lambda r, x: bool(_violates_all(F.evalFeedFwdNet(net, x)[:, None], normals, H[:, r])[0]))
        t_crown = time.perf_counter() - t0
    finally:
        if bounder is not None:
            bounder.close()
    out = []
    for r in range(R):
        leaves = []
        for k in range(int(res["leaf_start"][r]), int(res["leaf_start"][r + 1])):
            lit = int(res["literal"][k])
            leaves.append(Leaf(res["lo"][k].copy(), res["hi"][k].copy(), int(res["leaf_depth"][k]), "crown" if res["proved"][k] else None,
                               lit if lit >= 0 else None, float(res["bound"][k]) if lit >= 0 else None))
        verdict = str(res["verdict"][r])
        seconds = {"crown": t_crown, "setup": 0.0, "solve": 0.0, "finish": 0.0, "total": 0.0, "kernel": 1e-3 * res["kernel_ms"]}
        out.append(SplitResult(verdict, leaves, res["witness"][r].copy() if verdict == "violated" else None, int(res["visited"][r]), 0, seconds))
    total = time.perf_counter() - t_start
    for sr in out:
        sr.seconds["total"] = total
    return out


def _split_device(net, root_lo, root_hi, normals, hs, beta, opts, split, bounder, want_lits, seconds, t_start) -> SplitResult:
    """verifySplit with frontier = "device": one CrownBounder.search, then (sdp_per_level > 0 and the search ended "unknown") one SDP
    stage on its bounded open leaves, as step 3 of _split_levels does on a level"""
    t0 = time.perf_counter()
    r = bounder.search(root_lo, root_hi, hs, normals=None if want_lits else normals, literal_bounds=split.literal_bounds,
                       corner_points=split.corner_points, max_boxes=int(split.max_boxes), max_depth=int(split.max_depth),
                       chunk=int(split.chunk), confirm=lambda x: bool(_violates_all(F.evalFeedFwdNet(net, x)[:, None], normals, hs)[0]))
    seconds["crown"] += time.perf_counter() - t0
    seconds["kernel"] = 1e-3 * r["kernel_ms"]
    leaves = []
    for k in range(len(r["proved"])):
        lit = int(r["literal"][k])
        leaves.append(Leaf(r["lo"][k].copy(), r["hi"][k].copy(), int(r["leaf_depth"][k]), "crown" if r["proved"][k] else None,
                           lit if lit >= 0 else None, float(r["bound"][k]) if lit >= 0 else None))
    verdict, sdp_solves = r["verdict"], 0
    todo = [k for k, lf in enumerate(leaves) if lf.proved_by is None and lf.literal is not None]
    if verdict == "unknown" and split.sdp_per_level > 0 and todo:
        t0 = time.perf_counter()
        lo, hi = np.stack([leaves[k].lo for k in todo], axis=1), np.stack([leaves[k].hi for k in todo], axis=1)
        iv = bounder.bound(lo, hi)
        if want_lits:
            iv = tuple(iv[:-1])
        seconds["crown"] += time.perf_counter() - t0
        order = sorted(range(len(todo)), key=lambda b: (leaves[todo[b]].bound - hs[leaves[todo[b]].literal], b))[:int(split.sdp_per_level)]
        # (_solve_boxes reads lo and hi of a box, never its cuts)
        boxes = [(_Box(leaves[todo[b]].lo, leaves[todo[b]].hi, None), tuple(a[:, b] for a in iv)) for b in order]
        got = _solve_boxes(net, boxes, normals, hs, beta, opts, split.batch, seconds)
        sdp_solves = len(order) * len(hs)
        for b, res in zip(order, got):
            for li, (s, h0) in enumerate(res):
                rho = float(s.objective_value) + h0
                if s.termination_status == "TARGET_CERTIFIED" and V.isSolutionGood(s) and rho <= hs[li]:
                    lf = leaves[todo[b]]
                    leaves[todo[b]] = Leaf(lf.lo, lf.hi, lf.depth, "sdp", li, rho, s)
                    break
        if all(lf.proved_by is not None for lf in leaves):
            verdict = "holds"
    seconds["total"] = time.perf_counter() - t_start
    return SplitResult(verdict, leaves, r["witness"], r["visited"], sdp_solves, seconds)


def _split_levels(net, frontier, root_lo, root_hi, normals, hs, beta, opts, split, bounder, seconds, t_start) -> SplitResult:
    """the levels of verifySplit; bounder: the CrownBounder of crown_backend = "resident" (the caller closes it), else None"""
    n0 = net.xdims[0]
    leaves: List[Leaf] = []
    visited = sdp_solves = depth = 0
    splittable = root_hi > root_lo

    def done(verdict, witness=None):
        seconds["total"] = time.perf_counter() - t_start
        return SplitResult(verdict, leaves, witness, visited, sdp_solves, seconds)

    while frontier:
        room = int(split.max_boxes) - visited
        for box in frontier[max(room, 0):]:        # never bounded: open as they are
            leaves.append(Leaf(box.lo, box.hi, depth, None, None, None))
        frontier = frontier[:max(room, 0)]
        if not frontier:
            return done("unknown")
        for box in frontier:
            box.index = visited
            visited += 1
        # 1. bound
        t0 = time.perf_counter()
        lo, hi = np.stack([b.lo for b in frontier], axis=1), np.stack([b.hi for b in frontier], axis=1)
        lits, ak = None, {}
        if split.alpha_steps > 0:
            ak = dict(alpha_steps=int(split.alpha_steps), eta0=split.alpha_eta0, decay=split.alpha_decay)
            if split.alpha_inherit and frontier[0].alpha0 is not None:
                ak["alpha0"] = np.stack([b.alpha0 for b in frontier], axis=2)
        if bounder is not None:
            iv = bounder.bound(lo, hi, **ak)
        elif split.literal_bounds or split.corner_points:
            iv = F.makeIntervalsBatch(net, lo, hi, backend=split.crown_backend, normals=normals, **ak)
        else:
            iv = F.makeIntervalsBatch(net, lo, hi, backend=split.crown_backend)
        if split.literal_bounds or split.corner_points:
            *iv, lits = iv
            iv = tuple(iv)
        seconds["crown"] += time.perf_counter() - t0
        ymin, ymax = iv[4], iv[5]
        cheap = np.stack([np.maximum(nrm[:, None] * ymin, nrm[:, None] * ymax).sum(axis=0) for nrm in normals])   # literal x box
        if split.literal_bounds:
            cheap = np.minimum(cheap, lits.smax)
        excess = cheap - hs[:, None]
        best = np.argmin(excess, axis=0)
        open_ids = []
        for b, box in enumerate(frontier):
            if excess[best[b], b] <= 0.0:
                leaves.append(Leaf(box.lo, box.hi, depth, "crown", int(best[b]), float(cheap[best[b], b])))
            else:
                open_ids.append(b)
        # 2. refute
        if open_ids:
            pts = [0.5 * (lo[:, open_ids] + hi[:, open_ids])]
            if split.corner_points:
                pts.append(np.stack([np.where(lits.A[best[b], :, b] >= 0.0, hi[:, b], lo[:, b]) for b in open_ids], axis=1))
            if split.samples > 0:
                for b in open_ids:
                    rng = np.random.default_rng(frontier[b].index)
                    pts.append(lo[:, [b]] + rng.random((n0, int(split.samples))) * (hi[:, [b]] - lo[:, [b]]))
            X = np.concatenate(pts, axis=1)
            if bounder is not None:
                Y = bounder.eval(X)
            else:
                Y = F.evalFeedFwdNetBatch(net, X) if split.crown_backend == "gpu" else F.evalFeedFwdNet(net, X)
            for c in np.flatnonzero(_violates_all(Y, normals, hs)):
                x = X[:, c].copy()
                if bool(_violates_all(F.evalFeedFwdNet(net, x)[:, None], normals, hs)[0]):     # confirmed in fp64 on the host
                    for b in open_ids:
                        leaves.append(Leaf(frontier[b].lo, frontier[b].hi, depth, None, int(best[b]), float(cheap[best[b], b])))
                    return done("violated", x)
        # 3. SDP on the open boxes closest to a proof
        if open_ids and split.sdp_per_level > 0:
            order = sorted(open_ids, key=lambda b: (excess[best[b], b], b))[:int(split.sdp_per_level)]
            todo = [(frontier[b], tuple(a[:, b] for a in iv)) for b in order]
            got = _solve_boxes(net, todo, normals, hs, beta, opts, split.batch, seconds)
            sdp_solves += len(order) * len(hs)
            for b, res in zip(order, got):
                for li, (s, h0) in enumerate(res):
                    rho = float(s.objective_value) + h0
                    if s.termination_status == "TARGET_CERTIFIED" and V.isSolutionGood(s) and rho <= hs[li]:
                        leaves.append(Leaf(frontier[b].lo, frontier[b].hi, depth, "sdp", li, rho, s))
                        open_ids.remove(b)
                        break
        if not open_ids:
            break
        # 5. stop / 4. split
        if visited >= split.max_boxes or depth >= split.max_depth or not np.any(splittable):
            for b in open_ids:
                leaves.append(Leaf(frontier[b].lo, frontier[b].hi, depth, None, int(best[b]), float(cheap[best[b], b])))
            return done("unknown")
        nxt = []
        for b in open_ids:
            box = frontier[b]
            j = int(np.argmin(np.where(splittable, box.cuts, np.iinfo(np.int64).max)))     # widest relative to the root, lowest index on ties
            mid = 0.5 * (box.lo[j] + box.hi[j])
            cuts = box.cuts.copy()
            cuts[j] += 1
            left_hi, right_lo = box.hi.copy(), box.lo.copy()
            left_hi[j] = mid
            right_lo[j] = mid
            a0 = lits.alpha[:, :, b] if split.alpha_steps > 0 and split.alpha_inherit else None
            nxt.append(_Box(box.lo, left_hi, cuts, alpha0=a0))
            nxt.append(_Box(right_lo, box.hi, cuts.copy(), alpha0=a0))
        frontier = nxt
        depth += 1
    # every box of the last level was proved; boxes that the budget kept from being bounded are open leaves, and one open leaf is
    # enough for "unknown"
    return done("holds" if all(lf.proved_by is not None for lf in leaves) else "unknown")


# ----------------------------------------------------------------------------- reach: support values to a tolerance
@dataclass
class ReachLeaf:
    lo: np.ndarray
    hi: np.ndarray
    depth: int
    closed_by: Optional[str]      # "crown" | "sdp" | None (open: the budget ended the search)
    bound: np.ndarray             # nlit: the upper bound of every direction on the box


@dataclass
class ReachSplitResult:
    status: str                   # "converged" | "budget"
    lower: np.ndarray             # nlit: c_i' f(witness_i), recomputed on the host in fp64
    upper: np.ndarray             # nlit: the maximum of bound[i] over the leaves
    incumbent: np.ndarray         # nlit: the loop's own L_i (the value at witness_i as the backend's forward pass gave it)
    witnesses: np.ndarray         # nlit x n0
    leaves: List[ReachLeaf]
    visited: int
    depth: int
    sdp_solves: int
    seconds: Dict[str, float] = field(default_factory=dict)


def _support_values(Cn, Y) -> np.ndarray:
    """s[i, p] = c_i' Y[:, p] with a fixed order: c_i[0] Y[0, p], then + c_i[j] Y[j, p] for j ascending, every product and every sum
    rounded on its own (no BLAS, whose order and fused multiply-adds are its own business); csrc/crown_reach.hpp restates it"""
    s = Cn[:, 0:1] * Y[0:1, :]
    for j in range(1, Cn.shape[1]):
        s = s + Cn[:, j:j + 1] * Y[j:j + 1, :]
    return s


def reachSplit(net: M.FeedFwdNet, x1min, x1max, normals, tol, beta: int = 0, opts: M.AdmmSdpOptions = None,
               split: SplitOptions = None) -> ReachSplitResult:
    """Enclose the support values  max_x c_i' f(x)  over the box [x1min, x1max] for the rows c_i of `normals` (nlit x xdims[K],
    1 <= nlit <= 64) in [lower_i, upper_i] by branch and bound on ONE bisection tree for all directions; tol is a scalar or nlit values,
    finite and >= 0.  Per level of the tree, on its frontier of boxes:

      bound      the bound call of verifySplit with the normals always passed: ub[i, b] = min(per-output bound, literal bound)
      points     the box centres, then with corner_points per direction the corner  where(A[i, :, b] >= 0, hi, lo)  of every box,
                 through the backend's forward pass
      incumbent  L_i = the largest c_i' f(point) seen so far (the first of equal points), with its point x_i
      classify   a box is open when  ub[i, b] > L_i + tol_i  for some i; the others are leaves ("crown") carrying ub[:, b]
      sdp        (sdp_per_level > 0, host frontier) the open boxes closest to closing get one reach SDP per direction with the target
                 L_i + tol_i; a certified  rho <= L_i + tol_i  replaces ub[i, b], and a box with no direction left is a leaf ("sdp")
      stop       no open box: "converged".  depth >= max_depth, nothing splittable, or visited + 2 * open > max_boxes: "budget", the
                 open boxes become open leaves.  A level is only created when the budget holds all of it
      split      every open box is bisected along the coordinate widest relative to the root, as in verifySplit

    Guarantees: the leaves tile the root box; every leaf has a bound and visited <= max_boxes;  lower_i <= max c_i' f <= upper_i  up to
    the bound routine's own rounding slack; on "converged"  upper_i <= incumbent_i + tol_i  holds as a floating-point comparison.
    SplitOptions as in verifySplit (literal_bounds is implied; samples must be 0; alpha_steps > 0 on the host frontier with
    crown_backend "host" or "resident" on a ReLU network).  frontier = "device" runs the same loop in CrownBounder.reach
    (csrc/crown_reach.hpp) with the same result bit for bit as frontier = "host" with crown_backend = "resident"; it needs
    crown_backend "resident", samples = 0, alpha_steps = 0 and sdp_per_level = 0."""
    split = split or SplitOptions()
    opts = opts or M.AdmmSdpOptions()
    if split.crown_backend not in ("gpu", "host", "resident"):
        raise ValueError("crown_backend must be 'gpu', 'host' or 'resident'")
    if split.samples != 0:
        raise ValueError("reachSplit needs samples == 0")
    if split.alpha_steps < 0:
        raise ValueError("alpha_steps must be >= 0")
    if split.alpha_steps > 0:
        if split.crown_backend not in ("host", "resident"):
            raise ValueError("alpha_steps > 0 needs crown_backend 'host' or 'resident'")
        if M._activ_code(net.activ) != M.ACTIV_RELU:
            raise ValueError("alpha_steps > 0 is for ReLU networks")
    if split.frontier not in ("host", "device"):
        raise ValueError("frontier must be 'host' or 'device'")
    if split.frontier == "device":
        if split.crown_backend != "resident":
            raise ValueError("frontier 'device' needs crown_backend 'resident'")
        if split.alpha_steps != 0:
            raise ValueError("frontier 'device' needs alpha_steps == 0")
        if split.sdp_per_level != 0:
            raise ValueError("frontier 'device' of reachSplit needs sdp_per_level == 0")
    _check_crown_max_width(split)
    if int(split.max_boxes) < 1:
        raise ValueError("max_boxes must be >= 1")
    t_start = time.perf_counter()
    root_lo, root_hi = np.array(x1min, dtype=np.float64), np.array(x1max, dtype=np.float64)
    n0, ny = net.xdims[0], net.xdims[-1]
    if root_lo.shape != (n0,) or root_hi.shape != (n0,) or not np.all(root_lo <= root_hi):
        raise ValueError("x1min / x1max must have xdims[0] entries with x1min <= x1max")
    Cn = np.array(normals, dtype=np.float64)
    if Cn.ndim != 2 or Cn.shape[1] != ny or not 1 <= Cn.shape[0] <= 64:
        raise ValueError("normals must be nlit x xdims[K] with 1 <= nlit <= 64")
    nlit = Cn.shape[0]
    tol = np.array(tol, dtype=np.float64)
    if tol.ndim == 0:
        tol = np.full(nlit, float(tol))
    if tol.shape != (nlit,) or not np.all(np.isfinite(tol)) or not np.all(tol >= 0.0):
        raise ValueError("tol must be a scalar or nlit values, finite and >= 0")
    seconds = {"crown": 0.0, "setup": 0.0, "solve": 0.0, "finish": 0.0, "total": 0.0}
    bounder = _crown_bounder(net, Cn, split) if split.crown_backend == "resident" else None
    try:
        if split.frontier == "device":
            res = _reach_device(root_lo, root_hi, tol, split, bounder, seconds)
        else:
            res = _reach_levels(net, root_lo, root_hi, Cn, tol, beta, opts, split, bounder, seconds)
    finally:
        if bounder is not None:
            bounder.close()
    status, L, W, leaves, visited, depth, sdp_solves = res
    lower = np.array([float(Cn[i] @ F.evalFeedFwdNet(net, W[i])) for i in range(nlit)])
    upper = np.max(np.stack([lf.bound for lf in leaves], axis=1), axis=1)
    seconds["total"] = time.perf_counter() - t_start
    return ReachSplitResult(status, lower, upper, L, W, leaves, visited, depth, sdp_solves, seconds)


def _reach_device(root_lo, root_hi, tol, split, bounder, seconds):
    t0 = time.perf_counter()
    r = bounder.reach(root_lo, root_hi, tol, corner_points=split.corner_points, max_boxes=int(split.max_boxes),
                      max_depth=int(split.max_depth), chunk=int(split.chunk))
    seconds["crown"] += time.perf_counter() - t0
    seconds["kernel"] = 1e-3 * r["kernel_ms"]
    leaves = [ReachLeaf(r["lo"][k].copy(), r["hi"][k].copy(), int(r["leaf_depth"][k]), "crown" if r["closed"][k] else None, r["bound"][k].copy())
              for k in range(len(r["closed"]))]
    return r["status"], r["incumbent"], r["witnesses"], leaves, r["visited"], r["depth"], 0


def _reach_levels(net, root_lo, root_hi, Cn, tol, beta, opts, split, bounder, seconds):
    """the levels of reachSplit; bounder: the CrownBounder of crown_backend = "resident" (the caller closes it), else None"""
    n0, nlit = net.xdims[0], Cn.shape[0]
    frontier = [_Box(root_lo, root_hi, np.zeros(n0, dtype=np.int64))]
    leaves: List[ReachLeaf] = []
    L, W = np.full(nlit, -np.inf), np.zeros((nlit, n0))
    visited, sdp_solves, depth = 1, 0, 0
    splittable = root_hi > root_lo
    while True:
        nb = len(frontier)
        # 1. bound
        t0 = time.perf_counter()
        lo, hi = np.stack([b.lo for b in frontier], axis=1), np.stack([b.hi for b in frontier], axis=1)
        ak = {}
        if split.alpha_steps > 0:
            ak = dict(alpha_steps=int(split.alpha_steps), eta0=split.alpha_eta0, decay=split.alpha_decay)
            if split.alpha_inherit and frontier[0].alpha0 is not None:
                ak["alpha0"] = np.stack([b.alpha0 for b in frontier], axis=2)
        if bounder is not None:
            iv = bounder.bound(lo, hi, **ak)
        else:
            iv = F.makeIntervalsBatch(net, lo, hi, backend=split.crown_backend, normals=Cn, **ak)
        *iv, lits = iv
        iv = tuple(iv)
        seconds["crown"] += time.perf_counter() - t0
        ymin, ymax = iv[4], iv[5]
        cheap = np.stack([np.maximum(nrm[:, None] * ymin, nrm[:, None] * ymax).sum(axis=0) for nrm in Cn])   # direction x box
        ub = np.minimum(cheap, lits.smax)
        # 2. points: the centres, then per direction the corners of its linear upper bound
        pts = [0.5 * (lo + hi)]
        if split.corner_points:
            for i in range(nlit):
                pts.append(np.where(lits.A[i] >= 0.0, hi, lo))
        X = np.concatenate(pts, axis=1)
        if bounder is not None:
            Y = bounder.eval(X)
        else:
            Y = F.evalFeedFwdNetBatch(net, X) if split.crown_backend == "gpu" else F.evalFeedFwdNet(net, X)
        # 3. incumbent: the first of equal maxima
        s = _support_values(Cn, np.asarray(Y, dtype=np.float64))
        for i in range(nlit):
            p = int(np.argmax(s[i]))
            if s[i, p] > L[i]:
                L[i] = s[i, p]
                W[i] = X[:, p]
        # 4. classify
        thr = L + tol
        is_open = np.any(ub > thr[:, None], axis=0)
        for b in np.flatnonzero(~is_open):
            leaves.append(ReachLeaf(frontier[b].lo, frontier[b].hi, depth, "crown", ub[:, b].copy()))
        open_ids = [int(b) for b in np.flatnonzero(is_open)]
        # 5. SDP on the open boxes closest to closing
        if open_ids and split.sdp_per_level > 0:
            gap = np.max(ub - thr[:, None], axis=0)
            order = sorted(open_ids, key=lambda b: (gap[b], b))[:int(split.sdp_per_level)]
            todo = [(frontier[b], tuple(a[:, b] for a in iv)) for b in order]
            got = _solve_boxes(net, todo, Cn, thr, beta, opts, split.batch, seconds)
            sdp_solves += len(order) * nlit
            for b, res in zip(order, got):
                for li, (sol, h0) in enumerate(res):
                    if not ub[li, b] > thr[li]:
                        continue
                    rho = float(sol.objective_value) + h0
                    if sol.termination_status == "TARGET_CERTIFIED" and V.isSolutionGood(sol) and rho <= thr[li]:
                        ub[li, b] = rho
                if not np.any(ub[:, b] > thr):
                    leaves.append(ReachLeaf(frontier[b].lo, frontier[b].hi, depth, "sdp", ub[:, b].copy()))
                    open_ids.remove(b)
        # 6. stop or split
        if not open_ids:
            return "converged", L, W, leaves, visited, depth, sdp_solves
        if depth >= split.max_depth or not np.any(splittable) or visited + 2 * len(open_ids) > int(split.max_boxes):
            for b in open_ids:
                leaves.append(ReachLeaf(frontier[b].lo, frontier[b].hi, depth, None, ub[:, b].copy()))
            return "budget", L, W, leaves, visited, depth, sdp_solves
        nxt = []
        for b in open_ids:
            box = frontier[b]
            j = int(np.argmin(np.where(splittable, box.cuts, np.iinfo(np.int64).max)))     # widest relative to the root, lowest index on ties
            mid = 0.5 * (box.lo[j] + box.hi[j])
            cuts = box.cuts.copy()
            cuts[j] += 1
            left_hi, right_lo = box.hi.copy(), box.lo.copy()
            left_hi[j] = mid
            right_lo[j] = mid
            a0 = lits.alpha[:, :, b] if split.alpha_steps > 0 and split.alpha_inherit else None
            nxt.append(_Box(box.lo, left_hi, cuts, alpha0=a0))
            nxt.append(_Box(right_lo, box.hi, cuts.copy(), alpha0=a0))
        frontier = nxt
        visited += len(nxt)
        depth += 1


def findReach2DpolySplit(net: M.FeedFwdNet, x1min, x1max, tol, num_hplanes: int = 6, split: SplitOptions = None):
    """findReach2Dpoly by input splitting: the normals of findReach2Dpoly (angle 2 pi k / num_hplanes of a two-output network) through
    reachSplit -> ([(normal, upper_i)], the ReachSplitResult).  The polytope  normal_i' y <= upper_i  contains the reach set, and on
    "converged" each face is within tol of touching it."""
    if net.xdims[-1] != 2:
        raise ValueError("findReach2DpolySplit needs a network with two outputs")
    normals = np.array([[np.cos(2 * np.pi * i / num_hplanes), np.sin(2 * np.pi * i / num_hplanes)] for i in range(num_hplanes)])
    res = reachSplit(net, x1min, x1max, normals, tol, split=split)
    return [(normals[i].copy(), float(res.upper[i])) for i in range(len(normals))], res
