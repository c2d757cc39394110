"""Oracle-state harness: the CPU oracle's fixed-penalty ADMM (oracle/admm.py, AdmmState) stepped state for state from the
library's start, with snapshots in the layout of the library's test entries (nnsdp_solver_raw_multipliers).

The multiplier block of the fixed-point variable nu is returned by the library at full length ng_full: kept generators at
their full index, in solver coordinates (column-normalised and scaled as ScaledProblem does it), dropped generators exactly 0
(csrc/api.hip nnsdp_solver_raw_multipliers writes nu[g] to out[keep[g]]; csrc/setup.hpp scale_operator keeps a generator iff
its column norm exceeds 1e-150, the oracle's drop_tol - the layer order the library keeps them in internally is undone by keep).

Trajectories are cached per process (one per case key), so that every leg that needs W40-D20 shares one oracle run.
"""
import copy
import functools
import os

import numpy as np

import helpers
from oracle import admm as oadmm, nnet_io, operator as oop, qc


class Trajectory:
    """nu_k of the oracle's iteration at fixed sigma / alpha: kept where asked for, ||nu_k||_2 recorded for every k."""

    def __init__(self, L, sigma: float = 0.1, alpha: float = 1.6):
        self.L = L
        self.keep = set()                # iterations whose state is kept whenever the trajectory passes them
        self.P = oadmm.ScaledProblem(L)
        self.S = oadmm.AdmmState(self.P, sigma, alpha)
        self.k = 0
        self.norms = [float(np.linalg.norm(self.S.nu))]
        self.snaps = {0: self.S.nu.copy()}
        self.checks = {}

    def blocks(self):
        """(number of PSD blocks, largest block) - nnsdp_solver_info items 4 and 5"""
        return len(self.S.nk), max(self.S.nk)

    def advance(self, n: int, keep=()):
        """step up to iteration n, keeping the states of the iterations in `keep` (and n)"""
        keep = set(keep) | self.keep | {n}
        if n < self.k and n not in self.snaps:
            raise ValueError(f"state {n} was not kept (trajectory at {self.k})")
        while self.k < n:
            self.S.step()
            self.k += 1
            self.norms.append(float(np.linalg.norm(self.S.nu)))
            if self.k in keep:
                self.snaps[self.k] = self.S.nu.copy()

    def nu(self, n: int) -> np.ndarray:
        if n not in self.snaps:
            self.advance(n)
        return self.snaps[n]

    def multipliers(self, n: int) -> np.ndarray:
        """the multiplier block of nu_n as nnsdp_solver_raw_multipliers returns it"""
        full = np.zeros(self.P.ng_full)
        full[self.P.keep] = self.nu(n)[:self.S.ng]
        return full

    def bound_norm(self, n: int) -> float:
        """B = max_{k <= n} ||nu_k||_2"""
        self.nu(n)
        return max(self.norms[:n + 1])

    def check(self, n: int):
        """(pres, dres, pobj, dobj) of one check iteration taken from state n - what nnsdp_solver_residuals returns after n
        iterations - by the formulas of admm_solve (AdmmState.check_quantities); state n + 1 is kept as a side effect."""
        if n not in self.checks:
            S = copy.copy(self.S)            # step() rebinds nu: the trajectory's own state is not touched
            S.nu = self.nu(n).copy()
            nu_prev = S.nu
            w, x, res, Kxq = S.step()
            self.checks[n] = tuple(float(v) for v in S.check_quantities(nu_prev, w, x, res, Kxq))
            self.snaps.setdefault(n + 1, S.nu)
        return self.checks[n]

    def gamma(self, n: int) -> np.ndarray:
        """unscaled full-length gamma of state n (AdmmState.gamma)"""
        S = copy.copy(self.S)
        S.nu = self.nu(n).copy()
        return S.gamma()


def rigorous_bound(n_iters: int, tol: float, B: float, c: float = 1.0) -> float:
    """||nu_gpu - nu_oracle||_2 after n_iters steps from the same start when every projection is within c * tol * ||A||_F of the
    exact one: the fixed-sigma map is averaged (nonexpansive), and a projection error d reaches the next nu with a norm of at
    most alpha (2 + 1) |d| < 5 |d| (alpha = 1.6); ||A||_F <= ||nu_k||_2 <= B."""
    return 5.0 * n_iters * c * tol * B


# ----------------------------------------------------------------------------- cases: (product query, oracle query, decomposition)
def mirror_query(q):
    """the oracle's statement of a product query (same network, box, output QC and activation QCs)"""
    import nnsdp_amd as na
    net = q.ffnet
    act = "tanh" if na.methods._activ_code(net.activ) == na.methods.ACTIV_TANH else "relu"
    onet = nnet_io.FeedFwdNet(xdims=list(net.xdims), Ms=[np.array(M, dtype=np.float64) for M in net.Ms])
    qb, qs = q.qc_activs
    if isinstance(q, na.SafetyQuery):
        oout = qc.QcSafety(S=np.asarray(q.qc_safety.S, dtype=float))
    elif isinstance(q.qc_reach, na.QcReachHplane):
        oout = qc.QcReachHplane(normal=np.asarray(q.qc_reach.normal, dtype=float))
    elif isinstance(q.qc_reach, na.QcReachCircle):
        oout = qc.QcReachCircle(yc=np.asarray(q.qc_reach.yc, dtype=float))
    else:
        oout = qc.QcReachEllipsoid(invP=np.asarray(q.qc_reach.invP, dtype=float), yc=np.asarray(q.qc_reach.yc, dtype=float))
    return qc.Query(net=onet, qc_input=qc.QcInputBox(np.asarray(q.qc_input.x1min, float), np.asarray(q.qc_input.x1max, float)),
                    qc_out=oout, qc_bounded=qc.QcActivBounded(acymin=qb.acymin, acymax=qb.acymax),
                    qc_sector=qc.QcActivSector(acxdim=net.acdim, beta=int(qs.beta), smin=qs.smin, smax=qs.smax, activ=act))


def golden_net(name: str):
    import nnsdp_amd as na
    d = np.load(os.path.join(helpers.GOLDEN, "nets", f"scale-I2-O2-{name}.npz"))
    xd = [int(v) for v in d["xdims"]]
    return na.FeedFwdNet(xdims=xd, Ms=[np.array(d[f"M{k}"]) for k in range(len(xd) - 1)])


def net_hplane_query(name: str, beta: int, normal=(0.6, 0.8)):
    """reach-hyperplane query on [0.5, 1.5]^2 over a published net, with plain interval arithmetic (host only)"""
    import nnsdp_amd as na
    from nnsdp_amd import frontend as F
    net = golden_net(name)
    lo, hi = np.full(2, 0.5), np.full(2, 1.5)
    xi, acx = F.intervalsWorstCase(lo, hi, net)
    return na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi),
                         qc_reach=na.QcReachHplane(normal=np.asarray(normal, dtype=float)), qc_activs=F.makeQcActivsIntvs(net, xi, acx, beta))


# key -> (product query builder, oracle decomposition name)
CASES = {
    "W40-D20-b0-single": (lambda: helpers.product_query(helpers.load_problem("W40-D20", 0)), "single"),
    "W40-D20-b2-double": (lambda: helpers.product_query(helpers.load_problem("W40-D20", 2)), "double"),
    "W40-D40-b0-double": (lambda: helpers.product_query(helpers.load_problem("W40-D40", 0)), "double"),
    "W20-D10-b0-path": (lambda: helpers.product_query(helpers.load_problem("W20-D10", 0)), "path"),
    "W10-D5-b3-single": (lambda: helpers.product_query(helpers.load_problem("W10-D5", 3)), "single"),
    "W20-D20-b5-double-hplane": (lambda: net_hplane_query("W20-D20", 5), "double"),
    "W10-D10-b7-single-hplane": (lambda: net_hplane_query("W10-D10", 7), "single"),
    "acas50-path": (helpers.acas_shaped_query, "path"),
    "acas50-single": (helpers.acas_shaped_query, "single"),
}


def decomp(mode: str):
    import nnsdp_amd as na
    return {"single": na.SingleDecomp, "double": na.DoubleDecomp, "path": na.PathDecomp, "dense": na.DenseCone}[mode]()


@functools.lru_cache(maxsize=None)
def case_query(key: str):
    return CASES[key][0]()


@functools.lru_cache(maxsize=None)
def case_operator(key: str):
    """the library merges identical index sets into one block (csrc/solver.hpp reduced_cliques); so does the harness"""
    return oop.build_operator(mirror_query(case_query(key)), CASES[key][1], normalize=True, merge_identical=True)


@functools.lru_cache(maxsize=None)
def trajectory(key: str) -> Trajectory:
    """the cached fixed-penalty (sigma = 0.1, alpha = 1.6: the library's defaults) trajectory of a case"""
    return Trajectory(case_operator(key))
