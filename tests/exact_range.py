"""Exact ranges of small ReLU networks over a box, by enumeration of the feasible activation regions with one LP per question
(numpy + scipy only; nothing of the product, of the oracle package or of the numpy restatements `R` is used).  This is the ground truth of
tests/test_exact_range_cpu.py and tests/test_exact_soundness_gpu.py; tests/golden/make_exact_ranges.py records it in
tests/golden/exact_ranges.json, and the tests read that file instead of running the long enumerations.

The search is depth first over the hidden neurons in layer order.  Inside the current region (the box cut by the half-spaces of the
neurons decided so far) the next pre-activation is affine in x; its range over the region comes from two LPs (none where the box alone
decides the sign, and none for the minimum where the maximum is already <= 0); the search branches only where that range straddles 0 and
adds the half-space of the branch.  At a leaf the network is affine and one LP per objective row maximises it.

What is rigorous (exact_max):
  * `w` is the objective at the returned argmax, from a long-double forward pass of the network itself at a point of the box: a value the
    network attains in the box, therefore a lower bound of the true maximum whatever the LP solver did.
  * `v` is the true maximum up to the solver's feasibility tolerance (HiGHS: 1e-7 on the half-spaces, its default).  That tolerance moves
    a region's edge by 1e-7 and the value by at most L * 1e-7, L = |c| prod_k |W_k|_2 (+ |a|) the Lipschitz constant (`lipschitz`).
  * The generator refuses to write a value with |v - w| > 1e-9 (1 + |v|), so every recorded maximum is attained to that accuracy."""
import time
from collections import namedtuple

import numpy as np
from scipy.optimize import linprog

ExactMax = namedtuple("ExactMax", "v x w regions lps")
V_W_BOUND = 1e-9          # the generator asserts |v - w| <= V_W_BOUND (1 + |v|)


def split_layers(Ms):
    return [np.asarray(Mk, dtype=np.float64)[:, :-1] for Mk in Ms], [np.asarray(Mk, dtype=np.float64)[:, -1] for Mk in Ms]


def forward_ld(Ms, x, hidden=False):
    """long-double forward pass at one point x -> the output (with hidden=True: the list of hidden post-activations as well)"""
    ld = np.longdouble
    h, hid = np.asarray(x, dtype=ld), []
    for Mk in Ms[:-1]:
        Mk = np.asarray(Mk, dtype=ld)
        h = np.maximum(Mk[:, :-1] @ h + Mk[:, -1], ld(0))
        hid.append(h)
    ML = np.asarray(Ms[-1], dtype=ld)
    y = ML[:, :-1] @ h + ML[:, -1]
    return (y, hid) if hidden else y


def lifted(Ms, x):
    """(x, the hidden post-activations layer by layer, 1): the point x in the coordinates of the LMI matrix Z (oracle/qc.py: zdims =
    xdims[:-1] + [1], block k selected by E(k, zdims)), float64 from the long-double forward pass"""
    _, hid = forward_ld(Ms, x, hidden=True)
    return np.concatenate([np.asarray(x, dtype=np.float64)] + [np.asarray(h, dtype=np.float64) for h in hid] + [np.ones(1)])


def lipschitz(Ms, c, a=None):
    """|c| prod_k |W_k|_2 + |a|, per row of c"""
    W, _ = split_layers(Ms)
    C = np.atleast_2d(np.asarray(c, dtype=np.float64))
    L = np.linalg.norm(C, axis=1) * float(np.prod([np.linalg.norm(Wk, 2) for Wk in W]))
    if a is not None:
        L = L + np.linalg.norm(np.atleast_2d(np.asarray(a, dtype=np.float64)), axis=1)
    return L if np.ndim(c) == 2 else float(L[0])


def with_posts(Ms):
    """the network whose output is (post-activations of the last hidden layer, output of Ms): its rows serve both at one enumeration"""
    d = Ms[-1].shape[1] - 1
    return list(Ms[:-1]) + [np.vstack([np.hstack([np.eye(d), np.zeros((d, 1))]), np.asarray(Ms[-1], dtype=np.float64)])]


class _Search:
    def __init__(self, Ms, lo, hi, deadline=None):
        self.W, self.b = split_layers(Ms)
        self.deadline = deadline
        self.lo, self.hi = np.asarray(lo, dtype=np.float64).ravel(), np.asarray(hi, dtype=np.float64).ravel()
        self.n0 = len(self.lo)
        self.bounds = list(zip(self.lo, self.hi))
        self.lps = 0
        self.leaves = []              # (G, g, P, q): the region G x <= g and the affine map x -> P x + q of the last hidden layer

    def lp_max(self, p, G, g):
        """max p' x over the region -> (value, x) or None where the LP is infeasible"""
        self.lps += 1
        if self.deadline is not None and self.lps % 64 == 0 and time.monotonic() > self.deadline:
            raise TimeoutError("the enumeration passed its deadline")
        res = linprog(-p, A_ub=G if len(g) else None, b_ub=g if len(g) else None, bounds=self.bounds, method="highs")
        if res.status == 2:
            return None
        if res.status != 0:
            raise RuntimeError(f"linprog: status {res.status}: {res.message}")
        return -float(res.fun), np.clip(res.x, self.lo, self.hi)

    def box_range(self, p, q):
        c, r = 0.5 * (self.hi + self.lo), 0.5 * (self.hi - self.lo)
        return p @ c - np.abs(p) @ r + q, p @ c + np.abs(p) @ r + q

    def layer(self, k, P, q, G, g):
        if k == len(self.W) - 1:
            if len(g) and self.lp_max(np.zeros(self.n0), G, g) is None:
                return
            self.leaves.append((G, g, P, q))
            return
        Pz, qz = self.W[k] @ P, self.W[k] @ q + self.b[k]
        self.neuron(k, 0, Pz, qz, np.zeros(len(qz)), G, g)

    def neuron(self, k, i, Pz, qz, d, G, g):
        """decide neuron i of hidden layer k; d holds the 0 / 1 pattern of the neurons before it"""
        if i == len(qz):
            self.layer(k + 1, d[:, None] * Pz, d * qz, G, g)
            return
        p, q = Pz[i], qz[i]
        bl, bu = self.box_range(p, q)
        if not len(g) or bu <= 0.0 or bl >= 0.0:
            l, u = bl, bu                              # the box alone is the region, or the box alone decides the sign
        else:
            top = self.lp_max(p, G, g)
            if top is None:
                return                                 # the region is empty
            u = top[0] + q
            if u <= 0.0:
                l = u
            else:
                bot = self.lp_max(-p, G, g)
                if bot is None:
                    return
                l = -bot[0] + q
        if l >= 0.0 or u <= 0.0:
            d2 = d.copy()
            d2[i] = 1.0 if l >= 0.0 and u > 0.0 else 0.0
            self.neuron(k, i + 1, Pz, qz, d2, G, g)
            return
        for on in (1.0, 0.0):                           # on: -(p x + q) <= 0; off: p x + q <= 0
            s = -1.0 if on else 1.0
            d2 = d.copy()
            d2[i] = on
            self.neuron(k, i + 1, Pz, qz, d2, np.vstack([G, s * p[None, :]]), np.append(g, -s * q))


def regions(Ms, lo, hi, deadline=None):
    """the feasible activation regions of the hidden layers of Ms over the box -> the _Search with its leaves; past `deadline` (a
    time.monotonic() value) the search raises TimeoutError"""
    s = _Search(Ms, lo, hi, deadline)
    s.layer(0, np.eye(s.n0), np.zeros(s.n0), np.zeros((0, s.n0)), np.zeros(0))
    return s


def exact_max(Ms, lo, hi, c, a=None, search=None):
    """the maximum over the box [lo, hi] of  c' f(x) - a' x,  f the ReLU network Ms = [[W_0 b_0], ..] (linear last layer).
    -> ExactMax(v, x, w, regions, lps): v the largest LP value over the regions, x its argmax clipped to the box, w the objective at x
    from a long-double forward pass, the number of feasible regions and the number of LPs solved (the enumeration's included).
    c and a may hold one objective per row (nrow x ny, nrow x n0): then v, w are vectors and x is nrow x n0, from one enumeration.
    The range of a hidden neuron comes from the same function: truncate the network after that layer (its last layer is then linear:
    a pre-activation) or append an identity layer (a post-activation, `with_posts`) and pass a unit row.  `search` reuses the regions of
    an earlier call on the same network and box."""
    one = np.ndim(c) == 1
    C = np.atleast_2d(np.asarray(c, dtype=np.float64))
    n0 = len(np.ravel(lo))
    A = np.zeros((C.shape[0], n0)) if a is None else np.atleast_2d(np.asarray(a, dtype=np.float64))
    s = regions(Ms, lo, hi) if search is None else search
    WL, bL = s.W[-1], s.b[-1]
    v = np.full(C.shape[0], -np.inf)
    x = np.tile(0.5 * (s.lo + s.hi), (C.shape[0], 1))
    for G, g, P, q in s.leaves:
        Pa, qa = C @ (WL @ P) - A, C @ (WL @ q + bL)
        for i in range(C.shape[0]):
            got = s.lp_max(Pa[i], G, g)
            if got is not None and got[0] + qa[i] > v[i]:
                v[i], x[i] = got[0] + qa[i], got[1]
    ld = np.longdouble
    w = np.array([float(C[i].astype(ld) @ forward_ld(Ms, x[i]) - A[i].astype(ld) @ x[i].astype(ld)) for i in range(C.shape[0])])
    if one:
        return ExactMax(float(v[0]), x[0], float(w[0]), len(s.leaves), s.lps)
    return ExactMax(v, x, w, len(s.leaves), s.lps)


def exact_range(Ms, lo, hi, C, search=None):
    """max and min of every row of C f(x): (ExactMax of C, ExactMax of -C with v and w negated back), one enumeration"""
    s = regions(Ms, lo, hi) if search is None else search
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    top = exact_max(Ms, lo, hi, C, search=s)
    bot = exact_max(Ms, lo, hi, -C, search=s)
    return top, ExactMax(-bot.v, bot.x, -bot.w, bot.regions, bot.lps)
