"""Exact ranges of small ReLU networks over a node of a ReLU split: the set {x in box : s_n z_n(x) >= 0 for every forced neuron n},
s in {-1, 0, +1}^acdim ("Branching on unstable ReLUs").  numpy + scipy only; nothing of the product, of the oracle
package or of the numpy restatements `R` is used.  The enumeration is the one of tests/exact_range.py (its _Search, by subclass): a
forced neuron adds its half-space, takes the pattern of its sign and does not branch, and one feasibility LP prunes the region; a free
neuron is handled as there.  The leaves are the feasible activation regions of the node; on each the network and every hidden
pre-activation is affine, and one LP per question gives

  node_max / node_range      max (and min) over the node of every row of C f(x)           (exact_range.exact_max with search=)
  node_pre_range             max and min over the node of every hidden pre-activation
  node_depth                 max over the node of  min over the forced n of s_n z_n(x):  the margin by which the node is non-empty
  clause_max                 max over the node of  min_i (c_i' f(x) - h_i):  the clause OR_i c_i' f <= h_i holds on the node iff <= 0

Every maximum is a NodeMax(v, x, w, member, regions, lps): v the LP value, x the argmax clipped to the box, w the same quantity from a
long-double forward pass of the network at x, member the smallest s_n z_n(x) over the forced neurons at that x (long double; +inf
without forced neurons): how far outside the node the LP vertex lies.  HiGHS stops at a primal feasibility of 1e-7, so x may sit 1e-7
outside a forced half-space and w is attained on the box, not necessarily on the node: V_W_BOUND is 1e-6 here, not exact_range's 1e-9.
An empty node has no leaf: every maximum over it is -inf (a minimum +inf) with x the box centre and w = member = nan."""
from collections import namedtuple

import numpy as np
from scipy.optimize import linprog

import exact_range as er

NodeMax = namedtuple("NodeMax", "v x w member regions lps")
V_W_BOUND = 1e-6          # the generator asserts |v - w| <= V_W_BOUND (1 + |v|)


def offsets(Ms):
    return np.concatenate([[0], np.cumsum([Mk.shape[0] for Mk in Ms[:-1]])]).astype(int)


def hidden_ld(Ms, x):
    """the pre-activations of every hidden neuron at x, long double"""
    ld = np.longdouble
    h, zs = np.asarray(x, dtype=ld), []
    for Mk in Ms[:-1]:
        Mk = np.asarray(Mk, dtype=ld)
        z = Mk[:, :-1] @ h + Mk[:, -1]
        zs.append(z)
        h = np.maximum(z, ld(0))
    return np.concatenate(zs)


def membership(Ms, assign, x):
    """min over the forced n of s_n z_n(x), long double forward pass; +inf without forced neurons"""
    s = np.asarray(assign).astype(int).ravel()
    if not np.any(s != 0):
        return np.inf
    return float(np.min((s * hidden_ld(Ms, x))[s != 0]))


class _NodeSearch(er._Search):
    """the search of exact_range over a node.  Beside `leaves` it keeps, per leaf, the affine maps of all hidden pre-activations on the
    leaf: pre[i] = (Zw, Zb), z(x) = Zw x + Zb (acdim rows)"""

    def __init__(self, Ms, lo, hi, assign, deadline=None):
        super().__init__(Ms, lo, hi, deadline)
        self.Ms = [np.asarray(Mk, dtype=np.float64) for Mk in Ms]
        self.assign = np.asarray(assign).astype(int).ravel()
        self.off = offsets(self.Ms)
        assert len(self.assign) == self.off[-1] and np.all(np.abs(self.assign) <= 1)
        self.pre, self._zs = [], []

    def layer(self, k, P, q, G, g):
        if k == len(self.W) - 1:
            before = len(self.leaves)
            super().layer(k, P, q, G, g)
            if len(self.leaves) > before:
                self.pre.append((np.vstack([z[0] for z in self._zs]), np.concatenate([z[1] for z in self._zs])))
            return
        Pz, qz = self.W[k] @ P, self.W[k] @ q + self.b[k]
        self._zs.append((Pz, qz))
        self.neuron(k, 0, Pz, qz, np.zeros(len(qz)), G, g)
        self._zs.pop()

    def neuron(self, k, i, Pz, qz, d, G, g):
        s = self.assign[self.off[k] + i] if i < len(qz) else 0
        if s == 0:
            super().neuron(k, i, Pz, qz, d, G, g)
            return
        p, q = Pz[i], qz[i]
        bl, bu = self.box_range(p, q)
        if (bu < 0.0) if s > 0 else (bl > 0.0):
            return                                     # the box alone excludes the sign
        if not ((bl >= 0.0) if s > 0 else (bu <= 0.0)):        # s (p x + q) >= 0, unless the box alone grants it
            G, g = np.vstack([G, -s * p[None, :]]), np.append(g, s * q)
            if self.lp_max(np.zeros(self.n0), G, g) is None:
                return
        d2 = d.copy()
        d2[i] = 1.0 if s > 0 else 0.0
        self.neuron(k, i + 1, Pz, qz, d2, G, g)

    def lp_epi(self, F, f, G, g):
        """max over the region of min_r (F x + f)_r -> (value, x); the region is known to be feasible"""
        self.lps += 1
        nr = F.shape[0]
        A = np.vstack([np.hstack([-F, np.ones((nr, 1))]), np.hstack([G, np.zeros((len(g), 1))])])
        big = float(np.max(np.abs(F) @ np.maximum(np.abs(self.lo), np.abs(self.hi)) + np.abs(f))) + 1.0
        res = linprog(np.append(np.zeros(self.n0), -1.0), A_ub=A, b_ub=np.append(f, g), bounds=self.bounds + [(-big, big)], method="highs")
        if res.status == 2:
            return None
        if res.status != 0:
            raise RuntimeError(f"linprog: status {res.status}: {res.message}")
        return float(res.x[-1]), np.clip(res.x[:-1], self.lo, self.hi)


def node_regions(Ms, lo, hi, assign, deadline=None):
    """the feasible activation regions of the node -> the search with its leaves (none: the node is empty)"""
    s = _NodeSearch(Ms, lo, hi, assign, deadline)
    s.layer(0, np.eye(s.n0), np.zeros(s.n0), np.zeros((0, s.n0)), np.zeros(0))
    assert len(s.pre) == len(s.leaves)
    return s


def _empty(s, nrow, sign=1.0):
    return NodeMax(np.full(nrow, -sign * np.inf), np.tile(0.5 * (s.lo + s.hi), (nrow, 1)), np.full(nrow, np.nan), np.full(nrow, np.nan), 0, s.lps)


def node_max(search, C):
    """max over the node of every row of C f(x) -> NodeMax with v, w, member per row and x nrow x n0"""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    if not search.leaves:
        return _empty(search, C.shape[0])
    top = er.exact_max(search.Ms, search.lo, search.hi, C, search=search)
    return NodeMax(top.v, top.x, top.w, np.array([membership(search.Ms, search.assign, x) for x in top.x]), top.regions, top.lps)


def node_range(search, C):
    """(max, min) of every row of C f(x) over the node, the minimum with v and w negated back"""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    top, bot = node_max(search, C), node_max(search, -C)
    return top, bot._replace(v=-bot.v, w=-bot.w)


def node_pre_range(search):
    """(max, min) over the node of every hidden pre-activation, acdim rows each.  A leaf whose box bound cannot pass the best value so
    far costs no LP"""
    s, n = search, int(search.off[-1])
    if not s.leaves:
        return _empty(s, n), _empty(s, n, -1.0)
    out = []
    for sign in (1.0, -1.0):
        v, x = np.full(n, -np.inf), np.tile(0.5 * (s.lo + s.hi), (n, 1))
        for (G, g, _, _), (Zw, Zb) in zip(s.leaves, s.pre):
            for i in range(n):
                p, q = sign * Zw[i], sign * Zb[i]
                if s.box_range(p, q)[1] <= v[i]:
                    continue
                got = s.lp_max(p, G, g)
                if got is not None and got[0] + q > v[i]:
                    v[i], x[i] = got[0] + q, got[1]
        w = np.array([float(sign * hidden_ld(s.Ms, x[i])[i]) for i in range(n)])
        mem = np.array([membership(s.Ms, s.assign, x[i]) for i in range(n)])
        out.append(NodeMax(sign * v, x, sign * w, mem, len(s.leaves), s.lps))
    return tuple(out)


def node_depth(search):
    """max over the node of min over the forced n of s_n z_n(x) -> NodeMax (scalars): -inf for an empty node, +inf without forced
    neurons; otherwise >= 0"""
    s = search
    forced = np.flatnonzero(s.assign != 0)
    c = 0.5 * (s.lo + s.hi)
    if not s.leaves:
        return NodeMax(-np.inf, c, np.nan, np.nan, 0, s.lps)
    if not len(forced):
        return NodeMax(np.inf, c, np.inf, np.inf, len(s.leaves), s.lps)
    sg = s.assign[forced].astype(np.float64)
    v, x = -np.inf, c
    for (G, g, _, _), (Zw, Zb) in zip(s.leaves, s.pre):
        got = s.lp_epi(sg[:, None] * Zw[forced], sg * Zb[forced], G, g)
        if got is not None and got[0] > v:
            v, x = got
    w = membership(s.Ms, s.assign, x)
    return NodeMax(v, x, w, w, len(s.leaves), s.lps)


def clause_max(search, C, h):
    """max over the node of min_i (c_i' f(x) - h_i) -> NodeMax (scalars); -inf for an empty node"""
    s = search
    C, h = np.atleast_2d(np.asarray(C, dtype=np.float64)), np.atleast_1d(np.asarray(h, dtype=np.float64))
    c = 0.5 * (s.lo + s.hi)
    if not s.leaves:
        return NodeMax(-np.inf, c, np.nan, np.nan, 0, s.lps)
    WL, bL = s.W[-1], s.b[-1]
    v, x = -np.inf, c
    for G, g, P, q in s.leaves:
        got = s.lp_epi(C @ (WL @ P), C @ (WL @ q + bL) - h, G, g)
        if got is not None and got[0] > v:
            v, x = got
    ld = np.longdouble
    w = float(np.min(C.astype(ld) @ er.forward_ld(s.Ms, x) - h.astype(ld)))
    return NodeMax(v, x, w, membership(s.Ms, s.assign, x), len(s.leaves), s.lps)
