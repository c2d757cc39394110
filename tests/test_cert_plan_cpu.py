"""Host plan of the sparse NSD check (nnsdp_cert_plan, csrc/cert_plan.hpp) against a numpy elimination game on the oracle's clique
sets.  No GPU: symbolic elimination is integer work.

The game eliminates the vertices 0 .. n-2 of the clique graph in their stored order (the affine index a = n-1 is never eliminated):
the higher neighbours of an eliminated vertex become a clique, and every edge this adds is fill.  struct(j) = the higher neighbours of
j at its elimination.  The plan must reproduce it: a supernode is a run of columns j, j+1, ... with struct(j) = {j+1} + struct(j+1), its
row list is struct of its last column, the largest front is max_j 1 + |struct(j)|."""
import numpy as np
import pytest

import helpers
import nnsdp_amd as na
from nnsdp_amd import frontend as F
from oracle import nnet_io, operator as oop, qc

FRONT_MAX = 128
MODES = {"single": na.SingleDecomp, "double": na.DoubleDecomp, "path": na.PathDecomp, "dense": na.DenseCone}

# (xdims, beta, fill entries single / double / path, largest front single / double / path): the un-normalised pattern, a last
TABLE = [
    ([2] + [10] * 5 + [2], 0, (0, 100, 0), (31, 31, 21)),
    ([2] + [10] * 5 + [2], 3, (0, 70, 0), (34, 34, 24)),
    ([3, 7, 9, 8, 6, 7, 2], 2, (0, 49, 0), (27, 27, 20)),
    ([2] + [40] * 20 + [2], 0, (0, 25600, 0), (121, 121, 81)),
    ([2] + [40] * 20 + [2], 7, (0, 21120, 0), (128, 128, 88)),
    ([5] + [50] * 6 + [5], 1, (0, 4900, 0), (152, 152, 102)),
    ([2] + [20] * 30 + [2], 7, (0, 6760, 0), (68, 68, 48)),
]


def elimination_game(n, cliques):
    adj = np.zeros((n, n), dtype=bool)
    for c in cliques:
        adj[np.ix_(c, c)] = True
    np.fill_diagonal(adj, False)
    fill, struct = 0, []
    for j in range(n - 1):
        nb = np.nonzero(adj[j, j + 1:])[0] + j + 1
        sub = adj[np.ix_(nb, nb)]
        fill += (len(nb) * (len(nb) - 1) - int(sub.sum())) // 2
        adj[np.ix_(nb, nb)] = True
        adj[nb, nb] = False
        struct.append(nb.tolist())
    return fill, struct


def hplane_query(xdims, beta, seed=7):
    """a reach-hyperplane query on a random network (every decomposition fits it: no x_1 -- x_K coupling)"""
    net = na.randomNetwork(xdims, seed=seed)
    lo, hi = np.full(xdims[0], 0.25), np.full(xdims[0], 0.35)
    xi, acx = F.intervalsWorstCase(lo, hi, net)
    nrm = np.zeros(xdims[-1])
    nrm[0] = 1.0
    return na.ReachQuery(ffnet=net, qc_input=na.QcInputBox(x1min=lo, x1max=hi), qc_reach=na.QcReachHplane(normal=nrm),
                         qc_activs=F.makeQcActivsIntvs(net, xi, acx, beta))


def check_against_game(plan, n, cliques):
    fill, struct = elimination_game(n, cliques)
    assert plan["n"] == n
    assert plan["fill"] == fill
    cs = plan["col_start"]
    assert cs[0] == 0 and cs[-1] == n - 1 and all(b > a for a, b in zip(cs, cs[1:]))
    for s, rows in enumerate(plan["rows"]):
        assert rows[-1] == n - 1, "the affine index is the last row of every front"
        for j in range(cs[s], cs[s + 1]):
            assert struct[j] == list(range(j + 1, cs[s + 1])) + rows, (s, j)
    assert plan["max_front"] == max(1 + len(t) for t in struct)
    assert plan["supported"] == (plan["max_front"] <= FRONT_MAX)
    return fill


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_plan_equals_elimination_game(row):
    xdims, beta, fills, fronts = TABLE[row]
    q = hplane_query(xdims, beta)
    onet = nnet_io.FeedFwdNet(xdims=list(xdims), Ms=q.ffnet.Ms)
    n = sum(xdims[:-1]) + 1
    for mode, fill, front in zip(("single", "double", "path"), fills, fronts):
        plan = na.certPlan(q, na.AdmmSdpOptions(decomp_mode=MODES[mode](), normalize=False))
        check_against_game(plan, n, qc.clique_index_sets(onet, beta, mode))
        assert (plan["fill"], plan["max_front"]) == (fill, front), (mode, plan["fill"], plan["max_front"])
        assert plan["supported"] == (front <= FRONT_MAX)
        assert plan["n_super"] == len(plan["rows"]) == len(plan["col_start"]) - 1


def test_dense_cone_is_one_front():
    xdims, beta = TABLE[0][0], TABLE[0][1]
    q = hplane_query(xdims, beta)
    n = sum(xdims[:-1]) + 1
    plan = na.certPlan(q, na.AdmmSdpOptions(decomp_mode=MODES["dense"](), normalize=False))
    check_against_game(plan, n, [list(range(n))])
    assert (plan["n_super"], plan["max_front"], plan["fill"], plan["supported"]) == (1, n, 0, True)
    assert plan["rows"] == [[n - 1]]


@pytest.mark.parametrize("name,beta", [("W10-D5", 0), ("W10-D10", 2)])
def test_plan_of_the_normalised_solver_pattern(name, beta):
    """reach query, coordinates eliminated by the normalisation: the plan works on the solver's reduced pattern"""
    d = helpers.load_problem(name, beta)
    plan = na.certPlan(helpers.product_query(d), na.AdmmSdpOptions(normalize=True))
    L = oop.build_operator(helpers.oracle_query(d), "single", normalize=True)
    n = L.pat.Zdim
    assert n < sum(int(v) for v in d["xdims"][:-1]) + 1, "the fixture is expected to have eliminated coordinates"
    assert plan["n"] == n
    check_against_game(plan, n, [c.tolist() for c in L.pat.cliques])
    covered = np.zeros((n, n), dtype=bool)
    cs = plan["col_start"]
    for s, rows in enumerate(plan["rows"]):
        front = list(range(cs[s], cs[s + 1])) + rows
        covered[np.ix_(front, front)] = True
    assert np.all(covered[L.pat.rows, L.pat.cols]), "a pattern entry lies in no front"
    assert plan["supported"]
