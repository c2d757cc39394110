"""Shared by the ReLU-split tests (test_relu_split_cpu.py, test_relu_split_gpu.py): `R`, a numpy restatement of the node passes of
DESIGN.md section 5 ("Branching on unstable ReLUs") in any float type, the node generators, and the checks that the float32 host
routine (makeIntervalsNodes) and the kernels (CrownBounder.bound_nodes) share.  Nothing here needs a GPU.

A node is built from a point: draw x0 in the box and force a random subset of the neurons to the sign of z(x0).  Such a node is
non-empty by construction (x0 is in it), so no case is ever left out."""
import numpy as np

import crown_alpha_common as ca
import exact_common as xc
import literal_common as lc
import nnsdp_amd as na

_cache = {}
NETS = ca.NETS                      # 3-17-33-4, 1-64-64-2, 5-20-5: forced neurons on both sides of the 16-row tiles, width 64, n0 = 1
STEPS = (0, 1, 3, 8, 16)


def _wb(Ms, dt):
    return [np.asarray(Mk[:, :-1], dtype=dt) for Mk in Ms], [np.asarray(Mk[:, -1], dtype=dt) for Mk in Ms]


def offsets(xdims):
    return np.concatenate([[0], np.cumsum(xdims[1:-1])]).astype(int)


def hidden64(net, x):
    """the pre-activations of every hidden neuron at x (n0,) or X (n0 x N), float64: acdim (x N)"""
    a, zs = np.asarray(x, dtype=np.float64), []
    for Mk in net.Ms[:-1]:
        z = Mk[:, :-1] @ a + (Mk[:, -1] if a.ndim == 1 else Mk[:, -1:])
        zs.append(z)
        a = np.maximum(z, 0.0)
    return np.concatenate(zs, axis=0)


def R(Ms, lo, hi, s, Cm, steps=0, eta0=0.5, decay=0.9, dt=np.float64):
    """one node (lo, hi: n0; s: acdim in {-1, 0, 1}) -> dict: pre_lo, pre_hi (clipped), smin, smax_plain, smax, A, b0, best_step, branch,
    infeasible, gap (per literal the difference of the two best branching scores, inf with fewer than two candidates), beta (nlit x acdim)"""
    W, b = _wb(Ms, dt)
    K, zero, one = len(W), dt(0), dt(1)
    xd = [W[0].shape[1]] + [w.shape[0] for w in W]
    off = offsets(xd)
    lo, hi = np.asarray(lo, dtype=dt), np.asarray(hi, dtype=dt)
    c, r = (hi + lo) / dt(2), (hi - lo) / dt(2)
    s = np.asarray(s)
    rel = []                        # per hidden layer: du, dl, bu, candidates, the signs as dt

    def backward(A, cst, top, upper, beta=None):
        lam = [None] * (top + 1)
        for j in range(top, -1, -1):
            du, dl, bu, _, sj = rel[j]
            lam[j] = A
            Ap, An = np.maximum(A, zero), np.minimum(A, zero)
            cst = cst + (Ap if upper else An) @ bu
            A = Ap * du + An * dl if upper else Ap * dl + An * du
            if beta is not None:
                A = A + sj * beta[j]
            cst = cst + A @ b[j]
            A = A @ W[j]
        val = A @ c + (np.abs(A) @ r if upper else -(np.abs(A) @ r)) + cst
        return val, A, cst, lam

    pre_lo, pre_hi, infeasible = [], [], False
    for k in range(K - 1):
        l = backward(W[k].copy(), b[k].copy(), k - 1, False)[0]
        u = backward(W[k].copy(), b[k].copy(), k - 1, True)[0]
        sk = s[off[k]:off[k + 1]]
        l = np.where(sk > 0, np.maximum(l, zero), l)
        u = np.where(sk < 0, np.minimum(u, zero), u)
        infeasible = infeasible or bool(np.any(l > u))
        lr = np.minimum(l, zero)
        ur = np.maximum(np.maximum(u, zero), lr + dt(1e-8))
        du = ur / (ur - lr)
        dl = (du > dt(0.5)).astype(dt)
        bu = -lr * du
        du, dl, bu = np.where(sk > 0, one, np.where(sk < 0, zero, du)), np.where(sk > 0, one, np.where(sk < 0, zero, dl)), np.where(sk != 0, zero, bu)
        rel.append((du, dl, bu, (sk == 0) & (l < zero) & (u > zero), sk.astype(dt)))
        pre_lo.append(l)
        pre_hi.append(u)
    Cm = np.asarray(Cm, dtype=dt)
    Hw, Hb = Cm @ W[K - 1], Cm @ b[K - 1]
    nlit = Cm.shape[0]
    smin = backward(Hw.copy(), Hb.copy(), K - 2, False)[0]
    beta = [np.zeros((nlit, w.shape[0]), dtype=dt) for w in W[:-1]]
    live = np.ones(nlit, dtype=bool)
    best = None
    for t in range(steps + 1):
        smax, A, cst, lam = backward(Hw.copy(), Hb.copy(), K - 2, True, beta)
        if best is None:
            score = np.concatenate([np.where(rel[j][3][None, :], np.maximum(lam[j], zero) * rel[j][2][None, :], -one) for j in range(K - 1)], axis=1)
            branch = np.where(score.max(axis=1) >= zero, np.argmax(score, axis=1), -1).astype(np.int32)
            top2 = -np.sort(-score, axis=1)[:, :2] if score.shape[1] > 1 else np.concatenate([score, -np.ones_like(score)], axis=1)
            gap = np.where(top2[:, 1] >= zero, top2[:, 0] - top2[:, 1], np.inf)
            best = dict(smax_plain=smax.copy(), smax=smax.copy(), A=A.copy(), b0=cst.copy(), best_step=np.zeros(nlit, dtype=np.int32),
                        beta=np.concatenate(beta, axis=1))
        else:
            m = smax < best["smax"]
            best["smax"][m], best["A"][m], best["b0"][m], best["best_step"][m] = smax[m], A[m], cst[m], t
            best["beta"][m] = np.concatenate(beta, axis=1)[m]
        if t == steps:
            break
        a = c[None, :] + np.sign(A) * r[None, :]
        g = []
        for j in range(K - 1):
            du, dl, bu, _, sj = rel[j]
            z = a @ W[j].T + b[j]
            g.append(sj[None, :] * z)
            a = np.where(lam[j] > zero, du * z + bu, dl * z)
        gmax = np.max(np.abs(np.concatenate(g, axis=1)), axis=1)
        live &= gmax > 0
        if not live.any():
            break
        scale = np.where(live, dt(eta0) * dt(decay) ** t / np.where(gmax > 0, gmax, one), zero)
        beta = [np.maximum(bj - scale[:, None] * gj, zero) for bj, gj in zip(beta, g)]
    return dict(pre_lo=np.concatenate(pre_lo), pre_hi=np.concatenate(pre_hi), smin=smin, branch=branch, gap=gap, infeasible=infeasible, **best)


# ---- nodes
def node_from_point(net, lo, hi, rng, frac):
    """x0 uniform in the box, every hidden neuron forced with probability frac to the sign of z(x0) (+1 at z = 0) -> x0, assign (int8)"""
    x0 = lo + rng.random(len(lo)) * (hi - lo)
    z = hidden64(net, x0)
    s = np.where(rng.random(len(z)) < frac, np.where(z >= 0.0, 1, -1), 0).astype(np.int8)
    return x0, s


def kernel_cases():
    """per net of NETS: net, C (7 literals), and six nodes on boxes of half-width 0.05 / 0.3 / 1 around seeded centres with 10 % / 40 % of
    the neurons forced: lo, hi (n0 x 6), assign (acdim x 6), x0 (n0 x 6)"""
    if "kernel" not in _cache:
        out = []
        for xdims, seed in NETS:
            net, rng = lc.random_net(xdims, seed), np.random.default_rng(seed + 900)
            los, his, ss, x0s = [], [], [], []
            for hw in (0.05, 0.3, 1.0):
                for frac in (0.1, 0.4):
                    ctr = rng.uniform(-0.5, 0.5, xdims[0])
                    x0, s = node_from_point(net, ctr - hw, ctr + hw, rng, frac)
                    los.append(ctr - hw), his.append(ctr + hw), ss.append(s), x0s.append(x0)
            out.append(dict(net=net, C=lc.literal_rows(xdims[-1], 7, seed + 100), lo=np.stack(los, 1), hi=np.stack(his, 1),
                            assign=np.stack(ss, 1), x0=np.stack(x0s, 1)))
        _cache["kernel"] = out
    return _cache["kernel"]


def full_nodes(net, lo, hi, count, seed):
    """`count` nodes of the box lo / hi with every neuron forced to the pattern of a seeded point: assign (acdim x count), x0 (n0 x count)"""
    rng = np.random.default_rng(seed)
    got = [node_from_point(net, lo, hi, rng, 2.0) for _ in range(count)]
    return np.stack([s for _, s in got], 1), np.stack([x for x, _ in got], 1)


def affine_of_pattern(net, s):
    """on a fully forced node the network is affine: f(x) = Weff x + beff, and the pre-activations z(x) = Zw x + Zb (acdim rows)"""
    n0 = net.xdims[0]
    Wa, ba, Zw, Zb, o = np.eye(n0), np.zeros(n0), [], [], 0
    for Mk in net.Ms[:-1]:
        Wz, bz = Mk[:, :-1] @ Wa, Mk[:, :-1] @ ba + Mk[:, -1]
        Zw.append(Wz), Zb.append(bz)
        d = (s[o:o + Mk.shape[0]] > 0).astype(np.float64)
        Wa, ba, o = d[:, None] * Wz, d * bz, o + Mk.shape[0]
    return net.Ms[-1][:, :-1] @ Wa, net.Ms[-1][:, :-1] @ ba + net.Ms[-1][:, -1], np.vstack(Zw), np.concatenate(Zb)


def tols(net, Cm, lo, hi, host):
    """the slack of a bound on pre-activations and on literals: the float32 host routine has HOST_SLACK (1 + |v|); an fp64 kernel has
    exact_common.fp64_tols on the node's box (acymax for the hidden bounds, smax for the literals) -> (tol_pre(v), tol_lit(v))"""
    if host:
        return (lambda v: xc.HOST_SLACK * (1.0 + np.abs(v)),) * 2
    t = xc.fp64_tols(dict(net=net, C=Cm), lo[:, None], hi[:, None])
    return (lambda v: t["acymax"] + 0.0 * np.abs(v)), (lambda v: t["smax"] + 0.0 * np.abs(v))


# ---- the checks that both routes share; run(net, lo, hi, assign, C, steps) -> na.NodeBounds
def check_fully_forced(run, host):
    """test 2: every neuron forced to the pattern of x0, steps = 0: smax = |c' Weff| r + c' Weff xc + c' beff to 1e-12 (1 + |v|) in fp64
    (the host routine: HOST_SLACK)"""
    for cs in kernel_cases():
        net, Cm, lo, hi = cs["net"], cs["C"], cs["lo"], cs["hi"]
        s = np.stack([np.where(hidden64(net, cs["x0"][:, b]) >= 0.0, 1, -1) for b in range(lo.shape[1])], 1).astype(np.int8)
        nb = run(net, lo, hi, s, Cm, 0)
        assert not nb.infeasible.any()
        worst = 0.0
        for b in range(lo.shape[1]):
            We, be, _, _ = affine_of_pattern(net, s[:, b])
            cW, c, r = Cm @ We, 0.5 * (lo[:, b] + hi[:, b]), 0.5 * (hi[:, b] - lo[:, b])
            want = np.abs(cW) @ r + cW @ c + Cm @ be
            worst = max(worst, float(np.max(np.abs(nb.smax[:, b] - want) / (1.0 + np.abs(want)))))
            assert np.array_equal(nb.smax[:, b], nb.smax_plain[:, b]) and not nb.best_step[:, b].any()
            assert np.all(nb.branch[:, b] == -1)
        print(f"{net.xdims}: fully forced, max |smax - affine| / (1 + |v|) = {worst:.3e}")
        assert worst <= (xc.HOST_SLACK if host else 1e-12)


def satisfying_samples(net, lo, hi, s, x0, seed, want=2000, batches=20):
    """x0 and up to `want` uniform points of the box that satisfy the assignment (drawn 2000 at a time, at most `batches` draws)"""
    rng, keep, have = np.random.default_rng(seed), [x0[:, None]], 0
    forced = s != 0
    for _ in range(batches):
        X = lo[:, None] + rng.random((len(lo), 2000)) * (hi - lo)[:, None]
        ok = np.all((hidden64(net, X) * s[:, None])[forced] >= 0.0, axis=0)
        keep.append(X[:, ok])
        have += int(ok.sum())
        if have >= want:
            break
    return np.concatenate(keep, axis=1)[:, :want + 1]


def check_partial(run, host, steps=(0, 8)):
    """test 3: the clipped pre-activation bounds enclose z(x) and smax >= c' f(x) - tol at x0 and at the satisfying samples;
    smax <= smax_plain; a node built from a point is never infeasible"""
    for n, cs in enumerate(kernel_cases()):
        net, Cm, lo, hi, s = cs["net"], cs["C"], cs["lo"], cs["hi"], cs["assign"]
        for T in steps:
            nb = run(net, lo, hi, s, Cm, T)
            assert not nb.infeasible.any(), (net.xdims, T)
            assert np.all(nb.smax <= nb.smax_plain) and np.all((nb.best_step >= 0) & (nb.best_step <= T))
            for b in range(lo.shape[1]):
                X = satisfying_samples(net, lo[:, b], hi[:, b], s[:, b], cs["x0"][:, b], 40 + n)
                Z, Y = hidden64(net, X), Cm @ lc.forward(net, X)
                tp, tl = tols(net, Cm, lo[:, b], hi[:, b], host)
                assert np.all(nb.pre_lo[:, b, None] <= Z + tp(Z)) and np.all(nb.pre_hi[:, b, None] >= Z - tp(Z)), (net.xdims, T, b)
                assert np.all(nb.smax[:, b, None] >= Y - tl(Y)) and np.all(nb.smin[:, b, None] <= Y + tl(Y)), (net.xdims, T, b)
                forced = s[:, b]
                assert np.all(nb.pre_lo[forced > 0, b] >= 0.0) and np.all(nb.pre_hi[forced < 0, b] <= 0.0)
                if T == steps[0]:
                    print(f"{net.xdims} node {b}: {int((forced != 0).sum())} forced, {X.shape[1]} points, "
                          f"smax - max c'f = {float(np.min(nb.smax[:, b] - Y.max(axis=1))):.3e}")


def check_forced_infeasible(run):
    """test 4: force a neuron against a sign that the plain bounds already decide (+1 where u < 0, -1 where l > 0)"""
    hits = 0
    for cs in kernel_cases():
        net, Cm, lo, hi = cs["net"], cs["C"], cs["lo"], cs["hi"]
        zero = np.zeros_like(cs["assign"])
        plain = run(net, lo, hi, zero, Cm, 0)
        assert not plain.infeasible.any()
        s, expect = zero.copy(), np.zeros(lo.shape[1], dtype=bool)
        for b in range(lo.shape[1]):
            neg, pos = np.flatnonzero(plain.pre_hi[:, b] < -1e-3), np.flatnonzero(plain.pre_lo[:, b] > 1e-3)
            if len(neg) and (b % 2 == 0 or not len(pos)):
                s[neg[len(neg) // 2], b], expect[b] = 1, True
            elif len(pos):
                s[pos[len(pos) // 2], b], expect[b] = -1, True
        hits += int(expect.sum())
        nb = run(net, lo, hi, s, Cm, 3)
        assert np.array_equal(nb.infeasible, expect), (net.xdims, nb.infeasible, expect)
    assert hits >= 6


def toy():
    """net [1, 2, 1]: z = (x, x + 1), output relu(z_2), box [-1, 1], neuron 1 forced -1 (x <= 0): the true maximum is 1, the plain
    bound 2, the optimum over the multiplier 1 at beta = 1"""
    net = na.FeedFwdNet(xdims=[1, 2, 1], Ms=[np.array([[1.0, 0.0], [1.0, 1.0]]), np.array([[0.0, 1.0, 0.0]])])
    return net, np.array([[-1.0]]), np.array([[1.0]]), np.array([[-1], [0]], dtype=np.int8), np.array([[1.0]])


def check_toy(run, host):
    """test 6: steps = 8 with the default step sizes: 1 - tol <= smax <= 1.5, and smax_plain = 2"""
    net, lo, hi, s, Cm = toy()
    nb = run(net, lo, hi, s, Cm, 8)
    tol = xc.HOST_SLACK * 2.0 if host else 1e-12
    print(f"toy: smax_plain {nb.smax_plain[0, 0]:.6f}, smax {nb.smax[0, 0]:.6f} at step {nb.best_step[0, 0]}")
    assert abs(nb.smax_plain[0, 0] - 2.0) <= tol and not nb.infeasible[0]
    assert 1.0 - tol <= nb.smax[0, 0] <= 1.5
    assert nb.pre_hi[0, 0] == 0.0 and nb.pre_lo[0, 0] == -1.0


def check_lp_truth(run, host):
    """test 7: fully forced nodes of 2-8-8-2 and 3-10-10-3 (row 0 of the fixture's literals, the root box), steps = 16:
    smax >= the maximum over the node from tests/node_truth.py (one LP over box and sign half-spaces), minus tol.  The gaps are printed"""
    import node_truth as nt
    for name in xc.SMALL:
        st = xc.verdict_setting(name)
        net, lo, hi, Cm = st["net"], st["lo"], st["hi"], st["normal"][None, :]
        s, _ = full_nodes(net, lo, hi, 12, 321)
        nn = s.shape[1]
        nb = run(net, np.repeat(lo[:, None], nn, 1), np.repeat(hi[:, None], nn, 1), s, Cm, 16)
        assert not nb.infeasible.any()
        for b in range(nn):
            top = nt.node_max(nt.node_regions(net.Ms, lo, hi, s[:, b]), Cm)
            assert top.regions == 1, (name, b, top.regions)
            v = float(top.v[0])
            # HiGHS stops at a primal feasibility of 1e-7: its vertex may lie that far outside the node
            tol = (xc.HOST_SLACK if host else 1e-6) * (1.0 + abs(v))
            print(f"{name} node {b}: LP {v:.9f}  smax {nb.smax[0, b]:.9f} (plain {nb.smax_plain[0, b]:.9f}, step {nb.best_step[0, b]})  gap {nb.smax[0, b] - v:.3e}")
            assert nb.smax[0, b] >= v - tol, (name, b)


def r_tolerance(cs, b, T):
    """what tests/test_crown_alpha_gpu.py allows a_smax against its yardstick: 8 r, r = max |R(float64) - R(long double)| / (1 + |v|)
    of the compared arrays -> (R in long double, tolerance)"""
    args = (cs["net"].Ms, cs["lo"][:, b], cs["hi"][:, b], cs["assign"][:, b], cs["C"], T)
    r64, rld = R(*args, dt=np.float64), R(*args, dt=np.longdouble)
    r = max(ca.rel_err(r64[k], rld[k]) for k in ("smax", "A", "b0"))
    return rld, 8.0 * r


def check_yardstick(cs, nb, T):
    """smax, uA, ub0 within 8 r of R(long double), best_step equal; branch equal wherever the two best scores differ by more than that;
    the infeasible flag equal"""
    for b in range(cs["lo"].shape[1]):
        ref, tol = r_tolerance(cs, b, T)
        errs = [ca.rel_err(got, ref[k]) for got, k in ((nb.smax[:, b], "smax"), (nb.A[:, :, b], "A"), (nb.b0[:, b], "b0"))]
        print(f"{cs['net'].xdims} node {b} T {T}: err {max(errs):.3e}  tol {tol:.3e}  steps gpu {nb.best_step[:, b].tolist()} R {ref['best_step'].tolist()}")
        assert max(errs) <= tol, (b, errs, tol)
        assert np.array_equal(nb.best_step[:, b], ref["best_step"]), b
        clear = np.asarray(ref["gap"], dtype=np.float64) > tol * (1.0 + np.abs(np.asarray(ref["smax_plain"], dtype=np.float64)))
        assert np.array_equal(nb.branch[clear, b], ref["branch"][clear]), b
        assert bool(nb.infeasible[b]) == ref["infeasible"]


# ---- the driver
def literal_threshold(st, rel):
    return st["v"] + rel * (st["c0"] - st["v"])


def check_tree(res, acdim):
    """the leaves' assignments partition the tree: from the root, every internal node has exactly its two children"""
    nodes = {tuple(int(v) for v in lf.assign) for lf in list(res.leaves) + list(res.open)}
    assert len(nodes) == len(res.leaves) + len(res.open)

    def walk(prefix_nodes, fixed):
        """the leaves that agree with `fixed` (dict neuron -> sign): one leaf with exactly these forced, or a split on one more neuron"""
        if len(prefix_nodes) == 1:
            only = next(iter(prefix_nodes))
            assert {n for n, v in enumerate(only) if v != 0} == set(fixed), "a leaf forces more than its path"
            return
        assert len(prefix_nodes) > 1
        shared = [n for n in range(acdim) if n not in fixed and all(a[n] != 0 for a in prefix_nodes)]
        assert shared, "no neuron splits these leaves"
        n = shared[0]
        plus, minus = {a for a in prefix_nodes if a[n] > 0}, {a for a in prefix_nodes if a[n] < 0}
        assert plus and minus, "an internal node with one child"
        walk(plus, {**fixed, n: 1})
        walk(minus, {**fixed, n: -1})

    walk(nodes, {})


def check_driver_small(backend, name):
    """test 9 on a fixture net: for every rel of exact_common.RELS the true verdict within max_nodes = 4096, never "unknown" """
    st = xc.verdict_setting(name)
    acdim = sum(st["net"].xdims[1:-1])
    for rel in xc.RELS:
        h = literal_threshold(st, rel)
        res = na.verifyReluSplit(st["net"], st["lo"], st["hi"], [(st["normal"], h)], na.ReluSplitOptions(max_nodes=4096, crown_backend=backend))
        print(f"{name} {backend} rel {rel:+.0e}: {res.verdict} ({res.reason}), visited {res.visited}, depth {res.depth}, "
              f"{len(res.leaves)} leaves, {len(res.open)} open")
        truth = "holds" if rel > 0 else "violated"
        if res.verdict == "violated":
            x = res.witness
            assert x is not None and np.all(x >= st["lo"]) and np.all(x <= st["hi"])
            assert st["normal"] @ xc.forward64(st["net"], x) > h
        if res.verdict == "holds":
            assert res.witness is None and not res.open
            assert all((lf.closed_by == "bound" and lf.bound <= h) or lf.closed_by == "infeasible" for lf in res.leaves)
        check_tree(res, acdim)
        assert res.verdict == truth, (name, rel, res.verdict, res.reason, res.visited)
        assert res.visited <= 4096


def check_driver_16(backend):
    """test 9: lc.random_net([16, 16, 16, 2], 7), box [-0.5, 0.5]^16, literal (1, -1), h = 0.95: "holds" within max_nodes = 1024"""
    net = lc.random_net([16, 16, 16, 2], 7)
    lo, hi = -0.5 * np.ones(16), 0.5 * np.ones(16)
    res = na.verifyReluSplit(net, lo, hi, [(np.array([1.0, -1.0]), 0.95)], na.ReluSplitOptions(max_nodes=1024, crown_backend=backend))
    print(f"16-16-16-2 {backend}: {res.verdict} ({res.reason}), visited {res.visited}, depth {res.depth}, seconds {res.seconds}")
    assert res.verdict == "holds" and res.visited <= 1024
    assert all((lf.closed_by == "bound" and lf.bound <= 0.95) or lf.closed_by == "infeasible" for lf in res.leaves)
    check_tree(res, 32)
