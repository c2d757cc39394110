"""The exact-range oracle (tests/exact_range.py) checks itself, the fixture tests/golden/exact_ranges.json is what the oracle gives, and
the parts of the product that need no GPU (the float32 host routine, the split driver with crown_backend="host") are held against it:
bounds must respect values the network attains, verdicts must be the true ones.  tests/test_exact_soundness_gpu.py does the same for the
kernels."""
import itertools

import numpy as np
import pytest

import exact_common as ec
import exact_range as er
import literal_common as lc
import nnsdp_amd as na

ONE_D = [([1, 6, 6, 1], seed, hw) for seed, hw in ((3, 1.0), (4, 1.0), (5, 3.0), (6, 3.0))]


def f64(Ms, X):
    for Mk in Ms[:-1]:
        X = np.maximum(Mk[:, :-1] @ X + Mk[:, -1:], 0.0)
    return Ms[-1][:, :-1] @ X + Ms[-1][:, -1:]


def breakpoints(Ms, lo, hi):
    """the kinks of a 1-input ReLU net on [lo, hi], layer by layer: on a segment where the layers before are affine every
    pre-activation is p x + q, and its root, where it lies inside the segment, is a kink; sorted, with the two ends"""
    pts = [lo, hi]
    for k in range(len(Ms) - 1):
        new = []
        for a, b in zip(pts[:-1], pts[1:]):
            za, zb = np.array([a]), np.array([b])
            for Mj in Ms[:k]:
                za, zb = np.maximum(Mj[:, :-1] @ za + Mj[:, -1], 0.0), np.maximum(Mj[:, :-1] @ zb + Mj[:, -1], 0.0)
            za, zb = Ms[k][:, :-1] @ za + Ms[k][:, -1], Ms[k][:, :-1] @ zb + Ms[k][:, -1]
            cross = za * zb < 0
            new += list(a + (b - a) * za[cross] / (za[cross] - zb[cross]))
        pts = sorted(set(pts + new))
    return np.array(pts)


@pytest.mark.parametrize("xdims,seed,hw", ONE_D)
def test_one_input_nets_against_breakpoints_and_a_grid(xdims, seed, hw):
    """a piecewise-linear function of one variable has its extrema at kinks or ends: v equals the extremum over them to 1e-12; and a
    10^6-point grid never exceeds v (1e-12) and comes within L * spacing of it"""
    Ms = lc.random_net(xdims, seed).Ms
    lo, hi = np.array([-hw]), np.array([hw])
    top, bot = er.exact_range(Ms, lo, hi, np.ones((1, 1)))
    bp = f64(Ms, breakpoints(Ms, -hw, hw)[None, :])[0]
    grid = f64(Ms, np.linspace(-hw, hw, 10 ** 6)[None, :])[0]
    L, spacing = er.lipschitz(Ms, np.ones(1)), 2.0 * hw / (10 ** 6 - 1)
    print(f"seed {seed} hw {hw}: {top.regions} regions, {len(bp)} breakpoints, max {top.v[0]:.12f} min {bot.v[0]:.12f}, L {L:.3f}")
    assert top.regions >= 3, "the instance must have kinks"
    assert abs(top.v[0] - bp.max()) <= 1e-12 and abs(bot.v[0] - bp.min()) <= 1e-12
    assert grid.max() <= top.v[0] + 1e-12 and top.v[0] - grid.max() <= L * spacing
    assert grid.min() >= bot.v[0] - 1e-12 and grid.min() - bot.v[0] <= L * spacing
    assert abs(top.v[0] - top.w[0]) <= er.V_W_BOUND * (1 + abs(top.v[0])) and abs(bot.v[0] - bot.w[0]) <= er.V_W_BOUND * (1 + abs(bot.v[0]))


def test_the_linear_term():
    """c' f(x) - a' x on a 1-input net against the breakpoints"""
    Ms = lc.random_net([1, 6, 6, 1], 3).Ms
    bp = breakpoints(Ms, -1.0, 1.0)
    for a in (0.7, -0.4):
        r = er.exact_max(Ms, np.array([-1.0]), np.array([1.0]), np.ones(1), a=np.array([a]))
        assert abs(r.v - (f64(Ms, bp[None, :])[0] - a * bp).max()) <= 1e-12 and abs(r.v - r.w) <= 1e-12


def test_the_fixture_is_complete():
    """a missing case is an error, not a skip: the two small nets with their eight boxes, and the "holds" instance; a case the generator
    left out for its time cap is named in the header and absent"""
    fx = ec.fixture()
    for name in ec.SMALL:
        cs = ec.case(name)
        assert [bx["name"] for bx in cs["boxes"]] == list(ec.BOX_NAMES)
        n0, acdim, nrow = cs["net"].xdims[0], sum(cs["net"].xdims[1:-1]), len(cs["C"])
        for bx in cs["boxes"]:
            assert bx["lit"]["vmax"].shape == (nrow,) and bx["lit"]["xmin"].shape == (nrow, n0)
            assert bx["pre"]["vmax"].shape == bx["post"]["wmin"].shape == (acdim,)
            assert np.all(bx["lo"] <= bx["hi"])
        by = dict(zip(ec.BOX_NAMES, cs["boxes"]))
        assert np.array_equal(by["point"]["lo"], by["point"]["hi"]) and np.allclose(by["stable"]["hi"] - by["stable"]["lo"], 2e-6, rtol=1e-6)
        assert by["stable"]["regions"] == [1] * len(cs["net"].Ms) and by["root"]["regions"][-1] > 40
        assert (np.abs(by["edge0"]["pre"]["vmax"][:cs["net"].xdims[1]]) <= 1e-15).any(), "a first-layer pre-activation whose maximum is 0"
    assert "holds" in fx["cases"] and ec.case("holds")["boxes"][0]["regions"] == [4431]
    assert set(fx["header"]["left_out"]).isdisjoint(fx["cases"]) and set(fx["header"]["left_out"]) <= {"W10-D5", "violated"}
    assert set(fx["cases"]) | set(fx["header"]["left_out"]) == set(ec.SMALL) | {"holds", "W10-D5", "violated"}


def test_every_recorded_value_is_attained():
    """|v - w| within the bound the generator asserted, v_min <= v_max, and the argmax / argmin lie in the box and give w back"""
    for name in ec.fixture()["cases"]:
        cs = ec.case(name)
        for bx in cs["boxes"]:
            for blk in ("lit", "pre", "post"):
                if blk not in bx:
                    continue
                d = bx[blk]
                for v, w, x in ((d["vmax"], d["wmax"], d["xmax"]), (d["vmin"], d["wmin"], d["xmin"])):
                    assert np.all(np.abs(v - w) <= er.V_W_BOUND * (1 + np.abs(v))), (name, bx["name"], blk)
                    assert np.all(x >= bx["lo"]) and np.all(x <= bx["hi"])
                assert np.all(d["vmin"] <= d["vmax"] + 1e-12)
            again = np.array([float(cs["C"][i].astype(np.longdouble) @ er.forward_ld(cs["net"].Ms, bx["lit"]["xmax"][i])) for i in range(len(cs["C"]))])
            assert np.array_equal(again, bx["lit"]["wmax"]), (name, bx["name"])


def test_no_sample_passes_the_exact_range():
    """20 000 seeded points per box: every literal row, every hidden pre- and post-activation inside [v_min, v_max] (1e-12)"""
    for name in ec.fixture()["cases"]:
        cs = ec.case(name)
        Ms, n0 = cs["net"].Ms, cs["net"].xdims[0]
        rng = np.random.default_rng(9)
        for bx in cs["boxes"]:
            X = bx["lo"][:, None] + rng.random((n0, 20000)) * (bx["hi"] - bx["lo"])[:, None]
            pre, post = [], []
            for Mk in Ms[:-1]:
                pre.append(Mk[:, :-1] @ X + Mk[:, -1:])
                X = np.maximum(pre[-1], 0.0)
                post.append(X)
            vals = dict(lit=cs["C"] @ (Ms[-1][:, :-1] @ X + Ms[-1][:, -1:]), pre=np.concatenate(pre), post=np.concatenate(post))
            for blk, val in vals.items():
                if blk in bx:
                    assert np.all(val.max(axis=1) <= bx[blk]["vmax"] + 1e-12) and np.all(val.min(axis=1) >= bx[blk]["vmin"] - 1e-12), (name, bx["name"], blk)


@pytest.mark.parametrize("name", list(ec.SMALL))
def test_on_the_stable_box_the_network_is_affine(name):
    """v equals the extremum over the corners of the box, to 1e-12"""
    cs = ec.case(name)
    bx = cs["boxes"][ec.BOX_NAMES.index("stable")]
    corners = np.array(list(itertools.product(*zip(bx["lo"], bx["hi"])))).T
    val = cs["C"] @ f64(cs["net"].Ms, corners)
    assert np.all(np.abs(val.max(axis=1) - bx["lit"]["vmax"]) <= 1e-12) and np.all(np.abs(val.min(axis=1) - bx["lit"]["vmin"]) <= 1e-12)


@pytest.mark.parametrize("name", list(ec.SMALL))
def test_the_fixture_is_what_the_oracle_gives(name):
    """re-enumerated here: the root box for the literal y_0 - y_last (regions and both extrema), and every stored row of the cheap boxes"""
    cs = ec.case(name)
    Ms = cs["net"].Ms
    root = cs["boxes"][0]
    top, bot = er.exact_range(Ms, root["lo"], root["hi"], cs["C"][:1])
    assert top.regions == root["regions"][-1]
    assert abs(top.v[0] - root["lit"]["vmax"][0]) <= 1e-12 and abs(bot.v[0] - root["lit"]["vmin"][0]) <= 1e-12
    for bname in ("small-b", "stable", "point", "edge0"):
        bx = cs["boxes"][ec.BOX_NAMES.index(bname)]
        top, bot = er.exact_range(Ms, bx["lo"], bx["hi"], cs["C"])
        assert top.regions == bx["regions"][-1], bname
        assert np.all(np.abs(top.v - bx["lit"]["vmax"]) <= 1e-12) and np.all(np.abs(bot.v - bx["lit"]["vmin"]) <= 1e-12), bname
        # a hidden neuron through the same function: the network cut after the first layer, a unit row
        pre = er.exact_max(Ms[:1], bx["lo"], bx["hi"], np.eye(Ms[0].shape[0])[2])
        assert abs(pre.v - bx["pre"]["vmax"][2]) <= 1e-12, bname


# ----------------------------------------------------------------------------- the product without a GPU
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_the_host_routine_is_sound_at_the_witnesses(name):
    """makeIntervalsBatch(backend="host"), float32 by design: the six arrays and the literal bounds against the attained extrema of every
    fixture box, slack HOST_SLACK (1 + |w|) as tests/test_literal_bounds_cpu.py; tight on the point box and the all-stable box"""
    cs = ec.case(name)
    lo, hi = ec.box_arrays(cs)
    tol = ec.host_tols(cs)
    ec.check_sound(f"{name} host", cs, ec.entry_arrays(na.makeIntervalsBatch(cs["net"], lo, hi, backend="host", normals=cs["C"])), tol)
    ec.check_sound(f"{name} host, no literals", cs, ec.entry_arrays(na.makeIntervalsBatch(cs["net"], lo, hi, backend="host")), tol)
    for T in (3, 8):
        res = na.makeIntervalsBatch(cs["net"], lo, hi, backend="host", normals=cs["C"], alpha_steps=T)
        ec.check_sound(f"{name} host alpha {T}", cs, ec.entry_arrays(res), tol)


def test_the_host_linear_form_is_sound_on_the_whole_box():
    """2-8-8-2, the root and one box of half-width 0.5, the host routine plain and with alpha_steps = 8: max over the box of
    C_i f(x) - A_i' x, by the oracle, minus b0_i is <= HOST_SLACK (1 + |b0_i|).  2 boxes x 2 entries x 11 literals = 44 maxima on two
    enumerations (43 and 11 regions)"""
    cs = ec.case("2-8-8-2")
    Ms = cs["net"].Ms
    for bx in cs["boxes"][:2]:
        s = er.regions(Ms, bx["lo"], bx["hi"])
        for T in (0, 8):
            *_, lits = na.makeIntervalsBatch(cs["net"], bx["lo"][:, None], bx["hi"][:, None], backend="host", normals=cs["C"], alpha_steps=T)
            r = er.exact_max(Ms, bx["lo"], bx["hi"], cs["C"], a=lits.A[:, :, 0], search=s)
            excess = r.w - lits.b0[:, 0]
            print(f"{bx['name']} alpha {T}: worst max(C f - A x) - b0 = {excess.max():+.3e}")
            assert np.all(r.v - lits.b0[:, 0] <= ec.HOST_SLACK * (1 + np.abs(lits.b0[:, 0])))


OPTION_SETS = {"plain": {}, "literal_bounds": dict(literal_bounds=True), "corner_points": dict(corner_points=True),
               "alpha 4": dict(literal_bounds=True, alpha_steps=4)}


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_host_verdicts_are_true(name, opts):
    """h = v + rel (c0 - v), v the exact maximum of y_0 - y_last on the root box: rel > 0 is "holds", rel < 0 is "violated", decided
    within 4 096 boxes.  |rel| >= 1e-4: 1e-4 (c0 - v) (3.2e-5 and 3.7e-5 here) stays more than 50 times above both the float32 error of the
    host bounds (3.14e-7 (1 + |v|), tests/test_crown_batch_gpu.py) and the oracle's L * 1e-7, so the truth of the clause is not in doubt"""
    st = ec.verdict_setting(name)
    assert 1e-4 * (st["c0"] - st["v"]) >= 50 * max(3.14e-7 * (1 + abs(st["v"])), er.lipschitz(st["net"].Ms, st["normal"]) * 1e-7)
    for rel in ec.RELS:
        h, res = ec.run_split(st, rel, crown_backend="host", **OPTION_SETS[opts])
        ec.check_verdict(f"{name} host {opts}", st, rel, h, res)


def test_the_thresholds_of_the_split_instances_are_on_the_true_side():
    """tests/test_split_*: "holds" is asserted for thresholds placed above a sampled maximum.  The exact maximum says that it is the truth:
    h > v for the 3-17-33-4 instance (h = s + 0.05 (c0 - s)) and for W10-D5 on [0.5, 1.5]^2 (h = s + 0.25 (c0 - s))"""
    inst = lc.instance("holds")
    v = float(ec.case("holds")["boxes"][0]["lit"]["vmax"][0])
    print(f"holds: sampled max {inst['s']:.6f}, exact max {v:.6f}, h {inst['h']:.6f}, c0 {inst['c0']:.6f}")
    assert inst["s"] <= v < inst["h"]
    if "W10-D5" in ec.fixture()["cases"]:
        import test_split_cpu as sc
        s, c0 = sc.setting()
        v = float(ec.case("W10-D5")["boxes"][0]["lit"]["vmax"][0])
        print(f"W10-D5: sampled max {s:.6f}, exact max {v:.6f}, h {s + 0.25 * (c0 - s):.6f}, c0 {c0:.6f}")
        assert s <= v < s + 0.25 * (c0 - s)
    else:
        assert "W10-D5" in ec.fixture()["header"]["left_out"]
    if "violated" in ec.fixture()["cases"]:
        inst = lc.instance("violated")
        v = float(ec.case("violated")["boxes"][0]["lit"]["vmax"][0])
        assert inst["s"] <= v and inst["h"] < v


# ----------------------------------------------------------------------------- the S-procedure identity behind the SDP test
@pytest.mark.parametrize("name", list(ec.SMALL))
def test_the_s_procedure_identity_with_the_oracle_assembly(name):
    """z = (x, hidden activations, 1) of a point of the box, Z(gamma) from oracle/qc.py with gamma_in, gamma_ac >= 0:
    z' Z z = 2 (c' f(x) - gamma_out) + (terms that are >= 0 at a point of the box), so  c' f(x) - gamma_out <= lambda_max(Z) |z|^2 / 2.
    Checked at the exact argmax and at random points, with the multipliers drawn at random; this is what
    tests/test_exact_soundness_gpu.py asserts of the certified bound"""
    from oracle import nnet_io, qc
    cs = ec.case(name)
    root = cs["boxes"][0]
    nrm = cs["C"][0]
    onet = nnet_io.FeedFwdNet(xdims=cs["net"].xdims, Ms=cs["net"].Ms)
    q = qc.make_reach_hplane_query(onet, root["lo"], root["hi"], 0, nrm)
    nin = q.gamma_dims()[0]
    rng = np.random.default_rng(3)
    pts = [root["lit"]["xmax"][0]] + list(root["lo"] + rng.random((20, len(root["lo"]))) * (root["hi"] - root["lo"]))
    for x in pts:
        gamma = rng.random(q.ngamma)
        gamma[nin] = rng.normal()
        Z = qc.assemble_Z_literal(q, gamma)
        z = er.lifted(cs["net"].Ms, x)
        assert z.shape == (Z.shape[0],) and z[-1] == 1.0
        val = float(nrm @ np.asarray(er.forward_ld(cs["net"].Ms, x), dtype=np.float64))
        quad = float(z @ Z @ z)
        assert quad >= 2.0 * (val - gamma[nin]) - 1e-12 * (1 + abs(quad))
        assert val - gamma[nin] <= 0.5 * max(0.0, np.linalg.eigvalsh(Z)[-1]) * float(z @ z) + 1e-12 * (1 + abs(val))
    # exactness of the form: without activation and input multipliers z' Z z is 2 (c' f(x) - gamma_out)
    gamma = np.zeros(q.ngamma)
    gamma[nin] = 0.3
    z = er.lifted(cs["net"].Ms, pts[0])
    assert abs(float(z @ qc.assemble_Z_literal(q, gamma) @ z) - 2.0 * (root["lit"]["wmax"][0] - 0.3)) <= 1e-12
