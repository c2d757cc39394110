"""The exact ranges of tests/golden/exact_ranges.json on networks of width 17 to 128: tests/embed_common.py embeds the fixture's two
small nets in wide ones without changing their function, so the stored extrema, witnesses and thresholds hold for them.  Here, without
a GPU: the embedding itself, the yardstick of the GPU tests (a condition on the inputs, decided before any kernel runs), the numpy
recurrences on both nets, the float32 host routine and the host driver.  tests/test_exact_embedded_gpu.py holds the kernels."""
import numpy as np
import pytest

import embed_common as em_
import exact_common as ec
import literal_common as lc
import nnsdp_amd as na
import reach_common as rc

ALL = em_.combos(em_.WIDE) + em_.combos(em_.NARROW)
IDS = [em_.label(*c) for c in ALL]
TEN = lc.NAMES + lc.LIT_NAMES
YARDSTICK_CAP = 1e-12


def hidden(net, X):
    """float64 forward pass -> (pre-activations, post-activations, both acdim x npts, and the output)"""
    pre, post = [], []
    for Mk in net.Ms[:-1]:
        pre.append(Mk[:, :-1] @ X + Mk[:, -1:])
        X = np.maximum(pre[-1], 0.0)
        post.append(X)
    return np.concatenate(pre), np.concatenate(post), net.Ms[-1][:, :-1] @ X + net.Ms[-1][:, -1:]


def test_the_layouts_reach_the_slabs_the_second_tile_and_the_k_tail():
    """the placement the GPU tests rely on, stated on `live`.  A hidden layer is read as rows by the passes that bound it (rows 64 and
    above: the second slab) and, unless it is the last one, as columns by the products of every pass above it (columns 64 and above:
    tile w + 4); the last hidden layer is the k dimension of the product below the head.  Every wide layout has a live neuron at 64 or
    above in a layer read as rows and in one read as columns, live neurons on both sides of 15 | 16 and 63 | 64 and at the last
    position of every layer that has those positions; "cancel" and "split" leave no 16-wide tile of any hidden layer without a non-zero
    incoming row and a non-zero outgoing column"""
    for name, widths, kind in ALL:
        e = em_.case(name, widths, kind)
        live, net = e["live"], e["net"]
        for k, D in enumerate(widths):
            assert len(set(live[k].tolist())) == len(live[k]) == e["small"]["net"].xdims[k + 1] and live[k].min() >= 0 and live[k].max() < D
            assert {p for p in (0, 15, 16, 63, 64, D - 1) if p < D} <= set(live[k].tolist()), (name, widths, kind, k)
            if kind != "scatter":
                W, Wn = net.Ms[k][:, :-1], net.Ms[k + 1][:, :-1]
                for t in range(0, D, 16):
                    assert np.any(W[t:t + 16] != 0.0) and np.any(Wn[:, t:t + 16] != 0.0), (name, widths, kind, k, t)
        if (name, widths, kind) in em_.combos(em_.WIDE):
            assert max(widths) > 64
            assert any(live[k].max() >= 64 for k in range(len(widths))), "no live row in a second slab"
            assert any(live[k].max() >= 64 for k in range(len(widths) - 1)), "no live column in a tile w + 4"
            if max(widths) >= 127:
                k = int(np.argmax(widths))
                assert {79, 80} <= set(live[k].tolist()) or {111, 112} <= set(live[k].tolist())
            # on the point box every kind is tight: a live column >= 64 whose neuron is on there makes that check depend on tile w + 4
            post, off = e["small"]["boxes"][ec.BOX_NAMES.index("point")]["post"]["vmax"], 0
            for k, D in enumerate(widths[:-1]):
                n = len(live[k])
                if D > 64:
                    assert np.any((live[k] >= 64) & (post[off:off + n] > 0.0)), (name, widths, kind, k, "no active live column in a tile w + 4")
                off += n
        else:
            assert 16 < max(widths) <= 64


def test_split_counts_are_powers_of_two_and_fill_the_layer():
    for name, widths, kind in ALL:
        if kind != "split":
            continue
        e = em_.case(name, widths, kind)
        for k, D in enumerate(widths):
            m = np.array([len(c) for c in e["info"]["copies"][k]])
            assert np.all(m & (m - 1) == 0) and m.sum() + len(e["info"]["zero"][k]) == D and m.sum() + m.min() > D
            flat = [p for c in e["info"]["copies"][k] for p in c] + list(e["info"]["zero"][k])
            assert sorted(flat) == list(range(D))


# ----------------------------------------------------------------------------- a. the function
@pytest.mark.parametrize("name,widths,kind", ALL, ids=IDS)
def test_the_embedding_preserves_the_function(name, widths, kind):
    """5 000 uniform points of the root box: |f_wide - f_small| <= 1e-13, and the same for the live pre- and post-activations"""
    e = em_.case(name, widths, kind)
    root = e["small"]["boxes"][0]
    X = root["lo"][:, None] + np.random.default_rng(17).random((len(root["lo"]), 5000)) * (root["hi"] - root["lo"])[:, None]
    ps, qs, fs = hidden(e["small"]["net"], X)
    pw, qw, fw = hidden(e["net"], X)
    errs = [float(np.abs(a - b).max()) for a, b in ((fw, fs), (pw[e["rows"]], ps), (qw[e["rows"]], qs))]
    print(f"{e['label']}: |f_wide - f_small| {errs[0]:.2e}, pre {errs[1]:.2e}, post {errs[2]:.2e}")
    assert max(errs) <= 1e-13
    for k, z in enumerate(e["info"]["zero"]):
        assert not e["net"].Ms[k][z].any() and not e["net"].Ms[k + 1][:, z].any()


@pytest.mark.parametrize("kind", em_.KINDS)
def test_a_tanh_net_keeps_its_activation_and_its_function(kind):
    e = em_.case("2-8-8-2", (127, 65), kind, tanh=True)
    assert na.methods._activ_code(e["net"].activ) == na.methods.ACTIV_TANH
    X = np.random.default_rng(18).uniform(-1.0, 1.0, size=(2, 5000))
    assert np.abs(lc.forward(e["net"], X) - lc.forward(e["small_net"], X)).max() <= 1e-13


# ----------------------------------------------------------------------------- b. the yardstick
@pytest.mark.parametrize("name,widths,kind", ALL, ids=IDS)
def test_the_yardstick_is_usable(name, widths, kind):
    """per array and per box |R(float64) - R(long double)| <= 1e-12 on the 8 fixture boxes, every row of the embedded net: the
    tolerances of the GPU tests are 8 times this.  A seed that fails is replaced in embed_common.SEEDS"""
    e = em_.case(name, widths, kind)
    em_.tols(e)
    worst = 0.0
    for nm, a, b in zip(TEN, e["r64"], e["rld"]):
        d = np.abs(a - b).reshape(-1, a.shape[-1]).max(axis=0).astype(np.float64)
        worst = max(worst, float(d.max()))
        assert np.all(d <= YARDSTICK_CAP), (e["label"], nm, ec.BOX_NAMES[int(np.argmax(d))], float(d.max()))
    print(f"{e['label']}: worst |R(float64) - R(long double)| {worst:.2e}")


# ----------------------------------------------------------------------------- c. R on both nets
@pytest.mark.parametrize("name,widths,kind", [c for c in ALL if c[2] != "cancel"], ids=[i for i, c in zip(IDS, ALL) if c[2] != "cancel"])
def test_the_recurrences_agree_on_both_nets(name, widths, kind):
    """"scatter" and "split": in exact arithmetic every bound of a live neuron, of the outputs and of the literals is the small net's;
    R(float64) of the two agree within the sum of their ec.fp64_tols, all ten arrays"""
    e = em_.case(name, widths, kind)
    tw, ts = em_.tols(e), em_.small_tols(name)
    rs = lc.R(e["small"]["net"].Ms, e["lo"], e["hi"], np.float64, head=e["C"])
    for nm, a, b in zip(TEN, e["r64"], rs):
        a = a[e["rows"]] if nm.startswith("ac") else a
        err = float(np.abs(a - b).max())
        print(f"{e['label']} {nm}: |R_wide - R_small| {err:.2e}, tol {tw[nm] + ts[nm]:.2e}")
        assert a.shape == b.shape and err <= tw[nm] + ts[nm], (e["label"], nm, err)


# ----------------------------------------------------------------------------- d. the host routine
@pytest.mark.parametrize("name,widths,kind", ALL, ids=IDS)
def test_the_host_routine_is_sound_on_the_embedded_nets(name, widths, kind):
    e = em_.case(name, widths, kind)
    res = na.makeIntervalsBatch(e["net"], e["lo"], e["hi"], backend="host", normals=e["C"])
    tight = em_.tight_boxes(e, kind)
    worst, nm, box = ec.check_sound(f"{e['label']} host", e["small"], em_.cut(e, ec.entry_arrays(res)), ec.host_tols(e["small"]), tight=tight)
    print(f"{e['label']} host: tight on {tight}; worst (w - bound) / tol = {worst:+.3e} ({nm}, box {box})")


# ----------------------------------------------------------------------------- e. the host driver
@pytest.mark.parametrize("opts", [{}, dict(literal_bounds=True)], ids=["plain", "literal_bounds"])
@pytest.mark.parametrize("name,widths,kind", ALL, ids=IDS)
def test_host_verdicts_are_true_on_the_embedded_nets(name, widths, kind, opts):
    """h = v + rel (c0 - v) with v the fixture's exact maximum and c0 the embedded net's root bound: the true verdict within 4 096
    boxes at the four ec.RELS"""
    st = em_.verdict_setting(em_.case(name, widths, kind))
    for rel in ec.RELS:
        h, res = ec.run_split(st, rel, crown_backend="host", **opts)
        ec.check_verdict(f"{em_.label(name, widths, kind)} host {opts}", st, rel, h, res)
        assert res.visited <= ec.MAX_BOXES_CAP


REACH = [c + (cp,) for c in ALL for cp in (True, False) if cp or c[2] != "cancel"]


@pytest.mark.parametrize("name,widths,kind,corner_points", REACH, ids=[em_.label(*c[:3]) + (" corner_points" if c[3] else " centres") for c in REACH])
def test_host_reach_encloses_the_exact_maxima_on_the_embedded_nets(name, widths, kind, corner_points):
    """reachSplit at rc.TOL on the root box, every stored row: the enclosure of test_reach_split_cpu.py against the fixture's w, v.
    "cancel" with corner points only: without them its tree comes too close to the cap of 4 096 boxes"""
    e = em_.case(name, widths, kind)
    fb = rc.fixture_box(name, "root")
    opt = dict(crown_backend="host", sdp_per_level=0, corner_points=corner_points, max_boxes=ec.MAX_BOXES_CAP, max_depth=64)
    res = na.reachSplit(e["net"], fb["lo"], fb["hi"], fb["C"], rc.TOL, split=na.SplitOptions(**opt))
    rc.check_enclosure(f"{e['label']} host reach", res, fb["w"], fb["v"], ec.HOST_SLACK * (1.0 + np.abs(fb["w"])), rc.TOL, fb["lo"], fb["hi"])
    assert res.status == "converged" and res.visited < ec.MAX_BOXES_CAP
