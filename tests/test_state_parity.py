"""State-for-state parity of the solve loop with the CPU oracle at full size (run with -m gpu on an MI355X).

The oracle (oracle/admm.py, driven through tests/oracle_state.py) runs the library's iteration: same scaling, same start, sigma = 0.1,
alpha = 1.6.  The fixed-sigma map is averaged, hence nonexpansive, and a projection error d reaches the next nu with a norm below
5 |d|; projections within c * tol * |A|_F of the exact one (c = 1: Jacobi sweeps stopped at off(A) <= tol |A|_F; c = 30: the
refinement stage, include/nnsdp.h proj_refine) therefore keep the two trajectories within

    |nu_gpu - nu_oracle|_2  <=  5 N c tol B,      B = max_k |nu_k|_2 on the oracle side,

after N iterations from the same start.  Every tolerance below is at or under that bound; each leg prints its measured deviation
next to its tolerance and bound.  Everything goes through the public API (Solver, SolverBatch, runQuery)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import nnsdp_amd as na
import oracle_state as ost
from oracle import admm as oadmm, operator as oop

pytestmark = pytest.mark.gpu

N = 300                  # plain iterations of legs A, F, G
TOL = 1e-12              # projection tolerance of the exact legs
NC = 1200                # leg C: iterations with the refinement stage
TOL_C = 1e-6             # leg C: projection tolerance
KEEP = {N - 1, N, N + 1, NC}


def _traj(key):
    T = ost.trajectory(key)
    T.keep |= KEEP
    return T


def _exact_opts(mode, **kw):
    """leg A's options: exact sweeps (proj_refine = 0, so that c = 1), fixed penalty, raw iterate"""
    o = dict(decomp_mode=ost.decomp(mode), max_iters=10 ** 8, proj_tol=TOL, adapt_every=0, polish=False, proj_refine=0)
    o.update(kw)
    return na.AdmmSdpOptions(**o)


def _report(leg, key, dev, tol, bound=None):
    b = f"  rigorous bound {bound:.3e}" if bound is not None else ""
    print(f"\n[state parity] {leg} {key}: deviation {dev:.3e}  tolerance {tol:.3e}{b}")


def _state_tolerance(T, n):
    """1e-9 max(1, max|nu|), never above the rigorous bound (c = 1)"""
    bound = ost.rigorous_bound(n, TOL, T.bound_norm(n))
    return min(1e-9 * max(1.0, np.abs(T.nu(n)).max()), bound), bound


def _compare_state(leg, key, T, n, got):
    want = T.multipliers(n)
    tol, bound = _state_tolerance(T, n)
    dropped = np.setdiff1d(np.arange(len(want)), T.P.keep)
    assert np.all(got[dropped] == 0.0), (leg, key, "dropped multipliers must be exactly 0")
    dev = np.abs(got - want).max()
    _report(leg, key, dev, tol, bound)
    i = int(np.argmax(np.abs(got - want)))
    assert dev <= tol, (leg, key, n, dev, tol, "worst entry", i, got[i], want[i])
    return tol


# ----------------------------------------------------------------------------- A + B: exact state tracking, then one check iteration
STATE_CASES = [
    ("W40-D20-b0-single", 1), ("W40-D20-b0-single", 2),          # blocks up to 85: ping-pong sweeps, second workgroup (split)
    ("W40-D20-b2-double", 1), ("W40-D20-b2-double", 2),          # up to 68: ping-pong
    ("W40-D40-b0-double", 2),                                    # 40 distinct blocks (76 index sets) up to 59
    ("W20-D10-b0-path", 1),                                      # round robin; 46 columns of A above 64 nonzeros
    ("W20-D20-b5-double-hplane", 0), ("W10-D10-b7-single-hplane", 0),     # beta >= 5 inside the loop
    ("acas50-path", 0),                                          # 101: systolic sweeps
    ("acas50-single", 0),                                        # 151: packed sweeps
]


@pytest.mark.parametrize("key,minv", STATE_CASES)
def test_state_tracks_oracle(key, minv):
    T = _traj(key)
    s = na.Solver(ost.case_query(key), _exact_opts(ost.CASES[key][1], minv_mode=minv))
    try:
        assert (s.info(4), s.info(5)) == T.blocks()
        s.iterate(N)
        assert s.info(0) > 0 and s.info(3) == N                  # graph replay ran
        # A: the multiplier block of nu_N
        tol = _compare_state("A", f"{key} minv={minv}", T, N, s.raw_multipliers())
        step = np.abs(T.multipliers(N) - T.multipliers(N - 1)).max()
        assert step >= 100 * tol, (key, step, tol)               # a stalled or one-step-off state fails
        # B: one check iteration from nu_N - the residual kernels (k_check_dual incl. its long rows, k_check_obj, k_acc_reduce)
        got = s.residuals()
        want = T.check(N)
        # residuals relative to themselves, the two objectives relative to the larger of them (a hyperplane query's primal
        # objective is exactly 0 while y_gout is)
        oscale = max(abs(want[2]), abs(want[3]))
        rel = [abs(got[i] - want[i]) / max(abs(want[i]) if i < 2 else oscale, 1e-300) for i in range(4)]
        _report("B", f"{key} minv={minv} (pres, dres, pobj, dobj) relative", max(rel), 1e-8)
        assert max(rel) <= 1e-8, (key, got, want)
        _compare_state("B", f"{key} minv={minv} after the check", T, N + 1, s.raw_multipliers())
    finally:
        s.close()


# ----------------------------------------------------------------------------- C: refinement stage and split in the loop
@pytest.mark.parametrize("key", ["acas50-path"])
def test_refinement_stage_tracks_oracle(key):
    """the warm refinement stage (packed warm sweeps of the 101-blocks, the tile-parallel pipeline) inside NC iterations: within the
    stage's promise of 30 tol |A|_F per projection.  (W40-D20 Single at tol <= 1e-6: the stage carries under 1 % of the block visits
    in the first 2 000 iterations, so it is not a test of the stage there; its two-workgroup hand-over is in legs A, B, F and G.)"""
    T = _traj(key)
    s = na.Solver(ost.case_query(key), na.AdmmSdpOptions(decomp_mode=ost.decomp(ost.CASES[key][1]), max_iters=10 ** 8, proj_tol=TOL_C,
                                                         adapt_every=0, polish=False, proj_refine=1))
    try:
        s.advance(NC)                     # checks included: the pipeline switches itself on at check iterations
        assert s.info(3) == NC
        got, want = s.raw_multipliers(), T.multipliers(NC)
        dev = np.linalg.norm(got - want)
        bound = ost.rigorous_bound(NC, TOL_C, T.bound_norm(NC), c=30.0)
        rb = s.finish().summary["refine_blocks"]
    finally:
        s.close()
    share = rb[1] / max(sum(rb), 1)
    _report("C", f"{key} |d|_2 (stage carried {100 * share:.1f} % of {sum(rb)} block visits {rb})", dev, bound, bound)
    assert share >= 0.2, rb
    assert dev <= bound, (key, dev, bound)


# ----------------------------------------------------------------------------- D: full loop with penalty adaptation
@pytest.mark.parametrize("key", ["W40-D20-b0-single", "W40-D20-b2-double"])
def test_full_loop_with_sigma_adaptation_tracks_oracle(key):
    iters = 600
    r = oadmm.admm_solve(ost.case_operator(key), oadmm.AdmmOptions(max_iters=iters))
    sigmas = sorted({h[5] for h in r.history})
    assert len(sigmas) >= 3, r.history                            # several penalty changes inside the window
    s = na.runQuery(ost.case_query(key), na.AdmmSdpOptions(decomp_mode=ost.decomp(ost.CASES[key][1]), max_iters=iters, proj_tol=TOL,
                                                          polish=False, eps_rel=1e-14, proj_refine=0))
    assert s.summary["iters"] == r.iters and s.termination_status == r.status
    gam = np.concatenate([s.values[k] for k in ("γin", "γout", "γac1", "γac2")])
    keep = ost.trajectory(key).P.keep
    # the box multipliers of coordinates the normalisation eliminated have no column in the solver; the library raises them to
    # 100^t max(1, max gamma) in the returned certificate (csrc/solver.hpp certificate(), "large enough"), the oracle leaves them 0
    dropped = np.setdiff1d(np.arange(len(gam)), keep)
    assert np.all((gam[dropped] == 0.0) | (gam[dropped] >= 100.0 * max(1.0, gam[keep].max()))), key
    tol = 1e-8 * np.abs(r.gamma).max()
    dev = np.abs(gam[keep] - r.gamma[keep]).max()
    _report("D", f"{key} gamma (sigmas {['%.3g' % v for v in sigmas]})", dev, tol)
    assert dev <= tol, (key, dev, tol)
    odev = abs(s.objective_value - r.objective) / abs(r.objective)
    _report("D", f"{key} objective relative", odev, 1e-8)
    assert odev <= 1e-8, (s.objective_value, r.objective)


# ----------------------------------------------------------------------------- E: the Woodbury core against an independent solve
@pytest.mark.parametrize("key", ["W40-D20-b0-single", "W40-D20-b2-double", "W40-D40-b0-double"])
@pytest.mark.parametrize("minv", [1, 2])
def test_minv_matches_cholesky_of_the_oracle(key, minv):
    T = _traj(key)
    s = na.Solver(ost.case_query(key), _exact_opts(ost.CASES[key][1], minv_mode=minv))
    rng = np.random.default_rng(77)
    dropped = np.setdiff1d(np.arange(T.P.ng_full), T.P.keep)
    try:
        worst = 0.0
        for _ in range(3):
            q = rng.standard_normal(T.P.ng_full)
            out, structured, _ = s.apply_minv(q)
            assert structured == (minv == 2)
            assert np.all(out[dropped] == 0.0)
            want = sla.cho_solve(T.S.Mfac, q[T.P.keep])
            worst = max(worst, np.abs(out[T.P.keep] - want).max() / np.abs(want).max())
    finally:
        s.close()
    _report("E", f"{key} minv_mode={minv} relative", worst, 1e-10)
    assert worst <= 1e-10


def test_structured_minv_residual_w20_d100_beta7():
    """W20-D100 beta = 7 (the reference's headline row): M has far too many entries to form; the residual of M x = q through the
    oracle's sparse A instead (the finite check in test_structured_minv_matches_the_dense_inverse stays)"""
    from nnsdp_amd import frontend as F
    qq, _, _ = F.ellipsoidQuery(ost.golden_net("W20-D100"), [0.5, 0.5], [1.5, 1.5], 7)
    P = oadmm.ScaledProblem(oop.build_operator(ost.mirror_query(qq), "double", normalize=True))
    Dinv = sp.diags(1.0 / P.pat.count)
    s = na.Solver(qq, na.AdmmSdpOptions(decomp_mode=na.DoubleDecomp()))
    try:
        q = np.random.default_rng(78).standard_normal(P.ng_full)
        out, structured, _ = s.apply_minv(q)
    finally:
        s.close()
    assert structured
    dropped = np.setdiff1d(np.arange(P.ng_full), P.keep)
    assert np.all(out[dropped] == 0.0)
    x, qk = out[P.keep], q[P.keep]
    rel = np.linalg.norm(x + P.A.T @ (Dinv @ (P.A @ x)) - qk) / np.linalg.norm(qk)
    _report("E", f"W20-D100 beta=7 structured ({len(P.keep)} kept) relative residual", rel, 1e-10)
    assert rel <= 1e-10


# ----------------------------------------------------------------------------- F: batch handle
def test_batch_members_track_their_oracles():
    keys = ["W40-D20-b0-single", "W40-D20-b2-double", "W20-D10-b0-path", "W10-D5-b3-single"]
    sb = na.SolverBatch([ost.case_query(k) for k in keys], [_exact_opts(ost.CASES[k][1]) for k in keys])
    try:
        sb.iterate(N)
        for k, s in zip(keys, sb.solvers):
            assert s.info(3) == N
            _compare_state("F", f"batch member {k}", _traj(k), N, s.raw_multipliers())
    finally:
        sb.close()


# ----------------------------------------------------------------------------- G: graph replay vs eager launches
def test_graph_replay_matches_eager_launches(tmp_path):
    """NNSDP_NO_GRAPH is read once per process (a function-local static): the eager run goes into a fresh child process"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import state_worker
    replay = state_worker.run(N)
    assert replay["graph_launches"] > 0
    out = tmp_path / "eager.json"
    env = dict(os.environ, NNSDP_NO_GRAPH="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "state_worker.py"), str(N), str(out)],
                       env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    eager = json.loads(out.read_text())
    assert eager["graph_launches"] == 0
    print(f"\n[state parity] G graph replay vs eager: multiplier digests {replay['mult_digest'][:16]} / {eager['mult_digest'][:16]}")
    for k in ("mult_digest", "residuals", "mult_after_check_digest"):
        assert eager[k] == replay[k], k
