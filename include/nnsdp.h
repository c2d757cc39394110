/*
 * nnsdp.h -- C ABI of the MI355X-native Chordal-DeepSDP assembler + ADMM solver.
 *
 * This is the drop-in boundary for the hot path of AntonXue/nn-sdp.  The reference has no FFI
 * on this path; the seam is Julia multiple dispatch on the options type,
 *     Methods.runQuery(query::Query, opts::QueryOptions)      src/Methods/Methods.jl:91-131
 * which today builds a JuMP model (setupSafety!/setupReach!, src/Methods/deep_sdp.jl:10-61,
 * src/Methods/chordal_sdp.jl:96-153) and hands it to MOSEK (Methods.jl:61,64,83).  A Julia
 * method runQuery(query, opts::AdmmSdpOptions) ccall's nnsdp_solve() below instead
 * (INTEGRATION.md shows the stub); the Python mirror in nn-sdp_amd/nnsdp_amd binds the same
 * symbols through ctypes.
 *
 * Conventions: plain pointers and sizes only, caller owns every buffer, the library copies in,
 * writes results into caller memory and retains nothing after a call returns (handles excepted,
 * until destroyed).  All matrices are COLUMN-MAJOR Float64 (Julia layout).  Every function
 * returns 0 on success, <0 for an invalid argument, >0 for a runtime (HIP/rocSOLVER/RCCL)
 * failure; nnsdp_last_error() returns a thread-local message.  Nothing throws across the ABI.
 * Blocking calls; distinct handles may be used from distinct threads, one handle from one
 * thread at a time.
 *
 * WHAT "SAME RESULT AS THE REFERENCE" MEANS HERE (the parity contract; DESIGN.md section 7, tests/test_published_sweep.py on all 136
 * published (network, beta) pairs of dump/scale, tests/test_published_parity.py on 21 of them two-sided).  The returned (gamma, Z) is
 *   - FEASIBLE for the reference's own LMI with the caller's own interval bounds: gamma >= 0 exactly, eigmax(Z(gamma)) <= 1e-6 in the
 *     reference's coordinates (its own OPTIMAL rows: +1e-7 .. +5e-6), so `objective` is a valid bound whatever else holds;
 *   - NEVER LOOSER than what the reference published, up to the stopping rule: objective <= (1 + 2e-3) x the median of the three
 *     published values (DeepSDP, Chordal, Chordal-2) with cert_tol = 1e-3, <= (1 + 1e-3) x with eps_rel = 1e-6;
 *   - and NOT two-sided equal to them: the published objectives are MOSEK iterates accepted before optimality, one-signed, up to
 *     2.2 % ABOVE the optimum of their own LMI (an independent interior point encloses that optimum on the pinned rows and this library
 *     lands inside the enclosure: tests/test_oracle_ipm.py).  7 of 21 rows agree to 1e-3 two-sided, the others are strict xfails with
 *     their measured distance.  A caller that needs the reference's number reproduced to 1e-3 gets a tighter one instead.
 * Bit-exact parity holds where the path is integer / index work (cliques, selectors, gather lists) and 1e-12 relative for the
 * assembled LMI against the literal restatement of src/Qc (tests/test_gpu_parity.py).
 */
#ifndef NNSDP_H
#define NNSDP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNSDP_VERSION 230 /* 0.2.3 */

/* query_kind: Methods.SafetyQuery / Methods.ReachQuery (src/Methods/Methods.jl:22-43) */
enum { NNSDP_QUERY_SAFETY = 0, NNSDP_QUERY_REACH = 1 };
/* out_kind: Qc.QcSafety / QcReachHplane / QcReachCircle / QcReachEllipsoid (src/Qc/output.jl:3-31) */
enum { NNSDP_OUT_SAFETY_S = 0, NNSDP_OUT_HPLANE = 1, NNSDP_OUT_CIRCLE = 2, NNSDP_OUT_ELLIPSOID = 3 };
/* decomp_mode: DeepSdpOptions (one dense cone, src/Methods/deep_sdp.jl:2-7) or
 * ChordalSdpOptions.decomp_mode = SingleDecomp / DoubleDecomp (src/Methods/chordal_sdp.jl:4-16) */
enum { NNSDP_DECOMP_DENSE = 0, NNSDP_DECOMP_SINGLE = 1, NNSDP_DECOMP_DOUBLE = 2,
       NNSDP_DECOMP_PATH = 3 /* extension: cliques {x_k, x_k+1, affine}, exact when the output QC has S12 = 0 */,
       NNSDP_DECOMP_AUTO = 4 /* PATH when the query allows it (every reach query, hyperplane safety sets), DOUBLE otherwise: the
                                fastest exact decomposition (width-50 networks: 3.6 s instead of 13 s for the reference's cliques) */ };
/* ffnet.activ: ReluActiv / TanhActiv (src/MyNeuralNetwork/MyNeuralNetwork.jl:7-9) */
enum { NNSDP_ACTIV_RELU = 0, NNSDP_ACTIV_TANH = 1 };
/* termination status; strings as consumed by experiments/acas.jl:77 via nnsdp_status_string() */
enum { NNSDP_STATUS_OPTIMAL = 0, NNSDP_STATUS_ITERATION_LIMIT = 1, NNSDP_STATUS_TIME_LIMIT = 2,
       NNSDP_STATUS_SLOW_PROGRESS = 3, NNSDP_STATUS_NUMERICAL_ERROR = 4,
       NNSDP_STATUS_TARGET_CERTIFIED = 5   /* nnsdp_solver_set_target: a rigorous bound met the target (the certificate is the result) */,
       NNSDP_STATUS_TARGET_UNREACHABLE = 6 /* ... : the estimates of the optimum exclude the target; an "unknown", not a proof */ };
/* target modes of nnsdp_solver_set_target */
enum { NNSDP_TARGET_OFF = 0, NNSDP_TARGET_OBJECTIVE = 1 /* reach: objective <= target */, NNSDP_TARGET_FEASIBLE = 2 /* safety: any certificate */ };

/*
 * The numeric content of a Methods.Query: FeedFwdNet (src/MyNeuralNetwork/MyNeuralNetwork.jl:12-27),
 * QcInputBox (src/Qc/input.jl:3-8), QcActivBounded (src/Qc/activ_bounded.jl:3-10),
 * QcActivSector for ReLU (src/Qc/activ_sector.jl:2-20) and one QcOutput (src/Qc/output.jl:3-31).
 */
typedef struct nnsdp_problem {
  int32_t K;              /* number of affine layers = length(ffnet.Ms) */
  const int32_t* xdims;   /* K+1 layer sizes */
  const double* M;        /* Ms[1..K] back to back, each xdims[k+1] x (xdims[k]+1) column-major = [W_k b_k] */
  const double* x1min;    /* xdims[0] */
  const double* x1max;    /* xdims[0] */
  const double* acymin;   /* acdim = sum(xdims[1..K-1]) : QcActivBounded.acymin */
  const double* acymax;   /* acdim */
  const double* smin;     /* acdim : QcActivSector.smin (base_smin = 0) */
  const double* smax;     /* acdim : QcActivSector.smax (base_smax = 1) */
  int32_t beta;           /* QcActivSector.beta */
  int32_t query_kind;     /* NNSDP_QUERY_* */
  int32_t out_kind;       /* NNSDP_OUT_* */
  const double* normal;   /* HPLANE: xdims[K] */
  const double* yc;       /* CIRCLE / ELLIPSOID: xdims[K] */
  const double* invP;     /* ELLIPSOID: xdims[K] x xdims[K] column-major */
  const double* S;        /* SAFETY_S: (xdims[0]+xdims[K]+1)^2 column-major */
  int32_t activ;          /* NNSDP_ACTIV_*: ffnet.activ.  TANH: QcActivSector.vardim = lambda_dim, no eta / nu multipliers
                             (src/Qc/activ_sector.jl:19,49-57); smin/smax are then real numbers in [0,1] (:74-86) */
} nnsdp_problem;

/* The fields of `AdmmSdpOptions <: QueryOptions` (the replacement of ChordalSdpOptions). */
typedef struct nnsdp_options {
  int32_t decomp_mode;    /* NNSDP_DECOMP_* */
  int32_t max_iters;      /* ADMM iteration cap (MOSEK analogue: MSK_IPAR_INTPNT_MAX_ITERATIONS) */
  double eps_rel;         /* relative tolerance on both splitting residuals (INTPNT_CO_TOL_PFEAS/DFEAS) */
  double max_time;        /* seconds; <= 0: none (MSK_DPAR_OPTIMIZER_MAX_TIME, experiments/scale.jl:32) */
  double sigma;           /* initial ADMM penalty */
  double alpha;           /* over-relaxation in (0,2) */
  int32_t adapt_every;    /* residual-balancing period, iterations; 0 = fixed sigma */
  int32_t check_every;    /* convergence-check period, iterations (= iterations per hipGraph launch) */
  int32_t normalize;      /* 1: solver-internal interval congruence + fixed-neuron elimination (reach queries) (default) */
  int32_t warm_start;     /* 1: warm-start each eigendecomposition from the previous eigenvectors */
  double proj_tol;        /* Jacobi stops at off(A) <= proj_tol |A|_F; 0 = adaptive: 0.01 x the current residual,
                             clamped to [1e-9, 1e-4] (inexact projections well below the residual level) */
  int32_t polish;         /* 1: make the returned (gamma, Z) exactly feasible (diagonal shift + Schur complement for gout) */
  double cert_tol;        /* > 0 (reach queries): also stop once the polished, exactly feasible objective is within
                             cert_tol (relative) of the ADMM primal/dual objective estimates; 0 = residual test only.
                             A TARGET, not a proven bound: the polished objective is a rigorous UPPER bound of the optimum, but what it
                             is compared with are estimates of the optimum, trusted once both residuals are below cert_tol / 10 (no
                             dual-feasible point is constructed: DESIGN.md section 9).  Measured on the traced solves: 4.9e-4 .. 9.4e-4
                             above the converged optimum for cert_tol = 1e-3.  The stopping iteration is reproducible (no atomics). */
  int32_t verbose;        /* QueryOptions.verbose (src/Methods/Methods.jl:110) */
  int32_t device;         /* HIP device ordinal, -1 = current */
  double interval_guard;  /* (normalize = 1) a neuron interval [acymin, acymax] narrower than interval_guard x |midpoint| is
                             widened to that inside the solver (default 5e-5; 0 = take the bounds literally).  The returned
                             gamma stays feasible for the LMI with the caller's bounds.  The reference's float32 CROWN
                             boxes of collapsed deep nets are narrower than their own rounding error and, taken
                             literally, make the QC set empty (rho = 0 would be "optimal"); MOSEK at 1e-6 never
                             resolves that, an exact solver does. */
  int32_t minv_mode;      /* the Woodbury core M^-1, M = I + A'D^-1A over the kept multipliers: 1 = dense inverse (8 ng^2 bytes read
                             per iteration), 2 = structured (block-banded by network layer + low rank: two-level domain
                             decomposition, three launches, O(ng b) bytes), 0 = auto (structured from 3500 kept multipliers on,
                             when the generator table has that structure) */
  int32_t proj_refine;    /* 1 (default): warm PSD blocks of 41 .. 160 first try the GEMM-only refinement of the eigenbasis kept from the
                             previous iteration (one rotation of all pairs to second order on the matrix cores, accepted when its predicted
                             off(A) is below 30 x the projection tolerance) and fall back to the exact Jacobi sweeps - up to 96 with the
                             basis in LDS, 97 .. 160 in the packed-triangle variant with the basis in HBM; 2: blocks up to 96 whose
                             prediction misses by less than 30 x also take the step and are checked (B rebuilt, off(A) measured) before
                             the sweeps - measured: no gain on W40-D20; 0: sweeps only.
                             A launch that holds a block above 96 runs the same stage as FIVE short launches over the whole chip
                             (tile-parallel pipeline, csrc/refine_pipe.hpp: workgroup = (block, tile column, row group)) in front of the
                             one-CU kernel, which then only sees the blocks the pipeline did not carry; it switches itself on once 70 % of
                             a check window's block visits took the step and off below 40 % (width-50 networks: 2.1x per solve); a block
                             whose prediction misses the accepted level by less than 10x takes the step anyway and is analysed afresh by a
                             second pass of the five launches instead of going to the sweeps (another 1.5x on such networks).  Launches
                             of blocks up to 96 keep the one-CU form (the five launches tie with it there: DESIGN.md section 4). */
} nnsdp_options;

/* Contents of Methods.QuerySolution (src/Methods/Methods.jl:46-55) plus solver diagnostics.
 * gamma_* and Z are caller-allocated (any may be NULL to skip).  Sizes:
 *   gamma_in xdims[0]; gamma_out 1 (reach only); gamma_ac1 acdim;
 *   gamma_ac2 lambda_dim + 2*acdim (ReLU) or lambda_dim (Tanh), lambda_dim = (beta+1)*acdim - beta*(beta+1)/2;
 *   Z Zdim x Zdim column-major, Zdim = sum(xdims[0..K-1]) + 1  (values[:Z], Methods.jl:86). */
typedef struct nnsdp_result {
  double* gamma_in;
  double* gamma_out;
  double* gamma_ac1;
  double* gamma_ac2;
  double* Z;
  double objective;       /* objective_value */
  int32_t status;         /* NNSDP_STATUS_* */
  int32_t iters;
  double pres;            /* |K x + q - w| / max(|K x + q|, |w|)      (dual feasibility of (P)) */
  double dres;            /* |K'y - z0| / max(|K'y|, |z0|)           (LMI equality of (P)) */
  double lambda_max;      /* eigmax(Z(gamma)) in the reference's coordinates (Methods.jl:116) */
  double t_setup;         /* seconds: pattern + generators + factorisation (setup_time) */
  double t_solve;         /* seconds: ADMM loop (solve_time) */
  double t_total;         /* seconds (total_time) */
  double t_eig;           /* seconds of t_solve inside the PSD-projection kernel (HIP events) */
  int32_t n_cliques;      /* PSD blocks solved (after normalisation) */
  int32_t max_clique;     /* largest block dimension solved */
  int64_t eig_flops_per_iter; /* 10 * sum n_k^3 over the blocks solved */
  int64_t eig_bytes_per_iter; /* 2 * 8 * sum n_k^2 */
  double avg_sweeps;      /* Jacobi sweeps per block per iteration, averaged over the solve */
  double objective_admm;  /* objective of the raw ADMM iterate (before the polish) */
  double polish_shift;    /* diagonal shift applied by the polish in solver coordinates; -1: polish not applied */
  int64_t refine_blocks[5]; /* projection refinement stage, block visits over the solve: already converged / one GEMM step / sent on to
                             the Jacobi sweeps / attempt skipped (back-off after failures) / accepted after a checked step */
} nnsdp_result;

int nnsdp_version(void);
const char* nnsdp_last_error(void);
const char* nnsdp_status_string(int32_t status);
void nnsdp_default_options(nnsdp_options* opts);

/* Sizes derived from a problem: Zdim, acdim, length of gamma_ac2, total length of gamma. */
int nnsdp_problem_dims(const nnsdp_problem* p, int32_t* Zdim, int32_t* acdim, int32_t* nac2, int32_t* ngamma);

/* Replaces Methods.runQuery's setup + solve (src/Methods/Methods.jl:91-131). */
int nnsdp_solve(const nnsdp_problem* p, const nnsdp_options* o, nnsdp_result* r);

/* Handle form of the same solve, used by bench.py to time exactly K iterations. */
typedef struct nnsdp_solver nnsdp_solver;
int nnsdp_solver_create(const nnsdp_problem* p, const nnsdp_options* o, nnsdp_solver** out);
/* Solver families (no reference analogue): a SIBLING of `parent` solves a problem that differs from the parent's in the output data
 * only - normal / S / yc, invP, and the last affine layer Ms[K] (generators are built from layers 1 .. K-1; the output QC and the
 * last layer enter the constant term z0 and nothing else).  Everything else must be equal, compared exactly: K, xdims, Ms[1 .. K-1],
 * x1min / x1max, acymin / acymax, smin / smax, beta, activ, query_kind, out_kind (circle and ellipsoid count as one kind: the
 * same gout generator; hyperplane and ellipsoid do not); -1 with a message naming the first field that differs.  Options are the parent's (an AUTO decomposition as the parent resolved it; a sibling whose z0 does not fit the parent's
 * pattern - PATH with an S12 coupling - is refused, not re-decomposed).  A clique-sharded parent, or one that has been given a
 * communicator, is refused, and a family member cannot be given one.  The sibling owns its z0, its iteration state, scratch, stream,
 * graphs and statistics and SHARES BY REFERENCE COUNT what the set-up builds: the device operator (CSR / CSC, Dinv, c), the gather
 * tables, the row and column class lists, the block lists, and M^-1 (dense, or the structured factors).  Any member, the parent
 * included, may be destroyed first.  Inside a batch handle the members of a family whose M^-1 is dense are served by ONE pass over
 * the matrix per 16 members (always, also a member alone in its batch: the stage's bits do not depend on who else is there);
 * members of a family whose M^-1 is structured are served by the four stages of the structured form ONCE per 8 members (four
 * launches for all such groups of the batch; a lane loads each piece of the shared factors once and uses it for every member), with
 * every member's result bit-identical to its own single-solver stage - so a member alone in its batch simply keeps the
 * single-solver launches (as does a family of which ONE chunk slice or separator vector exceeds a CU's LDS: a chunk above 8 192
 * multipliers, a separator above 20 480).  NNSDP_FAMILY_STRUCT=0 (diagnostic, read once) keeps
 * them for every member.
 * nnsdp_solver_iterate / _run on a member outside a batch use the single-solver stage like any solver. */
int nnsdp_solver_create_sibling(nnsdp_solver* parent, const nnsdp_problem* p, nnsdp_solver** out);
/* run `iters` ADMM iterations (no convergence test); eig_ms (may be NULL) receives the HIP-event
 * time of the projection kernel summed over these iterations. */
int nnsdp_solver_iterate(nnsdp_solver* s, int32_t iters, double* eig_ms);
/* advance exactly `iters` iterations with the solve loop's convergence checks and sigma / projection-tolerance
 * adaptation, but without stopping (brings a handle to the solver's steady state before timing) */
int nnsdp_solver_advance(nnsdp_solver* s, int32_t iters);
/* enqueue `iters` iterations on the solver's own HIP stream without waiting: several handles (independent
 * SDPs: the beta sweep of experiments/scale.jl:28, the hyperplanes of NnSdp.findReach2Dpoly) then run
 * concurrently on one GPU; nnsdp_solver_sync waits for one handle. */
int nnsdp_solver_iterate_async(nnsdp_solver* s, int32_t iters);
int nnsdp_solver_sync(nnsdp_solver* s);
/* ADVANCES the handle by ONE check iteration (an ordinary ADMM iteration that also accumulates the residual sums) and returns
 * that iteration's relative residuals and primal / dual objective estimates; it does not stop, adapt the penalty or polish.
 * After calling it on members of a batch handle, call nnsdp_batch_resync (the batch advances its members in lockstep). */
int nnsdp_solver_residuals(nnsdp_solver* s, double* pres, double* dres, double* pobj, double* dobj);
/* test / diagnostic entry: out = M^-1 q for a full-length multiplier vector q (entries of dropped multipliers are ignored and
 * returned as 0), through whichever form the handle uses; *structured (may be NULL) tells which, *operand_bytes its size */
int nnsdp_solver_apply_minv(nnsdp_solver* s, const double* q, double* out, int32_t* structured, int64_t* operand_bytes);
/* test / diagnostic entry, the multi-vector form: Q and out hold `nrhs` full-length multiplier vectors back to back (dropped
 * multipliers ignored / returned 0); runs the fused kernel of the solver families on the handle's dense M^-1, 16 vectors per pass
 * (-1 for a handle whose M^-1 is structured).  Vector j of a call equals a one-vector call on the same vector bit for bit.
 * kernel_ms (may be NULL) receives the HIP-event time of the launch. */
int nnsdp_solver_apply_minv_multi(nnsdp_solver* s, int32_t nrhs, const double* Q, double* out, double* kernel_ms);
/* the same for a handle whose M^-1 is structured: runs the fused structured stages of the solver families on the handle's factors, 8
 * vectors per pass, all passes in the same four launches (-1 with a message for a handle whose M^-1 is dense).  Vector j equals nnsdp_solver_apply_minv on the same vector bit for bit, whatever nrhs and j.
 * kernel_ms (may be NULL) receives the HIP-event time of the four launches. */
int nnsdp_solver_apply_minv_structured_multi(nnsdp_solver* s, int32_t nrhs, const double* Q, double* out, double* kernel_ms);
/* test / diagnostic entry: the multiplier block of the solver's fixed-point variable nu (solver coordinates and scaling), one
 * entry per multiplier of the problem (dropped multipliers 0).  In clique-sharded mode this block is replicated; the two-rank
 * test compares it bit for bit between ranks. */
int nnsdp_solver_raw_multipliers(nnsdp_solver* s, double* out);
/* diagnostic: what = 0 hipGraph launches that advanced this solver so far (its own and those of a batch handle it is a member of), 1 whether an ncclAllReduce could be captured into a hipGraph (sharded mode over RCCL),
 * 2 clique-sharded mode on, 3 iterations done, 4 PSD blocks, 5 largest block, 6 the hipIpc transport (0 off, 1 on with ordinary device
 * memory behind the exchange buffers, 2 on with fine-grained device memory - the default), 7 family id (0 for a solver that shares
 * nothing, otherwise equal for all members of a family and distinct between the families of a process), 8 bytes of device memory this
 * handle owns exclusively, 9 bytes it shares with other members of its family (buffers with more than one holder), 10 chunks of the
 * structured M^-1 plan (0: dense), 11 how many of them start at an odd multiplier or an odd separator column (these take the
 * scalar-load paths of the structured stages), 12 sparse-bound evaluations so far (nnsdp_solver_certified_bound and the target rule),
 * 13 whether the pattern has a sparse-bound plan (nnsdp_cert_plan's `supported`; asking builds the plan) */
int nnsdp_solver_info(nnsdp_solver* s, int32_t what, double* out);
/* iterate until converged / limits; fills r like nnsdp_solve */
int nnsdp_solver_run(nnsdp_solver* s, nnsdp_result* r);
int nnsdp_solver_finish(nnsdp_solver* s, nnsdp_result* r);
int nnsdp_solver_destroy(nnsdp_solver* s);

/* Decide a target instead of converging (default off; before or between runs; every family / batch member carries its own).
 * Every ADMM iterate can be made exactly feasible - gamma >= 0, Z(gamma) NSD - by the two exact moves of the certificate polish (a
 * diagonal shift, then gout from the Schur complement of the affine index), and its objective is then a rigorous upper bound of the
 * optimum.  The moves are evaluated WITHOUT dense linear algebra: Z lives on the clique pattern, whose stored order is a perfect
 * elimination order, so 16 shift candidates at a time are factored side by side by a multifrontal Cholesky of -Z with every front in
 * LDS (nnsdp_cert_plan, nnsdp_sparse_nsd), twice per evaluation; as in the dense polish a candidate must have Z_xx <= -1e-9 I in the
 * solver's coordinates.
 *   mode NNSDP_TARGET_OBJECTIVE (reach queries; `target` in the units of nnsdp_result.objective): at every check iteration whose ADMM
 *     primal estimate is <= target the bound is evaluated, and the solve stops with NNSDP_STATUS_TARGET_CERTIFIED as soon as it is
 *     <= target.  It stops with NNSDP_STATUS_TARGET_UNREACHABLE once both residuals are <= 1e-3 and
 *     min(pobj, dobj) - target > 3.8 x max(pres, dres) x max(|pobj|, |dobj|)  (twice the smallest factor that is safe on every traced
 *     check point).  UNREACHABLE rests on estimates: it is an "unknown", never a proof that the target fails, and
 *     the rule can only ever produce such an unknown - a TARGET_CERTIFIED is always backed by the exactly feasible point returned.
 *   mode NNSDP_TARGET_FEASIBLE (safety queries: any certificate): the bound is evaluated at every check iteration and the solve stops
 *     with NNSDP_STATUS_TARGET_CERTIFIED at the first feasible candidate.
 * nnsdp_solver_finish / _finish_status then return exactly that point, checked by the dense eigmax like any other result.  A pattern
 * whose largest front exceeds 128 has no sparse route: the rule then uses the dense polish on the schedule of cert_tol.  -1 for a
 * clique-sharded solver, and for NNSDP_TARGET_OBJECTIVE on a safety query. */
int nnsdp_solver_set_target(nnsdp_solver* s, int32_t mode, double target);
/* The rigorous bound of the CURRENT iterate (any query kind; reach: objective = gout): *certified = 1 and the exactly feasible
 * multipliers in gamma (ngamma doubles, reference coordinates, may be NULL; multipliers of coordinates the normalisation removed are
 * set "large": 1e8 x the largest other one), or *certified = 0 when no candidate passed.  *ms receives the wall-clock time of the call.
 * Deterministic; the iteration state is not touched (the iterates that follow are bit-identical to those of a solver that never
 * asked).  A pattern without a sparse route answers through the dense polish. */
int nnsdp_solver_certified_bound(nnsdp_solver* s, double* objective, double* gamma, int32_t* certified, double* ms);

/* Batch handle (no reference analogue): several independent SDPs - the beta sweep of experiments/scale.jl:28, the
 * hyperplane directions of NnSdp.findReach2Dpoly (src/NnSdp.jl:73-95), the sub-queries of an ACAS clause
 * (experiments/acas.jl:96-114) - advanced in lockstep with ONE kernel launch per stage for all of them.  The solvers
 * stay owned by the caller and must outlive the batch; all on one device, not clique-sharded, same check_every, proj_refine on or
 * off for all of them.
 *   nnsdp_batch_iterate  exactly `iters` plain iterations of every SDP (no checks, fixed penalty), synchronous
 *   nnsdp_batch_run      full solves with the stopping rules of nnsdp_solve, each SDP on its own; status[count]
 *                        receives the NNSDP_STATUS_* of every solver (collect results with nnsdp_solver_finish_status) */
typedef struct nnsdp_batch nnsdp_batch;
int nnsdp_batch_create(nnsdp_solver** solvers, int32_t count, nnsdp_batch** out);
int nnsdp_batch_iterate(nnsdp_batch* b, int32_t iters);
int nnsdp_batch_run(nnsdp_batch* b, int32_t* status);
int nnsdp_batch_destroy(nnsdp_batch* b);
/* re-establish lockstep after members of the batch were advanced individually (nnsdp_solver_residuals / _iterate / _advance):
 * the next batched iteration is a cold one for every member and the launch tables are rebuilt */
int nnsdp_batch_resync(nnsdp_batch* b);
/* diagnostic: what = 0 members still active, 1 fused family groups with a dense M^-1 in the current launch tables, 2 members covered
 * by them, 3 fused family groups with a structured M^-1, 4 members covered by those */
int nnsdp_batch_info(nnsdp_batch* b, int32_t what, double* out);
/* result of a solver that stopped with `status` (as returned by nnsdp_batch_run): certificate polish, gamma, Z */
int nnsdp_solver_finish_status(nnsdp_solver* s, int32_t status, nnsdp_result* r);

/* Replaces Z = Zin + Zout + sum(Zacs) with numeric gamma: Qc.makeZin (src/Qc/input.jl:19-42),
 * makeZout (src/Qc/output.jl:52-106), makeZac (src/Qc/activ.jl:30-42).  gamma = [gin; gout; gac1; gac2]
 * (ngamma doubles); Z is Zdim x Zdim column-major.  Runs on the GPU. */
int nnsdp_assemble_Z(const nnsdp_problem* p, const double* gamma, double* Z);

/* Adjoint of the generator part: out[i] = <G_i, X> for every multiplier i (X symmetric Zdim x Zdim). */
int nnsdp_adjoint(const nnsdp_problem* p, const double* X, double* out);

/* Replaces Methods.makeCliques + the index sets used by setupZs!
 * (src/Methods/chordal_cliques.jl:13-59, src/Methods/chordal_sdp.jl:19-57).  Two-pass:
 * call with ptr == NULL to get n_cliques and total; then with ptr[n_cliques+1], idx[total]
 * (0-based z-indices, CSR). */
int nnsdp_make_cliques(int32_t K, const int32_t* xdims, int32_t beta, int32_t decomp_mode,
                       int32_t* n_cliques, int32_t* total, int32_t* ptr, int32_t* idx);

/* Interval pre-processing on the host: CROWN-sliced bounds of every hidden layer and
 * the sector flags, the direct inputs of the assembler.  Replaces Intervals.intervalsAutoLirpaSliced
 * (src/Intervals/intervals_auto_lirpa.jl:12-64; one PyCall + ONNX round trip per layer through
 * exts/auto_lirpa_bridge.py:97-112) and makeSectorMinMax's interval test (src/Qc/activ_sector.jl:63-72, eps = 1e-4).
 * K, xdims, M as in nnsdp_problem; acdim = xdims[1] + ... + xdims[K-1].  Outputs (caller-allocated, any may be NULL):
 * acymin/acymax[acdim] post-activation bounds, acxmin/acxmax[acdim] pre-activation bounds, smin/smax[acdim] sector
 * flags in {0,1}, ymin/ymax[xdims[K]] bounds of the network output.  No GPU needed. */
int nnsdp_make_intervals(int32_t K, const int32_t* xdims, const double* M, const double* x1min, const double* x1max,
                         double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                         double* ymin, double* ymax);

/* The same for either activation of the reference (ffnet.activ): activ = NNSDP_ACTIV_TANH restates auto_LiRPA's BoundTanh relaxation
 * (exts/auto_LiRPA/operators/activation.py:843-1016, reached through exts/auto_lirpa_bridge.py:31-37,86-87) and fills smin / smax by
 * makeSectorMinMax's tanh branch (src/Qc/activ_sector.jl:74-86: real slopes in [0, 1]).  activ = NNSDP_ACTIV_RELU is nnsdp_make_intervals. */
int nnsdp_make_intervals_activ(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                               double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                               double* ymin, double* ymax);

/* nnsdp_make_intervals_activ plus bounds of nlit literals  normal_i' f(x)  (the split driver's clause, nnsdp_amd/split.py): one more
 * backward pass whose head is [C W_{K-1} | C b_{K-1}], C the nlit x ny matrix of normals, float32 like the rest of the routine; ReLU
 * and Tanh, any width.  normals: ny x nlit column-major (one literal's normal after the other), nlit in 0..64.  Outputs (any may be
 * NULL): lit_smin / lit_smax [nlit] raw bounds of the literals, and the linear upper bound  normal_i' f(x) <= uA[:, i]' x + ub0[i]
 * on the box, uA [xdims[0] x nlit] column-major; lit_smax = uA' c + |uA|' r + ub0 with the box centre c and radius r.  The other
 * outputs have the bits of nnsdp_make_intervals_activ.  -1 with a message for nlit outside 0..64, normals NULL with nlit > 0, or a
 * non-finite normal entry ("literal i").  No GPU needed. */
int nnsdp_make_intervals_lits(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                              double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                              double* ymin, double* ymax, int32_t nlit, const double* normals, double* lit_smin, double* lit_smax,
                              double* uA, double* ub0);

/* nnsdp_make_intervals_lits plus optimised lower slopes of the unstable ReLUs for the literals' UPPER bounds (alpha-CROWN, DESIGN.md
 * section 5).  Plain CROWN gives a neuron with l < 0 < u the lower slope 1 if u / (u - l) > 0.5 else 0; any alpha in [0, 1] is sound.
 * Per literal, `steps` projected-gradient steps  alpha <- clip(alpha - eta0 decay^s g / max|g|, 0, 1)  on the literal's smax, g the
 * analytic gradient (one forward pass through the relaxed network at the maximiser of the linear bound); the result is the first
 * iterate with the smallest smax.  The hidden layers' pre-activation bounds stay plain CROWN; float32 like the rest of the routine.
 * The arguments of nnsdp_make_intervals_lits receive the bits that entry writes.  Then: steps in 0..64, eta0 > 0, decay in (0, 1];
 * alpha0 NULL (start from the plain rule) or [acdim x nlit], neuron index fastest, clipped to [0, 1], entries at neurons that are not
 * unstable ignored.  Outputs (any may be NULL): a_smax [nlit], a_uA [xdims[0] x nlit] column-major, a_ub0 [nlit] as lit_smax / uA /
 * ub0; alpha [acdim x nlit] the slopes of the result (the plain rule at neurons that are not unstable); best_step [nlit] the iterate
 * it came from.  steps = 0 without alpha0 returns the plain pass's bits.  -1 with a message for a Tanh network, nlit = 0, steps, eta0
 * or decay out of range, or a non-finite alpha0 entry.  ReLU only, any width.  No GPU needed. */
int nnsdp_make_intervals_lits_alpha(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min,
                                    const double* x1max, double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin,
                                    double* smax, double* ymin, double* ymax, int32_t nlit, const double* normals, double* lit_smin,
                                    double* lit_smax, double* uA, double* ub0, int32_t steps, double eta0, double decay,
                                    const double* alpha0, double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step);

/* Sampled forward pass on the GPU: Y[:, s] = ffnet(X[:, s]) for N points in fp64.  Replaces the
 * N = 1e5 calls of evalFeedFwdNet (src/MyNeuralNetwork/MyNeuralNetwork.jl:40-48) inside Utils.sampleTrajs (src/Utils/qc.jl:40-47),
 * whose outputs shape the ellipsoid of NnSdp.findEllipsoid (approxEllipsoid, src/Utils/qc.jl:50-67).  K, xdims, M as in
 * nnsdp_problem; activ = NNSDP_ACTIV_*; X is xdims[0] x N, Y is xdims[K] x N, both column-major and caller-owned.
 * kernel_ms (may be NULL) receives the HIP-event time of the launch.  Layer widths up to 639. */
int nnsdp_eval_network(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int64_t N, const double* X, double* Y,
                       double* kernel_ms);

/* CROWN-sliced bounds (the algorithm of nnsdp_make_intervals) for nbox input boxes of ONE network in one launch, fp64: the
 * screening stage of input splitting (nnsdp_amd/split.py), one workgroup per box, the A W_j products of the backward passes on
 * fp64 MFMA (csrc/crown_batch.hpp).  The host routine keeps float32 for parity with the reference; this one has no reference
 * counterpart and keeps every quantity in double, so the two agree to float32 level only.
 * x1min / x1max: xdims[0] x nbox column-major.  Outputs (HOST pointers, any may be NULL), column-major, one column per box:
 * acymin/acymax/acxmin/acxmax [acdim x nbox], ymin/ymax [xdims[K] x nbox].  ReLU only; every width (xdims[0..K]) <= 64.
 * -1 with a message otherwise (Tanh, a wider layer, x1min > x1max, NaN or an infinite bound); nbox = 0 returns 0.  The argument
 * checks need no GPU.
 * kernel_ms (may be NULL): HIP-event time of the launch. */
int nnsdp_make_intervals_batch(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nbox,
                               const double* x1min, const double* x1max,
                               double* acymin, double* acymax, double* acxmin, double* acxmax,
                               double* ymin, double* ymax, double* kernel_ms);

/* nnsdp_make_intervals_batch plus bounds of nlit literals  normal_i' f(x)  per box, from one more backward pass of the same kernel
 * whose head is H = [C W_{K-1} | C b_{K-1}] (C the nlit x ny matrix of normals; H is computed once on the host in fp64, plain sums
 * over ascending index).  normals: ny x nlit column-major, nlit in 0..64 (0: exactly nnsdp_make_intervals_batch).  Outputs (HOST
 * pointers, any may be NULL): smin / smax [nlit x nbox] raw (no min / max post-fix), uA [xdims[0] x nlit x nbox] (coefficient index
 * fastest, then the literal, then the box) and ub0 [nlit x nbox]:  normal_i' f(x) <= uA' x + ub0  on the box, and
 * smax = uA' c + |uA|' r + ub0 with the box centre c and radius r.  A literal's bits depend neither on nbox, nor on the box's
 * position, nor on the other literals of the call; the six interval arrays have the bits of nnsdp_make_intervals_batch.
 * -1 with a message as nnsdp_make_intervals_batch, and for nlit outside 0..64, normals NULL with nlit > 0, or a non-finite normal
 * entry ("literal i"); these checks need no GPU. */
int nnsdp_make_intervals_batch_lits(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nbox,
                                    const double* x1min, const double* x1max,
                                    double* acymin, double* acymax, double* acxmin, double* acxmax,
                                    double* ymin, double* ymax, int32_t nlit, const double* normals,
                                    double* smin, double* smax, double* uA, double* ub0, double* kernel_ms);

/* Resident CROWN bounder: nnsdp_make_intervals_batch_lits and nnsdp_eval_network for MANY calls on ONE network, as the split driver
 * (nnsdp_amd/split.py) makes them level after level.  The handle keeps on the device: xdims, the offsets, the network and the literal
 * head (uploaded once, at creation), and the box, scratch, output and sample buffers, which grow geometrically when a call exceeds
 * their capacity and never shrink; it owns pinned host staging, one stream and two events.  A bound call is one asynchronous upload
 * of the boxes, one launch, one asynchronous download and one stream synchronisation.
 * ReLU and Tanh networks (the one-shot batched entries stay ReLU-only), every width (xdims[0..K]) <= 64, nlit in 0..64.
 * Wide handles (nnsdp_crown_create_wide with max_width 128): hidden layers (xdims[1..K-1]) up to 128 wide, on a second instance of the
 * kernel (csrc/crown_wide.hpp) that walks a pass in slabs of 64 rows x 128 columns; xdims[0], xdims[K] and nlit stay at 64 or below.
 * It needs 137 KB of LDS - one workgroup per CU where the narrow instance has two - so it is asked for, never chosen.  bound, eval,
 * search, search_leaves, reach, reach_leaves, info and destroy work on a wide handle as on a narrow one; nnsdp_crown_bound_alpha does
 * not (the alpha kernel keeps a 64-wide layout).  On a network of widths <= 64 a wide handle returns the narrow handle's bits.  The ReLU
 * kernel is the one-shot entry's arithmetic operation for operation: same bits.  The Tanh kernel restates the host routine's
 * tanh relaxation (csrc/intervals.hpp, tanh_relax) in fp64; the relaxation of a layer is computed once per box, by the pass that
 * produces the layer's pre-activation bounds (csrc/crown_batch.hpp).  A box's bits depend neither on nbox, nor on its position, nor
 * on the other literals, nor on what the handle computed before.  Not thread-safe; distinct handles are independent. */
typedef struct nnsdp_crown nnsdp_crown;

/* K, xdims, M, activ, nlit, normals as in the one-shot _lits entry (normals: ny x nlit column-major; nlit = 0: no literal pass).
 * -1 with a message for a null / one-layer network, a width outside 1..64 (the message names the width and 64), an unknown
 * activation, nlit outside 0..64, normals NULL with nlit > 0, or a non-finite normal entry ("literal i"): all before the GPU is
 * touched. */
int nnsdp_crown_create(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nlit, const double* normals,
                       nnsdp_crown** out);

/* nnsdp_crown_create with the widest hidden layer the handle's kernel takes: max_width 64 is nnsdp_crown_create exactly (its checks and
 * messages); 128 creates a wide handle, which always launches the wide instance, also on a narrow network.
 * -1 with a message, before the GPU is touched: max_width not 64 or 128; with 128, a hidden width above 128 (the message names the
 * width and 128), xdims[0] or xdims[K] above 64 (the message names the width and 64); otherwise the refusals of nnsdp_crown_create. */
int nnsdp_crown_create_wide(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nlit, const double* normals,
                            int32_t max_width, nnsdp_crown** out);

/* Bounds of nbox boxes; arguments, layouts and refusals of the boxes as in the one-shot _lits entry (HOST pointers, NULL outputs are
 * skipped, nbox = 0 returns 0; smin / smax / uA / ub0 are left alone by a handle without literals). */
int nnsdp_crown_bound(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                      double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                      double* smin, double* smax, double* uA, double* ub0, double* kernel_ms);

/* nnsdp_crown_bound plus optimised lower slopes of the unstable ReLUs for the literals' upper bounds: the iteration of
 * nnsdp_make_intervals_lits_alpha in fp64, in a second kernel (csrc/crown_alpha.hpp, one workgroup per box, both products of a step on
 * fp64 MFMA) launched behind the plain one on the handle's stream.  The arguments of nnsdp_crown_bound receive exactly what that entry
 * writes.  steps, eta0, decay as there; alpha0 NULL or [acdim x nlit x nbox] (neuron index fastest, then the literal, then the box).
 * Outputs (HOST pointers, any may be NULL): a_smax [nlit x nbox], a_uA [xdims[0] x nlit x nbox], a_ub0 [nlit x nbox], alpha
 * [acdim x nlit x nbox], best_step [nlit x nbox].  One upload (the boxes and alpha0), two launches, one download, one synchronisation.
 * The per-(literal, neuron) state lives in buffers of the handle that are allocated at the first call of this entry, grow like the
 * others and are counted by nnsdp_crown_info; a handle that never calls it holds what it held without it.  No atomics: a literal's
 * bits depend neither on nbox, nor on the box's position, nor on the other literals, nor on earlier calls.
 * -1 with a message, before the GPU is touched, for a wide handle (max_width 128), a Tanh handle, a handle without literals, steps outside 0..64, eta0 not positive
 * and finite, decay outside (0, 1], or a non-finite alpha0 entry. */
int nnsdp_crown_bound_alpha(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                            double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                            double* smin, double* smax, double* uA, double* ub0, double* kernel_ms,
                            int32_t steps, double eta0, double decay, const double* alpha0,
                            double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step);

/* Bounds on the nodes of a ReLU split (beta-CROWN style; DESIGN.md section 5, csrc/crown_relu_split.hpp).  A node is an input box and
 * an assignment s in {-1, 0, +1}^acdim, ordered like acymin: +1 forces the pre-activation z_n >= 0, -1 forces z_n <= 0, 0 leaves the
 * neuron free.  Every number returned for a node is a valid bound over {x in box : s_n z_n(x) >= 0 for all forced n}.
 * Plain pass: a forced neuron's relaxation is exact (+1: du = dl = 1, -1: du = dl = 0, bu = 0), a free neuron keeps the arithmetic of
 * nnsdp_crown_bound; the pre-activation bounds of a forced neuron are clipped (+1: l <- max(l, 0), -1: u <- min(u, 0)) and a node with
 * l > u afterwards is infeasible (its other numbers mean nothing).  branch: per literal the free neuron with l < 0 < u that has the
 * largest  max(lambda, 0) bu  (lambda the upper matrix entry entering the neuron; ties: the lowest index), -1 without a candidate.
 * Multipliers: per literal, `steps` projected-gradient steps on one multiplier beta_n >= 0 per forced neuron, which enters the upper
 * bound's backward pass as  A[n] += s_n beta_n  behind the row scaling of the neuron's layer; g_n = s_n z_n(x*), z the pre-activations
 * of the relaxed network at the maximiser of the linear bound; beta <- max(beta - eta g / max|g|, 0), eta <- eta decay from eta0.
 * smax / uA / ub0 / best_step are the first iterate with the smallest smax: never above smax_plain (iterate 0), and with no forced
 * neuron equal to it with best_step 0.  steps in 0..64, eta0 > 0 finite, decay in (0, 1].
 * x1min / x1max [xdims[0] x nnode], assign [acdim x nnode] (neuron index fastest).  Outputs (HOST pointers, any may be NULL): pre_lo,
 * pre_hi [acdim x nnode] the clipped pre-activation bounds; smin, smax_plain, smax, ub0 [nlit x nnode]; uA [xdims[0] x nlit x nnode];
 * best_step, branch [nlit x nnode]; infeasible [nnode]; kernel_ms.  One upload, two launches, one download, one synchronisation; the
 * node buffers of the handle are allocated at the first call, grow like the others and are counted by nnsdp_crown_info.  No atomics:
 * a node's bits depend neither on nnode, nor on its position, nor on the other literals, nor on earlier calls.
 * -1 with a message, before the GPU is touched: steps, eta0 or decay out of range (checked first, also on a NULL handle), a wide
 * handle, a Tanh handle, a handle without literals, an assign entry outside {-1, 0, 1}. */
int nnsdp_crown_bound_nodes(nnsdp_crown* h, int32_t nnode, const double* x1min, const double* x1max, const int8_t* assign,
                            int32_t steps, double eta0, double decay, double* pre_lo, double* pre_hi, double* smin,
                            double* smax_plain, double* smax, double* uA, double* ub0, int32_t* best_step, int32_t* branch,
                            int32_t* infeasible, double* kernel_ms);

/* The same recurrences for ONE node in the float32 host routine (csrc/intervals.hpp), multiplier steps included; no GPU needed.
 * assign [acdim]; the outputs as above with nnode = 1 (uA [xdims[0] x nlit]), infeasible one int32.  -1 with a message for a Tanh
 * network, nlit outside 1..64, an assign entry outside {-1, 0, 1}, steps, eta0 or decay out of range.  ReLU only, any width. */
int nnsdp_make_intervals_nodes(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min,
                               const double* x1max, const int8_t* assign, int32_t nlit, const double* normals, int32_t steps,
                               double eta0, double decay, double* pre_lo, double* pre_hi, double* smin, double* smax_plain,
                               double* smax, double* uA, double* ub0, int32_t* best_step, int32_t* branch, int32_t* infeasible);

/* The sampled forward pass on the resident network: the kernel, launch geometry and bits of the one-shot sampled forward entry. */
int nnsdp_crown_eval(nnsdp_crown* h, int64_t N, const double* X, double* Y, double* kernel_ms);

/* The bounds-only input-splitting search of nnsdp_amd/split.py (_split_levels with sdp_per_level = 0, samples = 0) with the frontier
 * kept on the device (csrc/crown_search.hpp): decides the clause  OR_i normal_i' f(x) <= hs[i]  on the root box x1min / x1max
 * (xdims[0] each) by bisection along the coordinate that is widest relative to the root.  Per level: the handle's bound kernel on
 * chunks of at most `chunk` boxes read directly from the frontier, the proof test (sum_j max(n_ij ymin_j, n_ij ymax_j), with
 * literal_bounds the smaller of that and the literal pass's smax, minus hs[i]; the first minimum over i is the box's best literal; proved
 * when it is <= 0), the forward pass on the open boxes' centres and (corner_points) the corners where(uA[best] >= 0, hi, lo), the
 * bisection of the open boxes into the second frontier and the proved boxes' rows of a leaf log, all in device memory; the host reads
 * back four integers per level (boxes bounded, proved, open, candidate points).  The tree, the order of the leaves and every number
 * are those of the Python loop, bit for bit: the sum of the proof test has the order of numpy's pairwise reduction as split.py reaches
 * it (plain ascending below 8 outputs, eight interleaved partial sums from 8 on; csrc/crown_frontier.hpp, search_cheap).
 * The clause: a handle created with literals uses them (normals NULL, nlit the handle's); a handle without takes normals (ny x nlit
 * column-major, nlit in 1..64) and can neither use literal_bounds nor corner_points.
 * confirm: called on the host, only on a level that has candidate points, for each candidate in the order centres then corners, each
 * in box order, with `user` and the point (xdims[0] doubles); a return value other than 0 makes the point the witness and ends the
 * search (the split driver evaluates the network in fp64 there).  NULL accepts the first candidate as the device flagged it.
 * The search ends "holds" (verdict 0) when no box is open, "violated" (1) with the witness, "unknown" (2) when max_boxes boxes were
 * bounded, a level deeper than max_depth would be needed or no coordinate can be split.  Outputs: verdict, visited (boxes bounded),
 * depth_reached (the last level), nleaves (for nnsdp_crown_search_leaves), witness (xdims[0], written when violated), kernel_ms (may be
 * NULL: event time of all launches).
 * Device memory: 80 xdims[0] max_boxes bytes of frontiers (two of 2 max_boxes boxes) and, per box of max_boxes,
 * 8 (4 + (2 + p) xdims[0] + p xdims[K]) + 4 (4 + p) bytes of records, points and leaf log (p = 2 with corner_points, else 1), allocated at
 * the first search and reused by a later one that needs no more; the bound kernel's buffers grow with the
 * levels and stop at one chunk (min(chunk, max_boxes) boxes), unless an earlier bound call made them larger.  Counted by
 * nnsdp_crown_info.  On the host the handle keeps a pinned status record of four integers, a copy of its normals and the leaves of
 * the last search.
 * -1 with a message, before the GPU is touched and before anything is allocated: max_boxes < 1, chunk < 1, max_depth < 0, a null
 * handle or argument, literal_bounds / corner_points on a handle without literals, normals given to a handle with literals, nlit that
 * does not fit, a non-finite normal, threshold or box entry, x1min > x1max, frontiers above 2^31 bytes.  Not thread-safe. */
typedef int32_t (*nnsdp_confirm_fn)(void* user, const double* x);
int nnsdp_crown_search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                       int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                       nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                       int32_t* nleaves, double* witness, double* kernel_ms);

/* The leaves of the handle's last search, in the order of the Python loop (HOST arrays of nleaves entries; lo / hi xdims[0] x nleaves
 * column-major): proved 1 ("crown") or 0 (open); literal -1 for a box that the budget kept from being bounded (its bound is then
 * meaningless), else the proved literal, or the best literal of an open box, with its bound. */
int nnsdp_crown_search_leaves(nnsdp_crown* h, double* lo, double* hi, int32_t* depth, int32_t* proved, int32_t* literal, double* bound);

/* nnsdp_crown_search for nroot root boxes in ONE level loop (csrc/crown_forest.hpp): the same network and normals, root r the box
 * x1min / x1max column r (xdims[0] x nroot column-major) with the thresholds hs column r (nlit x nroot column-major), its own
 * splittable coordinates, and max_boxes / max_depth applied to it alone.  Level d of every root that is still undecided forms one
 * frontier in device memory, ordered by root, so one pass of launches (the bound kernel on chunks of at most `chunk` boxes, which
 * may cross root boundaries), one synchronisation and one read-back of three integers per undecided root serve all of them; a
 * decided root leaves the frontier.  Per root the outputs (verdict, visited, depth_reached, nleaves: nroot each; witness: xdims[0] x
 * nroot, column r written when root r is violated) and the leaves are those of nnsdp_crown_search on that root alone, bit for bit and
 * in the same order.  A root's level beyond its budget is bounded with the others and thrown away; visited does not count it.
 * confirm: as in nnsdp_crown_search, with the index of the root whose candidate it is; per root in that entry's order.
 * kernel_ms (may be NULL): event time of all launches.
 * Memory: the roots are handled in groups that share one set of buffers, one group after the other; a group is the largest number of
 * roots whose frontier buffers, point and leaf-log buffers and record buffers each stay within 2^31 bytes (nnsdp_crown_forest_plan
 * states the rule), or `group` when that is positive and smaller.  The results do not depend on the grouping.  The buffers are the
 * forest's own, allocated at the first call and reused by a later call that needs no more; counted by nnsdp_crown_info, where every
 * launch of the bound kernel counts as a bound call.
 * -1 with a message: max_boxes < 1, chunk < 1, max_depth < 0, group < 0, nroot < 0 (in this order, before the handle is used; nroot
 * = 0 then returns 0 at once), a null handle or argument, the clause refusals of nnsdp_crown_search, a non-finite threshold (the
 * message names the root and the literal) or box entry or x1min > x1max (it names the root), one root whose buffers exceed 2^31
 * bytes (it gives the byte count).  Not thread-safe. */
typedef int32_t (*nnsdp_confirm_many_fn)(void* user, int32_t root, const double* x);
int nnsdp_crown_search_many(nnsdp_crown* h, int32_t nroot, const double* x1min, const double* x1max, int32_t nlit, const double* normals,
                            const double* hs, int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth,
                            int32_t chunk, int32_t group, nnsdp_confirm_many_fn confirm, void* user, int32_t* verdict, int32_t* visited,
                            int32_t* depth_reached, int32_t* nleaves, double* witness, double* kernel_ms);

/* The leaves of root `root` of the handle's last nnsdp_crown_search_many, as nnsdp_crown_search_leaves gives them; root = -1: the
 * leaves of all roots, one root after the other (the sum of nleaves entries). */
int nnsdp_crown_search_many_leaves(nnsdp_crown* h, int32_t root, double* lo, double* hi, int32_t* depth, int32_t* proved, int32_t* literal,
                                   double* bound);

/* The grouping rule of nnsdp_crown_search_many, without a handle or a GPU: for input width n0, output width ny, nlit literals,
 * max_boxes, corner_points, nroot roots and the `group` argument, out[0] = roots per group, out[1] = boxes a level of the group can
 * hold (2 max_boxes per root; at most 2^26, the longest level of the scan), out[2] = bytes of the two frontiers, out[3] = bytes of the
 * point and leaf-log buffers, out[4] = bytes of the record buffers.  -1 with the byte count when one root does not fit. */
int nnsdp_crown_forest_plan(int32_t n0, int32_t ny, int32_t nlit, int32_t max_boxes, int32_t corner_points, int32_t nroot, int32_t group,
                            int64_t* out);

/* The reach search of nnsdp_amd/split.py (reachSplit, _reach_levels with sdp_per_level = 0) with the frontier kept on the device
 * (csrc/crown_reach.hpp): encloses the support values  max_x c_i' f(x)  of the handle's nlit directions c_i over the root box
 * x1min / x1max (xdims[0] each) by branch and bound with an incumbent, on ONE bisection tree for all directions.  Per level: the
 * handle's bound kernel on chunks of at most `chunk` boxes read directly from the frontier; per box  ub[i] = min(sum_j max(c_ij ymin_j,
 * c_ij ymax_j), smax_i)  (the sum as in nnsdp_crown_search), the centre and, with corner_points, per direction the corner
 * where(uA[i] >= 0, hi, lo); the forward pass on the level's (1 + nlit) nb (corner_points, else nb) points; per direction
 * s = c_i[0] y_0, then + c_i[j] y_j for j ascending, every product and sum rounded on its own, the first maximum over the points in the
 * order centres, then the corners of direction 0, 1, ..., each in box order; it replaces the incumbent L_i and its point when it is
 * greater; thr_i = L_i + tol[i]; a box is open when ub[i] > thr_i for some i; open boxes are bisected along the coordinate widest relative
 * to the root into the second frontier, closed ones write lo, hi, depth and ub to a leaf log, all in device memory; the host reads back
 * four integers per level.  The tree, the order of the leaves and every number are those of the Python loop with crown_backend
 * "resident", bit for bit.  No atomics.
 * The search ends "converged" (status 0) when no box is open, "budget" (1) when a level deeper than max_depth would be needed, no
 * coordinate can be split, or the children of the open boxes would make more than max_boxes boxes bounded: a level is only created
 * when the budget holds all of it, so visited <= max_boxes and every leaf has its bounds.  Outputs: status, visited (boxes bounded),
 * depth_reached (the last level), nleaves (for nnsdp_crown_reach_leaves), incumbent (nlit: L_i), witnesses (xdims[0] x nlit column-major:
 * the point of L_i), kernel_ms (may be NULL: event time of all launches).
 * Device memory: 40 xdims[0] max_boxes bytes of frontiers (two of max_boxes boxes) and, per box of max_boxes, 8 (1 + 2 nlit +
 * (2 + p) xdims[0] + p xdims[K]) + 12 bytes of records, points and leaf log (p = 1 + nlit with corner_points, else 1), allocated at the
 * first call from max_boxes and reused by a later call that needs no more (a second identical call allocates nothing); the buffers are
 * the reach search's own, so bound, search and reach can follow each other in any order on one handle; the bound kernel's buffers are
 * shared and grow as in nnsdp_crown_search.  Counted by nnsdp_crown_info.
 * -1 with a message, before the GPU is touched and before anything is allocated: max_boxes < 1, chunk < 1, max_depth < 0, a null handle
 * (in this order, before the handle is used) or argument, a handle created without normals, nlit that is not the handle's, a tol that is
 * negative or not finite, a non-finite box entry, x1min > x1max, frontiers or point buffers above 2^31 bytes.  Not thread-safe. */
int nnsdp_crown_reach(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* tol, int32_t corner_points,
                      int32_t max_boxes, int32_t max_depth, int32_t chunk, int32_t* status, int32_t* visited, int32_t* depth_reached,
                      int32_t* nleaves, double* incumbent, double* witnesses, double* kernel_ms);

/* The leaves of the handle's last reach search, in the order of the Python loop (HOST arrays of nleaves entries; lo / hi xdims[0] x
 * nleaves, bound nlit x nleaves, column-major): closed 1 ("crown") or 0 (open: the budget ended the search); bound: ub of every direction. */
int nnsdp_crown_reach_leaves(nnsdp_crown* h, double* lo, double* hi, int32_t* depth, int32_t* closed, double* bound);

/* The ReLU-split search of nnsdp_amd/relusplit.py (verifyReluSplit, _levels) with the node frontier kept on the device
 * (csrc/crown_node_search.hpp): decides the clause  OR_i normal_i' f(x) <= hs[i]  of the handle's literals on the root box x1min / x1max
 * (xdims[0] each) by forcing the signs of unstable ReLUs.  A node is an assignment in {-1, 0, +1}^acdim; the frontier is two buffers
 * of acdim x max_nodes bytes.  Per level: the two node kernels of nnsdp_crown_bound_nodes on chunks of at most `chunk` nodes, their
 * assignments read directly from the frontier and their boxes from one chunk of copies of the root box written once; per node the
 * infeasible flag first, else the first minimum over i of smax_i - hs[i] (closed by "bound" when it is <= 0, else stuck when the best
 * literal has no neuron to branch on, else branching); the forward pass on the level's points: the box centre and (corner_points) per
 * node and literal  c + sign(uA_i) r, c = 0.5 (lo + hi), r = 0.5 (hi - lo), sign(0) = 0, product and sum rounded separately; a point is
 * a candidate when every literal is false there and (except the centre) its node is open; closed nodes write assignment, depth, kind
 * and bound to a leaf log, stuck nodes to a second log, the r-th branching node its children 2r (its neuron forced +1) and 2r + 1 (-1)
 * into the other frontier, all in device memory.  The host reads back five integers per level (bounded, closed, stuck, branching,
 * candidates), the flags and points only on a level that counts candidates, and the leaves once at the end.  Verdict, reason, visited,
 * depth, witness and the order and bits of the leaves are those of the Python loop on the resident bounder, for any chunk.  No atomics.
 * confirm: called on the host for the flagged points of a level without duplicates, in lexicographic order of their coordinates (the
 * first most significant); a return value other than 0 makes the point the witness.  NULL accepts the first.
 * The search ends "holds" (verdict 0) when every node is closed, "violated" (1) with the witness, "unknown" (2) with reason 1 (budget:
 * the children of the branching nodes would make more than max_nodes nodes bounded, or be deeper than max_depth; a level is only
 * created when the budget holds all of it) or 2 (exhausted: stuck nodes remain and nothing branches).  Outputs: verdict, reason (0
 * unless unknown), visited, depth_reached, nleaves (closed leaves), nopen (open nodes), witness (xdims[0], written when violated),
 * kernel_ms (may be NULL: event time of all launches).
 * Device memory: 4 acdim max_nodes bytes of frontiers and logs, and per node of max_nodes 8 (3 + p (xdims[0] + xdims[K])) + 4 (9 + p)
 * bytes of records and points (p = nlit with corner_points, else 0), allocated at the first search and reused by a later one that
 * needs no more; the node kernels' buffers are those of nnsdp_crown_bound_nodes and hold min(chunk, max_nodes) nodes unless an
 * earlier call made them larger.  Counted by nnsdp_crown_info.
 * -1 with a message, before the GPU is touched and before anything is allocated: max_nodes < 1, chunk < 1, max_depth < 0, steps, eta0
 * or decay out of range (in this order, also on a NULL handle), a null handle, a wide handle, a Tanh handle, a handle without
 * literals, a null argument, nlit that is not the handle's, a non-finite threshold or box entry, x1min > x1max, buffers above 2^31
 * bytes.  Not thread-safe. */
int nnsdp_crown_search_nodes(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* hs, int32_t steps,
                             double eta0, double decay, int32_t corner_points, int32_t max_nodes, int32_t max_depth, int32_t chunk,
                             nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* reason, int32_t* visited, int32_t* depth_reached,
                             int32_t* nleaves, int32_t* nopen, double* witness, double* kernel_ms);

/* The leaves of the handle's last node search (HOST arrays of nleaves + nopen rows; assign acdim per row): the closed leaves in level
 * order and then node order (closed_by 0 infeasible, with a NaN bound, or 1 bound), then the open nodes (closed_by -1) in the order of
 * the Python loop: the stuck nodes of earlier levels, then on "violated" every open node of the last level, on "budget" its stuck
 * and then its branching nodes.  bound: smax of the literal closest to its threshold. */
int nnsdp_crown_search_nodes_leaves(nnsdp_crown* h, int8_t* assign, int32_t* depth, int32_t* closed_by, double* bound);

/* what: 0 device allocations made so far, 1 network uploads so far, 2 box capacity, 3 sample capacity, 4 bound calls (a search, a
 * search_many and a node search count one per chunk), 5 device bytes held, 6 reach searches so far, 7 the handle's max_width (64 or
 * 128), 8 node searches so far, 9 status records (levels) they read back, 10 levels whose flags and points they downloaded. */
int nnsdp_crown_info(nnsdp_crown* h, int32_t what, double* out);

/* NULL is a no-op returning 0. */
int nnsdp_crown_destroy(nnsdp_crown* h);

/* Batched projection onto the PSD cone, the hot kernel (replaces the cone handling inside MOSEK;
 * reference of the arithmetic: LinearAlgebra.eigen on Symmetric).  mats: `batch` symmetric
 * matrices back to back, matrix b is n[b] x n[b] column-major.  Matrices up to 160 go through the LDS-resident Jacobi kernel
 * (one launch for all of them; 129 .. 160 in its packed-triangle variant), larger ones (up to 4096) one at a time through rocSOLVER
 * dsyevd + rocBLAS dgemm.  out receives
 * the projections, eigvals (may be NULL) sum(n) eigenvalues.  in/out are HOST pointers. */
int nnsdp_project_psd_batched(int32_t batch, const int32_t* n, const double* mats, double* out,
                              double* eigvals, double* kernel_ms);

/* Test / diagnostic entry of the same kernel in its WARM form, as the solver runs it from the second iteration on: basis (in / out,
 * matrices back to back like mats, column-major, columns = eigenvectors) is the eigenbasis kept from the previous projection; tol
 * the relative stopping level off(V'AV) <= tol |A|_F; refine != 0 puts the GEMM-only refinement stage (nnsdp_options.proj_refine)
 * in front of the Jacobi sweeps (values as proj_refine).  outcome[5] (may be NULL) counts the blocks: converged as given / one
 * refinement step / sent on to the sweeps / not attempted / accepted after a checked step.  Matrices up to 160.  Host pointers. */
int nnsdp_project_psd_warm(int32_t batch, const int32_t* n, const double* mats, double* basis, double tol, int32_t refine, double* out,
                           int32_t* outcome, double* kernel_ms);
/* The same with the refinement stage's per-block state carried between calls, as a solver carries it between iterations: state (in /
 * out, 4 x batch int32, all zero before the first call; NULL = fresh state every call) holds the back-off word - bits 24..27 of word
 * 0 count the visits that may still run without the Gram product V'V - and the running estimate of |I - V'V|_F (words 2..3, a double). */
int nnsdp_project_psd_warm_state(int32_t batch, const int32_t* n, const double* mats, double* basis, double tol, int32_t refine, double* out,
                                 int32_t* outcome, double* kernel_ms, int32_t* state);

/* Multi-GPU clique-sharded mode (one SDP over several GPUs of one node): every rank creates the same solver,
 * then nnsdp_solver_set_comm() before the first iteration.  Rank r projects a contiguous range of cliques
 * (balanced by n_k^3); the consensus sum sum_k H_k'(2 w_k - nu_k) is exchanged with ONE ncclAllReduce (RCCL
 * over xGMI) per iteration, everything else is replicated.  The 128-byte unique id is produced on rank 0
 * and distributed by the host launcher (torch.distributed in bench.py --mode shard).  RCCL is dlopen'ed on
 * first use.  Independent SDPs need none of this (nnsdp_amd/parallel.py).  Every stopping / penalty / tolerance decision of
 * a sharded solve is taken from all-reduced numbers, so all ranks take it identically (including the time limit).
 * The replicated multiplier block is re-synchronised from rank 0 at every check iteration and the certificate (polish, eigmax) and
 * the cert_tol stop are computed by rank 0 alone and broadcast, so all ranks return the same bits; nnsdp_solver_run / _finish are
 * therefore COLLECTIVE calls in this mode.  Over RCCL the iterations between checks replay a hipGraph that contains the all-reduce
 * (probed at set_comm; eager otherwise).  Covered by a two-process run on one GPU through nnsdp_solver_set_comm_callback (below;
 * RCCL refuses two ranks on one device) and a one-rank RCCL run; RCCL with more than one rank has not run yet (the build pool
 * offers one GPU). */
int nnsdp_comm_unique_id(char* id128);
/* Host-only (no GPU, no RCCL): the PSD blocks the solver works on for (problem, options) and their partition over `nranks`
 * ranks - exactly what nnsdp_solver_set_comm uses.  Two-pass: n_blocks first (block_n = start = NULL), then
 * block_n[n_blocks] (block dimensions after the normalisation) and start[nranks+1] (rank r owns blocks start[r] .. start[r+1]-1). */
int nnsdp_shard_plan(const nnsdp_problem* p, const nnsdp_options* o, int32_t nranks, int32_t* n_blocks, int32_t* block_n,
                     int32_t* start);
/* Host-only (no GPU): the plan of the sparse NSD check for (problem, options) - symbolic elimination of the solver's clique pattern
 * (reduced coordinates, stored order, the affine index a = n - 1 last and never eliminated; a is a row of every front).  n: reduced
 * dimension; supernodes are the column ranges col_start[s] .. col_start[s+1]-1 (col_start[n_super] = n - 1); rows row_idx[row_ptr[s] ..
 * row_ptr[s+1]-1] lie below supernode s's diagonal block (ascending, fill included, the last one is a); the parent of s is the supernode
 * of its first row (none when that row is a: the plan may be a forest); max_front: the largest columns + rows; fill: entries of the
 * factor's structure outside the pattern; supported: max_front <= 128.  Two-pass: any of the three arrays may be NULL; row_idx needs
 * row_ptr[n_super] <= n_super x max_front entries. */
int nnsdp_cert_plan(const nnsdp_problem* p, const nnsdp_options* o, int32_t* n, int32_t* n_super, int32_t* max_front, int64_t* fill,
                    int32_t* supported, int32_t* col_start, int32_t* row_ptr, int32_t* row_idx);
/* Test / diagnostic entry of the sparse NSD check on dense input: `mats` holds `batch` symmetric n x n column-major matrices on the
 * clique pattern (ptr / idx as nnsdp_make_cliques returns them; index n - 1 is the affine index a).  Candidate b is negative
 * semidefinite exactly when ok[b] = 1 - every pivot of the Cholesky of -M_xx exceeded 1e-13 x the largest diagonal entry of its
 * supernode's columns as assembled - and schur[b] = M_aa - m_xa' M_xx^-1 m_xa <= 0.  min_pivot[b]: the smallest pivot met; for a
 * candidate with ok[b] = 0, schur[b] holds the first failing column instead.  A candidate's bits do not depend on the batch size or on
 * its position.  -1: a non-zero entry outside the pattern; -2 (before any launch): a front above 128.  kernel_ms: HIP-event time. */
int nnsdp_sparse_nsd(int32_t n, int32_t n_cliques, const int32_t* ptr, const int32_t* idx, int32_t batch, const double* mats, int32_t* ok,
                     double* min_pivot, double* schur, double* kernel_ms);
int nnsdp_solver_set_comm(nnsdp_solver* s, int32_t nranks, int32_t rank, const char* id128);
/* The same sharded mode over the CALLER's collective instead of RCCL (MPI.Allreduce! from the Julia side; gloo in the
 * two-process GPU test): fn(user, buf, count) replaces the HOST buffer buf[count] by its element-wise sum over all ranks and
 * returns 0.  The library stages the per-iteration exchange (and the 8 control numbers of a check iteration) through host
 * memory for it; partition, kernels and the collective control decisions are those of nnsdp_solver_set_comm. */
typedef int (*nnsdp_allreduce_fn)(void* user, double* buf, int64_t count);
int nnsdp_solver_set_comm_callback(nnsdp_solver* s, int32_t nranks, int32_t rank, nnsdp_allreduce_fn fn, void* user);
/* The sharded mode with a DEVICE-SIDE exchange for ranks that are processes of one node (one card, or peers over xGMI; at most 8):
 * every rank's exchange buffer is mapped into the others' address space with hipIpc, and the per-iteration exchange is a one-shot
 * all-gather + local reduce in rank order by the library's own kernels (slot of the rank's buffer, exchange number published behind a
 * system-scope release, bounded spin on the peers' numbers) - no library collective in the iteration, the same bits on every rank,
 * capturable into the iteration's hipGraph.  fn is used as in nnsdp_solver_set_comm_callback for the set-up (the 64-byte handles) and
 * for the control decisions of the check iterations.  A peer that does not publish within a few seconds fails the next check
 * iteration with an error instead of hanging the device.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver only supports dmabuf. */
int nnsdp_solver_set_comm_ipc(nnsdp_solver* s, int32_t nranks, int32_t rank, nnsdp_allreduce_fn fn, void* user);

#ifdef __cplusplus
}
#endif
#endif /* NNSDP_H */
