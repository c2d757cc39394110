// C ABI of libnnsdp_hip.so (include/nnsdp.h): host orchestration of the HIP kernels.
// One ADMM iteration = 6 kernels on one stream; `check_every` iterations are captured into a
// hipGraph and replayed, so the host only touches the device once per convergence check.
#include "host_common.hpp"
#include "kernels.hip"
#include "refine_pipe.hpp"
#include "setup.hpp"
#include "cert_plan.hpp"
#include "minv.hpp"
#include "intervals.hpp"
#include "forward.hpp"
#include "crown_batch.hpp"
#include "crown_wide.hpp"
#include "crown_alpha.hpp"
#include "crown_relu_split.hpp"
#include "crown_search.hpp"
#include "crown_forest.hpp"
#include "crown_reach.hpp"
#include "crown_node_search.hpp"
#include "solver.hpp"
#include "batch.hpp"
#include "crown_handle.hpp"
#include "crown_frontier_host.hpp"

#define API_BEGIN try {
#define API_END                                                                    \
  }                                                                                \
  catch (const std::invalid_argument& e) { g_err = e.what(); return -1; }          \
  catch (const HipError& e) { g_err = e.what(); return 2; }                        \
  catch (const std::bad_alloc&) { g_err = "out of host memory"; return 3; }        \
  catch (const std::exception& e) { g_err = e.what(); return 1; }                  \
  catch (...) { g_err = "unknown error"; return 1; }                               \
  return 0;

extern "C" {

int nnsdp_version(void) { return NNSDP_VERSION; }
const char* nnsdp_last_error(void) { return g_err.c_str(); }

const char* nnsdp_status_string(int32_t s) {
  switch (s) {
    case NNSDP_STATUS_OPTIMAL: return "OPTIMAL";
    case NNSDP_STATUS_ITERATION_LIMIT: return "ITERATION_LIMIT";
    case NNSDP_STATUS_TIME_LIMIT: return "TIME_LIMIT";
    case NNSDP_STATUS_SLOW_PROGRESS: return "SLOW_PROGRESS";
    case NNSDP_STATUS_NUMERICAL_ERROR: return "NUMERICAL_ERROR";
    case NNSDP_STATUS_TARGET_CERTIFIED: return "TARGET_CERTIFIED";
    case NNSDP_STATUS_TARGET_UNREACHABLE: return "TARGET_UNREACHABLE";
    default: return "UNKNOWN";
  }
}

void nnsdp_default_options(nnsdp_options* o) {
  if (!o) return;
  o->decomp_mode = NNSDP_DECOMP_SINGLE;
  o->max_iters = 20000;
  o->eps_rel = 1e-6;
  o->max_time = 0.0;
  o->sigma = 0.1;
  o->alpha = 1.6;
  o->adapt_every = 50;
  o->check_every = 50;
  o->normalize = 1;
  o->warm_start = 1;
  o->proj_tol = 0.0;
  o->polish = 1;
  o->cert_tol = 0.0;
  o->verbose = 0;
  o->device = -1;
  o->interval_guard = 5e-5;
  o->minv_mode = 0;
  o->proj_refine = 1;
}

int nnsdp_problem_dims(const nnsdp_problem* p, int32_t* Zdim, int32_t* acdim, int32_t* nac2, int32_t* ngamma) {
  API_BEGIN
  if (!p || !p->xdims) throw std::invalid_argument("null problem");
  if (p->K < 2) throw std::invalid_argument("K must be >= 2");
  int z = 1, ac = 0;
  for (int k = 0; k < p->K; ++k) z += p->xdims[k];
  for (int k = 1; k < p->K; ++k) ac += p->xdims[k];
  int beta = p->beta;
  if (beta < 0 || beta > ac) throw std::invalid_argument("beta out of range");
  int n2 = (beta + 1) * ac - beta * (beta + 1) / 2 + (p->activ == NNSDP_ACTIV_TANH ? 0 : 2 * ac);
  if (Zdim) *Zdim = z;
  if (acdim) *acdim = ac;
  if (nac2) *nac2 = n2;
  if (ngamma) *ngamma = p->xdims[0] + (p->query_kind == NNSDP_QUERY_REACH ? 1 : 0) + ac + n2;
  API_END
}

int nnsdp_solver_create(const nnsdp_problem* p, const nnsdp_options* o, nnsdp_solver** out) {
  API_BEGIN
  if (!p || !o || !out) throw std::invalid_argument("null argument");
  std::unique_ptr<nnsdp_solver> s(new nnsdp_solver());
  s->setup(p, o);
  *out = s.release();
  API_END
}

int nnsdp_solver_create_sibling(nnsdp_solver* parent, const nnsdp_problem* p, nnsdp_solver** out) {
  API_BEGIN
  if (!parent || !p || !out) throw std::invalid_argument("null argument");
  std::unique_ptr<nnsdp_solver> s(new nnsdp_solver());
  s->setup_sibling(*parent, p);
  *out = s.release();
  API_END
}

int nnsdp_solver_iterate(nnsdp_solver* s, int32_t iters, double* eig_ms) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (iters < 0) throw std::invalid_argument("iters must be >= 0");
  double t0 = now_s();
  s->iterate(iters, eig_ms);
  s->t_solve += now_s() - t0;
  API_END
}

int nnsdp_solver_advance(nnsdp_solver* s, int32_t iters) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (iters < 0) throw std::invalid_argument("iters must be >= 0");
  if (iters > 0) (void)s->run_loop(iters);
  API_END
}

int nnsdp_solver_iterate_async(nnsdp_solver* s, int32_t iters) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (iters < 0) throw std::invalid_argument("iters must be >= 0");
  s->iterate(iters, nullptr, false);
  API_END
}

int nnsdp_solver_sync(nnsdp_solver* s) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  HIPCHK(hipStreamSynchronize(s->st));
  API_END
}

int nnsdp_solver_residuals(nnsdp_solver* s, double* pres, double* dres, double* pobj, double* dobj) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  s->check_iteration();
  if (pres) *pres = s->last_pres;
  if (dres) *dres = s->last_dres;
  if (pobj) *pobj = s->last_pobj;
  if (dobj) *dobj = s->last_dobj;
  API_END
}

int nnsdp_solver_apply_minv(nnsdp_solver* s, const double* q, double* out, int32_t* structured, int64_t* operand_bytes) {
  API_BEGIN
  if (!s || !q || !out) throw std::invalid_argument("null argument");
  const int ng = s->S.ng;
  std::vector<double> qk(ng);
  for (int g = 0; g < ng; ++g) qk[g] = q[s->S.keep[g]];
  HIPCHK(hipMemcpy(s->qv.p, qk.data(), ng * sizeof(double), hipMemcpyHostToDevice));
  s->enqueue_minv(s->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->st));
  std::vector<double> o = s->ww.download();
  for (int g = 0; g < s->P.ng; ++g) out[g] = 0.0;
  for (int g = 0; g < ng; ++g) out[s->S.keep[g]] = o[g];
  if (structured) *structured = s->minv_structured ? 1 : 0;
  if (operand_bytes)
    *operand_bytes = s->minv_structured ? (int64_t)((s->m_P.n + s->m_H.n + s->m_HT.n + s->m_Sc.n + s->m_v.n) * sizeof(double))
                                        : (int64_t)(s->Minv.n * sizeof(double));
  API_END
}

int nnsdp_solver_apply_minv_multi(nnsdp_solver* s, int32_t nrhs, const double* Q, double* out, double* kernel_ms) {
  API_BEGIN
  if (!s || !Q || !out) throw std::invalid_argument("null argument");
  if (nrhs < 1) throw std::invalid_argument("nrhs must be >= 1");
  if (s->minv_structured) throw std::invalid_argument("the fused multi-vector product needs a dense M^-1 (this handle's is structured)");
  const int ng = s->S.ng, ldm = s->ldm, full = s->P.ng;
  // every vector gets an IterArgs slot of its own, as members of a batch have: the solver's binding with qv and ww redirected
  DBuf<double> qd, wd;
  std::vector<double> qh((size_t)nrhs * ldm, 0.0);
  for (int j = 0; j < nrhs; ++j)
    for (int g = 0; g < ng; ++g) qh[(size_t)j * ldm + g] = Q[(size_t)j * full + s->S.keep[g]];
  qd.upload(qh);
  wd.alloc((size_t)nrhs * ldm); wd.zero();
  std::vector<IterArgs> it(nrhs, s->iter_args());
  std::vector<int> mem(nrhs);
  std::vector<FusedPass> ps;
  for (int j = 0; j < nrhs; ++j) {
    it[j].qv = qd.p + (size_t)j * ldm; it[j].ww = wd.p + (size_t)j * ldm;
    mem[j] = j;
    if (j % kFusedWidth == 0) ps.push_back(FusedPass{j, std::min<int>(kFusedWidth, nrhs - j)});
  }
  DBuf<IterArgs> dit; DBuf<int> dmem; DBuf<FusedPass> dps;
  dit.upload(it); dmem.upload(mem); dps.upload(ps);
  EventPair ev;
  ev.create();
  HIPCHK(hipEventRecord(ev.e0, s->st));
  launch_minv_family(s->tg, dit.p, dmem.p, dps.p, (int)ps.size(), s->st);
  HIPCHK(hipEventRecord(ev.e1, s->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->st));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
  if (kernel_ms) *kernel_ms = ms;
  std::vector<double> o = wd.download();
  for (size_t i = 0; i < (size_t)nrhs * full; ++i) out[i] = 0.0;
  for (int j = 0; j < nrhs; ++j)
    for (int g = 0; g < ng; ++g) out[(size_t)j * full + s->S.keep[g]] = o[(size_t)j * ldm + g];
  API_END
}

int nnsdp_solver_apply_minv_structured_multi(nnsdp_solver* s, int32_t nrhs, const double* Q, double* out, double* kernel_ms) {
  API_BEGIN
  if (!s || !Q || !out) throw std::invalid_argument("null argument");
  if (nrhs < 1) throw std::invalid_argument("nrhs must be >= 1");
  if (!s->minv_structured) throw std::invalid_argument("the fused structured stages need a structured M^-1 (this handle's is dense)");
  auto even = [](size_t v) { return (v + 1) & ~(size_t)1; };      // (16-byte aligned pieces: the stages load vectors in pairs)
  const int ng = s->S.ng, full = s->P.ng;
  const size_t eg = even(ng), eS = even(std::max(s->mplan.ldS, 2)), esl = even(std::max(s->m_nslots, 1));
  // every vector gets work buffers of its own, as the members of a family have
  const size_t per = 3 * eg + esl + 2 * eS + 8 + 8 * kMinvParts;
  DBuf<double> buf;
  buf.alloc(per * nrhs); buf.zero();
  std::vector<double> qh(per * nrhs, 0.0);
  for (int j = 0; j < nrhs; ++j)
    for (int g = 0; g < ng; ++g) qh[per * j + g] = Q[(size_t)j * full + s->S.keep[g]];
  HIPCHK(hipMemcpy(buf.p, qh.data(), qh.size() * sizeof(double), hipMemcpyHostToDevice));
  std::vector<MinvWork> wk(nrhs);
  std::vector<MinvPass> ps;
  for (int j = 0; j < nrhs; ++j) {
    double* b = buf.p + per * j;
    wk[j].q = b; wk[j].out = b + eg; wk[j].t = b + 2 * eg; b += 3 * eg;
    wk[j].rpart = b; b += esl;
    wk[j].rvec = b; wk[j].xS = b + eS; b += 2 * eS;
    wk[j].coef = b; wk[j].dpart = b + 8;
    if (j % kMinvWidth == 0) ps.push_back(MinvPass{0, j, std::min<int>(kMinvWidth, nrhs - j)});
  }
  EventPair ev;
  ev.create();
  DBuf<MinvFactors> dfac; DBuf<MinvWork> dwk; DBuf<MinvPass> dps;
  if (s->m_lds.ok) {
    std::vector<MinvFactors> fc(1, s->mdev);
    dfac.upload(fc); dwk.upload(wk); dps.upload(ps);
    MinvMultiGrid G;
    G.add(s->mdev, s->m_lds, std::min<int>(kMinvWidth, nrhs));
    HIPCHK(minv_multi_allow_lds());
    HIPCHK(hipEventRecord(ev.e0, s->st));
    launch_minv_multi(G, dfac.p, dwk.p, dps.p, (int)ps.size(), s->st);
  } else {      // one vector of these factors does not fit in LDS: the single form per vector (the same bits)
    HIPCHK(hipEventRecord(ev.e0, s->st));
    for (int j = 0; j < nrhs; ++j) s->apply_structured_minv(wk[j].q, wk[j].out, s->st);
  }
  HIPCHK(hipEventRecord(ev.e1, s->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->st));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
  if (kernel_ms) *kernel_ms = ms;
  std::vector<double> o = buf.download();
  for (size_t i = 0; i < (size_t)nrhs * full; ++i) out[i] = 0.0;
  for (int j = 0; j < nrhs; ++j)
    for (int g = 0; g < ng; ++g) out[(size_t)j * full + s->S.keep[g]] = o[per * j + eg + g];
  API_END
}

int nnsdp_solver_raw_multipliers(nnsdp_solver* s, double* out) {
  API_BEGIN
  if (!s || !out) throw std::invalid_argument("null argument");
  HIPCHK(hipStreamSynchronize(s->st));
  std::vector<double> h(s->S.ng);
  if (s->S.ng) HIPCHK(hipMemcpy(h.data(), s->nu.p, (size_t)s->S.ng * sizeof(double), hipMemcpyDeviceToHost));
  for (int g = 0; g < s->P.ng; ++g) out[g] = 0.0;
  for (int g = 0; g < s->S.ng; ++g) out[s->S.keep[g]] = h[g];
  API_END
}

int nnsdp_solver_info(nnsdp_solver* s, int32_t what, double* out) {
  API_BEGIN
  if (!s || !out) throw std::invalid_argument("null argument");
  switch (what) {
    case 0: *out = (double)s->graph_launches; break;
    case 1: *out = s->rccl_graph_ok ? 1.0 : 0.0; break;
    case 2: *out = s->sharded ? 1.0 : 0.0; break;
    case 3: *out = (double)s->iters_done; break;
    case 4: *out = (double)s->ncl; break;
    case 5: *out = (double)s->nmax; break;
    case 6: *out = s->ipc ? (s->ipc_fine ? 2.0 : 1.0) : 0.0; break;
    case 7: *out = (double)s->family; break;
    case 10: *out = s->minv_structured ? (double)s->mplan.nchunk : 0.0; break;
    case 11: {
      int odd = 0;
      if (s->minv_structured) for (int j = 0; j < s->mplan.nchunk; ++j) odd += ((s->mplan.clo[j] | s->mplan.w0[j]) & 1);
      *out = (double)odd;
      break;
    }
    case 12: *out = (double)s->sparse_calls; break;
    case 13: *out = s->cert_ready() ? 1.0 : 0.0; break;
    case 8: case 9: { size_t own = 0, sh = 0; s->device_bytes(own, sh); *out = (double)(what == 8 ? own : sh); break; }
    default: throw std::invalid_argument("unknown info item");
  }
  API_END
}

int nnsdp_solver_run(nnsdp_solver* s, nnsdp_result* r) {
  API_BEGIN
  if (!s || !r) throw std::invalid_argument("null argument");
  int status = s->run_loop();
  s->finish(r, status);
  API_END
}

int nnsdp_solver_finish(nnsdp_solver* s, nnsdp_result* r) {
  API_BEGIN
  if (!s || !r) throw std::invalid_argument("null argument");
  int status = (s->last_pres <= s->opt.eps_rel && s->last_dres <= s->opt.eps_rel) ? NNSDP_STATUS_OPTIMAL : NNSDP_STATUS_ITERATION_LIMIT;
  s->finish(r, status);
  API_END
}

int nnsdp_solver_finish_status(nnsdp_solver* s, int32_t status, nnsdp_result* r) {
  API_BEGIN
  if (!s || !r) throw std::invalid_argument("null argument");
  if (status < NNSDP_STATUS_OPTIMAL || status > NNSDP_STATUS_TARGET_UNREACHABLE) throw std::invalid_argument("unrecognized status");
  s->finish(r, status);
  API_END
}

int nnsdp_solver_destroy(nnsdp_solver* s) {
  API_BEGIN
  delete s;
  API_END
}

int nnsdp_solve(const nnsdp_problem* p, const nnsdp_options* o, nnsdp_result* r) {
  API_BEGIN
  if (!p || !o || !r) throw std::invalid_argument("null argument");
  std::unique_ptr<nnsdp_solver> s(new nnsdp_solver());
  s->setup(p, o);
  int status = s->run_loop();
  s->finish(r, status);
  API_END
}

int nnsdp_assemble_Z(const nnsdp_problem* p, const double* gamma, double* Z) {
  API_BEGIN
  if (!p || !gamma || !Z) throw std::invalid_argument("null argument");
  require_gpu();
  FullOperator F;
  F.build(p);
  std::vector<double> g(gamma, gamma + F.P.ng);
  DBuf<double> Zd;
  F.assemble(g, Zd, nullptr);
  HIPCHK(hipMemcpy(Z, Zd.p, Zd.n * sizeof(double), hipMemcpyDeviceToHost));
  API_END
}

int nnsdp_adjoint(const nnsdp_problem* p, const double* X, double* out) {
  API_BEGIN
  if (!p || !X || !out) throw std::invalid_argument("null argument");
  require_gpu();
  FullOperator F;
  F.build(p);
  int n = F.P.Zdim, NE = F.S.NE, ng = F.S.ng;
  DBuf<double> Xd, xv, od;
  Xd.alloc((size_t)n * n);
  HIPCHK(hipMemcpy(Xd.p, X, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
  xv.alloc(NE);
  od.alloc(ng);
  hipLaunchKernelGGL(k_gather_dense, dim3(cdiv(NE, 256)), dim3(256), 0, nullptr, NE, n, F.D.erow.p, F.D.ecol.p, Xd.p, xv.p);
  hipLaunchKernelGGL(k_apply_At, dim3(cdiv((long long)ng * 64, kThreads)), dim3(kThreads), 0, nullptr, ng, F.D.csc_ptr.p, F.D.csc_row.p,
                     F.D.csc_val.p, xv.p, od.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> o = od.download();
  for (int g = 0; g < F.P.ng; ++g) out[g] = 0.0;
  for (int g = 0; g < ng; ++g) out[F.S.keep[g]] = o[g];
  API_END
}

int nnsdp_make_cliques(int32_t K, const int32_t* xdims, int32_t beta, int32_t mode, int32_t* n_cliques, int32_t* total,
                       int32_t* ptr, int32_t* idx) {
  API_BEGIN
  if (!xdims || K < 2) throw std::invalid_argument("bad xdims / K");
  if (beta < 0) throw std::invalid_argument("beta must be >= 0");
  if (mode < NNSDP_DECOMP_DENSE || mode > NNSDP_DECOMP_PATH) throw std::invalid_argument("unrecognized decomp_mode");
  auto cl = clique_index_sets(K, xdims, beta, mode);
  int tot = 0;
  for (auto& c : cl) tot += (int)c.size();
  if (n_cliques) *n_cliques = (int)cl.size();
  if (total) *total = tot;
  if (ptr && idx) {
    int o = 0;
    for (size_t k = 0; k < cl.size(); ++k) {
      ptr[k] = o;
      for (int v : cl[k]) idx[o++] = v;
    }
    ptr[cl.size()] = o;
  }
  API_END
}

// the options and outputs that the two _alpha entries add to their plain counterparts
struct AlphaReq {
  int32_t steps;
  double eta0, decay;
  const double* alpha0;
  double *a_smax, *a_uA, *a_ub0, *alpha;
  int32_t* best_step;
};
static int make_intervals_impl(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                         double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                         double* ymin, double* ymax, int32_t nlit = 0, const double* normals = nullptr, double* lit_smin = nullptr,
                         double* lit_smax = nullptr, double* uA = nullptr, double* ub0 = nullptr, const AlphaReq* ar = nullptr) {
  API_BEGIN
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  if (ar) {
    if (activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("optimised slopes (alpha) are for ReLU networks, not Tanh");
    if (nlit < 1) throw std::invalid_argument("optimised slopes (alpha) need literals: nlit must be in 1..64");
    check_pg_options("alpha", ar->steps, ar->eta0, ar->decay);
  }
  nnsdp::LitHead head;
  if (nlit != 0) {
    if (K < 2 || !xdims || !M) throw std::invalid_argument("make_intervals: bad arguments");
    for (int k = 0; k <= K; ++k)
      if (xdims[k] <= 0) throw std::invalid_argument("make_intervals: layer widths must be positive");
    check_literals(xdims[K], nlit, normals);
    head = nnsdp::make_lit_head(K, xdims, M, nlit, normals);
  }
  if (ar && ar->alpha0) {
    size_t acd = 0;
    for (int k = 1; k < K; ++k) acd += (size_t)xdims[k];
    check_alpha0(ar->alpha0, (size_t)nlit * acd);
  }
  nnsdp::IntervalsOut iv = nnsdp::make_intervals(K, xdims, M, x1min, x1max, activ == NNSDP_ACTIV_TANH, nlit > 0 ? &head : nullptr);
  for (int i = 0; i < nlit; ++i) {
    if (lit_smin) lit_smin[i] = iv.smin[i];
    if (lit_smax) lit_smax[i] = iv.smax[i];
    if (ub0) ub0[i] = iv.ub0[i];
  }
  if (uA && nlit > 0) std::copy(iv.uA.begin(), iv.uA.end(), uA);
  if (ar) {
    const nnsdp::AlphaOut ao = nnsdp::lits_alpha(K, xdims, M, head, iv.prel, iv.preu, x1min, x1max, ar->steps, ar->eta0, ar->decay, ar->alpha0);
    if (ar->a_smax) std::copy(ao.smax.begin(), ao.smax.end(), ar->a_smax);
    if (ar->a_uA) std::copy(ao.uA.begin(), ao.uA.end(), ar->a_uA);
    if (ar->a_ub0) std::copy(ao.ub0.begin(), ao.ub0.end(), ar->a_ub0);
    if (ar->alpha) std::copy(ao.alpha.begin(), ao.alpha.end(), ar->alpha);
    if (ar->best_step) std::copy(ao.best_step.begin(), ao.best_step.end(), ar->best_step);
  }
  const double eps = 1e-4;   // src/Qc/activ_sector.jl:65
  size_t o = 0;
  for (int k = 1; k < K; ++k)
    for (int i = 0; i < xdims[k]; ++i, ++o) {
      if (acymin) acymin[o] = iv.xlo[k][i];
      if (acymax) acymax[o] = iv.xhi[k][i];
      const double pl = iv.plo[k - 1][i], pu = iv.phi[k - 1][i];
      if (acxmin) acxmin[o] = pl;
      if (acxmax) acxmax[o] = pu;
      if (activ == NNSDP_ACTIV_RELU) {
        if (smin) smin[o] = pl > eps ? 1.0 : 0.0;
        if (smax) smax[o] = pu < -eps ? 0.0 : 1.0;
      } else {     // makeSectorMinMax, tanh branch (src/Qc/activ_sector.jl:74-86), including its 0/0 for a bound that is exactly 0
        const double tl = std::tanh(pl) / pl, tu = std::tanh(pu) / pu;
        const bool same = pl * pu >= 0.0;
        if (smin) smin[o] = same ? tu : std::min(tl, tu);
        if (smax) smax[o] = same ? tl : 1.0;
      }
    }
  for (int i = 0; i < xdims[K]; ++i) {
    if (ymin) ymin[i] = iv.xlo[K][i];
    if (ymax) ymax[i] = iv.xhi[K][i];
  }
  API_END
}

int nnsdp_make_intervals(int32_t K, const int32_t* xdims, const double* M, const double* x1min, const double* x1max,
                         double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                         double* ymin, double* ymax) {
  return make_intervals_impl(K, xdims, M, NNSDP_ACTIV_RELU, x1min, x1max, acymin, acymax, acxmin, acxmax, smin, smax, ymin, ymax);
}

int nnsdp_make_intervals_activ(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                               double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                               double* ymin, double* ymax) {
  return make_intervals_impl(K, xdims, M, activ, x1min, x1max, acymin, acymax, acxmin, acxmax, smin, smax, ymin, ymax);
}

int nnsdp_make_intervals_lits(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                              double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                              double* ymin, double* ymax, int32_t nlit, const double* normals, double* lit_smin, double* lit_smax,
                              double* uA, double* ub0) {
  return make_intervals_impl(K, xdims, M, activ, x1min, x1max, acymin, acymax, acxmin, acxmax, smin, smax, ymin, ymax, nlit, normals,
                             lit_smin, lit_smax, uA, ub0);
}

int nnsdp_make_intervals_lits_alpha(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min,
                                    const double* x1max, double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin,
                                    double* smax, double* ymin, double* ymax, int32_t nlit, const double* normals, double* lit_smin,
                                    double* lit_smax, double* uA, double* ub0, int32_t steps, double eta0, double decay,
                                    const double* alpha0, double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step) {
  const AlphaReq ar{steps, eta0, decay, alpha0, a_smax, a_uA, a_ub0, alpha, best_step};
  return make_intervals_impl(K, xdims, M, activ, x1min, x1max, acymin, acymax, acxmin, acxmax, smin, smax, ymin, ymax, nlit, normals,
                             lit_smin, lit_smax, uA, ub0, &ar);
}

int nnsdp_eval_network(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int64_t N, const double* X, double* Y,
                       double* kernel_ms) {
  API_BEGIN
  if (K < 1 || !xdims || !M) throw std::invalid_argument("null / empty network");
  if (N < 0) throw std::invalid_argument("N must be >= 0");
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  if (N == 0) return 0;
  if (!X || !Y) throw std::invalid_argument("null argument");
  require_gpu();
  for (int k = 0; k <= K; ++k)
    if (xdims[k] < 1) throw std::invalid_argument("layer widths must be >= 1");
  const nnsdp::NetLayout net(K, xdims);
  const size_t lds = nnsdp::fwd_lds_bytes(net.wp), nx = (size_t)net.n0() * N, nyN = (size_t)net.ny() * N;
  if (lds > 160 * 1024) throw std::invalid_argument("layer width above 639 is not supported by the sampled forward pass");
  if ((N + 15) / 16 > 0x7fffffffLL) throw std::invalid_argument("too many samples for one launch");
  DBuf<int> dxd; DBuf<long long> dmo; DBuf<double> dM, dX, dY;
  dxd.upload(net.xd); dmo.upload(net.moff);
  dM.alloc(net.mlen()); dX.alloc(nx); dY.alloc(nyN);
  HIPCHK(hipMemcpy(dM.p, M, net.mlen() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dX.p, X, nx * sizeof(double), hipMemcpyHostToDevice));
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nnsdp::k_forward_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EventPair ev;
  ev.create();
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  nnsdp::launch_forward(K, dxd.p, dmo.p, dM.p, dX.p, dY.p, N, activ, net.wp, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipEventSynchronize(ev.e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  HIPCHK(hipMemcpy(Y, dY.p, nyN * sizeof(double), hipMemcpyDeviceToHost));
  API_END
}

int nnsdp_make_intervals_batch(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nbox,
                               const double* x1min, const double* x1max,
                               double* acymin, double* acymax, double* acxmin, double* acxmax,
                               double* ymin, double* ymax, double* kernel_ms) {
  return nnsdp_make_intervals_batch_lits(K, xdims, M, activ, nbox, x1min, x1max, acymin, acymax, acxmin, acxmax, ymin, ymax, 0, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, kernel_ms);
}

int nnsdp_make_intervals_batch_lits(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nbox,
                                    const double* x1min, const double* x1max,
                                    double* acymin, double* acymax, double* acxmin, double* acxmax,
                                    double* ymin, double* ymax, int32_t nlit, const double* normals,
                                    double* smin, double* smax, double* uA, double* ub0, double* kernel_ms) {
  API_BEGIN
  if (K < 2 || !xdims || !M) throw std::invalid_argument("null / empty network (K >= 2 layers are needed)");
  if (activ == NNSDP_ACTIV_TANH) throw std::invalid_argument("Tanh networks are not supported by the batched intervals: use nnsdp_make_intervals_activ per box");
  if (activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("unknown activation");
  nnsdp_crown::check_widths(K, xdims);
  const nnsdp::NetLayout net(K, xdims);
  const int n0 = net.n0();
  check_literals(net.ny(), nlit, normals);
  if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
  if (nbox == 0) return 0;
  if (!x1min || !x1max) throw std::invalid_argument("null argument");
  nnsdp::check_boxes(nbox, n0, x1min, x1max);
  require_gpu();
  DBuf<int> dxd, dao; DBuf<long long> dmo; DBuf<double> dM, dlo, dhi, dscr, dout;
  dxd.upload(net.xd); dao.upload(net.acoff); dmo.upload(net.moff);
  const nnsdp::CrownLayout L{(size_t)nbox, (size_t)n0, (size_t)net.acdim(), (size_t)net.ny(), (size_t)nlit};
  dM.alloc(net.mlen() + net.head_len(nlit)); dlo.alloc(L.nbox * n0); dhi.alloc(L.nbox * n0); dscr.alloc(2 * L.na()); dout.alloc(L.total());
  nnsdp_crown::upload_network(dM.p, net, xdims, M, nlit, normals);
  HIPCHK(hipMemcpy(dlo.p, x1min, L.nbox * n0 * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dhi.p, x1max, L.nbox * n0 * sizeof(double), hipMemcpyHostToDevice));
  nnsdp::CrownArgs a;
  a.K = K; a.xdims = dxd.p; a.moff = dmo.p; a.acoff = dao.p; a.M = dM.p; a.H = dM.p + net.mlen();
  a.lo = dlo.p; a.hi = dhi.p; a.scratch = dscr.p;
  L.point(a, dout.p);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nnsdp::k_crown_batch), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)nnsdp::kCbLdsBytes));
  EventPair ev;
  ev.create();
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  hipLaunchKernelGGL(nnsdp::k_crown_batch, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytes, nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipEventSynchronize(ev.e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  // (pageable destinations, one copy per wanted segment: this entry keeps no pinned staging)
  double* const host[nnsdp::CrownLayout::kSegs] = {acymin, acymax, acxmin, acxmax, ymin, ymax, smin, smax, ub0, uA};
  size_t len[nnsdp::CrownLayout::kSegs];
  L.lens(len);
  const double* dev = dout.p;
  for (int o = 0; o < nnsdp::CrownLayout::kSegs; dev += len[o], ++o)
    if (host[o] && len[o]) HIPCHK(hipMemcpy(host[o], dev, len[o] * sizeof(double), hipMemcpyDeviceToHost));
  API_END
}

int nnsdp_crown_create(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nlit, const double* normals,
                       nnsdp_crown** out) {
  API_BEGIN
  if (!out) throw std::invalid_argument("null argument");
  *out = nullptr;
  if (K < 2 || !xdims || !M) throw std::invalid_argument("null / empty network (K >= 2 layers are needed)");
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  nnsdp_crown::check_widths(K, xdims);
  check_literals(xdims[K], nlit, normals);
  require_gpu();
  std::unique_ptr<nnsdp_crown> h(new nnsdp_crown);
  h->create(K, xdims, M, activ, nlit, normals);
  *out = h.release();
  API_END
}

int nnsdp_crown_create_wide(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nlit, const double* normals,
                            int32_t max_width, nnsdp_crown** out) {
  API_BEGIN
  if (!out) throw std::invalid_argument("null argument");
  *out = nullptr;
  if (K < 2 || !xdims || !M) throw std::invalid_argument("null / empty network (K >= 2 layers are needed)");
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  nnsdp_crown::check_widths_wide(K, xdims, max_width);
  check_literals(xdims[K], nlit, normals);
  require_gpu();
  std::unique_ptr<nnsdp_crown> h(new nnsdp_crown);
  h->create(K, xdims, M, activ, nlit, normals, max_width);
  *out = h.release();
  API_END
}

int nnsdp_crown_bound(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                      double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                      double* smin, double* smax, double* uA, double* ub0, double* kernel_ms) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  double* const host[nnsdp::CrownLayout::kSegs] = {acymin, acymax, acxmin, acxmax, ymin, ymax, smin, smax, ub0, uA};
  h->bound(nbox, x1min, x1max, host, kernel_ms);
  API_END
}

int nnsdp_crown_bound_alpha(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                            double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                            double* smin, double* smax, double* uA, double* ub0, double* kernel_ms,
                            int32_t steps, double eta0, double decay, const double* alpha0,
                            double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  double* const host[nnsdp::CrownLayout::kSegs] = {acymin, acymax, acxmin, acxmax, ymin, ymax, smin, smax, ub0, uA};
  h->bound_alpha(nbox, x1min, x1max, host, kernel_ms, steps, eta0, decay, alpha0, a_smax, a_uA, a_ub0, alpha, best_step);
  API_END
}

int nnsdp_crown_bound_nodes(nnsdp_crown* h, int32_t nnode, const double* x1min, const double* x1max, const int8_t* assign,
                            int32_t steps, double eta0, double decay, double* pre_lo, double* pre_hi, double* smin,
                            double* smax_plain, double* smax, double* uA, double* ub0, int32_t* best_step, int32_t* branch,
                            int32_t* infeasible, double* kernel_ms) {
  API_BEGIN
  const nnsdp_crown::NodeOut out{pre_lo, pre_hi, smin, smax_plain, smax, uA, ub0, best_step, branch, infeasible, kernel_ms};
  nnsdp_crown::bound_nodes(h, nnode, x1min, x1max, assign, steps, eta0, decay, out);
  API_END
}

int nnsdp_make_intervals_nodes(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min,
                               const double* x1max, const int8_t* assign, int32_t nlit, const double* normals, int32_t steps,
                               double eta0, double decay, double* pre_lo, double* pre_hi, double* smin, double* smax_plain,
                               double* smax, double* uA, double* ub0, int32_t* best_step, int32_t* branch, int32_t* infeasible) {
  API_BEGIN
  check_pg_options("nodes", steps, eta0, decay);
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  if (activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("a ReLU split is for ReLU networks, not Tanh");
  if (nlit < 1 || nlit > nnsdp::kCbW) throw std::invalid_argument("a ReLU split needs literals: nlit must be in 1..64, got " + std::to_string(nlit));
  if (K < 2 || !xdims || !M || !x1min || !x1max || !assign) throw std::invalid_argument("make_intervals_nodes: bad arguments");
  size_t acdim = 0;
  for (int k = 0; k <= K; ++k) {
    if (xdims[k] <= 0) throw std::invalid_argument("make_intervals_nodes: layer widths must be positive");
    if (k > 0 && k < K) acdim += (size_t)xdims[k];
  }
  check_literals(xdims[K], nlit, normals);
  nnsdp::check_boxes(1, xdims[0], x1min, x1max);
  check_assign(assign, acdim);
  const nnsdp::LitHead head = nnsdp::make_lit_head(K, xdims, M, nlit, normals);
  const nnsdp::NodeOut no = nnsdp::make_intervals_nodes(K, xdims, M, head, x1min, x1max, assign, steps, eta0, decay);
  auto put = [](const auto& v, auto* dst) { if (dst) std::copy(v.begin(), v.end(), dst); };
  put(no.pre_lo, pre_lo); put(no.pre_hi, pre_hi); put(no.smin, smin); put(no.smax_plain, smax_plain); put(no.smax, smax);
  put(no.uA, uA); put(no.ub0, ub0); put(no.best_step, best_step); put(no.branch, branch);
  if (infeasible) *infeasible = no.infeasible;
  API_END
}

int nnsdp_crown_eval(nnsdp_crown* h, int64_t N, const double* X, double* Y, double* kernel_ms) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  h->eval(N, X, Y, kernel_ms);
  API_END
}

int nnsdp_crown_search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                       int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                       nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                       int32_t* nleaves, double* witness, double* kernel_ms) {
  API_BEGIN
  nnsdp_crown::search(h, x1min, x1max, nlit, normals, hs, literal_bounds, corner_points, max_boxes, max_depth, chunk, confirm, user, verdict,
                      visited, depth_reached, nleaves, witness, kernel_ms);
  API_END
}

int nnsdp_crown_search_leaves(nnsdp_crown* h, double* lo, double* hi, int32_t* depth, int32_t* proved, int32_t* literal, double* bound) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  h->leaves.copy_out(lo, hi, depth, proved, literal, bound);
  API_END
}

int nnsdp_crown_search_many(nnsdp_crown* h, int32_t nroot, const double* x1min, const double* x1max, int32_t nlit, const double* normals,
                            const double* hs, int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth,
                            int32_t chunk, int32_t group, nnsdp_confirm_many_fn confirm, void* user, int32_t* verdict, int32_t* visited,
                            int32_t* depth_reached, int32_t* nleaves, double* witness, double* kernel_ms) {
  API_BEGIN
  nnsdp_crown::search_many(h, nroot, x1min, x1max, nlit, normals, hs, literal_bounds, corner_points, max_boxes, max_depth, chunk, group,
                           confirm, user, verdict, visited, depth_reached, nleaves, witness, kernel_ms);
  API_END
}

int nnsdp_crown_search_many_leaves(nnsdp_crown* h, int32_t root, double* lo, double* hi, int32_t* depth, int32_t* proved, int32_t* literal,
                                   double* bound) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  const int32_t nroot = (int32_t)h->fleaves.size();
  if (root < -1 || root >= nroot)
    throw std::invalid_argument("root must be -1 or in 0.." + std::to_string(nroot - 1) + " (the roots of the last search_many), got " + std::to_string(root));
  for (int32_t r = root < 0 ? 0 : root; r < (root < 0 ? nroot : root + 1); ++r) h->fleaves[(size_t)r].copy_out(lo, hi, depth, proved, literal, bound);
  API_END
}

int nnsdp_crown_forest_plan(int32_t n0, int32_t ny, int32_t nlit, int32_t max_boxes, int32_t corner_points, int32_t nroot, int32_t group,
                            int64_t* out) {
  API_BEGIN
  if (!out) throw std::invalid_argument("null argument");
  if (n0 < 1 || ny < 1 || nlit < 1) throw std::invalid_argument("n0, ny and nlit must be >= 1");
  if (max_boxes < 1) throw std::invalid_argument("max_boxes must be >= 1, got " + std::to_string(max_boxes));
  if (group < 0) throw std::invalid_argument("group must be >= 0 (0: derived from the memory cap), got " + std::to_string(group));
  if (nroot < 1) throw std::invalid_argument("nroot must be >= 1, got " + std::to_string(nroot));
  const nnsdp::ForestPlan P = nnsdp_crown::forest_group_plan(n0, ny, nlit, max_boxes, corner_points, nroot, group);
  out[0] = (int64_t)P.group; out[1] = (int64_t)P.cap; out[2] = (int64_t)P.frontier_bytes; out[3] = (int64_t)P.double_bytes; out[4] = (int64_t)P.int_bytes;
  API_END
}

int nnsdp_crown_reach(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* tol, int32_t corner_points,
                      int32_t max_boxes, int32_t max_depth, int32_t chunk, int32_t* status, int32_t* visited, int32_t* depth_reached,
                      int32_t* nleaves, double* incumbent, double* witnesses, double* kernel_ms) {
  API_BEGIN
  nnsdp_crown::reach(h, x1min, x1max, nlit, tol, corner_points, max_boxes, max_depth, chunk, status, visited, depth_reached, nleaves,
                     incumbent, witnesses, kernel_ms);
  API_END
}

int nnsdp_crown_reach_leaves(nnsdp_crown* h, double* lo, double* hi, int32_t* depth, int32_t* closed, double* bound) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  const nnsdp_crown::ReachLeaves& L = h->rleaves;
  if (!L.depth.empty() && (!lo || !hi || !depth || !closed || !bound)) throw std::invalid_argument("null argument");
  std::copy(L.lo.begin(), L.lo.end(), lo);
  std::copy(L.hi.begin(), L.hi.end(), hi);
  std::copy(L.depth.begin(), L.depth.end(), depth);
  std::copy(L.closed.begin(), L.closed.end(), closed);
  std::copy(L.bound.begin(), L.bound.end(), bound);
  API_END
}

int nnsdp_crown_search_nodes(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* hs, int32_t steps,
                             double eta0, double decay, int32_t corner_points, int32_t max_nodes, int32_t max_depth, int32_t chunk,
                             nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* reason, int32_t* visited, int32_t* depth_reached,
                             int32_t* nleaves, int32_t* nopen, double* witness, double* kernel_ms) {
  API_BEGIN
  nnsdp_crown::search_nodes(h, x1min, x1max, nlit, hs, steps, eta0, decay, corner_points, max_nodes, max_depth, chunk, confirm, user, verdict,
                            reason, visited, depth_reached, nleaves, nopen, witness, kernel_ms);
  API_END
}

int nnsdp_crown_search_nodes_leaves(nnsdp_crown* h, int8_t* assign, int32_t* depth, int32_t* closed_by, double* bound) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  const nnsdp_crown::NodeLeaves& L = h->nleaves_;
  if (!L.depth.empty() && (!assign || !depth || !closed_by || !bound)) throw std::invalid_argument("null argument");
  std::copy(L.assign.begin(), L.assign.end(), assign);
  std::copy(L.depth.begin(), L.depth.end(), depth);
  std::copy(L.closed_by.begin(), L.closed_by.end(), closed_by);
  std::copy(L.bound.begin(), L.bound.end(), bound);
  API_END
}

int nnsdp_crown_info(nnsdp_crown* h, int32_t what, double* out) {
  API_BEGIN
  if (!h || !out) throw std::invalid_argument("null argument");
  switch (what) {
    case 0: *out = (double)h->n_alloc; break;
    case 1: *out = (double)h->n_upload; break;
    case 2: *out = (double)h->box_cap; break;
    case 3: *out = (double)h->sample_cap; break;
    case 4: *out = (double)h->n_bound; break;
    case 5: *out = (double)h->device_bytes(); break;
    case 6: *out = (double)h->n_reach; break;
    case 7: *out = (double)h->max_width; break;
    case 8: *out = (double)h->n_node_search; break;
    case 9: *out = (double)h->n_node_levels; break;
    case 10: *out = (double)h->n_node_downloads; break;
    default: throw std::invalid_argument("nnsdp_crown_info: what must be in 0..10");
  }
  API_END
}

int nnsdp_crown_destroy(nnsdp_crown* h) {
  API_BEGIN
  delete h;
  API_END
}

int nnsdp_project_psd_batched(int32_t batch, const int32_t* n, const double* mats, double* out, double* eigvals, double* kernel_ms) {
  API_BEGIN
  if (batch < 0) throw std::invalid_argument("batch must be >= 0");
  if (batch == 0) return 0;
  if (!n || !mats || !out) throw std::invalid_argument("null argument");
  require_gpu();
  std::vector<int> cn(n, n + batch);
  std::vector<long long> coff(batch + 1), eoff(batch + 1);
  long long tot = 0, etot = 0;
  int nmax = 0;
  for (int b = 0; b < batch; ++b) {
    if (cn[b] < 1 || cn[b] > 4096) throw std::invalid_argument("matrix dimension must be in 1..4096");
    coff[b] = tot; eoff[b] = etot;
    tot += (long long)cn[b] * cn[b]; etot += cn[b];
    if (cn[b] <= nnsdp::kMaxLdsBlock) nmax = std::max(nmax, cn[b]);
  }
  coff[batch] = tot; eoff[batch] = etot;
  DBuf<int> dcn; DBuf<long long> dco, deo; DBuf<double> dnu, dw, dV, dE;
  dcn.upload(cn); dco.upload(coff); deo.upload(eoff);
  dnu.alloc(tot); dw.alloc(tot); dV.alloc(tot); dE.alloc(etot);
  HIPCHK(hipMemcpy(dnu.p, mats, tot * sizeof(double), hipMemcpyHostToDevice));
  nmax = std::max(nmax, 1);
  const ProjPlan plan = plan_projection(nmax);
  HIPCHK(proj_allow_big_lds(plan));
  ProjArgs a{};
  DBuf<double> dT;
  if (plan.packed()) dT.alloc(tot);       // the packed variant's sweeps log their rotations there
  a.cn = dcn.p; a.coff = dco.p; a.eoff = deo.p; a.nu = dnu.p; a.w = dw.p; a.Vg = dV.p; a.eig = dE.p; a.Tg = dT.p;
  a.kappa = nullptr; a.tol_dev = nullptr; a.stats = nullptr; a.warm = 0; a.max_sweeps = 30; a.tol = 1e-13;
  a.refine = 0; a.rstate = nullptr; a.refine_acc = 0.0; a.refine_kcap = 0.0; a.refine_loose = 1.0; a.refine_k2cap = 0.09; a.refine_pivots = 0;
  EventPair ev;
  ev.create();
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  {
    // matrices up to 128 through the LDS-resident Jacobi kernel (one launch), larger ones through the library path
    std::vector<int> cs, big;
    std::vector<long long> os, es;
    for (int b = 0; b < batch; ++b) {
      if (cn[b] <= nnsdp::kMaxLdsBlock) { cs.push_back(cn[b]); os.push_back(coff[b]); es.push_back(eoff[b]); }
      else big.push_back(b);
    }
    DBuf<int> dcs; DBuf<long long> dos, des;
    if (!big.empty() && !cs.empty()) { dcs.upload(cs); dos.upload(os); des.upload(es); a.cn = dcs.p; a.coff = dos.p; a.eoff = des.p; }
    if (!cs.empty()) launch_proj(plan, a, (int)cs.size(), nullptr);
    if (!big.empty()) {
      RocHandle rh;
      RBCHK(rocblas_set_stream(rh.h, nullptr));
      int nb = 0;
      for (int b : big) nb = std::max(nb, cn[b]);
      DBuf<double> A, T, Dv, Ev, scl; DBuf<rocblas_int> info;
      A.alloc((size_t)nb * nb); T.alloc((size_t)nb * nb); Dv.alloc(nb); Ev.alloc(nb); scl.alloc(2); info.alloc(big.size()); info.zero();
      for (size_t bi = 0; bi < big.size(); ++bi) {
        const int b = big[bi];
        project_big_block(rh.h, nullptr, cn[b], dnu.p + coff[b], dw.p + coff[b], A.p, T.p, Dv.p, Ev.p, info.p + bi, scl.p, dE.p + eoff[b]);
      }
      HIPCHK(hipDeviceSynchronize());
      for (rocblas_int v : info.download())
        if (v != 0) throw HipError("rocSOLVER dsyevd did not converge on a block above 128 (info = " + std::to_string((int)v) + ")");
    }
  }
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  HIPCHK(hipMemcpy(out, dw.p, tot * sizeof(double), hipMemcpyDeviceToHost));
  if (eigvals) HIPCHK(hipMemcpy(eigvals, dE.p, etot * sizeof(double), hipMemcpyDeviceToHost));
  API_END
}

int nnsdp_project_psd_warm(int32_t batch, const int32_t* n, const double* mats, double* basis, double tol, int32_t refine, double* out,
                           int32_t* outcome, double* kernel_ms) {
  return nnsdp_project_psd_warm_state(batch, n, mats, basis, tol, refine, out, outcome, kernel_ms, nullptr);
}

int nnsdp_project_psd_warm_state(int32_t batch, const int32_t* n, const double* mats, double* basis, double tol, int32_t refine, double* out,
                                 int32_t* outcome, double* kernel_ms, int32_t* state) {
  API_BEGIN
  if (batch < 0) throw std::invalid_argument("batch must be >= 0");
  if (batch == 0) return 0;
  if (!n || !mats || !basis || !out) throw std::invalid_argument("null argument");
  if (!(tol > 0.0)) throw std::invalid_argument("tol must be > 0");
  require_gpu();
  std::vector<int> cn(n, n + batch);
  std::vector<long long> coff(batch + 1);
  long long tot = 0;
  int nmax = 0;
  for (int b = 0; b < batch; ++b) {
    if (cn[b] < 1 || cn[b] > nnsdp::kMaxLdsBlock) throw std::invalid_argument("matrix dimension must be in 1..160 (the LDS-resident kernel)");
    coff[b] = tot;
    tot += (long long)cn[b] * cn[b];
    nmax = std::max(nmax, cn[b]);
  }
  coff[batch] = tot;
  DBuf<int> dcn, dst, drs; DBuf<long long> dco; DBuf<double> dnu, dw, dV, dT, dU;
  dcn.upload(cn); dco.upload(coff);
  // every matrix buffer carries a guard band behind its last block (64 doubles of a byte pattern, verified after the launch): an
  // index that runs past a block of the LAST matrix of a launch - the one overrun nothing else in a test would notice - fails the
  // call instead of corrupting a neighbour allocation (round 3's development fault on the first packed build, gpurun_out/
  // r03_call_q.txt, was never reproduced on a committed tree; this is the check that would have named the buffer)
  constexpr size_t kGuard = 64;
  DBuf<double>* guarded[] = {&dnu, &dw, &dV, &dT, &dU};
  for (DBuf<double>* bf : guarded) { bf->alloc(tot + kGuard); HIPCHK(hipMemset(bf->p + tot, 0xA5, kGuard * sizeof(double))); }
  dst.alloc(14); dst.zero(); drs.alloc(4 * (size_t)batch); drs.zero();
  if (state) HIPCHK(hipMemcpy(drs.p, state, 4 * (size_t)batch * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dnu.p, mats, tot * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dV.p, basis, tot * sizeof(double), hipMemcpyHostToDevice));
  // refine = 4: the tile-parallel pipeline (refine_pipe.hpp) in front of the kernel, as a solver runs it late in a solve; the kernel
  // behind it (refine = 1) takes the blocks the pipeline leaves
  const bool use_pipe = refine == 4;
  if (use_pipe) refine = 1;
  const ProjPlan plan = plan_projection(nmax, refine != 0);      // (97 .. 128 with the stage on: the packed variant, as in a solver's warm iterations)
  HIPCHK(proj_allow_big_lds(plan));
  nnsdp::RefinePipe pp;
  if (use_pipe) HIPCHK(pp.build(cn.data(), batch, tot));
  ProjArgs a{};
  a.cn = dcn.p; a.coff = dco.p; a.eoff = nullptr; a.nu = dnu.p; a.w = dw.p; a.Vg = dV.p; a.eig = nullptr; a.Tg = dT.p; a.Ug = dU.p;
  a.kappa = nullptr; a.tol_dev = nullptr; a.stats = dst.p; a.warm = 1; a.max_sweeps = 30; a.tol = tol;
  a.refine = refine; a.rstate = drs.p;
  RefineTuning::from_env().bind(a);
  SplitScratch split;
  // (test hook) NNSDP_SPLIT_WARM=<H>: H helper workgroups per block, as a solver's warm launches run
  if (plan.split_ok() && batch <= 120) {
    const int helpers = split_cap((int)env_int("NNSDP_SPLIT_WARM", 0), batch);
    if (helpers > 0) { split.alloc(batch, helpers); split.bind(a, batch); }
  }
  EventPair ev;
  ev.create();
  HIPCHK(hipEventRecord(ev.e0, nullptr));
#ifdef NNSDP_STAMPS
  DBuf<long long> ddbg;
  if (use_pipe && pp.ready) { ddbg.alloc(5 * (size_t)pp.nwg * 8); ddbg.zero(); }
#endif
  if (use_pipe && pp.ready) {
    nnsdp::PipeArgs pa = pp.args(a);
#ifdef NNSDP_STAMPS
    pa.dbg = ddbg.p;
#endif
    pp.launch(pa, nullptr); a.pmode = pp.pmode;
  }
  launch_proj(plan, a, batch, nullptr);
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  if (split.failed()) throw HipError("projection kernel, helper workgroup(s): a helper did not deliver its tiles in time");
  {
    std::vector<unsigned char> gb(kGuard * sizeof(double));
    const char* names[] = {"nu", "w", "V", "T scratch", "U scratch"};
    for (int q = 0; q < 5; ++q) {
      HIPCHK(hipMemcpy(gb.data(), guarded[q]->p + tot, gb.size(), hipMemcpyDeviceToHost));
      for (unsigned char c : gb)
        if (c != 0xA5) throw HipError(std::string("the projection kernel wrote past the end of the packed ") + names[q] + " buffer (guard band touched)");
    }
  }
#ifdef NNSDP_STAMPS
  if (use_pipe && pp.ready) {
    // (diagnostic build) wall-clock stamps (100 MHz) of thread 0 of every workgroup: spans and phase averages per kernel
    std::vector<long long> h = ddbg.download();
    const char* names[5] = {"T", "B", "X", "V", "W"};
    long long prev_end = 0;
    for (int kq = 0; kq < 5; ++kq) {
      long long lo = -1, hi = 0; double ph[4] = {0, 0, 0, 0}; int cnt = 0;
      for (int g = 0; g < pp.nwg; ++g) {
        const long long* d = &h[((size_t)kq * pp.nwg + g) * 8];
        if (d[0] == 0 || d[4] == 0 || d[3] == 0) continue;
        if (lo < 0 || d[0] < lo) lo = d[0];
        if (d[4] > hi) hi = d[4];
        for (int q = 0; q < 4; ++q) ph[q] += (double)(d[q + 1] - d[q]);
        ++cnt;
      }
      if (cnt == 0) continue;
      std::fprintf(stderr, "[stamps pipe %s] workgroups %d: first entry -> last exit %.2f us (gap to previous kernel's last exit %.2f us); thread 0: strips staged %.2f, barrier %.2f, chain %.2f, epilogue %.2f us\n",
                   names[kq], cnt, 0.01 * (hi - lo), prev_end ? 0.01 * (lo - prev_end) : 0.0, 0.01 * ph[0] / cnt, 0.01 * ph[1] / cnt, 0.01 * ph[2] / cnt, 0.01 * ph[3] / cnt);
      prev_end = hi;
      if (kq == 3) {
        double f[3] = {0, 0, 0}; int c2 = 0;
        for (int g = 0; g < pp.nwg; ++g) {
          const long long* d = &h[((size_t)kq * pp.nwg + g) * 8];
          if (d[0] == 0 || d[5] == 0 || d[6] == 0 || d[7] == 0) continue;
          f[0] += (double)(d[5] - d[0]); f[1] += (double)(d[6] - d[5]); f[2] += (double)(d[7] - d[6]); ++c2;
        }
        if (c2) std::fprintf(stderr, "[stamps pipe V, inside 'strips staged'] block size known (scalar loads) %.2f, all vector loads issued +%.2f, landed +%.2f us\n", 0.01 * f[0] / c2, 0.01 * f[1] / c2, 0.01 * f[2] / c2);
      }
    }
  }
#endif
  HIPCHK(hipMemcpy(out, dw.p, tot * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(basis, dV.p, tot * sizeof(double), hipMemcpyDeviceToHost));
  if (state) HIPCHK(hipMemcpy(state, drs.p, 4 * (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
  if (outcome) { std::vector<int> st = dst.download(); for (int i = 0; i < 5; ++i) outcome[i] = st[4 + i]; }
  API_END
}

int nnsdp_batch_create(nnsdp_solver** solvers, int32_t count, nnsdp_batch** out) {
  API_BEGIN
  if (!out) throw std::invalid_argument("null argument");
  require_gpu();
  std::unique_ptr<nnsdp_batch> b(new nnsdp_batch());
  b->create(solvers, count);
  *out = b.release();
  API_END
}

int nnsdp_batch_iterate(nnsdp_batch* b, int32_t iters) {
  API_BEGIN
  if (!b) throw std::invalid_argument("null batch");
  if (iters < 0) throw std::invalid_argument("iters must be >= 0");
  b->iterate(iters);
  API_END
}

int nnsdp_batch_run(nnsdp_batch* b, int32_t* status) {
  API_BEGIN
  if (!b) throw std::invalid_argument("null batch");
  b->run();
  if (status) for (size_t i = 0; i < b->all.size(); ++i) status[i] = b->status[i];
  API_END
}

int nnsdp_batch_info(nnsdp_batch* b, int32_t what, double* out) {
  API_BEGIN
  if (!b || !out) throw std::invalid_argument("null argument");
  switch (what) {
    case 0: *out = (double)b->act.size(); break;
    case 1: *out = (double)b->n_fgroups; break;
    case 2: *out = (double)b->n_fmembers; break;
    case 3: *out = (double)b->n_sgroups; break;
    case 4: *out = (double)b->n_smembers; break;
    default: throw std::invalid_argument("unknown info item");
  }
  API_END
}

int nnsdp_batch_resync(nnsdp_batch* b) {
  API_BEGIN
  if (!b) throw std::invalid_argument("null batch");
  b->rebuild();
  API_END
}

int nnsdp_batch_destroy(nnsdp_batch* b) {
  API_BEGIN
  delete b;
  API_END
}

int nnsdp_comm_unique_id(char* id128) {
  API_BEGIN
  if (!id128) throw std::invalid_argument("null argument");
  require_gpu();
  Rccl& R = Rccl::get();
  Rccl::UniqueId uid;
  R.check(R.GetUniqueId(&uid), "ncclGetUniqueId");
  std::memcpy(id128, uid.internal, 128);
  API_END
}

int nnsdp_shard_plan(const nnsdp_problem* p, const nnsdp_options* o, int32_t nranks, int32_t* n_blocks, int32_t* block_n,
                     int32_t* start) {
  API_BEGIN
  if (!p || !o || !n_blocks) throw std::invalid_argument("null argument");
  if (nranks < 1) throw std::invalid_argument("nranks must be >= 1");
  if (o->decomp_mode < NNSDP_DECOMP_DENSE || o->decomp_mode > NNSDP_DECOMP_AUTO) throw std::invalid_argument("unrecognized decomp_mode");
  ProblemCopy P;
  P.load(p);
  Congruence C = make_congruence(P, o->normalize != 0, o->interval_guard);
  int mode = o->decomp_mode;
  if (mode == NNSDP_DECOMP_AUTO) {      // (the solver's own rule: the path cliques when the generator table fits their pattern)
    mode = NNSDP_DECOMP_PATH;
    try {
      auto clp = reduced_cliques(P, C, mode);
      Pattern ptp = build_pattern(C.nred, clp);
      (void)OperatorBuilder(P, C, ptp).build();
    } catch (const std::runtime_error&) { mode = NNSDP_DECOMP_DOUBLE; }
  }
  auto cl = reduced_cliques(P, C, mode);
  *n_blocks = (int32_t)cl.size();
  if (block_n || start) {
    std::vector<int> cn(cl.size());
    for (size_t k = 0; k < cl.size(); ++k) cn[k] = (int)cl[k].size();
    if (block_n) for (size_t k = 0; k < cn.size(); ++k) block_n[k] = cn[k];
    if (start) { auto st = shard_ranges(cn, nranks); for (int r = 0; r <= nranks; ++r) start[r] = st[r]; }
  }
  API_END
}

int nnsdp_solver_set_target(nnsdp_solver* s, int32_t mode, double target) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  s->set_target(mode, target);
  API_END
}

int nnsdp_solver_certified_bound(nnsdp_solver* s, double* objective, double* gamma, int32_t* certified, double* ms) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (s->sharded) throw std::invalid_argument("a clique-sharded solver has no sparse bound");
  s->certified_bound(objective, gamma, certified, ms);
  API_END
}

int nnsdp_cert_plan(const nnsdp_problem* p, const nnsdp_options* o, int32_t* n, int32_t* n_super, int32_t* max_front, int64_t* fill,
                    int32_t* supported, int32_t* col_start, int32_t* row_ptr, int32_t* row_idx) {
  API_BEGIN
  if (!p || !o) throw std::invalid_argument("null argument");
  if (o->decomp_mode < NNSDP_DECOMP_DENSE || o->decomp_mode > NNSDP_DECOMP_AUTO) throw std::invalid_argument("unrecognized decomp_mode");
  ProblemCopy P;
  P.load(p);
  Congruence C = make_congruence(P, o->normalize != 0, o->interval_guard);
  const CertPlan pl = make_cert_plan(solver_pattern(P, C, o->decomp_mode));
  if (n) *n = pl.n;
  if (n_super) *n_super = pl.n_super;
  if (max_front) *max_front = pl.max_front;
  if (fill) *fill = pl.fill;
  if (supported) *supported = pl.supported ? 1 : 0;
  if (col_start) std::copy(pl.col_start.begin(), pl.col_start.end(), col_start);
  if (row_ptr) std::copy(pl.row_ptr.begin(), pl.row_ptr.end(), row_ptr);
  if (row_idx) std::copy(pl.row_idx.begin(), pl.row_idx.end(), row_idx);
  API_END
}

int nnsdp_sparse_nsd(int32_t n, int32_t n_cliques, const int32_t* ptr, const int32_t* idx, int32_t batch, const double* mats, int32_t* ok,
                     double* min_pivot, double* schur, double* kernel_ms) {
  API_BEGIN
  if (n < 1 || n_cliques < 1 || !ptr || !idx) throw std::invalid_argument("null / empty pattern");
  if (batch < 0) throw std::invalid_argument("batch must be >= 0");
  if (batch == 0) return 0;
  if (!mats || !ok) throw std::invalid_argument("null argument");
  std::vector<std::vector<int>> cl(n_cliques);
  for (int k = 0; k < n_cliques; ++k) {
    if (ptr[k + 1] < ptr[k]) throw std::invalid_argument("clique pointers must be nondecreasing");
    for (int q = ptr[k]; q < ptr[k + 1]; ++q) {
      if (idx[q] < 0 || idx[q] >= n) throw std::invalid_argument("clique index out of range");
      cl[k].push_back(idx[q]);
    }
  }
  const Pattern pat = build_pattern(n, cl);
  if (pat.pos(n - 1, n - 1) < 0) throw std::invalid_argument("the affine index n - 1 must lie in some clique");
  const size_t nn = (size_t)n * n;
  std::vector<double> z((size_t)batch * pat.NE);
  for (int b = 0; b < batch; ++b) {
    const double* M = mats + b * nn;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const int e = pat.pos(i, j);
        if (e < 0) {
          if (M[(size_t)j * n + i] != 0.0) throw std::invalid_argument("matrix " + std::to_string(b) + " has a non-zero entry outside the clique pattern");
        } else if (i >= j) z[(size_t)b * pat.NE + e] = i == j ? M[(size_t)j * n + i] : M[(size_t)j * n + i] * M_SQRT2;
      }
  }
  CertPlan pl = make_cert_plan(pat);
  if (!pl.supported) {
    g_err = "sparse NSD check: largest front " + std::to_string(pl.max_front) + " exceeds " + std::to_string(kCertFrontMax);
    return -2;
  }
  require_gpu();
  CertDev cd;
  cd.upload(std::move(pl));
  DBuf<double> dz;
  dz.upload(z);
  EventPair ev;
  ev.create();
  cd.reserve(batch);
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  cd.launch(dz.p, pat.NE, batch, nullptr);
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipDeviceSynchronize());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  HIPCHK(hipMemcpy(ok, cd.ok.p, batch * sizeof(int), hipMemcpyDeviceToHost));
  if (min_pivot) HIPCHK(hipMemcpy(min_pivot, cd.minp.p, batch * sizeof(double), hipMemcpyDeviceToHost));
  if (schur) HIPCHK(hipMemcpy(schur, cd.schur.p, batch * sizeof(double), hipMemcpyDeviceToHost));
  if (schur) {      // a candidate that failed has no Schur complement: its slot reports the first failing column instead
    const std::vector<int> fc = cd.fail.download();
    for (int b = 0; b < batch; ++b) if (!ok[b]) schur[b] = (double)fc[b];
  }
  API_END
}

int nnsdp_solver_set_comm(nnsdp_solver* s, int32_t nranks, int32_t rank, const char* id128) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  s->set_comm(nranks, rank, id128);
  API_END
}

int nnsdp_solver_set_comm_callback(nnsdp_solver* s, int32_t nranks, int32_t rank, nnsdp_allreduce_fn fn, void* user) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (!fn) throw std::invalid_argument("null all-reduce callback");
  s->set_comm(nranks, rank, nullptr, fn, user);
  API_END
}

int nnsdp_solver_set_comm_ipc(nnsdp_solver* s, int32_t nranks, int32_t rank, nnsdp_allreduce_fn fn, void* user) {
  API_BEGIN
  if (!s) throw std::invalid_argument("null solver");
  if (!fn) throw std::invalid_argument("null all-reduce callback");
  s->set_comm(nranks, rank, nullptr, fn, user, true);
  API_END
}

}  // extern "C"
