// C ABI of libnnsdp_hip.so (include/nnsdp.h): host orchestration of the HIP kernels.
// One ADMM iteration = 6 kernels on one stream; `check_every` iterations are captured into a
// hipGraph and replayed, so the host only touches the device once per convergence check.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../include/nnsdp.h"
#include "kernels.hip"
#include "refine_pipe.hpp"
#include "setup.hpp"
#include "cert_plan.hpp"
#include "minv.hpp"
#include "intervals.hpp"
#include "forward.hpp"
#include "crown_batch.hpp"
#include "crown_alpha.hpp"
#include "crown_search.hpp"

namespace nnsdp {

thread_local std::string g_err;

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess)                                                                           \
      throw HipError(std::string(#x) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" +    \
                     std::to_string(__LINE__) + ")");                                               \
  } while (0)
#define RBCHK(x)                                                                                    \
  do {                                                                                              \
    rocblas_status s_ = (x);                                                                        \
    if (s_ != rocblas_status_success)                                                               \
      throw HipError(std::string(#x) + " failed: rocblas_status " + std::to_string((int)s_));       \
  } while (0)

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  // the allocation is reference-counted: the members of a solver family (nnsdp_solver_create_sibling) hold the same set-up
  // buffers, and the last holder frees them
  std::shared_ptr<void> own;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  void release() { own.reset(); p = nullptr; }
  void adopt(void* q) { own = std::shared_ptr<void>(q, [](void* x) { (void)hipFree(x); }); p = static_cast<T*>(q); }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) { void* q = nullptr; HIPCHK(hipMalloc(&q, count * sizeof(T))); adopt(q); }
  }
  // a second holder of o's allocation (read-only use)
  void share(const DBuf& o) { own = o.own; p = o.p; n = o.n; }
  size_t bytes() const { return p ? n * sizeof(T) : 0; }
  bool shared() const { return own && own.use_count() > 1; }
  // fine-grained device memory: coherent across devices WHILE kernels run (the hipIpc exchange buffers: a peer's kernel polls a flag
  // and reads data another device's kernel is publishing; coarse-grained memory only promises that at kernel boundaries)
  bool alloc_finegrained(size_t count) {
    release();
    n = count;
    void* q = nullptr;
    if (hipExtMallocWithFlags(&q, count * sizeof(T), hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); n = 0; return false; }
    adopt(q);
    return true;
  }
  void upload(const std::vector<T>& h) {
    alloc(h.size());
    if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  void zero() { if (n) HIPCHK(hipMemset(p, 0, n * sizeof(T))); }
  std::vector<T> download() const {
    std::vector<T> h(n);
    if (n) HIPCHK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

static void require_gpu() {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    throw HipError("no HIP device available: libnnsdp_hip has no CPU fallback (the product path is GPU-only)");
}

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// tuning of the projection kernel's refinement stage (ProjArgs::refine_*, gram_credit), with the diagnostic environment overrides applied:
// read once per solver and once per warm test-entry call
struct RefineTuning {
  double acc = 30.0, kcap = 0.05, loose = 1.0;
  // |K|_F^2 above which the refinement step is not taken (NNSDP_REFINE_KMAX overrides |K|_F).  Round 3 had 0.09 (|K|_F <= 0.3, from the
  // Frobenius bound |K|^4 / 4 on the defect of I + K + K^2 / 2); that bound is 50x pessimistic on these blocks (a step with |K|_F = 0.28
  // leaves |I - V'V|_F = 2.7e-5), the 151-wide blocks of width-50 networks sit at |K|_F = 0.35 .. 0.45 with a predicted error INSIDE the
  // accepted level for thousands of iterations, and one such block in back-off makes every launch a sweep launch: 0.64 takes the
  // ACAS-shaped Single solve from 13.3 to 8.3 s (28.0 -> 15.1 s on bench.py's network) and leaves W40-D20 unchanged; the measured
  // defect (Gram visits, forced by the estimate) and the r2 <= 1e-4 guard stay in charge of orthogonality.
  double k2cap = 0.64;
  int pivots = 2, gram_credit = 3;
  static RefineTuning from_env() {
    RefineTuning t;
    if (const char* e = std::getenv("NNSDP_REFINE_ACC")) t.acc = std::atof(e);
    if (const char* e = std::getenv("NNSDP_REFINE_KCAP")) t.kcap = std::atof(e);
    if (const char* e = std::getenv("NNSDP_REFINE_LOOSE")) t.loose = std::atof(e);
    if (const char* e = std::getenv("NNSDP_REFINE_KMAX")) t.k2cap = std::atof(e) * std::atof(e);
    if (const char* e = std::getenv("NNSDP_REFINE_PIVOTS")) t.pivots = std::atoi(e);
    if (const char* e = std::getenv("NNSDP_GRAM_EVERY")) t.gram_credit = std::min(std::max(std::atoi(e) - 1, 0), 15);
    return t;
  }
  void bind(ProjArgs& a) const {
    a.refine_acc = acc; a.refine_kcap = kcap; a.refine_loose = loose; a.refine_k2cap = k2cap; a.refine_pivots = pivots; a.gram_credit = gram_credit;
  }
};

// scratch of two workgroups per block for the warm-start congruence (ProjArgs::split): helper tiles, hand-over counters, error flag
struct SplitScratch {
  DBuf<double> B;
  DBuf<unsigned> ack, seen, xcc;
  DBuf<int> err;
  bool on() const { return B.p != nullptr; }
  void alloc(int nblk) {
    B.alloc((size_t)nblk * kSplitTileDoubles);
    ack.alloc(nblk); ack.zero(); seen.alloc(nblk); seen.zero(); xcc.alloc(nblk); xcc.zero(); err.alloc(1); err.zero();
  }
  void bind(ProjArgs& a, int nblk) const {
    a.split = 1; a.nblk = nblk; a.sB = B.p; a.sack = ack.p; a.sseen = seen.p; a.sxcc = xcc.p; a.serr = err.p; a.spin_limit = 20000000;
  }
  bool failed() const { return on() && err.download()[0] != 0; }
};

// device-resident operator (CSR + CSC + pattern)
struct DevOperator {
  int NE = 0, ng = 0, n = 0;
  DBuf<int> csr_ptr, csr_col, csc_ptr, csc_row, erow, ecol;
  DBuf<double> csr_val, csc_val, z0, c, Dinv;
  void upload(const ScaledOperator& S, const Pattern& pat) {
    NE = S.NE; ng = S.ng; n = pat.n;
    csr_ptr.upload(S.csr_ptr); csr_col.upload(S.csr_col); csr_val.upload(S.csr_val);
    csc_ptr.upload(S.csc_ptr); csc_row.upload(S.csc_row); csc_val.upload(S.csc_val);
    z0.upload(S.z0); c.upload(S.c); Dinv.upload(S.Dinv);
    erow.upload(pat.erow); ecol.upload(pat.ecol);
  }
};

// reference-coordinates operator (dense pattern) for nnsdp_assemble_Z / nnsdp_adjoint / final Z
struct FullOperator {
  ProblemCopy P;
  Pattern pat;
  ScaledOperator S;
  DevOperator D;
  void build(const nnsdp_problem* p) {
    P.load(p);
    build_host();
    upload();
  }
  // the two halves apart: the host half (pure host code on this object's own copy of the problem) may run on another thread
  // while the solver iterates, the upload is the caller's
  void build_host() {
    Congruence C = make_congruence(P, false);
    pat = build_pattern(P.Zdim, {}, true);
    Operator op = OperatorBuilder(P, C, pat).build();
    S = scale_operator(op, false);
    pat = std::move(op.pat);
  }
  void upload() { D.upload(S, pat); }
  // Z (device, Zdim x Zdim column-major) from a full-length gamma (host)
  void assemble(const std::vector<double>& gamma_full, DBuf<double>& Zd, hipStream_t st) {
    std::vector<double> gk(S.ng);
    for (int g = 0; g < S.ng; ++g) gk[g] = gamma_full[S.keep[g]];
    DBuf<double> gd, zd;
    gd.upload(gk);
    zd.alloc(S.NE);
    if (Zd.n != (size_t)P.Zdim * P.Zdim) Zd.alloc((size_t)P.Zdim * P.Zdim);
    HIPCHK(hipMemsetAsync(Zd.p, 0, Zd.n * sizeof(double), st));
    hipLaunchKernelGGL(k_apply_A, dim3(cdiv((long long)S.NE * 16, kThreads)), dim3(kThreads), 0, st, S.NE, D.csr_ptr.p,
                       D.csr_col.p, D.csr_val.p, gd.p, D.z0.p, zd.p);
    hipLaunchKernelGGL(k_scatter_dense, dim3(cdiv(S.NE, 256)), dim3(256), 0, st, S.NE, P.Zdim, D.erow.p, D.ecol.p, zd.p, Zd.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
  }
};

// RCCL is loaded lazily (dlopen) and only in clique-sharded mode, so the default single-GPU / replica paths
// never touch it.  Minimal declarations matching /opt/rocm/include/rccl/rccl.h.
struct Rccl {
  struct UniqueId { char internal[128]; };
  typedef void* Comm;
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(Comm*, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, Comm, hipStream_t) = nullptr;
  int (*CommDestroy)(Comm) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  static constexpr int kFloat64 = 8, kSum = 0;
  static Rccl& get() {
    static Rccl r;
    if (!r.GetUniqueId) {
      void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
      if (!h) throw HipError(std::string("cannot load RCCL: ") + dlerror());
      auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) throw HipError(std::string("RCCL symbol missing: ") + n); return p; };
      r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
      r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
      r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
      r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
      r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    }
    return r;
  }
  void check(int rc, const char* what) {
    if (rc != 0) throw HipError(std::string(what) + " failed: " + (GetErrorString ? GetErrorString(rc) : "?"));
  }
};

struct RocHandle {
  rocblas_handle h = nullptr;
  RocHandle() {
    RBCHK(rocblas_create_handle(&h));
    // reproducible library results: no atomics-based (split-K) accumulation inside rocBLAS / rocSOLVER.  M^-1, the certificate
    // polish and the eigmax check are then the same bits run to run and rank to rank on one GPU model
    RBCHK(rocblas_set_atomics_mode(h, rocblas_atomics_not_allowed));
  }
  ~RocHandle() { if (h) rocblas_destroy_handle(h); }
};

static double lambda_max_dense(rocblas_handle h, const DBuf<double>& Zd, int n, double* lambda_min = nullptr) {
  DBuf<double> A, D, E;
  DBuf<rocblas_int> info;
  A.alloc((size_t)n * n); D.alloc(n); E.alloc(n); info.alloc(1);
  HIPCHK(hipMemcpy(A.p, Zd.p, (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice));
  RBCHK(rocsolver_dsyevd(h, rocblas_evect_none, rocblas_fill_lower, n, A.p, n, D.p, E.p, info.p));
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> d = D.download();
  if (lambda_min) *lambda_min = d.front();
  return d.back();
}

// ---- PSD blocks above 128 (library path: rocSOLVER dsyevd + rocBLAS dgemm, one block at a time) --------------------
// The library eigensolver has no scaling of its own: on a block of entries around 1e-150 dsyevd returned finite eigenvalues that were
// wrong by more than |A| (tests/test_projection_hard_cases.py, the library launches).  A block whose largest entry lies outside
// [2^-64, 2^64] is therefore solved as f A with the power of two f that brings the entry into [1, 2) - exact - and the eigenvalues are
// scaled back; every other block (a solver's normalised blocks) keeps f = 1 and its bits.  scl[0] = f, scl[1] = 1 / f.  One workgroup.
__global__ __launch_bounds__(1024) void k_big_absmax(long long n2, const double* __restrict__ nu, double* __restrict__ scl) {
  __shared__ double part[16];
  double v = 0.0;
  for (long long i = threadIdx.x; i < n2; i += 1024) v = fmax(v, fabs(nu[i]));
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 16; ++q) v = fmax(v, part[q]);
    const int e = (int)((__double_as_longlong(v) >> 52) & 0x7ff) - 1023;      // (-1023: zero or subnormal, 1024: infinity)
    const bool keep = v == 0.0 || e == 1024 || (e >= -64 && e <= 64);
    scl[0] = keep ? 1.0 : ldexp(1.0, -e);
    scl[1] = keep ? 1.0 : ldexp(1.0, e);
  }
}
// A = f sym(nu_k)
__global__ void k_big_sym(int n, const double* __restrict__ nu, double* __restrict__ A, const double* __restrict__ scl) {
  int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  const double f = scl[0];
  if (i < n) A[(size_t)j * n + i] = 0.5 * (f * nu[(size_t)j * n + i] + f * nu[(size_t)i * n + j]);
}
// T[:, j] = V[:, j] * max(lam_j, 0) / f
__global__ void k_big_scale(int n, const double* __restrict__ V, const double* __restrict__ lam, double* __restrict__ T, const double* __restrict__ scl) {
  int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < n) { double l = lam[j] * scl[1]; T[(size_t)j * n + i] = l > 0.0 ? l * V[(size_t)j * n + i] : 0.0; }
}
// eigenvalues of the block itself: lam / f
__global__ void k_big_eig(int n, const double* __restrict__ lam, const double* __restrict__ scl, double* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = lam[i] * scl[1];
}
// nu <- w + kappa (nu - w)   (penalty change, as the LDS kernel does for its blocks)
__global__ void k_big_rescale(long long n2, const double* __restrict__ w, double* __restrict__ nu, const double* __restrict__ kappa) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double kap = *kappa;
  if (i < n2 && kap != 1.0) { double wv = w[i]; nu[i] = wv + kap * (nu[i] - wv); }
}

// the library eigensolver's convergence report, made sticky: a failure of ANY call since the solver was created stays visible
// (big_info[slot] itself is overwritten by the next call of that slot)
__global__ void k_sticky_info(const rocblas_int* __restrict__ info, int* __restrict__ flag) { if (*info != 0) *flag = 1; }
// acc[7] (the control block's flag word: time limit of any rank in its low part) += 1024 when the sticky failure flag is set, so that
// the flag travels through the check iteration's all-reduce and every rank takes the NUMERICAL_ERROR exit together
__global__ void k_fold_flag(const int* __restrict__ flag, double* __restrict__ acc7) { if (*flag != 0) *acc7 += 1024.0; }

// w_k = proj_PSD(sym(nu_k)) for one block of any size through rocSOLVER dsyevd + rocBLAS dgemm, all on the handle's stream
// (scl: two doubles of device scratch for the block's scale factor, see k_big_absmax)
static void project_big_block(rocblas_handle h, hipStream_t st, int n, const double* nuk, double* wk, double* A, double* T, double* Dv,
                              double* Ev, rocblas_int* info, double* scl, double* eig_out = nullptr) {
  hipLaunchKernelGGL(k_big_absmax, dim3(1), dim3(1024), 0, st, (long long)n * n, nuk, scl);
  hipLaunchKernelGGL(k_big_sym, dim3((n + 255) / 256, n), dim3(256), 0, st, n, nuk, A, scl);
  RBCHK(rocsolver_dsyevd(h, rocblas_evect_original, rocblas_fill_lower, n, A, n, Dv, Ev, info));
  hipLaunchKernelGGL(k_big_scale, dim3((n + 255) / 256, n), dim3(256), 0, st, n, A, Dv, T, scl);
  const double one = 1.0, zero = 0.0;
  RBCHK(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_transpose, n, n, n, &one, T, n, A, n, &zero, wk, n));
  if (eig_out) hipLaunchKernelGGL(k_big_eig, dim3((n + 255) / 256), dim3(256), 0, st, n, Dv, scl, eig_out);
}

__global__ void k_symmetrize_lower(int n, int ld, double* A) {
  int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < n && i > j) A[(size_t)i * ld + j] = A[(size_t)j * ld + i];  // copy lower (col j,row i) to upper
}

}  // namespace nnsdp

using namespace nnsdp;

// PSD blocks the solver works on: the reference's index sets (makeCliques / setupZs!) mapped through the normalisation
// (eliminated coordinates dropped), identical sets merged - a sum of NSD matrices on one index set is NSD, so one block
// per distinct set is an equivalent feasible set.  Host only.
static std::vector<std::vector<int>> reduced_cliques(const ProblemCopy& P, const Congruence& C, int decomp_mode) {
  auto cl_full = clique_index_sets(P.K, P.xdims.data(), P.beta, decomp_mode);
  std::vector<std::vector<int>> cl;
  for (auto& cq : cl_full) {
    std::vector<int> r;
    for (int i : cq)
      if (C.newpos[i] >= 0) r.push_back(C.newpos[i]);
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
    if (std::find(cl.begin(), cl.end(), r) == cl.end()) cl.push_back(r);
  }
  return cl;
}

// clique-sharded mode: contiguous block ranges per rank, balanced by n_k^3 (blocks k, k+1 overlap, so neighbours stay
// on one rank); start has nranks + 1 entries, rank r owns blocks [start[r], start[r+1]).  Host only.
static std::vector<int> shard_ranges(const std::vector<int>& cn, int nr) {
  // linear partition: contiguous ranges minimising the heaviest rank's sum of n_k^3 (the iteration's critical path is
  // the slowest rank's projection launch); exact dynamic programme, ncl and nr are tiny
  const int ncl = (int)cn.size();
  std::vector<double> pre(ncl + 1, 0.0);
  for (int k = 0; k < ncl; ++k) pre[k + 1] = pre[k] + (double)cn[k] * cn[k] * cn[k];
  const int parts = std::min(nr, std::max(ncl, 1));
  const double inf = 1e300;
  // best[r][k]: minimal bottleneck of the first k blocks in r non-empty ranges
  std::vector<std::vector<double>> best(parts + 1, std::vector<double>(ncl + 1, inf));
  std::vector<std::vector<int>> cut(parts + 1, std::vector<int>(ncl + 1, 0));
  best[0][0] = 0.0;
  for (int r = 1; r <= parts; ++r)
    for (int k = r; k <= ncl; ++k)
      for (int j = r - 1; j < k; ++j) {
        double v = std::max(best[r - 1][j], pre[k] - pre[j]);
        if (v < best[r][k]) { best[r][k] = v; cut[r][k] = j; }
      }
  std::vector<int> start(nr + 1, ncl);
  int k = ncl;
  for (int r = parts; r >= 1; --r) { k = (ncl > 0) ? cut[r][k] : 0; start[r - 1] = k; }
  start[0] = 0;
  for (int r = parts; r <= nr; ++r) start[r] = ncl;     // more ranks than blocks: the surplus ranks own nothing
  return start;
}

// the pattern a solver for (problem, options) works on: its reduced cliques, NNSDP_DECOMP_AUTO resolved by the solver's own rule.  Host only.
static Pattern solver_pattern(const ProblemCopy& P, const Congruence& C, int mode) {
  if (mode == NNSDP_DECOMP_AUTO) {
    mode = NNSDP_DECOMP_PATH;
    try {
      Pattern ptp = build_pattern(C.nred, reduced_cliques(P, C, mode));
      (void)OperatorBuilder(P, C, ptp).build();
    } catch (const std::runtime_error&) { mode = NNSDP_DECOMP_DOUBLE; }
  }
  return build_pattern(C.nred, reduced_cliques(P, C, mode));
}

// Device half of the sparse NSD check (cert_plan.hpp / cert_chol.hpp): the plan's tables, the per-candidate scratch and results.
struct CertDev {
  CertPlan pl;
  DBuf<int> col_start, row_ptr, rel, child_ptr, child_idx, roots, gat_ptr, gat_pos, gat_ent, ok, fail;
  DBuf<long long> upd_off;
  DBuf<double> scratch, minp, schur;
  int cap = 0;
  static constexpr double kPivotFloor = 1e-13;
  void upload(CertPlan&& plan) {
    pl = std::move(plan);
    if (!pl.supported) throw std::invalid_argument("sparse NSD check: largest front " + std::to_string(pl.max_front) + " exceeds " + std::to_string(kCertFrontMax));
    col_start.upload(pl.col_start); row_ptr.upload(pl.row_ptr); rel.upload(pl.rel); child_ptr.upload(pl.child_ptr);
    child_idx.upload(pl.child_idx); roots.upload(pl.roots); gat_ptr.upload(pl.gat_ptr); gat_pos.upload(pl.gat_pos);
    gat_ent.upload(pl.gat_ent); upd_off.upload(pl.upd_off);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(nnsdp::k_cert_chol), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
  }
  void reserve(int batch) {
    if (batch <= cap) return;
    scratch.alloc((size_t)batch * pl.scratch); ok.alloc(batch); fail.alloc(batch); minp.alloc(batch); schur.alloc(batch);
    cap = batch;
  }
  // factor -Z of `batch` candidates whose NE-vectors lie zstride apart; results stay on the device until fetched
  void launch(const double* z, long long zstride, int batch, hipStream_t st, double diag_margin = 0.0) {
    reserve(batch);
    nnsdp::CertArgs a{};
    a.n_super = pl.n_super; a.e_aa = pl.e_aa; a.n_roots = (int)pl.roots.size();
    a.col_start = col_start.p; a.row_ptr = row_ptr.p; a.rel = rel.p; a.child_ptr = child_ptr.p; a.child_idx = child_idx.p;
    a.roots = roots.p; a.gat_ptr = gat_ptr.p; a.gat_pos = gat_pos.p; a.gat_ent = gat_ent.p; a.upd_off = upd_off.p;
    a.z = z; a.zstride = zstride; a.scratch = scratch.p; a.sstride = pl.scratch; a.pivot_floor = kPivotFloor; a.diag_margin = diag_margin;
    a.ld = nnsdp::cert_ld(pl.max_front);
    a.ok = ok.p; a.fail_col = fail.p; a.min_pivot = minp.p; a.schur = schur.p;
    hipLaunchKernelGGL(nnsdp::k_cert_chol, dim3(batch), dim3(nnsdp::kCertThreads), nnsdp::cert_lds_bytes(pl.max_front), st, a);
    HIPCHK(hipGetLastError());
  }
};

struct nnsdp_solver {
  nnsdp_options opt;
  ProblemCopy P;
  Congruence C;
  Pattern pat;
  ScaledOperator S;
  DevOperator D;
  std::vector<int> cn;
  std::vector<long long> coff;
  long long nmat = 0;
  int ncl = 0, nmax = 0, nmax_small = 0;
  std::vector<int> small_idx, big_idx;          // blocks for the LDS kernel (n <= 128) / for the library path
  DBuf<int> d_cn_s;
  DBuf<long long> d_coff_s;
  DBuf<double> big_A, big_T, big_D, big_E, big_scl;
  DBuf<rocblas_int> big_info;
  DBuf<int> big_flag;                   // sticky: some library eigensolve of this process reported info != 0 (k_sticky_info)
  int big_flag_host = 0;
  nnsdp::ProjPlan plan;                // projection kernel of the blocks up to kMaxLdsBlock
  int ldm = 0;
  // device state
  DBuf<int> d_cn, d_sptr, d_stats, d_long, d_rstate, d_medrows, d_medsrc, d_colcls;
  int ncs = 0;                            // multipliers whose column of A holds at most kShortCol nonzeros (listed first in d_colcls)
  int nmed = 0, nmsrc = 0, nnz_A = 0;     // rows of A with 3 .. kLongRow nonzeros / pattern entries with more than two sources (16 lanes each)
  RefineTuning tune;
  int nlong = 0;
  DBuf<long long> d_coff, d_soff;
  DBuf<unsigned char> d_isdiag;
  DBuf<unsigned int> d_gidx;
  DBuf<double> Tg, Ug;
  DBuf<double> nu, w, Vg, x, g, p, qv, ww, Minv, scal /* sigma, kappa */, acc /* 8 control numbers | ng multipliers (sharded resync) */, gs;
  DBuf<double> accp;                    // per-workgroup partial sums of the residual quantities: [7][acc_stride]
  int acc_stride = 0, nb_upd = 0, nb_dual = 0, nb_obj = 0;
  bool big_fail = false;                // a library eigensolve of a block above the LDS kernel's range reported info != 0
  // structured M^-1 (minv.hpp): used instead of the dense inverse for large multiplier counts
  bool minv_structured = false;
  MinvPlan mplan;
  MinvDev mdev{};
  DBuf<int> m_clo, m_chi, m_w0, m_w1, m_hslot0, m_chunk_of, m_sep_of, m_sep_gen, m_slot_chunk, m_slotA, m_slotB;
  DBuf<long long> m_poff, m_hoff;
  DBuf<double> m_P, m_H, m_HT, m_Sc, m_v, m_kap, m_t, m_rpart, m_rvec, m_xS, m_coef, m_dpart;
  DBuf<double> symv_part;   // batch handles: partial products of the tiled symmetric M^-1 q
  double sigma = 1.0, proj_tol = 1e-4;
  hipStream_t st = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int graph_iters = 0;
  bool graph_pipe = false;              // the captured iterations contain the tile-parallel pipeline
  // tile-parallel form of the refinement stage (refine_pipe.hpp): five short launches over the whole chip in front of the one-CU kernel.
  // pipe_mode 0: never; 1 (default): for launches whose largest block is above 96 (the packed variant's range: 0.30 ms -> 71 us per
  // launch of 106 + 4 x 151; at blocks up to 96 the five launches - ~1.7 us between two of them, 6-10 us each whatever the block
  // count, bound by the CU's vector-memory issue rate - only tie with the one-CU stage's 56 us), switched on / off
  // at check iterations from the share of block visits the stage carries (the first ~2 000 iterations of a solve run the exact sweeps:
  // the pipeline's launches would be pure overhead there); 2: as 1 for every block size (diagnostic); 3: always on (diagnostic)
  nnsdp::RefinePipe pipe;
  int pipe_mode = 1;
  bool pipe_on = false;
  long long pipe_seen[2] = {0, 0};      // stats counters at the last check: visits carried by the stage / all warm visits
  std::vector<hipEvent_t> ev;
  std::unique_ptr<RocHandle> roc;
  long long iters_done = 0, next_adapt = 0, next_trace = 0, next_cert = 500, best_iter = 0;
  double best_res = 1e300;
  double lr_ema = 0.0;      // smoothed log of the balancing ratio sqrt(pres / dres)
  bool have_ema = false;
  int trace_polish = 0;
  int since_cold = 0;
  double t_setup = 0, t_solve = 0, t_eig = 0, t_create0 = 0;
  double last_pres = 1e300, last_dres = 1e300, last_pobj = 0, last_dobj = 0;
  std::unique_ptr<FullOperator> full;
  // the certificate's operator (reference coordinates, no normalisation, no cliques) is only needed by finish(): its host half
  // (13-20 ms at W40-D20) is built on a second thread while the solve runs
  std::future<std::unique_ptr<FullOperator>> full_fut;
  // clique-sharded mode (one rank per GPU, RCCL all-reduce of the consensus sum per iteration)
  int nranks = 1, rank = 0, k0 = 0, k1 = 0;
  Rccl::Comm comm = nullptr;
  bool sharded = false;                // clique-sharded mode on (RCCL communicator or the caller's own all-reduce)
  bool rccl_graph_ok = false;          // an ncclAllReduce on the solver's stream can be captured into a hipGraph and replayed (probed in set_comm)
  long long graph_launches = 0;        // hipGraphLaunch calls so far (diagnostic, nnsdp_solver_info)
  nnsdp_allreduce_fn ar_fn = nullptr;  // caller's sum-all-reduce over host buffers (nnsdp_solver_set_comm_callback)
  void* ar_user = nullptr;
  std::vector<double> ar_host;
  DBuf<int> d_sptr_own;
  DBuf<long long> d_soff_own;
  DBuf<double> hsum;
  // device-side transport of the sharded mode (hipIpc-mapped peer buffers, kernels.hip: k_ipc_publish / k_ipc_reduce)
  bool ipc = false;
  DBuf<double> xbuf;                    // [2][NE] slots + 2 flag words
  DBuf<unsigned long long> ipc_ctr;
  DBuf<int> ipc_err;
  nnsdp::IpcArgs ipa{};
  std::vector<void*> ipc_opened;
  bool ipc_fine = false;               // exchange buffers in fine-grained device memory
  SplitScratch split;                   // two workgroups per block (ProjArgs::split): ping-pong variant, one SDP, no compacted block list

  ~nnsdp_solver() {
    if (comm) (void)Rccl::get().CommDestroy(comm);
    for (void* q : ipc_opened) (void)hipIpcCloseMemHandle(q);
    for (hipGraphExec_t g : gexec_chk) if (g) (void)hipGraphExecDestroy(g);
    if (acc_host) (void)hipHostFree(acc_host);
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }

  double* d_sigma() { return scal.p; }
  double* d_kappa() { return scal.p + 1; }

  // A solver is set up in two parts: setup_shared() builds what depends on the network, the input box, the intervals, beta and
  // the KIND of output QC only - the operator, the gather tables, the row / column classes and M^-1 - and setup_member() what one
  // SDP owns: its iteration state, scratch, graphs.  nnsdp_solver_create runs both; a sibling (nnsdp_solver_create_sibling) takes
  // the first part from its parent by reference count (share_from) and only builds its own z0.
  int family = 0;                       // nnsdp_solver_info(7): 0 = shares nothing
  bool setup_tm = false;
  double setup_tl = 0.0;
  void lap(const char* what) { if (setup_tm) { const double t = now_s(); std::fprintf(stderr, "[nnsdp setup] %-28s %7.2f ms\n", what, 1e3 * (t - setup_tl)); setup_tl = t; } }

  void setup(const nnsdp_problem* prob, const nnsdp_options* o) {
    t_create0 = now_s();
    check_options(o);
    setup_tm = std::getenv("NNSDP_SETUP_TIMING") != nullptr;     // diagnostic: where the set-up time goes (stderr)
    setup_tl = now_s();
    P.load(prob);
    open_device();
    setup_shared();
    setup_member();
    t_setup = now_s() - t_create0;
  }

  void check_options(const nnsdp_options* o) {
    opt = *o;
    if (opt.max_iters <= 0) throw std::invalid_argument("max_iters must be > 0");
    if (!(opt.alpha > 0.0 && opt.alpha < 2.0)) throw std::invalid_argument("alpha must be in (0,2)");
    if (!(opt.sigma > 0.0)) throw std::invalid_argument("sigma must be > 0");
    if (opt.check_every <= 0) opt.check_every = 50;
    if (opt.decomp_mode < NNSDP_DECOMP_DENSE || opt.decomp_mode > NNSDP_DECOMP_AUTO)
      throw std::invalid_argument("unrecognized decomp_mode");
    if (!(opt.interval_guard >= 0.0 && opt.interval_guard < 0.1)) throw std::invalid_argument("interval_guard must be in [0, 0.1)");
    if (opt.minv_mode < 0 || opt.minv_mode > 2) throw std::invalid_argument("minv_mode must be 0 (auto), 1 (dense) or 2 (structured)");
  }

  // the certificate's host half on a second thread, the device, the stream and the library handle of this SDP (P is loaded)
  void open_device() {
    if (!std::getenv("NNSDP_NO_ASYNC_SETUP")) {
      std::unique_ptr<FullOperator> fo(new FullOperator());
      fo->P = P;
      full_fut = std::async(std::launch::async, [](std::unique_ptr<FullOperator> f) { f->build_host(); return f; }, std::move(fo));
    }
    require_gpu();
    if (opt.device >= 0) HIPCHK(hipSetDevice(opt.device));
    HIPCHK(hipStreamCreate(&st));
    roc.reset(new RocHandle());
    RBCHK(rocblas_set_stream(roc->h, st));
    lap("stream + rocBLAS handle");
  }

  void setup_shared() {
    C = make_congruence(P, opt.normalize != 0, opt.interval_guard);
    // NNSDP_DECOMP_AUTO: the finest exact decomposition the query allows - the path cliques {x_k, x_k+1, affine} when the output QC
    // does not couple x_1 with x_K (every reach query, hyperplane safety sets: the generator table then fits their pattern, which
    // is what the builder checks), DoubleDecomp otherwise.  On the ACAS-shaped width-50 query the reference's Single cliques
    // (106 + 4 x 151) take 13-17 s, the path cliques (6 x 101) 3.6 s.
    const bool auto_mode = opt.decomp_mode == NNSDP_DECOMP_AUTO;
    if (auto_mode) opt.decomp_mode = NNSDP_DECOMP_PATH;
    std::vector<std::vector<int>> cl = reduced_cliques(P, C, opt.decomp_mode);
    Pattern pt = build_pattern(C.nred, cl);
    Operator op;
    try {
      op = OperatorBuilder(P, C, pt).build();
    } catch (const std::runtime_error& e) {
      if (auto_mode) {
        opt.decomp_mode = NNSDP_DECOMP_DOUBLE;
        cl = reduced_cliques(P, C, opt.decomp_mode);
        pt = build_pattern(C.nred, cl);
        op = OperatorBuilder(P, C, pt).build();
      } else if (opt.decomp_mode == NNSDP_DECOMP_PATH)
        throw std::invalid_argument(std::string("PATH decomposition needs an output QC without x_1 -- x_K coupling (S12 = 0): ") + e.what());
      else throw;
    }
    {
      std::vector<int> layers = P.generator_layers();
      S = scale_operator(op, opt.normalize != 0, &layers);     // multipliers ordered by network layer (any order is the same iteration)
    }
    lap("operator build (host)");
    pat = std::move(op.pat);
    D.upload(S, pat);
    lap("operator upload");
    ncl = (int)pat.cliques.size();
    cn.resize(ncl);
    coff.resize(ncl + 1);
    nmat = 0;
    nmax = 0;
    for (int k = 0; k < ncl; ++k) {
      cn[k] = (int)pat.cliques[k].size();
      coff[k] = nmat;
      nmat += (long long)cn[k] * cn[k];
      nmax = std::max(nmax, cn[k]);
    }
    coff[ncl] = nmat;
    // blocks up to 160 go to the LDS-resident Jacobi kernel (one launch for all of them; above 128 - the reference's 151-wide
    // cliques of width-50 nets, chordal_cliques.jl:33-36 - in its packed variant); larger ones - the single Zdim x Zdim cone of
    // DeepSdpOptions (deep_sdp.jl:57) - are projected one at a time through rocSOLVER dsyevd + rocBLAS dgemm
    nmax_small = 0;
    for (int k = 0; k < ncl; ++k) {
      if (cn[k] <= nnsdp::kMaxLdsBlock) { small_idx.push_back(k); nmax_small = std::max(nmax_small, cn[k]); }
      else big_idx.push_back(k);
    }
    if (!big_idx.empty()) build_compact_lists(0, ncl);
    const int nsm = std::max(nmax_small, 1);
    if (const char* e = std::getenv("NNSDP_REFINE")) opt.proj_refine = std::atoi(e);                   // (diagnostic override, read before the variant is chosen)
    tune = RefineTuning::from_env();
    plan = nnsdp::plan_projection(nsm, opt.proj_refine != 0);
    // gather sources: entry e <- (clique k, lower element (i,j))
    std::vector<int> sptr(S.NE + 1, 0);
    for (int k = 0; k < ncl; ++k) {
      auto& cq = pat.cliques[k];
      for (int j = 0; j < cn[k]; ++j)
        for (int i = j; i < cn[k]; ++i) sptr[pat.pos(cq[i], cq[j]) + 1]++;
    }
    for (int e = 0; e < S.NE; ++e) sptr[e + 1] += sptr[e];
    std::vector<long long> soff(sptr[S.NE]);
    {
      std::vector<int> fill(sptr.begin(), sptr.end() - 1);
      for (int k = 0; k < ncl; ++k) {
        auto& cq = pat.cliques[k];
        for (int j = 0; j < cn[k]; ++j)
          for (int i = j; i < cn[k]; ++i) soff[fill[pat.pos(cq[i], cq[j])]++] = coff[k] + (long long)j * cn[k] + i;
      }
    }
    std::vector<unsigned char> isdiag(S.NE);
    for (int e = 0; e < S.NE; ++e) isdiag[e] = pat.erow[e] == pat.ecol[e];
    std::vector<unsigned int> gidx(nmat);
    for (int k = 0; k < ncl; ++k) {
      auto& cq = pat.cliques[k];
      for (int j = 0; j < cn[k]; ++j)
        for (int i = 0; i < cn[k]; ++i)
          gidx[coff[k] + (long long)j * cn[k] + i] = (unsigned)pat.pos(cq[i], cq[j]) | (i == j ? 0x80000000u : 0u);
    }
    d_cn.upload(cn); d_coff.upload(coff); d_sptr.upload(sptr); d_soff.upload(soff);
    d_isdiag.upload(isdiag); d_gidx.upload(gidx);
    lap("gather tables + upload");
    giters = graph_iters_for(opt.check_every);
    {
      std::vector<int> lr;
      for (int e = 0; e < S.NE; ++e)
        if (S.csr_ptr[e + 1] - S.csr_ptr[e] > kLongRow) lr.push_back(e);
      nlong = (int)lr.size();
      d_long.upload(lr);
      std::vector<int> mr, ms;
      for (int e = 0; e < S.NE; ++e) {
        const int nz = S.csr_ptr[e + 1] - S.csr_ptr[e];
        if (nz > 2 && nz <= kLongRow) mr.push_back(e);
        if (sptr[e + 1] - sptr[e] > 2) ms.push_back(e);
      }
      nmed = (int)mr.size(); nmsrc = (int)ms.size(); nnz_A = std::max(S.csr_ptr[S.NE], 1);
      if (mr.empty()) mr.push_back(0);
      if (ms.empty()) ms.push_back(0);
      d_medrows.upload(mr); d_medsrc.upload(ms);
      std::vector<int> cc;
      cc.reserve(S.ng + 1);
      for (int g = 0; g < S.ng; ++g) if (S.csc_ptr[g + 1] - S.csc_ptr[g] <= nnsdp::kShortCol) cc.push_back(g);
      ncs = (int)cc.size();
      for (int g = 0; g < S.ng; ++g) if (S.csc_ptr[g + 1] - S.csc_ptr[g] > nnsdp::kShortCol) cc.push_back(g);
      if (cc.empty()) cc.push_back(0);
      d_colcls.upload(cc);
    }
    // M^-1 on the device (rocSOLVER potrf + potri; one-time plain-library factorisation)
    int ng = S.ng;
    ldm = (ng + 1) & ~1;
    if (opt.minv_mode == 2 || (opt.minv_mode == 0 && ng >= kStructuredMinvFrom)) {
      mplan = plan_minv(S);
      if (mplan.ok) minv_structured = true;
      else if (opt.minv_mode == 2) throw std::invalid_argument("structured M^-1 not applicable: too few layers or the generator table is not block-banded by layer");
    }
    if (minv_structured) { build_structured_minv(); lap("structured M^-1"); }
    else {
      std::unique_ptr<double[]> M(new double[(size_t)std::max(ng, 1) * std::max(ng, 1)]);      // (not initialised: the builder's threads touch it first)
      build_M_lower(S, M.get());
      lap("M = I + A'D^-1A (host)");
      Minv.alloc((size_t)ldm * std::max(ng, 1));
      Minv.zero();
      HIPCHK(hipMemcpy2D(Minv.p, (size_t)ldm * sizeof(double), M.get(), (size_t)ng * sizeof(double), (size_t)ng * sizeof(double),
                         ng, hipMemcpyHostToDevice));
    lap("M upload");
    DBuf<rocblas_int> info;
    info.alloc(1);
    RBCHK(rocsolver_dpotrf(roc->h, rocblas_fill_lower, ng, Minv.p, ldm, info.p));
    HIPCHK(hipStreamSynchronize(st));
    if (info.download()[0] != 0) throw HipError("Cholesky of M = I + A'D^-1A failed (potrf info != 0)");
    lap("potrf");
    RBCHK(rocsolver_dpotri(roc->h, rocblas_fill_lower, ng, Minv.p, ldm, info.p));
    hipLaunchKernelGGL(k_symmetrize_lower, dim3(cdiv(ng, 256), ng), dim3(256), 0, st, ng, ldm, Minv.p);
    HIPCHK(hipStreamSynchronize(st));
    if (info.download()[0] != 0) throw HipError("inverse of M = I + A'D^-1A failed (potri info != 0)");
    lap("potri + symmetrise");
    }
  }

  // what one SDP owns: scratch of the projection variants, counters, the iteration state (S, the plan and the tables are in place,
  // built by setup_shared or taken over by share_from)
  void setup_member() {
    const int ng = S.ng;
    if (!big_idx.empty()) {
      big_A.alloc((size_t)nmax * nmax); big_T.alloc((size_t)nmax * nmax); big_D.alloc(nmax); big_E.alloc(nmax); big_scl.alloc(2);
      big_info.alloc(big_idx.size()); big_info.zero();
      big_flag.alloc(1); big_flag.zero();
    }
    {
      const int nsm = std::max(nmax_small, 1);
      // two workgroups per block for the warm-start congruence (ProjArgs::split): only where the second workgroup finds a free CU (one
      // SDP's blocks; the batch handle fills the chip already and keeps the one-workgroup form) and where it pays (a block above 80:
      // six tile columns; at five and fewer the two forms tie - W40-D20 Double 57.8 / 58.3 us per step).  What the hand-over may cost
      // decided everything: with an agent-scope fence in every wave and an acquire in every poll (an L2 write-back / invalidate each)
      // the launch was SLOWER (66.4 against 61.8 us at n = 85); with workgroup-scope ordering only it was fast and WRONG under
      // multi-process contention (the two-rank test saw stale tiles in 2 runs of 3: the pair does not always share an L2 then); with
      // ONE agent-scope release behind the helper's barrier and ONE acquire fence after the leader's poll it is right and 3-4 us
      // faster per launch (56.8 against 59.9 us, W40-D20 76.5 against 78.1 us per step; profiles/r04_split_probe.log)
      int want = nsm > 80 ? 1 : 0;
      if (const char* e = std::getenv("NNSDP_SPLIT")) want = std::atoi(e);                              // (diagnostic override)
      if (want != 0 && plan.split_ok() && big_idx.empty() && ncl <= 120) split.alloc(ncl);
    }
    d_stats.alloc(14); d_stats.zero();
    {
      void* hp = nullptr;
      HIPCHK(hipHostMalloc(&hp, 8 * sizeof(double) + 16 * sizeof(int), hipHostMallocDefault));
      std::memset(hp, 0, 8 * sizeof(double) + 16 * sizeof(int));
      acc_host = static_cast<double*>(hp);
      stats_host = reinterpret_cast<int*>(acc_host + 8);
    }
    if (const char* e = std::getenv("NNSDP_PIPE")) pipe_mode = std::atoi(e);                             // (diagnostic override)
    d_rstate.alloc(4 * (size_t)std::max(ncl, 1)); d_rstate.zero();      // (4 ints per block: kernels.hip, ProjArgs::rstate)
    // iteration state
    nu.alloc(ng + nmat); w.alloc(ng + nmat); Vg.alloc(nmat);
    if (plan.packed()) { Tg.alloc(nmat); Tg.zero(); Ug.alloc(nmat); Ug.zero(); }      // scratch of the packed variant (warm start, rotation log; new basis of its refinement stage)
    x.alloc(S.NE); g.alloc(S.NE); p.alloc(ng); qv.alloc(ldm); ww.alloc(ng); gs.alloc(ng);
    scal.alloc(4); acc.alloc(8 + (size_t)ng); acc.zero();
    nb_upd = cdiv(ng + nmat, kThreads);
    nb_dual = cdiv((long long)S.NE * 16, kThreads) + nlong;
    nb_obj = cdiv(std::max(ng, S.NE), kThreads);
    acc_stride = std::max({nb_upd, nb_dual, nb_obj});
    accp.alloc(7 * (size_t)acc_stride);
    nu.zero(); w.zero(); Vg.zero(); x.zero(); g.zero(); qv.zero();
    {
      std::vector<double> s0(ng);
      for (int i = 0; i < ng; ++i) s0[i] = std::max(S.c[i], 0.0);
      HIPCHK(hipMemcpy(nu.p, s0.data(), ng * sizeof(double), hipMemcpyHostToDevice));
    }
    sigma = opt.sigma;
    proj_tol = opt.proj_tol > 0 ? opt.proj_tol : 1e-4;
    if (const char* e = std::getenv("NNSDP_PROJ_TOL_CAP")) { if (!(opt.proj_tol > 0)) proj_tol = std::atof(e); }
    double sc[4] = {sigma, 1.0, proj_tol, 0.0};
    HIPCHK(hipMemcpy(scal.p, sc, sizeof(sc), hipMemcpyHostToDevice));
    HIPCHK(proj_allow_big_lds(plan));
    k0 = 0; k1 = ncl;
    build_pipe();
    lap("state buffers");
  }

  // ---- solver families ---------------------------------------------------------------------------------------------------------
  // The output QC (normal / S / yc, invP) and the last affine layer enter z0 and nothing else (OperatorBuilder::build_z0): two SDPs
  // that agree in everything else have the same generators, cost, kept set, column scales, pattern, tables and M^-1.
  // First field in which q cannot share p's set-up, or nullptr.
  static const char* family_mismatch(const ProblemCopy& p, const ProblemCopy& q) {
    if (p.K != q.K) return "K";
    if (p.xdims != q.xdims) return "xdims";
    for (int k = 0; k + 1 < p.K; ++k) if (p.W[k] != q.W[k] || p.b[k] != q.b[k]) return "M (an affine layer before the last one)";
    if (p.x1min != q.x1min) return "x1min";
    if (p.x1max != q.x1max) return "x1max";
    if (p.acymin != q.acymin) return "acymin";
    if (p.acymax != q.acymax) return "acymax";
    if (p.smin != q.smin) return "smin";
    if (p.smax != q.smax) return "smax";
    if (p.beta != q.beta) return "beta";
    if (p.activ != q.activ) return "activ";
    if (p.query_kind != q.query_kind) return "query_kind";
    // (circle and ellipsoid are one kind here: both give the gout generator the coefficient -0.5, the hyperplane -1)
    auto gout_kind = [](int k) { return k == NNSDP_OUT_ELLIPSOID ? (int)NNSDP_OUT_CIRCLE : k; };
    if (gout_kind(p.out_kind) != gout_kind(q.out_kind)) return "out_kind";
    return nullptr;
  }

  // every set-up buffer of `o`, by reference
  void share_from(nnsdp_solver& o) {
    C = o.C; pat = o.pat; S = o.S;
    cn = o.cn; coff = o.coff; nmat = o.nmat; ncl = o.ncl; nmax = o.nmax; nmax_small = o.nmax_small;
    small_idx = o.small_idx; big_idx = o.big_idx; plan = o.plan; tune = o.tune; ldm = o.ldm; giters = o.giters;
    ncs = o.ncs; nmed = o.nmed; nmsrc = o.nmsrc; nnz_A = o.nnz_A; nlong = o.nlong;
    D.NE = o.D.NE; D.ng = o.D.ng; D.n = o.D.n;
    D.csr_ptr.share(o.D.csr_ptr); D.csr_col.share(o.D.csr_col); D.csr_val.share(o.D.csr_val);
    D.csc_ptr.share(o.D.csc_ptr); D.csc_row.share(o.D.csc_row); D.csc_val.share(o.D.csc_val);
    D.c.share(o.D.c); D.Dinv.share(o.D.Dinv); D.erow.share(o.D.erow); D.ecol.share(o.D.ecol);
    d_cn.share(o.d_cn); d_coff.share(o.d_coff); d_sptr.share(o.d_sptr); d_soff.share(o.d_soff); d_isdiag.share(o.d_isdiag);
    d_gidx.share(o.d_gidx); d_long.share(o.d_long); d_medrows.share(o.d_medrows); d_medsrc.share(o.d_medsrc); d_colcls.share(o.d_colcls);
    if (!big_idx.empty()) {      // (the compact lists of all blocks: a family member is never sharded)
      proj_small = o.proj_small; proj_big = o.proj_big; nmax_proj_small = o.nmax_proj_small;
      d_cn_s.share(o.d_cn_s); d_coff_s.share(o.d_coff_s);
    }
    minv_structured = o.minv_structured;
    if (!minv_structured) Minv.share(o.Minv);
    else {
      mplan = o.mplan; m_nslots = o.m_nslots; m_ntiles3 = o.m_ntiles3; m_ntiles_sep = o.m_ntiles_sep;
      m_tiles.share(o.m_tiles);
      m_clo.share(o.m_clo); m_chi.share(o.m_chi); m_w0.share(o.m_w0); m_w1.share(o.m_w1); m_hslot0.share(o.m_hslot0);
      m_chunk_of.share(o.m_chunk_of); m_sep_of.share(o.m_sep_of); m_sep_gen.share(o.m_sep_gen); m_slot_chunk.share(o.m_slot_chunk);
      m_slotA.share(o.m_slotA); m_slotB.share(o.m_slotB); m_poff.share(o.m_poff); m_hoff.share(o.m_hoff);
      m_P.share(o.m_P); m_H.share(o.m_H); m_HT.share(o.m_HT); m_Sc.share(o.m_Sc); m_v.share(o.m_v); m_kap.share(o.m_kap);
      bind_minv_dev(o.mdev.r);
    }
  }

  // device bytes this handle holds alone / together with other members of its family (nnsdp_solver_info 8, 9)
  void device_bytes(size_t& own, size_t& shared_b) const {
    own = shared_b = 0;
    auto add = [&](size_t b, bool sh) { (sh ? shared_b : own) += b; };
#define NNSDP_B(x) add((x).bytes(), (x).shared());
    NNSDP_B(D.csr_ptr) NNSDP_B(D.csr_col) NNSDP_B(D.csr_val) NNSDP_B(D.csc_ptr) NNSDP_B(D.csc_row) NNSDP_B(D.csc_val) NNSDP_B(D.z0) NNSDP_B(D.c)
    NNSDP_B(D.Dinv) NNSDP_B(D.erow) NNSDP_B(D.ecol) NNSDP_B(d_cn_s) NNSDP_B(d_coff_s) NNSDP_B(big_A) NNSDP_B(big_T) NNSDP_B(big_D) NNSDP_B(big_E) NNSDP_B(big_scl)
    NNSDP_B(big_info) NNSDP_B(big_flag) NNSDP_B(d_cn) NNSDP_B(d_sptr) NNSDP_B(d_stats) NNSDP_B(d_long) NNSDP_B(d_rstate) NNSDP_B(d_medrows)
    NNSDP_B(d_medsrc) NNSDP_B(d_colcls) NNSDP_B(d_coff) NNSDP_B(d_soff) NNSDP_B(d_isdiag) NNSDP_B(d_gidx) NNSDP_B(Tg) NNSDP_B(Ug) NNSDP_B(nu) NNSDP_B(w)
    NNSDP_B(Vg) NNSDP_B(x) NNSDP_B(g) NNSDP_B(p) NNSDP_B(qv) NNSDP_B(ww) NNSDP_B(Minv) NNSDP_B(scal) NNSDP_B(acc) NNSDP_B(gs) NNSDP_B(accp)
    NNSDP_B(m_clo) NNSDP_B(m_chi) NNSDP_B(m_w0) NNSDP_B(m_w1) NNSDP_B(m_hslot0) NNSDP_B(m_chunk_of) NNSDP_B(m_sep_of) NNSDP_B(m_sep_gen)
    NNSDP_B(m_slot_chunk) NNSDP_B(m_slotA) NNSDP_B(m_slotB) NNSDP_B(m_poff) NNSDP_B(m_hoff) NNSDP_B(m_P) NNSDP_B(m_H) NNSDP_B(m_HT) NNSDP_B(m_Sc)
    NNSDP_B(m_v) NNSDP_B(m_kap) NNSDP_B(m_t) NNSDP_B(m_rpart) NNSDP_B(m_rvec) NNSDP_B(m_xS) NNSDP_B(m_coef) NNSDP_B(m_dpart) NNSDP_B(m_tiles) NNSDP_B(symv_part)
    NNSDP_B(split.B) NNSDP_B(split.ack) NNSDP_B(split.seen) NNSDP_B(split.xcc) NNSDP_B(split.err)
#undef NNSDP_B
  }

  // a member of `parent`'s family for a problem that differs from the parent's in the output QC (and the last affine layer) only
  void setup_sibling(nnsdp_solver& parent, const nnsdp_problem* prob) {
    t_create0 = now_s();
    if (parent.sharded) throw std::invalid_argument("a clique-sharded solver (or one that has been given a communicator) cannot have siblings");
    opt = parent.opt;                   // (decomposition as the parent resolved it)
    setup_tm = std::getenv("NNSDP_SETUP_TIMING") != nullptr;
    setup_tl = now_s();
    P.load(prob);
    if (const char* f = family_mismatch(parent.P, P))
      throw std::invalid_argument(std::string("the sibling's problem differs from its parent's in `") + f + "`: only the output data (normal / S / yc, invP) and the last affine layer may differ");
    open_device();
    share_from(parent);
    // this member's z0 on the shared pattern, scaled as scale_operator scales it
    std::vector<double> z0;
    try {
      z0 = OperatorBuilder(P, C, pat).build_z0_only();
    } catch (const std::runtime_error& e) {
      if (opt.decomp_mode == NNSDP_DECOMP_PATH)
        throw std::invalid_argument(std::string("PATH decomposition needs an output QC without x_1 -- x_K coupling (S12 = 0): ") + e.what());
      throw std::invalid_argument(std::string("the sibling's output QC does not fit the parent's clique pattern: ") + e.what());
    }
    double zn = 0;
    for (double v : z0) zn += v * v;
    zn = std::sqrt(zn);
    S.zscale = (opt.normalize != 0 && zn > 0) ? 1.0 / zn : 1.0;
    S.z0 = std::move(z0);
    for (auto& v : S.z0) v *= S.zscale;
    D.z0.upload(S.z0);
    lap("sibling: z0 + shared set-up");
    setup_member();
    static std::atomic<int> next_family{0};
    if (parent.family == 0) parent.family = ++next_family;
    family = parent.family;
    t_setup = now_s() - t_create0;
  }

  // blocks [lo, hi) this process projects (all of them, or the rank's range in clique-sharded mode), split into the ones the
  // LDS-resident kernel takes in one launch (compact device lists) and the ones that go through the library path
  std::vector<int> proj_small, proj_big;
  int nmax_proj_small = 0;
  void build_compact_lists(int lo, int hi) {
    proj_small.clear(); proj_big.clear();
    std::vector<int> cs;
    std::vector<long long> os;
    nmax_proj_small = 0;
    for (int k = lo; k < hi; ++k) {
      if (cn[k] <= nnsdp::kMaxLdsBlock) { proj_small.push_back(k); cs.push_back(cn[k]); os.push_back(coff[k]); nmax_proj_small = std::max(nmax_proj_small, cn[k]); }
      else proj_big.push_back(k);
    }
    if (cs.empty()) { cs.push_back(1); os.push_back(0); }
    d_cn_s.upload(cs); d_coff_s.upload(os);
  }
  int big_slot(int k) const { return (int)(std::find(big_idx.begin(), big_idx.end(), k) - big_idx.begin()); }

  static constexpr int kStructuredMinvFrom = 3500;   // auto mode: kept multipliers from which the structured M^-1 replaces the dense one (98 MB)

  // device set-up of the structured M^-1 (minv.hpp): small dense inverses through rocSOLVER / rocBLAS, all on the solver's stream
  void build_structured_minv() {
    const MinvPlan& Q = mplan;
    MinvBlocks B = assemble_minv_blocks(S, Q);
    const int ng = S.ng, nc = Q.nchunk, nS = Q.nS, ldS = Q.ldS;
    if (opt.verbose || std::getenv("NNSDP_MINV_PLAN")) {
      double bp = 0, bh = 0;
      int nmaxc = 0, wmax = 0;
      for (int j = 0; j < nc; ++j) {
        const double n = Q.chi[j] - Q.clo[j], wj = Q.w1[j] - Q.w0[j];
        bp += 8.0 * n * n; bh += 8.0 * n * wj;
        nmaxc = std::max(nmaxc, (int)n); wmax = std::max(wmax, (int)wj);
      }
      std::fprintf(stderr, "[nnsdp] structured M^-1: %d multipliers, %d chunks (largest %d), separator %d (widest coupling %d), rank-%d term; "
                   "bytes per application: chunk inverses %.1f MB (stage 1), H %.1f MB (stage 1) + %.1f MB (stage 3), Schur inverse %.1f MB\n",
                   ng, nc, nmaxc, nS, wmax, Q.r, bp / 1e6, bh / 1e6, bh / 1e6, 8.0 * nS * (double)nS / 1e6);
    }
    DBuf<double> Tjs;
    m_P.upload(B.Tjj); Tjs.upload(B.Tjs); m_Sc.upload(B.Tss);
    m_H.alloc((size_t)Q.htot); m_HT.alloc((size_t)Q.htot);
    m_H.zero(); m_HT.zero();
    DBuf<rocblas_int> info;
    info.alloc(1);
    const double one = 1.0, zero = 0.0, mone = -1.0;
    for (int j = 0; j < nc; ++j) {
      const int n = Q.chi[j] - Q.clo[j], wj = Q.w1[j] - Q.w0[j], ldn = (n + 1) & ~1, ldw = (wj + 1) & ~1;
      double* Pj = m_P.p + Q.poff[j];
      RBCHK(rocsolver_dpotrf(roc->h, rocblas_fill_lower, n, Pj, ldn, info.p));
      HIPCHK(hipStreamSynchronize(st));
      if (info.download()[0] != 0) throw HipError("structured M^-1: Cholesky of a chunk block failed");
      RBCHK(rocsolver_dpotri(roc->h, rocblas_fill_lower, n, Pj, ldn, info.p));
      hipLaunchKernelGGL(k_symmetrize_lower, dim3(cdiv(n, 256), n), dim3(256), 0, st, n, ldn, Pj);
      if (wj > 0) {
        double* Hj = m_H.p + Q.hoff[j];
        const double* Tj = Tjs.p + Q.hoff[j];
        RBCHK(rocblas_dgemm(roc->h, rocblas_operation_none, rocblas_operation_none, n, wj, n, &one, Pj, ldn, Tj, ldn, &zero, Hj, ldn));
        RBCHK(rocblas_dgemm(roc->h, rocblas_operation_transpose, rocblas_operation_none, wj, wj, n, &mone, Tj, ldn, Hj, ldn, &one,
                            m_Sc.p + (size_t)Q.w0[j] * ldS + Q.w0[j], ldS));
        hipLaunchKernelGGL(k_minv_transpose, dim3(cdiv((long long)n * wj, 256)), dim3(256), 0, st, n, wj, ldn, ldw, Hj, m_HT.p + Q.hoff[j]);
      }
    }
    RBCHK(rocsolver_dpotrf(roc->h, rocblas_fill_lower, nS, m_Sc.p, ldS, info.p));
    HIPCHK(hipStreamSynchronize(st));
    if (info.download()[0] != 0) throw HipError("structured M^-1: Cholesky of the separator Schur complement failed");
    RBCHK(rocsolver_dpotri(roc->h, rocblas_fill_lower, nS, m_Sc.p, ldS, info.p));
    hipLaunchKernelGGL(k_symmetrize_lower, dim3(cdiv(nS, 256), nS), dim3(256), 0, st, nS, ldS, m_Sc.p);
    // index maps
    std::vector<int> sep_gen(nS), hslot0(nc), slot_chunk, slotA(nS), slotB(nS);
    for (int g = 0; g < ng; ++g) if (Q.sep_of[g] >= 0) sep_gen[Q.sep_of[g]] = g;
    int nslots = 0;
    for (int j = 0; j < nc; ++j) { hslot0[j] = nslots; for (int c = Q.w0[j]; c < Q.w1[j]; ++c) slot_chunk.push_back(j); nslots += Q.w1[j] - Q.w0[j]; }
    for (int sj = 0; sj + 1 < nc; ++sj)
      for (int c = Q.soff[sj]; c < Q.soff[sj + 1]; ++c) { slotA[c] = hslot0[sj] + (c - Q.w0[sj]); slotB[c] = hslot0[sj + 1] + (c - Q.w0[sj + 1]); }
    m_clo.upload(Q.clo); m_chi.upload(Q.chi); m_w0.upload(Q.w0); m_w1.upload(Q.w1); m_hslot0.upload(hslot0);
    m_poff.upload(Q.poff); m_hoff.upload(Q.hoff); m_chunk_of.upload(Q.chunk_of); m_sep_of.upload(Q.sep_of);
    m_sep_gen.upload(sep_gen); m_slot_chunk.upload(slot_chunk); m_slotA.upload(slotA); m_slotB.upload(slotB);
    m_v.alloc((size_t)ng * std::max(Q.r, 1)); m_kap.alloc(64);
    m_v.zero(); m_kap.zero();
    m_nslots = nslots;
    {      // row tiles of the multi-vector stages (minv.hpp): the stage-3 tiles (chunk rows, separators) come first
      const std::vector<int4> tiles = minv_tiles(Q, hslot0);
      m_ntiles3 = m_ntiles_sep = 0;
      for (const int4& t : tiles) { if (t.x == kTileP || t.x == kTileSep) ++m_ntiles3; if (t.x == kTileSep) ++m_ntiles_sep; }
      m_tiles.upload(tiles);
    }
    bind_minv_dev(0);
    // low-rank part: v = T^-1 U (the structured apply with r = 0), kap = (diag(1/d) + U'v)^-1 on the host (r x r, r <= 8)
    if (Q.r > 0) {
      DBuf<double> U, V;
      U.upload(B.U);
      V.alloc((size_t)ng * Q.r);
      for (int a = 0; a < Q.r; ++a) apply_structured_minv(U.p + (size_t)a * ng, V.p + (size_t)a * ng, st);
      HIPCHK(hipStreamSynchronize(st));
      std::vector<double> vh = V.download();
      const int r = Q.r;
      std::vector<double> Km((size_t)r * r, 0.0), Ki((size_t)r * r, 0.0);
      for (int a = 0; a < r; ++a)
        for (int b = 0; b < r; ++b) {
          double sdot = a == b ? 1.0 / B.dU[a] : 0.0;
          for (int g = 0; g < ng; ++g) sdot += B.U[(size_t)a * ng + g] * vh[(size_t)b * ng + g];
          Km[(size_t)a * r + b] = sdot;
        }
      for (int a = 0; a < r; ++a) Ki[(size_t)a * r + a] = 1.0;
      for (int cidx = 0; cidx < r; ++cidx) {       // Gauss-Jordan on the small symmetric positive definite matrix
        const double pv = Km[(size_t)cidx * r + cidx];
        if (!(pv > 0.0)) throw HipError("structured M^-1: low-rank capacitance matrix is not positive definite");
        for (int b = 0; b < r; ++b) { Km[(size_t)cidx * r + b] /= pv; Ki[(size_t)cidx * r + b] /= pv; }
        for (int a = 0; a < r; ++a) {
          if (a == cidx) continue;
          const double f = Km[(size_t)a * r + cidx];
          for (int b = 0; b < r; ++b) { Km[(size_t)a * r + b] -= f * Km[(size_t)cidx * r + b]; Ki[(size_t)a * r + b] -= f * Ki[(size_t)cidx * r + b]; }
        }
      }
      HIPCHK(hipMemcpy(m_v.p, vh.data(), vh.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(m_kap.p, Ki.data(), Ki.size() * sizeof(double), hipMemcpyHostToDevice));
      mdev.r = r;
    }
    HIPCHK(hipStreamSynchronize(st));
  }

  // scratch of one SDP's applications of the structured M^-1 and the device view of the (possibly shared) factors; r = rank of the
  // low-rank term in use
  int m_nslots = 0, m_ntiles3 = 0, m_ntiles_sep = 0;
  DBuf<int4> m_tiles;
  MinvMultiLds m_lds;                   // what the multi-vector stages put in LDS for these factors; !ok: ONE vector does not fit, single form only
  void bind_minv_dev(int r) {
    const MinvPlan& Q = mplan;
    const int ng = S.ng, nS = Q.nS, ldS = Q.ldS;
    m_t.alloc(ng); m_rpart.alloc(std::max(m_nslots, 1)); m_xS.alloc(std::max(ldS, 2)); m_rvec.alloc(std::max(ldS, 2)); m_coef.alloc(8);
    m_dpart.alloc(8 * kMinvParts);
    m_coef.zero(); m_rvec.zero(); m_xS.zero(); m_dpart.zero();
    mdev.ng = ng; mdev.nchunk = Q.nchunk; mdev.nS = nS; mdev.ldS = ldS; mdev.r = r; mdev.nslots = m_nslots;
    mdev.clo = m_clo.p; mdev.chi = m_chi.p; mdev.w0 = m_w0.p; mdev.w1 = m_w1.p; mdev.hslot0 = m_hslot0.p;
    mdev.poff = m_poff.p; mdev.hoff = m_hoff.p; mdev.chunk_of = m_chunk_of.p; mdev.sep_of = m_sep_of.p; mdev.sep_gen = m_sep_gen.p;
    mdev.slot_chunk = m_slot_chunk.p; mdev.slotA = m_slotA.p; mdev.slotB = m_slotB.p;
    mdev.Pinv = m_P.p; mdev.H = m_H.p; mdev.HT = m_HT.p; mdev.Scinv = m_Sc.p; mdev.v = m_v.p; mdev.kap = m_kap.p;
    mdev.tiles = m_tiles.p; mdev.ntiles = (int)m_tiles.n; mdev.ntiles3 = m_ntiles3; mdev.ntiles_sep = m_ntiles_sep;
    mdev.q = nullptr; mdev.out = nullptr;      // (set where a work table is built: structured_work)
    m_lds = minv_multi_lds(Q);
    mdev.t = m_t.p; mdev.rpart = m_rpart.p; mdev.rvec = m_rvec.p; mdev.xS = m_xS.p; mdev.coef = m_coef.p; mdev.dpart = m_dpart.p;
  }

  // out = M^-1 q through the structured form: four dependent launches (the second is tiny)
  void apply_structured_minv(const double* q, double* out, hipStream_t s_) {
    const int ng = S.ng;
    hipLaunchKernelGGL(k_minv_stage1, dim3(cdiv((long long)(ng + mdev.nslots + kMinvParts) * 64, kThreads)), dim3(kThreads), 0, s_, mdev, q);
    hipLaunchKernelGGL(k_minv_resid, dim3(cdiv(mdev.nS, kThreads) + 1), dim3(kThreads), 0, s_, mdev, q);
    hipLaunchKernelGGL(k_minv_schur, dim3(cdiv((long long)mdev.nS * 64, kThreads)), dim3(kThreads), 0, s_, mdev);
    hipLaunchKernelGGL(k_minv_stage3, dim3(cdiv((long long)ng * 64, kThreads)), dim3(kThreads), 0, s_, mdev, out);
  }

  // this solver's row of a multi-vector work table: its own work buffers, out = M^-1 q
  MinvWork structured_work(const double* q, double* out) const {
    MinvWork w = mdev;
    w.q = q; w.out = out;
    return w;
  }

  // ww = M^-1 qv on stream s_ (dense GEMV or the structured form)
  void enqueue_minv(hipStream_t s_) {
    if (minv_structured) apply_structured_minv(qv.p, ww.p, s_);
    else hipLaunchKernelGGL(k_gemv_sym, dim3(cdiv((long long)S.ng * 64, kThreads)), dim3(kThreads), 0, s_, S.ng, ldm, Minv.p, qv.p, ww.p);
  }

  void set_comm(int nr, int rk, const char* id128, nnsdp_allreduce_fn fn = nullptr, void* user = nullptr, bool use_ipc = false) {
    if (nr < 1 || rk < 0 || rk >= nr || (!id128 && !fn)) throw std::invalid_argument("bad communicator arguments");
    if (use_ipc && (!fn || nr > 8)) throw std::invalid_argument("the hipIpc transport needs the caller's host all-reduce for its set-up and at most 8 ranks");
    if (iters_done != 0) throw std::invalid_argument("set_comm must be called before the first iteration");
    if (family != 0) throw std::invalid_argument("a member of a solver family cannot be clique-sharded (its M^-1 is shared)");
    if (sharded) throw std::invalid_argument("the solver already has a communicator");
    if (target_mode != NNSDP_TARGET_OFF) throw std::invalid_argument("a solver with a target cannot be clique-sharded");
    if (fn) { ar_fn = fn; ar_user = user; }
    else {
      Rccl& R = Rccl::get();
      Rccl::UniqueId uid;
      std::memcpy(uid.internal, id128, 128);
      R.check(R.CommInitRank(&comm, nr, uid, rk), "ncclCommInitRank");
    }
    sharded = true;
    nranks = nr; rank = rk;
    std::vector<int> start = shard_ranges(cn, nr);
    k0 = start[rk]; k1 = start[rk + 1];
    if (!big_idx.empty()) build_compact_lists(k0, k1);      // blocks above 128 (library path) are sharded like the others
    build_pipe();                                           // (the tile-parallel pipeline works on the rank's own blocks)
    // source lists restricted to the owned cliques
    std::vector<int> sp = d_sptr.download();
    std::vector<long long> so = d_soff.download();
    std::vector<int> sp2(S.NE + 1, 0);
    std::vector<long long> so2;
    for (int e = 0; e < S.NE; ++e) {
      for (int q = sp[e]; q < sp[e + 1]; ++q)
        if (so[q] >= coff[k0] && so[q] < coff[k1]) so2.push_back(so[q]);
      sp2[e + 1] = (int)so2.size();
    }
    if (so2.empty()) so2.push_back(0);
    d_sptr_own.upload(sp2); d_soff_own.upload(so2);
    hsum.alloc(S.NE);
    hsum.zero();
    if (use_ipc) {
      // every rank maps every other rank's exchange buffer: the 64-byte hipIpc handles travel once through the caller's host
      // all-reduce (one byte per double: a sum of zeros and one value is exact whatever the bit pattern)
      static const bool coarse = [] { const char* e = std::getenv("NNSDP_IPC_COARSE"); return e && std::atoi(e) != 0; }();   // diagnostic
      hipIpcMemHandle_t mine;
      bool fine = !coarse && xbuf.alloc_finegrained(2 * (size_t)S.NE + 4);
      if (fine && hipIpcGetMemHandle(&mine, xbuf.p) != hipSuccess) { (void)hipGetLastError(); fine = false; }
      if (!fine) {                     // (a runtime that cannot share a fine-grained allocation: ordinary device memory, coherent by the
        xbuf.alloc(2 * (size_t)S.NE + 4);   //  system-scope release / acquire pair around the flag on one device)
        HIPCHK(hipIpcGetMemHandle(&mine, xbuf.p));
      }
      ipc_fine = fine;
      xbuf.zero();
      ipc_ctr.alloc(1); ipc_ctr.zero(); ipc_err.alloc(1); ipc_err.zero();
      static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpc handle size");
      std::vector<double> all((size_t)nr * 64, 0.0);
      const unsigned char* mb = reinterpret_cast<const unsigned char*>(&mine);
      for (int i = 0; i < 64; ++i) all[(size_t)rk * 64 + i] = (double)mb[i];
      if (fn(user, all.data(), (int64_t)all.size()) != 0) throw std::runtime_error("the caller's all-reduce reported a failure");
      ipa = nnsdp::IpcArgs{};
      ipa.nranks = nr; ipa.rank = rk; ipa.NE = S.NE; ipa.ctr = ipc_ctr.p; ipa.err = ipc_err.p;
      ipa.spin_limit = 4000000;      // (a few seconds: ranks reach their first exchange a set-up time apart)
      if (const char* e = std::getenv("NNSDP_IPC_SPIN_LIMIT")) ipa.spin_limit = std::atoll(e);
      for (int r = 0; r < nr; ++r) {
        if (r == rk) { ipa.peer[r] = xbuf.p; continue; }
        hipIpcMemHandle_t h;
        unsigned char* hb = reinterpret_cast<unsigned char*>(&h);
        for (int i = 0; i < 64; ++i) hb[i] = (unsigned char)all[(size_t)r * 64 + i];
        void* q = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess));
        ipc_opened.push_back(q);
        ipa.peer[r] = static_cast<double*>(q);
      }
      ipc = true;
      rccl_graph_ok = true;          // (kernels only: the exchange replays inside the iteration's hipGraph like any other launch)
    }
    // The Woodbury core is built per process by rocSOLVER / rocBLAS, and those do not return the same bits every time when several
    // processes share a card (1 set-up in 20 under three-process contention, profiles/r03_contention_repro.log: every deviating
    // solve had a different M^-1, every solve with the common M^-1 the same bits).  Rank 0's copy therefore replaces everybody's: the
    // replicated operator is identical on all ranks by construction (one-time; the others contribute zeros to a sum).
    {
      std::vector<std::pair<double*, size_t>> bufs;
      if (minv_structured) {
        for (DBuf<double>* bf : {&m_P, &m_H, &m_HT, &m_Sc, &m_v, &m_kap}) if (bf->n) bufs.emplace_back(bf->p, bf->n);
      } else if (Minv.n) bufs.emplace_back(Minv.p, Minv.n);
      for (auto& bf : bufs) {
        if (rank != 0) HIPCHK(hipMemsetAsync(bf.first, 0, bf.second * sizeof(double), st));
        for (size_t off = 0; off < bf.second; off += (size_t)1 << 24) allreduce(bf.first + off, std::min(bf.second - off, (size_t)1 << 24));
      }
      HIPCHK(hipStreamSynchronize(st));
    }
    // Can the exchange live inside a hipGraph?  Probed once, on this communicator and stream: capture one all-reduce of the
    // consensus buffer, instantiate, replay.  If any step fails the sharded iteration stays eager (as in round 2); the
    // callback transport synchronises with the host and can never be captured.
    if (comm && !(std::getenv("NNSDP_NO_RCCL_GRAPH") && std::atoi(std::getenv("NNSDP_NO_RCCL_GRAPH")) != 0)) {
      hipGraph_t pg = nullptr;
      hipGraphExec_t pe = nullptr;
      // (the probe itself contains a collective: a rank whose capture does not even begin must not leave its peers alone in it -
      // the 'capture began' bit is agreed on eagerly first, and the capture is ended again without the call where any rank failed)
      bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
      {
        hipGraph_t g0 = nullptr;
        if (ok) ok = hipStreamEndCapture(st, &g0) == hipSuccess;
        if (g0) (void)hipGraphDestroy(g0);
        std::vector<double> cb(1, ok ? 0.0 : 1.0);
        allreduce_host(cb);
        ok = cb[0] == 0.0 && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
        // (a failure of THIS second begin after the first one succeeded on every rank is not expected; it would leave the peers in
        // the captured call below, which records a node and returns - nothing blocks inside a capture)
      }
      if (ok) {
        Rccl& R = Rccl::get();
        const int rc = R.AllReduce(hsum.p, hsum.p, (size_t)S.NE, Rccl::kFloat64, Rccl::kSum, comm, st);
        const hipError_t ec = hipStreamEndCapture(st, &pg);          // always end the capture, whatever the call returned
        ok = rc == 0 && ec == hipSuccess && pg != nullptr;
      }
      if (ok) ok = hipGraphInstantiate(&pe, pg, nullptr, nullptr, 0) == hipSuccess;
      {
        // the replay EXECUTES the collective: only when every rank holds an instantiated graph
        std::vector<double> cb(1, ok ? 0.0 : 1.0);
        allreduce_host(cb);
        ok = cb[0] == 0.0;
      }
      if (ok) ok = hipGraphLaunch(pe, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
      if (pe) (void)hipGraphExecDestroy(pe);
      if (pg) (void)hipGraphDestroy(pg);
      (void)hipGetLastError();
      rccl_graph_ok = ok;
      if (opt.verbose) std::fprintf(stderr, "[nnsdp] rank %d: ncclAllReduce inside a hipGraph: %s\n", rank, ok ? "captured and replayed" : "not capturable, eager iterations");
    }
  }

  void allreduce(double* buf, size_t count) {
    if (ar_fn) {   // the caller's collective works on host memory: stage through a host buffer (stream order is kept)
      ar_host.resize(count);
      HIPCHK(hipMemcpyAsync(ar_host.data(), buf, count * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (ar_fn(ar_user, ar_host.data(), (int64_t)count) != 0) throw std::runtime_error("the caller's all-reduce reported a failure");
      HIPCHK(hipMemcpyAsync(buf, ar_host.data(), count * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
      return;
    }
    Rccl& R = Rccl::get();
    R.check(R.AllReduce(buf, buf, count, Rccl::kFloat64, Rccl::kSum, comm, st), "ncclAllReduce");
  }

  // sum-all-reduce of a small HOST vector (rank 0's certificate / stop flag travelling to every rank)
  DBuf<double> bc_dev;
  void allreduce_host(std::vector<double>& v) {
    if (!sharded || v.empty()) return;
    if (ar_fn) {
      if (ar_fn(ar_user, v.data(), (int64_t)v.size()) != 0) throw std::runtime_error("the caller's all-reduce reported a failure");
      return;
    }
    if (bc_dev.n < v.size()) bc_dev.alloc(v.size());
    HIPCHK(hipMemcpyAsync(bc_dev.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st));
    allreduce(bc_dev.p, v.size());
    HIPCHK(hipMemcpyAsync(v.data(), bc_dev.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  bool lead() const { return !sharded || rank == 0; }

  // scratch and workgroup map of the tile-parallel pipeline for the blocks THIS process projects in one launch of the one-CU kernel
  // (all of them, the rank's range in clique-sharded mode, or the compacted list beside library-path blocks)
  void build_pipe() {
    pipe.release();
    pipe_on = false;
    if (pipe_mode == 0 || opt.proj_refine != 1 || opt.warm_start == 0) return;
    if (!plan.has_refine_stage()) return;
    std::vector<int> lst;
    if (big_idx.empty()) lst.assign(cn.begin() + k0, cn.begin() + k1);
    else for (int k : proj_small) lst.push_back(cn[k]);
    if (lst.empty()) return;
    if (pipe_mode == 1 && *std::max_element(lst.begin(), lst.end()) <= 96) return;
    HIPCHK(pipe.build(lst.data(), (int)lst.size(), nmat));
    pipe_on = pipe.ready && pipe_mode == 3;
  }
  void enqueue_proj(bool warm) {
    ProjArgs a{};
    a.cn = d_cn.p + k0; a.coff = d_coff.p + k0; a.eoff = nullptr;
    a.nu = nu.p + S.ng; a.w = w.p + S.ng; a.Vg = Vg.p; a.eig = nullptr; a.Tg = Tg.p; a.Ug = Ug.p;
    a.kappa = d_kappa(); a.tol_dev = scal.p + 2; a.stats = d_stats.p;
    a.warm = warm ? 1 : 0;
    a.max_sweeps = 15;
    a.tol = kProjTol;
    a.refine = opt.proj_refine; a.rstate = d_rstate.p + 4 * k0;
    tune.bind(a);
    const bool use_pipe = warm && pipe_on && pipe.ready;
    if (split.on() && warm && big_idx.empty()) split.bind(a, k1 - k0);
    if (big_idx.empty()) {
      if (k1 > k0) {
        if (use_pipe) { pipe.launch(pipe.args(a), st); a.pmode = pipe.pmode; }
        nnsdp::launch_proj(plan, a, k1 - k0, st);
      }
      return;
    }
    if (!proj_small.empty()) {
      a.cn = d_cn_s.p; a.coff = d_coff_s.p; a.rstate = d_rstate.p;      // (compacted block list: the first proj_small.size() slots)
      if (use_pipe) { pipe.launch(pipe.args(a), st); a.pmode = pipe.pmode; }
      nnsdp::launch_proj(plan, a, (int)proj_small.size(), st);
    }
    enqueue_big_blocks(st);
    HIPCHK(hipGetLastError());
  }
  // blocks above 128 of this process through the library path on stream s_ (the handle's stream is switched for the call: a batch
  // handle runs them on ITS stream, in order behind the batched launch)
  void enqueue_big_blocks(hipStream_t strm) {
    if (proj_big.empty()) return;
    if (strm != st) RBCHK(rocblas_set_stream(roc->h, strm));
    for (int k : proj_big) {
      const int n = cn[k];
      double* nuk = nu.p + S.ng + coff[k];
      double* wk = w.p + S.ng + coff[k];
      project_big_block(roc->h, strm, n, nuk, wk, big_A.p, big_T.p, big_D.p, big_E.p, big_info.p + big_slot(k), big_scl.p);
      hipLaunchKernelGGL(k_sticky_info, dim3(1), dim3(1), 0, strm, big_info.p + big_slot(k), big_flag.p);
      hipLaunchKernelGGL(k_big_rescale, dim3(cdiv((long long)n * n, 256)), dim3(256), 0, strm, (long long)n * n, wk, nuk, d_kappa());
    }
    if (strm != st) RBCHK(rocblas_set_stream(roc->h, st));
  }

  // hsum <- sum over ranks of the rank's own partial consensus sum (dual = 1: of nu - w): RCCL / the caller's collective, or the
  // device-side transport (partial into this rank's mapped slot, publish, sum of all ranks' slots in rank order)
  void exchange_h(int dual) {
    const int ng = S.ng, NE = S.NE;
    hipLaunchKernelGGL(k_gather_h, dim3(cdiv((long long)NE * kGatherLanes, kThreads)), dim3(kThreads), 0, st, NE, d_sptr_own.p, d_soff_own.p, d_isdiag.p,
                       nu.p + ng, w.p + ng, dual, ipc ? xbuf.p : hsum.p, ipc ? ipc_ctr.p : (const unsigned long long*)nullptr);
    if (ipc) {
      hipLaunchKernelGGL(nnsdp::k_ipc_publish, dim3(1), dim3(64), 0, st, ipa);
      hipLaunchKernelGGL(nnsdp::k_ipc_reduce, dim3(cdiv(NE, kThreads)), dim3(kThreads), 0, st, ipa, hsum.p);
    } else allreduce(hsum.p, NE);
  }

  // enqueue one iteration on the stream; check=true also accumulates the residual sums
  void enqueue_iteration(bool check, bool warm, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    int ng = S.ng, NE = S.NE;
    if (e0) HIPCHK(hipEventRecord(e0, st));
    enqueue_proj(warm);
    if (e1) HIPCHK(hipEventRecord(e1, st));
    if (sharded) {
      exchange_h(0);                              // the overlap-consensus exchange: one all-reduce per iteration
      hipLaunchKernelGGL(k_finish_g, dim3(cdiv(NE, kThreads)), dim3(kThreads), 0, st, NE, hsum.p, D.z0.p, D.Dinv.p, d_sigma(), g.p);
    } else {
      const int nshort = cdiv(NE, kThreads);
      hipLaunchKernelGGL(k_gather_g, dim3(nshort + cdiv((long long)nmsrc * 16, kThreads)), dim3(kThreads), 0, st, nshort, NE, d_sptr.p, d_soff.p, d_isdiag.p,
                         nu.p + ng, w.p + ng, D.z0.p, D.Dinv.p, d_sigma(), g.p, d_medsrc.p, nmsrc);
    }
    {
      const int nsb = cdiv((long long)ncs * 16, kThreads);
      hipLaunchKernelGGL(k_spmv_At, dim3(std::max(nsb + cdiv((long long)(ng - ncs) * 64, kThreads), 1)), dim3(kThreads), 0, st, nsb, ng, D.csc_ptr.p, D.csc_row.p,
                         D.csc_val.p, g.p, nu.p, D.c.p, d_kappa(), p.p, qv.p, d_colcls.p, ncs);
    }
    if (check) {
      if (sharded) {
        exchange_h(1);
      }
      const int nreg_cd = nb_dual - nlong;
      hipLaunchKernelGGL(k_check_dual, dim3(nb_dual), dim3(kThreads), 0, st, NE, ng, nreg_cd, nlong, d_long.p, D.csr_ptr.p,
                         D.csr_col.p, D.csr_val.p, d_sptr.p, d_soff.p, d_isdiag.p, nu.p, w.p, D.z0.p, d_sigma(), accp.p,
                         sharded ? hsum.p : (const double*)nullptr, acc_stride);
    }
    enqueue_minv(st);
    {
      const int nshort = cdiv(NE, kThreads), nreg = nshort + cdiv((long long)nmed * 16, kThreads);
      hipLaunchKernelGGL(k_spmv_A_x_all, dim3(nreg + nlong), dim3(kThreads), 0, st, NE, nshort, nreg, nlong, d_long.p, D.csr_ptr.p, D.csr_col.p,
                         D.csr_val.p, ww.p, g.p, D.Dinv.p, x.p, d_medrows.p, nmed, nnz_A);
    }
    if (check)
      hipLaunchKernelGGL(k_check_obj, dim3(nb_obj), dim3(kThreads), 0, st, ng, NE, nu.p, D.c.p, D.z0.p, x.p, d_sigma(), accp.p, acc_stride);
    hipLaunchKernelGGL(k_update_nu, dim3(nb_upd), dim3(kThreads), 0, st, ng, nmat, p.p, ww.p, D.c.p, x.p,
                       d_gidx.p, nu.p, w.p, opt.alpha, d_kappa(), check ? accp.p : (double*)nullptr, coff[k0], coff[k1],
                       (!sharded || rank == 0) ? 1 : 0, acc_stride);
    if (check)   // fixed-order second stage of the residual sums (no atomics on the way to a stopping decision)
      hipLaunchKernelGGL(k_acc_reduce, dim3(1), dim3(kThreads), 0, st, accp.p, acc_stride, nb_upd, nb_dual, nb_obj, acc.p);
    if (check && sharded) {
      // every stopping / adaptation decision is taken from these 8 numbers, so they must be bit-identical on all ranks:
      // [0..2] residual sums of the clique blocks live on their owners (multiplier block counted on rank 0 only);
      // [3..6] are computed redundantly everywhere - rank 0's copy is used; [7] is the time-limit flag of any rank.
      // Behind them travels rank 0's copy of the REPLICATED multiplier block nu[0..ng): every rank continues from the same
      // bits, so the replicated state cannot drift apart between ranks whatever their libraries round like (identical by
      // construction at every check iteration; x + 0 + ... + 0 is exact).  One all-reduce distributes all of it.
      if (rank != 0) {
        HIPCHK(hipMemsetAsync(acc.p + 3, 0, 4 * sizeof(double), st));
        HIPCHK(hipMemsetAsync(acc.p + 8, 0, (size_t)ng * sizeof(double), st));
      } else HIPCHK(hipMemcpyAsync(acc.p + 8, nu.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToDevice, st));
      const double tflag = (opt.max_time > 0 && loop_t0 > 0 && now_s() - loop_t0 > opt.max_time) ? 1.0 : 0.0;
      tflag_host = tflag;
      HIPCHK(hipMemcpyAsync(acc.p + 7, &tflag_host, sizeof(double), hipMemcpyHostToDevice, st));
      if (!big_idx.empty()) hipLaunchKernelGGL(k_fold_flag, dim3(1), dim3(1), 0, st, big_flag.p, acc.p + 7);      // (only block owners run dsyevd)
      allreduce(acc.p, 8 + (size_t)ng);
      HIPCHK(hipMemcpyAsync(nu.p, acc.p + 8, (size_t)ng * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipGetLastError());
  }

  // a cold eigendecomposition every kColdPeriod iterations bounds the drift of the warm basis
  // Jacobi stops when off(A) <= 1e-8 |A|_F (measured directly): an inexact projection two orders below
  // the 1e-6 residual target; the certificate is checked independently at the end
  static constexpr double kProjTol = 1e-8;   // (fixed-tolerance fallback; the default is adaptive, see update_proj_tol)
  // (4096 since round 4 - was 512: Jacobi rotations keep the basis orthogonal to rounding, ~n eps per sweep, so 4096 swept iterations
  // stay below 1e-10; the refinement stage measures and restores the orthogonality of the blocks it carries itself; a cold projection
  // costs 0.5-0.9 ms at n = 85 and 8 ms at n = 151, every 512 iterations that was 2 % .. 9 % of a solve)
  static constexpr int kColdPeriod = 4096;
  static constexpr int kGraphIters = 8;
  // iterations per hipGraph replay: a divisor of the check_every - 1 plain iterations between two checks when there is one near 8
  // (49 = 7 x 7), so that no iteration of the stretch is launched eagerly
  static int graph_iters_for(int check_every) {
    for (int g : {8, 7, 9, 10, 6, 12, 11, 5}) if (check_every - 1 >= g && (check_every - 1) % g == 0) return g;
    return kGraphIters;
  }
  int giters = kGraphIters;
  bool next_is_warm() {
    bool warm = opt.warm_start != 0 && iters_done > 0 && since_cold < kColdPeriod;
    since_cold = warm ? since_cold + 1 : 1;
    return warm;
  }

  void build_graph(int n_iters) {
    if (gexec && graph_iters == n_iters && graph_pipe == pipe_on) return;
    if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < n_iters; ++i) enqueue_iteration(false, opt.warm_start != 0);
    HIPCHK(hipStreamEndCapture(st, &graph));
    HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
    graph_iters = n_iters;
    graph_pipe = pipe_on;
  }

  // run n plain iterations; timed=true launches eagerly with HIP events around the projection kernel
  void iterate(int n, double* eig_ms, bool sync = true) {
    if (n <= 0) return;
    if (eig_ms) {
      while ((int)ev.size() < 2 * n) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
      for (int i = 0; i < n; ++i) { enqueue_iteration(false, next_is_warm(), ev[2 * i], ev[2 * i + 1]); ++iters_done; }
      HIPCHK(hipStreamSynchronize(st));
      double tot = 0;
      for (int i = 0; i < n; ++i) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); tot += ms; }
      *eig_ms = tot;
      t_eig += tot * 1e-3;
      return;
    }
    // hipGraph replay of kGraphIters warm iterations at a time; cold iterations and remainders eagerly
    int left = n;
    while (left > 0) {
      bool can_warm = opt.warm_start != 0 && iters_done > 0 && since_cold < kColdPeriod;
      static const bool no_graph = [] { const char* e = std::getenv("NNSDP_NO_GRAPH"); return e && std::atoi(e) != 0; }();   // diagnostic: eager launches only
      // (clique-sharded: only over RCCL and only when the probe in set_comm replayed a captured all-reduce; every rank takes the
      // same branch - the counters deciding it are replicated - so the collective inside the graph is entered by all of them)
      if (!no_graph && (!sharded || rccl_graph_ok) && big_idx.empty() && can_warm && left >= giters && kColdPeriod - since_cold >= giters) {
        build_graph(giters);
        HIPCHK(hipGraphLaunch(gexec, st));
        ++graph_launches;
        since_cold += giters; iters_done += giters; left -= giters;
      } else {
        enqueue_iteration(false, next_is_warm());
        ++iters_done; --left;
      }
    }
    if (sync) HIPCHK(hipStreamSynchronize(st));
  }

  // one iteration with residual accumulation; fills last_*.  Split in two so that a batch handle can have the
  // check iterations of several SDPs in flight on their streams at once.
  // (the control numbers and the stage's counters land in PINNED host memory, so that the check iteration - a dozen launches and two
  // copies - can be captured and replayed as one graph launch like the plain ones: ~100 us less per check, 2 us per iteration)
  double* acc_host = nullptr;
  int* stats_host = nullptr;
  hipGraphExec_t gexec_chk[2] = {nullptr, nullptr};      // the check iteration's graph, without / with the tile-parallel pipeline
  double tflag_host = 0.0, loop_t0 = 0.0;
  void check_enqueue() {
    const bool warm = next_is_warm();
    static const bool no_graph = [] { const char* e = std::getenv("NNSDP_NO_GRAPH"); return e && std::atoi(e) != 0; }();
    if (!no_graph && warm && !sharded && big_idx.empty()) {
      hipGraphExec_t& ge = gexec_chk[pipe_on ? 1 : 0];
      if (!ge) {
        hipGraph_t gr = nullptr;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        enqueue_iteration(true, true);
        HIPCHK(hipMemcpyAsync(acc_host, acc.p, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stats_host, d_stats.p, 14 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamEndCapture(st, &gr));
        HIPCHK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
        (void)hipGraphDestroy(gr);
      }
      HIPCHK(hipGraphLaunch(ge, st));
      ++iters_done;
      return;
    }
    enqueue_iteration(true, warm);
    ++iters_done;
    HIPCHK(hipMemcpyAsync(acc_host, acc.p, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pipe.ready && pipe_mode != 3) HIPCHK(hipMemcpyAsync(stats_host, d_stats.p, 14 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  void check_finish() {
    HIPCHK(hipStreamSynchronize(st));
    // rocSOLVER's convergence report of the library eigensolves, sticky since the solver was created.  Clique-sharded: only a block's
    // owner runs dsyevd, so the flag rides in the all-reduced control block (acc[7] >= 1024) and all ranks leave the loop together;
    // a rank-local exit would strand the others in the next iteration's all-reduce.
    if (split.failed()) throw HipError("projection kernel, two workgroups per block: a helper workgroup did not deliver its tiles in time, or ran on another XCD than its leader");
    if (ipc && ipc_err.download()[0] != 0) throw HipError("clique-sharded exchange over hipIpc: a peer did not publish its partial sum in time (rank stopped or not co-scheduled)");
    if (!big_idx.empty()) {
      if (sharded) big_fail = big_fail || acc_host[7] >= 1024.0;
      else big_fail = big_fail || big_flag.download()[0] != 0;
    }
    if (pipe.ready && pipe_mode != 3) {
      // the pipeline pays once the stage carries the block visits (late phase); while the sweeps run it is five empty launches per
      // iteration.  Decided from the counters of the window since the last check (deterministic: no timing enters), with hysteresis.
      const long long carried = (long long)stats_host[4] + stats_host[5] + stats_host[8];
      const long long all = carried + stats_host[6] + stats_host[7];
      const long long dc = carried - pipe_seen[0], da = all - pipe_seen[1];
      pipe_seen[0] = carried; pipe_seen[1] = all;
      if (da > 0) {
        if (!pipe_on && 10 * dc >= 7 * da) pipe_on = true;
        else if (pipe_on && 10 * dc < 4 * da) pipe_on = false;
      }
    }
    const double* a = acc_host;
    double z0n = 0;  // |z0| (scaled) is 1 when normalised; compute anyway
    for (double v : S.z0) z0n += v * v;
    z0n = std::sqrt(z0n);
    last_pres = std::sqrt(a[0]) / std::max({std::sqrt(a[1]), std::sqrt(a[2]), 1e-300});
    last_dres = std::sqrt(a[3]) / std::max({std::sqrt(a[4]), z0n, 1e-300});
    last_pobj = a[5] / (S.zscale * S.cscale);
    last_dobj = a[6] / (S.zscale * S.cscale);
  }
  void check_iteration() { check_enqueue(); check_finish(); }

  // inexact projections: Jacobi tolerance two orders below the current residual level
  void update_proj_tol() {
    if (opt.proj_tol > 0) return;
    static const double factor = [] { const char* e = std::getenv("NNSDP_PROJ_TOL_FACTOR"); return e ? std::atof(e) : 0.01; }();   // diagnostic override
    static const double cap = [] { const char* e = std::getenv("NNSDP_PROJ_TOL_CAP"); return e ? std::atof(e) : 1e-4; }();   // (diagnostic override.  1e-3 was tried in round 4: sweeps per visit 0.38 -> 0.14 on W40-D20, solves 3-7 % shorter, iteration counts -10 % .. +1 % over six problems, profiles/r04_proj_tol_cap.log - and the W10-D5 safety query's converged objective moved 2.6e-4 away from the oracle's, outside that parity test's 1e-4: not adopted)
    double t = std::min(cap, std::max(1e-9, factor * std::max(last_pres, last_dres)));
    if (t < 0.5 * proj_tol || t > 2.0 * proj_tol) {
      proj_tol = t;
      HIPCHK(hipMemcpyAsync(scal.p + 2, &proj_tol, sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  }

  void set_sigma(double ns) {
    double sc[2] = {ns, sigma / ns};
    HIPCHK(hipMemcpyAsync(scal.p, sc, sizeof(sc), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    sigma = ns;
  }

  // cap < 0: run to opt.max_iters with the stopping tests; cap >= 0: advance exactly `cap` more iterations with the
  // same checks and sigma / tolerance adaptation but without stopping (bench burn-in)
  void loop_begin() {
    if (next_adapt == 0) next_adapt = opt.adapt_every;
    if (const char* e = std::getenv("NNSDP_TRACE_POLISH")) trace_polish = std::atoi(e);
  }
  // bookkeeping after a check iteration: projection tolerance, stopping tests, penalty adaptation.
  // Returns a status to stop with, or -1 to go on.
  int post_check(bool advance_only, double t0) {
    if (opt.verbose)
      std::fprintf(stderr, "[nnsdp] it %6lld pres %.3e dres %.3e obj %.8g dobj %.8g sigma %.3g\n", iters_done, last_pres,
                   last_dres, last_pobj, last_dobj, sigma);
    if (!(last_pres == last_pres) || !(last_dres == last_dres) || big_fail) return NNSDP_STATUS_NUMERICAL_ERROR;
    update_proj_tol();
    if (trace_polish > 0 && lead() && iters_done >= next_trace) {
      next_trace = iters_done + trace_polish;
      double tp = now_s();
      hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(S.ng, 256)), dim3(256), 0, st, S.ng, nu.p, d_sigma(), d_kappa(), gs.p);
      HIPCHK(hipStreamSynchronize(st));
      std::vector<double> gp = gs.download();
      bool ok = polish(gp);
      double o = 0.0;
      for (int i = 0; i < S.ng; ++i) o += S.c[i] * gp[i];
      std::fprintf(stderr, "[nnsdp] it %6lld t %.2f polished rho %.8g (ok %d shift %.2e) admm %.8g dobj %.8g pres %.1e dres %.1e polish_ms %.0f\n", iters_done,
                   now_s() - t0, o / (S.zscale * S.cscale), (int)ok, polish_shift, last_pobj, last_dobj, last_pres, last_dres, 1e3 * (now_s() - tp));
      if (cert_ready()) {      // the sparse route at the same iterate (tools/decision_timing.py reads both lines)
        tp = now_s();
        const SparseBound sb = sparse_bound();
        std::fprintf(stderr, "[nnsdp] it %6lld sparse rho %.10g (ok %d shift %.2e) dense %.10g sparse_ms %.3f\n", iters_done, sb.objective, (int)sb.certified,
                     sb.delta, o / (S.zscale * S.cscale), 1e3 * (now_s() - tp));
      }
    }
    // a target is decided at EVERY check iteration, the one on which the residual test would end the solve included: a solve that
    // converges at its first check (a hyperplane direction whose optimum is gout = 0) still answers the question it was asked
    if (!advance_only && target_mode != NNSDP_TARGET_OFF) {
      const int ts = target_check();
      if (ts >= 0) return ts;
    }
    if (!advance_only && last_pres <= opt.eps_rel && last_dres <= opt.eps_rel) return NNSDP_STATUS_OPTIMAL;
    // optional early stop on the CERTIFIED objective: the polished point is exactly feasible, so once it
    // is within cert_tol of the ADMM estimate of the optimum the certificate is as good as it gets
    // The polish costs about 75 iterations (10 ms at W40-D20), so it only runs once the free part of the test - the ADMM primal
    // and dual estimates agree within cert_tol - holds, and then at most every 10 % of the iterations done
    // (profiles/r02_polish_trace_*.log, tools/cert_rule_sim.py: the estimates oscillate by +-1e-3 long after the polished value is good enough).
    // The ADMM estimates are only as good as the residuals (they oscillate around the optimum with an amplitude of a few times
    // max(pres, dres)), so they are trusted at the cert_tol level once the residuals are a tenth of it: over the traced solves
    // every check point that passes all three conditions is within cert_tol of the true optimum (max 9.3e-4 for 1e-3), without
    // the residual condition one is 1.9e-3 off.
    if (!advance_only && opt.cert_tol > 0 && P.nout && iters_done >= next_cert && std::max(last_pres, last_dres) <= std::min(1e-3, 0.1 * opt.cert_tol) &&
        std::fabs(last_pobj - last_dobj) <= opt.cert_tol * std::max(std::fabs(last_pobj), std::fabs(last_dobj))) {
      next_cert = std::max<long long>(iters_done + 100, iters_done * 11 / 10);
      // clique-sharded: every rank reaches this point at the same iteration (the conditions above are all-reduced numbers and
      // replicated counters); rank 0 alone polishes and its verdict travels to everybody - ONE decision, so no rank can leave
      // the loop while another enters the next iteration's all-reduce
      std::vector<double> flag(2, 0.0);    // {stop, rank 0 failed}
      std::string err;
      if (lead()) {
        try {
          hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(S.ng, 256)), dim3(256), 0, st, S.ng, nu.p, d_sigma(), d_kappa(), gs.p);
          HIPCHK(hipStreamSynchronize(st));
          std::vector<double> gp = gs.download();
          if (polish(gp)) {
            double o = 0.0;
            for (int i = 0; i < S.ng; ++i) o += S.c[i] * gp[i];
            o /= (S.zscale * S.cscale);
            double ref = std::max(std::fabs(last_pobj), std::fabs(last_dobj));
            if (opt.verbose) std::fprintf(stderr, "[nnsdp] it %6lld certified rho %.8g  admm %.8g  dual %.8g\n", iters_done, o, last_pobj, last_dobj);
            if (o - std::min(last_pobj, last_dobj) <= opt.cert_tol * ref && std::fabs(last_pobj - last_dobj) <= opt.cert_tol * ref) {
              flag[0] = 1.0;
              cert_gp = gp; cert_shift = polish_shift; cert_iter = iters_done;      // finish() reuses this polish (same iterate): 11 ms at W40-D20
            }
          }
        } catch (const std::exception& e) {
          if (!sharded) throw;
          err = e.what(); flag[1] = 1.0;
        }
      }
      allreduce_host(flag);
      if (flag[1] != 0.0) throw HipError(lead() ? err : std::string("rank 0 failed while polishing the certificate"));
      if (flag[0] != 0.0) return NNSDP_STATUS_OPTIMAL;
    }
    if (!advance_only && opt.max_time > 0 && (sharded ? std::fmod(acc_host[7], 1024.0) > 0.0 : now_s() - t0 > opt.max_time)) return NNSDP_STATUS_TIME_LIMIT;
    // stall detector (MOSEK's SLOW_PROGRESS analogue): no 10 % improvement of the larger residual in 50 000 iterations
    {
      double worst = std::max(last_pres, last_dres);
      if (worst < 0.9 * best_res) { best_res = worst; best_iter = iters_done; }
      else if (!advance_only && iters_done - best_iter >= 50000) return NNSDP_STATUS_SLOW_PROGRESS;
    }
    // residual balancing on a geometric schedule (adapting at a fixed period makes sigma oscillate)
    // NNSDP_SIGMA_RULE=1 (diagnostic): the balancing ratio smoothed over the checks, geometric back-off only after an actual
    // change.  Fixes single traces (W40-D20 Double: sigma sat at 0.0027 from iteration 3 250 to 7 250 with pres = 3-4 x dres
    // because the one look at 4 900 fell on a dres spike) and changes nothing over 15 problems (negative result 15),
    // so the default stays round 1's rule.
    static const int sigma_rule = [] { const char* e = std::getenv("NNSDP_SIGMA_RULE"); return e ? std::atoi(e) : 0; }();
    {
      const double lr = 0.5 * std::log(std::max(last_pres, 1e-300) / std::max(last_dres, 1e-300));
      lr_ema = have_ema ? 0.7 * lr_ema + 0.3 * lr : lr;
      have_ema = true;
    }
    if (opt.adapt_every > 0 && iters_done >= next_adapt) {
      static const double geom = [] { const char* e = std::getenv("NNSDP_SIGMA_GEOM"); return e ? std::atof(e) : 1.5; }();   // diagnostic
      static const double powr = [] { const char* e = std::getenv("NNSDP_SIGMA_POW"); return e ? std::atof(e) : 1.0; }();    // diagnostic
      if (sigma_rule == 0) {
        next_adapt = std::max<long long>(iters_done + 2LL * opt.adapt_every, (long long)(iters_done * geom));
        double ratio = std::pow(std::sqrt(std::max(last_pres, 1e-300) / std::max(last_dres, 1e-300)), powr);
        if (ratio > 1.5 || ratio < 0.67) set_sigma(sigma * std::min(std::max(ratio, 0.2), 5.0));
      } else {
        const double ratio = std::exp(powr * lr_ema);
        if (ratio > 1.5 || ratio < 0.67) {
          set_sigma(sigma * std::min(std::max(ratio, 0.2), 5.0));
          next_adapt = std::max<long long>(iters_done + 2LL * opt.adapt_every, (long long)(iters_done * geom));
          have_ema = false;      // the residuals of the old penalty say nothing about the new one
        } else {
          next_adapt = iters_done + opt.adapt_every;
        }
      }
    }
    return -1;
  }
  int run_loop(long long cap = -1) {
    double t0 = now_s();
    int status = NNSDP_STATUS_ITERATION_LIMIT;
    const bool advance_only = cap >= 0;
    loop_t0 = advance_only ? 0.0 : t0;
    const long long limit = advance_only ? iters_done + cap : (long long)opt.max_iters;
    int ce = opt.check_every;
    loop_begin();
    while (iters_done < limit) {
      int n = (int)std::min<long long>(ce - 1, limit - iters_done - 1);
      iterate(n, nullptr);
      check_iteration();
      int st_ = post_check(advance_only, t0);
      if (st_ >= 0) { status = st_; break; }
    }
    t_solve += now_s() - t0;
    return status;
  }

  // ---- certificate polish -------------------------------------------------------------------
  // ADMM stops at a relative residual, so Z(gamma) is only approximately NSD.  The polish makes it NSD
  // to rounding with two exact moves in the solver's coordinates (a congruence of the reference's, so
  // definiteness carries over): (1) every coordinate i has a multiplier whose generator is a pure
  // negative diagonal on (i,i) (gin_i / gac1_t): raise them until Z_xx <= -margin; (2) reach queries:
  // gout only moves Z_aa, so the smallest feasible value follows from the Schur complement
  //   Z_aa - z_xa' Z_xx^-1 z_xa <= 0.
  // The result is a primal-feasible point: its objective is a valid (slightly conservative) bound.
  double polish_shift = 0.0, objective_admm = 0.0;
  std::vector<double> cert_gp;       // polished multipliers of the check that stopped the solve (cert_tol rule), valid at iteration cert_iter
  double cert_shift = 0.0;
  long long cert_iter = -1;
  void dense_from_gs(const std::vector<double>& gsh, DBuf<double>& Zt) {
    int n = pat.n;
    DBuf<double> gd, zd;
    gd.upload(gsh);
    zd.alloc(S.NE);
    if (Zt.n != (size_t)n * n) Zt.alloc((size_t)n * n);
    HIPCHK(hipMemsetAsync(Zt.p, 0, Zt.n * sizeof(double), st));
    hipLaunchKernelGGL(k_apply_A, dim3(cdiv((long long)S.NE * 16, kThreads)), dim3(kThreads), 0, st, S.NE, D.csr_ptr.p, D.csr_col.p,
                       D.csr_val.p, gd.p, D.z0.p, zd.p);
    hipLaunchKernelGGL(k_scatter_dense, dim3(cdiv(S.NE, 256)), dim3(256), 0, st, S.NE, n, D.erow.p, D.ecol.p, zd.p, Zt.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
  }
  // The two exact moves' tables: shift_gen[i] / dcoef[i] - the kept multiplier whose generator is a pure negative diagonal on the reduced
  // coordinate i and its (negative) coefficient there; jout / aout - gout and its coefficient on (a, a) (reach queries; -1 otherwise).
  // false: some coordinate has no such multiplier.
  bool shift_direction(std::vector<int>& shift_gen, std::vector<double>& dcoef, int& jout, double& aout) const {
    int n = pat.n, nx = n - 1;
    if (nx < 1) return false;
    // kept-generator index of the diagonal-shift multiplier of each reduced coordinate, and of gout
    std::vector<int> inv(P.ng, -1);
    for (int i = 0; i < S.ng; ++i) inv[S.keep[i]] = i;
    shift_gen.assign(nx, -1);
    for (int i = 0; i < P.Zdim - 1; ++i) {
      int ri = C.newpos[i];
      if (ri < 0 || ri >= nx) continue;
      int full = i < P.nin ? i : P.nin + P.nout + (i - P.nin);
      shift_gen[ri] = inv[full];
    }
    dcoef.assign(nx, 0.0);
    for (int i = 0; i < nx; ++i) {
      if (shift_gen[i] < 0) return false;
      dcoef[i] = op_entry(pat.pos(i, i), shift_gen[i]);
      if (!(dcoef[i] < 0.0)) return false;
    }
    jout = P.nout ? inv[P.nin] : -1;
    aout = jout >= 0 ? op_entry(pat.pos(nx, nx), jout) : 0.0;
    if (P.nout && !(aout < 0.0)) return false;
    return true;
  }
  double op_entry(int e, int g) const {   // A_s[e, g]
    for (int q = S.csr_ptr[e]; q < S.csr_ptr[e + 1]; ++q) if (S.csr_col[q] == g) return S.csr_val[q];
    return 0.0;
  }
  bool polish(std::vector<double>& gsh) {
    int n = pat.n, nx = n - 1;
    std::vector<int> shift_gen;
    std::vector<double> dcoef;
    int jout = -1;
    double aout = 0.0;
    if (!shift_direction(shift_gen, dcoef, jout, aout)) return false;
    auto entry = [&](int e, int g) { return op_entry(e, g); };
    DBuf<double> Zt, W, Dv, Ev;
    DBuf<rocblas_int> info;
    info.alloc(1); Dv.alloc(nx); Ev.alloc(nx); W.alloc((size_t)nx * nx);
    if (jout >= 0) gsh[jout] = 0.0;
    dense_from_gs(gsh, Zt);
    // (1) eigen-decomposition of the x-block: Z_xx = Q diag(lam) Q'
    HIPCHK(hipMemcpy2D(W.p, (size_t)nx * sizeof(double), Zt.p, (size_t)n * sizeof(double), (size_t)nx * sizeof(double), nx, hipMemcpyDeviceToDevice));
    RBCHK(rocsolver_dsyevd(roc->h, jout >= 0 ? rocblas_evect_original : rocblas_evect_none, rocblas_fill_lower, nx, W.p, nx, Dv.p, Ev.p, info.p));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> lam = Dv.download();
    double lmax = lam.back();
    const double margin = 1e-9;
    double delta = lmax > -margin ? lmax + margin + 1e-3 * std::fabs(lmax) : 0.0;
    if (jout >= 0) {
      // uniform shift delta >= delta_min chosen to MINIMISE the certified objective
      //   f(delta) = Z_aa + kappa*delta + sum_i c_i^2 / (mu_i + delta),   mu = -lam, c = Q' z_xa
      // (convex on delta > -min mu): near convergence Z_xx is NSD but almost singular, and a small extra
      // shift is much cheaper than the Schur term along the near-null directions
      std::vector<double> Q = W.download(), zall = Zt.download();
      std::vector<double> cvec(nx, 0.0);
      for (int i = 0; i < nx; ++i) {
        double sdot = 0.0;
        const double* qi = &Q[(size_t)i * nx];
        for (int r = 0; r < nx; ++r) sdot += qi[r] * zall[(size_t)nx * n + r];
        cvec[i] = sdot * sdot;
      }
      double kappa = 0.0;
      for (int i = 0; i < nx; ++i) kappa += entry(pat.pos(nx, nx), shift_gen[i]) / (-dcoef[i]);
      auto fprime = [&](double dl) {
        double sder = kappa;
        for (int i = 0; i < nx; ++i) { double m = -lam[i] + dl; sder -= cvec[i] / (m * m); }
        return sder;
      };
      double lo = delta;
      if (fprime(lo) < 0.0) {
        double hi = std::max(2.0 * lo, 1e-12);
        int guard = 0;
        while (fprime(hi) < 0.0 && guard++ < 200) hi *= 2.0;
        for (int itb = 0; itb < 100; ++itb) { double mid = 0.5 * (lo + hi); if (fprime(mid) < 0.0) lo = mid; else hi = mid; }
        delta = hi;
      }
    }
    polish_shift = delta;
    if (delta > 0.0) {
      for (int i = 0; i < nx; ++i) gsh[shift_gen[i]] += delta / (-dcoef[i]);
      dense_from_gs(gsh, Zt);
    }
    if (jout < 0) return true;
    // (2) Schur complement for gout:  -Z_xx = L L',  need Z_aa + |L^-1 z_xa|^2 + gout * aout <= 0
    std::vector<double> Zh((size_t)n * n);
    HIPCHK(hipMemcpy(Zh.data(), Zt.p, Zh.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> Nx((size_t)nx * nx);
    for (int j = 0; j < nx; ++j)
      for (int i = 0; i < nx; ++i) Nx[(size_t)j * nx + i] = -Zh[(size_t)j * n + i];
    HIPCHK(hipMemcpy(W.p, Nx.data(), Nx.size() * sizeof(double), hipMemcpyHostToDevice));
    RBCHK(rocsolver_dpotrf(roc->h, rocblas_fill_lower, nx, W.p, nx, info.p));
    HIPCHK(hipStreamSynchronize(st));
    if (info.download()[0] != 0) return false;
    std::vector<double> zxa(nx);
    for (int i = 0; i < nx; ++i) zxa[i] = Zh[(size_t)nx * n + i];
    DBuf<double> yv;
    yv.upload(zxa);
    RBCHK(rocblas_dtrsv(roc->h, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, nx, W.p, nx, yv.p, 1));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> y = yv.download();
    double q = 0.0;
    for (double v : y) q += v * v;
    double need = (Zh[(size_t)nx * n + nx] + q) / (-aout);
    gsh[jout] = std::max(0.0, need * (1.0 + 1e-12) + 1e-300);
    return true;
  }

  // ---- sparse certified bound ---------------------------------------------------------------
  // The same two exact moves as polish(), evaluated through the sparse Cholesky of -Z on the clique pattern (cert_plan.hpp,
  // cert_chol.hpp) instead of dense dsyevd / dpotrf: gout = 0, kSbCand candidates gamma + delta_b s along the diagonal-shift direction
  // s_i = 1 / (-dcoef_i) - delta = 0 and a geometric grid over twelve decades below `top` - become kSbCand NE-vectors in one launch
  // and are factored side by side in one launch.  top = (Gershgorin bound of Z_xx)+ + margin + |z_xa| / sqrt(kappa) brackets the
  // minimiser of polish()'s f(delta) = Z_aa + kappa delta + z_xa' (-Z_xx + delta I)^-1 z_xa: the first two terms make Z_xx <= -margin
  // for certain, and f' >= 0 from |z_xa| / sqrt(kappa) past that point on.  As in polish() a candidate must have Z_xx <= -margin I
  // (margin = 1e-9: the kernel factors -Z_xx - margin I, so its Schur complement errs on the safe side); it is then exactly feasible
  // once gout takes that Schur complement (a safety query has no gout: the Schur complement itself must be negative), the one with
  // the smallest objective is kept, and a second round of candidates between its neighbours refines it.  Deterministic (fixed grids,
  // fixed-order kernels), no host library, and nothing of the iteration state is touched (gs and the buffers below are scratch).
  static constexpr int kSbCand = 16;
  int target_mode = NNSDP_TARGET_OFF;
  double target = 0.0;
  long long sparse_calls = 0;
  int cert_state = 0;                  // 0: plan not built yet, 1: ready, -1: unsupported (front above kCertFrontMax, or no shift direction)
  std::unique_ptr<CertDev> cert;
  std::vector<int> sb_shift_gen;
  std::vector<double> sb_dcoef;
  int sb_jout = -1;
  double sb_aout = 0.0, sb_kappa = 0.0;   // kappa: what a unit shift adds to Z_aa
  static constexpr double kSbMargin = 1e-9;       // polish()'s margin on Z_xx
  DBuf<double> sb_g, sb_z;
  struct SparseBound {
    bool certified = false;
    double objective = 0.0, delta = 0.0;       // objective in the units of nnsdp_result.objective
    std::vector<double> gsh;                    // the multipliers (solver coordinates), gout included
  };
  bool cert_ready() {
    if (cert_state == 0) {
      cert_state = -1;
      if (const char* e = std::getenv("NNSDP_SPARSE_BOUND")) if (std::atoi(e) == 0) return false;      // (diagnostic: the dense route everywhere)
      CertPlan pl = make_cert_plan(pat);
      if (pl.supported && pl.n_super > 0 && shift_direction(sb_shift_gen, sb_dcoef, sb_jout, sb_aout)) {
        sb_kappa = 0.0;
        for (int i = 0; i < pat.n - 1; ++i) sb_kappa += op_entry(pat.pos(pat.n - 1, pat.n - 1), sb_shift_gen[i]) / (-sb_dcoef[i]);
        cert.reset(new CertDev());
        cert->upload(std::move(pl));
        sb_g.alloc((size_t)kSbCand * S.ng);
        sb_z.alloc((size_t)kSbCand * S.NE);
        cert->reserve(kSbCand);
        cert_state = 1;
      }
    }
    return cert_state == 1;
  }
  SparseBound sparse_bound() {
    SparseBound R;
    if (!cert_ready()) return R;
    ++sparse_calls;
    const int ng = S.ng, nx = pat.n - 1, NE = S.NE, B = kSbCand;
    hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(ng, 256)), dim3(256), 0, st, ng, nu.p, d_sigma(), d_kappa(), gs.p);
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> g0 = gs.download();
    if (sb_jout >= 0) g0[sb_jout] = 0.0;
    // Z(gamma) itself, for the Gershgorin bound of its x-block (the upper end of the shift grid) and the scale of the margin
    HIPCHK(hipMemcpyAsync(sb_g.p, g0.data(), (size_t)ng * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_apply_A, dim3(cdiv((long long)NE * 16, kThreads)), dim3(kThreads), 0, st, NE, D.csr_ptr.p, D.csr_col.p, D.csr_val.p,
                       sb_g.p, D.z0.p, sb_z.p);
    HIPCHK(hipGetLastError());
    std::vector<double> zv(NE);
    HIPCHK(hipMemcpyAsync(zv.data(), sb_z.p, (size_t)NE * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> dg(nx, 0.0), off(nx, 0.0);
    double zxa2 = 0.0;
    for (int e = 0; e < NE; ++e) {
      const int i = pat.erow[e], j = pat.ecol[e];
      if (i >= nx) { if (j < nx) zxa2 += 0.5 * zv[e] * zv[e]; continue; }
      if (i == j) dg[i] = zv[e];
      else { const double v = std::fabs(zv[e]) * M_SQRT1_2; off[i] += v; off[j] += v; }
    }
    double gersh = -1e300, scale = 0.0;
    for (int i = 0; i < nx; ++i) { gersh = std::max(gersh, dg[i] + off[i]); scale = std::max(scale, std::fabs(dg[i]) + off[i]); }
    if (!(scale > 0.0) || !(scale < 1e300)) return R;
    const double top = std::max(gersh, 0.0) * (1.0 + 1e-9) + kSbMargin + (sb_kappa > 0.0 ? std::sqrt(zxa2 / sb_kappa) : 1e-3 * scale), margin = 1e-12 * scale;
    std::vector<double> G((size_t)B * ng), obj(B);
    std::vector<int> okv(B);
    std::vector<double> sch(B);
    // one round: candidates at the shifts dl[0 .. B-1]; returns the best feasible one (-1: none)
    auto round = [&](const std::vector<double>& dl) {
      for (int b = 0; b < B; ++b) {
        double* gb = &G[(size_t)b * ng];
        std::copy(g0.begin(), g0.end(), gb);
        if (dl[b] > 0.0) for (int i = 0; i < nx; ++i) gb[sb_shift_gen[i]] += dl[b] / (-sb_dcoef[i]);
      }
      HIPCHK(hipMemcpyAsync(sb_g.p, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_apply_A_multi, dim3(cdiv((long long)NE * 16, kThreads), B), dim3(kThreads), 0, st, NE, D.csr_ptr.p, D.csr_col.p,
                         D.csr_val.p, sb_g.p, (long long)ng, D.z0.p, sb_z.p, (long long)NE);
      HIPCHK(hipGetLastError());
      cert->launch(sb_z.p, NE, B, st, kSbMargin);
      HIPCHK(hipMemcpyAsync(okv.data(), cert->ok.p, B * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(sch.data(), cert->schur.p, B * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      int best = -1;
      for (int b = 0; b < B; ++b) {
        obj[b] = 1e300;
        if (!okv[b] || !(sch[b] == sch[b])) continue;
        double* gb = &G[(size_t)b * ng];
        if (sb_jout >= 0) gb[sb_jout] = std::max(0.0, sch[b] / (-sb_aout) * (1.0 + 1e-12) + 1e-300);
        else if (!(sch[b] <= -margin)) continue;
        double o = 0.0;
        for (int i = 0; i < ng; ++i) o += S.c[i] * gb[i];
        obj[b] = o;
        if (best < 0 || o < obj[best]) best = b;
      }
      return best;
    };
    auto keep = [&](int b, const std::vector<double>& dl) {
      const double o = obj[b] / (S.zscale * S.cscale);
      if (R.certified && !(o < R.objective)) return;
      R.certified = true; R.objective = o; R.delta = dl[b];
      R.gsh.assign(G.begin() + (size_t)b * ng, G.begin() + (size_t)(b + 1) * ng);
    };
    std::vector<double> dl(B, 0.0);
    const double ratio = std::pow(1e12, 1.0 / (B - 2));
    for (int b = B - 1; b >= 1; --b) dl[b] = b == B - 1 ? top : dl[b + 1] / ratio;
    const int b1 = round(dl);
    if (b1 < 0) return R;
    keep(b1, dl);
    // second round: between the neighbours of the best
    const double hi = b1 < B - 1 ? dl[b1 + 1] : dl[b1];
    const double lo = b1 > 0 && dl[b1 - 1] > 0.0 ? dl[b1 - 1] : 1e-6 * hi;
    std::vector<double> d2(B);
    for (int b = 0; b < B; ++b) d2[b] = lo * std::pow(hi / lo, (b + 1.0) / (B + 1.0));
    const int b2 = round(d2);
    if (b2 >= 0) keep(b2, d2);
    return R;
  }
  // the target rule of post_check: 5 / 6 to stop with, -1 to go on (target_mode != OFF)
  static constexpr double kTargetUnreachM = 3.8;   // twice the smallest m that is safe on every traced check point
  int target_check() {
    const bool reach = target_mode == NNSDP_TARGET_OBJECTIVE;
    if (!reach || last_pobj <= target) {
      bool have = false;
      double o = 0.0, sh = 0.0;
      std::vector<double> gp;
      if (cert_ready()) {
        SparseBound sb = sparse_bound();
        have = sb.certified; o = sb.objective; sh = sb.delta; gp = std::move(sb.gsh);
      } else if (iters_done >= next_cert && std::max(last_pres, last_dres) <= 1e-3) {
        // no sparse route for this pattern: the dense polish, on the schedule of the cert_tol rule
        next_cert = std::max<long long>(iters_done + 100, iters_done * 11 / 10);
        hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(S.ng, 256)), dim3(256), 0, st, S.ng, nu.p, d_sigma(), d_kappa(), gs.p);
        HIPCHK(hipStreamSynchronize(st));
        gp = gs.download();
        have = polish(gp) && (P.nout != 0);     // (a safety query's dense polish does not look at the row of a: no certificate from it)
        sh = polish_shift;
        if (have) {
          for (int i = 0; i < S.ng; ++i) o += S.c[i] * gp[i];
          o /= (S.zscale * S.cscale);
        }
      }
      if (have && (!reach || o <= target)) {
        if (opt.verbose) std::fprintf(stderr, "[nnsdp] it %6lld target certified: bound %.8g target %.8g\n", iters_done, o, target);
        cert_gp = std::move(gp); cert_shift = sh; cert_iter = iters_done;      // finish() checks exactly this point
        return NNSDP_STATUS_TARGET_CERTIFIED;
      }
    }
    if (reach && std::max(last_pres, last_dres) <= 1e-3 &&
        std::min(last_pobj, last_dobj) - target > kTargetUnreachM * std::max(last_pres, last_dres) * std::max(std::fabs(last_pobj), std::fabs(last_dobj)))
      return NNSDP_STATUS_TARGET_UNREACHABLE;
    return -1;
  }
  void set_target(int mode, double tg) {
    if (mode < NNSDP_TARGET_OFF || mode > NNSDP_TARGET_FEASIBLE) throw std::invalid_argument("unrecognized target mode");
    if (sharded) throw std::invalid_argument("a clique-sharded solver takes no target");
    if (mode == NNSDP_TARGET_OBJECTIVE && !P.nout) throw std::invalid_argument("NNSDP_TARGET_OBJECTIVE needs a reach query (a safety query takes NNSDP_TARGET_FEASIBLE)");
    if (mode == NNSDP_TARGET_OBJECTIVE && !(tg == tg)) throw std::invalid_argument("the target is NaN");
    target_mode = mode; target = tg;
  }
  // rigorous bound of the current iterate on request: the sparse route, or the dense polish where the pattern has none
  void certified_bound(double* objective, double* gamma, int32_t* certified, double* ms) {
    const double t_in = now_s();
    bool have = false;
    double o = 0.0;
    std::vector<double> gp;
    if (cert_ready()) {
      SparseBound sb = sparse_bound();
      have = sb.certified; o = sb.objective; gp = std::move(sb.gsh);
    } else {
      hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(S.ng, 256)), dim3(256), 0, st, S.ng, nu.p, d_sigma(), d_kappa(), gs.p);
      HIPCHK(hipStreamSynchronize(st));
      gp = gs.download();
      have = polish(gp) && (P.nout != 0);
      if (have) {
        for (int i = 0; i < S.ng; ++i) o += S.c[i] * gp[i];
        o /= (S.zscale * S.cscale);
      }
    }
    if (ms) *ms = 1e3 * (now_s() - t_in);
    if (certified) *certified = have ? 1 : 0;
    if (objective) *objective = have ? o : std::nan("");
    if (gamma) {
      std::fill(gamma, gamma + P.ng, 0.0);
      if (have) {
        double gscale = 1.0;
        for (int i = 0; i < S.ng; ++i) { gamma[S.keep[i]] = gp[i] * S.ecol[i] / S.zscale; gscale = std::max(gscale, gamma[S.keep[i]]); }
        // coordinates removed by the normalisation: their box multipliers are cost-free and exact in the limit of infinity
        if (opt.normalize && P.query_kind == NNSDP_QUERY_REACH) {
          for (int i = 0; i < P.nin; ++i) if (C.newpos[i] < 0) gamma[i] = 1e8 * gscale;
          for (int t = 0; t < P.acdim; ++t) if (C.newpos[P.nin + t] < 0) gamma[P.nin + P.nout + t] = 1e8 * gscale;
        }
      }
    }
  }

  // The certificate (gamma, eigmax) is computed ONCE: in clique-sharded mode by rank 0 alone, whose result travels to every
  // rank through one all-reduce (the others contribute zeros) - identical on all ranks by construction, whatever the
  // libraries behind the polish round like.  finish() is therefore a collective call in sharded mode.
  void certificate(std::vector<double>& gam, double& lmax, bool& polished, DBuf<double>& Zd) {
    int ng = S.ng;
    hipLaunchKernelGGL(k_extract_gamma, dim3(cdiv(ng, 256)), dim3(256), 0, st, ng, nu.p, d_sigma(), d_kappa(), gs.p);
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> gsh = gs.download();
    {
      double o = 0.0;
      for (int i = 0; i < ng; ++i) o += S.c[i] * gsh[i];
      objective_admm = o / (S.zscale * S.cscale);
    }
    const bool tm = std::getenv("NNSDP_SETUP_TIMING") != nullptr;
    double tl = now_s();
    auto lap = [&](const char* what) { if (tm) { const double t = now_s(); std::fprintf(stderr, "[nnsdp finish] %-28s %7.2f ms\n", what, 1e3 * (t - tl)); tl = t; } };
    polished = false;
    if (opt.polish) {
      if (cert_iter == iters_done && cert_gp.size() == gsh.size()) { gsh = cert_gp; polish_shift = cert_shift; polished = true; }
      else {
        std::vector<double> gp = gsh;
        polished = polish(gp);
        if (polished) gsh = gp;
      }
    }
    lap("polish");
    gam.assign(P.ng, 0.0);
    for (int i = 0; i < ng; ++i) gam[S.keep[i]] = gsh[i] * S.ecol[i] / S.zscale;
    std::vector<int> elim;  // coordinates removed by the normalisation (full gamma index of their box multiplier): -> "large enough"
    if (opt.normalize && P.query_kind == NNSDP_QUERY_REACH) {
      for (int i = 0; i < P.nin; ++i)
        if (C.newpos[i] < 0) elim.push_back(i);                       // degenerate input box x1min[i] == x1max[i]
      for (int t = 0; t < P.acdim; ++t)
        if (C.newpos[P.nin + t] < 0) elim.push_back(P.nin + P.nout + t);
    }
    double gscale = 1.0;
    for (double v : gam) gscale = std::max(gscale, v);
    // multipliers of eliminated neurons are cost-free: raise them until eigmax(Z) stops improving
    double best_l = 1e300, best_big = 0.0, prev_l = 1e300;
    int ntrial = elim.empty() ? 1 : 6;
    for (int trial = 0; trial < ntrial; ++trial) {
      double big = elim.empty() ? 0.0 : gscale * std::pow(100.0, trial + 1);
      for (int t : elim) gam[t] = big;
      full->assemble(gam, Zd, st);
      lap("assemble Z(gamma)");
      lmax = lambda_max_dense(roc->h, Zd, P.Zdim);
      lap("eigmax (dense)");
      if (lmax < best_l) { best_l = lmax; best_big = big; }
      if (lmax <= 1e-7 || (trial > 0 && lmax >= 0.9 * prev_l)) break;
      prev_l = lmax;
    }
    if (!elim.empty() && gam[elim[0]] != best_big) {
      for (int t : elim) gam[t] = best_big;
      full->assemble(gam, Zd, st);
      lmax = lambda_max_dense(roc->h, Zd, P.Zdim);
    }
  }

  void finish(nnsdp_result* r, int status) {
    // final Z and certificate in the reference's coordinates.  Clique-sharded: this preparation is rank-local and can fail on ANY
    // rank (host allocation in the builder thread, upload), and the certificate below is a collective - so the outcome of the
    // preparation travels first, and every rank throws together instead of one leaving the others inside the all-reduce
    {
      std::vector<double> pflag(1, 0.0);
      std::string perr;
      try {
        if (!full) {
          if (full_fut.valid()) { full = full_fut.get(); full->upload(); }
          else {
            full.reset(new FullOperator());
            nnsdp_problem pp = problem_view();
            full->build(&pp);
          }
        }
      } catch (const std::exception& e) {
        if (!sharded) throw;
        perr = e.what(); pflag[0] = 1.0;
      }
      allreduce_host(pflag);
      if (pflag[0] != 0.0) throw HipError(!perr.empty() ? perr : std::string("another rank failed while preparing the certificate's operator"));
    }
    std::vector<double> gam(P.ng, 0.0);
    DBuf<double> Zd;
    double lmax = 0;
    bool polished = false;
    if (!sharded) certificate(gam, lmax, polished, Zd);
    else {
      std::vector<double> pack(P.ng + 5, 0.0);     // gamma | eigmax | objective of the raw iterate | polish shift | polished | failed
      std::string err;
      if (rank == 0) {
        try {
          certificate(gam, lmax, polished, Zd);
          std::copy(gam.begin(), gam.end(), pack.begin());
          pack[P.ng] = lmax; pack[P.ng + 1] = objective_admm; pack[P.ng + 2] = polish_shift; pack[P.ng + 3] = polished ? 1.0 : 0.0;
        } catch (const std::exception& e) { err = e.what(); std::fill(pack.begin(), pack.end(), 0.0); pack[P.ng + 4] = 1.0; }
      }
      allreduce_host(pack);
      if (pack[P.ng + 4] != 0.0) throw HipError(rank == 0 ? err : std::string("rank 0 failed while computing the certificate"));
      gam.assign(pack.begin(), pack.begin() + P.ng);
      lmax = pack[P.ng]; objective_admm = pack[P.ng + 1]; polish_shift = pack[P.ng + 2]; polished = pack[P.ng + 3] != 0.0;
      if (r->Z) full->assemble(gam, Zd, st);      // (fixed-order kernels: the same Z on every rank)
    }
    const double* gp = gam.data();
    if (r->gamma_in) std::memcpy(r->gamma_in, gp, P.nin * sizeof(double));
    if (r->gamma_out && P.nout) r->gamma_out[0] = gp[P.nin];
    if (r->gamma_ac1) std::memcpy(r->gamma_ac1, gp + P.nin + P.nout, P.n1 * sizeof(double));
    if (r->gamma_ac2) std::memcpy(r->gamma_ac2, gp + P.nin + P.nout + P.n1, P.n2 * sizeof(double));
    if (r->Z) HIPCHK(hipMemcpy(r->Z, Zd.p, (size_t)P.Zdim * P.Zdim * sizeof(double), hipMemcpyDeviceToHost));
    double obj = 0;
    if (P.nout) obj = gam[P.nin];
    else for (double v : gam) obj += v;
    r->objective = obj;
    r->status = status;
    r->iters = (int)iters_done;
    r->pres = last_pres;
    r->dres = last_dres;
    r->lambda_max = lmax;
    r->t_setup = t_setup;
    r->t_solve = t_solve;
    r->t_total = now_s() - t_create0;
    r->t_eig = t_eig;
    r->n_cliques = ncl;
    r->max_clique = nmax;
    long long f = 0, b = 0;
    for (int k = 0; k < ncl; ++k) { f += 10LL * cn[k] * cn[k] * cn[k]; b += 16LL * cn[k] * cn[k]; }
    r->eig_flops_per_iter = f;
    r->eig_bytes_per_iter = b;
    if (pipe.ready && std::getenv("NNSDP_PIPE_DEBUG")) {
      // (diagnostic) the pipeline's last decision per block: why a block is left to the sweeps
      std::vector<nnsdp::PipeRec> rc(pipe.nblocks);
      HIPCHK(hipMemcpy(rc.data(), pipe.drec, rc.size() * sizeof(nnsdp::PipeRec), hipMemcpyDeviceToHost));
      std::vector<int> rsv = d_rstate.download();
      for (int k = 0; k < pipe.nblocks; ++k) {
        const nnsdp::PipeRec& q = rc[k];
        const double pred0 = 1.5 * std::sqrt(q.off2) * std::sqrt(q.k2) + q.k2 * std::sqrt(q.kd2) / 3.0;
        std::fprintf(stderr, "[nnsdp pipe] block %d (n %d) state word %08x: mode %d |K| %.2e off %.2e second/third order %.2e unresolved ++ %.2e -- %.2e +- %.2e accepted level %.2e r2 %.1e\n",
                     k, cn[std::min(k0 + k, ncl - 1)], (unsigned)rsv[4 * (k0 + k)], q.mode, std::sqrt(q.k2), std::sqrt(q.off2), pred0, std::sqrt(q.unpp), std::sqrt(q.unnn), std::sqrt(q.unx), q.accT, q.r2);
      }
    }
    {
      std::vector<int> stv = d_stats.download();
      for (int i = 0; i < 5; ++i) r->refine_blocks[i] = stv[4 + i];
      if (opt.verbose || std::getenv("NNSDP_REFINE_STATS")) std::fprintf(stderr, "[nnsdp] refinement rejections by dominant term: second/third order %d, cross-sign or indefinite pairs %d, same-sign pairs on both sides %d; exact pair rotations: %d before accepted steps, %d before rejected ones\n", stv[9], stv[10], stv[11], stv[12], stv[13]);
      r->objective_admm = objective_admm;
    r->polish_shift = polished ? polish_shift : -1.0;
    r->avg_sweeps = iters_done > 0 ? (double)stv[0] / ((double)iters_done * ncl) : 0.0;
      if (opt.verbose && stv.size() >= 4 && stv[3] > 0) std::fprintf(stderr, "[nnsdp] nontrivial rotations: %.2f %% of pair visits\n", 100.0 * stv[2] / stv[3]);
    }
  }

  // a nnsdp_problem view over the deep copy (column-major M rebuilt)
  std::vector<double> Mpack;
  nnsdp_problem problem_view() {
    Mpack.clear();
    for (int k = 0; k < P.K; ++k) {
      int r = P.xdims[k + 1], c = P.xdims[k];
      for (int j = 0; j < c; ++j)
        for (int i = 0; i < r; ++i) Mpack.push_back(P.W[k][(size_t)i * c + j]);
      for (int i = 0; i < r; ++i) Mpack.push_back(P.b[k][i]);
    }
    nnsdp_problem pp{};
    pp.K = P.K; pp.xdims = P.xdims.data(); pp.M = Mpack.data();
    pp.x1min = P.x1min.data(); pp.x1max = P.x1max.data(); pp.acymin = P.acymin.data(); pp.acymax = P.acymax.data();
    pp.smin = P.smin.data(); pp.smax = P.smax.data(); pp.beta = P.beta; pp.query_kind = P.query_kind; pp.out_kind = P.out_kind;
    pp.activ = P.activ;
    pp.normal = P.normal.empty() ? nullptr : P.normal.data();
    pp.yc = P.yc.empty() ? nullptr : P.yc.data();
    pp.invP = P.invP.empty() ? nullptr : P.invP.data();
    pp.S = P.S.empty() ? nullptr : P.S.data();
    return pp;
  }
};

// ------------------------------------------------------------------------------------------ ABI
// ---------------------------------------------------------------------------------------------
// Batch handle: several independent SDPs (beta sweep of experiments/scale.jl:28, hyperplane directions of
// NnSdp.findReach2Dpoly, the sub-queries of an ACAS clause) advanced in lockstep with ONE launch per stage for all
// of them - blockIdx.y (small kernels) or a block map (projection) selects the SDP.  A single W40-D20 SDP keeps
// 19 of 256 CUs busy; one stream per SDP fills the chip only nominally, because every dependent launch of every
// stream pays the queue-scheduling latency of 13 queues (measured: 13 streams reach 3.1x the single-SDP rate).
// The solvers stay owned by the caller; plain iterations run through the batch, check iterations (one in
// check_every) run on the solvers' own streams, all in flight together.
// ---------------------------------------------------------------------------------------------
struct nnsdp_batch {
  std::vector<nnsdp_solver*> all;      // as given
  std::vector<nnsdp_solver*> act;      // still iterating
  std::vector<int> status;             // per solver of `all`, -1 while active
  hipStream_t st = nullptr;
  DBuf<IterArgs> d_it;
  DBuf<ProjArgs> d_pw, d_pc;           // warm / cold projection arguments
  DBuf<int2> d_map;
  // members of a solver family with a dense inverse: ONE pass over their common M^-1 per kFusedWidth members (k_minv_family) instead
  // of a tiled product per member.  d_it_sym lists the members that keep the per-member stage when the batch holds families.
  DBuf<IterArgs> d_it_sym;
  DBuf<int> d_fmem;
  DBuf<FusedPass> d_fpass;
  int n_sym = 0, n_fgroups = 0, n_fmembers = 0, n_fpass = 0, gx_fused = 0;
  // members of a solver family with a structured inverse: the four stages of minv.hpp once per kMinvWidth members of a group
  // (k_minv_*_multi) instead of four launches per member.  A group of one keeps its member's own launches (equal bits); so does a
  // group whose factors are too large to stage in LDS, and every group under NNSDP_FAMILY_STRUCT=0 (diagnostic).
  DBuf<MinvFactors> d_sfac;
  DBuf<MinvWork> d_swork;
  DBuf<MinvPass> d_spass;
  MinvMultiGrid sgrid;
  int n_sgroups = 0, n_smembers = 0, n_spass = 0;
  std::vector<nnsdp_solver*> struct_single;      // structured members that take their own four launches, in batch order
  int nblocks = 0, nmax = 0;
  bool any_structured = false, any_big = false;
  ProjPlan plan;
  int gx_gather = 0, gx_gather_med = 0, gx_at_s = 0, gx_at_l = 0, gx_gemv = 0, gx_ax = 0, gx_ax_med = 0, gx_long = 0, gx_upd = 0, gx_tiles = 0, gx_nb = 0;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  static constexpr int kGraphIters = 8;

  ~nnsdp_batch() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (st) (void)hipStreamDestroy(st);
  }

  void create(nnsdp_solver** sv, int count) {
    if (!sv || count <= 0) throw std::invalid_argument("batch needs at least one solver");
    for (int i = 0; i < count; ++i) {
      if (!sv[i]) throw std::invalid_argument("null solver in batch");
      if (sv[i]->sharded) throw std::invalid_argument("clique-sharded solvers cannot be batched");
      if (sv[i]->opt.device != sv[0]->opt.device) throw std::invalid_argument("batched solvers must live on one device");
      if (sv[i]->opt.check_every != sv[0]->opt.check_every) throw std::invalid_argument("batched solvers must share check_every");
      // (one kernel variant per batched launch, chosen from proj_refine: members that disagree would silently lose - or get - the
      // refinement stage, and the variant would change whenever the first member finishes)
      if ((sv[i]->opt.proj_refine != 0) != (sv[0]->opt.proj_refine != 0)) throw std::invalid_argument("batched solvers must share proj_refine (on / off)");
      for (int j = 0; j < i; ++j) if (sv[j] == sv[i]) throw std::invalid_argument("a solver appears twice in the batch");
      all.push_back(sv[i]);
    }
    if (sv[0]->opt.device >= 0) HIPCHK(hipSetDevice(sv[0]->opt.device));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    status.assign(count, -1);
    act = all;
    rebuild();
  }

  void rebuild() {
    if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    n_sym = n_fgroups = n_fmembers = n_fpass = gx_fused = 0;
    n_sgroups = n_smembers = n_spass = 0; sgrid = MinvMultiGrid(); struct_single.clear();
    if (act.empty()) return;
    std::vector<IterArgs> it;
    std::vector<ProjArgs> pw, pc;
    std::vector<int2> map;
    nmax = 0; gx_gather = gx_gather_med = gx_at_s = gx_at_l = gx_gemv = gx_ax = gx_ax_med = gx_long = gx_upd = gx_tiles = gx_nb = 0;
    any_structured = false; any_big = false;
    std::vector<IterArgs> it_sym;
    std::vector<std::pair<int, std::vector<int>>> fam;      // family id -> its dense members here, in batch order
    std::vector<std::pair<int, std::vector<int>>> sfam;     // family id -> its structured members here, in batch order
    static const bool fuse_struct = [] { const char* e = std::getenv("NNSDP_FAMILY_STRUCT"); return !(e && std::atoi(e) == 0); }();   // diagnostic: 0 keeps the per-member launches
    for (size_t b = 0; b < act.size(); ++b) {
      nnsdp_solver* s = act[b];
      any_structured = any_structured || s->minv_structured;
      const bool fused = s->family != 0 && !s->minv_structured;      // (always, also alone: a member's bits must not depend on its group's size)
      if (fused) {
        auto f = std::find_if(fam.begin(), fam.end(), [&](const std::pair<int, std::vector<int>>& x) { return x.first == s->family; });
        if (f == fam.end()) { fam.emplace_back(s->family, std::vector<int>()); f = fam.end() - 1; }
        f->second.push_back((int)b);
      }
      if (s->minv_structured && s->family != 0 && s->m_lds.ok && fuse_struct) {
        auto f = std::find_if(sfam.begin(), sfam.end(), [&](const std::pair<int, std::vector<int>>& x) { return x.first == s->family; });
        if (f == sfam.end()) { sfam.emplace_back(s->family, std::vector<int>()); f = sfam.end() - 1; }
        f->second.push_back((int)b);
      }
      HIPCHK(hipStreamSynchronize(s->st));
      s->since_cold = nnsdp_solver::kColdPeriod;   // lockstep: the next batched iteration is a cold one for everybody
      IterArgs a;
      a.ng = s->S.ng; a.NE = s->S.NE; a.ldm = s->ldm; a.nlong = s->nlong; a.nmat = s->nmat;
      a.sptr = s->d_sptr.p; a.soff = s->d_soff.p; a.isdiag = s->d_isdiag.p;
      a.csc_ptr = s->D.csc_ptr.p; a.csc_row = s->D.csc_row.p; a.csc_val = s->D.csc_val.p;
      a.csr_ptr = s->D.csr_ptr.p; a.csr_col = s->D.csr_col.p; a.csr_val = s->D.csr_val.p;
      a.longrows = s->d_long.p; a.gidx = s->d_gidx.p;
      a.medrows = s->d_medrows.p; a.medsrc = s->d_medsrc.p; a.nmed = s->nmed; a.nmsrc = s->nmsrc; a.nnz = s->nnz_A;
      a.colcls = s->d_colcls.p; a.ncs = s->ncs;
      a.z0 = s->D.z0.p; a.Dinv = s->D.Dinv.p; a.c = s->D.c.p; a.Minv = s->Minv.p;
      a.nu = s->nu.p; a.w = s->w.p; a.g = s->g.p; a.p = s->p.p; a.qv = s->qv.p; a.ww = s->ww.p; a.x = s->x.p;
      a.sigma = s->d_sigma(); a.kappa = s->d_kappa(); a.alpha = s->opt.alpha;
      if (fused) { a.symv_part = nullptr; gx_fused = std::max(gx_fused, cdiv(a.ng, kFusedCols)); }
      else {
        const size_t nb = (size_t)(a.ng + 63) / 64;
        if (!s->minv_structured && s->symv_part.n != nb * nb * 64) s->symv_part.alloc(nb * nb * 64);
        a.symv_part = s->symv_part.p;
        gx_tiles = std::max(gx_tiles, cdiv((long long)(nb * (nb + 1) / 2), kThreads / 64));
        gx_nb = std::max(gx_nb, (int)nb);
        if (!s->minv_structured) it_sym.push_back(a);
      }
      it.push_back(a);
      ProjArgs q{};
      q.cn = s->d_cn.p; q.coff = s->d_coff.p; q.eoff = nullptr;
      q.nu = s->nu.p + s->S.ng; q.w = s->w.p + s->S.ng; q.Vg = s->Vg.p; q.eig = nullptr; q.Tg = s->Tg.p; q.Ug = s->Ug.p;
      q.kappa = s->d_kappa(); q.tol_dev = s->scal.p + 2; q.stats = s->d_stats.p;
      q.max_sweeps = 15; q.tol = nnsdp_solver::kProjTol;
      q.refine = s->opt.proj_refine; q.rstate = s->d_rstate.p;
      s->tune.bind(q);
      q.warm = 1; pw.push_back(q);
      q.warm = 0; pc.push_back(q);
      // blocks up to 128 of every SDP share ONE launch of the LDS-resident kernel; blocks above (the reference's 151-wide cliques of
      // width-50 nets) follow per SDP through the library path on the batch's stream (eager: rocSOLVER is not captured into the graph)
      if (s->big_idx.empty()) {
        for (int k = 0; k < s->ncl; ++k) { map.push_back(make_int2((int)b, k)); nmax = std::max(nmax, s->cn[k]); }
      } else {
        // (the solver's compact list of its blocks up to 128, as its own launches use it: same slots, same back-off state)
        pw.back().cn = s->d_cn_s.p; pw.back().coff = s->d_coff_s.p;
        pc.back().cn = s->d_cn_s.p; pc.back().coff = s->d_coff_s.p;
        for (size_t pos = 0; pos < s->proj_small.size(); ++pos) { map.push_back(make_int2((int)b, (int)pos)); nmax = std::max(nmax, s->cn[s->proj_small[pos]]); }
        any_big = true;
      }
      gx_gather = std::max(gx_gather, cdiv(a.NE, kThreads));
      gx_gather_med = std::max(gx_gather_med, cdiv((long long)a.nmsrc * 16, kThreads));
      gx_ax_med = std::max(gx_ax_med, cdiv((long long)a.nmed * 16, kThreads));
      gx_at_s = std::max(gx_at_s, cdiv((long long)a.ncs * 16, kThreads));
      gx_at_l = std::max(gx_at_l, cdiv((long long)(a.ng - a.ncs) * 64, kThreads));
      gx_gemv = std::max(gx_gemv, cdiv((long long)a.ng * 64, kThreads));
      gx_ax = std::max(gx_ax, cdiv(a.NE, kThreads));
      gx_long = std::max(gx_long, a.nlong);
      gx_upd = std::max(gx_upd, cdiv(a.ng + a.nmat, kThreads));
    }
    nblocks = (int)map.size();
    nmax = std::max(nmax, 1);
    plan = plan_projection(nmax, !act.empty() && act[0]->opt.proj_refine != 0);
    if (plan.packed())          // one launch for all members in the packed variant: every member needs its warm-start scratch
      for (size_t b = 0; b < act.size(); ++b) {
        if (!act[b]->Tg.p) { act[b]->Tg.alloc(act[b]->nmat); act[b]->Tg.zero(); pw[b].Tg = pc[b].Tg = act[b]->Tg.p; }
        if (!act[b]->Ug.p) { act[b]->Ug.alloc(act[b]->nmat); act[b]->Ug.zero(); pw[b].Ug = pc[b].Ug = act[b]->Ug.p; }
      }
    HIPCHK(proj_allow_big_lds(plan));
    d_it.upload(it); d_pw.upload(pw); d_pc.upload(pc); d_map.upload(map);
    {
      std::vector<MinvFactors> sfac;
      std::vector<MinvWork> swork;
      std::vector<MinvPass> spass;
      std::vector<char> in_group(act.size(), 0);
      for (auto& f : sfam) {
        if (f.second.size() < 2) continue;      // a group of one: the member's own launches
        nnsdp_solver* head = act[f.second[0]];
        sgrid.add(head->mdev, head->m_lds, (int)std::min<size_t>(kMinvWidth, f.second.size()));
        for (size_t o = 0; o < f.second.size(); o += kMinvWidth) {
          const int cnt = (int)std::min<size_t>(kMinvWidth, f.second.size() - o);
          spass.push_back(MinvPass{(int)sfac.size(), (int)swork.size(), cnt});
          for (int i = 0; i < cnt; ++i) { nnsdp_solver* s = act[f.second[o + i]]; swork.push_back(s->structured_work(s->qv.p, s->ww.p)); in_group[f.second[o + i]] = 1; }
        }
        sfac.push_back(head->mdev);
        ++n_sgroups;
      }
      for (size_t b = 0; b < act.size(); ++b) if (act[b]->minv_structured && !in_group[b]) struct_single.push_back(act[b]);
      n_smembers = (int)swork.size(); n_spass = (int)spass.size();
      if (n_spass) { d_sfac.upload(sfac); d_swork.upload(swork); d_spass.upload(spass); HIPCHK(minv_multi_allow_lds()); }
    }
    if (!fam.empty()) {
      std::vector<int> fmem;
      std::vector<FusedPass> fpass;
      for (auto& f : fam)
        for (size_t o = 0; o < f.second.size(); o += kFusedWidth) {
          const int cnt = (int)std::min<size_t>(kFusedWidth, f.second.size() - o);
          fpass.push_back(FusedPass{(int)fmem.size(), cnt});
          fmem.insert(fmem.end(), f.second.begin() + o, f.second.begin() + o + cnt);
        }
      n_fgroups = (int)fam.size(); n_fmembers = (int)fmem.size(); n_fpass = (int)fpass.size();
      n_sym = (int)it_sym.size();
      d_fmem.upload(fmem); d_fpass.upload(fpass);
      if (n_sym) d_it_sym.upload(it_sym);
    }
  }

  // the structured members: four launches for all fused groups together, then the members outside a group
  void enqueue_structured() {
    if (n_spass > 0) launch_minv_multi(sgrid, d_sfac.p, d_swork.p, d_spass.p, n_spass, st);
    for (nnsdp_solver* s : struct_single) s->enqueue_minv(st);
  }

  void enqueue_iteration(bool warm) {
    const int B = (int)act.size();
    if (nblocks > 0) launch_proj_batched(plan, warm ? d_pw.p : d_pc.p, d_map.p, nblocks, st);
    if (any_big) for (nnsdp_solver* s : act) s->enqueue_big_blocks(st);
    hipLaunchKernelGGL(k_gather_g_b, dim3(gx_gather + gx_gather_med, B), dim3(kThreads), 0, st, d_it.p, gx_gather);
    hipLaunchKernelGGL(k_spmv_At_b, dim3(std::max(gx_at_s + gx_at_l, 1), B), dim3(kThreads), 0, st, d_it.p, gx_at_s);
    static const bool full_gemv = [] { const char* e = std::getenv("NNSDP_BATCH_FULL_GEMV"); return e && std::atoi(e) != 0; }();   // diagnostic
    if (n_fpass > 0) {
      // the batch holds family members: one pass per group over the common inverse; structured members and solvers of no family
      // take the stage they take without families around (d_it_sym: the dense ones among them)
      hipLaunchKernelGGL(k_minv_family, dim3(gx_fused, n_fpass), dim3(kThreads), 0, st, d_it.p, d_fmem.p, d_fpass.p);
      if (any_structured) { enqueue_structured(); for (nnsdp_solver* s : act) if (!s->minv_structured && s->family == 0) s->enqueue_minv(st); }
      else if (n_sym > 0 && full_gemv) hipLaunchKernelGGL(k_gemv_sym_b, dim3(gx_gemv, n_sym), dim3(kThreads), 0, st, d_it_sym.p);
      else if (n_sym > 0) {
        hipLaunchKernelGGL(k_symv_tiles_b, dim3(gx_tiles, n_sym), dim3(kThreads), 0, st, d_it_sym.p);
        hipLaunchKernelGGL(k_symv_reduce_b, dim3(gx_nb, n_sym), dim3(64), 0, st, d_it_sym.p);
      }
    }
    else if (any_structured) { enqueue_structured(); for (nnsdp_solver* s : act) if (!s->minv_structured) s->enqueue_minv(st); }     // large multiplier counts: each SDP's structured M^-1
    else if (full_gemv) hipLaunchKernelGGL(k_gemv_sym_b, dim3(gx_gemv, B), dim3(kThreads), 0, st, d_it.p);
    else {
      hipLaunchKernelGGL(k_symv_tiles_b, dim3(gx_tiles, B), dim3(kThreads), 0, st, d_it.p);
      hipLaunchKernelGGL(k_symv_reduce_b, dim3(gx_nb, B), dim3(64), 0, st, d_it.p);
    }
    hipLaunchKernelGGL(k_spmv_A_x_all_b, dim3(gx_ax + gx_ax_med + gx_long, B), dim3(kThreads), 0, st, d_it.p, gx_ax, gx_ax_med, 0);
    hipLaunchKernelGGL(k_update_nu_b, dim3(gx_upd, B), dim3(kThreads), 0, st, d_it.p);
    HIPCHK(hipGetLastError());
  }

  // n plain iterations of every active solver (no residual checks, no adaptation); synchronous
  void iterate(int n) {
    if (n <= 0 || act.empty()) return;
    int left = n;
    while (left > 0) {
      const int sc = act[0]->since_cold;   // equal for all active solvers
      const bool warm_ok = act[0]->opt.warm_start != 0 && sc < nnsdp_solver::kColdPeriod;
      int did;
      static const bool no_graph = [] { const char* e = std::getenv("NNSDP_NO_GRAPH"); return e && std::atoi(e) != 0; }();   // diagnostic: eager launches only
      const int giters = nnsdp_solver::graph_iters_for(act[0]->opt.check_every);      // (equal for all members)
      if (!no_graph && !any_big && warm_ok && left >= giters && nnsdp_solver::kColdPeriod - sc >= giters) {
        if (!gexec) {
          HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
          for (int i = 0; i < giters; ++i) enqueue_iteration(true);
          HIPCHK(hipStreamEndCapture(st, &graph));
          HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
        }
        HIPCHK(hipGraphLaunch(gexec, st));
        for (nnsdp_solver* s : act) ++s->graph_launches;      // (nnsdp_solver_info 0: the replay advanced every member)
        did = giters;
      } else {
        enqueue_iteration(warm_ok);
        did = 1;
      }
      for (nnsdp_solver* s : act) {
        s->iters_done += did;
        s->since_cold = (did == 1 && !warm_ok) ? 1 : s->since_cold + did;
      }
      left -= did;
    }
    HIPCHK(hipStreamSynchronize(st));
  }

  // full solves with the stopping rules of nnsdp_solver::run_loop, each SDP on its own
  void run() {
    double t0 = now_s();
    for (nnsdp_solver* s : act) s->loop_begin();
    while (!act.empty()) {
      long long n = act[0]->opt.check_every - 1;
      for (nnsdp_solver* s : act) n = std::min<long long>(n, (long long)s->opt.max_iters - s->iters_done - 1);
      iterate((int)std::max<long long>(n, 0));
      for (nnsdp_solver* s : act) s->check_enqueue();
      for (nnsdp_solver* s : act) s->check_finish();
      std::vector<nnsdp_solver*> keep;
      for (nnsdp_solver* s : act) {
        int stt = s->post_check(false, t0);
        if (stt < 0 && s->iters_done >= s->opt.max_iters) stt = NNSDP_STATUS_ITERATION_LIMIT;
        if (stt >= 0) {
          for (size_t i = 0; i < all.size(); ++i) if (all[i] == s) status[i] = stt;
          s->t_solve += now_s() - t0;
        } else keep.push_back(s);
      }
      if (keep.size() != act.size()) { act = keep; rebuild(); }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Resident CROWN bounder: the network, the literal head, the box / scratch / output buffers, pinned staging, one stream and two
// events stay alive across calls, so a level of a split tree pays one upload of its boxes, one launch, one download and one stream
// synchronisation (the one-shot entries pay the whole set-up per call).  Not thread-safe; distinct handles are independent.
// ---------------------------------------------------------------------------------------------
struct nnsdp_crown {
  int K = 0, activ = 0, nlit = 0, acdim = 0, n0 = 0, ny = 0, wp = 0;
  std::vector<long long> moff;
  DBuf<int> dxd, dao;
  DBuf<long long> dmo;
  DBuf<double> dM;                       // the network, then the literal head
  DBuf<double> din, dscr, dout, dX, dY;   // boxes (lo, then hi), per-box scratch, outputs; samples in / out
  double *hin = nullptr, *hout = nullptr, *hX = nullptr, *hY = nullptr;      // pinned staging of the four transfers
  // nnsdp_crown_bound_alpha only (nothing before its first call): boxes then alpha0; the plain outputs then the alpha outputs; the state
  DBuf<double> dain, daout, dast;
  double *hain = nullptr, *haout = nullptr;
  size_t box_cap = 0, pin_cap = 0, sample_cap = 0, alpha_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  long long n_alloc = 0, n_upload = 0, n_bound = 0;
  // nnsdp_crown_search only (nothing before its first call): the two frontiers (lo and hi of both, then the cuts of both), the
  // per-level records / points / leaf log / clause, the status record's pinned copy; the result of the last search
  std::vector<double> normals;           // the literals of the handle (ny x nlit), kept for the proof test of the search
  DBuf<double> sfr, sdb;
  DBuf<int> scu, sib;
  int* hstatus = nullptr;
  struct SearchLeaves {                  // flat, in the order of the Python loop; lo / hi n0 x nleaves column-major
    std::vector<double> lo, hi, bound;
    std::vector<int32_t> depth, proved, literal;
    void clear() { lo.clear(); hi.clear(); bound.clear(); depth.clear(); proved.clear(); literal.clear(); }
  } leaves;

  size_t scr_per_box() const { return (size_t)(activ == NNSDP_ACTIV_TANH ? 6 : 2) * acdim; }
  size_t out_per_box() const { return 4 * (size_t)acdim + 2 * (size_t)ny + 3 * (size_t)nlit + (size_t)nlit * n0; }
  size_t ain_per_box() const { return 2 * (size_t)n0 + (size_t)nlit * acdim; }
  size_t aout_per_box() const { return out_per_box() + (size_t)nlit * (3 + (size_t)n0 + (size_t)acdim); }
  size_t ast_per_box() const { return 3 * (size_t)nlit * acdim; }
  size_t lds_bytes() const { return activ == NNSDP_ACTIV_TANH ? kCbLdsBytesTanh : kCbLdsBytes; }
  const void* kernel() const {
    return activ == NNSDP_ACTIV_TANH ? reinterpret_cast<const void*>(&k_crown_resident<kCbTanh>)
                                     : reinterpret_cast<const void*>(&k_crown_resident<kCbRelu>);
  }
  void dalloc(DBuf<double>& b, size_t count) { b.alloc(count); if (count) ++n_alloc; }
  static void pinned(double*& h, size_t count) {
    if (h) { HIPCHK(hipHostFree(h)); h = nullptr; }
    if (count) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h), count * sizeof(double), hipHostMallocDefault));
  }
  size_t device_bytes() const {
    return dxd.bytes() + dao.bytes() + dmo.bytes() + dM.bytes() + din.bytes() + dscr.bytes() + dout.bytes() + dX.bytes() + dY.bytes() +
           dain.bytes() + daout.bytes() + dast.bytes() + sfr.bytes() + sdb.bytes() + scu.bytes() + sib.bytes();
  }
  // the capacity grows geometrically and never shrinks
  // staging = false (a search: nothing of a box crosses the bus): the pinned copies wait for the next bound call
  // limit: the geometric growth stops there (a search: one chunk); a call that needs more still gets it
  void reserve_boxes(size_t nbox, bool staging = true, size_t limit = (size_t)-1) {
    if (nbox > box_cap) {
      const size_t cap = std::max(nbox, std::min(2 * box_cap, limit));
      dalloc(din, 2 * cap * n0); dalloc(dscr, cap * scr_per_box()); dalloc(dout, cap * out_per_box());
      box_cap = cap;
    }
    if (staging && pin_cap < box_cap) {
      pinned(hin, 2 * box_cap * n0); pinned(hout, box_cap * out_per_box());
      pin_cap = box_cap;
    }
  }
  // the buffers of the alpha calls; the scratch is the plain calls' (reserve_boxes)
  void reserve_alpha(size_t nbox) {
    reserve_boxes(nbox);
    if (nbox <= alpha_cap) return;
    if (!alpha_cap)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crown_alpha), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCaLdsBytes));
    const size_t cap = std::max(nbox, 2 * alpha_cap);
    dalloc(dain, cap * ain_per_box()); dalloc(daout, cap * aout_per_box()); dalloc(dast, cap * ast_per_box());
    pinned(hain, cap * ain_per_box()); pinned(haout, cap * aout_per_box());
    alpha_cap = cap;
  }
  // the buffers of a search: frontiers of `cap` boxes each, `nd` doubles and `ni` ints of records; they only grow
  void reserve_search(size_t cap, size_t nd, size_t ni) {
    if (4 * cap * n0 > sfr.n) { dalloc(sfr, 4 * cap * n0); scu.alloc(2 * cap * n0); ++n_alloc; }
    if (nd > sdb.n) dalloc(sdb, nd);
    if (ni > sib.n) { sib.alloc(ni); ++n_alloc; }
    if (!hstatus) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hstatus), 4 * sizeof(int), hipHostMallocDefault));
  }
  void reserve_samples(size_t N) {
    if (N <= sample_cap) return;
    const size_t cap = std::max(N, 2 * sample_cap);
    dalloc(dX, cap * n0); dalloc(dY, cap * ny);
    pinned(hX, cap * n0); pinned(hY, cap * ny);
    sample_cap = cap;
  }
  ~nnsdp_crown() {
    if (st) (void)hipStreamSynchronize(st);
    for (double* h : {hin, hout, hX, hY, hain, haout}) if (h) (void)hipHostFree(h);
    if (hstatus) (void)hipHostFree(hstatus);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
};

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
  // every vector gets an IterArgs slot of its own (what the kernel reads of it: ng, ldm, Minv, qv, ww), as members of a batch have
  DBuf<double> qd, wd;
  std::vector<double> qh((size_t)nrhs * ldm, 0.0);
  for (int j = 0; j < nrhs; ++j)
    for (int g = 0; g < ng; ++g) qh[(size_t)j * ldm + g] = Q[(size_t)j * full + s->S.keep[g]];
  qd.upload(qh);
  wd.alloc((size_t)nrhs * ldm); wd.zero();
  std::vector<IterArgs> it(nrhs);
  std::vector<int> mem(nrhs);
  std::vector<FusedPass> ps;
  for (int j = 0; j < nrhs; ++j) {
    std::memset(&it[j], 0, sizeof(IterArgs));
    it[j].ng = ng; it[j].ldm = ldm; it[j].Minv = s->Minv.p; it[j].qv = qd.p + (size_t)j * ldm; it[j].ww = wd.p + (size_t)j * ldm;
    mem[j] = j;
    if (j % kFusedWidth == 0) ps.push_back(FusedPass{j, std::min<int>(kFusedWidth, nrhs - j)});
  }
  DBuf<IterArgs> dit; DBuf<int> dmem; DBuf<FusedPass> dps;
  dit.upload(it); dmem.upload(mem); dps.upload(ps);
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, s->st));
  hipLaunchKernelGGL(k_minv_family, dim3(cdiv(ng, kFusedCols), (int)ps.size()), dim3(kThreads), 0, s->st, dit.p, dmem.p, dps.p);
  HIPCHK(hipEventRecord(e1, s->st));
  const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(s->st);
  float ms = 0.f;
  if (le == hipSuccess && se == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  HIPCHK(le); HIPCHK(se);
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
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
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

// the refusals of the literal arguments, shared by the two _lits entries (xdims[K] must be valid)
static void check_literals(int32_t ny, int32_t nlit, const double* normals) {
  if (nlit < 0 || nlit > nnsdp::kCbW) throw std::invalid_argument("nlit must be in 0..64, got " + std::to_string(nlit));
  if (nlit > 0 && !normals) throw std::invalid_argument("normals is null with nlit > 0");
  for (int i = 0; i < nlit; ++i)
    for (int j = 0; j < ny; ++j)
      if (!std::isfinite(normals[(size_t)i * ny + j]))
        throw std::invalid_argument("literal " + std::to_string(i) + ": the normal has a non-finite entry (NaN or infinity)");
}

// the options and outputs that the two _alpha entries add to their plain counterparts
struct AlphaReq {
  int32_t steps;
  double eta0, decay;
  const double* alpha0;
  double *a_smax, *a_uA, *a_ub0, *alpha;
  int32_t* best_step;
};
static void check_alpha_options(int32_t steps, double eta0, double decay) {
  if (steps < 0 || steps > 64) throw std::invalid_argument("alpha: steps must be in 0..64, got " + std::to_string(steps));
  if (!std::isfinite(eta0) || !(eta0 > 0.0)) throw std::invalid_argument("alpha: eta0 must be positive and finite");
  if (!(decay > 0.0 && decay <= 1.0)) throw std::invalid_argument("alpha: decay must be in (0, 1]");
}
static void check_alpha0(const double* alpha0, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(alpha0[k])) throw std::invalid_argument("alpha0 has a non-finite entry (NaN or infinity) at index " + std::to_string(k));
}

static int make_intervals_impl(int32_t K, const int32_t* xdims, const double* M, int32_t activ, const double* x1min, const double* x1max,
                         double* acymin, double* acymax, double* acxmin, double* acxmax, double* smin, double* smax,
                         double* ymin, double* ymax, int32_t nlit = 0, const double* normals = nullptr, double* lit_smin = nullptr,
                         double* lit_smax = nullptr, double* uA = nullptr, double* ub0 = nullptr, const AlphaReq* ar = nullptr) {
  API_BEGIN
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  if (ar) {
    if (activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("optimised slopes (alpha) are for ReLU networks, not Tanh");
    if (nlit < 1) throw std::invalid_argument("optimised slopes (alpha) need literals: nlit must be in 1..64");
    check_alpha_options(ar->steps, ar->eta0, ar->decay);
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
  std::vector<int> xd(xdims, xdims + K + 1);
  std::vector<long long> moff(K + 1, 0);
  int wp = 0;
  for (int k = 0; k < K; ++k) {
    if (xd[k] < 1 || xd[k + 1] < 1) throw std::invalid_argument("layer widths must be >= 1");
    moff[k + 1] = moff[k] + (long long)xd[k + 1] * (xd[k] + 1);
    wp = std::max(wp, (xd[k] + 1 + 3) & ~3);
  }
  const size_t lds = 2 * (size_t)wp * 16 * sizeof(double);
  if (lds > 160 * 1024) throw std::invalid_argument("layer width above 639 is not supported by the sampled forward pass");
  if ((N + 15) / 16 > 0x7fffffffLL) throw std::invalid_argument("too many samples for one launch");
  DBuf<int> dxd; DBuf<long long> dmo; DBuf<double> dM, dX, dY;
  dxd.upload(xd); dmo.upload(moff);
  dM.alloc(moff[K]); dX.alloc((size_t)xd[0] * N); dY.alloc((size_t)xd[K] * N);
  HIPCHK(hipMemcpy(dM.p, M, moff[K] * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dX.p, X, (size_t)xd[0] * N * sizeof(double), hipMemcpyHostToDevice));
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nnsdp::k_forward_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  nnsdp::FwdArgs a;
  a.K = K; a.xdims = dxd.p; a.moff = dmo.p; a.M = dM.p; a.X = dX.p; a.Y = dY.p; a.N = N; a.activ = activ; a.wp = wp;
  struct Events {   // destroyed on every path out of this function, HIPCHK throws
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  hipLaunchKernelGGL(nnsdp::k_forward_mfma, dim3((unsigned)((N + 15) / 16)), dim3(64), lds, nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipEventSynchronize(ev.e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  HIPCHK(hipMemcpy(Y, dY.p, (size_t)xd[K] * N * sizeof(double), hipMemcpyDeviceToHost));
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
  std::vector<int> xd(xdims, xdims + K + 1), acoff(K, 0);
  std::vector<long long> moff(K + 1, 0);
  for (int k = 0; k <= K; ++k) {
    if (xd[k] < 1) throw std::invalid_argument("layer widths must be >= 1");
    if (xd[k] > nnsdp::kCbW)
      throw std::invalid_argument("layer width " + std::to_string(xd[k]) + " is above 64, the widest layer of the batched intervals");
  }
  for (int k = 0; k < K; ++k) {
    moff[k + 1] = moff[k] + (long long)xd[k + 1] * (xd[k] + 1);
    if (k > 0) acoff[k] = acoff[k - 1] + xd[k];
  }
  const int acdim = acoff[K - 1], n0 = xd[0], ny = xd[K];
  check_literals(ny, nlit, normals);
  if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
  if (nbox == 0) return 0;
  if (!x1min || !x1max) throw std::invalid_argument("null argument");
  for (long long b = 0; b < nbox; ++b)
    for (int i = 0; i < n0; ++i)
      if (!std::isfinite(x1min[b * n0 + i]) || !std::isfinite(x1max[b * n0 + i]) || !(x1min[b * n0 + i] <= x1max[b * n0 + i]))
        throw std::invalid_argument("box " + std::to_string(b) + ": x1min must be <= x1max and both finite (no NaN, no infinity)");
  require_gpu();
  DBuf<int> dxd, dao; DBuf<long long> dmo; DBuf<double> dM, dlo, dhi, dscr, dout;
  dxd.upload(xd); dao.upload(acoff); dmo.upload(moff);
  const size_t nb = (size_t)nbox, na = nb * acdim, ny_all = nb * ny;
  // the literal head H sits behind M; the literal outputs behind the six interval arrays: smin, smax, ub0 (nlit each per box), uA
  const size_t hlen = nlit > 0 ? (size_t)nlit * (xd[K - 1] + 1) : 0, nl_all = nb * (size_t)nlit, nA_all = nl_all * n0;
  dM.alloc(moff[K] + hlen); dlo.alloc(nb * n0); dhi.alloc(nb * n0); dscr.alloc(2 * na); dout.alloc(4 * na + 2 * ny_all + 3 * nl_all + nA_all);
  HIPCHK(hipMemcpy(dM.p, M, moff[K] * sizeof(double), hipMemcpyHostToDevice));
  if (nlit > 0) {
    const nnsdp::LitHead head = nnsdp::make_lit_head(K, xdims, M, nlit, normals);
    HIPCHK(hipMemcpy(dM.p + moff[K], head.H.data(), hlen * sizeof(double), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(dlo.p, x1min, nb * n0 * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dhi.p, x1max, nb * n0 * sizeof(double), hipMemcpyHostToDevice));
  nnsdp::CrownArgs a;
  a.K = K; a.xdims = dxd.p; a.moff = dmo.p; a.acoff = dao.p; a.M = dM.p; a.lo = dlo.p; a.hi = dhi.p; a.scratch = dscr.p;
  a.acymin = dout.p; a.acymax = dout.p + na; a.acxmin = dout.p + 2 * na; a.acxmax = dout.p + 3 * na;
  a.ymin = dout.p + 4 * na; a.ymax = a.ymin + ny_all; a.acdim = acdim;
  a.nlit = nlit; a.H = dM.p + moff[K];
  a.smin = a.ymax + ny_all; a.smax = a.smin + nl_all; a.ub0 = a.smax + nl_all; a.uA = a.ub0 + nl_all;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nnsdp::k_crown_batch), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)nnsdp::kCbLdsBytes));
  struct Events {   // destroyed on every path out of this function, HIPCHK throws
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
  HIPCHK(hipEventRecord(ev.e0, nullptr));
  hipLaunchKernelGGL(nnsdp::k_crown_batch, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytes, nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e1, nullptr));
  HIPCHK(hipEventSynchronize(ev.e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  double* host[6] = {acymin, acymax, acxmin, acxmax, ymin, ymax};
  const double* dev[6] = {a.acymin, a.acymax, a.acxmin, a.acxmax, a.ymin, a.ymax};
  for (int o = 0; o < 6; ++o)
    if (host[o] && (o < 4 ? na : ny_all))
      HIPCHK(hipMemcpy(host[o], dev[o], (o < 4 ? na : ny_all) * sizeof(double), hipMemcpyDeviceToHost));
  double* lhost[4] = {smin, smax, ub0, uA};
  const double* ldev[4] = {a.smin, a.smax, a.ub0, a.uA};
  for (int o = 0; o < 4; ++o)
    if (lhost[o] && (o < 3 ? nl_all : nA_all))
      HIPCHK(hipMemcpy(lhost[o], ldev[o], (o < 3 ? nl_all : nA_all) * sizeof(double), hipMemcpyDeviceToHost));
  API_END
}

int nnsdp_crown_create(int32_t K, const int32_t* xdims, const double* M, int32_t activ, int32_t nlit, const double* normals,
                       nnsdp_crown** out) {
  API_BEGIN
  if (!out) throw std::invalid_argument("null argument");
  *out = nullptr;
  if (K < 2 || !xdims || !M) throw std::invalid_argument("null / empty network (K >= 2 layers are needed)");
  if (activ != NNSDP_ACTIV_RELU && activ != NNSDP_ACTIV_TANH) throw std::invalid_argument("unknown activation");
  std::vector<int> xd(xdims, xdims + K + 1), acoff(K, 0);
  std::vector<long long> moff(K + 1, 0);
  int wp = 0;
  for (int k = 0; k <= K; ++k) {
    if (xd[k] < 1) throw std::invalid_argument("layer widths must be >= 1");
    if (xd[k] > nnsdp::kCbW)
      throw std::invalid_argument("layer width " + std::to_string(xd[k]) + " is above 64, the widest layer of the batched intervals");
  }
  for (int k = 0; k < K; ++k) {
    moff[k + 1] = moff[k] + (long long)xd[k + 1] * (xd[k] + 1);
    if (k > 0) acoff[k] = acoff[k - 1] + xd[k];
    wp = std::max(wp, (xd[k] + 1 + 3) & ~3);
  }
  check_literals(xd[K], nlit, normals);
  require_gpu();
  std::unique_ptr<nnsdp_crown> h(new nnsdp_crown);
  h->K = K; h->activ = activ; h->nlit = nlit; h->acdim = acoff[K - 1]; h->n0 = xd[0]; h->ny = xd[K]; h->wp = wp; h->moff = moff;
  if (nlit > 0) h->normals.assign(normals, normals + (size_t)nlit * xd[K]);
  h->dxd.upload(xd); h->dao.upload(acoff); h->dmo.upload(moff);
  const size_t hlen = nlit > 0 ? (size_t)nlit * (xd[K - 1] + 1) : 0;      // the literal head H sits behind M
  h->dM.alloc(moff[K] + hlen);
  h->n_alloc += 4;
  HIPCHK(hipMemcpy(h->dM.p, M, moff[K] * sizeof(double), hipMemcpyHostToDevice));
  ++h->n_upload;
  if (nlit > 0) {
    const nnsdp::LitHead head = nnsdp::make_lit_head(K, xdims, M, nlit, normals);
    HIPCHK(hipMemcpy(h->dM.p + moff[K], head.H.data(), hlen * sizeof(double), hipMemcpyHostToDevice));
  }
  // (k_forward_mfma needs no attribute here: widths <= 64 keep its LDS at 2 * 68 * 16 doubles)
  HIPCHK(hipFuncSetAttribute(h->kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes()));
  HIPCHK(hipStreamCreate(&h->st));
  HIPCHK(hipEventCreate(&h->e0)); HIPCHK(hipEventCreate(&h->e1));
  *out = h.release();
  API_END
}

int nnsdp_crown_bound(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                      double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                      double* smin, double* smax, double* uA, double* ub0, double* kernel_ms) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
  if (nbox == 0) return 0;
  if (!x1min || !x1max) throw std::invalid_argument("null argument");
  const int n0 = h->n0, acdim = h->acdim, ny = h->ny, nlit = h->nlit;
  for (long long b = 0; b < nbox; ++b)
    for (int i = 0; i < n0; ++i)
      if (!std::isfinite(x1min[b * n0 + i]) || !std::isfinite(x1max[b * n0 + i]) || !(x1min[b * n0 + i] <= x1max[b * n0 + i]))
        throw std::invalid_argument("box " + std::to_string(b) + ": x1min must be <= x1max and both finite (no NaN, no infinity)");
  const size_t nb = (size_t)nbox, nin = nb * n0, na = nb * acdim, ny_all = nb * ny, nl_all = nb * (size_t)nlit, nA_all = nl_all * n0;
  const size_t nout = nb * h->out_per_box();
  h->reserve_boxes(nb);
  std::copy(x1min, x1min + nin, h->hin);
  std::copy(x1max, x1max + nin, h->hin + nin);
  HIPCHK(hipMemcpyAsync(h->din.p, h->hin, 2 * nin * sizeof(double), hipMemcpyHostToDevice, h->st));
  // the layouts of nnsdp_make_intervals_batch_lits, packed for nbox boxes so that one copy brings everything back
  nnsdp::CrownArgs a;
  a.K = h->K; a.xdims = h->dxd.p; a.moff = h->dmo.p; a.acoff = h->dao.p; a.M = h->dM.p; a.lo = h->din.p; a.hi = h->din.p + nin;
  a.scratch = h->dscr.p;
  a.acymin = h->dout.p; a.acymax = a.acymin + na; a.acxmin = a.acymin + 2 * na; a.acxmax = a.acymin + 3 * na;
  a.ymin = a.acymin + 4 * na; a.ymax = a.ymin + ny_all; a.acdim = acdim;
  a.nlit = nlit; a.H = h->dM.p + h->moff[h->K];
  a.smin = a.ymax + ny_all; a.smax = a.smin + nl_all; a.ub0 = a.smax + nl_all; a.uA = a.ub0 + nl_all;
  HIPCHK(hipEventRecord(h->e0, h->st));
  if (h->activ == NNSDP_ACTIV_TANH)
    hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbTanh>, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytesTanh, h->st, a);
  else
    hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbRelu>, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytes, h->st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipMemcpyAsync(h->hout, h->dout.p, nout * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  ++h->n_bound;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  if (kernel_ms) *kernel_ms = ms;
  double* host[10] = {acymin, acymax, acxmin, acxmax, ymin, ymax, smin, smax, ub0, uA};
  const size_t len[10] = {na, na, na, na, ny_all, ny_all, nl_all, nl_all, nl_all, nA_all};
  const double* src = h->hout;
  for (int o = 0; o < 10; src += len[o], ++o)
    if (host[o]) std::copy(src, src + len[o], host[o]);
  API_END
}

int nnsdp_crown_bound_alpha(nnsdp_crown* h, int32_t nbox, const double* x1min, const double* x1max,
                            double* acymin, double* acymax, double* acxmin, double* acxmax, double* ymin, double* ymax,
                            double* smin, double* smax, double* uA, double* ub0, double* kernel_ms,
                            int32_t steps, double eta0, double decay, const double* alpha0,
                            double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  if (h->activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("optimised slopes (alpha) are for ReLU networks, not Tanh");
  if (h->nlit < 1) throw std::invalid_argument("optimised slopes (alpha) need literals: the handle was created without normals");
  check_alpha_options(steps, eta0, decay);
  if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
  if (nbox == 0) return 0;
  if (!x1min || !x1max) throw std::invalid_argument("null argument");
  const int n0 = h->n0, acdim = h->acdim, ny = h->ny, nlit = h->nlit;
  for (long long b = 0; b < nbox; ++b)
    for (int i = 0; i < n0; ++i)
      if (!std::isfinite(x1min[b * n0 + i]) || !std::isfinite(x1max[b * n0 + i]) || !(x1min[b * n0 + i] <= x1max[b * n0 + i]))
        throw std::invalid_argument("box " + std::to_string(b) + ": x1min must be <= x1max and both finite (no NaN, no infinity)");
  const size_t nb = (size_t)nbox, nin = nb * n0, na = nb * acdim, ny_all = nb * ny, nl_all = nb * (size_t)nlit, nA_all = nl_all * n0;
  const size_t nst_all = nl_all * acdim, nplain = nb * h->out_per_box(), nout = nb * h->aout_per_box();
  if (alpha0) check_alpha0(alpha0, nst_all);
  h->reserve_alpha(nb);
  // one upload: the boxes, then alpha0 when there is one
  std::copy(x1min, x1min + nin, h->hain);
  std::copy(x1max, x1max + nin, h->hain + nin);
  if (alpha0) std::copy(alpha0, alpha0 + nst_all, h->hain + 2 * nin);
  HIPCHK(hipMemcpyAsync(h->dain.p, h->hain, (2 * nin + (alpha0 ? nst_all : 0)) * sizeof(double), hipMemcpyHostToDevice, h->st));
  nnsdp::CrownAlphaArgs p;
  nnsdp::CrownArgs& a = p.c;
  a.K = h->K; a.xdims = h->dxd.p; a.moff = h->dmo.p; a.acoff = h->dao.p; a.M = h->dM.p; a.lo = h->dain.p; a.hi = h->dain.p + nin;
  a.scratch = h->dscr.p;
  a.acymin = h->daout.p; a.acymax = a.acymin + na; a.acxmin = a.acymin + 2 * na; a.acxmax = a.acymin + 3 * na;
  a.ymin = a.acymin + 4 * na; a.ymax = a.ymin + ny_all; a.acdim = acdim;
  a.nlit = nlit; a.H = h->dM.p + h->moff[h->K];
  a.smin = a.ymax + ny_all; a.smax = a.smin + nl_all; a.ub0 = a.smax + nl_all; a.uA = a.ub0 + nl_all;
  p.steps = steps; p.eta0 = eta0; p.decay = decay; p.alpha0 = alpha0 ? h->dain.p + 2 * nin : nullptr;
  p.cur = h->dast.p; p.lam = p.cur + nst_all; p.best = p.lam + nst_all;
  p.a_smax = h->daout.p + nplain; p.a_ub0 = p.a_smax + nl_all; p.a_step = p.a_ub0 + nl_all; p.a_uA = p.a_step + nl_all; p.alpha = p.a_uA + nA_all;
  HIPCHK(hipEventRecord(h->e0, h->st));
  hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbRelu>, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytes, h->st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(nnsdp::k_crown_alpha, dim3((unsigned)nbox), dim3(256), nnsdp::kCaLdsBytes, h->st, p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipMemcpyAsync(h->haout, h->daout.p, nout * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  ++h->n_bound;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  if (kernel_ms) *kernel_ms = ms;
  double* host[14] = {acymin, acymax, acxmin, acxmax, ymin, ymax, smin, smax, ub0, uA, a_smax, a_ub0, nullptr, a_uA};
  const size_t len[14] = {na, na, na, na, ny_all, ny_all, nl_all, nl_all, nl_all, nA_all, nl_all, nl_all, nl_all, nA_all};
  const double* src = h->haout;
  for (int o = 0; o < 14; src += len[o], ++o) {
    if (host[o]) std::copy(src, src + len[o], host[o]);
    if (o == 12 && best_step)
      for (size_t k = 0; k < nl_all; ++k) best_step[k] = (int32_t)src[k];
  }
  if (alpha) std::copy(src, src + nst_all, alpha);
  API_END
}

int nnsdp_crown_eval(nnsdp_crown* h, int64_t N, const double* X, double* Y, double* kernel_ms) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  if (N < 0) throw std::invalid_argument("N must be >= 0");
  if (N == 0) return 0;
  if (!X || !Y) throw std::invalid_argument("null argument");
  if ((N + 15) / 16 > 0x7fffffffLL) throw std::invalid_argument("too many samples for one launch");
  const size_t lds = 2 * (size_t)h->wp * 16 * sizeof(double), nx = (size_t)h->n0 * N, nyN = (size_t)h->ny * N;
  h->reserve_samples((size_t)N);
  std::copy(X, X + nx, h->hX);
  HIPCHK(hipMemcpyAsync(h->dX.p, h->hX, nx * sizeof(double), hipMemcpyHostToDevice, h->st));
  nnsdp::FwdArgs a;
  a.K = h->K; a.xdims = h->dxd.p; a.moff = h->dmo.p; a.M = h->dM.p; a.X = h->dX.p; a.Y = h->dY.p; a.N = N; a.activ = h->activ; a.wp = h->wp;
  HIPCHK(hipEventRecord(h->e0, h->st));
  hipLaunchKernelGGL(nnsdp::k_forward_mfma, dim3((unsigned)((N + 15) / 16)), dim3(64), lds, h->st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipMemcpyAsync(h->hY, h->dY.p, nyN * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  if (kernel_ms) *kernel_ms = ms;
  std::copy(h->hY, h->hY + nyN, Y);
  API_END
}

int nnsdp_crown_search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                       int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                       nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                       int32_t* nleaves, double* witness, double* kernel_ms) {
  API_BEGIN
  // (the scalar options come before the handle so that their refusals can be tested on a machine without a GPU, where no handle exists)
  if (max_boxes < 1) throw std::invalid_argument("max_boxes must be >= 1, got " + std::to_string(max_boxes));
  if (chunk < 1) throw std::invalid_argument("chunk must be >= 1, got " + std::to_string(chunk));
  if (max_depth < 0) throw std::invalid_argument("max_depth must be >= 0, got " + std::to_string(max_depth));
  if (!h) throw std::invalid_argument("null handle");
  if (!x1min || !x1max || !hs || !verdict || !visited || !depth_reached || !nleaves || !witness) throw std::invalid_argument("null argument");
  const int n0 = h->n0, ny = h->ny;
  if (h->nlit > 0) {
    if (normals) throw std::invalid_argument("the handle has literals of its own: normals must be NULL");
    if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
    normals = h->normals.data();
  } else {
    if (literal_bounds) throw std::invalid_argument("literal_bounds needs literals: the handle was created without normals");
    if (corner_points) throw std::invalid_argument("corner_points needs literals: the handle was created without normals");
    if (nlit < 1) throw std::invalid_argument("a clause needs at least one literal (nlit >= 1)");
    check_literals(ny, nlit, normals);
  }
  for (int i = 0; i < nlit; ++i)
    if (!std::isfinite(hs[i])) throw std::invalid_argument("literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
  unsigned long long splitmask = 0;
  for (int t = 0; t < n0; ++t) {
    if (!std::isfinite(x1min[t]) || !std::isfinite(x1max[t]) || !(x1min[t] <= x1max[t]))
      throw std::invalid_argument("the root box: x1min must be <= x1max and both finite (no NaN, no infinity)");
    if (x1max[t] > x1min[t]) splitmask |= 1ull << t;
  }
  // a level bounds at most max_boxes boxes and its children number at most twice that
  const size_t mb = (size_t)max_boxes, cap = 2 * mb, npmax = corner_points ? 2 * mb : mb, logw = 2 * (size_t)n0 + 3;
  const size_t frontier_bytes = 2 * cap * n0 * (2 * sizeof(double) + sizeof(int));
  if (frontier_bytes > nnsdp::kSearchFrontierCap)
    throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(frontier_bytes) +
                                " bytes of frontier buffers, above the cap of 2^31 bytes");
  // doubles: bound, points in, points out, leaf log, normals, hs;  ints: open, best, coord, slot, point flags, status
  const size_t o_bound = 0, o_X = o_bound + mb, o_Y = o_X + npmax * n0, o_log = o_Y + npmax * ny, o_nrm = o_log + mb * logw,
               o_hs = o_nrm + (size_t)nlit * ny, nd = o_hs + nlit;
  const size_t ni = 4 * mb + npmax + 4;
  const size_t cb = std::min((size_t)chunk, mb);
  h->leaves.clear();
  h->reserve_search(cap, nd, ni);
  hipStream_t st = h->st;
  double* D = h->sdb.p;
  int* I = h->sib.p;
  double *flo[2] = {h->sfr.p, h->sfr.p + 2 * cap * n0}, *fhi[2] = {flo[0] + cap * n0, flo[1] + cap * n0};
  int* fcu[2] = {h->scu.p, h->scu.p + cap * n0};
  HIPCHK(hipMemcpyAsync(flo[0], x1min, n0 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(fhi[0], x1max, n0 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(fcu[0], 0, n0 * sizeof(int), st));
  HIPCHK(hipMemcpyAsync(D + o_nrm, normals, (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_hs, hs, nlit * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));      // (the sources are the caller's pageable arrays)

  nnsdp::SearchArgs s;
  s.n0 = n0; s.ny = ny; s.nlit = nlit; s.literal_bounds = literal_bounds != 0; s.corner_points = corner_points != 0;
  s.splitmask = splitmask; s.normals = D + o_nrm; s.hs = D + o_hs;
  s.open = I; s.best = I + mb; s.coord = I + 2 * mb; s.slot = I + 3 * mb; s.pflag = I + 4 * mb; s.status = I + 4 * mb + npmax;
  s.bound = D + o_bound; s.X = D + o_X; s.Y = D + o_Y; s.log = D + o_log;
  nnsdp::CrownArgs a;
  a.K = h->K; a.xdims = h->dxd.p; a.moff = h->dmo.p; a.acoff = h->dao.p; a.M = h->dM.p; a.acdim = h->acdim;
  a.nlit = h->nlit; a.H = h->dM.p + h->moff[h->K];      // (scratch and outputs: per level, reserve_boxes may move them)
  nnsdp::FwdArgs f;
  f.K = h->K; f.xdims = h->dxd.p; f.moff = h->dmo.p; f.M = h->dM.p; f.X = s.X; f.Y = D + o_Y; f.activ = h->activ; f.wp = h->wp;
  const size_t fwd_lds = 2 * (size_t)h->wp * 16 * sizeof(double);

  int cur = 0, nlevel = 1, nb = 0, vis = 0, depth = 0, verd = -1;
  long long log_n = 0, log_before = 0;
  double ms_all = 0.0;
  std::vector<double> wit;
  for (;;) {
    nb = std::min(nlevel, max_boxes - vis);      // (>= 1: a level that uses the budget up is the last one)
    vis += nb;
    log_before = log_n;
    h->reserve_boxes(std::min(cb, (size_t)nb), false, cb);      // (the stream is idle here: the bound kernel's buffers grow with the levels)
    a.scratch = h->dscr.p;
    s.nb = nb; s.depth = depth; s.lo = flo[cur]; s.hi = fhi[cur]; s.cuts = fcu[cur];
    s.nlo = flo[cur ^ 1]; s.nhi = fhi[cur ^ 1]; s.ncuts = fcu[cur ^ 1]; s.log_base = log_n;
    HIPCHK(hipEventRecord(h->e0, st));
    for (int off = 0; off < nb; off += (int)cb) {
      const size_t nc = std::min(cb, (size_t)(nb - off)), na = nc * h->acdim, ny_all = nc * ny, nl_all = nc * (size_t)h->nlit;
      // the layout of nnsdp_crown_bound for nc boxes
      a.lo = flo[cur] + (size_t)off * n0; a.hi = fhi[cur] + (size_t)off * n0;
      a.acymin = h->dout.p; a.acymax = a.acymin + na; a.acxmin = a.acymin + 2 * na; a.acxmax = a.acymin + 3 * na;
      a.ymin = a.acymin + 4 * na; a.ymax = a.ymin + ny_all;
      a.smin = a.ymax + ny_all; a.smax = a.smin + nl_all; a.ub0 = a.smax + nl_all; a.uA = a.ub0 + nl_all;
      if (h->activ == NNSDP_ACTIV_TANH)
        hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbTanh>, dim3((unsigned)nc), dim3(256), nnsdp::kCbLdsBytesTanh, st, a);
      else
        hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbRelu>, dim3((unsigned)nc), dim3(256), nnsdp::kCbLdsBytes, st, a);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(nnsdp::k_search_classify, dim3((unsigned)cdiv((long long)nc, 256)), dim3(256), 0, st, s, off, (int)nc,
                         (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
      HIPCHK(hipGetLastError());
      ++h->n_bound;
    }
    const long long npts = (long long)nb * (corner_points ? 2 : 1);
    f.N = npts;
    hipLaunchKernelGGL(nnsdp::k_forward_mfma, dim3((unsigned)((npts + 15) / 16)), dim3(64), fwd_lds, st, f);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(nnsdp::k_search_refute, dim3((unsigned)cdiv(npts, 256)), dim3(256), 0, st, s, npts);
    HIPCHK(hipGetLastError());
    const bool stop = vis >= max_boxes || depth >= max_depth || splitmask == 0;
    hipLaunchKernelGGL(nnsdp::k_search_scan, dim3(1), dim3(256), 0, st, s, npts);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(nnsdp::k_search_scatter, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, s, stop ? 0 : 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->e1, st));
    HIPCHK(hipMemcpyAsync(h->hstatus, s.status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
    ms_all += ms;
    const int nproved = h->hstatus[1], nopen = h->hstatus[2], ncand = h->hstatus[3];
    if (h->hstatus[0] != nb || nproved + nopen != nb) throw std::runtime_error("nnsdp_crown_search: inconsistent status record");
    log_n += nproved;
    if (ncand > 0) {      // the level's flags and points, walked in the Python driver's order: the centres in box order, then the corners
      std::vector<int> pf((size_t)npts);
      std::vector<double> X((size_t)npts * n0);
      HIPCHK(hipMemcpy(pf.data(), s.pflag, pf.size() * sizeof(int), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(X.data(), s.X, X.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (long long p = 0; p < npts && wit.empty(); ++p)
        if (pf[(size_t)p] && (!confirm || confirm(user, X.data() + (size_t)p * n0) != 0)) wit.assign(X.begin() + (size_t)p * n0, X.begin() + (size_t)(p + 1) * n0);
    }
    if (!wit.empty()) { verd = 1; break; }
    if (nopen == 0) { verd = nb < nlevel ? 2 : 0; break; }
    if (stop) { verd = 2; break; }
    cur ^= 1; nlevel = 2 * nopen; ++depth;
  }
  // the leaves in the order of the Python loop: the log up to the last level, the boxes of the last level that the budget kept from
  // being bounded, the last level's proved boxes, its open boxes
  std::vector<double> log((size_t)log_n * logw), lo((size_t)nlevel * n0), hi((size_t)nlevel * n0), bnd((size_t)nb);
  std::vector<int> open((size_t)nb), best((size_t)nb);
  if (log_n) HIPCHK(hipMemcpy(log.data(), s.log, log.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lo.data(), flo[cur], lo.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), fhi[cur], hi.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bnd.data(), s.bound, bnd.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(open.data(), s.open, open.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(best.data(), s.best, best.size() * sizeof(int), hipMemcpyDeviceToHost));
  nnsdp_crown::SearchLeaves& L = h->leaves;
  const size_t nleaf = (size_t)log_n + (size_t)(nlevel - nb) + (size_t)h->hstatus[2];
  L.lo.reserve(nleaf * n0); L.hi.reserve(nleaf * n0); L.depth.reserve(nleaf); L.proved.reserve(nleaf); L.literal.reserve(nleaf); L.bound.reserve(nleaf);
  auto leaf = [&](const double* blo, const double* bhi, int d, int proved, int literal, double bound) {
    L.lo.insert(L.lo.end(), blo, blo + n0); L.hi.insert(L.hi.end(), bhi, bhi + n0);
    L.depth.push_back(d); L.proved.push_back(proved); L.literal.push_back(literal); L.bound.push_back(bound);
  };
  auto from_log = [&](long long r) {
    const double* row = log.data() + (size_t)r * logw;
    leaf(row, row + n0, (int)row[2 * n0], 1, (int)row[2 * n0 + 1], row[2 * n0 + 2]);
  };
  auto from_frontier = [&](int b, int literal, double bound) { leaf(lo.data() + (size_t)b * n0, hi.data() + (size_t)b * n0, depth, 0, literal, bound); };
  for (long long r = 0; r < log_before; ++r) from_log(r);
  for (int b = nb; b < nlevel; ++b) from_frontier(b, -1, 0.0);
  for (long long r = log_before; r < log_n; ++r) from_log(r);
  for (int b = 0; b < nb; ++b)
    if (open[b]) from_frontier(b, best[b], bnd[b]);
  *verdict = verd; *visited = vis; *depth_reached = depth; *nleaves = (int32_t)L.depth.size();
  if (verd == 1) std::copy(wit.begin(), wit.end(), witness);
  if (kernel_ms) *kernel_ms = ms_all;
  API_END
}

int nnsdp_crown_search_leaves(nnsdp_crown* h, double* lo, double* hi, int32_t* depth, int32_t* proved, int32_t* literal, double* bound) {
  API_BEGIN
  if (!h) throw std::invalid_argument("null handle");
  const nnsdp_crown::SearchLeaves& L = h->leaves;
  if (!L.depth.empty() && (!lo || !hi || !depth || !proved || !literal || !bound)) throw std::invalid_argument("null argument");
  std::copy(L.lo.begin(), L.lo.end(), lo);
  std::copy(L.hi.begin(), L.hi.end(), hi);
  std::copy(L.depth.begin(), L.depth.end(), depth);
  std::copy(L.proved.begin(), L.proved.end(), proved);
  std::copy(L.literal.begin(), L.literal.end(), literal);
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
    default: throw std::invalid_argument("nnsdp_crown_info: what must be in 0..5");
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
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, nullptr));
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
  HIPCHK(hipEventRecord(e1, nullptr));
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
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
  if (const char* e = std::getenv("NNSDP_SPLIT_WARM")) {       // (test hook) two workgroups per block, as a solver's warm launches run
    if (std::atoi(e) != 0 && plan.split_ok() && batch <= 120) { split.alloc(batch); split.bind(a, batch); }
  }
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
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
  if (split.failed()) throw HipError("projection kernel, two workgroups per block: a helper workgroup did not deliver its tiles in time");
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
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  cd.reserve(batch);
  HIPCHK(hipEventRecord(e0, nullptr));
  cd.launch(dz.p, pat.NE, batch, nullptr);
  HIPCHK(hipEventRecord(e1, nullptr));
  HIPCHK(hipDeviceSynchronize());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
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
