// CROWN-sliced interval bounds of many input boxes of one ReLU network in one launch (nnsdp_make_intervals_batch): the
// screening stage of input splitting (nnsdp_amd/split.py).  The recurrences are those of make_intervals / crown_backward in
// intervals.hpp, every quantity in fp64 (the host routine keeps float32 for parity with the reference's torch path).
//
// One workgroup of 256 threads per box, so a box's bits depend neither on nbox nor on its position.  The coefficient
// matrices lA, uA of a backward pass (at most 64 x 64) live in LDS, one copy each, stored [column t][row i] with the
// 16-row tiles of odd columns swapped (cb_idx), so the MFMA operand read - lanes 0..15 column t, lanes 16..31 column
// t + 1, 16 consecutive rows each - touches 64 different banks.  Per layer j of a pass:
//   1. the relaxation of layer j from its pre-activation bounds (global scratch, written by an earlier pass of this workgroup),
//   2. thread (matrix, row) scales its row by the sign-split slopes and accumulates its two bias terms, t ascending,
//   3. A <- A W_j on v_mfma_f64_16x16x4_f64: wave w owns the output columns 16 w .. 16 w + 15 of both matrices (8 tiles), W_j
//      is read from global memory / L2 in chunks of kCbChunk k-steps, the tiles stay in registers across a barrier and are
//      written back over A.
// Then thread (matrix, row) concretises its row over the box.  No atomics; 68 KB of LDS (69 632 B), two workgroups per CU.
//
// Literal pass (nlit > 0, nnsdp_make_intervals_batch_lits): after the K output passes the pre-activation bounds of every hidden
// layer are in the scratch, so one more pass whose head is H = [C W_{K-1} | C b_{K-1}] (nlit x (xdims[K-1] + 1), one row per literal
// normal, computed once on the host) bounds  normal' f(x)  directly instead of through the per-output boxes.  It is the same
// row pass and the same MFMA product with nout = nlit; its results are raw (no post-fix), and the upper bound's linear form
// uA x + ub0 is written out beside them (smax = uA c + |uA| r + ub0).  Every output element of the product is its own dot product
// and the row passes are per row, so a literal's bits do not depend on the other literals of the call.
//
// Resident kernel (k_crown_resident<ACT>, launched by the nnsdp_crown handle of crown_handle.hpp on its own buffers): the same passes
// as a template on the activation.  ACT = kCbRelu is the arithmetic above, operation for operation.  ACT = kCbTanh restates
// tanh_relax / crown_backward(..., tanh_act = true) of intervals.hpp in fp64: the relaxation  lw x + lb <= tanh(x) <= uw x + ub  of
// a layer is computed ONCE, by the pre-activation pass that produces the layer's bounds (threads tid < nout, right after l, u go to
// the scratch), and its four numbers are stored beside the bounds - the Tanh scratch is 6 acdim doubles per box: l, u, lw, lb, uw, ub.
// Every later pass reads them (the tangent-point bisection is a chain of ~200 dependent tanh / cosh evaluations; 2K - 1 passes visit
// every layer below them).  The row pass gains the lower relaxation's bias, one more 64-double vector: 70 144 B of LDS
// (kCbLdsBytesTanh), still two workgroups per CU.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace nnsdp {

struct CrownArgs {
  int K;                    // affine layers (>= 2)
  const int* xdims;         // K + 1 widths, each <= 64
  const long long* moff;    // offset of M_k = [W_k b_k] (xdims[k+1] x (xdims[k] + 1), column-major) in M
  const int* acoff;         // K entries: acoff[j] = xdims[1] + ... + xdims[j], where the outputs of affine layer j start; acoff[K-1] = acdim
  const double* M;
  const double* lo;         // xdims[0] x nbox, column-major
  const double* hi;
  double* scratch;          // 2 acdim per box: CROWN pre-activation bounds (lower, then upper); Tanh: 6 acdim, + lw, lb, uw, ub
  double *acymin, *acymax, *acxmin, *acxmax;   // acdim x nbox
  double *ymin, *ymax;      // xdims[K] x nbox
  int acdim;
  // literal pass (nlit == 0: none, the pointers below are unused)
  int nlit;                 // 0 .. 64
  const double* H;          // nlit x (xdims[K-1] + 1), column-major like an M_k block
  double *smin, *smax;      // nlit x nbox, raw
  double* uA;               // xdims[0] x nlit x nbox, coefficient index fastest
  double* ub0;              // nlit x nbox
};

// The node of a ReLU split (crown_relu_split.hpp), read by crown_pass<.., SPLIT = true> alone: the assignment of the node's hidden
// neurons (+1: z >= 0, -1: z <= 0, 0: free), where the literal pass records its branching neuron, and the thread's copy of the
// node's infeasibility flag (the same value in all 256 threads).
struct CrownSplit {
  const int8_t* assign;     // acdim x nnode
  double* branch;           // nlit x nnode, a neuron index or -1, as a double (one download brings everything back)
  int infeasible;
};

static constexpr int kCbW = 64;        // widest layer
static constexpr int kCbChunk = 8;     // k-steps whose weight operands are in flight together
static constexpr size_t kCbLdsBytes = (2 * kCbW * kCbW + 8 * kCbW) * sizeof(double);
static constexpr size_t kCbLdsBytesTanh = kCbLdsBytes + kCbW * sizeof(double);      // + the lower relaxation's bias
static constexpr int kCbRelu = 0, kCbTanh = 1;      // the values of NNSDP_ACTIV_RELU / NNSDP_ACTIV_TANH

// ---- host side: the layouts the kernels of this file and of forward.hpp are launched on, each stated once ----

// A network given as (K, xdims): what CrownArgs / FwdArgs call xdims, moff, acoff and wp.  Arithmetic only - the entries refuse K, null
// pointers and widths themselves, before they build this (their messages and the order of their refusals differ).
struct NetLayout {
  std::vector<int> xd, acoff;
  std::vector<long long> moff;
  int wp = 0;               // FwdArgs::wp
  NetLayout(int K, const int32_t* xdims) : xd(xdims, xdims + K + 1), acoff(K, 0), moff(K + 1, 0) {
    for (int k = 0; k < K; ++k) {
      moff[k + 1] = moff[k] + (long long)xd[k + 1] * (xd[k] + 1);
      if (k > 0) acoff[k] = acoff[k - 1] + xd[k];
      wp = std::max(wp, (xd[k] + 1 + 3) & ~3);
    }
  }
  int K() const { return (int)acoff.size(); }
  int n0() const { return xd.front(); }
  int ny() const { return xd.back(); }
  int acdim() const { return acoff.back(); }
  size_t mlen() const { return (size_t)moff.back(); }
  // the literal head H = [C W_{K-1} | C b_{K-1}] sits behind M
  size_t head_len(int nlit) const { return nlit > 0 ? (size_t)nlit * (xd[K() - 1] + 1) : 0; }
};

// the refusal of a box that is empty or not finite, shared by the entries that bound many boxes (lo, hi: n0 x nbox, column-major)
inline void check_boxes(long long nbox, int n0, const double* lo, const double* hi) {
  for (long long b = 0; b < nbox; ++b)
    for (int i = 0; i < n0; ++i)
      if (!std::isfinite(lo[b * n0 + i]) || !std::isfinite(hi[b * n0 + i]) || !(lo[b * n0 + i] <= hi[b * n0 + i]))
        throw std::invalid_argument("box " + std::to_string(b) + ": x1min must be <= x1max and both finite (no NaN, no infinity)");
}

// The kernel's outputs for nbox boxes, packed so that one copy brings everything back: ten segments in the order
//   acymin | acymax | acxmin | acxmax | ymin | ymax | smin | smax | ub0 | uA
// The alpha kernel (crown_alpha.hpp) appends  a_smax | a_ub0 | a_step | a_uA | alpha  (CrownOptArgs::smax, ub0, step, uA of crown_opt.hpp,
// then CrownAlphaArgs::alpha) and keeps three nst()-long state arrays.
struct CrownLayout {
  size_t nbox, n0, acdim, ny, nlit;
  static constexpr int kSegs = 10;
  size_t na() const { return nbox * acdim; }
  size_t ny_all() const { return nbox * ny; }
  size_t nl() const { return nbox * nlit; }
  size_t nA() const { return nl() * n0; }
  size_t nst() const { return nl() * acdim; }
  void lens(size_t* len) const {
    const size_t l[kSegs] = {na(), na(), na(), na(), ny_all(), ny_all(), nl(), nl(), nl(), nA()};
    std::copy(l, l + kSegs, len);
  }
  size_t total() const { return 4 * na() + 2 * ny_all() + 3 * nl() + nA(); }
  size_t alpha_total() const { return total() + 3 * nl() + nA() + nst(); }
  // the output pointers of `a` into a buffer of total() doubles, with the two counts the kernel reads of the layout
  void point(CrownArgs& a, double* base) const {
    a.acdim = (int)acdim; a.nlit = (int)nlit;
    a.acymin = base; a.acymax = a.acymin + na(); a.acxmin = a.acymax + na(); a.acxmax = a.acxmin + na();
    a.ymin = a.acxmax + na(); a.ymax = a.ymin + ny_all();
    a.smin = a.ymax + ny_all(); a.smax = a.smin + nl(); a.ub0 = a.smax + nl(); a.uA = a.ub0 + nl();
  }
  // n consecutive segments of a host copy `src` to the caller's arrays; a null pointer skips its segment.  Returns the end in src.
  static const double* copy_segments(const double* src, int n, const size_t* len, double* const* host) {
    for (int o = 0; o < n; src += len[o], ++o)
      if (host[o]) std::copy(src, src + len[o], host[o]);
    return src;
  }
};

__device__ __forceinline__ int cb_idx(int t, int i) { return t * kCbW + (i ^ ((t & 1) << 4)); }

// ---- tanh relaxation in fp64: tanh_relax of intervals.hpp line by line, with the host's constants (clamps at +-500, derivative
// mask at |x| < 25, the 1e-6 width switch, the 0.01 grid of the tangent-point look-up, the doubling search then 100 halvings)
__device__ inline double cb_dtanh(double x) {
  if (!(fabs(x) < 25.0)) return 0.0;
  const double c = cosh(x);
  return 1.0 / (c * c);
}
__device__ inline double cb_tanh_d_lower(double upper) {
  const long iu = (long)(upper / 0.01), idx = (iu > 0 ? iu : 0) + 1;
  const double U = 0.01 * (double)idx, fU = tanh(U);
  auto ok = [&](double d) { return cb_dtanh(d) * (U - d) + tanh(d) <= fU; };
  double l = -1.0, r = 0.0;
  for (int it = 0; it < 64 && !ok(l); ++it) l *= 2.0;
  for (int it = 0; it < 100; ++it) { const double m = (l + r) / 2.0; if (ok(m)) l = m; else r = m; }
  return l;
}
__device__ inline double cb_tanh_d_upper(double lower) {
  const long il = (long)(lower / -0.01), idx = (il > 0 ? il : 0) + 1;
  const double Lw = -0.01 * (double)idx, fL = tanh(Lw);
  auto ok = [&](double d) { return cb_dtanh(d) * (Lw - d) + tanh(d) >= fL; };
  double l = 0.0, r = 1.0;
  for (int it = 0; it < 64 && !ok(r); ++it) r *= 2.0;
  for (int it = 0; it < 100; ++it) { const double m = (l + r) / 2.0; if (ok(m)) r = m; else l = m; }
  return r;
}
// lw x + lb <= tanh(x) <= uw x + ub on [l, u]; only a crossing neuron (l < 0 < u) enters the bisections.  Two departures from the
// library, both for soundness (Tanh paragraph): l = u = 0 takes the l >= 0 regime alone (the library's two masks at once
// put the lower line above tanh(0) and the upper one below), and an end beyond the clamp at +-500 turns the line that the clamped
// fit would carry past it into a constant (tanh is monotone).  Any other interval keeps the library's operations and their bits.
__device__ inline void cb_tanh_relax(double l, double u, double& lw, double& lb, double& uw, double& ub) {
  const double lower = l > -500.0 ? l : -500.0, upper = u < 500.0 ? u : 500.0;
  const double yl = tanh(lower), yu = tanh(upper);
  const double wd = upper - lower;
  const double kd = wd < 1e-6 ? cb_dtanh(upper) : (yu - yl) / (wd > 1e-6 ? wd : 1e-6);
  const bool pos = l >= 0.0, neg = u <= 0.0 && !pos;
  const double m = (lower + upper) / 2.0, ym = tanh(m), km = cb_dtanh(m);
  lw = lb = uw = ub = 0.0;
  auto line = [](double k, double x0, double y0, double& w, double& b) { w += k; b += -x0 * k + y0; };
  const double fboth = 1.0 - (pos ? 1.0 : 0.0) - (neg ? 1.0 : 0.0);
  if (neg) { line(kd, lower, yl, uw, ub); line(km, m, ym, lw, lb); }
  if (pos) { line(kd, lower, yl, lw, lb); line(km, m, ym, uw, ub); }
  if (fboth != 0.0) {
    const double dl = cb_tanh_d_lower(upper), du = cb_tanh_d_upper(lower);
    double w = 0.0, b = 0.0;
    if (kd < cb_dtanh(lower)) line(kd, lower, yl, w, b); else line(cb_dtanh(dl), dl, tanh(dl), w, b);
    lw += fboth * w; lb += fboth * b;
    w = b = 0.0;
    if (kd < cb_dtanh(upper)) line(kd, lower, yl, w, b); else line(cb_dtanh(du), du, tanh(du), w, b);
    uw += fboth * w; ub += fboth * b;
  }
  if (u > 500.0) { lw = 0.0; lb = yl; }
  if (l < -500.0) { uw = 0.0; ub = yu; }
}

// One backward pass for box `box`.  head_identity == 0: bounds of W_{k-1} relu(... ) + b_{k-1}, i.e. the pre-activation of hidden
// layer k (k < K, raw, to the scratch) or the network output (k == K, post-fixed, to ymin / ymax).  head_identity == 1: the
// post-activation of hidden layer k through an identity head (post-fixed, to acymin / acymax).
// LIT: the literal pass (k == K, head_identity == 0): the head is a.H instead of M_{K-1}, nout = nlit, the results go raw to smin /
// smax with the upper bound's coefficients and constant to uA / ub0.
// ACT: the activation (kCbRelu / kCbTanh); the ReLU instance is what this function was before it had the parameter.
// SPLIT (ReLU only, LDS kCbLdsBytesTanh: v_bl marks the branching candidates): the passes on a node of a ReLU split.  A forced neuron's
// relaxation is exact (+1: du = dl = 1, -1: du = dl = 0, bu = 0 in both), a pre-activation pass clips the bounds it writes to the forced
// side and flags l > u, and the upper row of the literal pass records the free unstable neuron with the largest max(lambda, 0) bu
// (ties: the lowest neuron index).  SPLIT = false compiles to what the function was without the parameter.
// The ReLU relaxation stays inline here: cb_relu_relax (crown_opt.hpp, which includes this file) is the same arithmetic for the two
// optimisers, and this function's instantiations keep the code they had (profiles/crown_opt_resources.txt).
template <bool LIT, int ACT = kCbRelu, bool SPLIT = false>
__device__ void crown_pass(const CrownArgs& a, double* lds, long long box, int k, int head_identity, CrownSplit* sp = nullptr) {
  static_assert(!SPLIT || ACT == kCbRelu, "a ReLU split is for ReLU networks");
  double* A[2] = {lds, lds + kCbW * kCbW};
  double* v_du = lds + 2 * kCbW * kCbW;
  double* v_dl = v_du + kCbW;
  double* v_bu = v_dl + kCbW;
  double* v_bj = v_bu + kCbW;
  double* v_c = v_bj + kCbW;      // box centre
  double* v_r = v_c + kCbW;       // box radius
  double* v_res = v_r + kCbW;     // 2 x 64: a pass's lower / upper results, for the post-fix
  double* v_bl = v_res + 2 * kCbW;   // Tanh only (kCbLdsBytesTanh): the lower relaxation's bias
  constexpr int kScr = ACT == kCbTanh ? 6 : 2;      // doubles of scratch per hidden neuron
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lc = lane >> 4;
  const int mat = tid >> 6, row = tid & 63;      // the (matrix, row) a thread owns in the row passes (threads 0..127)
  const int nout = LIT ? a.nlit : a.xdims[k];
  int d = head_identity ? nout : a.xdims[k - 1];
  const int jtop = head_identity ? k - 1 : k - 2;
  double bias = 0.0;
  double br_score = -1.0;      // SPLIT, LIT, the upper rows: the best branching score so far and its neuron
  int br_n = -1;
  {
    const double* Mh = LIT ? a.H : a.M + a.moff[k - 1];
    for (int idx = tid; idx < nout * d; idx += 256) {
      const int t = idx / nout, i = idx - t * nout;
      const double v = head_identity ? (t == i ? 1.0 : 0.0) : Mh[(size_t)t * nout + i];
      A[0][cb_idx(t, i)] = v;
      A[1][cb_idx(t, i)] = v;
    }
    if (tid < 128 && row < nout && !head_identity) bias = Mh[(size_t)d * nout + row];
    if (tid < a.xdims[0]) {
      const double l = a.lo[(size_t)box * a.xdims[0] + tid], u = a.hi[(size_t)box * a.xdims[0] + tid];
      v_c[tid] = (u + l) / 2.0;
      v_r[tid] = (u - l) / 2.0;
    }
  }
  __syncthreads();
  for (int j = jtop; j >= 0; --j) {
    const int in = a.xdims[j];
    const double* Mj = a.M + a.moff[j];       // d x (in + 1), column-major
    if (ACT == kCbTanh) {
      if (tid < d) {
        const double* pre = a.scratch + (size_t)box * kScr * a.acdim + a.acoff[j] + tid;
        v_dl[tid] = pre[2 * (size_t)a.acdim];
        v_bl[tid] = pre[3 * (size_t)a.acdim];
        v_du[tid] = pre[4 * (size_t)a.acdim];
        v_bu[tid] = pre[5 * (size_t)a.acdim];
        v_bj[tid] = Mj[(size_t)in * d + tid];
      }
    } else if (tid < d) {
      const double* pre = a.scratch + (size_t)box * 2 * a.acdim + a.acoff[j];
      const double l = pre[tid], u = pre[a.acdim + tid];
      const double lrx = l < 0.0 ? l : 0.0;
      double ur = u > 0.0 ? u : 0.0;
      ur = ur > lrx + 1e-8 ? ur : lrx + 1e-8;
      const double du = ur / (ur - lrx);
      v_du[tid] = du;
      v_dl[tid] = du > 0.5 ? 1.0 : 0.0;
      v_bu[tid] = -lrx * du;
      v_bj[tid] = Mj[(size_t)in * d + tid];
      if (SPLIT) {
        const int sv = sp->assign[(size_t)box * a.acdim + a.acoff[j] + tid];
        if (sv != 0) {
          v_du[tid] = v_dl[tid] = sv > 0 ? 1.0 : 0.0;
          v_bu[tid] = 0.0;
        }
        v_bl[tid] = (sv == 0 && l < 0.0 && u > 0.0) ? 1.0 : 0.0;
      }
    }
    __syncthreads();
    if (tid < 128 && row < nout) {
      double* Am = A[mat];
      double s = 0.0, tl = 0.0;
      for (int t = 0; t < d; ++t) {
        const double x = Am[cb_idx(t, row)];
        const double xp = x > 0.0 ? x : 0.0, xn = x < 0.0 ? x : 0.0;
        const double du = v_du[t], dl = v_dl[t];
        if (ACT == kCbTanh) s += mat ? xp * v_bu[t] + xn * v_bl[t] : xn * v_bu[t] + xp * v_bl[t];
        else s += (mat ? xp : xn) * v_bu[t];
        if (SPLIT && LIT && mat && v_bl[t] != 0.0) {
          const double sc = xp * v_bu[t];
          const int n = a.acoff[j] + t;
          if (sc > br_score || (sc == br_score && n < br_n)) { br_score = sc; br_n = n; }
        }
        const double y = mat ? xp * du + xn * dl : xp * dl + xn * du;
        Am[cb_idx(t, row)] = y;
        tl += y * v_bj[t];
      }
      bias += s;
      bias += tl;
    }
    __syncthreads();
    // A (nout x d) <- A W_j (nout x in): MFMA operand a = A[16 it + lr][4 ks + lc] from LDS, b = W_j[4 ks + lc][16 w + lr] from global
    const int nit = (nout + 15) >> 4, nqt = (in + 15) >> 4, ks = (d + 3) >> 2;
    d4_t c[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int it = 0; it < 4; ++it) c[m][it] = d4_t{0.0, 0.0, 0.0, 0.0};
    const int q = 16 * w + lr;
    if (w < nqt) {
      for (int k0 = 0; k0 < ks; k0 += kCbChunk) {
        double bv[kCbChunk];
#pragma unroll
        for (int u = 0; u < kCbChunk; ++u) {
          const int t = 4 * (k0 + u) + lc;
          bv[u] = (q < in && t < d) ? Mj[(size_t)q * d + t] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kCbChunk; ++u) {
          if (k0 + u < ks) {
            const int t = 4 * (k0 + u) + lc;
            const int tc = t < d ? t : 0;      // a column past d multiplies a zero of bv: read a written one, never stale bits
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              if (it < nit) {
                const int i = 16 * it + lr;
                const bool ok = t < d && i < nout;
                const double al = ok ? A[0][cb_idx(tc, i)] : 0.0;
                const double au = ok ? A[1][cb_idx(tc, i)] : 0.0;
                c[0][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bv[u], c[0][it], 0, 0, 0);
                c[1][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv[u], c[1][it], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    __syncthreads();
    if (w < nqt && q < in) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        if (it < nit) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * it + lc + 4 * r;
            if (i < nout) {
              A[0][cb_idx(q, i)] = c[0][it][r];
              A[1][cb_idx(q, i)] = c[1][it][r];
            }
          }
        }
      }
    }
    d = in;
    __syncthreads();
  }
  if (tid < 128 && row < nout) {
    const double* Am = A[mat];
    double s = 0.0, rr = 0.0;
    for (int t = 0; t < d; ++t) {
      const double x = Am[cb_idx(t, row)];
      s += x * v_c[t];
      rr += fabs(x) * v_r[t];
    }
    v_res[mat * kCbW + row] = mat ? s + rr + bias : s - rr + bias;
    if (LIT && mat && a.ub0) a.ub0[(size_t)box * nout + row] = bias;
    if (SPLIT && LIT && mat) sp->branch[(size_t)box * nout + row] = (double)br_n;
  }
  __syncthreads();
  if (LIT) {
    if (tid < nout) {
      if (a.smin) a.smin[(size_t)box * nout + tid] = v_res[tid];
      if (a.smax) a.smax[(size_t)box * nout + tid] = v_res[kCbW + tid];
    }
    if (a.uA)
      for (int idx = tid; idx < nout * d; idx += 256) {       // d == xdims[0] here; A[1] is the upper bound's matrix after the last product
        const int i = idx / d, t = idx - i * d;
        a.uA[((size_t)box * nout + i) * d + t] = A[1][cb_idx(t, i)];
      }
  } else if (SPLIT && !head_identity && k < a.K) {
    bool bad = false;
    if (tid < nout) {
      double l = v_res[tid], u = v_res[kCbW + tid];
      const int sv = sp->assign[(size_t)box * a.acdim + a.acoff[k - 1] + tid];
      if (sv > 0) l = l > 0.0 ? l : 0.0;
      if (sv < 0) u = u < 0.0 ? u : 0.0;
      bad = l > u;
      double* pre = a.scratch + (size_t)box * kScr * a.acdim + a.acoff[k - 1];
      pre[tid] = l;
      pre[a.acdim + tid] = u;
    }
    // the node's flag through LDS, read back in a fixed order by every thread; the kernel stores it from one thread
    __syncthreads();
    if (tid < nout) v_res[tid] = bad ? 1.0 : 0.0;
    __syncthreads();
    for (int t = 0; t < nout; ++t)
      if (v_res[t] != 0.0) sp->infeasible = 1;
  } else if (tid < nout) {
    const double l = v_res[tid], u = v_res[kCbW + tid];
    if (!head_identity && k < a.K) {
      double* pre = a.scratch + (size_t)box * kScr * a.acdim + a.acoff[k - 1];
      pre[tid] = l;
      pre[a.acdim + tid] = u;
      if (ACT == kCbTanh) {      // the layer's relaxation, once: every later pass reads it
        double lw, lb, uw, ub;
        cb_tanh_relax(l, u, lw, lb, uw, ub);
        pre[2 * (size_t)a.acdim + tid] = lw;
        pre[3 * (size_t)a.acdim + tid] = lb;
        pre[4 * (size_t)a.acdim + tid] = uw;
        pre[5 * (size_t)a.acdim + tid] = ub;
      }
    } else {
      const double fl = l < u ? l : u, fu = fl > u ? fl : u;     // lb = min(lb, ub), ub = max(lb, ub)
      if (head_identity) {
        const size_t o = (size_t)box * a.acdim + a.acoff[k - 1] + tid;
        a.acymin[o] = fl;
        a.acymax[o] = fu;
      } else {
        const size_t o = (size_t)box * nout + tid;
        a.ymin[o] = fl;
        a.ymax[o] = fu;
      }
    }
  }
  __threadfence_block();
  __syncthreads();
}

// one interval step per layer for the pre-activations, from the post-fixed bounds of the layer below
__device__ __forceinline__ void crown_interval_step(const CrownArgs& a, long long box) {
  const int n0 = a.xdims[0];
  for (int idx = threadIdx.x; idx < a.acdim; idx += 256) {
    int k = 0;
    while (idx >= a.acoff[k + 1]) ++k;                   // affine layer k: acoff[k] <= idx < acoff[k + 1]
    const int r = a.xdims[k + 1], cdim = a.xdims[k], i = idx - a.acoff[k];
    const double* Mk = a.M + a.moff[k];
    const double* xl = k ? a.acymin + (size_t)box * a.acdim + a.acoff[k - 1] : a.lo + (size_t)box * n0;
    const double* xu = k ? a.acymax + (size_t)box * a.acdim + a.acoff[k - 1] : a.hi + (size_t)box * n0;
    double sl = Mk[(size_t)cdim * r + i], su = sl;
    for (int j = 0; j < cdim; ++j) {
      const double wv = Mk[(size_t)j * r + i];
      if (wv >= 0) { sl += wv * xl[j]; su += wv * xu[j]; }
      else { sl += wv * xu[j]; su += wv * xl[j]; }
    }
    a.acxmin[(size_t)box * a.acdim + idx] = sl;
    a.acxmax[(size_t)box * a.acdim + idx] = su;
  }
}

__global__ __launch_bounds__(256) void k_crown_batch(CrownArgs a) {
  extern __shared__ double cb_lds[];
  const long long box = blockIdx.x;
  for (int k = 1; k <= a.K; ++k) {
    crown_pass<false>(a, cb_lds, box, k, 0);
    if (k < a.K) crown_pass<false>(a, cb_lds, box, k, 1);
  }
  if (a.nlit > 0) crown_pass<true>(a, cb_lds, box, a.K, 0);
  crown_interval_step(a, box);
}

// The kernel of the resident bounder (nnsdp_crown): every buffer of `a` belongs to the handle; LDS kCbLdsBytes (ReLU) /
// kCbLdsBytesTanh (Tanh).
template <int ACT>
__global__ __launch_bounds__(256) void k_crown_resident(CrownArgs a) {
  extern __shared__ double cb_lds[];
  const long long box = blockIdx.x;
  for (int k = 1; k <= a.K; ++k) {
    crown_pass<false, ACT>(a, cb_lds, box, k, 0);
    if (k < a.K) crown_pass<false, ACT>(a, cb_lds, box, k, 1);
  }
  if (a.nlit > 0) crown_pass<true, ACT>(a, cb_lds, box, a.K, 0);
  crown_interval_step(a, box);
}

}  // namespace nnsdp
