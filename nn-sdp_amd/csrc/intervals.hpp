// Interval pre-processing on the host: CROWN-sliced bounds of every
// hidden layer, the direct inputs of the LMI assembler (acymin/acymax of QcActivBounded, smin/smax of
// QcActivSector).  Replaces Intervals.intervalsAutoLirpaSliced (src/Intervals/intervals_auto_lirpa.jl:12-64),
// which reaches auto_LiRPA 0.2 through PyCall + ONNX once per layer (exts/auto_lirpa_bridge.py:97-112).
// Rules restated from the vendored library (exts/auto_LiRPA/operators/activation.py:306-323,386-388,
// bound_general.py:1078-1079): backward LiRPA for the final node and for every intermediate pre-activation;
// ReLU relaxation lb_r = min(l,0), ub_r = max(max(u,0), lb_r + 1e-8), upper slope d = ub_r/(ub_r - lb_r) with
// intercept -lb_r d, lower slope 1 if d > 0.5 else 0.  float32 like the reference's torch path
// (exts/NNet/converters/nnet2onnx.py:47,51), the Julia post-fix lb = min(lb,ub), ub = max(lb,ub)
// (intervals_auto_lirpa.jl:38-39), then one float64 interval step per layer for the pre-activations (:55-62).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace nnsdp {

struct DenseF {             // row-major float matrix
  int r = 0, c = 0;
  std::vector<float> a;
  DenseF() {}
  DenseF(int r_, int c_) : r(r_), c(c_), a((size_t)r_ * c_, 0.0f) {}
  float& at(int i, int j) { return a[(size_t)i * c + j]; }
  float at(int i, int j) const { return a[(size_t)i * c + j]; }
};

struct IntervalsOut {
  std::vector<std::vector<double>> xlo, xhi;      // K+1 post-activation intervals (x_1 .. x_K, output)
  std::vector<std::vector<double>> plo, phi;      // K-1 pre-activation intervals (float64 interval step)
  // with a literal head (LitHead): raw bounds of the literals, and the upper bound's linear form  uA x + ub0  (uA row-major nlit x n0)
  std::vector<double> smin, smax, uA, ub0;
  std::vector<std::vector<float>> prel, preu;     // the raw float32 pre-activation bounds the backward passes used (lits_alpha reads them)
};

// The head of a literal pass: H = [C W_{K-1} | C b_{K-1}] for the nlit x ny matrix C of literal normals (normals: ny x nlit,
// column-major), in fp64 with plain sums over ascending index.  Stored like an M_k block: nlit x (xdims[K-1] + 1), column-major.
struct LitHead {
  int nlit = 0, d = 0;
  std::vector<double> H;
};
inline LitHead make_lit_head(int K, const int32_t* xdims, const double* M, int nlit, const double* normals) {
  LitHead h;
  h.nlit = nlit; h.d = xdims[K - 1];
  const int ny = xdims[K], d = h.d;
  size_t off = 0;
  for (int k = 0; k + 1 < K; ++k) off += (size_t)xdims[k + 1] * (xdims[k] + 1);
  const double* Mk = M + off;                  // ny x (d + 1), column-major
  h.H.assign((size_t)nlit * (d + 1), 0.0);
  for (int t = 0; t <= d; ++t)
    for (int i = 0; i < nlit; ++i) {
      double s = 0.0;
      for (int j = 0; j < ny; ++j) s += normals[(size_t)i * ny + j] * Mk[(size_t)t * ny + j];
      h.H[(size_t)t * nlit + i] = s;
    }
  return h;
}

// ---- tanh relaxation (exts/auto_LiRPA/operators/activation.py BoundTanh: dtanh :863-868, precompute_relaxation :872-917,
// bound_relax_impl, non-optimised branch :925-956,992-1016; the reference's bridge maps torch.nn.Tanh onto it,
// exts/auto_lirpa_bridge.py:31-37,86-87).  float32 like the library's default dtype.
inline float dtanh_f(float x) {
  if (!(std::fabs(x) < 25.0f)) return 0.0f;        // (mask: cosh(25)^2 overflows float32)
  const float c = std::cosh(x);
  return 1.0f / (c * c);
}
// the table entries the relaxation looks up, computed on demand: tangent point d <= 0 whose tangent stays below tanh at
// U = 0.01 (max(0, int(u / 0.01)) + 1), and its mirror image for the lower end (bisection, 100 halvings as the library's)
inline float tanh_d_lower(float upper) {
  const long idx = std::max(0L, (long)(upper / 0.01f)) + 1;
  const float U = 0.01f * (float)idx, fU = std::tanh(U);
  auto ok = [&](float d) { return dtanh_f(d) * (U - d) + std::tanh(d) <= fU; };
  float l = -1.0f, r = 0.0f;
  for (int it = 0; it < 64 && !ok(l); ++it) l *= 2.0f;
  for (int it = 0; it < 100; ++it) { const float m = (l + r) / 2.0f; if (ok(m)) l = m; else r = m; }
  return l;
}
inline float tanh_d_upper(float lower) {
  const long idx = std::max(0L, (long)(lower / -0.01f)) + 1;
  const float Lw = -0.01f * (float)idx, fL = std::tanh(Lw);
  auto ok = [&](float d) { return dtanh_f(d) * (Lw - d) + std::tanh(d) >= fL; };
  float l = 0.0f, r = 1.0f;
  for (int it = 0; it < 64 && !ok(r); ++it) r *= 2.0f;
  for (int it = 0; it < 100; ++it) { const float m = (l + r) / 2.0f; if (ok(m)) r = m; else l = m; }
  return r;
}
// lw x + lb <= tanh(x) <= uw x + ub on [l, u].  Two departures from the library, both for soundness (Tanh paragraph):
// l = u = 0 takes the l >= 0 regime alone, and an end beyond the clamp at +-500 turns the line that the clamped fit would carry past
// it into a constant.  Any other interval keeps the library's operations.
inline void tanh_relax(float l, float u, float& lw, float& lb, float& uw, float& ub) {
  const float lower = std::max(l, -500.0f), upper = std::min(u, 500.0f);
  const float yl = std::tanh(lower), yu = std::tanh(upper);
  const float kd = (upper - lower) < 1e-6f ? dtanh_f(upper) : (yu - yl) / std::max(upper - lower, 1e-6f);
  const bool pos = l >= 0.0f, neg = u <= 0.0f && !pos;
  const float m = (lower + upper) / 2.0f, ym = std::tanh(m), km = dtanh_f(m);
  lw = lb = uw = ub = 0.0f;
  auto line = [](float k, float x0, float y0, float& w, float& b) { w += k; b += -x0 * k + y0; };
  // (in the library a neuron with l = u = 0 carries BOTH masks and mask_both = 1 - pos - neg = -1; here the masks are exclusive)
  const float fpos = pos ? 1.0f : 0.0f, fneg = neg ? 1.0f : 0.0f, fboth = 1.0f - fpos - fneg;
  if (neg) { line(kd, lower, yl, uw, ub); line(km, m, ym, lw, lb); }
  if (pos) { line(kd, lower, yl, lw, lb); line(km, m, ym, uw, ub); }
  if (fboth != 0.0f) {
    const float dl = tanh_d_lower(upper), du = tanh_d_upper(lower);
    float w = 0.0f, b = 0.0f;
    if (kd < dtanh_f(lower)) line(kd, lower, yl, w, b); else line(dtanh_f(dl), dl, std::tanh(dl), w, b);
    lw += fboth * w; lb += fboth * b;
    w = b = 0.0f;
    if (kd < dtanh_f(upper)) line(kd, lower, yl, w, b); else line(dtanh_f(du), du, std::tanh(du), w, b);
    uw += fboth * w; ub += fboth * b;
  }
  if (u > 500.0f) { lw = 0.0f; lb = yl; }
  if (l < -500.0f) { uw = 0.0f; ub = yu; }
}

// the ReLU relaxation from raw pre-activation bounds (the rules at the top of this file)
inline void relu_relax_f(float l, float u, float& du, float& dl, float& bu) {
  const float lr = std::min(l, 0.0f), ur = std::max(std::max(u, 0.0f), lr + 1e-8f);
  du = ur / (ur - lr);
  dl = du > 0.5f ? 1.0f : 0.0f;
  bu = -lr * du;
}

// backward bound of  Ws[L-1] act(... act(Ws[0] x + bs[0]) ...) + bs[L-1]  over the box [lo, hi] (act = relu, or tanh when tanh_act);
// pre[j] = pre-activation bounds of layer j (j < L-1).  The head is Ws[L-1] / bs[L-1], whatever it is (a layer of the network, an
// identity, a literal head); out_uA / out_ub (optional) receive the upper bound's linear form  uA x + ub  on the box.
inline void crown_backward(const std::vector<const DenseF*>& Ws, const std::vector<const std::vector<float>*>& bs,
                           const std::vector<std::vector<float>>& prel, const std::vector<std::vector<float>>& preu,
                           const std::vector<float>& lo, const std::vector<float>& hi, std::vector<float>& out_lo,
                           std::vector<float>& out_hi, bool tanh_act = false, DenseF* out_uA = nullptr,
                           std::vector<float>* out_ub = nullptr) {
  const int L = (int)Ws.size();
  DenseF lA = *Ws[L - 1], uA = *Ws[L - 1];
  const int nout = lA.r;
  std::vector<float> lb(*bs[L - 1]), ub(*bs[L - 1]);
  for (int j = L - 2; j >= 0; --j) {
    const int d = lA.c;                       // width of layer j's output
    std::vector<float> du(d), dl(d), bu(d), bl(d, 0.0f);
    for (int t = 0; t < d; ++t) {
      if (tanh_act) { tanh_relax(prel[j][t], preu[j][t], dl[t], bl[t], du[t], bu[t]); continue; }
      relu_relax_f(prel[j][t], preu[j][t], du[t], dl[t], bu[t]);
    }
    for (int i = 0; i < nout; ++i) {
      float sl = 0.0f, su = 0.0f;
      for (int t = 0; t < d; ++t) {
        float a = lA.at(i, t), b = uA.at(i, t);
        sl += std::min(a, 0.0f) * bu[t] + std::max(a, 0.0f) * bl[t];
        su += std::max(b, 0.0f) * bu[t] + std::min(b, 0.0f) * bl[t];
        lA.at(i, t) = std::max(a, 0.0f) * dl[t] + std::min(a, 0.0f) * du[t];
        uA.at(i, t) = std::max(b, 0.0f) * du[t] + std::min(b, 0.0f) * dl[t];
      }
      lb[i] += sl; ub[i] += su;
      float tl = 0.0f, tu = 0.0f;
      for (int t = 0; t < d; ++t) { tl += lA.at(i, t) * (*bs[j])[t]; tu += uA.at(i, t) * (*bs[j])[t]; }
      lb[i] += tl; ub[i] += tu;
    }
    const DenseF& W = *Ws[j];
    DenseF nl(nout, W.c), nu(nout, W.c);
    for (int i = 0; i < nout; ++i)
      for (int t = 0; t < d; ++t) {
        const float a = lA.at(i, t), b = uA.at(i, t);
        if (a == 0.0f && b == 0.0f) continue;
        const float* w = &W.a[(size_t)t * W.c];
        float* pl = &nl.a[(size_t)i * W.c];
        float* pu = &nu.a[(size_t)i * W.c];
        for (int q = 0; q < W.c; ++q) { pl[q] += a * w[q]; pu[q] += b * w[q]; }
      }
    lA = std::move(nl); uA = std::move(nu);
  }
  const int n0 = lA.c;
  out_lo.assign(nout, 0.0f); out_hi.assign(nout, 0.0f);
  for (int i = 0; i < nout; ++i) {
    float sl = 0.0f, su = 0.0f, rl = 0.0f, ru = 0.0f;
    for (int q = 0; q < n0; ++q) {
      const float c = (hi[q] + lo[q]) / 2.0f, r = (hi[q] - lo[q]) / 2.0f;
      sl += lA.at(i, q) * c; rl += std::fabs(lA.at(i, q)) * r;
      su += uA.at(i, q) * c; ru += std::fabs(uA.at(i, q)) * r;
    }
    out_lo[i] = sl - rl + lb[i];
    out_hi[i] = su + ru + ub[i];
  }
  if (out_uA) *out_uA = std::move(uA);
  if (out_ub) *out_ub = std::move(ub);
}

// M: K matrices [W_k b_k], column-major xdims[k+1] x (xdims[k]+1), back to back (include/nnsdp.h, nnsdp_problem::M)
// head (optional): one more backward pass from the literal head over layers K-2 .. 0, float32 like the others, after them; it
// changes none of the other outputs.
inline IntervalsOut make_intervals(int K, const int32_t* xdims, const double* M, const double* x1min, const double* x1max,
                                   bool tanh_act = false, const LitHead* head = nullptr) {
  if (K < 2 || !xdims || !M || !x1min || !x1max) throw std::invalid_argument("make_intervals: bad arguments");
  std::vector<DenseF> W(K);
  std::vector<std::vector<float>> b(K);
  std::vector<std::vector<double>> Wd(K), bd(K);
  size_t off = 0;
  for (int k = 0; k < K; ++k) {
    const int r = xdims[k + 1], c = xdims[k];
    if (r <= 0 || c <= 0) throw std::invalid_argument("make_intervals: layer widths must be positive");
    W[k] = DenseF(r, c); b[k].resize(r); Wd[k].resize((size_t)r * c); bd[k].resize(r);
    for (int j = 0; j < c; ++j)
      for (int i = 0; i < r; ++i) { double v = M[off + (size_t)j * r + i]; W[k].at(i, j) = (float)v; Wd[k][(size_t)i * c + j] = v; }
    for (int i = 0; i < r; ++i) { double v = M[off + (size_t)c * r + i]; b[k][i] = (float)v; bd[k][i] = v; }
    off += (size_t)r * (c + 1);
  }
  const int n0 = xdims[0];
  std::vector<float> lo(n0), hi(n0);
  for (int i = 0; i < n0; ++i) {
    if (!(x1min[i] <= x1max[i])) throw std::invalid_argument("make_intervals: x1min must be <= x1max");
    lo[i] = (float)x1min[i]; hi[i] = (float)x1max[i];
  }
  IntervalsOut out;
  out.xlo.emplace_back(x1min, x1min + n0); out.xhi.emplace_back(x1max, x1max + n0);
  std::vector<std::vector<float>> prel, preu;
  auto fix = [&](const std::vector<float>& l, const std::vector<float>& u) {
    std::vector<double> L(l.size()), U(l.size());
    for (size_t i = 0; i < l.size(); ++i) { L[i] = std::min((double)l[i], (double)u[i]); U[i] = std::max(L[i], (double)u[i]); }
    out.xlo.push_back(std::move(L)); out.xhi.push_back(std::move(U));
  };
  for (int k = 1; k <= K; ++k) {
    std::vector<const DenseF*> Ws;
    std::vector<const std::vector<float>*> bs;
    for (int j = 0; j < std::min(k, K); ++j) { Ws.push_back(&W[j]); bs.push_back(&b[j]); }
    std::vector<float> l, u;
    if (k < K) {
      // slice k (intervals_auto_lirpa.jl:12-28): pre-activation of layer k, then its post-activation through an identity head
      crown_backward(Ws, bs, prel, preu, lo, hi, l, u, tanh_act);
      prel.push_back(l); preu.push_back(u);
      const int n = xdims[k];
      DenseF I(n, n);
      for (int i = 0; i < n; ++i) I.at(i, i) = 1.0f;
      std::vector<float> zero(n, 0.0f);
      Ws.push_back(&I); bs.push_back(&zero);
      crown_backward(Ws, bs, prel, preu, lo, hi, l, u, tanh_act);
      fix(l, u);
    } else {
      crown_backward(Ws, bs, prel, preu, lo, hi, l, u, tanh_act);
      fix(l, u);
    }
  }
  if (head && head->nlit > 0) {
    const int nlit = head->nlit, d = xdims[K - 1];
    DenseF Hw(nlit, d), uA;
    std::vector<float> Hb(nlit), l, u, ub;
    for (int i = 0; i < nlit; ++i) {
      for (int t = 0; t < d; ++t) Hw.at(i, t) = (float)head->H[(size_t)t * nlit + i];
      Hb[i] = (float)head->H[(size_t)d * nlit + i];
    }
    std::vector<const DenseF*> Ws;
    std::vector<const std::vector<float>*> bs;
    for (int j = 0; j + 1 < K; ++j) { Ws.push_back(&W[j]); bs.push_back(&b[j]); }
    Ws.push_back(&Hw); bs.push_back(&Hb);
    crown_backward(Ws, bs, prel, preu, lo, hi, l, u, tanh_act, &uA, &ub);
    out.smin.assign(l.begin(), l.end()); out.smax.assign(u.begin(), u.end());
    out.uA.assign(uA.a.begin(), uA.a.end()); out.ub0.assign(ub.begin(), ub.end());
  }
  for (int k = 0; k + 1 < K; ++k) {           // float64 interval step per layer (intervals_auto_lirpa.jl:55-62)
    const int r = xdims[k + 1], c = xdims[k];
    std::vector<double> l(r), u(r);
    for (int i = 0; i < r; ++i) {
      double sl = bd[k][i], su = bd[k][i];
      for (int j = 0; j < c; ++j) {
        const double w = Wd[k][(size_t)i * c + j];
        if (w >= 0) { sl += w * out.xlo[k][j]; su += w * out.xhi[k][j]; }
        else { sl += w * out.xhi[k][j]; su += w * out.xlo[k][j]; }
      }
      l[i] = sl; u[i] = su;
    }
    out.plo.push_back(std::move(l)); out.phi.push_back(std::move(u));
  }
  out.prel = std::move(prel); out.preu = std::move(preu);
  return out;
}

// ---- the two projected-gradient optimisers of the literal pass's upper bound, the float32 twins of the kernels
// around crown_pg_body (crown_opt.hpp): lits_alpha on the lower slopes of the unstable neurons, make_intervals_nodes on the multipliers of
// a node's forced neurons.  Both fill a PgContext and run pg_literal per literal.

// What a backward row and the loop of a literal read: the hidden layers of (K, xdims, M) in float32 (W[k] row-major, bs[k]; aoff[k]:
// where layer k's neurons start, aoff[K - 1] = acdim), the box as centre and radius, the relaxation du, dl, bu of every hidden neuron
// (filled by the caller) and the step sizes
struct PgContext {
  int K;
  const int32_t* xdims;
  std::vector<DenseF> W;
  std::vector<std::vector<float>> bs;
  std::vector<int> aoff;
  std::vector<float> c0, r0, du, dl, bu;
  int steps;
  double eta0, decay;
  PgContext(int K_, const int32_t* xdims_, const double* M, const double* x1min, const double* x1max, int steps_, double eta0_, double decay_)
      : K(K_), xdims(xdims_), W(K_ - 1), bs(K_ - 1), aoff(K_, 0), c0(xdims_[0]), r0(xdims_[0]), steps(steps_), eta0(eta0_), decay(decay_) {
    size_t off = 0;
    for (int k = 0; k + 1 < K; ++k) {
      const int r = xdims[k + 1], c = xdims[k];
      W[k] = DenseF(r, c); bs[k].resize(r);
      for (int j = 0; j < c; ++j)
        for (int i = 0; i < r; ++i) W[k].at(i, j) = (float)M[off + (size_t)j * r + i];
      for (int i = 0; i < r; ++i) bs[k][i] = (float)M[off + (size_t)c * r + i];
      off += (size_t)r * (c + 1);
      aoff[k + 1] = aoff[k] + r;
    }
    for (int q = 0; q < xdims[0]; ++q) {
      const float lo = (float)x1min[q], hi = (float)x1max[q];
      c0[q] = (hi + lo) / 2.0f; r0[q] = (hi - lo) / 2.0f;
    }
    du.resize(acdim()); dl.resize(acdim()); bu.resize(acdim());
  }
  int acdim() const { return aoff.back(); }
};

// One row of a backward pass from layer `top` (its coefficients in `row`, its constant in `cst`) down to the input, concretised over the
// box: the upper bound (else the lower).  entry(n, b, sb) returns the coefficient b of neuron n behind the row scaling and adds its bias
// term to sb.  `row` ends as the input row; nxt is working space.
template <class Entry>
inline float backward_row(const PgContext& c, int top, bool upper, std::vector<float>& row, float& cst, std::vector<float>& nxt, Entry entry) {
  for (int j = top; j >= 0; --j) {
    const int d = c.xdims[j + 1], in = c.xdims[j], o = c.aoff[j];
    float sb = 0.0f;
    for (int t = 0; t < d; ++t) row[t] = entry(o + t, row[t], sb);
    cst += sb;
    float tl = 0.0f;
    for (int t = 0; t < d; ++t) tl += row[t] * c.bs[j][t];
    cst += tl;
    nxt.assign(in, 0.0f);
    for (int t = 0; t < d; ++t) {
      const float b = row[t];
      if (b == 0.0f) continue;
      const float* w = &c.W[j].a[(size_t)t * in];
      for (int q = 0; q < in; ++q) nxt[q] += b * w[q];
    }
    row.swap(nxt);
  }
  float sc = 0.0f, rr = 0.0f;
  for (int q = 0; q < c.xdims[0]; ++q) { sc += row[q] * c.c0[q]; rr += std::fabs(row[q]) * c.r0[q]; }
  return upper ? sc + rr + cst : sc - rr + cst;
}

// the head row of literal i
inline void head_row(const LitHead& head, int i, std::vector<float>& row, float& cst) {
  row.assign(head.d, 0.0f);
  for (int t = 0; t < head.d; ++t) row[t] = (float)head.H[(size_t)t * head.nlit + i];
  cst = (float)head.H[(size_t)head.d * head.nlit + i];
}

// The projected-gradient loop of literal i on `state` (acdim values, set to the first iterate by the caller): per iterate the upper
// backward pass (entry as in backward_row; it leaves the coefficient that enters neuron n in lam[n]), keep the first smallest smax with
// its uA and ub0 in `out`, the maximiser x* = c + sgn(uA) r, the forward pass of the relaxed network that the backward pass chose
// (lambda > 0: du z + bu, else lower_slope(n) z) with the gradient g[n] = grad(n, lambda, z) and max|g|, the stationary break, and
// state <- project(state - eta g / max|g|), eta <- eta decay.  iterate(s, smax, better) sees every iterate behind its backward pass.
template <class Out, class Entry, class Grad, class Slope, class Project, class Iterate>
inline void pg_literal(const PgContext& c, const LitHead& head, int i, std::vector<float>& state, const std::vector<float>& lam, Out& out,
                       Entry entry, Grad grad, Slope lower_slope, Project project, Iterate iterate) {
  const int n0 = c.xdims[0], acdim = c.acdim();
  std::vector<float> g(acdim), row, nxt, z;
  float best = 0.0f, eta = (float)c.eta0;
  for (int s = 0; s <= c.steps; ++s) {
    float cst;
    head_row(head, i, row, cst);
    const float smax = backward_row(c, c.K - 2, true, row, cst, nxt, entry);
    const bool better = s == 0 || smax < best;
    if (better) {
      best = smax;
      out.smax[i] = smax; out.ub0[i] = cst; out.best_step[i] = s;
      for (int q = 0; q < n0; ++q) out.uA[(size_t)i * n0 + q] = row[q];
    }
    iterate(s, smax, better);
    if (s == c.steps) break;
    z.assign(n0, 0.0f);
    for (int q = 0; q < n0; ++q) z[q] = c.c0[q] + (row[q] > 0.0f ? c.r0[q] : row[q] < 0.0f ? -c.r0[q] : 0.0f);
    float gmax = 0.0f;
    for (int j = 0; j + 1 < c.K; ++j) {
      const int d = c.xdims[j + 1], in = c.xdims[j], o = c.aoff[j];
      nxt.assign(d, 0.0f);
      for (int t = 0; t < d; ++t) {
        float v = 0.0f;
        for (int q = 0; q < in; ++q) v += c.W[j].at(t, q) * z[q];
        v += c.bs[j][t];
        const float lm = lam[o + t];
        g[o + t] = grad(o + t, lm, v);
        gmax = std::max(gmax, std::fabs(g[o + t]));
        nxt[t] = lm > 0.0f ? c.du[o + t] * v + c.bu[o + t] : lower_slope(o + t) * v;
      }
      z.swap(nxt);
    }
    if (!(gmax > 0.0f)) break;          // stationary
    for (int n = 0; n < acdim; ++n) state[n] = project(state[n] - eta * g[n] / gmax);
    eta *= (float)c.decay;
  }
}

// ---- optimised ReLU slopes (alpha-CROWN): per literal, projected-gradient steps on the lower slope alpha in [0, 1] of every unstable
// neuron (l < 0 < u).  Iterate 0 without alpha0 is crown_backward's upper matrix operation for operation.  The hidden layers' bounds
// stay plain CROWN.
struct AlphaOut {
  std::vector<double> smax, uA, ub0, alpha;      // nlit, nlit x n0 (row-major), nlit, nlit x acdim (row-major)
  std::vector<int32_t> best_step;                // nlit
};
// prel / preu: IntervalsOut::prel / preu of the same network and box; alpha0: null or nlit x acdim (row-major)
inline AlphaOut lits_alpha(int K, const int32_t* xdims, const double* M, const LitHead& head, const std::vector<std::vector<float>>& prel,
                           const std::vector<std::vector<float>>& preu, const double* x1min, const double* x1max, int steps, double eta0,
                           double decay, const double* alpha0) {
  const int nlit = head.nlit, n0 = xdims[0];
  PgContext c(K, xdims, M, x1min, x1max, steps, eta0, decay);
  const int acdim = c.acdim();
  std::vector<char> uns(acdim);
  for (int j = 0; j + 1 < K; ++j)
    for (int t = 0; t < xdims[j + 1]; ++t) {
      const int n = c.aoff[j] + t;
      relu_relax_f(prel[j][t], preu[j][t], c.du[n], c.dl[n], c.bu[n]);
      uns[n] = prel[j][t] < 0.0f && preu[j][t] > 0.0f;
    }
  AlphaOut out;
  out.smax.assign(nlit, 0.0); out.uA.assign((size_t)nlit * n0, 0.0); out.ub0.assign(nlit, 0.0);
  out.alpha.assign((size_t)nlit * acdim, 0.0); out.best_step.assign(nlit, 0);
  std::vector<float> al(acdim), lam(acdim);
  for (int i = 0; i < nlit; ++i) {
    for (int n = 0; n < acdim; ++n) {
      al[n] = c.dl[n];
      if (alpha0 && uns[n]) al[n] = (float)std::min(std::max(alpha0[(size_t)i * acdim + n], 0.0), 1.0);
    }
    pg_literal(c, head, i, al, lam, out,
               [&](int n, float b, float& su) {
                 lam[n] = b;
                 su += std::max(b, 0.0f) * c.bu[n] + std::min(b, 0.0f) * 0.0f;
                 return std::max(b, 0.0f) * c.du[n] + std::min(b, 0.0f) * al[n];
               },
               [&](int n, float lm, float v) { return uns[n] ? std::min(lm, 0.0f) * v : 0.0f; },
               [&](int n) { return al[n]; },
               [](float x) { return std::min(std::max(x, 0.0f), 1.0f); },
               [&](int, float, bool better) {
                 if (better) for (int n = 0; n < acdim; ++n) out.alpha[(size_t)i * acdim + n] = al[n];
               });
  }
  return out;
}

// ---- bounds on a node of a ReLU split ("Branching on unstable ReLUs"; the kernels are in crown_relu_split.hpp): the
// box and an assignment s in {-1, 0, +1}^acdim (+1: z_n >= 0, -1: z_n <= 0, 0: free).  A forced neuron's relaxation is exact, the
// pre-activation bounds are clipped to the forced side (l > u afterwards: the node is infeasible), and per literal `steps`
// projected-gradient steps on one multiplier beta_n >= 0 per forced neuron tighten the upper bound.
struct NodeOut {
  std::vector<double> pre_lo, pre_hi;            // acdim, clipped
  std::vector<double> smin, smax_plain, smax, uA, ub0;      // nlit; uA nlit x n0 (row-major); smax / uA / ub0 of the best iterate
  std::vector<int32_t> best_step, branch;        // nlit
  int infeasible = 0;
};
inline NodeOut make_intervals_nodes(int K, const int32_t* xdims, const double* M, const LitHead& head, const double* x1min,
                                    const double* x1max, const int8_t* assign, int steps, double eta0, double decay) {
  const int nlit = head.nlit, n0 = xdims[0];
  PgContext c(K, xdims, M, x1min, x1max, steps, eta0, decay);
  const int acdim = c.acdim();
  std::vector<float> pl(acdim), pu(acdim);
  std::vector<char> cand(acdim);
  NodeOut out;
  // backward_row's entry.  upper: the upper bound's pair (else the lower bound's).  beta (upper only): the multipliers, added behind the
  // row scaling.  lam receives the coefficients that enter every neuron.
  auto entry = [&](bool upper, const float* beta, float* lam, int n, float b, float& sb) {
    const float bp = std::max(b, 0.0f), bn = std::min(b, 0.0f);
    if (lam) lam[n] = b;
    sb += (upper ? bp : bn) * c.bu[n];
    float y = upper ? bp * c.du[n] + bn * c.dl[n] : bp * c.dl[n] + bn * c.du[n];
    if (beta && assign[n] != 0) y += (float)assign[n] * beta[n];
    return y;
  };
  auto plain = [&](bool upper) { return [&entry, upper](int n, float b, float& sb) { return entry(upper, nullptr, nullptr, n, b, sb); }; };
  // the pre-activation bounds, layer by layer, clipped; then the layer's relaxation
  std::vector<float> row, nxt;
  for (int k = 0; k + 1 < K; ++k) {
    const int d = xdims[k + 1], in = xdims[k], o = c.aoff[k];
    for (int t = 0; t < d; ++t) {
      float l = 0.0f, u = 0.0f;
      for (int side = 0; side < 2; ++side) {
        row.assign(c.W[k].a.begin() + (size_t)t * in, c.W[k].a.begin() + (size_t)(t + 1) * in);
        float cst = c.bs[k][t];
        (side ? u : l) = backward_row(c, k - 1, side == 1, row, cst, nxt, plain(side == 1));
      }
      const int sv = assign[o + t];
      if (sv > 0) l = std::max(l, 0.0f);
      if (sv < 0) u = std::min(u, 0.0f);
      if (l > u) out.infeasible = 1;
      pl[o + t] = l; pu[o + t] = u;
    }
    for (int t = 0; t < d; ++t) {
      const int n = o + t, sv = assign[n];
      relu_relax_f(pl[n], pu[n], c.du[n], c.dl[n], c.bu[n]);
      if (sv != 0) { c.du[n] = c.dl[n] = sv > 0 ? 1.0f : 0.0f; c.bu[n] = 0.0f; }
      cand[n] = sv == 0 && pl[n] < 0.0f && pu[n] > 0.0f;
    }
  }
  out.pre_lo.assign(pl.begin(), pl.end()); out.pre_hi.assign(pu.begin(), pu.end());
  out.smin.assign(nlit, 0.0); out.smax_plain.assign(nlit, 0.0); out.smax.assign(nlit, 0.0); out.ub0.assign(nlit, 0.0);
  out.uA.assign((size_t)nlit * n0, 0.0); out.best_step.assign(nlit, 0); out.branch.assign(nlit, -1);
  std::vector<float> beta(acdim), lam(acdim);
  for (int i = 0; i < nlit; ++i) {
    float cst;
    head_row(head, i, row, cst);
    out.smin[i] = backward_row(c, K - 2, false, row, cst, nxt, plain(false));
    std::fill(beta.begin(), beta.end(), 0.0f);
    pg_literal(c, head, i, beta, lam, out,
               [&](int n, float b, float& sb) { return entry(true, beta.data(), lam.data(), n, b, sb); },
               [&](int n, float, float v) { return assign[n] != 0 ? (float)assign[n] * v : 0.0f; },
               [&](int n) { return c.dl[n]; },
               [](float x) { return std::max(x, 0.0f); },
               [&](int s, float smax, bool) {
                 if (s != 0) return;
                 // the plain pass: its bound, and the branching neuron - the candidate with the largest max(lambda, 0) bu, the first of equals
                 out.smax_plain[i] = smax;
                 float bscore = -1.0f;
                 for (int n = 0; n < acdim; ++n) {
                   const float sc = std::max(lam[n], 0.0f) * c.bu[n];
                   if (cand[n] && sc > bscore) { bscore = sc; out.branch[i] = n; }
                 }
               });
  }
  return out;
}

}  // namespace nnsdp
