// Optimised ReLU slopes for the literal pass of the resident CROWN bounder (alpha-CROWN, nnsdp_crown_bound_alpha).
// k_crown_alpha runs on the handle's stream after k_crown_resident<kCbRelu> and reads the raw pre-activation bounds that kernel left in
// the scratch.  It is the projected-gradient loop of crown_opt.hpp (the passes, the LDS, the state buffers and what the bits depend on
// are described there) on the lower slope alpha in [0, 1] of every unstable neuron (l < 0 < u):
//   the state starts at the plain rule dl, or at alpha0 clipped on the unstable neurons; the row scaling takes it as the lower slope
//   (lambda > 0: du and bu; else alpha and no bias), so iterate 0 without alpha0 has the bits of the plain literal pass;
//   g = min(lambda, 0) z on the unstable neurons;  alpha <- clip(alpha - eta0 decay^s g / max|g|, 0, 1);
//   the best iterate's alpha is kept in a third state buffer and written out at the end, neuron index fastest.
#pragma once
#include "crown_opt.hpp"

namespace nnsdp {

struct CrownAlphaArgs {
  CrownOptArgs o;           // c: the arguments of the plain launch before this one
  const double* alpha0;     // null, or acdim x nlit x nbox (neuron index fastest)
  double* best;             // state like o.cur: the best alpha
  double* alpha;            // acdim x nlit x nbox (neuron index fastest)
};

struct CbSlopes {
  static constexpr bool kKeepsBest = true, kScaleUsesLayer = false;
  const double* alpha0;     // of the box: acdim x nlit (neuron index fastest), or null
  double* best;             // of the box
  __device__ double start(const double* pre, int acdim, int n, int i) const {
    double du, dl, bu;
    const bool uns = cb_relu_relax(pre[n], pre[acdim + n], 0, du, dl, bu);
    if (!(alpha0 && uns)) return dl;
    const double x = alpha0[(size_t)i * acdim + n];
    return x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
  }
  __device__ double relax(const double* pre, int acdim, int n, double& du, double& dl, double& bu) const {
    return cb_relu_relax(pre[n], pre[acdim + n], 0, du, dl, bu) ? 1.0 : 0.0;
  }
  __device__ double scale(double xp, double xn, double du, double, double, const double* alpha) const { return xp * du + xn * *alpha; }
  __device__ double grad(double m, double lm, double z) const { return m != 0.0 ? (lm < 0.0 ? lm : 0.0) * z : 0.0; }
  __device__ double lower_slope(double, const double* alpha) const { return *alpha; }
  __device__ double project(double v) const { return v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v; }
  __device__ void keep(int idx, double alpha) const { best[idx] = alpha; }
};

__global__ __launch_bounds__(256) void k_crown_alpha(CrownAlphaArgs p) {
  const long long box = blockIdx.x;
  const int nlit = p.o.c.nlit, acdim = p.o.c.acdim, nst = nlit * acdim;
  const size_t sbase = (size_t)box * nst;
  double* best = p.best + sbase;
  crown_pg_body(p.o, CbSlopes{p.alpha0 ? p.alpha0 + sbase : nullptr, best});
  // the best alpha, neuron index fastest
  __threadfence_block();
  __syncthreads();
  for (int idx = threadIdx.x; idx < nst; idx += 256) {
    const int i = idx / acdim, n = idx - i * acdim;
    p.alpha[sbase + idx] = best[(size_t)n * nlit + i];
  }
}

}  // namespace nnsdp
