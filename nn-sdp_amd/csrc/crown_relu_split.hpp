// Bounds on the nodes of a ReLU split (nnsdp_crown_bound_nodes; DESIGN.md section 5, "Branching on unstable ReLUs").  A node is an input
// box and an assignment s in {-1, 0, +1}^acdim of the hidden neurons: +1 forces the pre-activation z_n >= 0, -1 forces z_n <= 0, 0 leaves
// the neuron free.  Every number is a valid bound over {x in box : s_n z_n(x) >= 0 for every forced n}.  Two kernels on the handle's
// stream, one workgroup of 256 threads per node each:
//   k_crown_nodes: the pre-activation passes and the literal pass of crown_batch.hpp with SPLIT (exact relaxation of the forced neurons,
//     clipped bounds in the scratch, the infeasibility flag, the branching neuron of every literal).  It runs no identity-head pass, no
//     output pass and no interval step: the literal pass reads the scratch alone.
//   k_crown_beta: the projected-gradient loop of crown_opt.hpp (the passes, the LDS, the state buffers and what the bits depend on are
//     described there) on one multiplier beta_{i,n} >= 0 per literal and forced neuron.  The state starts at zero; the constraint enters
//     the upper bound's backward pass as  A[i][n] += s_n beta_{i,n}  after the row scaling of the neuron's layer, so iterate 0 adds
//     nothing and has the bits of the plain literal pass;  g_n = s_n z_n(x*);  beta <- max(beta - eta g / max|g|, 0), eta <- eta decay.
//     No best state is kept: the result is the best iterate's smax with its uA and ub0.
#pragma once
#include "crown_opt.hpp"

namespace nnsdp {

struct CrownNodeArgs {
  CrownOptArgs o;           // c: the network, the head, the boxes; scratch: the clipped pre-activation bounds, 2 acdim per node (an output)
  CrownSplit sp;            // the assignments; where the branching neurons go
  double* infeasible;       // nnode, 0.0 / 1.0
};

// The outputs of nnode nodes, packed so that one copy brings everything back:
//   pre (per node: acdim lower, then acdim upper) | smin | smax_plain | smax | ub0 | step | branch | uA | infeasible
struct CrownNodeLayout {
  size_t nnode, n0, acdim, nlit;
  size_t npre() const { return 2 * nnode * acdim; }
  size_t nl() const { return nnode * nlit; }
  size_t nA() const { return nl() * n0; }
  size_t nst() const { return nl() * acdim; }
  size_t total() const { return npre() + 6 * nl() + nA() + nnode; }
  // the boxes (lo, then hi) as doubles, then one byte per (node, neuron), rounded up to whole doubles
  size_t in_doubles() const { return 2 * nnode * n0 + (nnode * acdim + 7) / 8; }
  void point(CrownNodeArgs& p, double* base) const {
    p.o.c.acdim = (int)acdim; p.o.c.nlit = (int)nlit;
    p.o.c.scratch = base;
    p.o.c.smin = base + npre(); p.o.c.smax = p.o.c.smin + nl();
    p.o.smax = p.o.c.smax + nl(); p.o.ub0 = p.o.smax + nl(); p.o.step = p.o.ub0 + nl(); p.sp.branch = p.o.step + nl();
    p.o.uA = p.sp.branch + nl(); p.infeasible = p.o.uA + nA();
    // the plain pass's linear form and everything that only the box entries produce stay unwritten
    p.o.c.uA = p.o.c.ub0 = p.o.c.acymin = p.o.c.acymax = p.o.c.acxmin = p.o.c.acxmax = p.o.c.ymin = p.o.c.ymax = nullptr;
  }
};

__global__ __launch_bounds__(256) void k_crown_nodes(CrownNodeArgs p) {
  extern __shared__ double cn_lds[];
  const long long node = blockIdx.x;
  CrownSplit sp = p.sp;
  sp.infeasible = 0;
  for (int k = 1; k < p.o.c.K; ++k) crown_pass<false, kCbRelu, true>(p.o.c, cn_lds, node, k, 0, &sp);
  crown_pass<true, kCbRelu, true>(p.o.c, cn_lds, node, p.o.c.K, 0, &sp);
  if (threadIdx.x == 0) p.infeasible[node] = sp.infeasible ? 1.0 : 0.0;
}

struct CbMultipliers {
  static constexpr bool kKeepsBest = false, kScaleUsesLayer = true;
  const int8_t* assign;     // of the node
  __device__ double start(const double*, int, int, int) const { return 0.0; }
  __device__ double relax(const double* pre, int acdim, int n, double& du, double& dl, double& bu) const {
    const int sv = assign[n];
    cb_relu_relax(pre[n], pre[acdim + n], sv, du, dl, bu);
    return (double)sv;
  }
  __device__ double scale(double xp, double xn, double du, double dl, double sv, const double* beta) const {
    double y = xp * du + xn * dl;
    if (sv != 0.0) y += sv * *beta;     // a free neuron keeps the plain pass's bits
    return y;
  }
  __device__ double grad(double sv, double, double z) const { return sv != 0.0 ? sv * z : 0.0; }
  __device__ double lower_slope(double dl, const double*) const { return dl; }
  __device__ double project(double v) const { return v < 0.0 ? 0.0 : v; }
};

__global__ __launch_bounds__(256) void k_crown_beta(CrownNodeArgs p) {
  crown_pg_body(p.o, CbMultipliers{p.sp.assign + (size_t)blockIdx.x * p.o.c.acdim});
}

}  // namespace nnsdp
