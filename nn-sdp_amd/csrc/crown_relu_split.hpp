// Bounds on the nodes of a ReLU split (nnsdp_crown_bound_nodes; DESIGN.md section 5, "Branching on unstable ReLUs").  A node is an input
// box and an assignment s in {-1, 0, +1}^acdim of the hidden neurons: +1 forces the pre-activation z_n >= 0, -1 forces z_n <= 0, 0 leaves
// the neuron free.  Every number is a valid bound over {x in box : s_n z_n(x) >= 0 for every forced n}.  Two kernels on the handle's
// stream, one workgroup of 256 threads per node each:
//   k_crown_nodes: the pre-activation passes and the literal pass of crown_batch.hpp with SPLIT (exact relaxation of the forced neurons,
//     clipped bounds in the scratch, the infeasibility flag, the branching neuron of every literal).  It runs no identity-head pass, no
//     output pass and no interval step: the literal pass reads the scratch alone.
//   k_crown_beta: per literal i, independently of the others, projected-gradient steps on one multiplier beta_{i,n} >= 0 per forced
//     neuron.  The constraint enters the upper bound's backward pass as  A[i][n] += s_n beta_{i,n}  after the row scaling of the neuron's
//     layer; iterate 0 (beta = 0) adds nothing and has the bits of the plain literal pass.  The gradient is g_n = s_n z_n(x*), z the
//     pre-activations of the relaxed network that the backward pass chose at x* = c + sgn(uA) r;  beta <- max(beta - eta g / max|g|, 0),
//     eta <- eta decay.  The result is the first iterate with the smallest smax, with its uA and ub0.
// Both follow k_crown_alpha (crown_alpha.hpp): the upper matrix A in the cb_idx layout, a second 64 x 64 region B (a layer's beta, then
// its lambda; the forward values), A <- A W_j and Z = B W_j' on v_mfma_f64_16x16x4_f64, the per-(literal, neuron) state [neuron][literal]
// per node in buffers of the handle.  No atomics; every sum is per row with t ascending, max|g| is taken in a fixed order.  A node's
// bits depend neither on the number of nodes, nor on its position, nor on the other literals, nor on earlier calls.
#pragma once
#include "crown_batch.hpp"

namespace nnsdp {

struct CrownNodeArgs {
  CrownArgs c;              // the network, the head, the boxes; scratch: the clipped pre-activation bounds, 2 acdim per node (an output)
  CrownSplit sp;            // the assignments; where the branching neurons go
  double* infeasible;       // nnode, 0.0 / 1.0
  int steps;                // 0..64
  double eta0, decay;
  double *cur, *lam;        // state, acdim x nlit doubles per node each, [neuron][literal]: beta^s; lambda, then g
  double *b_smax, *b_ub0;   // nlit x nnode, the best iterate
  double* b_step;           // nlit x nnode, its index as a double
  double* b_uA;             // xdims[0] x nlit x nnode
};

static constexpr size_t kCnLdsBytes = (2 * kCbW * kCbW + 10 * kCbW) * sizeof(double);

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
    p.c.acdim = (int)acdim; p.c.nlit = (int)nlit;
    p.c.scratch = base;
    p.c.smin = base + npre(); p.c.smax = p.c.smin + nl();
    p.b_smax = p.c.smax + nl(); p.b_ub0 = p.b_smax + nl(); p.b_step = p.b_ub0 + nl(); p.sp.branch = p.b_step + nl();
    p.b_uA = p.sp.branch + nl(); p.infeasible = p.b_uA + nA();
    // the plain pass's linear form and everything that only the box entries produce stay unwritten
    p.c.uA = p.c.ub0 = p.c.acymin = p.c.acymax = p.c.acxmin = p.c.acxmax = p.c.ymin = p.c.ymax = nullptr;
  }
};

// the relaxation of crown_pass<.., SPLIT = true> from the (clipped) pre-activation bounds and the neuron's assignment
__device__ __forceinline__ void cn_relax(double l, double u, int sv, double& du, double& dl, double& bu) {
  const double lrx = l < 0.0 ? l : 0.0;
  double ur = u > 0.0 ? u : 0.0;
  ur = ur > lrx + 1e-8 ? ur : lrx + 1e-8;
  du = ur / (ur - lrx);
  dl = du > 0.5 ? 1.0 : 0.0;
  bu = -lrx * du;
  if (sv != 0) {
    du = dl = sv > 0 ? 1.0 : 0.0;
    bu = 0.0;
  }
}

__global__ __launch_bounds__(256) void k_crown_nodes(CrownNodeArgs p) {
  extern __shared__ double cn_lds[];
  const long long node = blockIdx.x;
  CrownSplit sp = p.sp;
  sp.infeasible = 0;
  for (int k = 1; k < p.c.K; ++k) crown_pass<false, kCbRelu, true>(p.c, cn_lds, node, k, 0, &sp);
  crown_pass<true, kCbRelu, true>(p.c, cn_lds, node, p.c.K, 0, &sp);
  if (threadIdx.x == 0) p.infeasible[node] = sp.infeasible ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_crown_beta(CrownNodeArgs p) {
  extern __shared__ double cn_lds[];
  const CrownArgs& a = p.c;
  double* A = cn_lds;                       // the upper matrix; |g| during the forward pass
  double* B = cn_lds + kCbW * kCbW;         // a layer's beta, then its lambda (backward); the forward values (gradient)
  double* v_du = B + kCbW * kCbW;
  double* v_dl = v_du + kCbW;
  double* v_bu = v_dl + kCbW;
  double* v_bj = v_bu + kCbW;
  double* v_s = v_bj + kCbW;                // the layer's assignment as doubles
  double* v_c = v_s + kCbW;
  double* v_r = v_c + kCbW;
  double* v_gmax = v_r + kCbW;
  double* v_flag = v_gmax + kCbW;           // 1.0: the literal's iterate is its best so far
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lc = lane >> 4;
  const long long node = blockIdx.x;
  const int K = a.K, nlit = a.nlit, acdim = a.acdim, n0 = a.xdims[0], nst = nlit * acdim;
  const size_t sbase = (size_t)node * nst;
  double *cur = p.cur + sbase, *lam = p.lam + sbase;
  const double* pre = a.scratch + (size_t)node * 2 * acdim;
  const int8_t* asg = p.sp.assign + (size_t)node * acdim;
  const int nit = (nlit + 15) >> 4;

  for (int idx = tid; idx < nst; idx += 256) cur[idx] = 0.0;      // beta^0
  if (tid < n0) {
    const double l = a.lo[(size_t)node * n0 + tid], u = a.hi[(size_t)node * n0 + tid];
    v_c[tid] = (u + l) / 2.0;
    v_r[tid] = (u - l) / 2.0;
  }
  __threadfence_block();
  __syncthreads();

  double best_smax = 0.0, eta = p.eta0;
  for (int s = 0; s <= p.steps; ++s) {
    // ---- backward pass at beta^s: the upper matrix of crown_pass<true, kCbRelu, true>, plus s beta behind the row scaling
    int d = a.xdims[K - 1];
    double bias = 0.0;
    for (int idx = tid; idx < nlit * d; idx += 256) {
      const int t = idx / nlit, i = idx - t * nlit;
      A[cb_idx(t, i)] = a.H[(size_t)t * nlit + i];
    }
    if (tid < nlit) bias = a.H[(size_t)d * nlit + tid];
    __syncthreads();
    for (int j = K - 2; j >= 0; --j) {
      const int in = a.xdims[j], o = a.acoff[j];
      const double* Mj = a.M + a.moff[j];       // d x (in + 1), column-major
      if (tid < d) {
        const int sv = asg[o + tid];
        double du, dl, bu;
        cn_relax(pre[o + tid], pre[acdim + o + tid], sv, du, dl, bu);
        v_du[tid] = du;
        v_dl[tid] = dl;
        v_bu[tid] = bu;
        v_bj[tid] = Mj[(size_t)in * d + tid];
        v_s[tid] = (double)sv;
      }
      for (int idx = tid; idx < nlit * d; idx += 256) {
        const int t = idx / nlit, i = idx - t * nlit;
        B[cb_idx(t, i)] = cur[(size_t)o * nlit + idx];
      }
      __syncthreads();
      if (tid < nlit) {
        double sb = 0.0, tl = 0.0;
        for (int t = 0; t < d; ++t) {
          const double x = A[cb_idx(t, tid)];
          const double xp = x > 0.0 ? x : 0.0, xn = x < 0.0 ? x : 0.0;
          const double du = v_du[t], dl = v_dl[t], sv = v_s[t];
          sb += xp * v_bu[t];
          double y = xp * du + xn * dl;
          if (sv != 0.0) y += sv * B[cb_idx(t, tid)];      // a free neuron keeps the plain pass's bits
          A[cb_idx(t, tid)] = y;
          B[cb_idx(t, tid)] = x;
          tl += y * v_bj[t];
        }
        bias += sb;
        bias += tl;
      }
      __syncthreads();
      for (int idx = tid; idx < nlit * d; idx += 256) {
        const int t = idx / nlit, i = idx - t * nlit;
        lam[(size_t)o * nlit + idx] = B[cb_idx(t, i)];
      }
      // A (nlit x d) <- A W_j (nlit x in): a = A[16 it + lr][4 ks + lc] from LDS, b = W_j[4 ks + lc][16 w + lr] from global
      const int nqt = (in + 15) >> 4, ks = (d + 3) >> 2;
      d4_t c[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) c[it] = d4_t{0.0, 0.0, 0.0, 0.0};
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
                  const double au = (t < d && i < nlit) ? A[cb_idx(tc, i)] : 0.0;
                  c[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv[u], c[it], 0, 0, 0);
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
              if (i < nlit) A[cb_idx(q, i)] = c[it][r];
            }
          }
        }
      }
      d = in;
      __syncthreads();
    }
    // ---- concretise (d == n0), keep the first smallest
    if (tid < nlit) {
      double sc = 0.0, rr = 0.0;
      for (int t = 0; t < d; ++t) {
        const double x = A[cb_idx(t, tid)];
        sc += x * v_c[t];
        rr += fabs(x) * v_r[t];
      }
      const double smax = sc + rr + bias;
      const bool better = s == 0 || smax < best_smax;
      v_flag[tid] = better ? 1.0 : 0.0;
      if (better) {
        best_smax = smax;
        p.b_smax[(size_t)node * nlit + tid] = smax;
        p.b_ub0[(size_t)node * nlit + tid] = bias;
        p.b_step[(size_t)node * nlit + tid] = (double)s;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nlit * n0; idx += 256) {
      const int i = idx / n0, t = idx - i * n0;
      if (v_flag[i] != 0.0) p.b_uA[((size_t)node * nlit + i) * n0 + t] = A[cb_idx(t, i)];
    }
    if (s == p.steps) break;

    // ---- gradient: the relaxed network that the pass chose, at x* = c + sgn(uA) r
    for (int idx = tid; idx < nlit * n0; idx += 256) {
      const int t = idx / nlit, i = idx - t * nlit;
      const double ua = A[cb_idx(t, i)], r = v_r[t];
      B[cb_idx(t, i)] = v_c[t] + (ua > 0.0 ? r : ua < 0.0 ? -r : 0.0);
    }
    double gmax = 0.0;
    int din = n0;
    __syncthreads();
    for (int j = 0; j + 1 < K; ++j) {
      const int dj = a.xdims[j + 1], o = a.acoff[j];
      const double* Mj = a.M + a.moff[j];       // dj x (din + 1), column-major
      if (tid < dj) {
        const int sv = asg[o + tid];
        double du, dl, bu;
        cn_relax(pre[o + tid], pre[acdim + o + tid], sv, du, dl, bu);
        v_du[tid] = du;
        v_dl[tid] = dl;
        v_bu[tid] = bu;
        v_bj[tid] = Mj[(size_t)din * dj + tid];
        v_s[tid] = (double)sv;
      }
      // Z (nlit x dj) = B (nlit x din) W_j': a = B[16 it + lr][4 ks + lc] from LDS, b = W_j[16 w + lr][4 ks + lc] from global
      const int nqt = (dj + 15) >> 4, ks = (din + 3) >> 2;
      d4_t c[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) c[it] = d4_t{0.0, 0.0, 0.0, 0.0};
      const int q = 16 * w + lr;
      if (w < nqt) {
        for (int k0 = 0; k0 < ks; k0 += kCbChunk) {
          double bv[kCbChunk];
#pragma unroll
          for (int u = 0; u < kCbChunk; ++u) {
            const int t = 4 * (k0 + u) + lc;
            bv[u] = (q < dj && t < din) ? Mj[(size_t)t * dj + q] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < kCbChunk; ++u) {
            if (k0 + u < ks) {
              const int t = 4 * (k0 + u) + lc;
              const int tc = t < din ? t : 0;
#pragma unroll
              for (int it = 0; it < 4; ++it) {
                if (it < nit) {
                  const int i = 16 * it + lr;
                  const double av = (t < din && i < nlit) ? B[cb_idx(tc, i)] : 0.0;
                  c[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], c[it], 0, 0, 0);
                }
              }
            }
          }
        }
      }
      __syncthreads();
      if (w < nqt && q < dj) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          if (it < nit) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = 16 * it + lc + 4 * r;
              if (i < nlit) B[cb_idx(q, i)] = c[it][r];
            }
          }
        }
      }
      __syncthreads();
      for (int idx = tid; idx < nlit * dj; idx += 256) {
        const int t = idx / nlit, i = idx - t * nlit;
        const size_t sidx = (size_t)o * nlit + idx;
        const double z = B[cb_idx(t, i)] + v_bj[t];
        const double lm = lam[sidx], sv = v_s[t];
        const double g = sv != 0.0 ? sv * z : 0.0;
        lam[sidx] = g;
        A[cb_idx(t, i)] = fabs(g);
        B[cb_idx(t, i)] = lm > 0.0 ? v_du[t] * z + v_bu[t] : v_dl[t] * z;
      }
      __syncthreads();
      if (tid < nlit)
        for (int t = 0; t < dj; ++t) {
          const double ag = A[cb_idx(t, tid)];
          gmax = ag > gmax ? ag : gmax;
        }
      din = dj;
    }
    // ---- step; a literal whose gradient vanishes (no forced neuron among them) is stationary and stays where it is
    if (tid < nlit) v_gmax[tid] = gmax;
    if (__syncthreads_and(tid >= nlit || !(gmax > 0.0))) break;
    for (int idx = tid; idx < nst; idx += 256) {
      const int n = idx / nlit, i = idx - n * nlit;
      const double gm = v_gmax[i];
      if (gm > 0.0) {
        const double v = cur[idx] - eta * lam[idx] / gm;
        cur[idx] = v < 0.0 ? 0.0 : v;
      }
    }
    eta *= p.decay;
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace nnsdp
