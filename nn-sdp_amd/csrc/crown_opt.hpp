// The projected-gradient loop that the two optimisers of the literal bounds share: k_crown_alpha (crown_alpha.hpp,
// the lower slopes of the unstable ReLUs) and k_crown_beta (crown_relu_split.hpp, the multipliers of a node's forced neurons).  Per box
// (or node) and per literal i, independently of the other literals: T steps on one state value per hidden neuron of the UPPER bound's
// backward pass; the result is the first iterate with the smallest smax, with its uA and ub0.
//
// One workgroup of 256 threads per box.  LDS: the upper matrix A (64 x 64, the cb_idx layout of crown_batch.hpp) and a second 64 x 64
// region B in the place of crown_pass's lower matrix, plus ten 64-double vectors: 70 656 B (kCoLdsBytes).  The LDS would let two
// workgroups share a CU; the registers do not (274 of 512 per SIMD, profiles/crown_alpha_resources.txt): one workgroup per CU.
//   backward pass at state^s: crown_pass<true>'s upper matrix, operation for operation - per layer the state of the layer comes from
//     the state buffer into B, thread (row i) scales its row (the variant says what the state does there) and leaves lambda in B, which
//     goes back to the state buffer; then A <- A W_j on v_mfma_f64_16x16x4_f64 exactly as there.  An iterate whose state changes
//     nothing (the plain slopes, multipliers of zero) therefore has the bits of the plain literal pass.
//   gradient: x* = c + sgn(uA) r per literal goes to B, and per layer Z (nlit x d_j) = B (nlit x in) W_j' on the same instruction (a from
//     B in LDS, b = W_j[q][t] from global memory); the element pass turns Z into the variant's g and into the next layer's input
//     D z + beta  with the pair the backward pass chose; |g| goes through A for the per-literal maximum.
//   step: state <- project(state - eta0 decay^s g / max|g|); a literal whose gradient vanishes is stationary and stays where it is,
//     and the loop ends when every literal is.
// A variant (CbSlopes, CbMultipliers) supplies the six places where the two differ: how the state starts, what the row scaling does
// with it, the gradient, the lower slope of the forward pass, the projection, and whether the best state is kept.
// The per-(literal, neuron) state - the iterate, lambda / g, a variant's best iterate - lives in device buffers of the handle, stored
// [neuron][literal] per box so that a layer's slice moves between global memory and LDS with consecutive lanes on consecutive addresses
// of both.  No atomics; max|g| is a maximum of absolute values (exact in any order) taken in a fixed order anyway, every other sum is
// per row, t ascending.  A literal's bits depend neither on nbox, nor on the box's position, nor on the other literals, nor on earlier
// calls.
#pragma once
#include <type_traits>

#include "crown_batch.hpp"

namespace nnsdp {

// what both argument blocks (CrownAlphaArgs, CrownNodeArgs) start with
struct CrownOptArgs {
  CrownArgs c;              // the network, the head, the boxes and the scratch with the pre-activation bounds, 2 acdim per box
  double *cur, *lam;        // state, acdim x nlit doubles per box each, [neuron][literal]: the iterate; lambda, then g
  double *smax, *ub0;       // nlit x nbox, the best iterate
  double* step;             // nlit x nbox, its index as a double (one download brings everything back)
  double* uA;               // xdims[0] x nlit x nbox
  int steps;                // T in 0..64
  double eta0, decay;
  // (the order of the members decides how the kernels load them, and through the scalar registers that takes, their vector registers.
  // After any edit here compile with  hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S api.hip  and hold .vgpr_count /
  // .agpr_count of k_crown_alpha and k_crown_beta against profiles/crown_opt_resources.txt: 274 / 18 and 272 / 16)
};

static constexpr size_t kCoLdsBytes = (2 * kCbW * kCbW + 10 * kCbW) * sizeof(double);

// du, dl, bu of the ReLU relaxation from raw pre-activation bounds, the arithmetic of crown_pass (SPLIT: a forced neuron, sv != 0, has
// the exact pair); returns l < 0 < u
__device__ __forceinline__ bool cb_relu_relax(double l, double u, int sv, double& du, double& dl, double& bu) {
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
  return l < 0.0 && u > 0.0;
}

// out (nlit x nq) <- mat (nlit x nk) W on v_mfma_f64_16x16x4_f64, W[t][q] = Mj[q nk + t] (backward, A <- A W_j) or, TRANSPOSED,
// Mj[t nq + q] (forward, Z = B W_j'): a = mat[16 it + lr][4 ks + lc] from LDS, b = W[4 ks + lc][16 w + lr] from global memory in chunks
// of kCbChunk k-steps.  Wave w owns the output columns 16 w .. 16 w + 15; the tiles stay in registers across a barrier, so out may be
// mat.  Ends behind a barrier.
template <bool TRANSPOSED>
__device__ __forceinline__ void cb_lit_product(const double* mat, const double* Mj, int nlit, int nk, int nq, double* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lc = lane >> 4;
  const int nit = (nlit + 15) >> 4, nqt = (nq + 15) >> 4, ks = (nk + 3) >> 2;
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
        bv[u] = (q < nq && t < nk) ? Mj[TRANSPOSED ? (size_t)t * nq + q : (size_t)q * nk + t] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kCbChunk; ++u) {
        if (k0 + u < ks) {
          const int t = 4 * (k0 + u) + lc;
          const int tc = t < nk ? t : 0;      // a column past nk multiplies a zero of bv: read a written one, never stale bits
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            if (it < nit) {
              const int i = 16 * it + lr;
              const double av = (t < nk && i < nlit) ? mat[cb_idx(tc, i)] : 0.0;
              c[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], c[it], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (w < nqt && q < nq) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (it < nit) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * it + lc + 4 * r;
          if (i < nlit) out[cb_idx(q, i)] = c[it][r];
        }
      }
    }
  }
  __syncthreads();
}

// The loop for the box blockIdx.x.  A variant V has (n a hidden neuron, i a literal; `state` is a pointer, so that the value is loaded only
// where a variant's own test lets it be - a reference would let the compiler load it for every neuron):
//   double start(pre, acdim, n, i)            the state's first iterate
//   double relax(pre, acdim, n, du, dl, bu)   the neuron's relaxation; returns its mark m (0.0: the neuron has no state)
//   double scale(xp, xn, du, dl, m, state)    a row entry behind the row scaling, from its positive and negative part
//   double grad(m, lambda, z)                 d smax / d state
//   double lower_slope(dl, state)             the lower slope that scale() used
//   double project(v)
//   kScaleUsesLayer                           scale() and lower_slope() read dl and m (else they get 0.0 and the body stages neither
//                                             for the backward pass)
//   void keep(idx, state)                     (kKeepsBest) idx = n nlit + i: the iterate of literal i is its best so far
template <class V>
__device__ __forceinline__ void crown_pg_body(const CrownOptArgs& p, const V& v) {
  // kCoLdsBytes; named here: handed in as an argument it costs k_crown_alpha two registers (the check: see CrownOptArgs)
  extern __shared__ double co_lds[];
  double* lds = co_lds;
  const CrownArgs& a = p.c;
  double* A = lds;                          // the upper matrix; |g| during the forward pass
  double* B = lds + kCbW * kCbW;            // a layer's state, then its lambda (backward); the forward values (gradient)
  double* v_du = B + kCbW * kCbW;
  double* v_dl = v_du + kCbW;
  double* v_bu = v_dl + kCbW;
  double* v_bj = v_bu + kCbW;
  double* v_m = v_bj + kCbW;                // the variant's mark of the layer's neurons
  double* v_c = v_m + kCbW;
  double* v_r = v_c + kCbW;
  double* v_gmax = v_r + kCbW;
  double* v_flag = v_gmax + kCbW;           // 1.0: the literal's iterate is its best so far
  const int tid = threadIdx.x;
  const long long box = blockIdx.x;
  const int K = a.K, nlit = a.nlit, acdim = a.acdim, n0 = a.xdims[0], nst = nlit * acdim;
  const size_t sbase = (size_t)box * nst;
  double *cur = p.cur + sbase, *lam = p.lam + sbase;
  const double* pre = a.scratch + (size_t)box * 2 * acdim;
  // a layer of d neurons from offset o with the bias column bj: its relaxation and bias; dl and the mark only where they are read - by
  // scale() if the variant says so (kScaleUsesLayer), the mark by grad() in the forward pass
  auto layer = [&](const double* bj, int d, int o, auto forward) {
    if (tid < d) {
      double du, dl, bu;
      const double m = v.relax(pre, acdim, o + tid, du, dl, bu);
      v_du[tid] = du;
      v_bu[tid] = bu;
      v_bj[tid] = bj[tid];
      if constexpr (V::kScaleUsesLayer) v_dl[tid] = dl;
      if constexpr (V::kScaleUsesLayer || decltype(forward)::value) v_m[tid] = m;
    }
  };

  for (int idx = tid; idx < nst; idx += 256) {
    const int n = idx / nlit, i = idx - n * nlit;
    cur[idx] = v.start(pre, acdim, n, i);
  }
  if (tid < n0) {
    const double l = a.lo[(size_t)box * n0 + tid], u = a.hi[(size_t)box * n0 + tid];
    v_c[tid] = (u + l) / 2.0;
    v_r[tid] = (u - l) / 2.0;
  }
  __threadfence_block();
  __syncthreads();

  double best_smax = 0.0, eta = p.eta0;
  for (int s = 0; s <= p.steps; ++s) {
    // ---- backward pass at state^s: the upper matrix of crown_pass<true>
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
      layer(Mj + (size_t)in * d, d, o, std::false_type{});
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
          sb += xp * v_bu[t];
          const double dl = V::kScaleUsesLayer ? v_dl[t] : 0.0, m = V::kScaleUsesLayer ? v_m[t] : 0.0;      // (else not staged)
          const double y = v.scale(xp, xn, v_du[t], dl, m, &B[cb_idx(t, tid)]);
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
      cb_lit_product<false>(A, Mj, nlit, d, in, A);
      d = in;
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
        p.smax[(size_t)box * nlit + tid] = smax;
        p.ub0[(size_t)box * nlit + tid] = bias;
        p.step[(size_t)box * nlit + tid] = (double)s;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nlit * n0; idx += 256) {
      const int i = idx / n0, t = idx - i * n0;
      if (v_flag[i] != 0.0) p.uA[((size_t)box * nlit + i) * n0 + t] = A[cb_idx(t, i)];
    }
    if constexpr (V::kKeepsBest)
      for (int idx = tid; idx < nst; idx += 256) {
        const int n = idx / nlit, i = idx - n * nlit;
        if (v_flag[i] != 0.0) v.keep(idx, cur[idx]);
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
      layer(Mj + (size_t)din * dj, dj, o, std::true_type{});
      cb_lit_product<true>(B, Mj, nlit, din, dj, B);
      for (int idx = tid; idx < nlit * dj; idx += 256) {
        const int t = idx / nlit, i = idx - t * nlit;
        const size_t sidx = (size_t)o * nlit + idx;
        const double z = B[cb_idx(t, i)] + v_bj[t];
        const double lm = lam[sidx];
        const double g = v.grad(v_m[t], lm, z);
        lam[sidx] = g;
        A[cb_idx(t, i)] = fabs(g);
        B[cb_idx(t, i)] = lm > 0.0 ? v_du[t] * z + v_bu[t] : v.lower_slope(V::kScaleUsesLayer ? v_dl[t] : 0.0, &cur[sidx]) * z;
      }
      __syncthreads();
      if (tid < nlit)
        for (int t = 0; t < dj; ++t) {
          const double ag = A[cb_idx(t, tid)];
          gmax = ag > gmax ? ag : gmax;
        }
      din = dj;
    }
    // ---- step; a literal whose gradient vanishes is stationary and stays where it is
    if (tid < nlit) v_gmax[tid] = gmax;
    if (__syncthreads_and(tid >= nlit || !(gmax > 0.0))) break;
    for (int idx = tid; idx < nst; idx += 256) {
      const int n = idx / nlit, i = idx - n * nlit;
      const double gm = v_gmax[i];
      if (gm > 0.0) cur[idx] = v.project(cur[idx] - eta * lam[idx] / gm);
    }
    eta *= p.decay;
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace nnsdp
