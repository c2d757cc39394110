// Optimised ReLU slopes for the literal pass of the resident CROWN bounder (alpha-CROWN, nnsdp_crown_bound_alpha).
// k_crown_alpha runs on the handle's stream after k_crown_resident<kCbRelu> and reads the raw pre-activation bounds that kernel left in
// the scratch.  Per box and per literal i, independently of the other literals: T projected-gradient steps on the lower slope alpha in
// [0, 1] of every unstable neuron (l < 0 < u) of the UPPER bound's backward pass; the result is the first iterate with the smallest smax.
//
// One workgroup of 256 threads per box.  LDS: the upper matrix A (64 x 64, the cb_idx layout of crown_batch.hpp) and a second 64 x 64
// region B in the place of crown_pass's lower matrix, plus ten 64-double vectors: 70 656 B (kCaLdsBytes).  The LDS would let two
// workgroups share a CU; the registers do not (274 of 512 per SIMD, profiles/crown_alpha_resources.txt): one workgroup per CU.
//   backward pass at alpha^s: crown_pass<true>'s upper matrix, operation for operation - per layer the slopes of the layer come from the
//     state buffer into B, thread (row i) scales its row (lambda > 0: du and bu; else alpha and no bias) and leaves lambda in B, which
//     goes back to the state buffer; then A <- A W_j on v_mfma_f64_16x16x4_f64 exactly as there.  Iterate 0 without alpha0 therefore has
//     the bits of the plain literal pass.
//   gradient: x* = c + sgn(uA) r per literal goes to B, and per layer Z (nlit x d_j) = B (nlit x in) W_j' on the same instruction (a from
//     B in LDS, b = W_j[q][t] from global memory); the element pass turns Z into g = min(lambda, 0) z (unstable neurons) and into the
//     next layer's input  D z + beta  with the pair the backward pass chose; |g| goes through A for the per-literal maximum.
//   step: alpha <- clip(alpha - eta0 decay^s g / max|g|, 0, 1).
// The per-(literal, neuron) state - alpha, lambda / g, the best alpha - lives in device buffers of the handle, stored [neuron][literal]
// per box so that a layer's slice moves between global memory and LDS with consecutive lanes on consecutive addresses of both.
// No atomics; max|g| is a maximum of absolute values (exact in any order) taken in a fixed order anyway, every other sum is per row, t
// ascending.  A literal's bits depend neither on nbox, nor on the box's position, nor on the other literals, nor on earlier calls.
#pragma once
#include "crown_batch.hpp"

namespace nnsdp {

struct CrownAlphaArgs {
  CrownArgs c;              // the network, the head, the boxes and the scratch of the plain launch before this one
  int steps;                // T in 0..64
  double eta0, decay;
  const double* alpha0;     // null, or acdim x nlit x nbox (neuron index fastest)
  double *cur, *lam, *best; // state, acdim x nlit doubles per box each, [neuron][literal]: alpha^s; lambda, then g; the best alpha
  double *a_smax, *a_ub0;   // nlit x nbox
  double* a_step;           // nlit x nbox, the best iterate's index as a double (one download brings everything back)
  double* a_uA;             // xdims[0] x nlit x nbox
  double* alpha;            // acdim x nlit x nbox (neuron index fastest)
};

static constexpr size_t kCaLdsBytes = (2 * kCbW * kCbW + 10 * kCbW) * sizeof(double);

// du, bu of the plain relaxation from raw pre-activation bounds (the arithmetic of crown_pass), the plain lower slope, l < 0 < u
__device__ __forceinline__ void ca_relax(double l, double u, double& du, double& dl, double& bu, bool& uns) {
  const double lrx = l < 0.0 ? l : 0.0;
  double ur = u > 0.0 ? u : 0.0;
  ur = ur > lrx + 1e-8 ? ur : lrx + 1e-8;
  du = ur / (ur - lrx);
  dl = du > 0.5 ? 1.0 : 0.0;
  bu = -lrx * du;
  uns = l < 0.0 && u > 0.0;
}

__global__ __launch_bounds__(256) void k_crown_alpha(CrownAlphaArgs p) {
  extern __shared__ double ca_lds[];
  const CrownArgs& a = p.c;
  double* A = ca_lds;                       // the upper matrix; |g| during the forward pass
  double* B = ca_lds + kCbW * kCbW;         // a layer's alpha, then its lambda (backward); the forward values (gradient)
  double* v_du = B + kCbW * kCbW;
  double* v_bu = v_du + kCbW;
  double* v_bj = v_bu + kCbW;
  double* v_uns = v_bj + kCbW;              // 1.0 at an unstable neuron
  double* v_c = v_uns + kCbW;
  double* v_r = v_c + kCbW;
  double* v_gmax = v_r + kCbW;
  double* v_flag = v_gmax + kCbW;           // 1.0: the literal's iterate is its best so far
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lc = lane >> 4;
  const long long box = blockIdx.x;
  const int K = a.K, nlit = a.nlit, acdim = a.acdim, n0 = a.xdims[0], nst = nlit * acdim;
  const size_t sbase = (size_t)box * nst;
  double *cur = p.cur + sbase, *lam = p.lam + sbase, *best = p.best + sbase;
  const double* pre = a.scratch + (size_t)box * 2 * acdim;
  const int nit = (nlit + 15) >> 4;

  // alpha^0: the plain rule, or alpha0 clipped on the unstable neurons
  for (int idx = tid; idx < nst; idx += 256) {
    const int n = idx / nlit, i = idx - n * nlit;
    double du, dl, bu;
    bool uns;
    ca_relax(pre[n], pre[acdim + n], du, dl, bu, uns);
    double v = dl;
    if (p.alpha0 && uns) {
      const double x = p.alpha0[((size_t)box * nlit + i) * acdim + n];
      v = x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
    }
    cur[idx] = v;
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
    // ---- backward pass at alpha^s: the upper matrix of crown_pass<true>
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
        double du, dl, bu;
        bool uns;
        ca_relax(pre[o + tid], pre[acdim + o + tid], du, dl, bu, uns);
        v_du[tid] = du;
        v_bu[tid] = bu;
        v_bj[tid] = Mj[(size_t)in * d + tid];
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
          const double du = v_du[t], dl = B[cb_idx(t, tid)];
          sb += xp * v_bu[t];
          const double y = xp * du + xn * dl;
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
        p.a_smax[(size_t)box * nlit + tid] = smax;
        p.a_ub0[(size_t)box * nlit + tid] = bias;
        p.a_step[(size_t)box * nlit + tid] = (double)s;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nlit * n0; idx += 256) {
      const int i = idx / n0, t = idx - i * n0;
      if (v_flag[i] != 0.0) p.a_uA[((size_t)box * nlit + i) * n0 + t] = A[cb_idx(t, i)];
    }
    for (int idx = tid; idx < nst; idx += 256) {
      const int n = idx / nlit, i = idx - n * nlit;
      if (v_flag[i] != 0.0) best[idx] = cur[idx];
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
        double du, dl, bu;
        bool uns;
        ca_relax(pre[o + tid], pre[acdim + o + tid], du, dl, bu, uns);
        v_du[tid] = du;
        v_bu[tid] = bu;
        v_bj[tid] = Mj[(size_t)din * dj + tid];
        v_uns[tid] = uns ? 1.0 : 0.0;
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
        const double lm = lam[sidx];
        const double g = v_uns[t] != 0.0 ? (lm < 0.0 ? lm : 0.0) * z : 0.0;
        lam[sidx] = g;
        A[cb_idx(t, i)] = fabs(g);
        B[cb_idx(t, i)] = lm > 0.0 ? v_du[t] * z + v_bu[t] : cur[sidx] * z;
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
      if (gm > 0.0) {
        const double v = cur[idx] - eta * lam[idx] / gm;
        cur[idx] = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
      }
    }
    eta *= p.decay;
    __threadfence_block();
    __syncthreads();
  }
  // the best alpha, neuron index fastest
  __threadfence_block();
  __syncthreads();
  for (int idx = tid; idx < nst; idx += 256) {
    const int i = idx / acdim, n = idx - i * acdim;
    p.alpha[((size_t)box * nlit + i) * acdim + n] = best[(size_t)n * nlit + i];
  }
}

}  // namespace nnsdp
