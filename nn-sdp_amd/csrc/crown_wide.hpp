// The wide instance of the resident CROWN kernel (k_crown_wide<ACT>, launched by an nnsdp_crown handle created with max_width 128):
// the passes of crown_batch.hpp for hidden layers up to 128 wide; xdims[0], xdims[K] and nlit stay at 64 or below.  The recurrences
// are those of crown_pass, operation for operation; what changes is where the numbers sit (crown_wide_layout.hpp).  The pass is a
// copy of crown_pass with the slab loop and the second tile rather than one more parameter of it: k_crown_batch and k_crown_resident
// keep their source and with it their instruction streams (profiles/crown_wide_resources.txt), and neither pays for a loop it never
// takes.  The tanh relaxation, the interval step and the argument block are shared; cb_idx's swizzle is restated as cw_idx in the
// layout header, which has to compile without HIP.
//
// Slabs.  The rows of a backward pass do not depend on each other, so a pass of nout rows runs in ceil(nout / 64) slabs of at most 64
// rows: LDS holds the two coefficient matrices as 64 rows x 128 columns ([column][row] with cb_idx's swizzle and its row stride of
// 64, so the bank argument of crown_batch.hpp holds as it stands).  A slab loads its rows of the head (its rows of I for the identity
// head), walks the layers, concretises over the box and writes its rows of the results; the relaxation vectors of a layer (128 long
// here) are read again by every slab.  A layer's Tanh relaxation is still computed once per box, by the pre-activation pass, each
// slab for its own rows.  One workgroup per box, no atomics.  137 216 B of LDS (ReLU) / 138 240 B (Tanh): one workgroup per CU, where
// the narrow instance has two - the reason why the caller has to ask for this instance.
//
// Product.  A <- A W_j has up to eight 16-wide column tiles.  The workgroup keeps its 256 threads and wave w owns the column tiles w
// and w + 4 of both matrices (16 accumulator tiles, 128 registers) rather than running eight waves with one tile each: the A operand
// of a k-step is read from LDS once and feeds the MFMAs of both tiles, which halves the LDS traffic of the product; one workgroup per
// CU leaves a wave 512 registers, so the 16 tiles fit without a spill; and the (matrix, row) threads of the row passes, the launch
// geometry and the frontier kernels behind it stay as they are.  Tile w + 4 is skipped as a whole (wave-uniform) when the layer has
// no such columns, so a layer of at most 64 inputs does the narrow instance's work.  Every tile of a slab is in registers before the
// barrier behind which the first one is written back.
//
// Order of sums, per output element, as in the narrow instance: the k-steps ascending in groups of four that start at multiples of
// four, padded steps skipped (never added), the row passes ascending in t.  A network of widths at most 64 has one slab per pass and
// no second tile, and gets the bits of k_crown_resident<ACT> (tests/test_crown_wide_gpu.py).
#pragma once
#include "crown_batch.hpp"
#include "crown_wide_layout.hpp"

namespace nnsdp {

// crown_pass of crown_batch.hpp in slabs; the arguments are its arguments.  (Inlined by force: left to itself the compiler keeps the
// literal pass as a call, and the kernel's arguments then live in scratch memory.)
template <bool LIT, int ACT>
__device__ __forceinline__ void crown_pass_wide(const CrownArgs& a, double* lds, long long box, int k, int head_identity) {
  double* A[2] = {lds, lds + kCwMat};
  double* v_du = lds + kCwOffDu;
  double* v_dl = lds + kCwOffDl;
  double* v_bu = lds + kCwOffBu;
  double* v_bj = lds + kCwOffBj;
  double* v_c = lds + kCwOffC;        // box centre
  double* v_r = lds + kCwOffR;        // box radius
  double* v_res = lds + kCwOffRes;    // 2 x 64: a slab's lower / upper results, for the post-fix
  double* v_bl = lds + kCwOffBl;      // Tanh only (kCwLdsBytesTanh): the lower relaxation's bias
  constexpr int kScr = ACT == kCbTanh ? 6 : 2;      // doubles of scratch per hidden neuron
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lc = lane >> 4;
  const int mat = tid >> 6, row = tid & 63;      // the (matrix, row of the slab) a thread owns in the row passes (threads 0..127)
  const int nout = LIT ? a.nlit : a.xdims[k];
  const int jtop = head_identity ? k - 1 : k - 2;
  if (tid < a.xdims[0]) {
    const double l = a.lo[(size_t)box * a.xdims[0] + tid], u = a.hi[(size_t)box * a.xdims[0] + tid];
    v_c[tid] = (u + l) / 2.0;
    v_r[tid] = (u - l) / 2.0;
  }
  for (int slab = 0; slab < cw_slabs(nout); ++slab) {
    const int r0 = kCwRows * slab, nr = cw_slab_rows(nout, slab);      // the slab's rows r0 .. r0 + nr - 1 of the pass
    int d = head_identity ? nout : a.xdims[k - 1];
    double bias = 0.0;
    {
      const double* Mh = LIT ? a.H : a.M + a.moff[k - 1];
      for (int idx = tid; idx < nr * d; idx += 256) {
        const int t = idx / nr, i = idx - t * nr;
        const double v = head_identity ? (t == r0 + i ? 1.0 : 0.0) : Mh[(size_t)t * nout + r0 + i];
        A[0][cw_idx(t, i)] = v;
        A[1][cw_idx(t, i)] = v;
      }
      if (tid < 128 && row < nr && !head_identity) bias = Mh[(size_t)d * nout + r0 + row];
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
      }
      __syncthreads();
      if (tid < 128 && row < nr) {
        double* Am = A[mat];
        double s = 0.0, tl = 0.0;
        for (int t = 0; t < d; ++t) {
          const double x = Am[cw_idx(t, row)];
          const double xp = x > 0.0 ? x : 0.0, xn = x < 0.0 ? x : 0.0;
          const double du = v_du[t], dl = v_dl[t];
          if (ACT == kCbTanh) s += mat ? xp * v_bu[t] + xn * v_bl[t] : xn * v_bu[t] + xp * v_bl[t];
          else s += (mat ? xp : xn) * v_bu[t];
          const double y = mat ? xp * du + xn * dl : xp * dl + xn * du;
          Am[cw_idx(t, row)] = y;
          tl += y * v_bj[t];
        }
        bias += s;
        bias += tl;
      }
      __syncthreads();
      // A (nr x d) <- A W_j (nr x in): MFMA operand a = A[16 it + lr][4 ks + lc] from LDS, b = W_j[4 ks + lc][16 (w + 4 h) + lr] from
      // global, h = 0, 1 the wave's two column tiles
      const int nit = (nr + 15) >> 4, nqt = (in + 15) >> 4, ks = (d + 3) >> 2;
      const bool two = w + 4 < nqt;      // (wave-uniform)
      d4_t c[2][2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int it = 0; it < 4; ++it) c[h][m][it] = d4_t{0.0, 0.0, 0.0, 0.0};
      const int q0 = 16 * w + lr, q1 = q0 + 64;
      if (w < nqt) {
        for (int k0 = 0; k0 < ks; k0 += kCbChunk) {
          double bv[2][kCbChunk];
#pragma unroll
          for (int u = 0; u < kCbChunk; ++u) {
            const int t = 4 * (k0 + u) + lc;
            bv[0][u] = (q0 < in && t < d) ? Mj[(size_t)q0 * d + t] : 0.0;
            bv[1][u] = (two && q1 < in && t < d) ? Mj[(size_t)q1 * d + t] : 0.0;
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
                  const bool ok = t < d && i < nr;
                  const double al = ok ? A[0][cw_idx(tc, i)] : 0.0;
                  const double au = ok ? A[1][cw_idx(tc, i)] : 0.0;
                  c[0][0][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bv[0][u], c[0][0][it], 0, 0, 0);
                  c[0][1][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv[0][u], c[0][1][it], 0, 0, 0);
                  if (two) {
                    c[1][0][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bv[1][u], c[1][0][it], 0, 0, 0);
                    c[1][1][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv[1][u], c[1][1][it], 0, 0, 0);
                  }
                }
              }
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = h ? q1 : q0;
        if ((h ? two : w < nqt) && q < in) {
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            if (it < nit) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int i = 16 * it + lc + 4 * r;
                if (i < nr) {
                  A[0][cw_idx(q, i)] = c[h][0][it][r];
                  A[1][cw_idx(q, i)] = c[h][1][it][r];
                }
              }
            }
          }
        }
      }
      d = in;
      __syncthreads();
    }
    if (tid < 128 && row < nr) {
      const double* Am = A[mat];
      double s = 0.0, rr = 0.0;
      for (int t = 0; t < d; ++t) {
        const double x = Am[cw_idx(t, row)];
        s += x * v_c[t];
        rr += fabs(x) * v_r[t];
      }
      v_res[mat * kCwRows + row] = mat ? s + rr + bias : s - rr + bias;
      if (LIT && mat && a.ub0) a.ub0[(size_t)box * nout + r0 + row] = bias;
    }
    __syncthreads();
    if (LIT) {      // (nout = nlit <= 64: one slab, r0 = 0)
      if (tid < nr) {
        if (a.smin) a.smin[(size_t)box * nout + r0 + tid] = v_res[tid];
        if (a.smax) a.smax[(size_t)box * nout + r0 + tid] = v_res[kCwRows + tid];
      }
      if (a.uA)
        for (int idx = tid; idx < nr * d; idx += 256) {       // d == xdims[0] here; A[1] is the upper bound's matrix after the last product
          const int i = idx / d, t = idx - i * d;
          a.uA[((size_t)box * nout + r0 + i) * d + t] = A[1][cw_idx(t, i)];
        }
    } else if (tid < nr) {
      const double l = v_res[tid], u = v_res[kCwRows + tid];
      const int g = r0 + tid;      // the row of the pass
      if (!head_identity && k < a.K) {
        double* pre = a.scratch + (size_t)box * kScr * a.acdim + a.acoff[k - 1];
        pre[g] = l;
        pre[a.acdim + g] = u;
        if (ACT == kCbTanh) {      // the layer's relaxation, once: every later pass reads it
          double lw, lb, uw, ub;
          cb_tanh_relax(l, u, lw, lb, uw, ub);
          pre[2 * (size_t)a.acdim + g] = lw;
          pre[3 * (size_t)a.acdim + g] = lb;
          pre[4 * (size_t)a.acdim + g] = uw;
          pre[5 * (size_t)a.acdim + g] = ub;
        }
      } else {
        const double fl = l < u ? l : u, fu = fl > u ? fl : u;     // lb = min(lb, ub), ub = max(lb, ub)
        if (head_identity) {
          const size_t o = (size_t)box * a.acdim + a.acoff[k - 1] + g;
          a.acymin[o] = fl;
          a.acymax[o] = fu;
        } else {
          const size_t o = (size_t)box * nout + g;
          a.ymin[o] = fl;
          a.ymax[o] = fu;
        }
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// The kernel of a wide resident bounder: k_crown_resident<ACT> of crown_batch.hpp on the slab passes; LDS kCwLdsBytes (ReLU) /
// kCwLdsBytesTanh (Tanh).
template <int ACT>
__global__ __launch_bounds__(256) void k_crown_wide(CrownArgs a) {
  extern __shared__ double cb_lds[];
  const long long box = blockIdx.x;
  for (int k = 1; k <= a.K; ++k) {
    crown_pass_wide<false, ACT>(a, cb_lds, box, k, 0);
    if (k < a.K) crown_pass_wide<false, ACT>(a, cb_lds, box, k, 1);
  }
  if (a.nlit > 0) crown_pass_wide<true, ACT>(a, cb_lds, box, a.K, 0);
  crown_interval_step(a, box);
}

}  // namespace nnsdp
