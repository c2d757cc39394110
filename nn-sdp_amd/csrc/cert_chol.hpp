// Sparse negative-semidefiniteness check of Z on the clique pattern: a multifrontal Cholesky of N = -Z along the plan of
// cert_plan.hpp, ONE WORKGROUP PER CANDIDATE, every front a full square in LDS.  Included by kernels.hip.
//
// Per supernode (columns c0 .. c1-1, rows below r_0 < ... < a):
//   assemble   F = 0; F <- -Z entries of the supernode's columns from the candidate's NE-vector (off-diagonal entries carry the svec
//              factor sqrt 2: undone here); F += update matrices of the children, one child after the other (extend-add through
//              the plan's relative positions; within one child every target is distinct)
//   factor     right-looking in panels of 16 columns: the panel column by column on the vector units (pivot test, sqrt, scale, rank-1
//              update inside the panel), then the trailing update F22 -= P P' on v_mfma_f64_16x16x4_f64, lower 16 x 16 tiles anchored
//              at the first trailing row; a panel narrower than 16 (the supernode's last) masks the missing k, tiles that stick out
//              past the front mask their stores - sizes need not be multiples of 16 or 4
//   hand over  the trailing rows x rows square is the supernode's update matrix: to the candidate's scratch (lower triangle)
// The row of a is the last row of every front, so the forward solve of z_xa is part of the factorisation; the roots' 1 x 1 update
// matrices plus -Z_aa are the Schur complement of N, summed in root order by one lane.
//
// LDS layout: column-major, leading dimension ld = 16 (mod 32) doubles and >= front rounded to 16, plus 16.  An MFMA operand read
// takes, per 32-lane half, rows r .. r+15 of two neighbouring columns: 16 consecutive doubles = 32 banks each, the second column 16
// doubles (mod 32) further = the other 32 of the 64 banks ds_read_b64 sees: conflict-free.  Front 128: 128 x 144 x 8 B = 144 KiB of
// the CU's 160.  Tiles may READ up to 15 rows past the front (inside the column's padding or the next column, never past the
// allocation); those rows only reach result rows whose stores are masked.
// No atomics, fixed order everywhere, nothing depends on blockIdx but the candidate's own pointers: a candidate's bits are the same
// for every batch size and position.
#pragma once

namespace nnsdp {

static constexpr int kCertThreads = 256;

struct CertArgs {
  int n_super, e_aa, n_roots;
  const int* col_start;
  const int* row_ptr;
  const int* rel;
  const int* child_ptr;
  const int* child_idx;
  const int* roots;
  const int* gat_ptr;
  const int* gat_pos;
  const int* gat_ent;
  const long long* upd_off;
  const double* z;          // candidates' NE-vectors (svec-scaled), zstride apart
  long long zstride;
  double* scratch;          // sstride doubles per candidate
  long long sstride;
  double pivot_floor;       // a pivot must exceed pivot_floor x the largest diagonal entry of its supernode's columns as assembled
  double diag_margin;       // subtracted from every diagonal entry of -Z_xx as it is gathered: ok then says Z_xx <= -diag_margin I, and the
                            // Schur complement, taken with (-Z_xx - diag_margin I)^-1 >= (-Z_xx)^-1, errs on the safe (larger) side
  int ld;
  int* ok;                  // per candidate: 1 = every pivot passed
  int* fail_col;            //   first failing column (-1)
  double* min_pivot;        //   smallest pivot met (the failing one included)
  double* schur;            //   Z_aa - z_xa' Z_xx^-1 z_xa  (NaN when !ok)
};

static inline int cert_ld(int max_front) {
  const int mp = (max_front + 15) & ~15;
  return ((mp + 16 + 15) / 32) * 32 + 16;
}
static inline size_t cert_lds_bytes(int max_front) {
  const int mp = (max_front + 15) & ~15;
  return (size_t)mp * cert_ld(max_front) * sizeof(double);
}

__global__ __launch_bounds__(kCertThreads) void k_cert_chol(CertArgs a) {
  extern __shared__ double lds[];
  __shared__ double s_red[kCertThreads / 64];
  double* const F = lds;
  const int ld = a.ld;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lc = lane >> 4;
  constexpr int NW = kCertThreads / 64;
  const int b = blockIdx.x;
  const double* const z = a.z + (size_t)b * a.zstride;
  double* const scr = a.scratch + (size_t)b * a.sstride;
  double minp = 1e300;
  for (int s = 0; s < a.n_super; ++s) {
    const int c0 = a.col_start[s], nc = a.col_start[s + 1] - c0;
    const int nr = a.row_ptr[s + 1] - a.row_ptr[s], m = nc + nr;
    // assemble
    for (int q = tid; q < m * m; q += kCertThreads) { const int j = q / m, i = q - j * m; F[i + j * ld] = 0.0; }
    __syncthreads();
    for (int q = a.gat_ptr[s] + tid; q < a.gat_ptr[s + 1]; q += kCertThreads) {
      const int pos = a.gat_pos[q], i = pos >> 8, j = pos & 255;
      const double v = z[a.gat_ent[q]];
      F[i + j * ld] = i == j ? -v - a.diag_margin : -v * kInvSqrt2;      // (a is no column of any supernode: every diagonal here is an x one)
    }
    __syncthreads();
    for (int t = a.child_ptr[s]; t < a.child_ptr[s + 1]; ++t) {
      const int c = a.child_idx[t];
      const int rp = a.row_ptr[c], nrc = a.row_ptr[c + 1] - rp;
      const double* const U = scr + a.upd_off[c];
      for (int q = tid; q < nrc * nrc; q += kCertThreads) {
        const int j = q / nrc, i = q - j * nrc;
        if (i >= j) F[a.rel[rp + i] + a.rel[rp + j] * ld] += U[q];
      }
      __syncthreads();
    }
    // largest diagonal entry of the supernode's columns as assembled
    double dm = 0.0;
    for (int j = tid; j < nc; j += kCertThreads) dm = fmax(dm, F[j + j * ld]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o, 64));
    if (lane == 0) s_red[wv] = dm;
    __syncthreads();
    dm = s_red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) dm = fmax(dm, s_red[w]);
    const double floor_abs = a.pivot_floor * dm;
    // factor
    for (int j0 = 0; j0 < nc; j0 += 16) {
      const int w = min(16, nc - j0);
      for (int k = 0; k < w; ++k) {
        const int col = j0 + k;
        const double piv = F[col + col * ld];          // (uniform: every thread reads the same word after the barrier)
        minp = fmin(minp, piv);
        if (!(piv > floor_abs)) {
          if (tid == 0) { a.ok[b] = 0; a.fail_col[b] = c0 + col; a.min_pivot[b] = minp; a.schur[b] = __builtin_nan(""); }
          return;
        }
        const double dinv = 1.0 / sqrt(piv);           // (the factor's diagonal itself is never read again: not stored)
        for (int i = col + 1 + tid; i < m; i += kCertThreads) F[i + col * ld] *= dinv;
        __syncthreads();
        // rank-1 update of the panel's remaining columns, lower part
        const int rest = w - 1 - k, below = m - col - 1;
        for (int q = tid; q < rest * below; q += kCertThreads) {
          const int cc = q / below, i = col + 1 + (q - cc * below), j = col + 1 + cc;
          if (i >= j) F[i + j * ld] -= F[i + col * ld] * F[j + col * ld];
        }
        __syncthreads();
      }
      // trailing update on the matrix cores: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]; result r is C[(l >> 4) + 4 r][l & 15]
      const int r0 = j0 + w, nt = (m - r0 + 15) >> 4;
      for (int t = wv; t < nt * (nt + 1) / 2; t += NW) {
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2;
        const double* const ap = F + (r0 + 16 * ti + lr) + (j0 + lc) * ld;
        const double* const bp = F + (r0 + 16 * tj + lr) + (j0 + lc) * ld;
        d4_t c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const bool in = 4 * kk + lc < w;
          const double av = in ? ap[4 * kk * ld] : 0.0, bv = in ? bp[4 * kk * ld] : 0.0;
          c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
        }
        const int j = r0 + 16 * tj + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = r0 + 16 * ti + lc + 4 * r;
          if (i < m && i >= j) F[i + j * ld] -= c[r];
        }
      }
      __syncthreads();
    }
    // hand over the update matrix (lower triangle of the trailing nr x nr square)
    double* const U = scr + a.upd_off[s];
    for (int q = tid; q < nr * nr; q += kCertThreads) {
      const int j = q / nr, i = q - j * nr;
      if (i >= j) U[q] = F[(nc + i) + (nc + j) * ld];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double naa = a.e_aa >= 0 ? -z[a.e_aa] : 0.0;
    for (int t = 0; t < a.n_roots; ++t) naa += scr[a.upd_off[a.roots[t]]];
    a.ok[b] = 1; a.fail_col[b] = -1; a.min_pivot[b] = minp; a.schur[b] = -naa;
  }
}

// z_b = z0 + A gamma_b for B multiplier vectors in one launch (blockIdx.y = candidate); row by row the arithmetic of k_apply_A
__global__ __launch_bounds__(kThreads) void k_apply_A_multi(int NE, const int* __restrict__ ptr, const int* __restrict__ col,
                                                             const double* __restrict__ val, const double* __restrict__ gam, long long gstride,
                                                             const double* __restrict__ z0, double* __restrict__ z, long long zstride) {
  int e = (blockIdx.x * kThreads + threadIdx.x) >> 4;
  int sub = threadIdx.x & 15;
  const double* g = gam + (size_t)blockIdx.y * gstride;
  double s = 0.0;
  if (e < NE)
    for (int q = ptr[e] + sub; q < ptr[e + 1]; q += 16) s += val[q] * g[col[q]];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
  if (e < NE && sub == 0) z[(size_t)blockIdx.y * zstride + e] = (z0 ? z0[e] : 0.0) + s;
}

}  // namespace nnsdp
