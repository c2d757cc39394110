// What the device-resident split searches share on the device: the single clause search (csrc/crown_search.hpp), the reach search
// (csrc/crown_reach.hpp), the forest of searches (csrc/crown_forest.hpp) and the ReLU-split node search (csrc/crown_node_search.hpp,
// which takes the centre, its own corner, the flag "every literal false" and the scan tile from here).  Each search's result is defined
// as the Python loop's tree (nnsdp_amd/split.py, nnsdp_amd/relusplit.py) bit for bit, so every piece of arithmetic that decides
// something is stated here ONCE and the kernels of the headers are thin bodies over it: a literal's bound and the best literal of a box, the split coordinate, the centre and a corner of
// a box, normal' y and the flag "every literal false", the bisection, the head of a leaf-log row, the 256-wide scan tile.
//
// The arithmetic restates numpy's operation for operation: products and sums are rounded separately, sums have numpy's order, minima
// and maxima keep the first of equal values.  Contraction into FMA is a property of the function a statement is written in, not of the
// kernel it is inlined into, so EVERY helper below that does floating-point arithmetic carries its own #pragma clang fp contract(off)
// (the __dmul_rn / __dadd_rn of the HIP headers are inline functions compiled with contraction allowed and fuse after inlining, so
// they are not used).  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace nnsdp {

// the two frontiers of a search (2 buffers x 2 max_boxes boxes x n0 x (lo, hi, cuts) = 80 n0 max_boxes bytes) may not exceed this
static constexpr size_t kSearchFrontierCap = (size_t)1 << 31;

// What SearchArgs, ReachArgs and ForestArgs have in common.  Frontier: lo, hi (doubles) and cuts (ints), each n0 x nbox column-major,
// the layout CrownArgs.lo / hi read; two of them: the level being bounded and the one its children are written to.  The host fills the
// level's part with FrontierBufs::level (csrc/crown_handle.hpp)
struct FrontierArgs {
  int n0, ny, nlit;               // input width, output width, literals (directions) of the search
  int depth;                      // the level
  int corner_points;
  const double* normals;          // ny x nlit column-major
  const double *lo, *hi;          // the level's frontier
  const int* cuts;
  double *nlo, *nhi;              // the next frontier
  int* ncuts;
  double* X;                      // n0 x points: the centres of the level's boxes, then their corners
  const double* Y;                // ny x points
  double* log;                    // leaf log; this level's rows start at log_base
  long long log_base;
};

// max(n_j ymin_j, n_j ymax_j), numpy's maximum (the first of equal values)
__device__ __forceinline__ double search_term(const double* nrm, const double* ymin, const double* ymax, int j) {
#pragma clang fp contract(off)
  const double p = nrm[j] * ymin[j], q = nrm[j] * ymax[j];
  return p >= q ? p : q;
}

// sum_j max(n_j ymin_j, n_j ymax_j) in the order of numpy's sum(axis=0) in split.py.  The bounder returns ymin / ymax as transposes of
// nbox x ny arrays, so the ny x nbox array of terms is column-major, the reduced axis is the contiguous one and numpy takes its pairwise
// routine for every box, whatever nbox: below 8 terms a plain ascending sum from 0.0; from 8 terms on eight partial sums r_k over the
// terms k, k + 8, ... of the leading multiple of 8, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining
// terms added in ascending order (the recursive halving starts above 128 terms; ny <= 64 here)
__device__ __forceinline__ double search_cheap(const double* nrm, const double* ymin, const double* ymax, int ny) {
#pragma clang fp contract(off)
  if (ny < 8) {
    double s = 0.0;
    for (int j = 0; j < ny; ++j) s = s + search_term(nrm, ymin, ymax, j);
    return s;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = search_term(nrm, ymin, ymax, k);
  int i = 8;
  for (; i < ny - (ny & 7); i += 8)
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = r[k] + search_term(nrm, ymin, ymax, i + k);
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < ny; ++i) s = s + search_term(nrm, ymin, ymax, i);
  return s;
}

// the bound of one literal on one box: the cheap bound, or (smax != null) min(cheap, *smax), numpy's minimum (the first of equal values)
__device__ __forceinline__ double search_literal(const double* nrm, const double* ymin, const double* ymax, int ny, const double* smax) {
#pragma clang fp contract(off)
  const double cheap = search_cheap(nrm, ymin, ymax, ny);
  if (!smax) return cheap;
  const double s = *smax;
  return cheap <= s ? cheap : s;
}

// the best literal of a box: the first minimum of bound_i - hs_i; ymin / ymax (ny) and smax (nlit) are the box's outputs of the bound kernel
struct BestLiteral {
  int best;
  double bexc, bcheap;            // its excess over the threshold and its bound
};
__device__ __forceinline__ BestLiteral search_best(const double* normals, const double* hs, const double* ymin, const double* ymax,
                                                   const double* smax, int nlit, int ny, int literal_bounds) {
#pragma clang fp contract(off)
  BestLiteral r{0, 0.0, 0.0};
  for (int i = 0; i < nlit; ++i) {
    const double cheap = search_literal(normals + (size_t)i * ny, ymin, ymax, ny, literal_bounds ? smax + i : nullptr);
    const double exc = cheap - hs[i];
    if (i == 0 || exc < r.bexc) { r.best = i; r.bexc = exc; r.bcheap = cheap; }
  }
  return r;
}

// the split coordinate of a box: the first coordinate of the mask (bit t: root_hi[t] > root_lo[t]) with the fewest cuts; -1: none
__device__ __forceinline__ int frontier_coord(const int* cuts, int n0, unsigned long long mask) {
  int coord = -1, cmin = 0;
  for (int t = 0; t < n0; ++t)
    if ((mask >> t) & 1ull) {
      const int v = cuts[t];
      if (coord < 0 || v < cmin) { coord = t; cmin = v; }
    }
  return coord;
}

// the centre of a box, and its corner  where(A >= 0, hi, lo)  for a row A of uA
__device__ __forceinline__ void frontier_centre(double* x, const double* lo, const double* hi, int n0) {
#pragma clang fp contract(off)
  for (int t = 0; t < n0; ++t) x[t] = 0.5 * (lo[t] + hi[t]);
}
__device__ __forceinline__ void frontier_corner(double* x, const double* A, const double* lo, const double* hi, int n0) {
  for (int t = 0; t < n0; ++t) x[t] = A[t] >= 0.0 ? hi[t] : lo[t];
}

// the ReLU-split driver's corner  c + sign(A) r  with c = 0.5 (lo + hi), r = 0.5 (hi - lo) and numpy's sign (sign(0) = 0, sign(NaN) =
// NaN); the product and the sum are rounded separately.  Not frontier_corner: where A is zero this is the centre's coordinate
__device__ __forceinline__ void frontier_sign_corner(double* x, const double* A, const double* lo, const double* hi, int n0) {
#pragma clang fp contract(off)
  for (int t = 0; t < n0; ++t) {
    const double c = 0.5 * (lo[t] + hi[t]), r = 0.5 * (hi[t] - lo[t]), v = A[t];
    const double sg = v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : v == 0.0 ? 0.0 : v;
    const double m = sg * r;
    x[t] = c + m;
  }
}

// normal' y as numpy's  (normal[:, None] * Y).sum(axis=0)  gives it: n_0 y_0, then + n_j y_j for j ascending (ny >= 1)
__device__ __forceinline__ double frontier_dot(const double* nrm, const double* y, int ny) {
#pragma clang fp contract(off)
  double s = nrm[0] * y[0];
  for (int j = 1; j < ny; ++j) {
    const double m = nrm[j] * y[j];
    s = s + m;
  }
  return s;
}

// every literal false at the point y:  normal_i' y > hs_i  for all i
__device__ __forceinline__ int search_all_false(const double* normals, const double* hs, const double* y, int nlit, int ny) {
  for (int i = 0; i < nlit; ++i)
    if (!(frontier_dot(normals + (size_t)i * ny, y, ny) > hs[i])) return 0;
  return 1;
}

// box b of the level is bisected at the middle of coordinate j; its children go to slots k, k + 1 of the next frontier
__device__ __forceinline__ void frontier_bisect(const FrontierArgs& f, int b, int j, size_t k) {
#pragma clang fp contract(off)
  const int n0 = f.n0;
  const double* lo = f.lo + (size_t)b * n0;
  const double* hi = f.hi + (size_t)b * n0;
  const double mid = 0.5 * (lo[j] + hi[j]);
  const size_t L = k * n0, R = L + n0;
  for (int t = 0; t < n0; ++t) {
    const int cv = f.cuts[(size_t)b * n0 + t] + (t == j ? 1 : 0);
    f.nlo[L + t] = lo[t];
    f.nhi[L + t] = t == j ? mid : hi[t];
    f.nlo[R + t] = t == j ? mid : lo[t];
    f.nhi[R + t] = hi[t];
    f.ncuts[L + t] = cv;
    f.ncuts[R + t] = cv;
  }
}

// the head of a leaf-log row of logw doubles: lo, hi and the depth of box b of the level; the tail (what the search knows about the box)
// starts where the returned pointer points
__device__ __forceinline__ double* frontier_log_row(const FrontierArgs& f, double* log, long long row, size_t logw, int b) {
  const int n0 = f.n0;
  double* r = log + (size_t)row * logw;
  for (int t = 0; t < n0; ++t) { r[t] = f.lo[(size_t)b * n0 + t]; r[n0 + t] = f.hi[(size_t)b * n0 + t]; }
  r[2 * n0] = (double)f.depth;
  return r + 2 * n0 + 1;
}

static constexpr int kScanTile = 256;

// Inclusive scan of Q rows of 256 ints across the 256 threads of a workgroup (all of them call it): v holds the thread's Q counts on
// entry and their inclusive prefixes on return, when s[q][255] holds the row's total.  A barrier must separate that read from the next call
template <int Q>
__device__ __forceinline__ void scan_tile(int (&s)[Q][kScanTile], int tid, int (&v)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) s[q][tid] = v[q];
  __syncthreads();
  for (int d = 1; d < kScanTile; d <<= 1) {
    int add[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) add[q] = tid >= d ? s[q][tid - d] : 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q][tid] += add[q];
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = s[q][tid];
}

// ONE workgroup walks n counts in tiles of 256 with a carried offset: out[k] = in[0] + ... + in[k - 1]; returns the total.  in == out is allowed
__device__ __forceinline__ int scan_walk(int (&s)[1][kScanTile], int tid, const int* in, int* out, int n) {
  int carry = 0;
  for (int t0 = 0; t0 < n; t0 += kScanTile) {
    const int k = t0 + tid;
    const int c = k < n ? in[k] : 0;
    int v[1] = {c};
    scan_tile<1>(s, tid, v);
    if (k < n) out[k] = carry + v[0] - c;
    carry += s[0][kScanTile - 1];
    __syncthreads();
  }
  return carry;
}

}  // namespace nnsdp
