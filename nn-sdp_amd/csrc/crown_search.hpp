// Device-resident frontier of the bounds-only split search (nnsdp_crown::search of crown_handle.hpp; nnsdp_amd/split.py with frontier = "device").
// The level loop of split.py (_split_levels) with the boxes kept in device memory: per level the host launches, per chunk of the
// level, the handle's bound kernel (k_crown_resident, csrc/crown_batch.hpp, its lo / hi pointers offset into the frontier) and
// k_search_classify on the chunk's outputs; then k_forward_mfma on the level's points, k_search_refute, k_search_scan and
// k_search_scatter, and reads back the four integers of the status record.
//
// Frontier: lo, hi (doubles) and cuts (ints), each n0 x nbox column-major, the layout CrownArgs.lo / hi read.  Two of them: the
// level being bounded and the one its children are written to.
// Per-level records, indexed by the box's position in the level: open flag, best literal, its bound, the split coordinate, the
// box's rank among the level's open boxes (slot).  Points: the centres of the level's boxes, then (corner_points) their corners.
// Leaf log: one row of 2 n0 + 3 doubles per proved box, in the order split.py appends them: lo, hi, depth, literal, bound.
//
// The arithmetic that decides anything restates numpy's operation for operation, so that the tree is the Python loop's bit for bit:
// products and sums are rounded separately (contraction into FMA is switched off inside these kernels; the __dmul_rn / __dadd_rn of the
// HIP headers are inline functions compiled with contraction allowed and fuse after inlining, so they are not used), the proof test's sum has the order of numpy's pairwise routine
// (search_cheap below), minima keep the first of equal values.  No atomics: the ranks come from a scan by one workgroup that walks
// the level in tiles of 256 with a carried offset, the candidate count from a tree reduction of per-thread counts.
#pragma once
#include <hip/hip_runtime.h>

namespace nnsdp {

// the two frontiers of a search (2 buffers x 2 max_boxes boxes x n0 x (lo, hi, cuts) = 80 n0 max_boxes bytes) may not exceed this
static constexpr size_t kSearchFrontierCap = (size_t)1 << 31;

struct SearchArgs {
  int n0, ny, nlit;               // input width, output width, literals of the clause
  int nb;                         // boxes of the level that are bounded (the first nb of the frontier)
  int depth;                      // the level
  int literal_bounds, corner_points;
  unsigned long long splitmask;   // bit t: root_hi[t] > root_lo[t]
  const double* normals;          // ny x nlit column-major
  const double* hs;               // nlit
  const double *lo, *hi;          // the level's frontier
  const int* cuts;
  double *nlo, *nhi;              // the next frontier
  int* ncuts;
  int *open, *best, *coord, *slot;      // records, nb each
  double* bound;
  double* X;                      // n0 x (nb or 2 nb): centres, then corners
  const double* Y;                // ny x (points)
  int* pflag;                     // per point: every literal false there and the box open
  double* log;                    // leaf log; this level's rows start at log_base
  long long log_base;
  int* status;                    // bounded, proved, open, candidates
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

// one thread per box of a chunk: boxes off .. off + nc - 1 of the level; ymin / ymax / smax / uA are the chunk's outputs of the bound
// kernel (indexed by the box's position in the chunk)
__global__ __launch_bounds__(256) void k_search_classify(SearchArgs a, int off, int nc, const double* ymin, const double* ymax,
                                                         const double* smax, const double* uA) {
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const int b = off + c, n0 = a.n0, ny = a.ny;
  int best = 0;
  double bexc = 0.0, bcheap = 0.0;
  for (int i = 0; i < a.nlit; ++i) {
    const double* nrm = a.normals + (size_t)i * ny;
    double cheap = search_cheap(nrm, ymin + (size_t)c * ny, ymax + (size_t)c * ny, ny);
    if (a.literal_bounds) {
      const double s = smax[(size_t)c * a.nlit + i];
      cheap = cheap <= s ? cheap : s;
    }
    const double exc = cheap - a.hs[i];
    if (i == 0 || exc < bexc) { best = i; bexc = exc; bcheap = cheap; }
  }
  const int open = bexc <= 0.0 ? 0 : 1;
  int coord = -1, cmin = 0;
  for (int t = 0; t < n0; ++t)
    if ((a.splitmask >> t) & 1ull) {
      const int v = a.cuts[(size_t)b * n0 + t];
      if (coord < 0 || v < cmin) { coord = t; cmin = v; }
    }
  a.open[b] = open;
  a.best[b] = best;
  a.coord[b] = coord;
  a.bound[b] = bcheap;
  // the points of a proved box are never looked at; they are written so that the forward pass reads defined numbers
  const double* A = a.corner_points ? uA + ((size_t)c * a.nlit + best) * n0 : nullptr;
  for (int t = 0; t < n0; ++t) {
    const double l = a.lo[(size_t)b * n0 + t], u = a.hi[(size_t)b * n0 + t];
    a.X[(size_t)b * n0 + t] = 0.5 * (l + u);
    if (a.corner_points) a.X[((size_t)a.nb + b) * n0 + t] = A[t] >= 0.0 ? u : l;
  }
}

// one thread per point: the flag of  every literal false:  normal_i' y > h_i  for all i
__global__ __launch_bounds__(256) void k_search_refute(SearchArgs a, long long npts) {
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const int b = (int)(p % a.nb), ny = a.ny;
  int f = a.open[b];
  for (int i = 0; i < a.nlit && f; ++i) {
    const double* nrm = a.normals + (size_t)i * ny;
    double s = 0.0;
    for (int j = 0; j < ny; ++j) {
      const double m = nrm[j] * a.Y[(size_t)p * ny + j];
      s = j ? s + m : m;
    }
    if (!(s > a.hs[i])) f = 0;
  }
  a.pflag[p] = f;
}

// ONE workgroup: the exclusive rank of every box among the level's open boxes, tile after tile with a carried offset, then the number
// of candidate points, then the status record
__global__ __launch_bounds__(256) void k_search_scan(SearchArgs a, long long npts) {
  __shared__ int s[256];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int t0 = 0; t0 < a.nb; t0 += 256) {
    const int b = t0 + tid;
    const int v = b < a.nb ? a.open[b] : 0;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int add = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    if (b < a.nb) a.slot[b] = carry + s[tid] - v;
    carry += s[255];
    __syncthreads();
  }
  int cnt = 0;
  for (long long p = tid; p < npts; p += 256) cnt += a.pflag[p];
  s[tid] = cnt;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) s[tid] += s[tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    a.status[0] = a.nb;
    a.status[1] = a.nb - carry;
    a.status[2] = carry;
    a.status[3] = s[0];
  }
}

// one thread per box: the r-th open box writes its children to slots 2r, 2r + 1 of the next frontier (children != 0), a proved box its
// row of the leaf log (its rank among the proved boxes is its position minus its rank among the open ones)
__global__ __launch_bounds__(256) void k_search_scatter(SearchArgs a, int children) {
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  const int n0 = a.n0, r = a.slot[b];
  const double* lo = a.lo + (size_t)b * n0;
  const double* hi = a.hi + (size_t)b * n0;
  if (!a.open[b]) {
    double* row = a.log + (size_t)(a.log_base + (b - r)) * (2 * n0 + 3);
    for (int t = 0; t < n0; ++t) { row[t] = lo[t]; row[n0 + t] = hi[t]; }
    row[2 * n0] = (double)a.depth;
    row[2 * n0 + 1] = (double)a.best[b];
    row[2 * n0 + 2] = a.bound[b];
    return;
  }
  const int j = a.coord[b];
  if (!children || j < 0) return;
  const double mid = 0.5 * (lo[j] + hi[j]);
  const size_t L = (size_t)(2 * (size_t)r) * n0, R = L + n0;
  for (int t = 0; t < n0; ++t) {
    const int cv = a.cuts[(size_t)b * n0 + t] + (t == j ? 1 : 0);
    a.nlo[L + t] = lo[t];
    a.nhi[L + t] = t == j ? mid : hi[t];
    a.nlo[R + t] = t == j ? mid : lo[t];
    a.nhi[R + t] = hi[t];
    a.ncuts[L + t] = cv;
    a.ncuts[R + t] = cv;
  }
}

}  // namespace nnsdp
