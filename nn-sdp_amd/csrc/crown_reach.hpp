// Device-resident frontier of the reach search (nnsdp_crown::reach of crown_frontier_host.hpp; nnsdp_amd/split.py, reachSplit with frontier =
// "device"): branch and bound with an incumbent that encloses the support values  max_x c_i' f(x)  of every direction c_i of the handle
// on ONE bisection tree.  The level loop of split.py (_reach_levels) with the boxes, the incumbents and the leaf log in device memory:
// per level the host launches, per chunk of the level, the handle's bound kernel (k_crown_resident, csrc/crown_batch.hpp) and
// k_reach_points on the chunk's outputs; then k_forward_mfma on the level's points, k_reach_incumbent, k_reach_classify, k_search_scan
// (csrc/crown_search.hpp, with no points to count) and k_reach_scatter, and reads back the four integers of the status record.
//
// Frontier: lo, hi (doubles) and cuts (ints), each n0 x nbox column-major, two of them (the level and its children), as in the search.
// Per-level records, by the box's position in the level: ub (nlit x nb column-major: the bounds of every direction), the open flag, the
// split coordinate, the rank among the open boxes.  Points (n0 x npts): the centres in box order, then (corner_points) for direction
// 0, 1, ... the corner  where(A[i, :, b] >= 0, hi, lo)  of every box in box order: point (1 + i) nb + b.
// Incumbent state, nlit each: L (the largest c_i' f(point) so far), thr = L + tol, and the point xw (n0 x nlit column-major).
// Leaf log: one row of 2 n0 + 1 + nlit doubles per closed box, in the order split.py appends them: lo, hi, depth, ub[:, b].
//
// As in the search, whatever decides anything restates numpy operation for operation, so the tree is the Python loop's bit for bit; the
// arithmetic is the search's, stated once in csrc/crown_frontier.hpp (products and sums rounded separately: its helpers switch
// contraction off for themselves).  The maximum of a direction over the level's points is numpy's argmax, the FIRST of equal values:
// (value, index) pairs are combined by "greater value, or equal value and smaller index", which is associative and commutative, so the
// order of the per-thread walk, the cross-lane steps and the LDS tree does not matter.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "crown_search.hpp"

namespace nnsdp {

struct ReachArgs {
  FrontierArgs f;                 // nlit: directions; X: n0 x npts
  int nb;                         // boxes of the level
  int children;                   // 0: depth >= max_depth or nothing splittable; the scatter kernel never writes children then
  int visited, max_boxes;         // boxes bounded up to and including this level; children only if visited + 2 open <= max_boxes
  unsigned long long splitmask;   // bit t: root_hi[t] > root_lo[t]
  const double* tol;              // nlit
  int *open, *coord, *slot;       // records, nb each
  double* ub;                     // nlit x nb
  double *L, *thr, *xw;           // incumbents
  const int* status;              // k_search_scan's record: bounded, closed, open, 0
};

// one thread per box of a chunk: boxes off .. off + nc - 1 of the level; ymin / ymax / smax / uA are the chunk's outputs of the bound
// kernel (indexed by the box's position in the chunk).  ub[i, b] = min(cheap_i, smax_i), the centre and the corners of the box
__global__ __launch_bounds__(256) void k_reach_points(ReachArgs a, int off, int nc, const double* ymin, const double* ymax,
                                                      const double* smax, const double* uA) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const FrontierArgs& f = a.f;
  const int b = off + c, n0 = f.n0, ny = f.ny, nlit = f.nlit;
  for (int i = 0; i < nlit; ++i)
    a.ub[(size_t)b * nlit + i] = search_literal(f.normals + (size_t)i * ny, ymin + (size_t)c * ny, ymax + (size_t)c * ny, ny, smax + (size_t)c * nlit + i);
  const double* lo = f.lo + (size_t)b * n0;
  const double* hi = f.hi + (size_t)b * n0;
  frontier_centre(f.X + (size_t)b * n0, lo, hi, n0);
  if (f.corner_points)
    for (int i = 0; i < nlit; ++i) frontier_corner(f.X + ((size_t)(1 + i) * a.nb + b) * n0, uA + ((size_t)c * nlit + i) * n0, lo, hi, n0);
}

// (v, p) <- the better of (v, p) and (w, q): greater value, or equal value and smaller index
__device__ __forceinline__ void reach_take(double& v, long long& p, double w, long long q) {
  if (w > v || (w == v && q < p)) { v = w; p = q; }
}

// ONE workgroup per direction: s[i, p] = c_i' Y[:, p] (frontier_dot); the first maximum over the level's points; L_i, x_i are replaced
// when it is greater than L_i; thr_i = L_i + tol_i.  A thread that saw no point carries (-inf, LLONG_MAX)
__global__ __launch_bounds__(256) void k_reach_incumbent(ReachArgs a, long long npts) {
#pragma clang fp contract(off)      // numpy rounds every sum (L + tol below)
  __shared__ double sv[4];
  __shared__ long long sp[4];
  const FrontierArgs& f = a.f;
  const int i = blockIdx.x, tid = threadIdx.x, ny = f.ny;
  const double* nrm = f.normals + (size_t)i * ny;
  double v = -__builtin_inf();
  long long p = 0x7fffffffffffffffLL;
  for (long long q = tid; q < npts; q += 256) reach_take(v, p, frontier_dot(nrm, f.Y + (size_t)q * ny, ny), q);
  // wave64: six cross-lane steps; every lane takes part in every step (no divergence around __shfl_down)
  for (int d = 32; d > 0; d >>= 1) {
    const double w = __shfl_down(v, d, 64);
    const long long q = __shfl_down(p, d, 64);
    reach_take(v, p, w, q);
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = v; sp[tid >> 6] = p; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) reach_take(v, p, sv[w], sp[w]);
    double L = a.L[i];
    if (npts > 0 && v > L) {
      L = v;
      a.L[i] = v;
      for (int t = 0; t < f.n0; ++t) a.xw[(size_t)i * f.n0 + t] = f.X[(size_t)p * f.n0 + t];
    }
    a.thr[i] = L + a.tol[i];
  }
}

// one thread per box: open when some direction's bound is above its threshold; the split coordinate
__global__ __launch_bounds__(256) void k_reach_classify(ReachArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  const FrontierArgs& f = a.f;
  int open = 0;
  for (int i = 0; i < f.nlit; ++i)
    if (a.ub[(size_t)b * f.nlit + i] > a.thr[i]) open = 1;
  a.open[b] = open;
  a.coord[b] = frontier_coord(f.cuts + (size_t)b * f.n0, f.n0, a.splitmask);
}

// one thread per box: a closed box writes its row of the leaf log: lo, hi, depth, ub[:, b] (its rank among the closed boxes is its
// position minus its rank among the open ones); the r-th open box writes its children to slots 2r, 2r + 1 of the next frontier when the
// level's children fit the budget (the host applies the same rule to the status record it reads back)
__global__ __launch_bounds__(256) void k_reach_scatter(ReachArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  const FrontierArgs& f = a.f;
  const int nlit = f.nlit, r = a.slot[b];
  if (!a.open[b]) {
    double* tail = frontier_log_row(f, f.log, f.log_base + (b - r), 2 * (size_t)f.n0 + 1 + nlit, b);
    for (int i = 0; i < nlit; ++i) tail[i] = a.ub[(size_t)b * nlit + i];
    return;
  }
  const int j = a.coord[b];
  const long long nopen = a.status[2];
  if (a.children && j >= 0 && (long long)a.visited + 2 * nopen <= (long long)a.max_boxes) frontier_bisect(f, b, j, 2 * (size_t)r);
}

}  // namespace nnsdp
