// Device-resident frontier of the bounds-only split search (nnsdp_crown::search of crown_frontier_host.hpp; nnsdp_amd/split.py with frontier = "device").
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
// The arithmetic that decides anything restates numpy's operation for operation, so that the tree is the Python loop's bit for bit.  It
// is stated once, in csrc/crown_frontier.hpp, for this search, the reach search and the forest: products and sums are rounded
// separately (every helper there switches contraction into FMA off for itself), the proof test's sum has the order of numpy's pairwise
// routine (search_cheap), minima keep the first of equal values.  No atomics: the ranks come from a scan by one workgroup that walks
// the level in tiles of 256 with a carried offset (scan_walk), the candidate count from a tree reduction of per-thread counts.
#pragma once
#include <hip/hip_runtime.h>

#include "crown_frontier.hpp"

namespace nnsdp {

struct SearchArgs {
  FrontierArgs f;                 // nlit: literals of the clause; X: n0 x (nb or 2 nb)
  int nb;                         // boxes of the level that are bounded (the first nb of the frontier)
  int literal_bounds;
  unsigned long long splitmask;   // bit t: root_hi[t] > root_lo[t]
  const double* hs;               // nlit
  int *open, *best, *coord, *slot;      // records, nb each
  double* bound;
  int* pflag;                     // per point: every literal false there and the box open
  int* status;                    // bounded, proved, open, candidates
};

// one thread per box of a chunk: boxes off .. off + nc - 1 of the level; ymin / ymax / smax / uA are the chunk's outputs of the bound
// kernel (indexed by the box's position in the chunk)
__global__ __launch_bounds__(256) void k_search_classify(SearchArgs a, int off, int nc, const double* ymin, const double* ymax,
                                                         const double* smax, const double* uA) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const FrontierArgs& f = a.f;
  const int b = off + c, n0 = f.n0, ny = f.ny;
  const BestLiteral r = search_best(f.normals, a.hs, ymin + (size_t)c * ny, ymax + (size_t)c * ny, smax + (size_t)c * f.nlit, f.nlit, ny,
                                    a.literal_bounds);
  a.open[b] = r.bexc <= 0.0 ? 0 : 1;
  a.best[b] = r.best;
  a.coord[b] = frontier_coord(f.cuts + (size_t)b * n0, n0, a.splitmask);
  a.bound[b] = r.bcheap;
  // the points of a proved box are never looked at; they are written so that the forward pass reads defined numbers
  frontier_centre(f.X + (size_t)b * n0, f.lo + (size_t)b * n0, f.hi + (size_t)b * n0, n0);
  if (f.corner_points)
    frontier_corner(f.X + ((size_t)a.nb + b) * n0, uA + ((size_t)c * f.nlit + r.best) * n0, f.lo + (size_t)b * n0, f.hi + (size_t)b * n0, n0);
}

// one thread per point: the flag of  every literal false  at a point of an open box
__global__ __launch_bounds__(256) void k_search_refute(SearchArgs a, long long npts) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const FrontierArgs& f = a.f;
  a.pflag[p] = a.open[(int)(p % a.nb)] && search_all_false(f.normals, a.hs, f.Y + (size_t)p * f.ny, f.nlit, f.ny);
}

// ONE workgroup: the exclusive rank (slot) of every box among the nb boxes' open ones, tile after tile with a carried offset, then the
// number of candidate points (the sum of pflag over npts points; npts == 0: pflag is not read and may be null), then the status record
__global__ __launch_bounds__(256) void k_search_scan(const int* open, int nb, int* slot, const int* pflag, long long npts, int* status) {
  __shared__ int s[1][kScanTile];
  const int tid = threadIdx.x;
  const int carry = scan_walk(s, tid, open, slot, nb);
  int cnt = 0;
  for (long long p = tid; p < npts; p += 256) cnt += pflag[p];
  s[0][tid] = cnt;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) s[0][tid] += s[0][tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    status[0] = nb;
    status[1] = nb - carry;
    status[2] = carry;
    status[3] = s[0][0];
  }
}

// one thread per box: the r-th open box writes its children to slots 2r, 2r + 1 of the next frontier (children != 0), a proved box its
// row of the leaf log: lo, hi, depth, literal, bound (its rank among the proved boxes is its position minus its rank among the open ones)
__global__ __launch_bounds__(256) void k_search_scatter(SearchArgs a, int children) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  const FrontierArgs& f = a.f;
  const int r = a.slot[b];
  if (!a.open[b]) {
    double* tail = frontier_log_row(f, f.log, f.log_base + (b - r), 2 * (size_t)f.n0 + 3, b);
    tail[0] = (double)a.best[b];
    tail[1] = a.bound[b];
    return;
  }
  const int j = a.coord[b];
  if (children && j >= 0) frontier_bisect(f, b, j, 2 * (size_t)r);
}

}  // namespace nnsdp
