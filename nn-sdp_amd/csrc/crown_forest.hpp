// Forest of device-resident bounds-only split searches (nnsdp_crown::search_many of crown_frontier_host.hpp; nnsdp_amd/split.py, verifySplitMany
// with frontier = "device"): R root boxes, one network, one set of literal normals, thresholds per root, decided by ONE level loop.
// Level d of every tree that is still active forms one frontier, so one pass of launches, one synchronisation and one read-back serve
// every root.  Per root the result is the one of the single search (csrc/crown_search.hpp) bit for bit: the kernels below call the
// pieces k_search_classify / k_search_refute / k_search_scatter call (csrc/crown_frontier.hpp: search_best, frontier_coord,
// search_all_false, frontier_bisect, frontier_log_row) with the thresholds and the splittable mask of the box's root.
//
// Frontier: lo, hi (doubles), cuts (ints), each n0 x nbox column-major, and one int per box: the root it belongs to (its index within
// the group of roots that share the buffers).  Two of them.  The boxes of a level are ordered by root, and within a root as the single
// search orders them, so a root owns one contiguous segment [seg, seg + len) of the level.  Its first nb boxes are bounded; the others
// are the ones its budget keeps from being bounded (they are bounded with the rest of the level and the result is thrown away).  The
// segment of a root that the host found violated one level earlier is dead: bounded, thrown away, no children, no leaves.
// Per-root records (indexed by root): thresholds (nlit), splittable mask, and per level seg, len, nb, flags (bit 0: the root's open
// boxes get children; bit 1: dead); the host, which owns visited / verdict / depth of every root, sends the level's table and
// k_forest_roots scatters it.
// Per-box records, indexed by the position in the level: state (1 open, 0 proved, -1 not bounded or dead), best literal, its bound,
// the split coordinate.  Points: the centres of the level's boxes, then (corner_points) their corners.
//
// Ranks: five counts per box (open; open in a root that continues; proved; candidate points; never bounded) are scanned together in
// three steps that kernel boundaries on the stream order: k_forest_scan_block (256 boxes per workgroup: exclusive ranks within the
// block, the block's totals; scan_tile on five rows), k_forest_scan_totals (one workgroup turns the block totals into block offsets, tile
// after tile with a carried offset, scan_walk, and appends the grand totals), and the sum of both wherever a rank is read
// (forest_rank).  No atomics, no flags and no waiting between workgroups.  Because a root's segment is contiguous, the rank among "open boxes of roots that continue" gives
// every root a contiguous segment of the next level (children at 2 rank, 2 rank + 1), and a root's counts are rank differences at
// the ends of its segment (k_forest_counts: three ints per active root, all the host reads back per level).
// Leaf logs, rows of 2 n0 + 4 doubles (lo, hi, depth, literal, bound, root): the proved boxes in level order; and the boxes that end a
// root which does not continue (its never bounded boxes, literal -1, and its open boxes).
#pragma once
#include <hip/hip_runtime.h>
#include "crown_search.hpp"

namespace nnsdp {

// the longest level the hierarchical scan is used on: 2^18 blocks of 256 boxes, whose totals the single workgroup of
// k_forest_scan_totals walks in 1024 tiles.  No buffer of a group within kSearchFrontierCap holds more boxes (a box of the two frontiers
// takes at least 48 bytes), so the rule below groups around it and it is never the reason of a refusal
static constexpr size_t kForestMaxLevel = (size_t)1 << 26;
static constexpr int kForestScanBlock = kScanTile;
static constexpr int kForestCounts = 5;      // open, open and continuing, proved, candidates, never bounded
enum { kFoOpen = 0, kFoCont = 1, kFoProved = 2, kFoCand = 3, kFoUnb = 4 };

// The buffers of one group of `group` roots, in one place: the level capacity, the element offsets and the byte counts that the cap
// (kSearchFrontierCap) applies to.  Host only.
struct ForestPlan {
  size_t group = 0, mb = 0, cap = 0, npmax = 0, nblk = 0, logw = 0;
  // doubles: masks (as 64-bit words), thresholds, normals, bound, points in, points out, proved log, end log
  size_t o_mask = 0, o_hs = 0, o_nrm = 0, o_bound = 0, o_X = 0, o_Y = 0, o_log = 0, o_elog = 0, nd = 0;
  // ints: seg, len, nb, flags, act, the level's table as sent (5 per root), counts (3 per root), state, best, coord, point flags,
  // ranks within the block (5 per box), block offsets (5 per block and the totals)
  size_t o_seg = 0, o_len = 0, o_nb = 0, o_flags = 0, o_act = 0, o_tab = 0, o_cnt = 0, o_open = 0, o_best = 0, o_coord = 0, o_pflag = 0,
         o_pre = 0, o_bt = 0, ni = 0;
  size_t frontier_bytes = 0, double_bytes = 0, int_bytes = 0;
  bool fits() const {
    return cap <= kForestMaxLevel && frontier_bytes <= kSearchFrontierCap && double_bytes <= kSearchFrontierCap && int_bytes <= kSearchFrontierCap;
  }
};

inline ForestPlan forest_plan(size_t n0, size_t ny, size_t nlit, size_t max_boxes, bool corner_points, size_t group) {
  ForestPlan p;
  p.group = group; p.mb = max_boxes;
  p.cap = 2 * max_boxes * group;      // a root's level bounds at most max_boxes boxes and its children number at most twice that
  p.npmax = corner_points ? 2 * p.cap : p.cap;
  p.nblk = (p.cap + kForestScanBlock - 1) / kForestScanBlock;
  p.logw = 2 * n0 + 4;
  p.o_mask = 0; p.o_hs = p.o_mask + group; p.o_nrm = p.o_hs + nlit * group; p.o_bound = p.o_nrm + nlit * ny; p.o_X = p.o_bound + p.cap;
  p.o_Y = p.o_X + p.npmax * n0; p.o_log = p.o_Y + p.npmax * ny; p.o_elog = p.o_log + max_boxes * group * p.logw;
  p.nd = p.o_elog + p.cap * p.logw;
  p.o_seg = 0; p.o_len = p.o_seg + group; p.o_nb = p.o_len + group; p.o_flags = p.o_nb + group; p.o_act = p.o_flags + group;
  p.o_tab = p.o_act + group; p.o_cnt = p.o_tab + 5 * group; p.o_open = p.o_cnt + 3 * group; p.o_best = p.o_open + p.cap;
  p.o_coord = p.o_best + p.cap; p.o_pflag = p.o_coord + p.cap; p.o_pre = p.o_pflag + p.npmax; p.o_bt = p.o_pre + kForestCounts * p.cap;
  p.ni = p.o_bt + kForestCounts * (p.nblk + 1);
  // two frontiers: lo, hi, cuts per coordinate and the root per box
  p.frontier_bytes = 2 * p.cap * (n0 * (2 * sizeof(double) + sizeof(int)) + sizeof(int));
  p.double_bytes = p.nd * sizeof(double);
  p.int_bytes = p.ni * sizeof(int);
  return p;
}

// the roots per group: the most (at most `limit`, >= 1) whose buffers all stay within the cap; 0 when one root alone does not fit
inline size_t forest_group(size_t n0, size_t ny, size_t nlit, size_t max_boxes, bool corner_points, size_t limit) {
  if (!forest_plan(n0, ny, nlit, max_boxes, corner_points, 1).fits()) return 0;
  size_t lo = 1, hi = limit;      // every size grows with the group, so the groups that fit are 1 .. some G
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (forest_plan(n0, ny, nlit, max_boxes, corner_points, mid).fits()) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct ForestArgs {
  FrontierArgs f;                 // nlit: literals of the clause; X: n0 x (nl or 2 nl); log: the proved log
  int nl;                         // boxes of the level (all of them are bounded; a root's first nb count)
  int literal_bounds;
  int nblk;                       // blocks of the scan: ceil(nl / 256)
  const double* hs;               // nlit x group column-major
  const unsigned long long* mask; // per root, bit t: root_hi[t] > root_lo[t]
  int *seg, *len, *nb, *flags;    // per root: the level's table
  int* act;                       // per entry of the level's table: its root
  const int* tab;                 // the table as the host sent it: root, seg, len, nb, flags per entry
  int* counts;                    // per entry: proved, open, candidates
  const int* root;                // per box of the level's frontier: its root
  int* nroot;                     // the same of the next frontier
  int *open, *best, *coord;       // records, nl each
  double* bound;
  int* pflag;                     // per point: every literal false there and the box open
  int* pre;                       // kForestCounts x pre_stride: exclusive ranks within the box's block
  int* bt;                        // kForestCounts x (bt_stride): block totals, then block offsets and, at nblk, the grand totals
  long long pre_stride, bt_stride;
  double* elog;                   // the end log; this level's rows start at elog_base
  long long elog_base;
};

// the exclusive rank of box b of the level in count q (b == nl: the total), from the two levels of the scan
__device__ __forceinline__ int forest_rank(const ForestArgs& a, int q, int b) {
  const int* bt = a.bt + (size_t)q * a.bt_stride;
  if (b >= a.nl) return bt[a.nblk];
  return a.pre[(size_t)q * a.pre_stride + b] + bt[b / kForestScanBlock];
}

// one thread per entry of the level's table
__global__ __launch_bounds__(256) void k_forest_roots(ForestArgs a, int nent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nent) return;
  const int* t = a.tab + (size_t)5 * i;
  const int r = t[0];
  a.act[i] = r;
  a.seg[r] = t[1]; a.len[r] = t[2]; a.nb[r] = t[3]; a.flags[r] = t[4];
}

// k_search_classify with the thresholds and the mask of the box's root; one thread per box of a chunk: boxes off .. off + nc - 1 of the
// level; ymin / ymax / smax / uA are the chunk's outputs of the bound kernel (indexed by the box's position in the chunk)
__global__ __launch_bounds__(256) void k_forest_classify(ForestArgs a, int off, int nc, const double* ymin, const double* ymax,
                                                         const double* smax, const double* uA) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const FrontierArgs& f = a.f;
  const int b = off + c, n0 = f.n0, ny = f.ny;
  const int r = a.root[b];
  const bool live = b - a.seg[r] < a.nb[r];
  const BestLiteral q = search_best(f.normals, a.hs + (size_t)r * f.nlit, ymin + (size_t)c * ny, ymax + (size_t)c * ny,
                                    smax + (size_t)c * f.nlit, f.nlit, ny, a.literal_bounds);
  a.open[b] = !live ? -1 : q.bexc <= 0.0 ? 0 : 1;
  a.best[b] = q.best;
  a.coord[b] = frontier_coord(f.cuts + (size_t)b * n0, n0, a.mask[r]);
  a.bound[b] = q.bcheap;
  // the points of a box that is not open are never looked at; they are written so that the forward pass reads defined numbers
  frontier_centre(f.X + (size_t)b * n0, f.lo + (size_t)b * n0, f.hi + (size_t)b * n0, n0);
  if (f.corner_points)
    frontier_corner(f.X + ((size_t)a.nl + b) * n0, uA + ((size_t)c * f.nlit + q.best) * n0, f.lo + (size_t)b * n0, f.hi + (size_t)b * n0, n0);
}

// k_search_refute with the thresholds of the box's root; one thread per point
__global__ __launch_bounds__(256) void k_forest_refute(ForestArgs a, long long npts) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const FrontierArgs& f = a.f;
  const int b = (int)(p % a.nl);
  a.pflag[p] = a.open[b] == 1 && search_all_false(f.normals, a.hs + (size_t)a.root[b] * f.nlit, f.Y + (size_t)p * f.ny, f.nlit, f.ny);
}

// first step of the scan, one workgroup per 256 boxes: the exclusive ranks of the five counts within the block and the block's totals
__global__ __launch_bounds__(256) void k_forest_scan_block(ForestArgs a) {
  __shared__ int s[kForestCounts][kForestScanBlock];
  const int tid = threadIdx.x, b = blockIdx.x * kForestScanBlock + tid;
  int v[kForestCounts] = {0, 0, 0, 0, 0};
  if (b < a.nl) {
    const int op = a.open[b], fl = a.flags[a.root[b]];
    v[kFoOpen] = op == 1;
    v[kFoCont] = op == 1 && (fl & 1);
    v[kFoProved] = op == 0;
    v[kFoCand] = a.pflag[b] + (a.f.corner_points ? a.pflag[(size_t)a.nl + b] : 0);
    v[kFoUnb] = op < 0 && !(fl & 2);
  }
  int incl[kForestCounts];
#pragma unroll
  for (int q = 0; q < kForestCounts; ++q) incl[q] = v[q];
  scan_tile<kForestCounts>(s, tid, incl);
#pragma unroll
  for (int q = 0; q < kForestCounts; ++q) {
    if (b < a.nl) a.pre[(size_t)q * a.pre_stride + b] = incl[q] - v[q];
    if (tid == kForestScanBlock - 1) a.bt[(size_t)q * a.bt_stride + blockIdx.x] = incl[q];
  }
}

// second step, ONE workgroup: the block totals become exclusive block offsets (scan_walk); entry nblk gets the grand total
__global__ __launch_bounds__(256) void k_forest_scan_totals(ForestArgs a) {
  __shared__ int s[1][kScanTile];
  for (int q = 0; q < kForestCounts; ++q) {
    int* bt = a.bt + (size_t)q * a.bt_stride;
    const int total = scan_walk(s, threadIdx.x, bt, bt, a.nblk);
    if (threadIdx.x == 0) bt[a.nblk] = total;
  }
}

// one thread per entry of the level's table: the root's proved boxes, open boxes and candidate points
__global__ __launch_bounds__(256) void k_forest_counts(ForestArgs a, int nent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nent) return;
  const int r = a.act[i], s = a.seg[r], e = s + a.len[r];
  a.counts[3 * i] = forest_rank(a, kFoProved, e) - forest_rank(a, kFoProved, s);
  a.counts[3 * i + 1] = forest_rank(a, kFoOpen, e) - forest_rank(a, kFoOpen, s);
  a.counts[3 * i + 2] = forest_rank(a, kFoCand, e) - forest_rank(a, kFoCand, s);
}

// a row of either leaf log: lo, hi, depth (frontier_log_row), then literal, bound, root
__device__ __forceinline__ void forest_log_row(const FrontierArgs& f, double* log, long long row, int b, int literal, double bound, int root) {
  double* tail = frontier_log_row(f, log, row, 2 * (size_t)f.n0 + 4, b);
  tail[0] = (double)literal;
  tail[1] = bound;
  tail[2] = (double)root;
}

// one thread per box: a proved box writes its row of the proved log; an open box of a root that continues writes its children and
// their root to slots 2 rank, 2 rank + 1 of the next frontier (frontier_bisect); the never bounded and the open boxes of a
// root that ends here write their rows of the end log; the boxes of a dead segment write nothing
__global__ __launch_bounds__(256) void k_forest_scatter(ForestArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nl) return;
  const FrontierArgs& f = a.f;
  const int op = a.open[b], r = a.root[b], fl = a.flags[r];
  if (op == 0) {
    forest_log_row(f, f.log, f.log_base + forest_rank(a, kFoProved, b), b, a.best[b], a.bound[b], r);
    return;
  }
  if (fl & 2) return;
  if (op < 0 || !(fl & 1)) {
    const int e = forest_rank(a, kFoUnb, b) + forest_rank(a, kFoOpen, b) - forest_rank(a, kFoCont, b);
    forest_log_row(f, a.elog, a.elog_base + e, b, op < 0 ? -1 : a.best[b], op < 0 ? 0.0 : a.bound[b], r);
    return;
  }
  const int j = a.coord[b];
  if (j < 0) return;
  const size_t k = 2 * (size_t)forest_rank(a, kFoCont, b);
  frontier_bisect(f, b, j, k);
  a.nroot[k] = r;
  a.nroot[k + 1] = r;
}

}  // namespace nnsdp
