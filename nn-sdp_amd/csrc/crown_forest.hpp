// Forest of device-resident bounds-only split searches (nnsdp_crown::search_many of crown_handle.hpp; nnsdp_amd/split.py, verifySplitMany
// with frontier = "device"): R root boxes, one network, one set of literal normals, thresholds per root, decided by ONE level loop.
// Level d of every tree that is still active forms one frontier, so one pass of launches, one synchronisation and one read-back serve
// every root.  Per root the result is the one of the single search (csrc/crown_search.hpp) bit for bit: the arithmetic below restates
// k_search_classify / k_search_refute / k_search_scatter with the thresholds and the splittable mask of the box's root.
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
// block, the block's totals), k_forest_scan_totals (one workgroup turns the block totals into block offsets, tile after tile with a
// carried offset, and appends the grand totals), and the sum of both wherever a rank is read (forest_rank).  No atomics, no flags and
// no waiting between workgroups.  Because a root's segment is contiguous, the rank among "open boxes of roots that continue" gives
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
static constexpr int kForestScanBlock = 256;
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
  int n0, ny, nlit;
  int nl;                         // boxes of the level (all of them are bounded; a root's first nb count)
  int depth;                      // the level
  int literal_bounds, corner_points;
  int nblk;                       // blocks of the scan: ceil(nl / 256)
  const double* normals;          // ny x nlit column-major
  const double* hs;               // nlit x group column-major
  const unsigned long long* mask; // per root, bit t: root_hi[t] > root_lo[t]
  int *seg, *len, *nb, *flags;    // per root: the level's table
  int* act;                       // per entry of the level's table: its root
  const int* tab;                 // the table as the host sent it: root, seg, len, nb, flags per entry
  int* counts;                    // per entry: proved, open, candidates
  const double *lo, *hi;          // the level's frontier
  const int *cuts, *root;
  double *nlo, *nhi;              // the next frontier
  int *ncuts, *nroot;
  int *open, *best, *coord;       // records, nl each
  double* bound;
  double* X;                      // n0 x (nl or 2 nl): centres, then corners
  const double* Y;                // ny x (points)
  int* pflag;                     // per point: every literal false there and the box open
  int* pre;                       // kForestCounts x pre_stride: exclusive ranks within the box's block
  int* bt;                        // kForestCounts x (bt_stride): block totals, then block offsets and, at nblk, the grand totals
  long long pre_stride, bt_stride;
  double *log, *elog;             // leaf logs; this level's rows start at log_base / elog_base
  long long log_base, elog_base;
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
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const int b = off + c, n0 = a.n0, ny = a.ny;
  const int r = a.root[b];
  const bool live = b - a.seg[r] < a.nb[r];
  const double* hs = a.hs + (size_t)r * a.nlit;
  const unsigned long long mask = a.mask[r];
  int best = 0;
  double bexc = 0.0, bcheap = 0.0;
  for (int i = 0; i < a.nlit; ++i) {
    const double* nrm = a.normals + (size_t)i * ny;
    double cheap = search_cheap(nrm, ymin + (size_t)c * ny, ymax + (size_t)c * ny, ny);
    if (a.literal_bounds) {
      const double s = smax[(size_t)c * a.nlit + i];
      cheap = cheap <= s ? cheap : s;
    }
    const double exc = cheap - hs[i];
    if (i == 0 || exc < bexc) { best = i; bexc = exc; bcheap = cheap; }
  }
  const int open = !live ? -1 : bexc <= 0.0 ? 0 : 1;
  int coord = -1, cmin = 0;
  for (int t = 0; t < n0; ++t)
    if ((mask >> t) & 1ull) {
      const int v = a.cuts[(size_t)b * n0 + t];
      if (coord < 0 || v < cmin) { coord = t; cmin = v; }
    }
  a.open[b] = open;
  a.best[b] = best;
  a.coord[b] = coord;
  a.bound[b] = bcheap;
  // the points of a box that is not open are never looked at; they are written so that the forward pass reads defined numbers
  const double* A = a.corner_points ? uA + ((size_t)c * a.nlit + best) * n0 : nullptr;
  for (int t = 0; t < n0; ++t) {
    const double l = a.lo[(size_t)b * n0 + t], u = a.hi[(size_t)b * n0 + t];
    a.X[(size_t)b * n0 + t] = 0.5 * (l + u);
    if (a.corner_points) a.X[((size_t)a.nl + b) * n0 + t] = A[t] >= 0.0 ? u : l;
  }
}

// k_search_refute with the thresholds of the box's root; one thread per point
__global__ __launch_bounds__(256) void k_forest_refute(ForestArgs a, long long npts) {
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const int b = (int)(p % a.nl), ny = a.ny;
  const double* hs = a.hs + (size_t)a.root[b] * a.nlit;
  int f = a.open[b] == 1 ? 1 : 0;
  for (int i = 0; i < a.nlit && f; ++i) {
    const double* nrm = a.normals + (size_t)i * ny;
    double s = 0.0;
    for (int j = 0; j < ny; ++j) {
      const double m = nrm[j] * a.Y[(size_t)p * ny + j];
      s = j ? s + m : m;
    }
    if (!(s > hs[i])) f = 0;
  }
  a.pflag[p] = f;
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
    v[kFoCand] = a.pflag[b] + (a.corner_points ? a.pflag[(size_t)a.nl + b] : 0);
    v[kFoUnb] = op < 0 && !(fl & 2);
  }
#pragma unroll
  for (int q = 0; q < kForestCounts; ++q) s[q][tid] = v[q];
  __syncthreads();
  for (int d = 1; d < kForestScanBlock; d <<= 1) {
    int add[kForestCounts];
#pragma unroll
    for (int q = 0; q < kForestCounts; ++q) add[q] = tid >= d ? s[q][tid - d] : 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kForestCounts; ++q) s[q][tid] += add[q];
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kForestCounts; ++q) {
    if (b < a.nl) a.pre[(size_t)q * a.pre_stride + b] = s[q][tid] - v[q];
    if (tid == kForestScanBlock - 1) a.bt[(size_t)q * a.bt_stride + blockIdx.x] = s[q][tid];
  }
}

// second step, ONE workgroup: the block totals become exclusive block offsets, tile after tile with a carried offset; entry nblk gets
// the grand total
__global__ __launch_bounds__(256) void k_forest_scan_totals(ForestArgs a) {
  __shared__ int s[256];
  const int tid = threadIdx.x;
  for (int q = 0; q < kForestCounts; ++q) {
    int* bt = a.bt + (size_t)q * a.bt_stride;
    int carry = 0;
    for (int t0 = 0; t0 < a.nblk; t0 += 256) {
      const int k = t0 + tid;
      const int v = k < a.nblk ? bt[k] : 0;
      s[tid] = v;
      __syncthreads();
      for (int d = 1; d < 256; d <<= 1) {
        const int add = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
      }
      if (k < a.nblk) bt[k] = carry + s[tid] - v;
      carry += s[255];
      __syncthreads();
    }
    if (tid == 0) bt[a.nblk] = carry;
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

__device__ __forceinline__ void forest_log_row(double* row, int n0, const double* lo, const double* hi, int depth, int literal, double bound, int root) {
  for (int t = 0; t < n0; ++t) { row[t] = lo[t]; row[n0 + t] = hi[t]; }
  row[2 * n0] = (double)depth;
  row[2 * n0 + 1] = (double)literal;
  row[2 * n0 + 2] = bound;
  row[2 * n0 + 3] = (double)root;
}

// one thread per box: a proved box writes its row of the proved log; an open box of a root that continues writes its children and
// their root to slots 2 rank, 2 rank + 1 of the next frontier (k_search_scatter's bisection); the never bounded and the open boxes of a
// root that ends here write their rows of the end log; the boxes of a dead segment write nothing
__global__ __launch_bounds__(256) void k_forest_scatter(ForestArgs a) {
#pragma clang fp contract(off)      // numpy rounds every product and every sum
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nl) return;
  const int n0 = a.n0, op = a.open[b], r = a.root[b], fl = a.flags[r];
  const double* lo = a.lo + (size_t)b * n0;
  const double* hi = a.hi + (size_t)b * n0;
  const size_t logw = 2 * (size_t)n0 + 4;
  if (op == 0) {
    forest_log_row(a.log + (size_t)(a.log_base + forest_rank(a, kFoProved, b)) * logw, n0, lo, hi, a.depth, a.best[b], a.bound[b], r);
    return;
  }
  if (fl & 2) return;
  if (op < 0 || !(fl & 1)) {
    const int e = forest_rank(a, kFoUnb, b) + forest_rank(a, kFoOpen, b) - forest_rank(a, kFoCont, b);
    forest_log_row(a.elog + (size_t)(a.elog_base + e) * logw, n0, lo, hi, a.depth, op < 0 ? -1 : a.best[b], op < 0 ? 0.0 : a.bound[b], r);
    return;
  }
  const int j = a.coord[b];
  if (j < 0) return;
  const double mid = 0.5 * (lo[j] + hi[j]);
  const size_t k = 2 * (size_t)forest_rank(a, kFoCont, b);
  const size_t L = k * n0, R = L + n0;
  for (int t = 0; t < n0; ++t) {
    const int cv = a.cuts[(size_t)b * n0 + t] + (t == j ? 1 : 0);
    a.nlo[L + t] = lo[t];
    a.nhi[L + t] = t == j ? mid : hi[t];
    a.nlo[R + t] = t == j ? mid : lo[t];
    a.nhi[R + t] = hi[t];
    a.ncuts[L + t] = cv;
    a.ncuts[R + t] = cv;
  }
  a.nroot[k] = r;
  a.nroot[k + 1] = r;
}

}  // namespace nnsdp
