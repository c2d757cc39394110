// Device-resident frontier of the ReLU-split search (nnsdp_crown::search_nodes of crown_frontier_host.hpp; nnsdp_amd/relusplit.py with
// frontier = "device").  The level loop of relusplit.py (_levels) with the nodes kept in device memory: per level the host launches, per
// chunk of the level, the node kernels k_crown_nodes and k_crown_beta (csrc/crown_relu_split.hpp, unchanged, sp.assign offset into the
// frontier) and k_node_classify on the chunk's outputs; then k_forward_mfma on the level's points, k_node_refute, k_node_scan and
// k_node_scatter, and reads back the five integers of the status record.
//
// Frontier: int8 assignments, acdim x nnode column-major, the layout CrownSplit.assign reads.  Two of them: the level being bounded and
// the one its children are written to.  The box is the root's for every node: lo / hi of one chunk are written once (k_node_boxes).
// Per-level records, indexed by the node's position in the level: kind, best literal, its smax, the branching neuron, and the node's
// exclusive ranks among the level's closed, stuck and branching nodes.  Points: point 0 is the box centre, point 1 + b nlit + i the
// maximiser of literal i's linear bound on node b (corner_points).
// Logs: a closed node writes assignment, depth, kind and bound to the leaf log, a stuck node (open, no neuron to branch on) to the
// stuck log, both in level order and then node order, the order relusplit.py appends them.
//
// The arithmetic that decides anything restates numpy's operation for operation (contraction into FMA off): excess_i = smax_i - hs_i,
// the first minimum, c + sign(uA) r with the product and the sum rounded separately.  No atomics: the ranks come from a scan by one
// workgroup that walks the level in tiles of 256 with carried offsets (scan_tile), the candidate count from a tree reduction.
#pragma once
#include <hip/hip_runtime.h>

#include "crown_frontier.hpp"

namespace nnsdp {

static constexpr int kNodeInfeasible = 0, kNodeBound = 1, kNodeStuck = 2, kNodeBranching = 3;      // kinds; closed: < kNodeStuck
static constexpr int kNodeLanes = 32;       // lanes that copy one node's assignment in k_node_scatter

struct NodeSearchArgs {
  int n0, ny, nlit, acdim;
  int depth;                      // the level
  int corner_points;
  int nb;                         // nodes of the level
  int children;                   // 0: depth + 1 > max_depth; the scatter kernel never writes children then
  int visited, max_nodes;         // nodes bounded up to and including this level; children only if visited + 2 branching <= max_nodes
  const double* normals;          // ny x nlit column-major
  const double* hs;               // nlit
  const double *lo, *hi;          // the root box (the first node of the chunk's boxes)
  const int8_t* cur;              // the level's frontier
  int8_t* nxt;                    // the next frontier
  int *kind, *best, *neuron;      // records, nb each
  int *rclosed, *rstuck, *rbranch;
  double* bound;
  double* X;                      // n0 x points
  const double* Y;                // ny x points
  int* pflag;                     // per point: every literal false there and the node open (point 0: the centre, no node)
  int* status;                    // bounded, closed, stuck, branching, candidates
  int8_t* lassign;                // leaf log: acdim per row; this level's rows start at log_base
  int *ldepth, *lkind;
  double* lbound;
  long long log_base;
  int8_t* sassign;                // stuck log; this level's rows start at slog_base
  int* sdepth;
  double* sbound;
  long long slog_base;
};

// lo / hi of `count` nodes, n0 x count column-major: the root box in every column
__global__ __launch_bounds__(256) void k_node_boxes(const double* root_lo, const double* root_hi, int n0, long long count, double* lo, double* hi) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= count * n0) return;
  lo[k] = root_lo[k % n0];
  hi[k] = root_hi[k % n0];
}

// one thread per node of a chunk: nodes off .. off + nc - 1 of the level; smax / uA / branch / infeasible are the chunk's outputs of the
// node kernels (indexed by the node's position in the chunk).  Step 1 of the driver: the infeasible flag first, then the first minimum
// of smax_i - hs_i (numpy's argmin: a NaN is a minimum)
__global__ __launch_bounds__(256) void k_node_classify(NodeSearchArgs a, int off, int nc, const double* smax, const double* uA,
                                                       const double* branch, const double* infeasible) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const int b = off + c, n0 = a.n0, nlit = a.nlit;
  const bool inf = infeasible[c] != 0.0;
  int best = 0, kind = kNodeInfeasible, neuron = -1;
  double bound = __builtin_nan("");
  if (!inf) {
    double bexc = 0.0;
    for (int i = 0; i < nlit; ++i) {
      const double exc = smax[(size_t)c * nlit + i] - a.hs[i];
      if (i == 0 || exc < bexc || (exc != exc && bexc == bexc)) { best = i; bexc = exc; }
    }
    bound = smax[(size_t)c * nlit + best];
    neuron = (int)branch[(size_t)c * nlit + best];
    kind = bexc <= 0.0 ? kNodeBound : neuron < 0 ? kNodeStuck : kNodeBranching;
  }
  a.kind[b] = kind; a.best[b] = best; a.neuron[b] = neuron; a.bound[b] = bound;
  if (b == 0) frontier_centre(a.X, a.lo, a.hi, n0);
  // the points of a closed node are never looked at; they are written so that the forward pass reads defined numbers (an infeasible
  // node's linear bounds mean nothing: it gets the centre)
  if (a.corner_points)
    for (int i = 0; i < nlit; ++i) {
      double* x = a.X + (1 + (size_t)b * nlit + i) * n0;
      if (inf) frontier_centre(x, a.lo, a.hi, n0);
      else frontier_sign_corner(x, uA + ((size_t)c * nlit + i) * n0, a.lo, a.hi, n0);
    }
}

// one thread per point: the flag of  every literal false  at the centre or at a point of an open node
__global__ __launch_bounds__(256) void k_node_refute(NodeSearchArgs a, long long npts) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const bool open = p == 0 || a.kind[(int)((p - 1) / a.nlit)] >= kNodeStuck;
  a.pflag[p] = open && search_all_false(a.normals, a.hs, a.Y + (size_t)p * a.ny, a.nlit, a.ny);
}

// ONE workgroup: the exclusive ranks of every node among the level's closed, stuck and branching nodes, tile after tile with carried
// offsets; then the number of candidate points (none when no node is open: the driver looks at no point then); then the status record
__global__ __launch_bounds__(256) void k_node_scan(NodeSearchArgs a, long long npts) {
  __shared__ int s[3][kScanTile];
  const int tid = threadIdx.x, nb = a.nb;
  int carry[3] = {0, 0, 0};
  for (int t0 = 0; t0 < nb; t0 += kScanTile) {
    const int k = t0 + tid;
    const int kd = k < nb ? a.kind[k] : -1;
    const int c[3] = {kd >= 0 && kd < kNodeStuck ? 1 : 0, kd == kNodeStuck ? 1 : 0, kd == kNodeBranching ? 1 : 0};
    int v[3] = {c[0], c[1], c[2]};
    scan_tile<3>(s, tid, v);
    if (k < nb) {
      a.rclosed[k] = carry[0] + v[0] - c[0];
      a.rstuck[k] = carry[1] + v[1] - c[1];
      a.rbranch[k] = carry[2] + v[2] - c[2];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) carry[q] += s[q][kScanTile - 1];
    __syncthreads();
  }
  int cnt = 0;
  for (long long p = tid; p < npts; p += 256) cnt += a.pflag[p];
  s[0][tid] = cnt;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) s[0][tid] += s[0][tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    a.status[0] = nb;
    a.status[1] = carry[0];
    a.status[2] = carry[1];
    a.status[3] = carry[2];
    a.status[4] = carry[1] + carry[2] > 0 ? s[0][0] : 0;
  }
}

// kNodeLanes lanes per node: a closed node writes its row of the leaf log (assignment, depth, kind, bound), a stuck node its row of
// the stuck log, the r-th branching node its children 2r (the neuron forced +1) and 2r + 1 (-1) into the next frontier when the level's
// children fit the budget (the host applies the same rule to the status record it reads back).  Plain byte and dword stores
__global__ __launch_bounds__(256) void k_node_scatter(NodeSearchArgs a) {
  const int b = blockIdx.x * (256 / kNodeLanes) + threadIdx.x / kNodeLanes, lane = threadIdx.x % kNodeLanes;
  if (b >= a.nb) return;
  const int acdim = a.acdim, kd = a.kind[b];
  const int8_t* src = a.cur + (size_t)b * acdim;
  if (kd < kNodeStuck) {
    const size_t row = (size_t)(a.log_base + a.rclosed[b]);
    int8_t* dst = a.lassign + row * acdim;
    for (int j = lane; j < acdim; j += kNodeLanes) dst[j] = src[j];
    if (lane == 0) { a.ldepth[row] = a.depth; a.lkind[row] = kd; a.lbound[row] = a.bound[b]; }
    return;
  }
  if (kd == kNodeStuck) {
    const size_t row = (size_t)(a.slog_base + a.rstuck[b]);
    int8_t* dst = a.sassign + row * acdim;
    for (int j = lane; j < acdim; j += kNodeLanes) dst[j] = src[j];
    if (lane == 0) { a.sdepth[row] = a.depth; a.sbound[row] = a.bound[b]; }
    return;
  }
  if (!a.children || (long long)a.visited + 2LL * a.status[3] > (long long)a.max_nodes) return;
  const int n = a.neuron[b];
  int8_t* plus = a.nxt + 2 * (size_t)a.rbranch[b] * acdim;
  int8_t* minus = plus + acdim;
  for (int j = lane; j < acdim; j += kNodeLanes) {
    const int8_t v = src[j];
    plus[j] = j == n ? (int8_t)1 : v;
    minus[j] = j == n ? (int8_t)-1 : v;
  }
}

}  // namespace nnsdp
