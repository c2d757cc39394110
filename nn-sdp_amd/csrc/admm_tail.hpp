// The ADMM iteration behind the projection - gather, A' product, M^-1 product, A product, multiplier update - and the check
// iteration's residual kernels: the argument block (IterArgs; nnsdp_solver::iter_args() is its one binding to a solver's state), the
// kernels, the block counts (TailGrid) and one launch function per stage and form.  A stage's arithmetic is a *_body function; its
// single-SDP kernel takes the operands as a scalar list, which the launch function unpacks from the IterArgs (by value the 280-byte
// block measured outside the timing rule, profiles/admm_tail_refactor_timing.md), its batch kernel (`_b`) reads the IterArgs from a
// device table at blockIdx.y; the check kernels, one launch in check_every iterations, take it by value.  Included by kernels.hip.
#pragma once

namespace nnsdp {

// everything one plain ADMM iteration of one SDP needs besides the projection
struct IterArgs {
  int ng, NE, ldm, nlong;
  long long nmat;
  const int* sptr; const long long* soff; const unsigned char* isdiag;
  const int* csc_ptr; const int* csc_row; const double* csc_val;
  const int* csr_ptr; const int* csr_col; const double* csr_val;
  const int* longrows; const unsigned int* gidx;
  const int* medrows; const int* medsrc; int nmed, nmsrc, nnz;   // rows of A with 3 .. kLongRow nonzeros / pattern entries with more than 2 sources
  const int* colcls; int ncs;                                      // multipliers by column length: the first ncs of colcls have <= kShortCol nonzeros
  const double* z0; const double* Dinv; const double* c; const double* Minv;
  double* nu; double* w; double* g; double* p; double* qv; double* ww; double* x;
  const double* sigma; double* kappa;
  double alpha;
  double* symv_part;     // [nb][nb][64] partial products of the tiled symmetric M^-1 q (batch handles), nb = ceil(ng / 64)
};

static constexpr int kGatherLanes = 8;   // lanes per pattern entry of the sharded gather (k_gather_h)
static constexpr int kFusedCols = 4;     // columns of M^-1 per workgroup of the family pass (k_minv_family)
// (host_common.hpp's cdiv is not visible here: kernels.hip is also built alone, by tools/prof_jacobi.hip)
static inline int tail_blocks(long long items, int per = kThreads) { return (int)((items + per - 1) / per); }

// Workgroups per stage and class of one SDP.  A batch launch takes the maximum over its members (cover); every batch kernel sends
// the blocks past a member's own counts home at once.
struct TailGrid {
  int entries = 0, med_src = 0;         // gather: pattern entries one thread each / 16 lanes per entry with more than two sources
  int short_cols = 0, long_cols = 0;    // A': 16 lanes per column of up to kShortCol nonzeros / a wave per longer column
  int gemv = 0;                         // dense M^-1: a wave per row
  int med_rows = 0, long_rows = 0;      // A (its short rows take `entries`): 16 lanes per medium row / a workgroup per long row
  int update = 0;                       // multiplier update: a thread per element of nu
  int tiles = 0, nb = 0;                // tiled symmetric M^-1 of the batch handle: 64 x 64 tiles, four to a workgroup / row blocks
  int family = 0;                       // family pass over a shared M^-1: kFusedCols columns per workgroup
  int own_src = 0, dual = 0, obj = 0;   // sharded gather (kGatherLanes lanes per entry) / check kernels: 16 lanes per entry, max(ng, NE)
  TailGrid() = default;
  explicit TailGrid(const IterArgs& a)
      : entries(tail_blocks(a.NE)), med_src(tail_blocks((long long)a.nmsrc * 16)), short_cols(tail_blocks((long long)a.ncs * 16)),
        long_cols(tail_blocks((long long)(a.ng - a.ncs) * 64)), gemv(tail_blocks((long long)a.ng * 64)),
        med_rows(tail_blocks((long long)a.nmed * 16)), long_rows(a.nlong), update(tail_blocks(a.ng + a.nmat)),
        tiles(tail_blocks((long long)((a.ng + 63) / 64) * ((a.ng + 63) / 64 + 1) / 2, kThreads / 64)), nb((a.ng + 63) / 64),
        family(tail_blocks(a.ng, kFusedCols)), own_src(tail_blocks((long long)a.NE * kGatherLanes)),
        dual(tail_blocks((long long)a.NE * 16)), obj(tail_blocks(std::max(a.ng, a.NE))) {}
  void cover(const TailGrid& o) {
    using T = TailGrid;
    for (int T::*m : {&T::entries, &T::med_src, &T::short_cols, &T::long_cols, &T::gemv, &T::med_rows, &T::long_rows, &T::update, &T::tiles, &T::nb,
                      &T::family, &T::own_src, &T::dual, &T::obj}) this->*m = std::max(this->*m, o.*m);
  }
  int check_dual() const { return dual + long_rows; }      // blocks of k_check_dual: the 16-lane ones, then one per long row
  int check_stride() const { return std::max({update, check_dual(), obj}); }      // per-quantity stride of the check kernels' partial sums
};

// ---------------------------------------------------------------------------------------------
// multiplier block: w_s = max(nu_s, 0), reflection p = 2 w_s - nu_s - c   (also applies kappa)
// fused into the A' product: qv[g] = sum_e A[e,g] gvec[e] - p[g]; one wave per multiplier.
// ---------------------------------------------------------------------------------------------
// Columns of A (one per multiplier) by length (round 4): two thirds of them hold at most 64 nonzeros - a wave per column left most lanes
// idle and, in the batch handle, 29 k waves for three dependent round trips each (16.9 us for 13 SDPs).  Columns of up to kShortCol
// nonzeros take 16 lanes (blocks [0, nsb): 16 columns per workgroup, the whole column in flight at once), the others a wave with four
// chunks of 64 in flight; colcls lists the short ones first.
static constexpr int kShortCol = 64;
__device__ __forceinline__ void spmv_At_body(const int bid, const int nsb, int ng, const int* __restrict__ ptr, const int* __restrict__ row,
    const double* __restrict__ val, const double* __restrict__ gvec, double* __restrict__ nus, const double* __restrict__ c,
    const double* __restrict__ kappa, double* __restrict__ p, double* __restrict__ qv, const int* __restrict__ colcls, const int ncs) {
  int g, lane;
  double s = 0.0;
  const bool shortc = bid < nsb;
  if (shortc) {
    const int gi = bid * (kThreads / 16) + (threadIdx.x >> 4);
    lane = threadIdx.x & 15;
    if (gi >= ncs) return;            // (whole 16-lane groups leave together: the DPP row sums below stay inside a group)
    g = colcls[gi];
  } else {
    const int wi = (bid - nsb) * (kThreads / 64) + (threadIdx.x >> 6);
    lane = threadIdx.x & 63;
    if (wi >= ng - ncs) return;
    g = colcls[ncs + wi];
  }
  // (everything lane 0 needs at the end is requested before the column loop: a dependent round trip less)
  const double v0 = nus[g], cg = c[g];
  const double kap = kappa ? *kappa : 1.0;
  const int q0 = ptr[g], q1 = ptr[g + 1];
  if (shortc) {
    double vv[4]; int rr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int qq = max(min(q0 + lane + 16 * u, q1 - 1), 0); vv[u] = val[qq]; rr[u] = row[qq]; }      // (an empty column reads a neighbour's entry and discards it)
    double gg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) gg[u] = gvec[rr[u]];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (q0 + lane + 16 * u < q1) ? vv[u] * gg[u] : 0.0;
    s = row_sum16(s);
  } else {
    // (a tenth of the columns hold 250 .. 530 nonzeros - the sector multipliers' W' diag W blocks: four chunks of 64 are requested
    // together, index / value loads first and the gathers behind them, instead of one dependent chain per chunk)
    for (int q = q0 + lane; q < q1; q += 256) {
      double vv[4]; int rr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int qq = min(q + 64 * u, q1 - 1); vv[u] = val[qq]; rr[u] = row[qq]; }
      double gg[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) gg[u] = gvec[rr[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) s += (q + 64 * u < q1) ? vv[u] * gg[u] : 0.0;
    }
    s = wave_sum(s);
  }
  if (lane == 0) {
    double v = v0, wv = v > 0.0 ? v : 0.0;
    if (kap != 1.0) { v = wv + kap * (v - wv); nus[g] = v; }
    double pp = 2.0 * wv - v - cg;
    p[g] = pp;
    qv[g] = s - pp;
  }
}
__global__ __launch_bounds__(kThreads) void k_spmv_At(int nsb, int ng, const int* __restrict__ ptr, const int* __restrict__ row,
    const double* __restrict__ val, const double* __restrict__ gvec, double* __restrict__ nus, const double* __restrict__ c,
    const double* __restrict__ kappa, double* __restrict__ p, double* __restrict__ qv, const int* __restrict__ colcls, int ncs) {
  spmv_At_body(blockIdx.x, nsb, ng, ptr, row, val, gvec, nus, c, kappa, p, qv, colcls, ncs);
}
__global__ __launch_bounds__(kThreads) void k_spmv_At_b(const IterArgs* __restrict__ A, const int nsb_max) {
  const IterArgs a = A[blockIdx.y];
  spmv_At_body(blockIdx.x, nsb_max, a.ng, a.csc_ptr, a.csc_row, a.csc_val, a.g, a.nu, a.c, a.kappa, a.p, a.qv, a.colcls, a.ncs);
}
inline void launch_At(const TailGrid& G, const IterArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_spmv_At, dim3(std::max(G.short_cols + G.long_cols, 1)), dim3(kThreads), 0, st, G.short_cols, a.ng, a.csc_ptr, a.csc_row,
                     a.csc_val, a.g, a.nu, a.c, a.kappa, a.p, a.qv, a.colcls, a.ncs);
}
inline void launch_At(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_spmv_At_b, dim3(std::max(G.short_cols + G.long_cols, 1), B), dim3(kThreads), 0, st, A, G.short_cols);
}

// g[e] = Dinv[e] (z0[e] / sigma + wgt * sum_src (2 w - nu)[src]); kGatherLanes lanes per pattern entry: the entries of the
// block every clique shares ((x_K, a): 19 sources at W40-D20, 39 at W40-D40) are a dependent chain of 19-39 indirect loads for
// ONE thread otherwise, and the launch lasts as long as that chain (11.1 us for 27.6 k entries)
__device__ __forceinline__ double gather_sum(double s) {   // sum over the kGatherLanes lanes of an entry, valid in all of them
#pragma unroll
  for (int o = 1; o < kGatherLanes; o <<= 1) s += __shfl_xor(s, o, kGatherLanes);
  return s;
}
// Round 4: most pattern entries have ONE source (an element of one clique) or two (an overlap); only the block every clique shares
// and the overlap strips have more.  Eight lanes per entry for all of them meant 8 x NE threads whose launches, in the batch handle,
// ran at 1.6 TB/s for want of resident waves (13 SDPs: 11 k workgroups, five rounds of three dependent round trips).  Entries with
// up to two sources now take ONE thread (blocks [0, nshort)), the others 16 lanes each from a list built at set-up (blocks behind).
__device__ __forceinline__ void gather_g_body(const int bid, const int nshort, int NE, const int* __restrict__ sptr,
    const long long* __restrict__ soff, const unsigned char* __restrict__ isdiag, const double* __restrict__ nuk, const double* __restrict__ wk,
    const double* __restrict__ z0, const double* __restrict__ Dinv, const double* __restrict__ sigma, double* __restrict__ g,
    const int* __restrict__ medsrc, const int nmsrc) {
  if (bid < nshort) {
    const int e = bid * kThreads + threadIdx.x;
    if (e >= NE) return;
    const int p0 = sptr[e], ns = sptr[e + 1] - p0;
    const double zz = z0[e], dd = Dinv[e], sg = *sigma;
    const bool dg = isdiag[e] != 0;
    if (ns > 2) return;
    // (both source slots are read whatever ns is - clamped, masked afterwards: no load waits behind a branch)
    const long long o0 = soff[p0], o1 = soff[p0 + (ns > 1 ? 1 : 0)];
    const double a0 = 2.0 * wk[o0] - nuk[o0], a1 = 2.0 * wk[o1] - nuk[o1];
    double s = (ns > 0 ? a0 : 0.0) + (ns > 1 ? a1 : 0.0);
    if (!dg) s *= kSqrt2;
    g[e] = dd * (zz / sg + s);
    return;
  }
  const int t = (bid - nshort) * kThreads + threadIdx.x;
  const int r = t >> 4, sub = t & 15;
  if (r >= nmsrc) return;   // (the lanes of one entry leave together)
  const int e = medsrc[r];
  double s = 0.0;
  for (int q = sptr[e] + sub; q < sptr[e + 1]; q += 16) { long long o = soff[q]; s += 2.0 * wk[o] - nuk[o]; }
  s = row_sum16(s);
  if (sub != 0) return;
  if (!isdiag[e]) s *= kSqrt2;
  g[e] = Dinv[e] * (z0[e] / (*sigma) + s);
}
__global__ __launch_bounds__(kThreads) void k_gather_g(int nshort, int NE, const int* __restrict__ sptr, const long long* __restrict__ soff,
    const unsigned char* __restrict__ isdiag, const double* __restrict__ nuk, const double* __restrict__ wk, const double* __restrict__ z0,
    const double* __restrict__ Dinv, const double* __restrict__ sigma, double* __restrict__ g, const int* __restrict__ medsrc, int nmsrc) {
  gather_g_body(blockIdx.x, nshort, NE, sptr, soff, isdiag, nuk, wk, z0, Dinv, sigma, g, medsrc, nmsrc);
}
// batch handles: blocks [0, nshort_max) one thread per entry, blocks behind 16 lanes per listed entry (every member leaves the blocks
// past its own counts at once)
__global__ __launch_bounds__(kThreads) void k_gather_g_b(const IterArgs* __restrict__ A, int nshort_max) {
  const IterArgs a = A[blockIdx.y];
  const int mine = (a.NE + kThreads - 1) / kThreads;
  int bid = blockIdx.x;
  if (bid < nshort_max) { if (bid >= mine) return; }
  else { bid = bid - nshort_max + mine; if ((long long)(bid - mine) * kThreads >= (long long)a.nmsrc * 16) return; }
  gather_g_body(bid, mine, a.NE, a.sptr, a.soff, a.isdiag, a.nu + a.ng, a.w + a.ng, a.z0, a.Dinv, a.sigma, a.g, a.medsrc, a.nmsrc);
}
inline void launch_gather(const TailGrid& G, const IterArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_gather_g, dim3(G.entries + G.med_src), dim3(kThreads), 0, st, G.entries, a.NE, a.sptr, a.soff, a.isdiag, a.nu + a.ng,
                     a.w + a.ng, a.z0, a.Dinv, a.sigma, a.g, a.medsrc, a.nmsrc);
}
inline void launch_gather(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_gather_g_b, dim3(G.entries + G.med_src, B), dim3(kThreads), 0, st, A, G.entries);
}

// clique-sharded mode: h[e] = wgt * sum over the rank's OWN sources of (2 w - nu), or of (nu - w) when dual != 0;
// summed over ranks with one all-reduce, then k_finish_g
__global__ __launch_bounds__(kThreads) void k_gather_h(int NE, const int* __restrict__ sptr, const long long* __restrict__ soff,
    const unsigned char* __restrict__ isdiag, const double* __restrict__ nuk, const double* __restrict__ wk, int dual, double* __restrict__ h,
    const unsigned long long* __restrict__ ipc_ctr) {
  // (device-side transport: the partial sum goes into the slot of the NEXT exchange of this rank's mapped buffer; the exchange
  // number lives on the device, so a replayed hipGraph picks the right slot whatever ran between two replays)
  if (ipc_ctr) h += (size_t)((*ipc_ctr + 1) & 1) * NE;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int e = t / kGatherLanes, sub = t % kGatherLanes;
  if (e >= NE) return;
  double s = 0.0;
  for (int q = sptr[e] + sub; q < sptr[e + 1]; q += kGatherLanes) {
    long long o = soff[q];
    s += dual ? nuk[o] - wk[o] : 2.0 * wk[o] - nuk[o];
  }
  s = gather_sum(s);
  if (sub != 0) return;
  if (!isdiag[e]) s *= kSqrt2;
  h[e] = s;
}
inline void launch_gather_h(const TailGrid& G, const IterArgs& a, const int* sptr_own, const long long* soff_own, int dual, double* h,
    const unsigned long long* ipc_ctr, hipStream_t st) {
  hipLaunchKernelGGL(k_gather_h, dim3(G.own_src), dim3(kThreads), 0, st, a.NE, sptr_own, soff_own, a.isdiag, a.nu + a.ng, a.w + a.ng, dual, h, ipc_ctr);
}

// ---------------------------------------------------------------------------------------------
// Clique-sharded mode, device-side transport (round 4): the ranks are processes of one node whose exchange buffers are mapped into
// each other's address space with hipIpc (one card, or peers over xGMI).  Every rank writes its partial consensus sum into slot
// (exchange number & 1) of ITS buffer, publishes the exchange number behind a system-scope release, and then sums the slots of all
// ranks in rank order - one-shot all-gather + local reduce, the same bits on every rank, no library kernel
// in the iteration.  Two slots are enough: a rank can only reach exchange c + 2 after every peer has published c + 1, i.e. after it
// has finished reading slot c & 1.  The wait is a bounded spin (a peer that never publishes sets the error word and the caller
// throws at its next check instead of hanging the card).
//   layout of a rank's buffer: [2][NE] doubles | flags[2] (unsigned long long) at double offset 2 NE
// ---------------------------------------------------------------------------------------------
struct IpcArgs {
  double* peer[8];              // every rank's buffer in THIS process's address space (own buffer included), rank order
  int nranks, rank, NE;
  unsigned long long* ctr;      // this rank's exchange counter (device)
  int* err;                     // set to 1 when a wait ran out
  long long spin_limit;
};
__global__ void k_ipc_publish(IpcArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long c = *a.ctr + 1;
  *a.ctr = c;
  unsigned long long* flags = reinterpret_cast<unsigned long long*>(a.peer[a.rank] + 2 * (size_t)a.NE);
  __threadfence_system();                                   // the slot's stores (previous kernel) are complete and visible
  __hip_atomic_store(flags + (c & 1), c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(kThreads) void k_ipc_reduce(IpcArgs a, double* __restrict__ out) {
  __shared__ int bad;
  const unsigned long long c = *a.ctr;                      // (published by this rank earlier on the stream)
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  if ((int)threadIdx.x < a.nranks && (int)threadIdx.x != a.rank) {      // one lane per peer: the waits (a fabric round trip each) overlap
    const int r = threadIdx.x;
    const unsigned long long* f = reinterpret_cast<const unsigned long long*>(a.peer[r] + 2 * (size_t)a.NE) + (c & 1);
    long long spins = 0;
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < c) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > a.spin_limit) { atomicExch(a.err, 1); bad = 1; break; }
    }
    __threadfence_system();
  }
  __syncthreads();
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.NE) return;
  const size_t o = (size_t)(c & 1) * a.NE + e;
  double s = 0.0;
  for (int r = 0; r < a.nranks; ++r)      // (system-scope loads: a peer's lines may sit stale in this XCD's L2 from two exchanges ago)
    s += __hip_atomic_load(a.peer[r] + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  out[e] = s;
}
inline void launch_ipc_exchange(const TailGrid& G, const IpcArgs& a, double* out, hipStream_t st) {      // publish this rank's slot, sum all ranks'
  hipLaunchKernelGGL(k_ipc_publish, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_ipc_reduce, dim3(G.entries), dim3(kThreads), 0, st, a, out);
}

__global__ __launch_bounds__(kThreads) void k_finish_g(int NE, const double* __restrict__ h, const double* __restrict__ z0,
    const double* __restrict__ Dinv, const double* __restrict__ sigma, double* __restrict__ g) {
  int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < NE) g[e] = Dinv[e] * (z0[e] / (*sigma) + h[e]);
}
inline void launch_finish_g(const TailGrid& G, const IterArgs& a, const double* h, hipStream_t st) {
  hipLaunchKernelGGL(k_finish_g, dim3(G.entries), dim3(kThreads), 0, st, a.NE, h, a.z0, a.Dinv, a.sigma, a.g);
}

// ww = Minv qv  (Minv symmetric, column-major): one wave per output row, coalesced column reads
static constexpr int kGemvGroup = 8;      // 16-byte pairs of a row a lane has in flight at once (8 x 128 columns per group)
__device__ __forceinline__ void gemv_sym_body(const int bid, int n, int ldm, const double* __restrict__ Minv, const double* __restrict__ x,
    double* __restrict__ y) {
  int i = (bid * kThreads + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  if (i >= n) return;
  const double* col = Minv + (size_t)i * ldm;  // ldm even: 16-byte aligned columns
  double s0 = 0.0, s1 = 0.0;
  // A lane's sums run over the pairs (j, j + 1), j = 2 lane + 128 k, in the order of k: s0 over the even elements, s1 over the odd
  // ones, then the last element of an odd n in the lane whose next pair it would have begun.  The pairs are read kGemvGroup at a time
  // into registers and multiplied in the same order; how many of a group's 16 loads are issued in front of the first product's wait
  // is the compiler's choice (DESIGN.md section 5 has what it does and what forcing all of them there costs).  The last group reads
  // pair 0 in place of a pair past the end and leaves its sums alone.
  const bool rem = (n & 1) && (((n - 1) >> 1) & 63) == lane;
  const double mr = rem ? col[n - 1] : 0.0, xr = rem ? x[n - 1] : 0.0;
  const int j0 = lane * 2;
  int base = 0;
  for (; base + 128 * kGemvGroup <= n; base += 128 * kGemvGroup) {      // (every pair of the group inside the row, for all lanes)
    double2 m[kGemvGroup], xv[kGemvGroup];
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) m[u] = *reinterpret_cast<const double2*>(col + base + j0 + 128 * u);
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) xv[u] = *reinterpret_cast<const double2*>(x + base + j0 + 128 * u);
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) { s0 = fma(m[u].x, xv[u].x, s0); s1 = fma(m[u].y, xv[u].y, s1); }
  }
  if (base + 1 < n) {      // (uniform: n >= 2 here, so pair 0 exists)
    double2 m[kGemvGroup], xv[kGemvGroup];
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) { const int j = base + j0 + 128 * u; m[u] = *reinterpret_cast<const double2*>(col + (j + 1 < n ? j : 0)); }
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) { const int j = base + j0 + 128 * u; xv[u] = *reinterpret_cast<const double2*>(x + (j + 1 < n ? j : 0)); }
#pragma unroll
    for (int u = 0; u < kGemvGroup; ++u) {
      const bool in = base + j0 + 128 * u + 1 < n;
      const double t0 = fma(m[u].x, xv[u].x, s0), t1 = fma(m[u].y, xv[u].y, s1);
      s0 = in ? t0 : s0;
      s1 = in ? t1 : s1;
    }
  }
  if (rem) s0 = fma(mr, xr, s0);
  double s = wave_sum(s0 + s1);
  if (lane == 0) y[i] = s;
}
__global__ __launch_bounds__(kThreads) void k_gemv_sym(int n, int ldm, const double* __restrict__ Minv, const double* __restrict__ x,
    double* __restrict__ y) { gemv_sym_body(blockIdx.x, n, ldm, Minv, x, y); }
__global__ __launch_bounds__(kThreads) void k_gemv_sym_b(const IterArgs* __restrict__ A) {
  const IterArgs a = A[blockIdx.y];
  if ((long long)blockIdx.x * kThreads >= (long long)a.ng * 64) return;
  gemv_sym_body(blockIdx.x, a.ng, a.ldm, a.Minv, a.qv, a.ww);
}
inline void launch_gemv(const TailGrid& G, const IterArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_gemv_sym, dim3(G.gemv), dim3(kThreads), 0, st, a.ng, a.ldm, a.Minv, a.qv, a.ww);
}
inline void launch_gemv(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_gemv_sym_b, dim3(G.gemv, B), dim3(kThreads), 0, st, A);
}

// ---------------------------------------------------------------------------------------------
// Batch handles: ww = Minv qv reading only the LOWER triangle of the symmetric Minv (half the HBM traffic of
// k_gemv_sym; with 13 SDPs the product is 26 % of a lockstep iteration).  64 x 64 tiles (I >= J), one wave per tile:
// lane r owns row r of the tile and adds T[r][c] x_J[c] over the columns (direct part, y_I); the transposed part
// y_J[c] = sum_r T[r][c] x_I[r] needs a sum ACROSS lanes per column - done 8 columns at a time with a halving
// exchange (4 + 2 + 1 values, then three full steps on one value: 10 exchanges per 8 columns instead of 48).
// Every tile writes its two 64-vectors into its own slot of part[block][other block][64]; a second launch adds the
// nb slots of every block in a fixed order, so the result does not depend on scheduling.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_symv_tiles_b(const IterArgs* __restrict__ A) {
  const IterArgs a = A[blockIdx.y];
  const int n = a.ng, nb = (n + 63) >> 6;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= nb * (nb + 1) / 2) return;
  int I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (I * (I + 1) / 2 > t) --I;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  const int J = t - I * (I + 1) / 2;
  const int r0 = I << 6, c0 = J << 6;
  const int row = r0 + lane;
  const bool rv = row < n;
  const double* __restrict__ x = a.qv;
  const double* __restrict__ Mp = a.Minv + row;
  const double xi = rv ? x[row] : 0.0;
  double acc = 0.0;        // direct part: row `row` of y_I
  double outT = 0.0;       // transposed part: column tcol(lane) of y_J
  const int ldm = a.ldm;
#pragma unroll 1
  for (int g8 = 0; g8 < 8; ++g8) {
    double p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = c0 + 8 * g8 + i;
      const double v = (rv && c < n) ? Mp[(size_t)c * ldm] : 0.0;
      const double xc = c < n ? x[c] : 0.0;      // wave-uniform
      acc += v * xc;
      p[i] = v * xi;
    }
    if (I != J) {
      // 8 column sums over 64 lanes.  Halving steps over lane bits 5, 4, 3 ...
      const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
      double q[4], r[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) { const double send = h5 ? p[i] : p[4 + i], keep = h5 ? p[4 + i] : p[i]; q[i] = keep + __shfl_xor(send, 32, 64); }
#pragma unroll
      for (int i = 0; i < 2; ++i) { const double send = h4 ? q[i] : q[2 + i], keep = h4 ? q[2 + i] : q[i]; r[i] = keep + __shfl_xor(send, 16, 64); }
      double sv;
      { const double send = h3 ? r[0] : r[1], keep = h3 ? r[1] : r[0]; sv = keep + __shfl_xor(send, 8, 64); }
      // ... then plain butterfly steps over bits 2, 1, 0
      sv += __shfl_xor(sv, 4, 64);
      sv += __shfl_xor(sv, 2, 64);
      sv += __shfl_xor(sv, 1, 64);
      // lane holds the sum of column 8 g8 + 4 h5 + 2 h4 + h3 of the tile; lanes with (lane & 7) == g8 keep it
      if ((lane & 7) == g8) outT = sv;
    }
  }
  double* part = a.symv_part;
  part[((size_t)I * nb + J) * 64 + lane] = acc;
  if (I != J) {
    const int tc = 8 * (lane & 7) + ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
    part[((size_t)J * nb + I) * 64 + tc] = outT;
  }
}
__global__ __launch_bounds__(64) void k_symv_reduce_b(const IterArgs* __restrict__ A) {
  const IterArgs a = A[blockIdx.y];
  const int n = a.ng, nb = (n + 63) >> 6;
  const int b = blockIdx.x;
  if (b >= nb) return;
  const double* part = a.symv_part + (size_t)b * nb * 64 + threadIdx.x;
  double s = 0.0;
  int k = 0;
  for (; k + 8 <= nb; k += 8) {          // loads of 8 slots in flight, added in slot order
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(k + i) * 64];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; k < nb; ++k) s += part[(size_t)k * 64];
  const int row = b * 64 + threadIdx.x;
  if (row < n) a.ww[row] = s;
}
inline void launch_symv(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {      // tiles, then their sums in slot order
  hipLaunchKernelGGL(k_symv_tiles_b, dim3(G.tiles, B), dim3(kThreads), 0, st, A);
  hipLaunchKernelGGL(k_symv_reduce_b, dim3(G.nb, B), dim3(64), 0, st, A);
}

// ---------------------------------------------------------------------------------------------
// Solver families (members that share ONE M^-1): ww_b = Minv qv_b for up to kFusedWidth members in one pass over the matrix.
// A workgroup owns kFusedCols columns of Minv (= rows: it is symmetric) over their whole height, its four waves take the
// 128-row chunks c = wave, wave + 4, ...: per chunk one 16-byte load per lane and column (kFusedCols independent loads in
// flight) and one 16-byte load of every member's qv (L2: the vectors of a group are a few hundred KB), then
// 2 x kFusedCols x nb FMAs.  Both triangles are read: 8 ng ldm bytes per pass whatever nb is (W40-D20: 30.9 MB, ~1970 waves).
// Per member the arithmetic is a fixed sequence the other members only sit beside - lane partial over the wave's chunks in chunk
// order (two FMAs per chunk), wave_sum, the four waves' sums added in wave order through LDS - so a member's result depends neither
// on nb nor on the slot it sits in; no atomics.  Several groups share one launch: blockIdx.y selects the pass.
// ---------------------------------------------------------------------------------------------
static constexpr int kFusedWidth = 16;   // members per pass
struct FusedPass { int first, count; };  // slots [first, first + count) of the member list
__global__ __launch_bounds__(kThreads) void k_minv_family(const IterArgs* __restrict__ A, const int* __restrict__ members,
    const FusedPass* __restrict__ passes) {
  __shared__ double red[kThreads / 64][kFusedCols][kFusedWidth];
  const FusedPass ps = passes[blockIdx.y];
  const int* __restrict__ mem = members + ps.first;
  const int nb = ps.count;
  const IterArgs& a0 = A[mem[0]];
  const int n = a0.ng, ldm = a0.ldm;
  const int col0 = blockIdx.x * kFusedCols;
  if (col0 >= n) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double* __restrict__ mc[kFusedCols];
#pragma unroll
  for (int r = 0; r < kFusedCols; ++r) mc[r] = a0.Minv + (size_t)min(col0 + r, n - 1) * ldm;   // (a column past the end repeats the last one; not written)
  const double* __restrict__ q[kFusedWidth];
#pragma unroll
  for (int b = 0; b < kFusedWidth; ++b) q[b] = A[mem[b < nb ? b : 0]].qv;
  double acc[kFusedCols][kFusedWidth];
#pragma unroll
  for (int r = 0; r < kFusedCols; ++r)
#pragma unroll
    for (int b = 0; b < kFusedWidth; ++b) acc[r][b] = 0.0;
  for (int j = wv * 128 + lane * 2; j < n; j += (kThreads / 64) * 128) {
    const bool two = j + 1 < n;
    double2 m[kFusedCols];
#pragma unroll
    for (int r = 0; r < kFusedCols; ++r) {
      if (two) m[r] = *reinterpret_cast<const double2*>(mc[r] + j);
      else { m[r].x = mc[r][j]; m[r].y = 0.0; }
    }
#pragma unroll
    for (int b = 0; b < kFusedWidth; ++b) {
      if (b < nb) {        // (uniform over the workgroup)
        double2 x;
        if (two) x = *reinterpret_cast<const double2*>(q[b] + j);
        else { x.x = q[b][j]; x.y = 0.0; }
#pragma unroll
        for (int r = 0; r < kFusedCols; ++r) acc[r][b] = fma(m[r].y, x.y, fma(m[r].x, x.x, acc[r][b]));
      }
    }
  }
#pragma unroll
  for (int b = 0; b < kFusedWidth; ++b) {
    if (b < nb) {
#pragma unroll
      for (int r = 0; r < kFusedCols; ++r) {
        const double s = wave_sum(acc[r][b]);
        if (lane == 0) red[wv][r][b] = s;
      }
    }
  }
  __syncthreads();
  const int r = threadIdx.x / kFusedWidth, b = threadIdx.x % kFusedWidth;
  if (r < kFusedCols && b < nb && col0 + r < n)
    A[mem[b]].ww[col0 + r] = ((red[0][r][b] + red[1][r][b]) + red[2][r][b]) + red[3][r][b];
}
inline void launch_minv_family(const TailGrid& G, const IterArgs* A, const int* members, const FusedPass* passes, int npass, hipStream_t st) {
  hipLaunchKernelGGL(k_minv_family, dim3(G.family, npass), dim3(kThreads), 0, st, A, members, passes);
}

// x[e] = g[e] - Dinv[e] * sum_g A[e,g] ww[g]; 4 lanes per pattern entry (W40-D20: 27.6 k rows, 60 % of them with no
// multiplier at all and 37 % with one; only 2 880 rows carry more than 16 nonzeros)
static constexpr int kLongRow = 256;   // rows of A with more nonzeros go to the block-per-row kernel
// Round 4: 60 % of the rows of A have no multiplier at all and 37 % one (W40-D20); rows with up to two nonzeros take ONE thread
// (blocks [0, nshort)), rows with 3 .. kLongRow nonzeros 16 lanes each from a list built at set-up (the first form gave every row 8
// lanes: 8 x NE threads per SDP, and the batched launch ran at 0.6 TB/s - resident-wave-bound, five rounds of dependent round trips)
__device__ __forceinline__ void spmv_A_x_body(const int bid, const int nshort, int NE, const int* __restrict__ ptr, const int* __restrict__ col,
    const double* __restrict__ val, const double* __restrict__ ww, const double* __restrict__ g, const double* __restrict__ Dinv,
    double* __restrict__ x, const int* __restrict__ medrows, const int nmed, const int nnz) {
  if (bid < nshort) {
    const int e = bid * kThreads + threadIdx.x;
    if (e >= NE) return;
    const int p0 = ptr[e], n = ptr[e + 1] - p0;
    const double ge = g[e], de = Dinv[e];
    if (n > 2) return;
    // (both slots read whatever n is - clamped into the table, masked afterwards)
    const int q0 = min(p0, nnz - 1), q1 = min(p0 + 1, nnz - 1);
    const double t0 = val[q0] * ww[col[q0]], t1 = val[q1] * ww[col[q1]];
    const double s = (n > 0 ? t0 : 0.0) + (n > 1 ? t1 : 0.0);
    x[e] = ge - de * s;
    return;
  }
  const int t = (bid - nshort) * kThreads + threadIdx.x;
  const int r = t >> 4, sub = t & 15;
  if (r >= nmed) return;
  const int e = medrows[r];
  const double ge = g[e], de = Dinv[e];
  double s = 0.0;
  const int q1 = ptr[e + 1];
  for (int q = ptr[e] + sub; q < q1; q += 64) {      // (four chunks of 16 in flight)
    double vv[4]; int cc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int qq = min(q + 16 * u, q1 - 1); vv[u] = val[qq]; cc[u] = col[qq]; }
    double xx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xx[u] = ww[cc[u]];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (q + 16 * u < q1) ? vv[u] * xx[u] : 0.0;
  }
  s = row_sum16(s);
  if (sub == 0) x[e] = ge - de * s;
}

// the few long rows (the affine-affine entry touches every multiplier): one workgroup per row
__device__ __forceinline__ void spmv_A_x_long_body(const int bid, const int* __restrict__ rows, const int* __restrict__ ptr,
    const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ ww, const double* __restrict__ g,
    const double* __restrict__ Dinv, double* __restrict__ x) {
  __shared__ double red[8];
  int e = rows[bid];
  const double ge = g[e], de = Dinv[e];
  double s = 0.0;
  const int q1 = ptr[e + 1];
  for (int q = ptr[e] + threadIdx.x; q < q1; q += 8 * kThreads) {      // (eight chunks in flight: the affine-affine row touches every multiplier)
    double vv[8]; int cc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int qq = min(q + kThreads * u, q1 - 1); vv[u] = val[qq]; cc[u] = col[qq]; }
    double xx[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xx[u] = ww[cc[u]];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (q + kThreads * u < q1) ? vv[u] * xx[u] : 0.0;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) x[e] = ge - de * s;
}

// all forms in one launch: blocks [0, nshort) one thread per row (rows with up to two nonzeros), [nshort, nreg) 16 lanes per listed
// medium row, [nreg, nreg + nlong) one workgroup per long row
__global__ __launch_bounds__(kThreads) void k_spmv_A_x_all(int NE, int nshort, int nreg, const int* __restrict__ rows, const int* __restrict__ ptr,
    const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ ww, const double* __restrict__ g,
    const double* __restrict__ Dinv, double* __restrict__ x, const int* __restrict__ medrows, int nmed, int nnz) {
  if ((int)blockIdx.x < nreg) spmv_A_x_body(blockIdx.x, nshort, NE, ptr, col, val, ww, g, Dinv, x, medrows, nmed, nnz);
  else spmv_A_x_long_body(blockIdx.x - nreg, rows, ptr, col, val, ww, g, Dinv, x);
}
// batch handles: [0, nshort_max) short rows, [nshort_max, nshort_max + nmedb_max) medium rows, behind them the long rows
__global__ __launch_bounds__(kThreads) void k_spmv_A_x_all_b(const IterArgs* __restrict__ A, int nshort_max, int nmedb_max) {
  const IterArgs a = A[blockIdx.y];
  const int mine = (a.NE + kThreads - 1) / kThreads;
  const int b = blockIdx.x;
  if (b < nshort_max) {
    if (b >= mine) return;
    spmv_A_x_body(b, mine, a.NE, a.csr_ptr, a.csr_col, a.csr_val, a.ww, a.g, a.Dinv, a.x, a.medrows, a.nmed, a.nnz);
  } else if (b < nshort_max + nmedb_max) {
    const int bm = b - nshort_max;
    if ((long long)bm * kThreads >= (long long)a.nmed * 16) return;
    spmv_A_x_body(mine + bm, mine, a.NE, a.csr_ptr, a.csr_col, a.csr_val, a.ww, a.g, a.Dinv, a.x, a.medrows, a.nmed, a.nnz);
  } else {
    const int bl = b - nshort_max - nmedb_max;
    if (bl >= a.nlong) return;
    spmv_A_x_long_body(bl, a.longrows, a.csr_ptr, a.csr_col, a.csr_val, a.ww, a.g, a.Dinv, a.x);
  }
}
inline void launch_Ax(const TailGrid& G, const IterArgs& a, hipStream_t st) {
  const int nreg = G.entries + G.med_rows;
  hipLaunchKernelGGL(k_spmv_A_x_all, dim3(nreg + G.long_rows), dim3(kThreads), 0, st, a.NE, G.entries, nreg, a.longrows, a.csr_ptr, a.csr_col,
                     a.csr_val, a.ww, a.g, a.Dinv, a.x, a.medrows, a.nmed, a.nnz);
}
inline void launch_Ax(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_spmv_A_x_all_b, dim3(G.entries + G.med_rows + G.long_rows, B), dim3(kThreads), 0, st, A, G.entries, G.med_rows);
}

// nu <- nu + alpha (K x + q - w).  acc (may be null) accumulates at check iterations:
//   |Kx+q-w|^2, |Kx+q|^2, |w|^2 as per-workgroup partial sums acc[{0,1,2} * astride + block]; k_acc_reduce adds the partials
//   in block order, so the residuals (and with them every stopping / penalty decision) are reproducible run to run
__device__ __forceinline__ void update_nu_body(const int bid, int ng, long long nmat, const double* __restrict__ p, const double* __restrict__ ww,
    const double* __restrict__ c, const double* __restrict__ x, const unsigned int* __restrict__ gidx, double* __restrict__ nu,
    const double* __restrict__ w, double alpha, double* __restrict__ kappa, double* __restrict__ acc, long long lo, long long hi, int acc_s,
    int astride) {
  // [lo, hi): the clique elements this rank owns (everything when not sharded); acc_s: count the
  // multiplier block in the residual sums (rank 0 only when sharded, the sums are all-reduced)
  __shared__ double red[8];
  long long i = (long long)bid * kThreads + threadIdx.x;
  double r2 = 0.0, k2 = 0.0, w2 = 0.0;
  if (i < ng) {
    double v = nu[i], wv = v > 0.0 ? v : 0.0;
    double kxq = p[i] + ww[i] + c[i];
    double res = kxq - wv;
    nu[i] = v + alpha * res;
    if (acc_s) { r2 = res * res; k2 = kxq * kxq; w2 = wv * wv; }
  } else if (i < ng + nmat && i - ng >= lo && i - ng < hi) {
    long long m = i - ng;
    unsigned int gi = gidx[m];
    double xv = x[gi & 0x7fffffffu];
    if (!(gi >> 31)) xv *= kInvSqrt2;
    double wv = w[i];
    double res = xv - wv;
    nu[i] += alpha * res;
    r2 = res * res; k2 = xv * xv; w2 = wv * wv;
  }
  if (acc) {
    r2 = block_sum(r2, red);
    k2 = block_sum(k2, red + 4);
    w2 = block_sum(w2, red);
    if (threadIdx.x == 0) { acc[bid] = r2; acc[astride + bid] = k2; acc[2 * astride + bid] = w2; }
  }
  // the one-shot penalty rescale is consumed: kappa is READ only by the projection and the A' kernels, which precede this
  // launch on the iteration's single stream, and never by this kernel - so resetting it here cannot race with a reader
  if (i == 0 && kappa) *kappa = 1.0;
}
__global__ __launch_bounds__(kThreads) void k_update_nu(int ng, long long nmat, const double* __restrict__ p, const double* __restrict__ ww,
    const double* __restrict__ c, const double* __restrict__ x, const unsigned int* __restrict__ gidx, double* __restrict__ nu,
    const double* __restrict__ w, double alpha, double* __restrict__ kappa, double* __restrict__ acc, long long lo, long long hi, int acc_s,
    int astride) {
  update_nu_body(blockIdx.x, ng, nmat, p, ww, c, x, gidx, nu, w, alpha, kappa, acc, lo, hi, acc_s, astride);
}
__global__ __launch_bounds__(kThreads) void k_update_nu_b(const IterArgs* __restrict__ A) {
  const IterArgs a = A[blockIdx.y];
  if ((long long)blockIdx.x * kThreads >= (long long)a.ng + a.nmat) return;
  update_nu_body(blockIdx.x, a.ng, a.nmat, a.p, a.ww, a.c, a.x, a.gidx, a.nu, a.w, a.alpha, a.kappa, nullptr, 0LL, a.nmat, 1, 0);
}
inline void launch_update(const TailGrid& G, const IterArgs& a, double* acc, long long lo, long long hi, int acc_s, hipStream_t st) {
  hipLaunchKernelGGL(k_update_nu, dim3(G.update), dim3(kThreads), 0, st, a.ng, a.nmat, a.p, a.ww, a.c, a.x, a.gidx, a.nu, a.w, a.alpha, a.kappa,
                     acc, lo, hi, acc_s, G.check_stride());
}
inline void launch_update(const TailGrid& G, const IterArgs* A, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_update_nu_b, dim3(G.update, B), dim3(kThreads), 0, st, A);
}

// check iteration, dual side: t[e] = (K'y)[e] = sum_g A[e,g] ys[g] + wgt * sum_src y_k[src],
// y = sigma (nu - w).  acc[3] += |t - z0|^2, acc[4] += |t|^2; 16 lanes per entry.
__device__ __forceinline__ void check_dual_body(int NE, int ng, int nreg, const int* __restrict__ longrows, const int* __restrict__ ptr,
    const int* __restrict__ col, const double* __restrict__ val, const int* __restrict__ sptr, const long long* __restrict__ soff,
    const unsigned char* __restrict__ isdiag, const double* __restrict__ nu, const double* __restrict__ w, const double* __restrict__ z0,
    const double* __restrict__ sigma, double* __restrict__ acc, const double* __restrict__ hsum, int astride) {
  // hsum != null (clique-sharded mode): the clique part of K'y/sigma, already summed over ranks.
  // Blocks [0, nreg): 16 lanes per entry, rows with more than kLongRow nonzeros skipped; blocks [nreg, nreg + nlong): one
  // workgroup per long row (the (a,a) entry meets every multiplier: 3 203 nonzeros at W40-D20, 200 steps for 16 lanes)
  __shared__ double red[8];
  double sg = *sigma;
  double d2 = 0.0, t2 = 0.0;
  if ((int)blockIdx.x < nreg) {
    int e = (blockIdx.x * kThreads + threadIdx.x) >> 4;
    int sub = threadIdx.x & 15;
    double s = 0.0, h = 0.0;
    const bool mine = e < NE && ptr[e + 1] - ptr[e] <= kLongRow;
    if (mine) {
      for (int q = ptr[e] + sub; q < ptr[e + 1]; q += 16) { double v = nu[col[q]]; s += val[q] * (v < 0.0 ? v : 0.0); }
      if (hsum) { if (sub == 0) h = hsum[e]; }
      else {
        for (int q = sptr[e] + sub; q < sptr[e + 1]; q += 16) { long long o = soff[q]; h += nu[ng + o] - w[ng + o]; }
        if (!isdiag[e]) h *= kSqrt2;
      }
    }
    s += h;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
    if (mine && sub == 0) { double t = sg * s; double d = t - z0[e]; d2 = d * d; t2 = t * t; }
  } else {
    const int b = blockIdx.x - nreg;
    const int e = longrows[b];      // (the grid is exactly nreg + nlong workgroups)
    double s = 0.0, h = 0.0;
    for (int q = ptr[e] + threadIdx.x; q < ptr[e + 1]; q += kThreads) { double v = nu[col[q]]; s += val[q] * (v < 0.0 ? v : 0.0); }
    if (hsum) { if (threadIdx.x == 0) h = hsum[e]; }
    else {
      for (int q = sptr[e] + threadIdx.x; q < sptr[e + 1]; q += kThreads) { long long o = soff[q]; h += nu[ng + o] - w[ng + o]; }
      if (!isdiag[e]) h *= kSqrt2;
    }
    s = block_sum(s + h, red);
    if (threadIdx.x == 0) { double t = sg * s; double d = t - z0[e]; d2 = d * d; t2 = t * t; }
    __syncthreads();
  }
  d2 = block_sum(d2, red);
  t2 = block_sum(t2, red + 4);
  if (threadIdx.x == 0) { acc[3 * astride + blockIdx.x] = d2; acc[4 * astride + blockIdx.x] = t2; }
}
__global__ __launch_bounds__(kThreads) void k_check_dual(const IterArgs a, const int nreg, double* __restrict__ accp, const double* __restrict__ hsum,
    int astride) {
  check_dual_body(a.NE, a.ng, nreg, a.longrows, a.csr_ptr, a.csr_col, a.csr_val, a.sptr, a.soff, a.isdiag, a.nu, a.w, a.z0, a.sigma, accp, hsum, astride);
}
inline void launch_check_dual(const TailGrid& G, const IterArgs& a, double* accp, const double* hsum, hipStream_t st) {
  hipLaunchKernelGGL(k_check_dual, dim3(G.check_dual()), dim3(kThreads), 0, st, a, G.dual, accp, hsum, G.check_stride());
}

// acc[5] += -c' ys  (scaled primal objective), acc[6] += z0' x (scaled dual objective)
__device__ __forceinline__ void check_obj_body(int ng, int NE, const double* __restrict__ nu, const double* __restrict__ c,
    const double* __restrict__ z0, const double* __restrict__ x, const double* __restrict__ sigma, double* __restrict__ acc, int astride) {
  __shared__ double red[8];
  int i = blockIdx.x * kThreads + threadIdx.x;
  double a = 0.0, b = 0.0;
  if (i < ng) { double v = nu[i]; a = -c[i] * (*sigma) * (v < 0.0 ? v : 0.0); }
  if (i < NE) b = z0[i] * x[i];
  a = block_sum(a, red);
  b = block_sum(b, red + 4);
  if (threadIdx.x == 0) { acc[5 * astride + blockIdx.x] = a; acc[6 * astride + blockIdx.x] = b; }
}
__global__ __launch_bounds__(kThreads) void k_check_obj(const IterArgs a, double* __restrict__ accp, int astride) {
  check_obj_body(a.ng, a.NE, a.nu, a.c, a.z0, a.x, a.sigma, accp, astride);
}
inline void launch_check_obj(const TailGrid& G, const IterArgs& a, double* accp, hipStream_t st) {
  hipLaunchKernelGGL(k_check_obj, dim3(G.obj), dim3(kThreads), 0, st, a, accp, G.check_stride());
}

// second stage of the residual sums: acc[q] = sum of the nb[q] workgroup partials of quantity q, added in a fixed order
// (thread t takes partials t, t + 256, ...; then the block tree) - no atomics anywhere on the way to a stopping decision.
__global__ __launch_bounds__(kThreads) void k_acc_reduce(const double* __restrict__ accp, int astride, int nb_upd, int nb_dual, int nb_obj,
    double* __restrict__ acc) {
  __shared__ double red[8];
#pragma unroll 1
  for (int q = 0; q < 7; ++q) {
    const int nb = q < 3 ? nb_upd : (q < 5 ? nb_dual : nb_obj);
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += kThreads) s += accp[(size_t)q * astride + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) acc[q] = s;
  }
}
inline void launch_acc_reduce(const TailGrid& G, const double* accp, double* acc, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_reduce, dim3(1), dim3(kThreads), 0, st, accp, G.check_stride(), G.update, G.check_dual(), G.obj, acc);
}

}  // namespace nnsdp
