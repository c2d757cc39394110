// The resident CROWN bounder (nnsdp_crown) and the argument checks of the entries that take literals or alpha options.  Part of the
// translation unit api.hip, which includes the kernel headers and host_common.hpp first.
#pragma once

// the refusals of the literal arguments, shared by the entries that take literals (xdims[K] must be valid)
static void check_literals(int32_t ny, int32_t nlit, const double* normals) {
  if (nlit < 0 || nlit > nnsdp::kCbW) throw std::invalid_argument("nlit must be in 0..64, got " + std::to_string(nlit));
  if (nlit > 0 && !normals) throw std::invalid_argument("normals is null with nlit > 0");
  for (int i = 0; i < nlit; ++i)
    for (int j = 0; j < ny; ++j)
      if (!std::isfinite(normals[(size_t)i * ny + j]))
        throw std::invalid_argument("literal " + std::to_string(i) + ": the normal has a non-finite entry (NaN or infinity)");
}

// the options of the projected-gradient entries; prefix: "alpha" (the slope entries) or "nodes" (nnsdp_crown_bound_nodes,
// nnsdp_make_intervals_nodes)
static void check_pg_options(const std::string& prefix, int32_t steps, double eta0, double decay) {
  if (steps < 0 || steps > 64) throw std::invalid_argument(prefix + ": steps must be in 0..64, got " + std::to_string(steps));
  if (!std::isfinite(eta0) || !(eta0 > 0.0)) throw std::invalid_argument(prefix + ": eta0 must be positive and finite");
  if (!(decay > 0.0 && decay <= 1.0)) throw std::invalid_argument(prefix + ": decay must be in (0, 1]");
}
static void check_alpha0(const double* alpha0, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(alpha0[k])) throw std::invalid_argument("alpha0 has a non-finite entry (NaN or infinity) at index " + std::to_string(k));
}

// the assignments of the node entries
static void check_assign(const int8_t* assign, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (assign[k] < -1 || assign[k] > 1)
      throw std::invalid_argument("nodes: assign must hold -1, 0 or +1, got " + std::to_string((int)assign[k]) + " at index " + std::to_string(k));
}

// The device buffers of one kind of frontier search (csrc/crown_frontier_host.hpp): the two frontiers (fr: lo and hi of the first, then
// of the second; cu: the cuts of both, then, with `roots`, the root of every box of both), one block of doubles and one of ints that
// the search carves into records, points and leaf logs.  They only grow.  A handle has one set per kind of search
struct FrontierBufs {
  DBuf<double> fr, db;
  DBuf<int> cu, ib;
  size_t cap = 0, n0 = 0;      // the carving of the last reserve: boxes per frontier, input width
  size_t bytes() const { return fr.bytes() + db.bytes() + cu.bytes() + ib.bytes(); }
  // frontiers of `cap` boxes each, `nd` doubles, `ni` ints; returns the device allocations made.  (Every size of a handle's search grows
  // with cap, so the frontier and its cuts grow together)
  int reserve(size_t cap_, size_t n0_, bool roots, size_t nd, size_t ni) {
    cap = cap_; n0 = n0_;
    int made = 0;
    if (4 * cap * n0 > fr.n) { fr.alloc(4 * cap * n0); cu.alloc(2 * cap * (n0 + (roots ? 1 : 0))); made += 2; }
    if (nd > db.n) { db.alloc(nd); ++made; }
    if (ni > ib.n) { ib.alloc(ni); ++made; }
    return made;
  }
  double* lo(int k) const { return fr.p + (size_t)k * 2 * cap * n0; }
  double* hi(int k) const { return lo(k) + cap * n0; }
  int* cuts(int k) const { return cu.p + (size_t)k * cap * n0; }
  int* root(int k) const { return cu.p + 2 * cap * n0 + (size_t)k * cap; }
  // level `depth` lives in frontier cur, its children go to cur ^ 1; the level's rows of the leaf log start at log_base
  void level(nnsdp::FrontierArgs& f, int cur, int depth, long long log_base) const {
    f.depth = depth; f.log_base = log_base;
    f.lo = lo(cur); f.hi = hi(cur); f.cuts = cuts(cur);
    f.nlo = lo(cur ^ 1); f.nhi = hi(cur ^ 1); f.ncuts = cuts(cur ^ 1);
  }
  // level 0: `count` root boxes (n0 x count column-major, pageable), no cuts
  void roots(const double* x1min, const double* x1max, size_t count, hipStream_t st) const {
    HIPCHK(hipMemcpyAsync(lo(0), x1min, count * n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(hi(0), x1max, count * n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(cuts(0), 0, count * n0 * sizeof(int), st));
  }
};

// ---------------------------------------------------------------------------------------------
// Resident CROWN bounder: the network, the literal head, the box / scratch / output buffers, pinned staging, one stream and two
// events stay alive across calls, so a level of a split tree pays one upload of its boxes, one launch, one download and one stream
// synchronisation (the one-shot entries pay the whole set-up per call).  Not thread-safe; distinct handles are independent.
// ---------------------------------------------------------------------------------------------
struct nnsdp_crown {
  int K = 0, activ = 0, nlit = 0, acdim = 0, n0 = 0, ny = 0, wp = 0;
  int max_width = nnsdp::kCbW;           // 64: k_crown_resident; 128: k_crown_wide (crown_wide.hpp), also on a narrow network
  std::vector<long long> moff;
  DBuf<int> dxd, dao;
  DBuf<long long> dmo;
  DBuf<double> dM;                       // the network, then the literal head
  DBuf<double> din, dscr, dout, dX, dY;   // boxes (lo, then hi), per-box scratch, outputs; samples in / out
  double *hin = nullptr, *hout = nullptr, *hX = nullptr, *hY = nullptr;      // pinned staging of the four transfers
  // nnsdp_crown_bound_alpha only (nothing before its first call): boxes then alpha0; the plain outputs then the alpha outputs; the state
  DBuf<double> dain, daout, dast;
  double *hain = nullptr, *haout = nullptr;
  // nnsdp_crown_bound_nodes only (nothing before its first call): boxes then assignments; every output; the multiplier state
  DBuf<double> dnin, dnout, dnst;
  double *hnin = nullptr, *hnout = nullptr;
  size_t box_cap = 0, pin_cap = 0, sample_cap = 0, alpha_cap = 0, node_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  long long n_alloc = 0, n_upload = 0, n_bound = 0;
  // the frontier searches (csrc/crown_frontier_host.hpp); nothing before the first call of each.  nnsdp_crown_search, nnsdp_crown_reach
  // and nnsdp_crown_search_many have buffers of their own (sbuf, rbuf, fbuf), sized from max_boxes at the call; the bound kernel's
  // buffers are shared, and so is the pinned copy of the status record of the first two.  The forest has the pinned copy of a level's
  // table and counts.  The results of the last call of each are kept for the *_leaves entries
  std::vector<double> normals;           // the literals of the handle (ny x nlit), kept for the proof test of the search
  FrontierBufs sbuf, rbuf, fbuf;
  int *hstatus = nullptr, *hforest = nullptr;
  size_t hforest_cap = 0;
  long long n_reach = 0;
  struct SearchLeaves {                  // flat, in the order of the Python loop; lo / hi n0 x nleaves column-major
    std::vector<double> lo, hi, bound;
    std::vector<int32_t> depth, proved, literal;
    void clear() { lo.clear(); hi.clear(); bound.clear(); depth.clear(); proved.clear(); literal.clear(); }
    void add(int n0, const double* blo, const double* bhi, int d, int prov, int lit, double bnd) {
      lo.insert(lo.end(), blo, blo + n0); hi.insert(hi.end(), bhi, bhi + n0);
      depth.push_back(d); proved.push_back(prov); literal.push_back(lit); bound.push_back(bnd);
    }
    // appends the leaves to the caller's arrays and moves the six pointers behind them
    void copy_out(double*& plo, double*& phi, int32_t*& pdepth, int32_t*& pproved, int32_t*& pliteral, double*& pbound) const {
      if (depth.empty()) return;
      if (!plo || !phi || !pdepth || !pproved || !pliteral || !pbound) throw std::invalid_argument("null argument");
      plo = std::copy(lo.begin(), lo.end(), plo); phi = std::copy(hi.begin(), hi.end(), phi);
      pdepth = std::copy(depth.begin(), depth.end(), pdepth); pproved = std::copy(proved.begin(), proved.end(), pproved);
      pliteral = std::copy(literal.begin(), literal.end(), pliteral); pbound = std::copy(bound.begin(), bound.end(), pbound);
    }
  } leaves;                              // nnsdp_crown_search
  std::vector<SearchLeaves> fleaves;     // nnsdp_crown_search_many, per root
  struct ReachLeaves {                   // flat, in the order of the Python loop; lo / hi n0 x nleaves, bound nlit x nleaves column-major
    std::vector<double> lo, hi, bound;
    std::vector<int32_t> depth, closed;
    void clear() { lo.clear(); hi.clear(); bound.clear(); depth.clear(); closed.clear(); }
  } rleaves;
  // nnsdp_crown_search_nodes (csrc/crown_node_search.hpp; nothing before its first call): the two frontiers and the two logs of
  // assignments, one block of doubles and one of ints, sized from max_nodes at the call; they only grow.  The node kernels' buffers
  // (reserve_nodes) are shared with nnsdp_crown_bound_nodes and hold one chunk
  DBuf<int8_t> nsby;
  DBuf<double> nsdb;
  DBuf<int> nsib;
  int* hnstatus = nullptr;               // pinned: the five integers of a level
  long long n_node_search = 0, n_node_levels = 0, n_node_downloads = 0;      // searches, status records read, levels whose points came back
  struct NodeLeaves {                    // closed leaves, then the open nodes, each in the order of the Python loop; assign acdim per row
    std::vector<int8_t> assign;
    std::vector<int32_t> depth, closed_by;      // closed_by: 0 infeasible, 1 bound, -1 open
    std::vector<double> bound;
    void clear() { assign.clear(); depth.clear(); closed_by.clear(); bound.clear(); }
    void add(int acdim, const int8_t* s, int d, int by, double bnd) {
      assign.insert(assign.end(), s, s + acdim);
      depth.push_back(d); closed_by.push_back(by); bound.push_back(bnd);
    }
  } nleaves_;

  size_t scr_per_box() const { return (size_t)(activ == NNSDP_ACTIV_TANH ? 6 : 2) * acdim; }
  nnsdp::CrownLayout layout(size_t nbox) const { return nnsdp::CrownLayout{nbox, (size_t)n0, (size_t)acdim, (size_t)ny, (size_t)nlit}; }
  size_t out_per_box() const { return layout(1).total(); }
  size_t ain_per_box() const { return 2 * (size_t)n0 + layout(1).nst(); }
  size_t aout_per_box() const { return layout(1).alpha_total(); }
  size_t ast_per_box() const { return 3 * layout(1).nst(); }
  nnsdp::CrownNodeLayout node_layout(size_t nnode) const { return nnsdp::CrownNodeLayout{nnode, (size_t)n0, (size_t)acdim, (size_t)nlit}; }
  bool wide() const { return max_width > nnsdp::kCbW; }
  size_t lds_bytes() const {
    if (wide()) return activ == NNSDP_ACTIV_TANH ? kCwLdsBytesTanh : kCwLdsBytes;
    return activ == NNSDP_ACTIV_TANH ? kCbLdsBytesTanh : kCbLdsBytes;
  }
  const void* kernel() const {
    if (wide())
      return activ == NNSDP_ACTIV_TANH ? reinterpret_cast<const void*>(&k_crown_wide<kCbTanh>)
                                       : reinterpret_cast<const void*>(&k_crown_wide<kCbRelu>);
    return activ == NNSDP_ACTIV_TANH ? reinterpret_cast<const void*>(&k_crown_resident<kCbTanh>)
                                     : reinterpret_cast<const void*>(&k_crown_resident<kCbRelu>);
  }
  void dalloc(DBuf<double>& b, size_t count) { b.alloc(count); if (count) ++n_alloc; }
  static void pinned(double*& h, size_t count) {
    if (h) { HIPCHK(hipHostFree(h)); h = nullptr; }
    if (count) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h), count * sizeof(double), hipHostMallocDefault));
  }
  size_t device_bytes() const {
    return dxd.bytes() + dao.bytes() + dmo.bytes() + dM.bytes() + din.bytes() + dscr.bytes() + dout.bytes() + dX.bytes() + dY.bytes() +
           dain.bytes() + daout.bytes() + dast.bytes() + dnin.bytes() + dnout.bytes() + dnst.bytes() + sbuf.bytes() + rbuf.bytes() + fbuf.bytes() +
           nsby.bytes() + nsdb.bytes() + nsib.bytes();
  }
  // the capacity grows geometrically and never shrinks
  // staging = false (a search: nothing of a box crosses the bus): the pinned copies wait for the next bound call
  // limit: the geometric growth stops there (a search: one chunk); a call that needs more still gets it
  void reserve_boxes(size_t nbox, bool staging = true, size_t limit = (size_t)-1) {
    if (nbox > box_cap) {
      const size_t cap = std::max(nbox, std::min(2 * box_cap, limit));
      dalloc(din, 2 * cap * n0); dalloc(dscr, cap * scr_per_box()); dalloc(dout, cap * out_per_box());
      box_cap = cap;
    }
    if (staging && pin_cap < box_cap) {
      pinned(hin, 2 * box_cap * n0); pinned(hout, box_cap * out_per_box());
      pin_cap = box_cap;
    }
  }
  // the buffers of the alpha calls; the scratch is the plain calls' (reserve_boxes)
  void reserve_alpha(size_t nbox) {
    reserve_boxes(nbox);
    if (nbox <= alpha_cap) return;
    if (!alpha_cap)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crown_alpha), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCoLdsBytes));
    const size_t cap = std::max(nbox, 2 * alpha_cap);
    dalloc(dain, cap * ain_per_box()); dalloc(daout, cap * aout_per_box()); dalloc(dast, cap * ast_per_box());
    pinned(hain, cap * ain_per_box()); pinned(haout, cap * aout_per_box());
    alpha_cap = cap;
  }
  // the buffers of the node calls: they share nothing with the box entries, whose scratch holds no clipped bounds
  void reserve_nodes(size_t nnode) {
    if (nnode <= node_cap) return;
    if (!node_cap) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crown_nodes), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCbLdsBytesTanh));
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crown_beta), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCoLdsBytes));
    }
    const size_t cap = std::max(nnode, 2 * node_cap);
    const nnsdp::CrownNodeLayout L = node_layout(cap);
    dalloc(dnin, L.in_doubles()); dalloc(dnout, L.total()); dalloc(dnst, 2 * L.nst());
    pinned(hnin, L.in_doubles()); pinned(hnout, L.total());
    node_cap = cap;
  }
  void reserve_samples(size_t N) {
    if (N <= sample_cap) return;
    const size_t cap = std::max(N, 2 * sample_cap);
    dalloc(dX, cap * n0); dalloc(dY, cap * ny);
    pinned(hX, cap * n0); pinned(hY, cap * ny);
    sample_cap = cap;
  }

  // the width refusals of the CROWN kernels (the one-shot entry and the handle)
  static void check_widths(int K, const int32_t* xdims) {
    for (int k = 0; k <= K; ++k) {
      if (xdims[k] < 1) throw std::invalid_argument("layer widths must be >= 1");
      if (xdims[k] > nnsdp::kCbW)
        throw std::invalid_argument("layer width " + std::to_string(xdims[k]) + " is above 64, the widest layer of the batched intervals");
    }
  }
  // the width refusals of nnsdp_crown_create_wide: max_width 64 is check_widths; 128 lets the hidden layers go up to 128
  static void check_widths_wide(int K, const int32_t* xdims, int max_width) {
    if (max_width != nnsdp::kCbW && max_width != nnsdp::kCwCols)
      throw std::invalid_argument("max_width must be 64 or 128, got " + std::to_string(max_width));
    if (max_width == nnsdp::kCbW) return check_widths(K, xdims);
    for (int k = 0; k <= K; ++k) {
      if (xdims[k] < 1) throw std::invalid_argument("layer widths must be >= 1");
      const bool end = k == 0 || k == K;
      if (end && xdims[k] > nnsdp::kCwRows)
        throw std::invalid_argument((k == 0 ? "input width " : "output width ") + std::to_string(xdims[k]) +
                                    " is above 64, the widest input and output of the wide bounder (only hidden layers go up to 128)");
      if (!end && xdims[k] > nnsdp::kCwCols)
        throw std::invalid_argument("layer width " + std::to_string(xdims[k]) + " is above 128, the widest hidden layer of the wide bounder");
    }
  }
  // M, then the literal head behind it, into dM (net.mlen() + net.head_len(nlit) doubles)
  static void upload_network(double* dM, const nnsdp::NetLayout& net, const int32_t* xdims, const double* M, int nlit, const double* normals) {
    HIPCHK(hipMemcpy(dM, M, net.mlen() * sizeof(double), hipMemcpyHostToDevice));
    if (nlit > 0) {
      const nnsdp::LitHead head = nnsdp::make_lit_head(net.K(), xdims, M, nlit, normals);
      HIPCHK(hipMemcpy(dM + net.mlen(), head.H.data(), net.head_len(nlit) * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  void create(int K_, const int32_t* xdims, const double* M, int activ_, int nlit_, const double* normals_, int max_width_ = nnsdp::kCbW) {
    const nnsdp::NetLayout net(K_, xdims);
    max_width = max_width_;
    K = K_; activ = activ_; nlit = nlit_; acdim = net.acdim(); n0 = net.n0(); ny = net.ny(); wp = net.wp; moff = net.moff;
    if (nlit > 0) normals.assign(normals_, normals_ + (size_t)nlit * ny);
    dxd.upload(net.xd); dao.upload(net.acoff); dmo.upload(net.moff);
    dM.alloc(net.mlen() + net.head_len(nlit));
    n_alloc += 4;
    upload_network(dM.p, net, xdims, M, nlit, normals_);
    ++n_upload;
    // (k_forward_mfma needs no attribute here: widths <= 128 keep its LDS at 2 * 132 * 16 doubles, 33.8 KB)
    HIPCHK(hipFuncSetAttribute(kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes()));
    HIPCHK(hipStreamCreate(&st));
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  }

  // the bound kernel's arguments for the boxes lo / hi of layout L, outputs at `out` (L.total() doubles); the scratch is dscr
  nnsdp::CrownArgs bound_args(const nnsdp::CrownLayout& L, const double* lo, const double* hi, double* out) const {
    nnsdp::CrownArgs a;
    a.K = K; a.xdims = dxd.p; a.moff = dmo.p; a.acoff = dao.p; a.M = dM.p; a.H = dM.p + moff[K];
    a.lo = lo; a.hi = hi; a.scratch = dscr.p;
    L.point(a, out);
    return a;
  }
  void launch_bound(const nnsdp::CrownArgs& a, size_t nbox) {
    if (wide() && activ == NNSDP_ACTIV_TANH)
      hipLaunchKernelGGL(nnsdp::k_crown_wide<nnsdp::kCbTanh>, dim3((unsigned)nbox), dim3(256), nnsdp::kCwLdsBytesTanh, st, a);
    else if (wide())
      hipLaunchKernelGGL(nnsdp::k_crown_wide<nnsdp::kCbRelu>, dim3((unsigned)nbox), dim3(256), nnsdp::kCwLdsBytes, st, a);
    else if (activ == NNSDP_ACTIV_TANH)
      hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbTanh>, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytesTanh, st, a);
    else
      hipLaunchKernelGGL(nnsdp::k_crown_resident<nnsdp::kCbRelu>, dim3((unsigned)nbox), dim3(256), nnsdp::kCbLdsBytes, st, a);
    HIPCHK(hipGetLastError());
  }
  // the sampled forward pass of the handle's network on its stream: Y = f(X) at N points
  void launch_forward(const double* X, double* Y, long long N) {
    nnsdp::launch_forward(K, dxd.p, dmo.p, dM.p, X, Y, N, activ, wp, st);
    HIPCHK(hipGetLastError());
  }
  float elapsed_ms() {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  }

  // nnsdp_crown_bound; host: the caller's ten output arrays in the order of CrownLayout (null: not wanted)
  void bound(int32_t nbox, const double* x1min, const double* x1max, double* const host[nnsdp::CrownLayout::kSegs], double* kernel_ms) {
    if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
    if (nbox == 0) return;
    if (!x1min || !x1max) throw std::invalid_argument("null argument");
    nnsdp::check_boxes(nbox, n0, x1min, x1max);
    const nnsdp::CrownLayout L = layout((size_t)nbox);
    const size_t nin = L.nbox * n0;
    reserve_boxes(L.nbox);
    std::copy(x1min, x1min + nin, hin);
    std::copy(x1max, x1max + nin, hin + nin);
    HIPCHK(hipMemcpyAsync(din.p, hin, 2 * nin * sizeof(double), hipMemcpyHostToDevice, st));
    const nnsdp::CrownArgs a = bound_args(L, din.p, din.p + nin, dout.p);
    HIPCHK(hipEventRecord(e0, st));
    launch_bound(a, L.nbox);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(hout, dout.p, L.total() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ++n_bound;
    const float ms = elapsed_ms();
    if (kernel_ms) *kernel_ms = ms;
    size_t len[nnsdp::CrownLayout::kSegs];
    L.lens(len);
    nnsdp::CrownLayout::copy_segments(hout, nnsdp::CrownLayout::kSegs, len, host);
  }

  // nnsdp_crown_bound_alpha: bound(), then the slope iteration on the same boxes in the same launch sequence
  void bound_alpha(int32_t nbox, const double* x1min, const double* x1max, double* const host[nnsdp::CrownLayout::kSegs], double* kernel_ms,
                   int32_t steps, double eta0, double decay, const double* alpha0,
                   double* a_smax, double* a_uA, double* a_ub0, double* alpha, int32_t* best_step) {
    if (wide()) throw std::invalid_argument("optimised slopes (alpha) are not available on a wide bounder (max_width 128): the alpha kernel keeps a 64-wide layout");
    if (activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("optimised slopes (alpha) are for ReLU networks, not Tanh");
    if (nlit < 1) throw std::invalid_argument("optimised slopes (alpha) need literals: the handle was created without normals");
    check_pg_options("alpha", steps, eta0, decay);
    if (nbox < 0) throw std::invalid_argument("nbox must be >= 0");
    if (nbox == 0) return;
    if (!x1min || !x1max) throw std::invalid_argument("null argument");
    nnsdp::check_boxes(nbox, n0, x1min, x1max);
    constexpr int kSegs = nnsdp::CrownLayout::kSegs;
    const nnsdp::CrownLayout L = layout((size_t)nbox);
    const size_t nin = L.nbox * n0, nl_all = L.nl(), nA_all = L.nA(), nst_all = L.nst();
    if (alpha0) check_alpha0(alpha0, nst_all);
    reserve_alpha(L.nbox);
    // one upload: the boxes, then alpha0 when there is one
    std::copy(x1min, x1min + nin, hain);
    std::copy(x1max, x1max + nin, hain + nin);
    if (alpha0) std::copy(alpha0, alpha0 + nst_all, hain + 2 * nin);
    HIPCHK(hipMemcpyAsync(dain.p, hain, (2 * nin + (alpha0 ? nst_all : 0)) * sizeof(double), hipMemcpyHostToDevice, st));
    nnsdp::CrownAlphaArgs p;
    p.o.c = bound_args(L, dain.p, dain.p + nin, daout.p);
    p.o.steps = steps; p.o.eta0 = eta0; p.o.decay = decay; p.alpha0 = alpha0 ? dain.p + 2 * nin : nullptr;
    p.o.cur = dast.p; p.o.lam = p.o.cur + nst_all; p.best = p.o.lam + nst_all;
    p.o.smax = daout.p + L.total(); p.o.ub0 = p.o.smax + nl_all; p.o.step = p.o.ub0 + nl_all; p.o.uA = p.o.step + nl_all; p.alpha = p.o.uA + nA_all;
    HIPCHK(hipEventRecord(e0, st));
    launch_bound(p.o.c, L.nbox);
    hipLaunchKernelGGL(nnsdp::k_crown_alpha, dim3((unsigned)nbox), dim3(256), nnsdp::kCoLdsBytes, st, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(haout, daout.p, L.alpha_total() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ++n_bound;
    const float ms = elapsed_ms();
    if (kernel_ms) *kernel_ms = ms;
    // the plain segments, then a_smax | a_ub0 | a_step (doubles on the device, int32 for the caller) | a_uA | alpha
    size_t len[kSegs + 5];
    L.lens(len);
    len[kSegs] = len[kSegs + 1] = len[kSegs + 2] = nl_all; len[kSegs + 3] = nA_all; len[kSegs + 4] = nst_all;
    double* all[kSegs + 5];
    std::copy(host, host + kSegs, all);
    all[kSegs] = a_smax; all[kSegs + 1] = a_ub0; all[kSegs + 2] = nullptr; all[kSegs + 3] = a_uA; all[kSegs + 4] = alpha;
    nnsdp::CrownLayout::copy_segments(haout, kSegs + 5, len, all);
    if (best_step) {
      const double* step = haout + L.total() + 2 * nl_all;
      for (size_t k = 0; k < nl_all; ++k) best_step[k] = (int32_t)step[k];
    }
  }

  // nnsdp_crown_bound_nodes (csrc/crown_relu_split.hpp).  h may be null: the scalar options come first so that their refusals can be
  // tested on a machine without a GPU, where no handle exists
  struct NodeOut {
    double *pre_lo, *pre_hi, *smin, *smax_plain, *smax, *uA, *ub0;
    int32_t *best_step, *branch, *infeasible;
    double* kernel_ms;
  };
  static void bound_nodes(nnsdp_crown* h, int32_t nnode, const double* x1min, const double* x1max, const int8_t* assign, int32_t steps,
                          double eta0, double decay, const NodeOut& out) {
    check_pg_options("nodes", steps, eta0, decay);
    if (!h) throw std::invalid_argument("null handle");
    if (h->wide()) throw std::invalid_argument("a ReLU split is not available on a wide bounder (max_width 128): the node kernels keep a 64-wide layout");
    if (h->activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("a ReLU split is for ReLU networks, not Tanh");
    if (h->nlit < 1) throw std::invalid_argument("a ReLU split needs literals: the handle was created without normals");
    if (nnode < 0) throw std::invalid_argument("nnode must be >= 0");
    if (nnode == 0) return;
    if (!x1min || !x1max || !assign) throw std::invalid_argument("null argument");
    const int n0 = h->n0, acdim = h->acdim;
    nnsdp::check_boxes(nnode, n0, x1min, x1max);
    check_assign(assign, (size_t)nnode * acdim);
    const nnsdp::CrownNodeLayout L = h->node_layout((size_t)nnode);
    const size_t nin = L.nnode * n0, nl = L.nl();
    h->reserve_nodes(L.nnode);
    // one upload: the boxes, then the assignments as bytes
    std::copy(x1min, x1min + nin, h->hnin);
    std::copy(x1max, x1max + nin, h->hnin + nin);
    int8_t* hasg = reinterpret_cast<int8_t*>(h->hnin + 2 * nin);
    std::copy(assign, assign + L.nnode * acdim, hasg);
    hipStream_t st = h->st;
    HIPCHK(hipMemcpyAsync(h->dnin.p, h->hnin, 2 * nin * sizeof(double) + L.nnode * acdim, hipMemcpyHostToDevice, st));
    const nnsdp::CrownNodeArgs p = h->node_args(L, h->dnin.p, h->dnin.p + nin, reinterpret_cast<const int8_t*>(h->dnin.p + 2 * nin), steps, eta0, decay);
    HIPCHK(hipEventRecord(h->e0, st));
    h->launch_nodes(p, L.nnode);
    HIPCHK(hipEventRecord(h->e1, st));
    HIPCHK(hipMemcpyAsync(h->hnout, h->dnout.p, L.total() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ++h->n_bound;
    const float ms = h->elapsed_ms();
    if (out.kernel_ms) *out.kernel_ms = ms;
    const double* src = h->hnout;
    for (size_t b = 0; b < L.nnode; ++b, src += 2 * acdim) {
      if (out.pre_lo) std::copy(src, src + acdim, out.pre_lo + b * acdim);
      if (out.pre_hi) std::copy(src + acdim, src + 2 * acdim, out.pre_hi + b * acdim);
    }
    auto ints = [](const double* s, size_t n, int32_t* dst) {
      if (dst) for (size_t k = 0; k < n; ++k) dst[k] = (int32_t)s[k];
    };
    double* const dbl[4] = {out.smin, out.smax_plain, out.smax, out.ub0};
    for (int o = 0; o < 4; ++o, src += nl)
      if (dbl[o]) std::copy(src, src + nl, dbl[o]);
    ints(src, nl, out.best_step); src += nl;
    ints(src, nl, out.branch); src += nl;
    if (out.uA) std::copy(src, src + L.nA(), out.uA);
    src += L.nA();
    ints(src, L.nnode, out.infeasible);
  }

  // the node kernels' arguments for the nodes lo / hi / assign of layout L: outputs in dnout, multiplier state in dnst (reserve_nodes)
  nnsdp::CrownNodeArgs node_args(const nnsdp::CrownNodeLayout& L, const double* lo, const double* hi, const int8_t* assign, int32_t steps,
                                 double eta0, double decay) const {
    nnsdp::CrownNodeArgs p;
    p.o.c.K = K; p.o.c.xdims = dxd.p; p.o.c.moff = dmo.p; p.o.c.acoff = dao.p; p.o.c.M = dM.p; p.o.c.H = dM.p + moff[K];
    p.o.c.lo = lo; p.o.c.hi = hi;
    p.sp.assign = assign; p.sp.infeasible = 0;
    L.point(p, dnout.p);
    p.o.steps = steps; p.o.eta0 = eta0; p.o.decay = decay;
    p.o.cur = dnst.p; p.o.lam = p.o.cur + L.nst();
    return p;
  }
  // the one place that launches the two node kernels (nnsdp_crown_bound_nodes, and every chunk of nnsdp_crown_search_nodes)
  void launch_nodes(const nnsdp::CrownNodeArgs& p, size_t nnode) {
    hipLaunchKernelGGL(nnsdp::k_crown_nodes, dim3((unsigned)nnode), dim3(256), nnsdp::kCbLdsBytesTanh, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(nnsdp::k_crown_beta, dim3((unsigned)nnode), dim3(256), nnsdp::kCoLdsBytes, st, p);
    HIPCHK(hipGetLastError());
  }

  // nnsdp_crown_eval
  void eval(int64_t N, const double* X, double* Y, double* kernel_ms) {
    if (N < 0) throw std::invalid_argument("N must be >= 0");
    if (N == 0) return;
    if (!X || !Y) throw std::invalid_argument("null argument");
    if ((N + 15) / 16 > 0x7fffffffLL) throw std::invalid_argument("too many samples for one launch");
    const size_t nx = (size_t)n0 * N, nyN = (size_t)ny * N;
    reserve_samples((size_t)N);
    std::copy(X, X + nx, hX);
    HIPCHK(hipMemcpyAsync(dX.p, hX, nx * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    launch_forward(dX.p, dY.p, N);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(hY, dY.p, nyN * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const float ms = elapsed_ms();
    if (kernel_ms) *kernel_ms = ms;
    std::copy(hY, hY + nyN, Y);
  }

  // The frontier searches, defined in csrc/crown_frontier_host.hpp.  h may be null: the scalar options come first so that their
  // refusals can be tested on a machine without a GPU, where no handle exists
  static void search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                     int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                     nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                     int32_t* nleaves, double* witness, double* kernel_ms);
  static nnsdp::ForestPlan forest_group_plan(int n0, int ny, int nlit, int32_t max_boxes, int32_t corner_points, int32_t nroot, int32_t group);
  static void search_many(nnsdp_crown* h, int32_t nroot, const double* x1min, const double* x1max, int32_t nlit, const double* normals,
                          const double* hs, int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                          int32_t group, nnsdp_confirm_many_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                          int32_t* nleaves, double* witness, double* kernel_ms);
  static void reach(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* tol, int32_t corner_points,
                    int32_t max_boxes, int32_t max_depth, int32_t chunk, int32_t* status, int32_t* visited, int32_t* depth_reached,
                    int32_t* nleaves, double* incumbent, double* witnesses, double* kernel_ms);
  static void search_nodes(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* hs, int32_t steps, double eta0,
                           double decay, int32_t corner_points, int32_t max_nodes, int32_t max_depth, int32_t chunk, nnsdp_confirm_fn confirm,
                           void* user, int32_t* verdict, int32_t* reason, int32_t* visited, int32_t* depth_reached, int32_t* nleaves,
                           int32_t* nopen, double* witness, double* kernel_ms);

  ~nnsdp_crown() {
    if (st) (void)hipStreamSynchronize(st);
    for (double* h : {hin, hout, hX, hY, hain, haout, hnin, hnout}) if (h) (void)hipHostFree(h);
    if (hstatus) (void)hipHostFree(hstatus);
    if (hforest) (void)hipHostFree(hforest);
    if (hnstatus) (void)hipHostFree(hnstatus);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
};
