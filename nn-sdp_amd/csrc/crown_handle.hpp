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

// the options of the alpha entries
static void check_alpha_options(int32_t steps, double eta0, double decay) {
  if (steps < 0 || steps > 64) throw std::invalid_argument("alpha: steps must be in 0..64, got " + std::to_string(steps));
  if (!std::isfinite(eta0) || !(eta0 > 0.0)) throw std::invalid_argument("alpha: eta0 must be positive and finite");
  if (!(decay > 0.0 && decay <= 1.0)) throw std::invalid_argument("alpha: decay must be in (0, 1]");
}
static void check_alpha0(const double* alpha0, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(alpha0[k])) throw std::invalid_argument("alpha0 has a non-finite entry (NaN or infinity) at index " + std::to_string(k));
}

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
  size_t box_cap = 0, pin_cap = 0, sample_cap = 0, alpha_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  long long n_alloc = 0, n_upload = 0, n_bound = 0;
  // nnsdp_crown_search only (nothing before its first call): the two frontiers (lo and hi of both, then the cuts of both), the
  // per-level records / points / leaf log / clause, the status record's pinned copy; the result of the last search
  std::vector<double> normals;           // the literals of the handle (ny x nlit), kept for the proof test of the search
  DBuf<double> sfr, sdb;
  DBuf<int> scu, sib;
  int* hstatus = nullptr;
  struct SearchLeaves {                  // flat, in the order of the Python loop; lo / hi n0 x nleaves column-major
    std::vector<double> lo, hi, bound;
    std::vector<int32_t> depth, proved, literal;
    void clear() { lo.clear(); hi.clear(); bound.clear(); depth.clear(); proved.clear(); literal.clear(); }
  } leaves;
  // nnsdp_crown_reach only (nothing before its first call): its own two frontiers, records / points / leaf log / incumbents, sized from
  // max_boxes at the first call; the bound kernel's buffers and the status record's pinned copy are the ones the search uses
  DBuf<double> rfr, rdb;
  DBuf<int> rcu, rib;
  long long n_reach = 0;
  struct ReachLeaves {                   // flat, in the order of the Python loop; lo / hi n0 x nleaves, bound nlit x nleaves column-major
    std::vector<double> lo, hi, bound;
    std::vector<int32_t> depth, closed;
    void clear() { lo.clear(); hi.clear(); bound.clear(); depth.clear(); closed.clear(); }
  } rleaves;
  // nnsdp_crown_search_many only (nothing before its first call): the two frontiers of a group of roots with the root of every box, the
  // records / points / leaf logs / per-root tables (csrc/crown_forest.hpp, ForestPlan), the pinned copy of a level's table and counts;
  // the leaves of the last call, per root
  DBuf<double> ffr, fdb;
  DBuf<int> fcu, fib;
  int* hforest = nullptr;
  size_t hforest_cap = 0;
  std::vector<SearchLeaves> fleaves;

  size_t scr_per_box() const { return (size_t)(activ == NNSDP_ACTIV_TANH ? 6 : 2) * acdim; }
  nnsdp::CrownLayout layout(size_t nbox) const { return nnsdp::CrownLayout{nbox, (size_t)n0, (size_t)acdim, (size_t)ny, (size_t)nlit}; }
  size_t out_per_box() const { return layout(1).total(); }
  size_t ain_per_box() const { return 2 * (size_t)n0 + layout(1).nst(); }
  size_t aout_per_box() const { return layout(1).alpha_total(); }
  size_t ast_per_box() const { return 3 * layout(1).nst(); }
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
           dain.bytes() + daout.bytes() + dast.bytes() + sfr.bytes() + sdb.bytes() + scu.bytes() + sib.bytes() +
           rfr.bytes() + rdb.bytes() + rcu.bytes() + rib.bytes() + ffr.bytes() + fdb.bytes() + fcu.bytes() + fib.bytes();
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
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crown_alpha), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCaLdsBytes));
    const size_t cap = std::max(nbox, 2 * alpha_cap);
    dalloc(dain, cap * ain_per_box()); dalloc(daout, cap * aout_per_box()); dalloc(dast, cap * ast_per_box());
    pinned(hain, cap * ain_per_box()); pinned(haout, cap * aout_per_box());
    alpha_cap = cap;
  }
  // the buffers of a search: frontiers of `cap` boxes each, `nd` doubles and `ni` ints of records; they only grow
  void reserve_search(size_t cap, size_t nd, size_t ni) {
    if (4 * cap * n0 > sfr.n) { dalloc(sfr, 4 * cap * n0); scu.alloc(2 * cap * n0); ++n_alloc; }
    if (nd > sdb.n) dalloc(sdb, nd);
    if (ni > sib.n) { sib.alloc(ni); ++n_alloc; }
    if (!hstatus) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hstatus), 4 * sizeof(int), hipHostMallocDefault));
  }
  // the buffers of a reach search: frontiers of `cap` boxes each, `nd` doubles and `ni` ints of records; they only grow
  void reserve_reach(size_t cap, size_t nd, size_t ni) {
    if (4 * cap * n0 > rfr.n) { dalloc(rfr, 4 * cap * n0); rcu.alloc(2 * cap * n0); ++n_alloc; }
    if (nd > rdb.n) dalloc(rdb, nd);
    if (ni > rib.n) { rib.alloc(ni); ++n_alloc; }
    if (!hstatus) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hstatus), 4 * sizeof(int), hipHostMallocDefault));
  }
  // the buffers of a forest search (one group of roots): they only grow
  void reserve_forest(const nnsdp::ForestPlan& p) {
    if (4 * p.cap * n0 > ffr.n) dalloc(ffr, 4 * p.cap * n0);
    if (2 * p.cap * (n0 + 1) > fcu.n) { fcu.alloc(2 * p.cap * (n0 + 1)); ++n_alloc; }
    if (p.nd > fdb.n) dalloc(fdb, p.nd);
    if (p.ni > fib.n) { fib.alloc(p.ni); ++n_alloc; }
    if (8 * p.group > hforest_cap) {
      if (hforest) { HIPCHK(hipHostFree(hforest)); hforest = nullptr; }
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hforest), 8 * p.group * sizeof(int), hipHostMallocDefault));
      hforest_cap = 8 * p.group;
    }
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
    check_alpha_options(steps, eta0, decay);
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
    p.c = bound_args(L, dain.p, dain.p + nin, daout.p);
    p.steps = steps; p.eta0 = eta0; p.decay = decay; p.alpha0 = alpha0 ? dain.p + 2 * nin : nullptr;
    p.cur = dast.p; p.lam = p.cur + nst_all; p.best = p.lam + nst_all;
    p.a_smax = daout.p + L.total(); p.a_ub0 = p.a_smax + nl_all; p.a_step = p.a_ub0 + nl_all; p.a_uA = p.a_step + nl_all; p.alpha = p.a_uA + nA_all;
    HIPCHK(hipEventRecord(e0, st));
    launch_bound(p.c, L.nbox);
    hipLaunchKernelGGL(nnsdp::k_crown_alpha, dim3((unsigned)nbox), dim3(256), nnsdp::kCaLdsBytes, st, p);
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

  // nnsdp_crown_search.  h may be null: the scalar options come first so that their refusals can be tested on a machine without a GPU,
  // where no handle exists
  static void search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                     int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                     nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                     int32_t* nleaves, double* witness, double* kernel_ms) {
    if (max_boxes < 1) throw std::invalid_argument("max_boxes must be >= 1, got " + std::to_string(max_boxes));
    if (chunk < 1) throw std::invalid_argument("chunk must be >= 1, got " + std::to_string(chunk));
    if (max_depth < 0) throw std::invalid_argument("max_depth must be >= 0, got " + std::to_string(max_depth));
    if (!h) throw std::invalid_argument("null handle");
    if (!x1min || !x1max || !hs || !verdict || !visited || !depth_reached || !nleaves || !witness) throw std::invalid_argument("null argument");
    const int n0 = h->n0, ny = h->ny;
    if (h->nlit > 0) {
      if (normals) throw std::invalid_argument("the handle has literals of its own: normals must be NULL");
      if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
      normals = h->normals.data();
    } else {
      if (literal_bounds) throw std::invalid_argument("literal_bounds needs literals: the handle was created without normals");
      if (corner_points) throw std::invalid_argument("corner_points needs literals: the handle was created without normals");
      if (nlit < 1) throw std::invalid_argument("a clause needs at least one literal (nlit >= 1)");
      check_literals(ny, nlit, normals);
    }
    for (int i = 0; i < nlit; ++i)
      if (!std::isfinite(hs[i])) throw std::invalid_argument("literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
    unsigned long long splitmask = 0;
    for (int t = 0; t < n0; ++t) {
      if (!std::isfinite(x1min[t]) || !std::isfinite(x1max[t]) || !(x1min[t] <= x1max[t]))
        throw std::invalid_argument("the root box: x1min must be <= x1max and both finite (no NaN, no infinity)");
      if (x1max[t] > x1min[t]) splitmask |= 1ull << t;
    }
    // a level bounds at most max_boxes boxes and its children number at most twice that
    const size_t mb = (size_t)max_boxes, cap = 2 * mb, npmax = corner_points ? 2 * mb : mb, logw = 2 * (size_t)n0 + 3;
    const size_t frontier_bytes = 2 * cap * n0 * (2 * sizeof(double) + sizeof(int));
    if (frontier_bytes > nnsdp::kSearchFrontierCap)
      throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(frontier_bytes) +
                                  " bytes of frontier buffers, above the cap of 2^31 bytes");
    // doubles: bound, points in, points out, leaf log, normals, hs;  ints: open, best, coord, slot, point flags, status
    const size_t o_bound = 0, o_X = o_bound + mb, o_Y = o_X + npmax * n0, o_log = o_Y + npmax * ny, o_nrm = o_log + mb * logw,
                 o_hs = o_nrm + (size_t)nlit * ny, nd = o_hs + nlit;
    const size_t ni = 4 * mb + npmax + 4;
    const size_t cb = std::min((size_t)chunk, mb);
    h->leaves.clear();
    h->reserve_search(cap, nd, ni);
    hipStream_t st = h->st;
    double* D = h->sdb.p;
    int* I = h->sib.p;
    double *flo[2] = {h->sfr.p, h->sfr.p + 2 * cap * n0}, *fhi[2] = {flo[0] + cap * n0, flo[1] + cap * n0};
    int* fcu[2] = {h->scu.p, h->scu.p + cap * n0};
    HIPCHK(hipMemcpyAsync(flo[0], x1min, n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(fhi[0], x1max, n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(fcu[0], 0, n0 * sizeof(int), st));
    HIPCHK(hipMemcpyAsync(D + o_nrm, normals, (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(D + o_hs, hs, nlit * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));      // (the sources are the caller's pageable arrays)

    nnsdp::SearchArgs s;
    s.n0 = n0; s.ny = ny; s.nlit = nlit; s.literal_bounds = literal_bounds != 0; s.corner_points = corner_points != 0;
    s.splitmask = splitmask; s.normals = D + o_nrm; s.hs = D + o_hs;
    s.open = I; s.best = I + mb; s.coord = I + 2 * mb; s.slot = I + 3 * mb; s.pflag = I + 4 * mb; s.status = I + 4 * mb + npmax;
    s.bound = D + o_bound; s.X = D + o_X; s.Y = D + o_Y; s.log = D + o_log;

    int cur = 0, nlevel = 1, nb = 0, vis = 0, depth = 0, verd = -1;
    long long log_n = 0, log_before = 0;
    double ms_all = 0.0;
    std::vector<double> wit;
    for (;;) {
      nb = std::min(nlevel, max_boxes - vis);      // (>= 1: a level that uses the budget up is the last one)
      vis += nb;
      log_before = log_n;
      h->reserve_boxes(std::min(cb, (size_t)nb), false, cb);      // (the stream is idle here: the bound kernel's buffers grow with the levels)
      s.nb = nb; s.depth = depth; s.lo = flo[cur]; s.hi = fhi[cur]; s.cuts = fcu[cur];
      s.nlo = flo[cur ^ 1]; s.nhi = fhi[cur ^ 1]; s.ncuts = fcu[cur ^ 1]; s.log_base = log_n;
      HIPCHK(hipEventRecord(h->e0, st));
      for (int off = 0; off < nb; off += (int)cb) {
        const size_t nc = std::min(cb, (size_t)(nb - off));
        // (per chunk: reserve_boxes may have moved the scratch and the outputs)
        const nnsdp::CrownArgs a = h->bound_args(h->layout(nc), flo[cur] + (size_t)off * n0, fhi[cur] + (size_t)off * n0, h->dout.p);
        h->launch_bound(a, nc);
        hipLaunchKernelGGL(nnsdp::k_search_classify, dim3((unsigned)cdiv((long long)nc, 256)), dim3(256), 0, st, s, off, (int)nc,
                           (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
        HIPCHK(hipGetLastError());
        ++h->n_bound;
      }
      const long long npts = (long long)nb * (corner_points ? 2 : 1);
      h->launch_forward(s.X, D + o_Y, npts);
      hipLaunchKernelGGL(nnsdp::k_search_refute, dim3((unsigned)cdiv(npts, 256)), dim3(256), 0, st, s, npts);
      HIPCHK(hipGetLastError());
      const bool stop = vis >= max_boxes || depth >= max_depth || splitmask == 0;
      hipLaunchKernelGGL(nnsdp::k_search_scan, dim3(1), dim3(256), 0, st, s, npts);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(nnsdp::k_search_scatter, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, s, stop ? 0 : 1);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(h->e1, st));
      HIPCHK(hipMemcpyAsync(h->hstatus, s.status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      ms_all += h->elapsed_ms();
      const int nproved = h->hstatus[1], nopen = h->hstatus[2], ncand = h->hstatus[3];
      if (h->hstatus[0] != nb || nproved + nopen != nb) throw std::runtime_error("nnsdp_crown_search: inconsistent status record");
      log_n += nproved;
      if (ncand > 0) {      // the level's flags and points, walked in the Python driver's order: the centres in box order, then the corners
        std::vector<int> pf((size_t)npts);
        std::vector<double> X((size_t)npts * n0);
        HIPCHK(hipMemcpy(pf.data(), s.pflag, pf.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(X.data(), s.X, X.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (long long p = 0; p < npts && wit.empty(); ++p)
          if (pf[(size_t)p] && (!confirm || confirm(user, X.data() + (size_t)p * n0) != 0)) wit.assign(X.begin() + (size_t)p * n0, X.begin() + (size_t)(p + 1) * n0);
      }
      if (!wit.empty()) { verd = 1; break; }
      if (nopen == 0) { verd = nb < nlevel ? 2 : 0; break; }
      if (stop) { verd = 2; break; }
      cur ^= 1; nlevel = 2 * nopen; ++depth;
    }
    // the leaves in the order of the Python loop: the log up to the last level, the boxes of the last level that the budget kept from
    // being bounded, the last level's proved boxes, its open boxes
    std::vector<double> log((size_t)log_n * logw), lo((size_t)nlevel * n0), hi((size_t)nlevel * n0), bnd((size_t)nb);
    std::vector<int> open((size_t)nb), best((size_t)nb);
    if (log_n) HIPCHK(hipMemcpy(log.data(), s.log, log.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lo.data(), flo[cur], lo.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hi.data(), fhi[cur], hi.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(bnd.data(), s.bound, bnd.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(open.data(), s.open, open.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(best.data(), s.best, best.size() * sizeof(int), hipMemcpyDeviceToHost));
    SearchLeaves& L = h->leaves;
    const size_t nleaf = (size_t)log_n + (size_t)(nlevel - nb) + (size_t)h->hstatus[2];
    L.lo.reserve(nleaf * n0); L.hi.reserve(nleaf * n0); L.depth.reserve(nleaf); L.proved.reserve(nleaf); L.literal.reserve(nleaf); L.bound.reserve(nleaf);
    auto leaf = [&](const double* blo, const double* bhi, int d, int proved, int literal, double bound) {
      L.lo.insert(L.lo.end(), blo, blo + n0); L.hi.insert(L.hi.end(), bhi, bhi + n0);
      L.depth.push_back(d); L.proved.push_back(proved); L.literal.push_back(literal); L.bound.push_back(bound);
    };
    auto from_log = [&](long long r) {
      const double* row = log.data() + (size_t)r * logw;
      leaf(row, row + n0, (int)row[2 * n0], 1, (int)row[2 * n0 + 1], row[2 * n0 + 2]);
    };
    auto from_frontier = [&](int b, int literal, double bound) { leaf(lo.data() + (size_t)b * n0, hi.data() + (size_t)b * n0, depth, 0, literal, bound); };
    for (long long r = 0; r < log_before; ++r) from_log(r);
    for (int b = nb; b < nlevel; ++b) from_frontier(b, -1, 0.0);
    for (long long r = log_before; r < log_n; ++r) from_log(r);
    for (int b = 0; b < nb; ++b)
      if (open[b]) from_frontier(b, best[b], bnd[b]);
    *verdict = verd; *visited = vis; *depth_reached = depth; *nleaves = (int32_t)L.depth.size();
    if (verd == 1) std::copy(wit.begin(), wit.end(), witness);
    if (kernel_ms) *kernel_ms = ms_all;
  }

  // the group size of nnsdp_crown_search_many and its refusal (nnsdp_crown_forest_plan enumerates it without a handle)
  static nnsdp::ForestPlan forest_group_plan(int n0, int ny, int nlit, int32_t max_boxes, int32_t corner_points, int32_t nroot, int32_t group) {
    const size_t limit = std::max<size_t>(1, group > 0 ? std::min<size_t>((size_t)group, (size_t)nroot) : (size_t)nroot);
    const size_t g = nnsdp::forest_group((size_t)n0, (size_t)ny, (size_t)nlit, (size_t)max_boxes, corner_points != 0, limit);
    if (!g) {
      const nnsdp::ForestPlan one = nnsdp::forest_plan((size_t)n0, (size_t)ny, (size_t)nlit, (size_t)max_boxes, corner_points != 0, 1);
      const bool fr = one.frontier_bytes > nnsdp::kSearchFrontierCap, db = !fr && one.double_bytes > nnsdp::kSearchFrontierCap;
      throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " +
                                  std::to_string(fr ? one.frontier_bytes : db ? one.double_bytes : one.int_bytes) + " bytes of " +
                                  (fr ? "frontier" : db ? "point and leaf-log" : "record") + " buffers for one root, above the cap of 2^31 bytes");
    }
    return nnsdp::forest_plan((size_t)n0, (size_t)ny, (size_t)nlit, (size_t)max_boxes, corner_points != 0, g);
  }

  // nnsdp_crown_search_many: search() for nroot root boxes with thresholds of their own in one level loop (csrc/crown_forest.hpp); per
  // root the result of search().  h may be null: the scalar options come first, as in search()
  static void search_many(nnsdp_crown* h, int32_t nroot, const double* x1min, const double* x1max, int32_t nlit, const double* normals,
                          const double* hs, int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                          int32_t group, nnsdp_confirm_many_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                          int32_t* nleaves, double* witness, double* kernel_ms) {
    if (max_boxes < 1) throw std::invalid_argument("max_boxes must be >= 1, got " + std::to_string(max_boxes));
    if (chunk < 1) throw std::invalid_argument("chunk must be >= 1, got " + std::to_string(chunk));
    if (max_depth < 0) throw std::invalid_argument("max_depth must be >= 0, got " + std::to_string(max_depth));
    if (group < 0) throw std::invalid_argument("group must be >= 0 (0: derived from the memory cap), got " + std::to_string(group));
    if (nroot < 0) throw std::invalid_argument("nroot must be >= 0, got " + std::to_string(nroot));
    if (kernel_ms) *kernel_ms = 0.0;
    if (nroot == 0) {
      if (h) h->fleaves.clear();
      return;
    }
    if (!h) throw std::invalid_argument("null handle");
    if (!x1min || !x1max || !hs || !verdict || !visited || !depth_reached || !nleaves || !witness) throw std::invalid_argument("null argument");
    const int n0 = h->n0, ny = h->ny;
    if (h->nlit > 0) {
      if (normals) throw std::invalid_argument("the handle has literals of its own: normals must be NULL");
      if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
      normals = h->normals.data();
    } else {
      if (literal_bounds) throw std::invalid_argument("literal_bounds needs literals: the handle was created without normals");
      if (corner_points) throw std::invalid_argument("corner_points needs literals: the handle was created without normals");
      if (nlit < 1) throw std::invalid_argument("a clause needs at least one literal (nlit >= 1)");
      check_literals(ny, nlit, normals);
    }
    std::vector<unsigned long long> masks((size_t)nroot, 0);
    for (int r = 0; r < nroot; ++r) {
      for (int i = 0; i < nlit; ++i)
        if (!std::isfinite(hs[(size_t)r * nlit + i]))
          throw std::invalid_argument("root " + std::to_string(r) + ", literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
      for (int t = 0; t < n0; ++t) {
        const double l = x1min[(size_t)r * n0 + t], u = x1max[(size_t)r * n0 + t];
        if (!std::isfinite(l) || !std::isfinite(u) || !(l <= u))
          throw std::invalid_argument("root " + std::to_string(r) + ": x1min must be <= x1max and both finite (no NaN, no infinity)");
        if (u > l) masks[(size_t)r] |= 1ull << t;
      }
    }
    const nnsdp::ForestPlan P = forest_group_plan(n0, ny, nlit, max_boxes, corner_points, nroot, group);
    const size_t G = P.group, cap = P.cap, logw = P.logw;
    const size_t cb = std::min((size_t)chunk, cap);
    h->fleaves.assign((size_t)nroot, SearchLeaves());
    h->reserve_forest(P);
    hipStream_t st = h->st;
    double* D = h->fdb.p;
    int* I = h->fib.p;
    double *flo[2] = {h->ffr.p, h->ffr.p + 2 * cap * n0}, *fhi[2] = {flo[0] + cap * n0, flo[1] + cap * n0};
    int *fcu[2] = {h->fcu.p, h->fcu.p + cap * n0}, *fro[2] = {h->fcu.p + 2 * cap * n0, h->fcu.p + 2 * cap * n0 + cap};
    HIPCHK(hipMemcpyAsync(D + P.o_nrm, normals, (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));

    nnsdp::ForestArgs s;
    s.n0 = n0; s.ny = ny; s.nlit = nlit; s.literal_bounds = literal_bounds != 0; s.corner_points = corner_points != 0;
    s.normals = D + P.o_nrm; s.hs = D + P.o_hs; s.mask = reinterpret_cast<const unsigned long long*>(D + P.o_mask);
    s.seg = I + P.o_seg; s.len = I + P.o_len; s.nb = I + P.o_nb; s.flags = I + P.o_flags; s.act = I + P.o_act; s.tab = I + P.o_tab;
    s.counts = I + P.o_cnt; s.open = I + P.o_open; s.best = I + P.o_best; s.coord = I + P.o_coord; s.pflag = I + P.o_pflag;
    s.pre = I + P.o_pre; s.bt = I + P.o_bt; s.pre_stride = (long long)cap; s.bt_stride = (long long)(P.nblk + 1);
    s.bound = D + P.o_bound; s.X = D + P.o_X; s.Y = D + P.o_Y; s.log = D + P.o_log; s.elog = D + P.o_elog;

    struct Ent { int r, seg, len, nb, flags; };      // a root's segment of a level (flags as in ForestArgs)
    struct Tail { std::vector<double> lo, hi, bound; std::vector<int> literal; };      // open boxes of a root read from the frontier
    double ms_all = 0.0;
    std::vector<int> iota(G);
    for (size_t k = 0; k < G; ++k) iota[k] = (int)k;
    for (size_t g0 = 0; g0 < (size_t)nroot; g0 += G) {
      const size_t ng = std::min(G, (size_t)nroot - g0);
      // level 0: the roots themselves, in order (the caller's columns g0 .. g0 + ng - 1 are contiguous)
      HIPCHK(hipMemcpyAsync(flo[0], x1min + g0 * n0, ng * n0 * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(fhi[0], x1max + g0 * n0, ng * n0 * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(fcu[0], 0, ng * n0 * sizeof(int), st));
      HIPCHK(hipMemcpyAsync(fro[0], iota.data(), ng * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(D + P.o_hs, hs + g0 * nlit, ng * nlit * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(D + P.o_mask, masks.data() + g0, ng * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));      // (the sources are pageable arrays)

      std::vector<int> vis(ng, 0), verd(ng, -1), dep(ng, 0);
      std::vector<Tail> tails(ng);
      std::vector<char> has_tail(ng, 0);
      std::vector<Ent> lev(ng), nxt;
      for (size_t r = 0; r < ng; ++r) lev[r] = Ent{(int)r, (int)r, 1, 0, 0};
      int cur = 0, depth = 0;
      long long log_n = 0, elog_n = 0;
      for (;;) {
        int nl = 0, nlive = 0;
        for (Ent& e : lev) {
          nl += e.len;
          if (e.flags & 2) { e.nb = 0; continue; }
          ++nlive;
          const size_t r = (size_t)e.r;
          e.nb = std::min(e.len, max_boxes - vis[r]);      // (>= 1: a level that uses the budget up is the root's last one)
          vis[r] += e.nb;
          const bool stop = vis[r] >= max_boxes || depth >= max_depth || masks[g0 + r] == 0;
          e.flags = stop ? 0 : 1;
        }
        if (!nlive) break;
        const int nent = (int)lev.size();
        int* tab = h->hforest;
        int* cnt = h->hforest + 5 * G;
        for (int i = 0; i < nent; ++i) {
          const Ent& e = lev[(size_t)i];
          tab[5 * i] = e.r; tab[5 * i + 1] = e.seg; tab[5 * i + 2] = e.len; tab[5 * i + 3] = e.nb; tab[5 * i + 4] = e.flags;
        }
        h->reserve_boxes(std::min(cb, (size_t)nl), false, cb);      // (the stream is idle here: the bound kernel's buffers grow with the levels)
        s.nl = nl; s.depth = depth; s.nblk = (int)cdiv(nl, nnsdp::kForestScanBlock);
        s.lo = flo[cur]; s.hi = fhi[cur]; s.cuts = fcu[cur]; s.root = fro[cur];
        s.nlo = flo[cur ^ 1]; s.nhi = fhi[cur ^ 1]; s.ncuts = fcu[cur ^ 1]; s.nroot = fro[cur ^ 1];
        s.log_base = log_n; s.elog_base = elog_n;
        HIPCHK(hipMemcpyAsync(I + P.o_tab, tab, (size_t)5 * nent * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(h->e0, st));
        hipLaunchKernelGGL(nnsdp::k_forest_roots, dim3((unsigned)cdiv(nent, 256)), dim3(256), 0, st, s, nent);
        HIPCHK(hipGetLastError());
        for (int off = 0; off < nl; off += (int)cb) {
          const size_t nc = std::min(cb, (size_t)(nl - off));
          // (per chunk: reserve_boxes may have moved the scratch and the outputs)
          const nnsdp::CrownArgs a = h->bound_args(h->layout(nc), flo[cur] + (size_t)off * n0, fhi[cur] + (size_t)off * n0, h->dout.p);
          h->launch_bound(a, nc);
          hipLaunchKernelGGL(nnsdp::k_forest_classify, dim3((unsigned)cdiv((long long)nc, 256)), dim3(256), 0, st, s, off, (int)nc,
                             (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
          HIPCHK(hipGetLastError());
          ++h->n_bound;
        }
        const long long npts = (long long)nl * (corner_points ? 2 : 1);
        h->launch_forward(s.X, D + P.o_Y, npts);
        hipLaunchKernelGGL(nnsdp::k_forest_refute, dim3((unsigned)cdiv(npts, 256)), dim3(256), 0, st, s, npts);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nnsdp::k_forest_scan_block, dim3((unsigned)s.nblk), dim3(256), 0, st, s);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nnsdp::k_forest_scan_totals, dim3(1), dim3(256), 0, st, s);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nnsdp::k_forest_counts, dim3((unsigned)cdiv(nent, 256)), dim3(256), 0, st, s, nent);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(nnsdp::k_forest_scatter, dim3((unsigned)cdiv(nl, 256)), dim3(256), 0, st, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->e1, st));
        HIPCHK(hipMemcpyAsync(cnt, s.counts, (size_t)3 * nent * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ms_all += h->elapsed_ms();
        bool any_cand = false;
        for (int i = 0; i < nent; ++i) {
          const Ent& e = lev[(size_t)i];
          if (e.flags & 2) continue;
          if (cnt[3 * i] < 0 || cnt[3 * i + 1] < 0 || cnt[3 * i] + cnt[3 * i + 1] != e.nb)
            throw std::runtime_error("nnsdp_crown_search_many: inconsistent counts of root " + std::to_string(g0 + (size_t)e.r));
          log_n += cnt[3 * i];
          if (!(e.flags & 1)) elog_n += (e.len - e.nb) + cnt[3 * i + 1];
          any_cand = any_cand || cnt[3 * i + 2] > 0;
        }
        std::vector<int> pf;
        std::vector<double> X;
        if (any_cand) {      // the level's flags and points; per root walked in the single search's order: the centres in box order, then the corners
          pf.resize((size_t)npts); X.resize((size_t)npts * n0);
          HIPCHK(hipMemcpy(pf.data(), s.pflag, pf.size() * sizeof(int), hipMemcpyDeviceToHost));
          HIPCHK(hipMemcpy(X.data(), s.X, X.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        nxt.clear();
        int acc = 0;
        for (int i = 0; i < nent; ++i) {
          const Ent& e = lev[(size_t)i];
          if (e.flags & 2) continue;
          const size_t r = (size_t)e.r;
          const int nopen = cnt[3 * i + 1];
          bool wit = false;
          if (cnt[3 * i + 2] > 0)
            for (int half = 0; half < (corner_points ? 2 : 1) && !wit; ++half)
              for (int b = e.seg; b < e.seg + e.nb && !wit; ++b) {
                const size_t p = (size_t)half * nl + b;
                if (pf[p] && (!confirm || confirm(user, (int32_t)(g0 + r), X.data() + p * n0) != 0)) {
                  std::copy(X.begin() + p * n0, X.begin() + (p + 1) * n0, witness + (g0 + r) * n0);
                  wit = true;
                }
              }
          const bool cont = (e.flags & 1) != 0;
          if (wit) verd[r] = 1;
          else if (nopen == 0) verd[r] = e.nb < e.len ? 2 : 0;
          else if (!cont) verd[r] = 2;
          if (verd[r] >= 0) dep[r] = depth;
          if (wit && cont && nopen > 0) {      // its open boxes are leaves, and only the frontier has them: the end log holds roots that do not continue
            const size_t nb = (size_t)e.nb;
            std::vector<double> lo(nb * n0), hi(nb * n0), bnd(nb);
            std::vector<int> open(nb), best(nb);
            HIPCHK(hipMemcpy(lo.data(), flo[cur] + (size_t)e.seg * n0, lo.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hi.data(), fhi[cur] + (size_t)e.seg * n0, hi.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(bnd.data(), s.bound + e.seg, nb * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(open.data(), s.open + e.seg, nb * sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(best.data(), s.best + e.seg, nb * sizeof(int), hipMemcpyDeviceToHost));
            Tail& T = tails[r];
            has_tail[r] = 1;
            for (size_t b = 0; b < nb; ++b)
              if (open[b] == 1) {
                T.lo.insert(T.lo.end(), lo.begin() + b * n0, lo.begin() + (b + 1) * n0);
                T.hi.insert(T.hi.end(), hi.begin() + b * n0, hi.begin() + (b + 1) * n0);
                T.bound.push_back(bnd[b]); T.literal.push_back(best[b]);
              }
          }
          // the children were written before the host looked at the candidates: a violated root keeps its segment of the next level, dead
          if (cont && nopen > 0) { nxt.push_back(Ent{e.r, acc, 2 * nopen, 0, wit ? 2 : 0}); acc += 2 * nopen; }
        }
        lev.swap(nxt);
        if (lev.empty()) break;
        cur ^= 1; ++depth;
      }
      // the leaves of every root in the single search's order: the proved log up to the root's last level, the boxes of the last level
      // that the budget kept from being bounded, the last level's proved boxes, its open boxes
      std::vector<double> log((size_t)log_n * logw), elog((size_t)elog_n * logw);
      if (log_n) HIPCHK(hipMemcpy(log.data(), s.log, log.size() * sizeof(double), hipMemcpyDeviceToHost));
      if (elog_n) HIPCHK(hipMemcpy(elog.data(), s.elog, elog.size() * sizeof(double), hipMemcpyDeviceToHost));
      auto leaf = [&](SearchLeaves& L, const double* blo, const double* bhi, int d, int proved, int literal, double bound) {
        L.lo.insert(L.lo.end(), blo, blo + n0); L.hi.insert(L.hi.end(), bhi, bhi + n0);
        L.depth.push_back(d); L.proved.push_back(proved); L.literal.push_back(literal); L.bound.push_back(bound);
      };
      auto root_of = [&](const double* row) {
        const long long r = (long long)row[2 * n0 + 3];
        if (r < 0 || r >= (long long)ng) throw std::runtime_error("nnsdp_crown_search_many: a leaf-log row names no root of its group");
        return (size_t)r;
      };
      auto from_row = [&](const double* row, int proved) {
        leaf(h->fleaves[g0 + root_of(row)], row, row + n0, (int)row[2 * n0], proved, (int)row[2 * n0 + 1], row[2 * n0 + 2]);
      };
      for (long long k = 0; k < log_n; ++k) {
        const double* row = log.data() + (size_t)k * logw;
        if ((int)row[2 * n0] < dep[root_of(row)]) from_row(row, 1);
      }
      for (long long k = 0; k < elog_n; ++k) {
        const double* row = elog.data() + (size_t)k * logw;
        if ((int)row[2 * n0 + 1] < 0) from_row(row, 0);
      }
      for (long long k = 0; k < log_n; ++k) {
        const double* row = log.data() + (size_t)k * logw;
        if ((int)row[2 * n0] == dep[root_of(row)]) from_row(row, 1);
      }
      for (long long k = 0; k < elog_n; ++k) {
        const double* row = elog.data() + (size_t)k * logw;
        if ((int)row[2 * n0 + 1] >= 0) from_row(row, 0);
      }
      for (size_t r = 0; r < ng; ++r) {
        if (has_tail[r]) {
          const Tail& T = tails[r];
          for (size_t k = 0; k < T.literal.size(); ++k)
            leaf(h->fleaves[g0 + r], T.lo.data() + k * n0, T.hi.data() + k * n0, dep[r], 0, T.literal[k], T.bound[k]);
        }
        if (verd[r] < 0) throw std::runtime_error("nnsdp_crown_search_many: root " + std::to_string(g0 + r) + " was left undecided");
        verdict[g0 + r] = verd[r]; visited[g0 + r] = vis[r]; depth_reached[g0 + r] = dep[r];
        nleaves[g0 + r] = (int32_t)h->fleaves[g0 + r].depth.size();
      }
    }
    if (kernel_ms) *kernel_ms = ms_all;
  }

  // nnsdp_crown_reach.  h may be null: the scalar options come first so that their refusals can be tested on a machine without a GPU,
  // where no handle exists; every refusal comes before anything is allocated
  static void reach(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* tol, int32_t corner_points,
                    int32_t max_boxes, int32_t max_depth, int32_t chunk, int32_t* status, int32_t* visited, int32_t* depth_reached,
                    int32_t* nleaves, double* incumbent, double* witnesses, double* kernel_ms) {
    if (max_boxes < 1) throw std::invalid_argument("max_boxes must be >= 1, got " + std::to_string(max_boxes));
    if (chunk < 1) throw std::invalid_argument("chunk must be >= 1, got " + std::to_string(chunk));
    if (max_depth < 0) throw std::invalid_argument("max_depth must be >= 0, got " + std::to_string(max_depth));
    if (!h) throw std::invalid_argument("null handle");
    if (!x1min || !x1max || !tol || !status || !visited || !depth_reached || !nleaves || !incumbent || !witnesses) throw std::invalid_argument("null argument");
    const int n0 = h->n0, ny = h->ny;
    if (h->nlit < 1) throw std::invalid_argument("reach needs directions: the handle was created without normals");
    if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
    for (int i = 0; i < nlit; ++i)
      if (!std::isfinite(tol[i]) || !(tol[i] >= 0.0))
        throw std::invalid_argument("direction " + std::to_string(i) + ": tol must be finite and >= 0 (no NaN, no infinity)");
    unsigned long long splitmask = 0;
    for (int t = 0; t < n0; ++t) {
      if (!std::isfinite(x1min[t]) || !std::isfinite(x1max[t]) || !(x1min[t] <= x1max[t]))
        throw std::invalid_argument("the root box: x1min must be <= x1max and both finite (no NaN, no infinity)");
      if (x1max[t] > x1min[t]) splitmask |= 1ull << t;
    }
    // every level fits the budget as a whole, so no level and no set of children has more than max_boxes boxes
    const size_t mb = (size_t)max_boxes, npmax = corner_points ? (size_t)(1 + nlit) * mb : mb, logw = 2 * (size_t)n0 + 1 + (size_t)nlit;
    const size_t frontier_bytes = 2 * mb * n0 * (2 * sizeof(double) + sizeof(int));
    if (frontier_bytes > nnsdp::kSearchFrontierCap)
      throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(frontier_bytes) +
                                  " bytes of frontier buffers, above the cap of 2^31 bytes");
    // doubles: ub, points in, points out, leaf log, normals, tol, L, thr, xw;  ints: open, coord, slot, status
    const size_t o_ub = 0, o_X = o_ub + (size_t)nlit * mb, o_Y = o_X + npmax * n0, o_log = o_Y + npmax * ny, o_nrm = o_log + mb * logw,
                 o_tol = o_nrm + (size_t)nlit * ny, o_L = o_tol + nlit, o_thr = o_L + nlit, o_xw = o_thr + nlit, nd = o_xw + (size_t)nlit * n0;
    if (nd * sizeof(double) > nnsdp::kSearchFrontierCap)
      throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(nd * sizeof(double)) +
                                  " bytes of point and leaf-log buffers, above the cap of 2^31 bytes");
    const size_t ni = 3 * mb + 4;
    const size_t cb = std::min((size_t)chunk, mb);
    h->rleaves.clear();
    h->reserve_reach(mb, nd, ni);
    ++h->n_reach;
    hipStream_t st = h->st;
    double* D = h->rdb.p;
    int* I = h->rib.p;
    double *flo[2] = {h->rfr.p, h->rfr.p + 2 * mb * n0}, *fhi[2] = {flo[0] + mb * n0, flo[1] + mb * n0};
    int* fcu[2] = {h->rcu.p, h->rcu.p + mb * n0};
    const std::vector<double> Linit((size_t)nlit, -HUGE_VAL);
    HIPCHK(hipMemcpyAsync(flo[0], x1min, n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(fhi[0], x1max, n0 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(fcu[0], 0, n0 * sizeof(int), st));
    HIPCHK(hipMemcpyAsync(D + o_nrm, h->normals.data(), (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(D + o_tol, tol, nlit * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(D + o_L, Linit.data(), nlit * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(D + o_thr, 0, ((size_t)nlit + (size_t)nlit * n0) * sizeof(double), st));
    HIPCHK(hipStreamSynchronize(st));      // (the sources are pageable arrays)

    nnsdp::ReachArgs r;
    r.n0 = n0; r.ny = ny; r.nlit = nlit; r.corner_points = corner_points != 0; r.max_boxes = max_boxes; r.splitmask = splitmask;
    r.normals = D + o_nrm; r.tol = D + o_tol; r.open = I; r.coord = I + mb; r.slot = I + 2 * mb; r.status = I + 3 * mb;
    r.ub = D + o_ub; r.X = D + o_X; r.Y = D + o_Y; r.L = D + o_L; r.thr = D + o_thr; r.xw = D + o_xw; r.log = D + o_log;
    // k_search_scan as it is: it reads nb, open and (no points: never) pflag of its SearchArgs and writes slot and status
    nnsdp::SearchArgs s{};
    s.open = r.open; s.slot = r.slot; s.pflag = I + 3 * mb; s.status = I + 3 * mb;

    int cur = 0, nb = 1, vis = 1, depth = 0, stat = -1;
    long long log_n = 0;
    double ms_all = 0.0;
    for (;;) {
      h->reserve_boxes(std::min(cb, (size_t)nb), false, cb);      // (the stream is idle here: the bound kernel's buffers grow with the levels)
      r.nb = nb; r.depth = depth; r.visited = vis; r.children = depth < max_depth && splitmask != 0;
      r.lo = flo[cur]; r.hi = fhi[cur]; r.cuts = fcu[cur]; r.nlo = flo[cur ^ 1]; r.nhi = fhi[cur ^ 1]; r.ncuts = fcu[cur ^ 1]; r.log_base = log_n;
      s.nb = nb;
      HIPCHK(hipEventRecord(h->e0, st));
      for (int off = 0; off < nb; off += (int)cb) {
        const size_t nc = std::min(cb, (size_t)(nb - off));
        const nnsdp::CrownArgs a = h->bound_args(h->layout(nc), flo[cur] + (size_t)off * n0, fhi[cur] + (size_t)off * n0, h->dout.p);
        h->launch_bound(a, nc);
        hipLaunchKernelGGL(nnsdp::k_reach_points, dim3((unsigned)cdiv((long long)nc, 256)), dim3(256), 0, st, r, off, (int)nc,
                           (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
        HIPCHK(hipGetLastError());
        ++h->n_bound;
      }
      const long long npts = (long long)nb * (corner_points ? 1 + nlit : 1);
      h->launch_forward(r.X, D + o_Y, npts);
      hipLaunchKernelGGL(nnsdp::k_reach_incumbent, dim3((unsigned)nlit), dim3(256), 0, st, r, npts);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(nnsdp::k_reach_classify, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, r);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(nnsdp::k_search_scan, dim3(1), dim3(256), 0, st, s, 0LL);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(nnsdp::k_reach_scatter, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, r);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(h->e1, st));
      HIPCHK(hipMemcpyAsync(h->hstatus, r.status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      ms_all += h->elapsed_ms();
      const int nclosed = h->hstatus[1], nopen = h->hstatus[2];
      if (h->hstatus[0] != nb || nclosed < 0 || nopen < 0 || nclosed + nopen != nb) throw std::runtime_error("nnsdp_crown_reach: inconsistent status record");
      log_n += nclosed;
      if (nopen == 0) { stat = 0; break; }
      if (!r.children || (long long)vis + 2LL * nopen > (long long)max_boxes) { stat = 1; break; }      // (k_reach_scatter's rule)
      cur ^= 1; nb = 2 * nopen; vis += nb; ++depth;
    }
    // the leaves in the order of the Python loop: the log, then (budget) the open boxes of the last level
    std::vector<double> log((size_t)log_n * logw);
    if (log_n) HIPCHK(hipMemcpy(log.data(), r.log, log.size() * sizeof(double), hipMemcpyDeviceToHost));
    ReachLeaves& Lv = h->rleaves;
    auto leaf = [&](const double* blo, const double* bhi, int d, int closed, const double* bound) {
      Lv.lo.insert(Lv.lo.end(), blo, blo + n0); Lv.hi.insert(Lv.hi.end(), bhi, bhi + n0);
      Lv.bound.insert(Lv.bound.end(), bound, bound + nlit);
      Lv.depth.push_back(d); Lv.closed.push_back(closed);
    };
    for (long long k = 0; k < log_n; ++k) {
      const double* row = log.data() + (size_t)k * logw;
      leaf(row, row + n0, (int)row[2 * n0], 1, row + 2 * n0 + 1);
    }
    if (stat == 1) {
      std::vector<double> lo((size_t)nb * n0), hi((size_t)nb * n0), ub((size_t)nb * nlit);
      std::vector<int> open((size_t)nb);
      HIPCHK(hipMemcpy(lo.data(), flo[cur], lo.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hi.data(), fhi[cur], hi.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(ub.data(), r.ub, ub.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(open.data(), r.open, open.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int b = 0; b < nb; ++b)
        if (open[b]) leaf(lo.data() + (size_t)b * n0, hi.data() + (size_t)b * n0, depth, 0, ub.data() + (size_t)b * nlit);
    }
    HIPCHK(hipMemcpy(incumbent, r.L, nlit * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(witnesses, r.xw, (size_t)nlit * n0 * sizeof(double), hipMemcpyDeviceToHost));
    *status = stat; *visited = vis; *depth_reached = depth; *nleaves = (int32_t)Lv.depth.size();
    if (kernel_ms) *kernel_ms = ms_all;
  }

  ~nnsdp_crown() {
    if (st) (void)hipStreamSynchronize(st);
    for (double* h : {hin, hout, hX, hY, hain, haout}) if (h) (void)hipHostFree(h);
    if (hstatus) (void)hipHostFree(hstatus);
    if (hforest) (void)hipHostFree(hforest);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
};
