// The level loops of the device-resident split searches of the resident bounder: nnsdp_crown::search (kernels: csrc/crown_search.hpp),
// nnsdp_crown::reach (csrc/crown_reach.hpp), nnsdp_crown::search_many (csrc/crown_forest.hpp) and nnsdp_crown::search_nodes (the ReLU
// split, csrc/crown_node_search.hpp; its frontier holds assignments, not boxes), and what they share on the host: the
// refusals, the carving of a level's frontier (FrontierBufs, csrc/crown_handle.hpp), the chunked "bound, then classify" pass and the
// end of a level.  Part of the translation unit api.hip, behind crown_handle.hpp.
#pragma once

// the scalar options of every search; they come before the null handle, and the null handle before the null arguments, so that these
// refusals can be tested on a machine without a GPU, where no handle exists
static void check_search_options(int32_t max_boxes, int32_t chunk, int32_t max_depth, const char* budget = "max_boxes") {
  if (max_boxes < 1) throw std::invalid_argument(std::string(budget) + " must be >= 1, got " + std::to_string(max_boxes));
  if (chunk < 1) throw std::invalid_argument("chunk must be >= 1, got " + std::to_string(chunk));
  if (max_depth < 0) throw std::invalid_argument("max_depth must be >= 0, got " + std::to_string(max_depth));
}

// the literals of a clause search: the handle's own (the caller passes none) or the caller's, which then allow neither option that
// needs the literal head
static const double* search_literals(const nnsdp_crown* h, int32_t nlit, const double* normals, int32_t literal_bounds, int32_t corner_points) {
  if (h->nlit > 0) {
    if (normals) throw std::invalid_argument("the handle has literals of its own: normals must be NULL");
    if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
    return h->normals.data();
  }
  if (literal_bounds) throw std::invalid_argument("literal_bounds needs literals: the handle was created without normals");
  if (corner_points) throw std::invalid_argument("corner_points needs literals: the handle was created without normals");
  if (nlit < 1) throw std::invalid_argument("a clause needs at least one literal (nlit >= 1)");
  check_literals(h->ny, nlit, normals);
  return normals;
}

// the refusal of a root box and its splittable mask (bit t: x1max[t] > x1min[t]); root >= 0: the box is root `root` of several
static unsigned long long root_box_mask(int n0, const double* x1min, const double* x1max, long long root = -1) {
  unsigned long long mask = 0;
  for (int t = 0; t < n0; ++t) {
    if (!std::isfinite(x1min[t]) || !std::isfinite(x1max[t]) || !(x1min[t] <= x1max[t]))
      throw std::invalid_argument((root < 0 ? std::string("the root box") : "root " + std::to_string(root)) +
                                  ": x1min must be <= x1max and both finite (no NaN, no infinity)");
    if (x1max[t] > x1min[t]) mask |= 1ull << t;
  }
  return mask;
}

// the cap on the two frontiers of `cap` boxes each of a search with one root
static void check_frontier_bytes(int32_t max_boxes, size_t cap, size_t n0) {
  const size_t frontier_bytes = 2 * cap * n0 * (2 * sizeof(double) + sizeof(int));
  if (frontier_bytes > nnsdp::kSearchFrontierCap)
    throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(frontier_bytes) +
                                " bytes of frontier buffers, above the cap of 2^31 bytes");
}

// the buffers of a search with a four-integer status record (search, reach)
static void reserve_frontier(nnsdp_crown* h, FrontierBufs& B, size_t cap, size_t nd, size_t ni) {
  h->n_alloc += B.reserve(cap, (size_t)h->n0, false, nd, ni);
  if (!h->hstatus) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->hstatus), 4 * sizeof(int), hipHostMallocDefault));
}

template <class T>
static std::vector<T> from_device(const T* p, size_t count) {
  std::vector<T> v(count);
  if (count) HIPCHK(hipMemcpy(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost));
  return v;
}

// The first part of a level: its n boxes (frontier `cur` of B) are bounded in chunks of at most cb, and per_chunk(off, nc, a) launches the
// search's kernel on the outputs a.ymin / a.ymax / a.smax / a.uA of boxes off .. off + nc - 1.  No kernel is on the stream on entry, so the
// bound kernel's buffers may grow with the levels; the timed span of the level starts behind that, and start() launches what precedes the chunks
template <class Start, class PerChunk>
static void bound_level(nnsdp_crown* h, const FrontierBufs& B, int cur, int n, size_t cb, Start&& start, PerChunk&& per_chunk) {
  h->reserve_boxes(std::min(cb, (size_t)n), false, cb);
  HIPCHK(hipEventRecord(h->e0, h->st));
  start();
  for (int off = 0; off < n; off += (int)cb) {
    const size_t nc = std::min(cb, (size_t)(n - off));
    // (per chunk: reserve_boxes may have moved the scratch and the outputs)
    const nnsdp::CrownArgs a = h->bound_args(h->layout(nc), B.lo(cur) + (size_t)off * h->n0, B.hi(cur) + (size_t)off * h->n0, h->dout.p);
    h->launch_bound(a, nc);
    per_chunk(off, (int)nc, a);
    HIPCHK(hipGetLastError());
    ++h->n_bound;
  }
}

// the end of a level: the timed span closes, the level's `count` integers come back into the pinned `host`; returns the span's milliseconds
static float finish_level(nnsdp_crown* h, int* host, const int* dev, size_t count) {
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipMemcpyAsync(host, dev, count * sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return h->elapsed_ms();
}

#define FRONTIER_LAUNCH(kernel, blocks, ...)                                                        \
  do {                                                                                              \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(256), 0, st, __VA_ARGS__);            \
    HIPCHK(hipGetLastError());                                                                      \
  } while (0)

// nnsdp_crown_search
inline void nnsdp_crown::search(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* normals, const double* hs,
                                int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth, int32_t chunk,
                                nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* visited, int32_t* depth_reached,
                                int32_t* nleaves, double* witness, double* kernel_ms) {
  check_search_options(max_boxes, chunk, max_depth);
  if (!h) throw std::invalid_argument("null handle");
  if (!x1min || !x1max || !hs || !verdict || !visited || !depth_reached || !nleaves || !witness) throw std::invalid_argument("null argument");
  const int n0 = h->n0, ny = h->ny;
  normals = search_literals(h, nlit, normals, literal_bounds, corner_points);
  for (int i = 0; i < nlit; ++i)
    if (!std::isfinite(hs[i])) throw std::invalid_argument("literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
  const unsigned long long splitmask = root_box_mask(n0, x1min, x1max);
  // a level bounds at most max_boxes boxes and its children number at most twice that
  const size_t mb = (size_t)max_boxes, cap = 2 * mb, npmax = corner_points ? 2 * mb : mb, logw = 2 * (size_t)n0 + 3;
  check_frontier_bytes(max_boxes, cap, (size_t)n0);
  // doubles: bound, points in, points out, leaf log, normals, hs;  ints: open, best, coord, slot, point flags, status
  const size_t o_bound = 0, o_X = o_bound + mb, o_Y = o_X + npmax * n0, o_log = o_Y + npmax * ny, o_nrm = o_log + mb * logw,
               o_hs = o_nrm + (size_t)nlit * ny, nd = o_hs + nlit;
  const size_t ni = 4 * mb + npmax + 4;
  const size_t cb = std::min((size_t)chunk, mb);
  FrontierBufs& B = h->sbuf;
  h->leaves.clear();
  reserve_frontier(h, B, cap, nd, ni);
  hipStream_t st = h->st;
  double* D = B.db.p;
  int* I = B.ib.p;
  B.roots(x1min, x1max, 1, st);
  HIPCHK(hipMemcpyAsync(D + o_nrm, normals, (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_hs, hs, nlit * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));      // (the sources are the caller's pageable arrays)

  nnsdp::SearchArgs s;
  s.f.n0 = n0; s.f.ny = ny; s.f.nlit = nlit; s.f.corner_points = corner_points != 0; s.f.normals = D + o_nrm;
  s.f.X = D + o_X; s.f.Y = D + o_Y; s.f.log = D + o_log;
  s.literal_bounds = literal_bounds != 0; s.splitmask = splitmask; s.hs = D + o_hs;
  s.open = I; s.best = I + mb; s.coord = I + 2 * mb; s.slot = I + 3 * mb; s.pflag = I + 4 * mb; s.status = I + 4 * mb + npmax;
  s.bound = D + o_bound;

  int cur = 0, nlevel = 1, nb = 0, vis = 0, depth = 0, verd = -1;
  long long log_n = 0, log_before = 0;
  double ms_all = 0.0;
  std::vector<double> wit;
  for (;;) {
    nb = std::min(nlevel, max_boxes - vis);      // (>= 1: a level that uses the budget up is the last one)
    vis += nb;
    log_before = log_n;
    s.nb = nb;
    B.level(s.f, cur, depth, log_n);
    bound_level(h, B, cur, nb, cb, [] {}, [&](int off, int nc, const nnsdp::CrownArgs& a) {
      hipLaunchKernelGGL(nnsdp::k_search_classify, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, st, s, off, nc,
                         (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
    });
    const long long npts = (long long)nb * (corner_points ? 2 : 1);
    h->launch_forward(s.f.X, D + o_Y, npts);
    FRONTIER_LAUNCH(nnsdp::k_search_refute, cdiv(npts, 256), s, npts);
    const bool stop = vis >= max_boxes || depth >= max_depth || splitmask == 0;
    FRONTIER_LAUNCH(nnsdp::k_search_scan, 1, (const int*)s.open, nb, s.slot, (const int*)s.pflag, npts, s.status);
    FRONTIER_LAUNCH(nnsdp::k_search_scatter, cdiv(nb, 256), s, stop ? 0 : 1);
    ms_all += finish_level(h, h->hstatus, s.status, 4);
    const int nproved = h->hstatus[1], nopen = h->hstatus[2], ncand = h->hstatus[3];
    if (h->hstatus[0] != nb || nproved + nopen != nb) throw std::runtime_error("nnsdp_crown_search: inconsistent status record");
    log_n += nproved;
    if (ncand > 0) {      // the level's flags and points, walked in the Python driver's order: the centres in box order, then the corners
      const std::vector<int> pf = from_device(s.pflag, (size_t)npts);
      const std::vector<double> X = from_device(s.f.X, (size_t)npts * n0);
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
  const std::vector<double> log = from_device(s.f.log, (size_t)log_n * logw), lo = from_device(B.lo(cur), (size_t)nlevel * n0),
                            hi = from_device(B.hi(cur), (size_t)nlevel * n0), bnd = from_device(s.bound, (size_t)nb);
  const std::vector<int> open = from_device(s.open, (size_t)nb), best = from_device(s.best, (size_t)nb);
  SearchLeaves& L = h->leaves;
  const size_t nleaf = (size_t)log_n + (size_t)(nlevel - nb) + (size_t)h->hstatus[2];
  L.lo.reserve(nleaf * n0); L.hi.reserve(nleaf * n0); L.depth.reserve(nleaf); L.proved.reserve(nleaf); L.literal.reserve(nleaf); L.bound.reserve(nleaf);
  auto from_log = [&](long long r) {
    const double* row = log.data() + (size_t)r * logw;
    L.add(n0, row, row + n0, (int)row[2 * n0], 1, (int)row[2 * n0 + 1], row[2 * n0 + 2]);
  };
  auto from_frontier = [&](int b, int literal, double bound) { L.add(n0, lo.data() + (size_t)b * n0, hi.data() + (size_t)b * n0, depth, 0, literal, bound); };
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
inline nnsdp::ForestPlan nnsdp_crown::forest_group_plan(int n0, int ny, int nlit, int32_t max_boxes, int32_t corner_points, int32_t nroot, int32_t group) {
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
// root the result of search()
inline void nnsdp_crown::search_many(nnsdp_crown* h, int32_t nroot, const double* x1min, const double* x1max, int32_t nlit, const double* normals,
                                     const double* hs, int32_t literal_bounds, int32_t corner_points, int32_t max_boxes, int32_t max_depth,
                                     int32_t chunk, int32_t group, nnsdp_confirm_many_fn confirm, void* user, int32_t* verdict, int32_t* visited,
                                     int32_t* depth_reached, int32_t* nleaves, double* witness, double* kernel_ms) {
  check_search_options(max_boxes, chunk, max_depth);
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
  normals = search_literals(h, nlit, normals, literal_bounds, corner_points);
  std::vector<unsigned long long> masks((size_t)nroot, 0);
  for (int r = 0; r < nroot; ++r) {
    for (int i = 0; i < nlit; ++i)
      if (!std::isfinite(hs[(size_t)r * nlit + i]))
        throw std::invalid_argument("root " + std::to_string(r) + ", literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
    masks[(size_t)r] = root_box_mask(n0, x1min + (size_t)r * n0, x1max + (size_t)r * n0, r);
  }
  const nnsdp::ForestPlan P = forest_group_plan(n0, ny, nlit, max_boxes, corner_points, nroot, group);
  const size_t G = P.group, cap = P.cap, logw = P.logw;
  const size_t cb = std::min((size_t)chunk, cap);
  FrontierBufs& B = h->fbuf;
  h->fleaves.assign((size_t)nroot, SearchLeaves());
  h->n_alloc += B.reserve(cap, (size_t)n0, true, P.nd, P.ni);
  if (8 * G > h->hforest_cap) {
    if (h->hforest) { HIPCHK(hipHostFree(h->hforest)); h->hforest = nullptr; }
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->hforest), 8 * G * sizeof(int), hipHostMallocDefault));
    h->hforest_cap = 8 * G;
  }
  hipStream_t st = h->st;
  double* D = B.db.p;
  int* I = B.ib.p;
  HIPCHK(hipMemcpyAsync(D + P.o_nrm, normals, (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));

  nnsdp::ForestArgs s;
  s.f.n0 = n0; s.f.ny = ny; s.f.nlit = nlit; s.f.corner_points = corner_points != 0; s.f.normals = D + P.o_nrm;
  s.f.X = D + P.o_X; s.f.Y = D + P.o_Y; s.f.log = D + P.o_log; s.elog = D + P.o_elog;
  s.literal_bounds = literal_bounds != 0; s.hs = D + P.o_hs; s.mask = reinterpret_cast<const unsigned long long*>(D + P.o_mask);
  s.seg = I + P.o_seg; s.len = I + P.o_len; s.nb = I + P.o_nb; s.flags = I + P.o_flags; s.act = I + P.o_act; s.tab = I + P.o_tab;
  s.counts = I + P.o_cnt; s.open = I + P.o_open; s.best = I + P.o_best; s.coord = I + P.o_coord; s.pflag = I + P.o_pflag;
  s.pre = I + P.o_pre; s.bt = I + P.o_bt; s.pre_stride = (long long)cap; s.bt_stride = (long long)(P.nblk + 1);
  s.bound = D + P.o_bound;

  struct Ent { int r, seg, len, nb, flags; };      // a root's segment of a level (flags as in ForestArgs)
  struct Tail { std::vector<double> lo, hi, bound; std::vector<int> literal; };      // open boxes of a root read from the frontier
  double ms_all = 0.0;
  std::vector<int> iota(G);
  for (size_t k = 0; k < G; ++k) iota[k] = (int)k;
  for (size_t g0 = 0; g0 < (size_t)nroot; g0 += G) {
    const size_t ng = std::min(G, (size_t)nroot - g0);
    // level 0: the roots themselves, in order (the caller's columns g0 .. g0 + ng - 1 are contiguous)
    B.roots(x1min + g0 * n0, x1max + g0 * n0, ng, st);
    HIPCHK(hipMemcpyAsync(B.root(0), iota.data(), ng * sizeof(int), hipMemcpyHostToDevice, st));
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
      s.nl = nl; s.nblk = (int)cdiv(nl, nnsdp::kForestScanBlock);
      B.level(s.f, cur, depth, log_n);
      s.root = B.root(cur); s.nroot = B.root(cur ^ 1); s.elog_base = elog_n;
      HIPCHK(hipMemcpyAsync(I + P.o_tab, tab, (size_t)5 * nent * sizeof(int), hipMemcpyHostToDevice, st));
      bound_level(h, B, cur, nl, cb, [&] { FRONTIER_LAUNCH(nnsdp::k_forest_roots, cdiv(nent, 256), s, nent); },
                  [&](int off, int nc, const nnsdp::CrownArgs& a) {
                    hipLaunchKernelGGL(nnsdp::k_forest_classify, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, st, s, off, nc,
                                       (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
                  });
      const long long npts = (long long)nl * (corner_points ? 2 : 1);
      h->launch_forward(s.f.X, D + P.o_Y, npts);
      FRONTIER_LAUNCH(nnsdp::k_forest_refute, cdiv(npts, 256), s, npts);
      FRONTIER_LAUNCH(nnsdp::k_forest_scan_block, s.nblk, s);
      FRONTIER_LAUNCH(nnsdp::k_forest_scan_totals, 1, s);
      FRONTIER_LAUNCH(nnsdp::k_forest_counts, cdiv(nent, 256), s, nent);
      FRONTIER_LAUNCH(nnsdp::k_forest_scatter, cdiv(nl, 256), s);
      ms_all += finish_level(h, cnt, s.counts, (size_t)3 * nent);
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
        pf = from_device(s.pflag, (size_t)npts);
        X = from_device(s.f.X, (size_t)npts * n0);
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
          const std::vector<double> lo = from_device(B.lo(cur) + (size_t)e.seg * n0, nb * n0), hi = from_device(B.hi(cur) + (size_t)e.seg * n0, nb * n0),
                                    bnd = from_device(s.bound + e.seg, nb);
          const std::vector<int> open = from_device(s.open + e.seg, nb), best = from_device(s.best + e.seg, nb);
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
    const std::vector<double> log = from_device(s.f.log, (size_t)log_n * logw), elog = from_device(s.elog, (size_t)elog_n * logw);
    auto root_of = [&](const double* row) {
      const long long r = (long long)row[2 * n0 + 3];
      if (r < 0 || r >= (long long)ng) throw std::runtime_error("nnsdp_crown_search_many: a leaf-log row names no root of its group");
      return (size_t)r;
    };
    auto from_row = [&](const double* row, int proved) {
      h->fleaves[g0 + root_of(row)].add(n0, row, row + n0, (int)row[2 * n0], proved, (int)row[2 * n0 + 1], row[2 * n0 + 2]);
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
          h->fleaves[g0 + r].add(n0, T.lo.data() + k * n0, T.hi.data() + k * n0, dep[r], 0, T.literal[k], T.bound[k]);
      }
      if (verd[r] < 0) throw std::runtime_error("nnsdp_crown_search_many: root " + std::to_string(g0 + r) + " was left undecided");
      verdict[g0 + r] = verd[r]; visited[g0 + r] = vis[r]; depth_reached[g0 + r] = dep[r];
      nleaves[g0 + r] = (int32_t)h->fleaves[g0 + r].depth.size();
    }
  }
  if (kernel_ms) *kernel_ms = ms_all;
}

// nnsdp_crown_reach; every refusal comes before anything is allocated
inline void nnsdp_crown::reach(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* tol, int32_t corner_points,
                               int32_t max_boxes, int32_t max_depth, int32_t chunk, int32_t* status, int32_t* visited, int32_t* depth_reached,
                               int32_t* nleaves, double* incumbent, double* witnesses, double* kernel_ms) {
  check_search_options(max_boxes, chunk, max_depth);
  if (!h) throw std::invalid_argument("null handle");
  if (!x1min || !x1max || !tol || !status || !visited || !depth_reached || !nleaves || !incumbent || !witnesses) throw std::invalid_argument("null argument");
  const int n0 = h->n0, ny = h->ny;
  if (h->nlit < 1) throw std::invalid_argument("reach needs directions: the handle was created without normals");
  if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
  for (int i = 0; i < nlit; ++i)
    if (!std::isfinite(tol[i]) || !(tol[i] >= 0.0))
      throw std::invalid_argument("direction " + std::to_string(i) + ": tol must be finite and >= 0 (no NaN, no infinity)");
  const unsigned long long splitmask = root_box_mask(n0, x1min, x1max);
  // every level fits the budget as a whole, so no level and no set of children has more than max_boxes boxes
  const size_t mb = (size_t)max_boxes, npmax = corner_points ? (size_t)(1 + nlit) * mb : mb, logw = 2 * (size_t)n0 + 1 + (size_t)nlit;
  check_frontier_bytes(max_boxes, mb, (size_t)n0);
  // doubles: ub, points in, points out, leaf log, normals, tol, L, thr, xw;  ints: open, coord, slot, status
  const size_t o_ub = 0, o_X = o_ub + (size_t)nlit * mb, o_Y = o_X + npmax * n0, o_log = o_Y + npmax * ny, o_nrm = o_log + mb * logw,
               o_tol = o_nrm + (size_t)nlit * ny, o_L = o_tol + nlit, o_thr = o_L + nlit, o_xw = o_thr + nlit, nd = o_xw + (size_t)nlit * n0;
  if (nd * sizeof(double) > nnsdp::kSearchFrontierCap)
    throw std::invalid_argument("max_boxes = " + std::to_string(max_boxes) + " needs " + std::to_string(nd * sizeof(double)) +
                                " bytes of point and leaf-log buffers, above the cap of 2^31 bytes");
  const size_t ni = 3 * mb + 4;
  const size_t cb = std::min((size_t)chunk, mb);
  FrontierBufs& B = h->rbuf;
  h->rleaves.clear();
  reserve_frontier(h, B, mb, nd, ni);
  ++h->n_reach;
  hipStream_t st = h->st;
  double* D = B.db.p;
  int* I = B.ib.p;
  const std::vector<double> Linit((size_t)nlit, -HUGE_VAL);
  B.roots(x1min, x1max, 1, st);
  HIPCHK(hipMemcpyAsync(D + o_nrm, h->normals.data(), (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_tol, tol, nlit * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_L, Linit.data(), nlit * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(D + o_thr, 0, ((size_t)nlit + (size_t)nlit * n0) * sizeof(double), st));
  HIPCHK(hipStreamSynchronize(st));      // (the sources are pageable arrays)

  nnsdp::ReachArgs r;
  r.f.n0 = n0; r.f.ny = ny; r.f.nlit = nlit; r.f.corner_points = corner_points != 0; r.f.normals = D + o_nrm;
  r.f.X = D + o_X; r.f.Y = D + o_Y; r.f.log = D + o_log;
  r.max_boxes = max_boxes; r.splitmask = splitmask; r.tol = D + o_tol;
  r.open = I; r.coord = I + mb; r.slot = I + 2 * mb; r.status = I + 3 * mb;
  r.ub = D + o_ub; r.L = D + o_L; r.thr = D + o_thr; r.xw = D + o_xw;
  int* const dstatus = I + 3 * mb;

  int cur = 0, nb = 1, vis = 1, depth = 0, stat = -1;
  long long log_n = 0;
  double ms_all = 0.0;
  for (;;) {
    r.nb = nb; r.visited = vis; r.children = depth < max_depth && splitmask != 0;
    B.level(r.f, cur, depth, log_n);
    bound_level(h, B, cur, nb, cb, [] {}, [&](int off, int nc, const nnsdp::CrownArgs& a) {
      hipLaunchKernelGGL(nnsdp::k_reach_points, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, st, r, off, nc,
                         (const double*)a.ymin, (const double*)a.ymax, (const double*)a.smax, (const double*)a.uA);
    });
    const long long npts = (long long)nb * (corner_points ? 1 + nlit : 1);
    h->launch_forward(r.f.X, D + o_Y, npts);
    FRONTIER_LAUNCH(nnsdp::k_reach_incumbent, nlit, r, npts);
    FRONTIER_LAUNCH(nnsdp::k_reach_classify, cdiv(nb, 256), r);
    // the ranks of the open boxes; reach has no candidate points to count
    FRONTIER_LAUNCH(nnsdp::k_search_scan, 1, (const int*)r.open, nb, r.slot, (const int*)nullptr, 0LL, dstatus);
    FRONTIER_LAUNCH(nnsdp::k_reach_scatter, cdiv(nb, 256), r);
    ms_all += finish_level(h, h->hstatus, r.status, 4);
    const int nclosed = h->hstatus[1], nopen = h->hstatus[2];
    if (h->hstatus[0] != nb || nclosed < 0 || nopen < 0 || nclosed + nopen != nb) throw std::runtime_error("nnsdp_crown_reach: inconsistent status record");
    log_n += nclosed;
    if (nopen == 0) { stat = 0; break; }
    if (!r.children || (long long)vis + 2LL * nopen > (long long)max_boxes) { stat = 1; break; }      // (k_reach_scatter's rule)
    cur ^= 1; nb = 2 * nopen; vis += nb; ++depth;
  }
  // the leaves in the order of the Python loop: the log, then (budget) the open boxes of the last level
  const std::vector<double> log = from_device(r.f.log, (size_t)log_n * logw);
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
    const std::vector<double> lo = from_device(B.lo(cur), (size_t)nb * n0), hi = from_device(B.hi(cur), (size_t)nb * n0),
                              ub = from_device(r.ub, (size_t)nb * nlit);
    const std::vector<int> open = from_device(r.open, (size_t)nb);
    for (int b = 0; b < nb; ++b)
      if (open[b]) leaf(lo.data() + (size_t)b * n0, hi.data() + (size_t)b * n0, depth, 0, ub.data() + (size_t)b * nlit);
  }
  HIPCHK(hipMemcpy(incumbent, r.L, nlit * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(witnesses, r.xw, (size_t)nlit * n0 * sizeof(double), hipMemcpyDeviceToHost));
  *status = stat; *visited = vis; *depth_reached = depth; *nleaves = (int32_t)Lv.depth.size();
  if (kernel_ms) *kernel_ms = ms_all;
}

// nnsdp_crown_search_nodes: the level loop of relusplit.py (_levels) on the handle's stream (csrc/crown_node_search.hpp); every refusal
// comes before anything is allocated
inline void nnsdp_crown::search_nodes(nnsdp_crown* h, const double* x1min, const double* x1max, int32_t nlit, const double* hs, int32_t steps,
                                      double eta0, double decay, int32_t corner_points, int32_t max_nodes, int32_t max_depth, int32_t chunk,
                                      nnsdp_confirm_fn confirm, void* user, int32_t* verdict, int32_t* reason, int32_t* visited,
                                      int32_t* depth_reached, int32_t* nleaves, int32_t* nopen_out, double* witness, double* kernel_ms) {
  check_search_options(max_nodes, chunk, max_depth, "max_nodes");
  check_pg_options("nodes", steps, eta0, decay);
  if (!h) throw std::invalid_argument("null handle");
  if (h->wide()) throw std::invalid_argument("a ReLU split is not available on a wide bounder (max_width 128): the node kernels keep a 64-wide layout");
  if (h->activ != NNSDP_ACTIV_RELU) throw std::invalid_argument("a ReLU split is for ReLU networks, not Tanh");
  if (h->nlit < 1) throw std::invalid_argument("a ReLU split needs literals: the handle was created without normals");
  if (!x1min || !x1max || !hs || !verdict || !reason || !visited || !depth_reached || !nleaves || !nopen_out || !witness) throw std::invalid_argument("null argument");
  if (nlit != h->nlit) throw std::invalid_argument("nlit must be the handle's " + std::to_string(h->nlit) + ", got " + std::to_string(nlit));
  for (int i = 0; i < nlit; ++i)
    if (!std::isfinite(hs[i])) throw std::invalid_argument("literal " + std::to_string(i) + ": the threshold hs is not finite (NaN or infinity)");
  const int n0 = h->n0, ny = h->ny, acdim = h->acdim;
  (void)root_box_mask(n0, x1min, x1max);
  // every level fits the budget as a whole, so no level, no log and no set of children has more than max_nodes nodes
  const size_t mn = (size_t)max_nodes, npmax = corner_points ? 1 + mn * (size_t)nlit : 1, cb = std::min((size_t)chunk, mn);
  // bytes: the two frontiers, the leaf log, the stuck log
  const size_t nby = 4 * mn * (size_t)acdim;
  // doubles: bound, points in, points out, the bounds of the two logs, normals, hs, the root box
  const size_t o_bound = 0, o_X = o_bound + mn, o_Y = o_X + npmax * n0, o_lb = o_Y + npmax * ny, o_sb = o_lb + mn, o_nrm = o_sb + mn,
               o_hs = o_nrm + (size_t)nlit * ny, o_root = o_hs + nlit, nd = o_root + 2 * (size_t)n0;
  // ints: kind, best, neuron, the three ranks, depth and kind of the leaf log, depth of the stuck log, point flags, status
  const size_t o_pf = 9 * mn, o_st = o_pf + npmax, ni = o_st + 5;
  const size_t worst = std::max(nby, std::max(nd * sizeof(double), ni * sizeof(int)));
  if (worst > nnsdp::kSearchFrontierCap)
    throw std::invalid_argument("max_nodes = " + std::to_string(max_nodes) + " needs " + std::to_string(worst) +
                                " bytes of " + (worst == nby ? "frontier and log" : worst == nd * sizeof(double) ? "point and record" : "record") +
                                " buffers, above the cap of 2^31 bytes");
  h->nleaves_.clear();
  h->reserve_nodes(cb);
  if (nby > h->nsby.n) { h->nsby.alloc(nby); ++h->n_alloc; }
  if (nd > h->nsdb.n) { h->nsdb.alloc(nd); ++h->n_alloc; }
  if (ni > h->nsib.n) { h->nsib.alloc(ni); ++h->n_alloc; }
  if (!h->hnstatus) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->hnstatus), 5 * sizeof(int), hipHostMallocDefault));
  ++h->n_node_search;
  hipStream_t st = h->st;
  double* D = h->nsdb.p;
  int* I = h->nsib.p;
  int8_t* const fr[2] = {h->nsby.p, h->nsby.p + mn * acdim};
  HIPCHK(hipMemcpyAsync(D + o_nrm, h->normals.data(), (size_t)nlit * ny * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_hs, hs, nlit * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_root, x1min, n0 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(D + o_root + n0, x1max, n0 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(fr[0], 0, (size_t)acdim, st));      // the root: every neuron free
  HIPCHK(hipStreamSynchronize(st));      // (the sources are the caller's pageable arrays)
  // the boxes of one chunk, written once: every node has the root's
  double* const blo = h->dnin.p;
  double* const bhi = blo + cb * n0;
  FRONTIER_LAUNCH(nnsdp::k_node_boxes, cdiv(cb * n0, 256), (const double*)(D + o_root), (const double*)(D + o_root + n0), n0, (long long)cb, blo, bhi);

  nnsdp::NodeSearchArgs a;
  a.n0 = n0; a.ny = ny; a.nlit = nlit; a.acdim = acdim; a.corner_points = corner_points != 0; a.max_nodes = max_nodes;
  a.normals = D + o_nrm; a.hs = D + o_hs; a.lo = blo; a.hi = bhi;
  a.kind = I; a.best = I + mn; a.neuron = I + 2 * mn; a.rclosed = I + 3 * mn; a.rstuck = I + 4 * mn; a.rbranch = I + 5 * mn;
  a.ldepth = I + 6 * mn; a.lkind = I + 7 * mn; a.sdepth = I + 8 * mn; a.pflag = I + o_pf; a.status = I + o_st;
  a.bound = D + o_bound; a.X = D + o_X; a.Y = D + o_Y; a.lbound = D + o_lb; a.sbound = D + o_sb;
  a.lassign = h->nsby.p + 2 * mn * acdim; a.sassign = h->nsby.p + 3 * mn * acdim;

  int cur = 0, nb = 1, vis = 0, depth = 0, verd = -1, reas = 0, tail = 0;      // tail: 0 no open node of the last level, 1 all, 2 the branching ones
  long long log_n = 0, slog_n = 0;
  double ms_all = 0.0;
  std::vector<double> wit;
  for (;;) {
    vis += nb;
    a.nb = nb; a.depth = depth; a.visited = vis; a.children = depth + 1 <= max_depth;
    a.cur = fr[cur]; a.nxt = fr[cur ^ 1]; a.log_base = log_n; a.slog_base = slog_n;
    HIPCHK(hipEventRecord(h->e0, st));
    for (int off = 0; off < nb; off += (int)cb) {
      const size_t nc = std::min(cb, (size_t)(nb - off));
      const nnsdp::CrownNodeArgs p = h->node_args(h->node_layout(nc), blo, bhi, a.cur + (size_t)off * acdim, steps, eta0, decay);
      h->launch_nodes(p, nc);
      FRONTIER_LAUNCH(nnsdp::k_node_classify, cdiv(nc, 256), a, off, (int)nc, (const double*)p.o.smax, (const double*)p.o.uA,
                      (const double*)p.sp.branch, (const double*)p.infeasible);
      ++h->n_bound;
    }
    const long long npts = corner_points ? 1 + (long long)nb * nlit : 1;
    h->launch_forward(a.X, D + o_Y, npts);
    FRONTIER_LAUNCH(nnsdp::k_node_refute, cdiv(npts, 256), a, npts);
    FRONTIER_LAUNCH(nnsdp::k_node_scan, 1, a, npts);
    FRONTIER_LAUNCH(nnsdp::k_node_scatter, cdiv(nb, 256 / nnsdp::kNodeLanes), a);
    ms_all += finish_level(h, h->hnstatus, a.status, 5);
    ++h->n_node_levels;
    const int nclosed = h->hnstatus[1], nstuck = h->hnstatus[2], nbranch = h->hnstatus[3], ncand = h->hnstatus[4];
    if (h->hnstatus[0] != nb || nclosed < 0 || nstuck < 0 || nbranch < 0 || nclosed + nstuck + nbranch != nb)
      throw std::runtime_error("nnsdp_crown_search_nodes: inconsistent status record");
    log_n += nclosed;
    if (nstuck + nbranch == 0) { verd = slog_n > 0 ? 2 : 0; reas = slog_n > 0 ? 2 : 0; break; }
    if (ncand > 0) {      // the level's flags and points; the flagged points without duplicates, in lexicographic order (np.unique(axis=1))
      ++h->n_node_downloads;
      const std::vector<int> pf = from_device(a.pflag, (size_t)npts);
      const std::vector<double> X = from_device(a.X, (size_t)npts * n0);
      std::vector<size_t> cand;
      for (size_t p = 0; p < (size_t)npts; ++p)
        if (pf[p]) cand.push_back(p);
      auto less = [&](size_t p, size_t q) { return std::lexicographical_compare(X.begin() + p * n0, X.begin() + (p + 1) * n0, X.begin() + q * n0, X.begin() + (q + 1) * n0); };
      auto same = [&](size_t p, size_t q) { return std::equal(X.begin() + p * n0, X.begin() + (p + 1) * n0, X.begin() + q * n0); };
      std::stable_sort(cand.begin(), cand.end(), less);
      cand.erase(std::unique(cand.begin(), cand.end(), same), cand.end());
      for (size_t k = 0; k < cand.size() && wit.empty(); ++k) {
        const double* x = X.data() + cand[k] * n0;
        if (!confirm || confirm(user, x) != 0) wit.assign(x, x + n0);
      }
    }
    if (!wit.empty()) { verd = 1; tail = 1; break; }
    slog_n += nstuck;
    if (nbranch == 0) { verd = 2; reas = 2; break; }
    if ((long long)vis + 2LL * nbranch > (long long)max_nodes || depth + 1 > max_depth) { verd = 2; reas = 1; tail = 2; break; }      // (k_node_scatter's rule)
    cur ^= 1; nb = 2 * nbranch; ++depth;
  }
  // the leaves once, at the end: the closed log; then the open nodes: the stuck log, then what the last level leaves open
  NodeLeaves& Lv = h->nleaves_;
  {
    const std::vector<int8_t> as = from_device((const int8_t*)a.lassign, (size_t)log_n * acdim);
    const std::vector<int> dp = from_device((const int*)a.ldepth, (size_t)log_n), kd = from_device((const int*)a.lkind, (size_t)log_n);
    const std::vector<double> bd = from_device((const double*)a.lbound, (size_t)log_n);
    for (size_t r = 0; r < (size_t)log_n; ++r) Lv.add(acdim, as.data() + r * acdim, dp[r], kd[r], bd[r]);
  }
  const size_t nclosed_all = Lv.depth.size();
  {
    const std::vector<int8_t> as = from_device((const int8_t*)a.sassign, (size_t)slog_n * acdim);
    const std::vector<int> dp = from_device((const int*)a.sdepth, (size_t)slog_n);
    const std::vector<double> bd = from_device((const double*)a.sbound, (size_t)slog_n);
    for (size_t r = 0; r < (size_t)slog_n; ++r) Lv.add(acdim, as.data() + r * acdim, dp[r], -1, bd[r]);
  }
  if (tail) {
    const std::vector<int8_t> as = from_device((const int8_t*)a.cur, (size_t)nb * acdim);
    const std::vector<int> kd = from_device((const int*)a.kind, (size_t)nb);
    const std::vector<double> bd = from_device((const double*)a.bound, (size_t)nb);
    for (size_t b = 0; b < (size_t)nb; ++b)
      if (tail == 1 ? kd[b] >= nnsdp::kNodeStuck : kd[b] == nnsdp::kNodeBranching) Lv.add(acdim, as.data() + b * acdim, depth, -1, bd[b]);
  }
  *verdict = verd; *reason = reas; *visited = vis; *depth_reached = depth;
  *nleaves = (int32_t)nclosed_all; *nopen_out = (int32_t)(Lv.depth.size() - nclosed_all);
  if (verd == 1) std::copy(wit.begin(), wit.end(), witness);
  if (kernel_ms) *kernel_ms = ms_all;
}

#undef FRONTIER_LAUNCH
