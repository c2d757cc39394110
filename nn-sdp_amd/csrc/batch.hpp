// The batch handle (nnsdp_batch): several solvers advanced in lockstep.  Part of the translation unit api.hip, after solver.hpp.
// Behind the projection it launches the batch forms of admm_tail.hpp over a device table of the members' nnsdp_solver::iter_args().
#pragma once

// ---------------------------------------------------------------------------------------------
// Batch handle: several independent SDPs (beta sweep of experiments/scale.jl:28, hyperplane directions of
// NnSdp.findReach2Dpoly, the sub-queries of an ACAS clause) advanced in lockstep with ONE launch per stage for all
// of them - blockIdx.y (small kernels) or a block map (projection) selects the SDP.  A single W40-D20 SDP keeps
// 19 of 256 CUs busy; one stream per SDP fills the chip only nominally, because every dependent launch of every
// stream pays the queue-scheduling latency of 13 queues (measured: 13 streams reach 3.1x the single-SDP rate).
// The solvers stay owned by the caller; plain iterations run through the batch, check iterations (one in
// check_every) run on the solvers' own streams, all in flight together.
// ---------------------------------------------------------------------------------------------
struct nnsdp_batch {
  std::vector<nnsdp_solver*> all;      // as given
  std::vector<nnsdp_solver*> act;      // still iterating
  std::vector<int> status;             // per solver of `all`, -1 while active
  hipStream_t st = nullptr;
  DBuf<IterArgs> d_it;
  DBuf<ProjArgs> d_pw, d_pc;           // warm / cold projection arguments
  DBuf<int2> d_map;
  // members of a solver family with a dense inverse: ONE pass over their common M^-1 per kFusedWidth members (k_minv_family) instead
  // of a tiled product per member.  d_it_sym lists the members that keep the per-member stage when the batch holds families.
  DBuf<IterArgs> d_it_sym;
  DBuf<int> d_fmem;
  DBuf<FusedPass> d_fpass;
  int n_sym = 0, n_fgroups = 0, n_fmembers = 0, n_fpass = 0;
  // members of a solver family with a structured inverse: the four stages of minv.hpp once per kMinvWidth members of a group
  // (k_minv_*_multi) instead of four launches per member.  A group of one keeps its member's own launches (equal bits); so does a
  // group whose factors are too large to stage in LDS, and every group under NNSDP_FAMILY_STRUCT=0 (diagnostic).
  DBuf<MinvFactors> d_sfac;
  DBuf<MinvWork> d_swork;
  DBuf<MinvPass> d_spass;
  MinvMultiGrid sgrid;
  int n_sgroups = 0, n_smembers = 0, n_spass = 0;
  std::vector<nnsdp_solver*> struct_single;      // structured members that take their own four launches, in batch order
  int nblocks = 0, nmax = 0;
  bool any_structured = false, any_big = false;
  ProjPlan plan;
  TailGrid grid;                       // per stage, the largest member's block count (admm_tail.hpp)
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  static constexpr int kGraphIters = 8;

  ~nnsdp_batch() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (st) (void)hipStreamDestroy(st);
  }

  void create(nnsdp_solver** sv, int count) {
    if (!sv || count <= 0) throw std::invalid_argument("batch needs at least one solver");
    for (int i = 0; i < count; ++i) {
      if (!sv[i]) throw std::invalid_argument("null solver in batch");
      if (sv[i]->sharded) throw std::invalid_argument("clique-sharded solvers cannot be batched");
      if (sv[i]->opt.device != sv[0]->opt.device) throw std::invalid_argument("batched solvers must live on one device");
      if (sv[i]->opt.check_every != sv[0]->opt.check_every) throw std::invalid_argument("batched solvers must share check_every");
      // (one kernel variant per batched launch, chosen from proj_refine: members that disagree would silently lose - or get - the
      // refinement stage, and the variant would change whenever the first member finishes)
      if ((sv[i]->opt.proj_refine != 0) != (sv[0]->opt.proj_refine != 0)) throw std::invalid_argument("batched solvers must share proj_refine (on / off)");
      for (int j = 0; j < i; ++j) if (sv[j] == sv[i]) throw std::invalid_argument("a solver appears twice in the batch");
      all.push_back(sv[i]);
    }
    if (sv[0]->opt.device >= 0) HIPCHK(hipSetDevice(sv[0]->opt.device));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    status.assign(count, -1);
    act = all;
    rebuild();
  }

  void rebuild() {
    if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    n_sym = n_fgroups = n_fmembers = n_fpass = 0;
    n_sgroups = n_smembers = n_spass = 0; sgrid = MinvMultiGrid(); struct_single.clear();
    if (act.empty()) return;
    std::vector<IterArgs> it;
    std::vector<ProjArgs> pw, pc;
    std::vector<int2> map;
    nmax = 0; grid = TailGrid();
    any_structured = false; any_big = false;
    std::vector<IterArgs> it_sym;
    std::vector<std::pair<int, std::vector<int>>> fam;      // family id -> its dense members here, in batch order
    std::vector<std::pair<int, std::vector<int>>> sfam;     // family id -> its structured members here, in batch order
    static const bool fuse_struct = env_int("NNSDP_FAMILY_STRUCT", 1) != 0;   // diagnostic: 0 keeps the per-member launches
    for (size_t b = 0; b < act.size(); ++b) {
      nnsdp_solver* s = act[b];
      any_structured = any_structured || s->minv_structured;
      const bool fused = s->family != 0 && !s->minv_structured;      // (always, also alone: a member's bits must not depend on its group's size)
      if (fused) {
        auto f = std::find_if(fam.begin(), fam.end(), [&](const std::pair<int, std::vector<int>>& x) { return x.first == s->family; });
        if (f == fam.end()) { fam.emplace_back(s->family, std::vector<int>()); f = fam.end() - 1; }
        f->second.push_back((int)b);
      }
      if (s->minv_structured && s->family != 0 && s->m_lds.ok && fuse_struct) {
        auto f = std::find_if(sfam.begin(), sfam.end(), [&](const std::pair<int, std::vector<int>>& x) { return x.first == s->family; });
        if (f == sfam.end()) { sfam.emplace_back(s->family, std::vector<int>()); f = sfam.end() - 1; }
        f->second.push_back((int)b);
      }
      HIPCHK(hipStreamSynchronize(s->st));
      s->since_cold = nnsdp_solver::kColdPeriod;   // lockstep: the next batched iteration is a cold one for everybody
      IterArgs a = s->iter_args();
      TailGrid mine(a);
      if (fused) { a.symv_part = nullptr; mine.tiles = mine.nb = 0; }      // (the family pass; the tiled product's grid covers the others only)
      else {
        const size_t nb = (size_t)mine.nb;
        if (!s->minv_structured && s->symv_part.n != nb * nb * 64) s->symv_part.alloc(nb * nb * 64);
        a.symv_part = s->symv_part.p;
        mine.family = 0;
        if (!s->minv_structured) it_sym.push_back(a);
      }
      grid.cover(mine);
      it.push_back(a);
      pw.push_back(s->proj_args(true));      // (k0 = 0, k1 = ncl: create() refuses sharded solvers)
      pc.push_back(s->proj_args(false));
      // blocks up to 128 of every SDP share ONE launch of the LDS-resident kernel; blocks above (the reference's 151-wide cliques of
      // width-50 nets) follow per SDP through the library path on the batch's stream (eager: rocSOLVER is not captured into the graph)
      if (s->big_idx.empty()) {
        for (int k = 0; k < s->ncl; ++k) { map.push_back(make_int2((int)b, k)); nmax = std::max(nmax, s->cn[k]); }
      } else {
        // (the solver's compact list of its blocks up to 128, as its own launches use it: same slots, same back-off state)
        pw.back().cn = s->d_cn_s.p; pw.back().coff = s->d_coff_s.p;
        pc.back().cn = s->d_cn_s.p; pc.back().coff = s->d_coff_s.p;
        for (size_t pos = 0; pos < s->proj_small.size(); ++pos) { map.push_back(make_int2((int)b, (int)pos)); nmax = std::max(nmax, s->cn[s->proj_small[pos]]); }
        any_big = true;
      }
    }
    nblocks = (int)map.size();
    nmax = std::max(nmax, 1);
    plan = plan_projection(nmax, !act.empty() && act[0]->opt.proj_refine != 0);
    if (plan.packed())          // one launch for all members in the packed variant: every member needs its warm-start scratch
      for (size_t b = 0; b < act.size(); ++b) {
        if (!act[b]->Tg.p) { act[b]->Tg.alloc(act[b]->nmat); act[b]->Tg.zero(); pw[b].Tg = pc[b].Tg = act[b]->Tg.p; }
        if (!act[b]->Ug.p) { act[b]->Ug.alloc(act[b]->nmat); act[b]->Ug.zero(); pw[b].Ug = pc[b].Ug = act[b]->Ug.p; }
      }
    HIPCHK(proj_allow_big_lds(plan));
    d_it.upload(it); d_pw.upload(pw); d_pc.upload(pc); d_map.upload(map);
    {
      std::vector<MinvFactors> sfac;
      std::vector<MinvWork> swork;
      std::vector<MinvPass> spass;
      std::vector<char> in_group(act.size(), 0);
      for (auto& f : sfam) {
        if (f.second.size() < 2) continue;      // a group of one: the member's own launches
        nnsdp_solver* head = act[f.second[0]];
        sgrid.add(head->mdev, head->m_lds, (int)std::min<size_t>(kMinvWidth, f.second.size()));
        for (size_t o = 0; o < f.second.size(); o += kMinvWidth) {
          const int cnt = (int)std::min<size_t>(kMinvWidth, f.second.size() - o);
          spass.push_back(MinvPass{(int)sfac.size(), (int)swork.size(), cnt});
          for (int i = 0; i < cnt; ++i) { nnsdp_solver* s = act[f.second[o + i]]; swork.push_back(s->structured_work(s->qv.p, s->ww.p)); in_group[f.second[o + i]] = 1; }
        }
        sfac.push_back(head->mdev);
        ++n_sgroups;
      }
      for (size_t b = 0; b < act.size(); ++b) if (act[b]->minv_structured && !in_group[b]) struct_single.push_back(act[b]);
      n_smembers = (int)swork.size(); n_spass = (int)spass.size();
      if (n_spass) { d_sfac.upload(sfac); d_swork.upload(swork); d_spass.upload(spass); HIPCHK(minv_multi_allow_lds()); }
    }
    if (!fam.empty()) {
      std::vector<int> fmem;
      std::vector<FusedPass> fpass;
      for (auto& f : fam)
        for (size_t o = 0; o < f.second.size(); o += kFusedWidth) {
          const int cnt = (int)std::min<size_t>(kFusedWidth, f.second.size() - o);
          fpass.push_back(FusedPass{(int)fmem.size(), cnt});
          fmem.insert(fmem.end(), f.second.begin() + o, f.second.begin() + o + cnt);
        }
      n_fgroups = (int)fam.size(); n_fmembers = (int)fmem.size(); n_fpass = (int)fpass.size();
      n_sym = (int)it_sym.size();
      d_fmem.upload(fmem); d_fpass.upload(fpass);
      if (n_sym) d_it_sym.upload(it_sym);
    }
  }

  // the structured members: four launches for all fused groups together, then the members outside a group
  void enqueue_structured() {
    if (n_spass > 0) launch_minv_multi(sgrid, d_sfac.p, d_swork.p, d_spass.p, n_spass, st);
    for (nnsdp_solver* s : struct_single) s->enqueue_minv(st);
  }

  void enqueue_iteration(bool warm) {
    const int B = (int)act.size();
    if (nblocks > 0) launch_proj_batched(plan, warm ? d_pw.p : d_pc.p, d_map.p, nblocks, st);
    if (any_big) for (nnsdp_solver* s : act) s->enqueue_big_blocks(st);
    launch_gather(grid, d_it.p, B, st);
    launch_At(grid, d_it.p, B, st);
    static const bool full_gemv = env_flag("NNSDP_BATCH_FULL_GEMV");   // diagnostic
    if (n_fpass > 0) {
      // the batch holds family members: one pass per group over the common inverse; structured members and solvers of no family
      // take the stage they take without families around (d_it_sym: the dense ones among them)
      launch_minv_family(grid, d_it.p, d_fmem.p, d_fpass.p, n_fpass, st);
      if (any_structured) { enqueue_structured(); for (nnsdp_solver* s : act) if (!s->minv_structured && s->family == 0) s->enqueue_minv(st); }
      else if (n_sym > 0 && full_gemv) launch_gemv(grid, d_it_sym.p, n_sym, st);
      else if (n_sym > 0) launch_symv(grid, d_it_sym.p, n_sym, st);
    }
    else if (any_structured) { enqueue_structured(); for (nnsdp_solver* s : act) if (!s->minv_structured) s->enqueue_minv(st); }     // large multiplier counts: each SDP's structured M^-1
    else if (full_gemv) launch_gemv(grid, d_it.p, B, st);
    else launch_symv(grid, d_it.p, B, st);
    launch_Ax(grid, d_it.p, B, st);
    launch_update(grid, d_it.p, B, st);
    HIPCHK(hipGetLastError());
  }

  // n plain iterations of every active solver (no residual checks, no adaptation); synchronous
  void iterate(int n) {
    if (n <= 0 || act.empty()) return;
    int left = n;
    while (left > 0) {
      const int sc = act[0]->since_cold;   // equal for all active solvers
      const bool warm_ok = act[0]->opt.warm_start != 0 && sc < nnsdp_solver::kColdPeriod;
      int did;
      static const bool no_graph = env_flag("NNSDP_NO_GRAPH");   // diagnostic: eager launches only
      const int giters = nnsdp_solver::graph_iters_for(act[0]->opt.check_every);      // (equal for all members)
      if (!no_graph && !any_big && warm_ok && left >= giters && nnsdp_solver::kColdPeriod - sc >= giters) {
        if (!gexec) {
          HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
          for (int i = 0; i < giters; ++i) enqueue_iteration(true);
          HIPCHK(hipStreamEndCapture(st, &graph));
          HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
        }
        HIPCHK(hipGraphLaunch(gexec, st));
        for (nnsdp_solver* s : act) ++s->graph_launches;      // (nnsdp_solver_info 0: the replay advanced every member)
        did = giters;
      } else {
        enqueue_iteration(warm_ok);
        did = 1;
      }
      for (nnsdp_solver* s : act) {
        s->iters_done += did;
        s->since_cold = (did == 1 && !warm_ok) ? 1 : s->since_cold + did;
      }
      left -= did;
    }
    HIPCHK(hipStreamSynchronize(st));
  }

  // full solves with the stopping rules of nnsdp_solver::run_loop, each SDP on its own
  void run() {
    double t0 = now_s();
    for (nnsdp_solver* s : act) s->loop_begin();
    while (!act.empty()) {
      long long n = act[0]->opt.check_every - 1;
      for (nnsdp_solver* s : act) n = std::min<long long>(n, (long long)s->opt.max_iters - s->iters_done - 1);
      iterate((int)std::max<long long>(n, 0));
      for (nnsdp_solver* s : act) s->check_enqueue();
      for (nnsdp_solver* s : act) s->check_finish();
      std::vector<nnsdp_solver*> keep;
      for (nnsdp_solver* s : act) {
        int stt = s->post_check(false, t0);
        if (stt < 0 && s->iters_done >= s->opt.max_iters) stt = NNSDP_STATUS_ITERATION_LIMIT;
        if (stt >= 0) {
          for (size_t i = 0; i < all.size(); ++i) if (all[i] == s) status[i] = stt;
          s->t_solve += now_s() - t0;
        } else keep.push_back(s);
      }
      if (keep.size() != act.size()) { act = keep; rebuild(); }
    }
  }
};
