// part of engine.hip (included there behind trees_run, not compiled alone): B MIQPs on ONE model beyond one workgroup's
// product form, every tree in one launch in the reduced form (C ABI miosqp_qp_solve_trees_large, _rf, _sb; kernels
// k_tree_r / k_tree_rf_r / k_tree_sb_r in kernels_tree.inc; the layout of the batch's arena in trees_large_plan.hpp).
// trees_run for an engine whose tree_form_large_of is 3: the same arguments and layouts, the kernel and its settings
// (sp_off, pv_off, r_dense, TG1) chosen as models_run chooses them for that engine, so that an instance comes out bit for
// bit as miosqp_qp_solve_trees_models_large gives it alone.
static int trees_large_run(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u, const double *x0,
                           const double *y0, const double *upper0, const double *x_inc0, int32_t tree_explor_rule,
                           int32_t max_iter_bb, int32_t leaf_cap, double *x_out, miosqp_tree_info *info,
                           int32_t rf_candidates = 0, int32_t rf_max_iter = 0, int32_t rf_every = 0,
                           miosqp_tree_rf_info *rf_info = nullptr, const TreesSb *sb = nullptr) {
  namespace tl = miosqp::trees_large;
  // ---- refused before anything is queued ----
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || max_iter_bb < 1 || tree_explor_rule < 0 ||
      tree_explor_rule > 3)
    return MIOSQP_EARG;
  if (leaf_cap < 2) {  // (the rule of check_leaf_cap: room for the two children of the root's branching)
    g_err = "solve_trees_large: leaf_cap must be at least 2 (got " + std::to_string(leaf_cap) + ")";
    return MIOSQP_EARG;
  }
  ENTER(e);
  {
    const int form = tree_form_large_of(e, leaf_cap);
    if (form < 0) return form;
    if (form != 3) {
      g_err = "solve_trees_large: only for an engine beyond the other one-launch forms whose packed triangle of L^-1, iterates "
              "and leaf list fit 160 KB of LDS (miosqp_qp_tree_form_large)";
      return MIOSQP_EUNSUPPORTED;
    }
  }
  const int n = e->n, M = e->M, p = e->d.n_int;
  const size_t blk = 3 * (size_t)M + n;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) return MIOSQP_EBOUNDS;
  tl::Plan P;
  {
    std::string err;
    int rc = tl::plan(n, M, p, B, leaf_cap, rf_info ? tl::RF : sb ? tl::SB : tl::PLAIN, P, err);
    if (!rc && P.total_doubles > e->tl_cap) {  // the leaf stores are the large part: refused by name, not a failed allocation
      size_t fr = 0, tot = 0;
      HIPCHK(hipMemGetInfo(&fr, &tot));
      const size_t room = fr > ((size_t)256 << 20) ? fr - ((size_t)256 << 20) : 0;
      rc = tl::check_room(P, B, std::max(e->tl_cap * sizeof(double), room) / sizeof(double), err);
    }
    if (rc) {
      g_err = err;
      return rc;
    }
  }
  const double t0 = wall();
  if (P.total_doubles > e->tl_cap) {  // (a larger batch takes a new arena; the old one stays with the pool until cleanup)
    size_t cap = std::max(P.total_doubles, 2 * e->tl_cap);
    if (cap > P.total_doubles) {  // (growing ahead only where the device has the room)
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess || cap * sizeof(double) + 4096 > fr / 2) cap = P.total_doubles;
    }
    int rc = pool_reserve(e, cap * sizeof(double) + 4096);
    if (!rc) rc = dalloc(e, &e->tl_dev, cap);
    if (rc) return rc;
    e->tl_cap = cap;
  }
  TreeArgs ta{};
  const void *kernel = rf_info ? (const void *)k_tree_rf_r : sb ? (const void *)k_tree_sb_r : (const void *)k_tree_r;
  HIPCHK(lds_limit_once(kernel, rf_info ? 26 : sb ? 27 : 25));
  const size_t lds = tree_r_lds_bytes(e, leaf_cap, &ta.sp_off, &ta.pv_off);
  // ---- the staged part: roots, costs, incumbents' values, incumbents, cleared records ----
  static_assert(sizeof(TreeOut) == tl::OUT_DOUBLES * sizeof(double), "TreeOut is the stride of its array in the arena");
  static_assert(sizeof(TreeRfOut) == tl::RF_DOUBLES * sizeof(double), "TreeRfOut is the stride of its array in the arena");
  static_assert(sizeof(TreeSbOut) == tl::SB_DOUBLES * sizeof(double), "TreeSbOut is the stride of its array in the arena");
  if (e->tl_host.size() < P.up_doubles) e->tl_host.resize(P.up_doubles);
  double *hs = e->tl_host.data(), *dv = e->tl_dev;
  memset(hs, 0, sizeof(double) * P.up_doubles);
  for (int b = 0; b < B; b++) {
    double *r = hs + P.raw + (size_t)b * blk;
    memcpy(r, l + (size_t)b * M, sizeof(double) * M);
    memcpy(r + M, u + (size_t)b * M, sizeof(double) * M);
    memcpy(r + 2 * (size_t)M, x0 + (size_t)b * n, sizeof(double) * n);
    memcpy(r + 2 * (size_t)M + n, y0 + (size_t)b * M, sizeof(double) * M);
    const bool have = x_inc0 != nullptr && upper0[b] < 1.7e308;
    hs[P.upper + b] = have ? upper0[b] : 1.0 / 0.0;
    if (have) memcpy(hs + P.inc + (size_t)b * n, x_inc0 + (size_t)b * n, sizeof(double) * n);
  }
  memcpy(hs + P.qraw, q, sizeof(double) * (size_t)B * n);
  ta.rule = tree_explor_rule;
  ta.max_nodes = max_iter_bb;
  ta.max_iter = e->st.max_iter;
  ta.check_every = e->st.check_termination;
  tree_lane_groups(n, M, ta);
  ta.TG1 = miosqp::tree_reduced::TGR;  // rows of Abar in the prologue, the test and the epilogue: as the iteration walks them
  ta.upper0 = 1.0 / 0.0;
  ta.lf_lo = dv + P.lf_lo; ta.lf_hi = dv + P.lf_hi; ta.lf_x = dv + P.lf_x; ta.lf_y = dv + P.lf_y;
  ta.inc_x = dv + P.inc;
  ta.out = reinterpret_cast<TreeOut *>(dv + P.out);
  ta.done = nullptr;
  ta.batch = 1;
  ta.upper_b = dv + P.upper;
  ta.leaf_cap = leaf_cap;
  ta.r_dense = tree_r_dense(e);
  if (rf_info) {
    ta.rf_K = rf_candidates;
    ta.rf_max_iter = rf_max_iter;
    ta.rf_every = rf_every;
    ta.rf_out = reinterpret_cast<TreeRfOut *>(dv + P.rf);
  }
  if (sb) {
    ta.sb_rule = sb->rule;
    ta.sb_K = sb->K;
    ta.sb_max_iter = sb->max_iter;
    ta.sb_rel = sb->reliability;
    ta.sb_eps = sb->eps;
    ta.sb_work = dv + P.sb_work;
    ta.sb_pc = dv + P.sb_pc;
    ta.sb_out = reinterpret_cast<TreeSbOut *>(dv + P.sb);
  }
  Dev db = e->d;  // instance 0's arrays; workgroup b moves on from there (tree_instance)
  db.q = dv + P.q;
  db.qraw = dv + P.qraw;
  db.raw_l = dv + P.raw;
  db.raw_u = dv + P.raw + M;
  db.raw_x = dv + P.raw + 2 * (size_t)M;
  db.raw_y = dv + P.raw + 2 * (size_t)M + n;
  db.prof = nullptr;
  // ---- one upload, the costs scaled, one tree launch, one download, one synchronisation ----
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  HIPCHK(hipMemcpyAsync(dv, hs, sizeof(double) * P.up_doubles, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, e->d, dv + P.qraw,
                     dv + P.q, B);
  if (rf_info) hipLaunchKernelGGL(k_tree_rf_r, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  else if (sb) hipLaunchKernelGGL(k_tree_sb_r, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  else hipLaunchKernelGGL(k_tree_r, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  HIPCHK(hipMemcpyAsync(hs + P.down_off, dv + P.down_off, sizeof(double) * P.down_doubles, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  int64_t iters = 0;
  for (int b = 0; b < B; b++) {
    TreeOut o;
    memcpy(&o, hs + P.out + (size_t)b * tl::OUT_DOUBLES, sizeof o);
    info[b].nodes = o.nodes;
    info[b].osqp_iter = o.osqp_iter;
    info[b].leaves_left = o.leaves_left;
    info[b].overflow = o.overflow;
    info[b].max_leaves = o.max_leaves;
    info[b].found = o.found;
    info[b].upper_glob = o.upper;
    info[b].lower_glob = o.lower_glob;
    info[b].device_time = 1e-3 * ms / B;  // the launch's device time, shared equally
    info[b].run_time = wall_s / B;
    const bool have = x_inc0 != nullptr && upper0[b] < 1.7e308;
    if (o.found) memcpy(x_out + (size_t)b * n, hs + P.inc + (size_t)b * n, sizeof(double) * n);
    else if (have) memcpy(x_out + (size_t)b * n, x_inc0 + (size_t)b * n, sizeof(double) * n);
    iters += o.osqp_iter;
    if (rf_info) {
      TreeRfOut r;
      memcpy(&r, hs + P.rf + (size_t)b * tl::RF_DOUBLES, sizeof r);
      rf_info[b] = miosqp_tree_rf_info{r.calls, r.candidates, r.feasible, r.improved, r.osqp_iter, 5, 0, 0};
    }
    if (sb) {
      TreeSbOut r;
      memcpy(&r, hs + P.sb + (size_t)b * tl::SB_DOUBLES, sizeof r);
      sb->info[b] = miosqp_tree_sb_info{r.calls, r.children, r.osqp_iter, 7, 0, 0, 0, 0};
    }
  }
  e->loop_ms += ms;
  e->loop_iters += iters;
  return 0;
}

int miosqp_qp_solve_trees_large(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, double *x_out,
                                miosqp_tree_info *info) {
  return trees_large_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap, x_out, info);
}

int miosqp_qp_solve_trees_large_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, int32_t rf_candidates,
                                   int32_t rf_max_iter, int32_t rf_every, double *x_out, miosqp_tree_info *info,
                                   miosqp_tree_rf_info *rf_info) {
  std::string err;
  if (int rc = miosqp::models::check_rf(1, &rf_candidates, &rf_max_iter, &rf_every, rf_info, 1, "solve_trees_large_rf", err)) {
    g_err = err;
    return rc;
  }
  return trees_large_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap, x_out, info,
                         rf_candidates, rf_max_iter, rf_every, rf_info);
}

int miosqp_qp_solve_trees_large_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, int32_t branching_rule,
                                   int32_t sb_candidates, int32_t sb_max_iter, int32_t sb_reliability, double sb_eps,
                                   double *x_out, miosqp_tree_info *info, miosqp_tree_sb_info *sb_info) {
  std::string err;
  if (int rc = miosqp::models::check_sb(1, &branching_rule, &sb_candidates, &sb_max_iter, &sb_reliability, &sb_eps, sb_info, 1,
                                        "solve_trees_large_sb", err)) {
    g_err = err;
    return rc;
  }
  const TreesSb sb{branching_rule, sb_candidates, sb_max_iter, sb_reliability, sb_eps, sb_info};
  return trees_large_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap, x_out, info, 0, 0, 0,
                         nullptr, &sb);
}
