// part of engine.hip (included there, not compiled alone): the polishes of DIFFERENT models beyond one workgroup's LDS in
// one launch (C ABI miosqp_qp_polish_models_large; kernel k_pol_many_gm in polish_many_large.hip; fit rule, workgroups
// and arena layout in polish_models_large_plan.hpp, argument checks in polish_models_plan.hpp).  This is
// polish_models_run with another plan and another launch: no engine's polish scratch is built or touched -- the unscaled
// rows of A by constraint and by variable travel in the call's arena (an engine that has the single polish's scratch
// lends its copies), everything else of a model is on the device since its set-up --, and the arena, now with the
// workgroups' slabs behind the records, is the one miosqp_qp_solve_trees_models keeps in engines[0] (models_reserve).
static int polish_models_large_run(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                   const double *const *u, const double *const *x, const double *const *y, double tau,
                                   const double *delta, const int32_t *refine_iter, const int32_t *repair_iter,
                                   double *const *x_out, double *const *y_out, int8_t *const *cls_out,
                                   miosqp_polish_repair_info *info, miosqp_polish_models_large_stats *stats) {
  namespace pm = miosqp::polish_models;
  namespace pl = miosqp::polish_models_large;
  const std::string who = std::string(pl::ENTRY) + ": ";
  // ---- refused before anything is queued ----
  {
    std::vector<int> nv, Mv;
    if (B >= 1 && engines)
      for (int b = 0; b < B; b++) {
        nv.push_back(engines[b] ? engines[b]->n : 0);
        Mv.push_back(engines[b] ? engines[b]->M : 0);
      }
    std::string err;
    if (int rc = pm::check_args(B, (const void *const *)engines, nv.data(), Mv.data(), q, l, u, x, y, tau, delta, refine_iter,
                                repair_iter, (const void *const *)x_out, (const void *const *)y_out, info, stats, err, pl::ENTRY)) {
      g_err = err;
      return rc;
    }
  }
  *stats = miosqp_polish_models_large_stats{};
  miosqp_qp_engine *e0 = engines[0];
  std::vector<pl::Shape> sh((size_t)B);
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    if (e->device != e0->device) {
      g_err = who + "model " + std::to_string(b) + " lives on device " + std::to_string(e->device) + ", model 0 on device " +
              std::to_string(e0->device);
      return MIOSQP_EARG;
    }
    if (e->pool_pending) {
      g_err = who + "streaming chunks are still in flight (pool_collect first), model " + std::to_string(b);
      return MIOSQP_EARG;
    }
    sh[(size_t)b] = pl::Shape{e->n, e->M, e->pol ? (size_t)0 : e->fa.panel_by_con.idx.size(),
                              e->pol ? (size_t)0 : e->fa.panel_by_var.idx.size(), q[b] != nullptr, y[b] != nullptr};
  }
  {
    std::string err;
    if (int rc = pl::check_fit(sh, err)) {
      g_err = err;
      return rc;
    }
  }
  ENTER(e0);
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e0->device));
  const pl::Plan P = pl::plan(sh, cus);
  if (P.W < 1) {
    g_err = who + "the largest slab of the call exceeds the budget";
    return MIOSQP_EUNSUPPORTED;
  }
  if (int rc = models_reserve(e0, P.total_doubles, P.pinned_doubles)) return rc;
  const double t0 = wall();
  double *hs = e0->mm_host, *dv = e0->mm_dev;
  // ---- the staged part: every model's rows of A both ways, its vectors, its table entry ----
  miosqp::PolManyLargeModel *tab_h = reinterpret_cast<miosqp::PolManyLargeModel *>(hs);
  const miosqp::PolManyLargeModel *tab_d = reinterpret_cast<const miosqp::PolManyLargeModel *>(dv);
  std::vector<double> by_var;
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    const pl::Slot &s = P.slot[(size_t)b];
    const size_t n = (size_t)e->n, M = (size_t)e->M;
    if (s.A != pm::NONE) {
      if (!polish_raw_rows(e, hs + s.A, &by_var) || by_var.size() != sh[(size_t)b].rows_var) {
        g_err = who + "the rows of A of model " + std::to_string(b) +
                " on the device do not follow the order of the matrix given at set-up: polish that model on its own";
        return MIOSQP_EUNSUPPORTED;
      }
      if (!by_var.empty()) memcpy(hs + s.At, by_var.data(), sizeof(double) * by_var.size());
    }
    if (s.q != pm::NONE) memcpy(hs + s.q, q[b], sizeof(double) * n);
    memcpy(hs + s.l, l[b], sizeof(double) * M);
    memcpy(hs + s.u, u[b], sizeof(double) * M);
    memcpy(hs + s.x, x[b], sizeof(double) * n);
    if (s.y != pm::NONE) memcpy(hs + s.y, y[b], sizeof(double) * M);
    miosqp::PolManyLargeModel &t = tab_h[b];
    memset(&t, 0, sizeof t);
    miosqp::PolManyArgs &a = t.g.a;
    const Dev &d = e->d;
    a.n = e->n; a.M = e->M; a.B = 1; a.refine_iter = refine_iter[b]; a.repair_iter = repair_iter[b];
    a.delta = delta[b]; a.inv_delta = 1.0 / delta[b];
    a.pc_ptr = d.pc_ptr; a.pc_idx = d.pc_idx; a.pr_ptr = d.pr_ptr; a.pr_idx = d.pr_idx;
    a.A = s.A != pm::NONE ? dv + s.A : e->pol->p.A;
    a.pr_val = d.pr_val;
    a.q = s.q != pm::NONE ? dv + s.q : nullptr;
    a.q_engine = d.qraw;
    a.l = dv + s.l; a.u = dv + s.u; a.x = dv + s.x;
    a.y = s.y != pm::NONE ? dv + s.y : nullptr;
    a.out = dv + s.out;
    t.g.pv_ptr = d.pv_ptr; t.g.pv_idx = d.pv_idx;
    t.g.At = s.At != pm::NONE ? dv + s.At : e->pol->p.At;
    t.tau = tau;
  }
  // every other engine's stream in front of the launch: an update of its cost or its set-up queued there has finished
  for (int b = 1; b < B; b++) {
    if (int rc = stage_wait(engines[b], 0)) return rc;
    if (int rc = stage_wait(engines[b], 1)) return rc;
    if (engines[b]->stream != e0->stream) HIPCHK(hipStreamSynchronize(engines[b]->stream));
  }
  // ---- one upload, one launch, one download, one synchronisation ----
  hipStream_t st = e0->stream;
  HIPCHK(hipEventRecord(e0->ev0, st));
  HIPCHK(hipMemcpyAsync(dv, hs, sizeof(double) * P.up_doubles, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(e0->evc0, st));
  if (int lrc = miosqp::polish_models_large_launch(tab_d, B, P.W, dv + P.slab_off, P.slab_doubles, (void *)st)) {
    set_err("polish_models_large: launch", (hipError_t)lrc, __FILE__, __LINE__);
    return MIOSQP_EHIP;
  }
  HIPCHK(hipEventRecord(e0->evc1, st));
  HIPCHK(hipMemcpyAsync(hs + P.down_off, dv + P.down_off, sizeof(double) * P.down_doubles, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(e0->ev1, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0, ms_up = 0, ms_run = 0, ms_down = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0->ev0, e0->ev1));
  HIPCHK(hipEventElapsedTime(&ms_up, e0->ev0, e0->evc0));
  HIPCHK(hipEventElapsedTime(&ms_run, e0->evc0, e0->evc1));
  HIPCHK(hipEventElapsedTime(&ms_down, e0->evc1, e0->ev1));
  for (int b = 0; b < B; b++) {
    const size_t n = (size_t)engines[b]->n, M = (size_t)engines[b]->M;
    const double *o = hs + P.slot[(size_t)b].out;
    const miosqp::PolManyRec &r = *(const miosqp::PolManyRec *)o;
    miosqp_polish_repair_info &f = info[b];
    f.polish.accepted = r.accepted;
    f.polish.reason = r.reason;
    f.polish.n_lower = r.n_lower;
    f.polish.n_upper = r.n_upper;
    f.polish.pri_before = r.pri_before;
    f.polish.dua_before = r.dua_before;
    f.polish.pri_after = r.pri_after;
    f.polish.dua_after = r.dua_after;
    f.polish.obj = r.obj;
    f.polish.device_time = 1e-3 * ms;
    f.rounds = r.rounds;
    f.stop = r.stop;
    f.n_added = r.n_added;
    f.n_dropped = r.n_dropped;
    f.accepted0 = r.accepted0;
    f.reason0 = r.reason0;
    memcpy(x_out[b], o + miosqp::POLM_REC_DOUBLES, sizeof(double) * n);
    memcpy(y_out[b], o + miosqp::POLM_REC_DOUBLES + n, sizeof(double) * M);
    if (cls_out && cls_out[b]) memcpy(cls_out[b], o + miosqp::POLM_REC_DOUBLES + n + M, M);
  }
  const double rt = wall() - t0;
  for (int b = 0; b < B; b++) info[b].polish.run_time = rt;
  stats->launches = 1;
  stats->models = B;
  stats->workgroups = P.W;
  stats->slab_bytes = (int64_t)(P.slab_doubles * sizeof(double));
  stats->arena_bytes = (int64_t)(P.total_doubles * sizeof(double));
  stats->device_time = 1e-3 * ms;
  stats->run_time = rt;
  stats->upload_time = 1e-3 * ms_up;
  stats->launch_time = 1e-3 * ms_run;
  stats->download_time = 1e-3 * ms_down;
  return 0;
}
