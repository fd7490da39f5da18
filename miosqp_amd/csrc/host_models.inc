// part of engine.hip (included there, not compiled alone): what the one-launch tree entries share, and the trees of
// DIFFERENT models in one launch (C ABI miosqp_qp_tree_form, miosqp_qp_solve_trees_models, and with the reduced form for
// models beyond one workgroup's product form miosqp_qp_tree_form_large, miosqp_qp_solve_trees_models_large; kernels
// k_tree_m / k_tree_w_m / k_tree_r_m / k_scale_q_models in kernels_tree.inc; argument checks and arena layout in
// models_plan.hpp).  With round and fix inside the trees (miosqp_qp_solve_trees_models_rf): the models that have it on
// form up to two more launches, k_tree_rf_m and k_tree_rf_r_m, behind the other three.  With strong / reliability
// branching inside the trees (miosqp_qp_solve_trees_models_sb): the models with a rule form the launches k_tree_sb_m and
// k_tree_sb_r_m in the same way.
extern "C" {
static int stage_wait(miosqp_qp_engine *e, int k);
}

namespace {

// dynamic LDS of k_tree for this engine as it stands, and where the LDS copy of the sparse rows starts inside it (or -1)
size_t tree_lds_bytes(const miosqp_qp_engine *e, int *sp_off) {
  const int n = e->n, M = e->M;
  // (the tree kernels decide the same way on the device: explicit inverse there and n + M small enough -> no product
  //  form in LDS; an engine without W yet gets it in tree_wave_prepare when n + M <= 64, which only shrinks what the kernel uses)
  const bool tree_w = e->d.W != nullptr && n + M <= RES_W_MAX;
  size_t lds = tree_lds_doubles(n, M, tree_w) * sizeof(double);
  *sp_off = -1;
  const size_t sp_bytes = res_sp_doubles(e->sp_nnzA, e->sp_nnzP, n, M) * sizeof(double);
  if (tree_w && e->sp_nnzA > 0 && lds + sp_bytes <= 160 * 1024 && !(getenv("MIOSQP_RES_SP") && atoi(getenv("MIOSQP_RES_SP")) == 0)) {
    *sp_off = (int)(lds / sizeof(double));
    lds += sp_bytes;
  }
  return lds;
}

// n + M <= 64: the whole search in ONE wavefront on the explicit KKT inverse (k_tree_w); MIOSQP_TREE_WAVE=0 keeps k_tree.
// An engine in the LDS-resident form has not built Kc (and perhaps W) yet: built here, once, and the inverse is checked.
int tree_wave_prepare(miosqp_qp_engine *e, bool *wave_out) {
  const int n = e->n, M = e->M;
  bool wave = n + M <= TW && !e->guard_tripped && !(getenv("MIOSQP_TREE_WAVE") && atoi(getenv("MIOSQP_TREE_WAVE")) == 0);
  if (wave && !e->d.Kc) {
    Dev &d = e->d;
    const int N = n + M;
    d.ldw = (N + 7) & ~7;
    double *Wd = const_cast<double *>(d.W), *Kc = nullptr;
    int rcw = 0;
    if (!Wd) {
      rcw = dalloc(e, &Wd, (size_t)N * d.ldw + 64);
      if (!rcw) rcw = miosqp_device_kkt_inverse(d.f_rows, d.ldf, d.d2inv, n, M, Wd, d.ldw, e->stream);
    }
    if (!rcw) rcw = dalloc(e, &Kc, (size_t)N * d.ldw + 64);
    if (rcw) return rcw;
    d.W = Wd;
    d.Kc = Kc;
    hipLaunchKernelGGL(k_build_kc, dim3((N + 255) / 256, N), dim3(256), 0, e->stream, d, Kc);
    if (int rcg = inverse_guard(e)) return rcg;
    if (e->guard_tripped) {  // (kernels_guard.inc) the explicit inverse failed its check: the workgroup kernel with the sweeps
      d.W = nullptr;
      d.Kc = nullptr;
      wave = false;
    }
  }
  *wave_out = wave;
  return 0;
}

// lanes per row of the two sweeps, as the LDS-resident solver picks them
void tree_lane_groups(int n, int M, TreeArgs &ta) {
  auto pow2_floor = [](int v) { int q = 1; while (2 * q <= v) q *= 2; return q; };
  ta.TG1 = std::min(64, std::max(1, pow2_floor(RES_THREADS / n)));
  ta.TG2 = std::min(64, std::max(1, pow2_floor(RES_THREADS / (n + M))));
}

// miosqp_qp_tree_form without the entry's own checks: 0, 1, 2, or a negative error code of the lazy build
int tree_form_of(miosqp_qp_engine *e) {
  if (!e->have_int || !e->d.digest) return 0;
  int sp_off = -1;
  if (!e->fold || e->d.n_int < 1 || tree_lds_bytes(e, &sp_off) > 160 * 1024) return 0;
  bool wave = false;
  if (int rc = tree_wave_prepare(e, &wave)) return rc < 0 ? rc : MIOSQP_EHIP;
  return wave ? 1 : 2;
}

// dynamic LDS of k_tree_r_m (the reduced form) for this engine with a leaf list of `leaf_cap` places, and where the LDS
// copies of Abar start inside it -- the rows the test walks at sp_off, the rows of Abar^T at pv_off --, both or neither
// (the sp_off rule of res_sp_load: they are there when they fit behind everything else).  The rows of Abar^T are sized by
// a bound: their padded length is at most that of the rows by constraint plus one per variable.
size_t tree_r_lds_bytes(const miosqp_qp_engine *e, int leaf_cap, int *sp_off, int *pv_off) {
  const int n = e->n, M = e->M;
  size_t lds = tree_r_lds_doubles(n, M, leaf_cap);
  *sp_off = *pv_off = -1;
  const size_t sp = res_sp_doubles(e->sp_nnzA, e->sp_nnzP, n, M), pv = miosqp::tree_reduced::pv_doubles(e->sp_nnzA + (size_t)n, n);
  if (e->sp_nnzA > 0 && (lds + sp + pv) * sizeof(double) <= miosqp::tree_reduced::LDS_LIMIT &&
      !(getenv("MIOSQP_RES_SP") && atoi(getenv("MIOSQP_RES_SP")) == 0)) {
    *sp_off = (int)lds;
    *pv_off = (int)(lds + sp);
    lds += sp + pv;
  }
  return lds * sizeof(double);
}

// miosqp_qp_tree_form_large without the entry's own checks: 3 when the reduced form takes an engine that no other form
// takes, else 0 (or a negative error code of tree_form_of's lazy build)
int tree_form_large_of(miosqp_qp_engine *e, int leaf_cap) {
  if (leaf_cap < 2) return 0;
  const int form = tree_form_of(e);
  if (form != 0) return form < 0 ? form : 0;  // an engine that fits an existing form keeps that form
  if (!e->have_int || !e->d.digest || !e->fold || !e->d.f_rows || e->d.n_int < 1) return 0;
  return tree_r_lds_doubles(e->n, e->M, leaf_cap) * sizeof(double) <= miosqp::tree_reduced::LDS_LIMIT ? 3 : 0;
}

// which rows of Abar the reduced iteration reads from L2 (no LDS copy): 1 the dense copies, 0 the packed panels.
// Measured (profiles/solve_models_large.txt); MIOSQP_TREE_R_DENSE overrides for that measurement.
int tree_r_dense(const miosqp_qp_engine *e) {
  if (!e->d.f_Ad || !e->d.f_Atd) return 0;
  if (const char *v = getenv("MIOSQP_TREE_R_DENSE")) return atoi(v) != 0;
  return 1;
}

// the arena of miosqp_qp_solve_trees_models and its pinned mirror: they belong to the engine that was first in the call
int models_reserve(miosqp_qp_engine *e, size_t total_doubles, size_t up_doubles) {
  if (total_doubles > e->mm_cap) {  // (a larger call takes a new arena; the old one stays with the pool until cleanup)
    size_t cap = std::max(total_doubles, 2 * e->mm_cap);
    if (cap > total_doubles) {  // (growing ahead only where the device has the room; the caller checked total_doubles itself)
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess || cap * sizeof(double) + 4096 > fr / 2) cap = total_doubles;
    }
    int rc = pool_reserve(e, cap * sizeof(double) + 4096);
    if (!rc) rc = dalloc(e, &e->mm_dev, cap);
    if (rc) return rc;
    e->mm_cap = cap;
  }
  if (up_doubles > e->mm_host_cap) {
    const size_t cap = std::max(up_doubles, 2 * e->mm_host_cap);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->mm_host) hipHostFree(e->mm_host);
    e->mm_host = nullptr;
    e->mm_host_cap = 0;
    HIPCHK(hipHostMalloc((void **)&e->mm_host, cap * sizeof(double), hipHostMallocDefault));
    e->mm_host_cap = cap;
  }
  return 0;
}

// the per-model settings of strong / reliability branching (miosqp_qp_solve_trees_models_sb), and where the counters go
struct ModelsSb {
  const int32_t *rule, *K, *max_iter, *reliability;
  const double *eps;
  miosqp_tree_sb_info *info;
};

int models_run(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
               const double *const *u, const double *const *x0, const double *const *y0, const double *upper0,
               const double *const *x_inc0, const int32_t *rule, const int32_t *max_iter_bb, double *const *x_out,
               miosqp_tree_info *info, miosqp_models_stats *stats, bool large = false, int32_t leaf_cap = 0,
               bool with_rf = false, const int32_t *rf_candidates = nullptr, const int32_t *rf_max_iter = nullptr,
               const int32_t *rf_every = nullptr, miosqp_tree_rf_info *rf_info = nullptr, const ModelsSb *sb = nullptr) {
  namespace mm = miosqp::models;
  // ---- refused before anything is queued ----
  if (large) {
    std::string err;
    if (int rc = mm::check_leaf_cap(leaf_cap, err)) {
      g_err = err;
      return rc;
    }
  }
  {
    std::vector<int> Mv;
    if (B >= 1 && engines)
      for (int b = 0; b < B; b++) Mv.push_back(engines[b] ? engines[b]->M : 0);
    std::string err;
    if (int rc = mm::check_args(B, (const void *const *)engines, Mv.data(), q, l, u, x0, y0, upper0, x_inc0, rule, max_iter_bb,
                                (const void *const *)x_out, info, stats, err)) {
      g_err = err;
      return rc;
    }
  }
  if (with_rf) {  // miosqp_qp_solve_trees_models_rf: the per-model settings of round and fix
    std::string err;
    if (int rc = mm::check_rf(B, rf_candidates, rf_max_iter, rf_every, rf_info, 0, "solve_trees_models_rf", err)) {
      g_err = err;
      return rc;
    }
  }
  if (sb) {  // miosqp_qp_solve_trees_models_sb: the per-model settings of strong / reliability branching
    std::string err;
    if (int rc = mm::check_sb(B, sb->rule, sb->K, sb->max_iter, sb->reliability, sb->eps, sb->info, 0, "solve_trees_models_sb", err)) {
      g_err = err;
      return rc;
    }
  }
  miosqp_qp_engine *e0 = engines[0];
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    if (e->device != e0->device) {
      g_err = "solve_trees_models: model " + std::to_string(b) + " lives on device " + std::to_string(e->device) + ", model 0 on device " +
              std::to_string(e0->device);
      return MIOSQP_EARG;
    }
    if (e->pool_pending) {
      g_err = "solve_trees_models: streaming chunks are still in flight (pool_collect first), model " + std::to_string(b);
      return MIOSQP_EARG;
    }
  }
  ENTER(e0);
  const double t0 = wall();
  std::vector<mm::Shape> sh((size_t)B);
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    int form = tree_form_of(e);  // (the lazy build of W / Kc and its guard: the engine's own state, on its own stream)
    if (form < 0) return form;
    if (form == 0 && large) form = tree_form_large_of(e, leaf_cap);
    if (form < 0) return form;
    if (form == 0) {
      g_err = "solve_trees_models: the one-launch trees do not take model " + std::to_string(b) +
              " (integer rows and root set? product-form factor, iterates and leaf list within 160 KB of LDS?)";
      return MIOSQP_EUNSUPPORTED;
    }
    // with the heuristic on: the workgroup form (the wave-sized models too), or the reduced form
    if (with_rf && rf_candidates[b] > 0) form = form == 3 ? 5 : 4;
    // with a branching rule: the same two forms with strong / reliability branching inside
    if (sb && sb->rule[b] > 0) form = form == 3 ? 7 : 6;
    sh[(size_t)b] = mm::Shape{e->n, e->M, e->d.n_int, form};
  }
  const mm::Plan P = mm::plan(sh, sizeof(TreeModel), (size_t)TREE_CAP, (size_t)leaf_cap, with_rf ? mm::RF_DOUBLES : 0,
                              sb ? mm::SB_DOUBLES : 0);
  if (P.n3 || P.n5 || P.n7) {  // the leaf stores of the reduced form are the large part of an arena: refused by name, not a failed allocation
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const size_t have = e0->mm_cap * sizeof(double), room = (fr > ((size_t)256 << 20) ? fr - ((size_t)256 << 20) : 0);
    std::string err;
    if (int rc = mm::check_arena(P, sh, (size_t)TREE_CAP, (size_t)leaf_cap, std::max(have, room) / sizeof(double), err)) {
      g_err = err;
      return rc;
    }
  }
  if (int rc = models_reserve(e0, P.total_doubles, P.up_doubles)) return rc;
  if (P.n2) HIPCHK(lds_limit_once((const void *)k_tree_m, 13));
  if (P.n3) HIPCHK(lds_limit_once((const void *)k_tree_r_m, 16));
  if (P.n4) HIPCHK(lds_limit_once((const void *)k_tree_rf_m, 20));
  if (P.n5) HIPCHK(lds_limit_once((const void *)k_tree_rf_r_m, 21));
  if (P.n6) HIPCHK(lds_limit_once((const void *)k_tree_sb_m, 23));
  if (P.n7) HIPCHK(lds_limit_once((const void *)k_tree_sb_r_m, 24));
  // every other engine's stream in front of the launches: an update or a lazy build queued there has finished
  for (int b = 1; b < B; b++) {
    if (int rc = stage_wait(engines[b], 0)) return rc;
    if (int rc = stage_wait(engines[b], 1)) return rc;
    if (engines[b]->stream != e0->stream) HIPCHK(hipStreamSynchronize(engines[b]->stream));
  }
  // ---- the staged part: table, roots and costs, incumbents (the table is rebuilt every call: Dev changes under
  //      update_lin_cost, a lazy build of W or a tripped guard) ----
  double *hs = e0->mm_host, *dv = e0->mm_dev;
  TreeModel *tab_h = reinterpret_cast<TreeModel *>(hs), *tab_d = reinterpret_cast<TreeModel *>(dv);
  size_t lds_max = 0, lds_max_r = 0, lds_max_rf = 0, lds_max_rf_r = 0, lds_max_sb = 0, lds_max_sb_r = 0;
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    const mm::Slot &s = P.slot[(size_t)b];
    const size_t n = (size_t)e->n, M = (size_t)e->M;
    double *r = hs + s.raw;
    memcpy(r, l[b], sizeof(double) * M);
    memcpy(r + M, u[b], sizeof(double) * M);
    memcpy(r + 2 * M, x0[b], sizeof(double) * n);
    memcpy(r + 2 * M + n, y0[b], sizeof(double) * M);
    memcpy(hs + s.qraw, q[b], sizeof(double) * n);
    const bool have = x_inc0[b] != nullptr && upper0[b] < 1.7e308;
    if (have) memcpy(hs + s.inc, x_inc0[b], sizeof(double) * n);
    else memset(hs + s.inc, 0, sizeof(double) * n);
    memset(hs + s.out, 0, sizeof(double) * mm::OUT_DOUBLES);
    if (with_rf) memset(hs + s.rf, 0, sizeof(double) * mm::RF_DOUBLES);
    if (sb) memset(hs + s.sb, 0, sizeof(double) * mm::SB_DOUBLES);
    TreeModel &t = tab_h[s.entry];
    t.d = e->d;
    t.d.q = dv + s.q;
    t.d.qraw = dv + s.qraw;
    t.d.raw_l = dv + s.raw;
    t.d.raw_u = dv + s.raw + M;
    t.d.raw_x = dv + s.raw + 2 * M;
    t.d.raw_y = dv + s.raw + 2 * M + n;
    t.d.root_l = t.d.raw_l;  // the rounded point is tested against the instance's own root rows
    t.d.root_u = t.d.raw_u;
    t.d.prof = nullptr;
    TreeArgs ta{};
    ta.rule = rule[b];
    ta.max_nodes = max_iter_bb[b];
    ta.max_iter = e->st.max_iter;
    ta.check_every = e->st.check_termination;
    tree_lane_groups(e->n, e->M, ta);
    ta.upper0 = have ? upper0[b] : 1.0 / 0.0;
    ta.lf_lo = dv + s.lf_lo;
    ta.lf_hi = dv + s.lf_hi;
    ta.lf_x = dv + s.lf_x;
    ta.lf_y = dv + s.lf_y;
    ta.inc_x = dv + s.inc;
    ta.out = reinterpret_cast<TreeOut *>(dv + s.out);
    ta.done = nullptr;
    ta.sp_off = -1;
    ta.batch = 0;
    ta.upper_b = nullptr;
    ta.leaf_cap = TREE_CAP;
    ta.pv_off = -1;
    ta.r_dense = 0;
    const int form = sh[(size_t)b].form;
    if (form == 4 || form == 5) {
      ta.rf_K = rf_candidates[b];
      ta.rf_max_iter = rf_max_iter[b];
      ta.rf_every = rf_every[b];
      ta.rf_out = reinterpret_cast<TreeRfOut *>(dv + s.rf);
    }
    if (form == 6 || form == 7) {
      ta.sb_rule = sb->rule[b];
      ta.sb_K = sb->K[b];
      ta.sb_max_iter = sb->max_iter[b];
      ta.sb_rel = sb->reliability[b];
      ta.sb_eps = sb->eps[b];
      ta.sb_work = dv + s.sb_work;
      ta.sb_pc = dv + s.sb_pc;
      ta.sb_out = reinterpret_cast<TreeSbOut *>(dv + s.sb);
    }
    if (mm::reduced_form(form)) {
      ta.leaf_cap = leaf_cap;
      ta.TG1 = miosqp::tree_reduced::TGR;  // rows of Abar in the prologue, the test and the epilogue: as the iteration walks them
      ta.r_dense = tree_r_dense(e);
      size_t &most = form == 5 ? lds_max_rf_r : form == 7 ? lds_max_sb_r : lds_max_r;
      most = std::max(most, tree_r_lds_bytes(e, leaf_cap, &ta.sp_off, &ta.pv_off));
    }
    if (form == 2 || form == 4 || form == 6) {  // (after the form is settled: W may have come or gone in tree_form_of)
      const size_t lds = tree_lds_bytes(e, &ta.sp_off);
      size_t &most = form == 4 ? lds_max_rf : form == 6 ? lds_max_sb : lds_max;
      most = std::max(most, lds);
    }
    t.ta = ta;
  }
  static_assert(sizeof(TreeOut) <= mm::OUT_DOUBLES * sizeof(double), "TreeOut fits its place in the arena");
  static_assert(sizeof(TreeRfOut) <= mm::RF_DOUBLES * sizeof(double), "TreeRfOut fits its place in the arena");
  static_assert(sizeof(TreeSbOut) <= mm::SB_DOUBLES * sizeof(double), "TreeSbOut fits its place in the arena");
  // ---- one upload, the costs scaled, one tree launch per form that has a model, one download, one synchronisation ----
  HIPCHK(hipEventRecord(e0->ev0, e0->stream));
  HIPCHK(hipMemcpyAsync(dv, hs, sizeof(double) * P.up_doubles, hipMemcpyHostToDevice, e0->stream));
  hipLaunchKernelGGL(k_scale_q_models, dim3((unsigned)B), dim3(64), 0, e0->stream, tab_d);
  if (P.n1) hipLaunchKernelGGL(k_tree_w_m, dim3((unsigned)P.n1), dim3(TW), 0, e0->stream, tab_d);
  if (P.n2) hipLaunchKernelGGL(k_tree_m, dim3((unsigned)P.n2), dim3(RES_THREADS), lds_max, e0->stream, tab_d + P.n1);
  if (P.n3) hipLaunchKernelGGL(k_tree_r_m, dim3((unsigned)P.n3), dim3(RES_THREADS), lds_max_r, e0->stream, tab_d + P.n1 + P.n2);
  if (P.n4)
    hipLaunchKernelGGL(k_tree_rf_m, dim3((unsigned)P.n4), dim3(RES_THREADS), lds_max_rf, e0->stream, tab_d + P.n1 + P.n2 + P.n3);
  if (P.n5)
    hipLaunchKernelGGL(k_tree_rf_r_m, dim3((unsigned)P.n5), dim3(RES_THREADS), lds_max_rf_r, e0->stream,
                       tab_d + P.n1 + P.n2 + P.n3 + P.n4);
  if (P.n6)
    hipLaunchKernelGGL(k_tree_sb_m, dim3((unsigned)P.n6), dim3(RES_THREADS), lds_max_sb, e0->stream,
                       tab_d + P.n1 + P.n2 + P.n3 + P.n4 + P.n5);
  if (P.n7)
    hipLaunchKernelGGL(k_tree_sb_r_m, dim3((unsigned)P.n7), dim3(RES_THREADS), lds_max_sb_r, e0->stream,
                       tab_d + P.n1 + P.n2 + P.n3 + P.n4 + P.n5 + P.n6);
  HIPCHK(hipMemcpyAsync(hs + P.down_off, dv + P.down_off, sizeof(double) * P.down_doubles, hipMemcpyDeviceToHost, e0->stream));
  HIPCHK(hipEventRecord(e0->ev1, e0->stream));
  HIPCHK(hipStreamSynchronize(e0->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0->ev0, e0->ev1));
  const double wall_s = wall() - t0;
  for (int b = 0; b < B; b++) {
    miosqp_qp_engine *e = engines[b];
    const mm::Slot &s = P.slot[(size_t)b];
    TreeOut o;
    memcpy(&o, hs + s.out, sizeof o);
    info[b].nodes = o.nodes;
    info[b].osqp_iter = o.osqp_iter;
    info[b].leaves_left = o.leaves_left;
    info[b].overflow = o.overflow;
    info[b].max_leaves = o.max_leaves;
    info[b].found = o.found;
    info[b].upper_glob = o.upper;
    info[b].lower_glob = o.lower_glob;
    info[b].device_time = 1e-3 * ms / B;  // the call's device time, shared equally
    info[b].run_time = wall_s / B;
    const bool have = x_inc0[b] != nullptr && upper0[b] < 1.7e308;
    if (o.found) memcpy(x_out[b], hs + s.inc, sizeof(double) * (size_t)e->n);
    else if (have) memcpy(x_out[b], x_inc0[b], sizeof(double) * (size_t)e->n);
    e->loop_ms += ms / B;
    e->loop_iters += o.osqp_iter;
    if (with_rf) {
      TreeRfOut r;
      memcpy(&r, hs + s.rf, sizeof r);
      rf_info[b] = miosqp_tree_rf_info{r.calls, r.candidates, r.feasible, r.improved, r.osqp_iter, sh[(size_t)b].form, 0, 0};
    }
    if (sb) {
      TreeSbOut r;
      memcpy(&r, hs + s.sb, sizeof r);
      sb->info[b] = miosqp_tree_sb_info{r.calls, r.children, r.osqp_iter, sh[(size_t)b].form, 0, 0, 0, 0};
    }
  }
  stats->launches = (P.n1 ? 1 : 0) + (P.n2 ? 1 : 0) + (P.n3 ? 1 : 0) + (P.n4 ? 1 : 0) + (P.n5 ? 1 : 0) + (P.n6 ? 1 : 0) + (P.n7 ? 1 : 0);
  stats->models_wave = P.n1;
  stats->models_group = P.n2;
  stats->pad = P.n3;  // (models run by the reduced form: 0 unless the call came through miosqp_qp_solve_trees_models_large)
  stats->lds_bytes = (int64_t)std::max(std::max(std::max(lds_max, lds_max_r), std::max(lds_max_rf, lds_max_rf_r)),
                                       std::max(lds_max_sb, lds_max_sb_r));
  stats->device_time = 1e-3 * ms;
  stats->run_time = wall_s;
  return 0;
}

}  // namespace
