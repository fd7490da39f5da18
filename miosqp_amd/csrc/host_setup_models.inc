// part of engine.hip (included there, not compiled alone): the set-up of many small models in one launch (C ABI
// miosqp_qp_setup_models; kernel k_setup_models in kernels_setup_models.inc; argument checks, eligibility and the layout of
// the arena in setup_plan.hpp).  The engines of one call share a GROUP: one stream, one device arena, one pinned slab.
namespace {

// What the engines of one miosqp_qp_setup_models call share.  Reference-counted: every engine holds one reference and
// drops it in miosqp_qp_cleanup; the last one frees the three objects.  Nothing of a group goes to the per-process caches
// of rt_release / the parked chunks.
struct SetupGroup {
  int device = -1;
  hipStream_t stream = nullptr;
  char *arena = nullptr, *slab = nullptr;
  size_t arena_bytes = 0, slab_bytes = 0;
  int refs = 0;
  int64_t id = 0;
};
std::mutex g_group_mutex;
int g_groups_live = 0;
int64_t g_group_next = 1;
// The three objects of ONE freed group wait here for the next call on the same device (creating them is ~2.8 ms, more
// than the whole set-up of eight small models; a loop that sets up a few models at a time would pay it every time).  A
// cache of its own, one entry, nothing above 32 MB; MIOSQP_NO_CACHE keeps it empty like the other caches.
SetupGroup g_group_spare;
bool g_group_spare_set = false;

void group_release_objects(SetupGroup &g) {
  if (g.device >= 0) (void)hipSetDevice(g.device);
  if (g.stream) {
    (void)hipStreamSynchronize(g.stream);
    (void)hipStreamDestroy(g.stream);
  }
  if (g.arena) (void)hipFree(g.arena);
  if (g.slab) (void)hipHostFree(g.slab);
  g = SetupGroup();
}

void group_unref(SetupGroup *g) {
  if (!g) return;
  {
    std::lock_guard<std::mutex> lk(g_group_mutex);
    if (--g->refs > 0) return;
    g_groups_live--;
  }
  SetupGroup old;
  const bool whole = g->stream && g->arena && g->slab;
  if (whole && g->arena_bytes <= CHUNK_PARK_MAX && g->slab_bytes <= CHUNK_PARK_MAX && !getenv("MIOSQP_NO_CACHE") &&
      hipStreamSynchronize(g->stream) == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_group_mutex);
    if (g_group_spare_set) old = g_group_spare;  // (the newer one stays: it fitted the last call)
    g_group_spare = *g;
    g_group_spare.refs = 0;
    g_group_spare_set = true;
  } else {
    old = *g;
  }
  group_release_objects(old);
  delete g;
}

// the parked objects, if they are on this device and large enough
bool group_take_spare(SetupGroup *g, int device, size_t arena_bytes, size_t slab_bytes) {
  if (getenv("MIOSQP_NO_CACHE")) return false;
  std::lock_guard<std::mutex> lk(g_group_mutex);
  if (!g_group_spare_set || g_group_spare.device != device || g_group_spare.arena_bytes < arena_bytes ||
      g_group_spare.slab_bytes < slab_bytes)
    return false;
  g->stream = g_group_spare.stream;
  g->arena = g_group_spare.arena;
  g->slab = g_group_spare.slab;
  g->arena_bytes = g_group_spare.arena_bytes;
  g->slab_bytes = g_group_spare.slab_bytes;
  g_group_spare = SetupGroup();
  g_group_spare_set = false;
  return true;
}

// miosqp_qp_cleanup of a group's engine: its own events (and the lazily built tree block) go, the stream and the pinned
// buffers belong to the group
void group_engine_release(miosqp_qp_engine *e) {
  SetupGroup *g = e->group;
  e->rt.stream = nullptr;
  e->rt.h_in = e->rt.h_out = nullptr;
  e->rt.h_ctrl = e->rt.h_ctrl2 = nullptr;
  rt_destroy(e->rt);
  e->group = nullptr;
  group_unref(g);
}

// the form-changing switches of the environment under which miosqp_qp_setup would NOT build resident + fold + W
bool setup_models_env_ok() {
  if (const char *ev = getenv("MIOSQP_COOP"))
    if (atoi(ev) == 1) return false;
  if (const char *ev = getenv("MIOSQP_RES_W"))
    if (atoi(ev) == 0) return false;
  return true;
}

miosqp::setup_models::Args setup_args_of(const miosqp_setup_model &m) {
  miosqp::setup_models::Args a;
  a.n = m.n; a.M = m.M;
  a.Pp = m.Pp; a.Pi = m.Pi; a.Px = m.Px; a.Ap = m.Ap; a.Ai = m.Ai; a.Ax = m.Ax; a.q = m.q;
  a.l = m.l; a.u = m.u;
  a.settings = m.settings;
  if (m.settings) {
    const miosqp_qp_settings &s = *m.settings;
    a.rho = s.rho; a.sigma = s.sigma; a.alpha = s.alpha; a.max_iter = s.max_iter; a.rho_auto = s.rho_auto;
    a.coop = s.coop; a.resident = s.resident; a.fold = s.fold; a.setup_on_device = s.setup_on_device; a.pers = s.pers;
  }
  a.n_int = m.n_int; a.m_orig = m.m_orig; a.i_idx = m.i_idx;
  a.l_root = m.l_root; a.u_root = m.u_root;
  return a;
}

template <typename T>
T *arena_at(char *base, const miosqp::setup_models::Slot &s, int part) {
  return reinterpret_cast<T *>(base + s.part[part].off);
}
template <typename T>
void stage_vec(char *slab, const miosqp::setup_models::Slot &s, int part, const T *src, size_t count) {
  if (count) memcpy(slab + s.part[part].off, src, count * sizeof(T));
}

// the switches of the environment under which miosqp_qp_setup would NOT build the engine of the large launch (product
// form, captured chunks; neither cooperative grid nor persistent kernel)
bool setup_models_large_env_ok() {
  if (const char *ev = getenv("MIOSQP_COOP"))
    if (atoi(ev) == 1) return false;
  if (const char *ev = getenv("MIOSQP_PERS"))
    if (atoi(ev) > 0) return false;
  return true;
}

// rho_auto_in_launch (miosqp_qp_setup_models_auto): models with settings->rho_auto = 1 are taken, and when there is one
// the launch is k_setup_models_auto.  large (miosqp_qp_setup_models_large): a model that k_setup_models does not take for
// its size is built by k_setup_models_large, a second launch of the same call, as the engine miosqp_qp_setup builds with
// coop = 0, resident = 0, fold = 1, pers = 0; the table holds the small models first.  large_rho_auto
// (miosqp_qp_setup_models_large_auto): large models with rho_auto = 1 are taken, and when there is one the large launch
// is k_setup_models_large_auto.  prepare (miosqp_qp_setup_models_prepared): the raw problem goes up and k_prepare_models,
// one more launch ahead of the others, builds what scale_problem and pack_factor_rows build on the host otherwise; the
// host's mirrors (e->sc, e->fa) are filled from the download behind the launches.
int setup_models_run(int32_t B, const miosqp_setup_model *ms, miosqp_qp_engine **out, miosqp_setup_models_stats *stats,
                     bool rho_auto_in_launch, bool large = false, bool large_rho_auto = false, bool prepare = false) {
  namespace sm = miosqp::setup_models;
  namespace pm = miosqp::prepare_models;
  static_assert(sizeof(Ctrl) <= sm::CTRL_BYTES, "Ctrl fits its place in the arena and the slab");
  // ---- refused before anything is queued ----
  {
    std::vector<sm::Args> av;
    if (B >= 1 && ms)
      for (int b = 0; b < B; b++) av.push_back(setup_args_of(ms[b]));
    std::string err;
    if (int rc = sm::check_args(B, ms ? av.data() : nullptr, out, stats, err, rho_auto_in_launch, large, large_rho_auto)) {
      g_err = err;
      return rc;
    }
  }
  for (int b = 0; b < B; b++)
    if (!sm::csc_strictly_ascending(ms[b].n, ms[b].Pp, ms[b].Pi) || !sm::csc_strictly_ascending(ms[b].n, ms[b].Ap, ms[b].Ai)) {
      g_err = "setup_models: the row indices of P and A must ascend strictly within a column, no entry twice (model " + std::to_string(b) + ")";
      return MIOSQP_EUNSUPPORTED;
    }
  std::vector<int> form((size_t)B, sm::FORM_SMALL);
  int n_large = 0;
  for (int b = 0; b < B; b++)
    if (large && !sm::eligible_shape(ms[b].n, ms[b].M)) {
      form[(size_t)b] = sm::FORM_LARGE;
      n_large++;
    }
  if (n_large < B && !setup_models_env_ok()) {
    g_err = "setup_models: MIOSQP_COOP=1 or MIOSQP_RES_W=0 asks for another engine form than the launch builds";
    return MIOSQP_EUNSUPPORTED;
  }
  if (n_large > 0 && !setup_models_large_env_ok()) {
    g_err = "setup_models: MIOSQP_COOP=1 or MIOSQP_PERS asks for another engine form than the large launch builds";
    return MIOSQP_EUNSUPPORTED;
  }
  for (int b = 1; b < B; b++)
    if (ms[b].settings->device != ms[0].settings->device) {
      g_err = "setup_models: model " + std::to_string(b) + " asks for device " + std::to_string(ms[b].settings->device) +
              ", model 0 for device " + std::to_string(ms[0].settings->device);
      return MIOSQP_EARG;
    }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device visible: the relaxation engine has no CPU fallback";
    return MIOSQP_ENODEV;
  }
  if (ms[0].settings->device >= 0) HIPCHK(hipSetDevice(ms[0].settings->device));
  int device = 0;
  HIPCHK(hipGetDevice(&device));
  const bool t_on = getenv("MIOSQP_SETUP_TIMING") != nullptr;
  const double t_begin = wall();
  double t_last = t_begin;
  auto tick = [&](const char *what) {
    if (!t_on) return;
    const double now = wall();
    fprintf(stderr, "[miosqp setup_models] %-36s %8.3f ms  (%d models)\n", what, 1e3 * (now - t_last), (int)B);
    t_last = now;
  };
  for (int b = 0; b < B; b++) out[b] = nullptr;
  bool any_auto = false, any_auto_large = false;  // per launch: a small model, a large model that asks for rho_auto
  for (int b = 0; b < B; b++)
    if (ms[b].settings->rho_auto != 0) (form[(size_t)b] == sm::FORM_LARGE ? any_auto_large : any_auto) = true;
  const int64_t made0[3] = {g_made_device_mallocs, g_made_host_mallocs, g_made_streams};
  std::vector<miosqp_qp_engine *> eng((size_t)B, nullptr);
  SetupGroup *grp = nullptr;
  // everything of the call goes: engines that joined the group through their clean-up, the others as plain objects, then
  // the call's own reference
  auto fail = [&](int rc) {
    const std::string keep = g_err;
    for (miosqp_qp_engine *e : eng) {
      if (!e) continue;
      if (e->group) miosqp_qp_cleanup(e);
      else delete e;
    }
    group_unref(grp);
    g_err = keep;
    return rc;
  };
#define SMCHK(call)                                   \
  do {                                                \
    hipError_t e__ = (call);                          \
    if (e__ != hipSuccess) {                          \
      set_err(#call, e__, __FILE__, __LINE__);        \
      return fail(MIOSQP_EHIP);                       \
    }                                                 \
  } while (0)
  // ---- host: equilibration (scale_problem, as the per-model set-up) and the packed rows ----
  std::vector<sm::Shape> sh((size_t)B);
  for (int b = 0; b < B; b++) {
    const miosqp_setup_model &m = ms[b];
    miosqp_qp_engine *e = new miosqp_qp_engine();
    eng[(size_t)b] = e;
    e->device = device;
    e->n = m.n;
    e->M = m.M;
    e->st = *m.settings;
    if (e->st.check_termination <= 0 || e->st.check_termination > e->st.max_iter) e->st.check_termination = e->st.max_iter;
    if (form[(size_t)b] == sm::FORM_LARGE) e->st.coop = 0;  // (the engine that comes out is not the cooperative grid's)
    e->setup_on_device = false;
    if (!prepare) miosqp::scale_problem(m.n, m.M, m.Pp, m.Pi, m.Px, m.Ap, m.Ai, m.Ax, m.q, m.settings->scaling, e->sc);
    miosqp::Factor &f = e->fa;  // the rows; Linv / LinvT stay empty on the host, as where the device keeps them
    f.n = m.n; f.M = m.M; f.rho = m.settings->rho; f.sigma = m.settings->sigma;
    f.ld = (m.n + 15) & ~15;
    if (!prepare) {
      miosqp::pack_factor_rows(e->sc, m.Pp, m.Pi, m.Px, f.rho, f);
    } else {
      // the integer half of both: the patterns of the scaled problem's mirror (P's upper triangle, A) and the pointer arrays
      // of the four packed structures; the values and the column indices of the rows come back with the download
      miosqp::Scaled &sc = e->sc;
      sc.n = m.n; sc.M = m.M;
      sc.Pp.assign((size_t)m.n + 1, 0);
      sc.Pi.clear();
      int64_t ndiag = 0;
      for (int j = 0; j < m.n; j++) {
        sc.Pp[(size_t)j] = (int)sc.Pi.size();
        for (int p = m.Pp[j]; p < m.Pp[j + 1]; p++)
          if (m.Pi[p] <= j) {
            sc.Pi.push_back(m.Pi[p]);
            ndiag += m.Pi[p] == j;
          }
      }
      sc.Pp[(size_t)m.n] = (int)sc.Pi.size();
      sc.Ap.assign(m.Ap, m.Ap + m.n + 1);
      sc.Ai.assign(m.Ai, m.Ai + m.Ap[m.n]);
      f.panel_by_var.rows = m.n; f.panel_by_var.cols = m.M;
      f.panel_by_con.rows = m.M; f.panel_by_con.cols = m.n;
      f.Pbar.rows = f.Pbar.cols = f.Praw.rows = f.Praw.cols = m.n;
      f.panel_by_var.ptr.resize((size_t)m.n + 1);
      f.panel_by_con.ptr.resize((size_t)m.M + 1);
      f.Pbar.ptr.resize((size_t)m.n + 1);
      int64_t up = 0;
      pm::prepare_pointers(m.n, m.M, m.Pp, m.Pi, m.Ap, m.Ai, f.panel_by_var.ptr.data(), f.panel_by_con.ptr.data(), f.Pbar.ptr.data(), &up);
      f.Praw.ptr = f.Pbar.ptr;
      f.panel_by_var.nnz = f.panel_by_con.nnz = f.nnz_panel = m.Ap[m.n];
      f.Pbar.nnz = f.Praw.nnz = 2 * up - ndiag;
      const size_t nv = (size_t)f.panel_by_var.ptr[(size_t)m.n], nc = (size_t)f.panel_by_con.ptr[(size_t)m.M], np = (size_t)f.Pbar.ptr[(size_t)m.n];
      f.panel_by_var.idx.resize(nv); f.panel_by_var.val.resize(nv); f.At_val.resize(nv);
      f.panel_by_con.idx.resize(nc); f.panel_by_con.val.resize(nc); f.A_val.resize(nc);
      f.Pbar.idx.resize(np); f.Pbar.val.resize(np); f.Praw.idx.resize(np); f.Praw.val.resize(np);
    }
    f.nnz_tail = (int64_t)m.n * (m.n - 1) / 2;
    e->nnzA = m.Ap[m.n];
    e->A_raw.assign(m.Ax, m.Ax + m.Ap[m.n]);
    e->nnzPtriu = (int64_t)e->sc.Pi.size();
    sh[(size_t)b] = sm::Shape{m.n, m.M, f.panel_by_var.idx.size(), f.panel_by_con.idx.size(), f.Pbar.idx.size(), f.Praw.idx.size(),
                              m.settings->rho_auto ? 1 : 0, form[(size_t)b]};
    if (prepare) {
      sh[(size_t)b].prepare = 1;
      sh[(size_t)b].nnzP = (size_t)m.Pp[m.n];
      sh[(size_t)b].nnzA = (size_t)m.Ap[m.n];
    }
  }
  const sm::Plan P = sm::plan(sh, sizeof(SetupModel), sizeof(pm::IO));
  tick(prepare ? "host: patterns + row pointers" : "host: equilibration + packed rows");
  // ---- the group: one stream, one arena (zero-filled on that stream, ahead of the upload), one pinned slab ----
  grp = new SetupGroup();
  grp->device = device;
  grp->refs = 1;  // the call's own, dropped at its end
  {
    std::lock_guard<std::mutex> lk(g_group_mutex);
    grp->id = g_group_next++;
    g_groups_live++;
  }
  if (!group_take_spare(grp, device, P.total_bytes, P.pin_bytes)) {
    SMCHK(hipStreamCreateWithFlags(&grp->stream, hipStreamNonBlocking));
    g_made_streams++;
    SMCHK(hipMalloc((void **)&grp->arena, P.total_bytes));
    g_made_device_mallocs++;
    grp->arena_bytes = P.total_bytes;
    SMCHK(hipHostMalloc((void **)&grp->slab, P.pin_bytes, hipHostMallocDefault));
    g_made_host_mallocs++;
    grp->slab_bytes = P.pin_bytes;
  }
  SMCHK(hipMemsetAsync(grp->arena, 0, P.total_bytes, grp->stream));
  tick("group: stream, arena, pinned slab");
  // ---- the upload's image in the slab, the table, every engine's Dev ----
  char *const dv = grp->arena, *const hs = grp->slab;
  memset(hs, 0, P.up_bytes);
  SetupModel *tab_h = reinterpret_cast<SetupModel *>(hs);
  double tol = COOP_GUARD_TOL;
  if (const char *ev = getenv("MIOSQP_GUARD_TOL")) tol = atof(ev);
  for (int b = 0; b < B; b++) {
    const miosqp_setup_model &m = ms[b];
    miosqp_qp_engine *e = eng[(size_t)b];
    const sm::Slot &s = P.slot[(size_t)b];
    const miosqp::Factor &f = e->fa;
    const miosqp_qp_settings *st = m.settings;
    const int n = m.n, M = m.M;
    stage_vec(hs, s, sm::PV_PTR, f.panel_by_var.ptr.data(), f.panel_by_var.ptr.size());
    stage_vec(hs, s, sm::PC_PTR, f.panel_by_con.ptr.data(), f.panel_by_con.ptr.size());
    stage_vec(hs, s, sm::PB_PTR, f.Pbar.ptr.data(), f.Pbar.ptr.size());
    stage_vec(hs, s, sm::PR_PTR, f.Praw.ptr.data(), f.Praw.ptr.size());
    if (!prepare) {
      stage_vec(hs, s, sm::PV_IDX, f.panel_by_var.idx.data(), f.panel_by_var.idx.size());
      stage_vec(hs, s, sm::PV_L, f.panel_by_var.val.data(), f.panel_by_var.val.size());
      stage_vec(hs, s, sm::PV_AT, f.At_val.data(), f.At_val.size());
      stage_vec(hs, s, sm::PC_IDX, f.panel_by_con.idx.data(), f.panel_by_con.idx.size());
      stage_vec(hs, s, sm::PC_L, f.panel_by_con.val.data(), f.panel_by_con.val.size());
      stage_vec(hs, s, sm::PC_A, f.A_val.data(), f.A_val.size());
      stage_vec(hs, s, sm::PB_IDX, f.Pbar.idx.data(), f.Pbar.idx.size());
      stage_vec(hs, s, sm::PB_VAL, f.Pbar.val.data(), f.Pbar.val.size());
      stage_vec(hs, s, sm::PR_IDX, f.Praw.idx.data(), f.Praw.idx.size());
      stage_vec(hs, s, sm::PR_VAL, f.Praw.val.data(), f.Praw.val.size());
      stage_vec(hs, s, sm::D_, e->sc.D.data(), (size_t)n);
      stage_vec(hs, s, sm::DINV, e->sc.Dinv.data(), (size_t)n);
      stage_vec(hs, s, sm::E_, e->sc.E.data(), (size_t)M);
      stage_vec(hs, s, sm::EINV, e->sc.Einv.data(), (size_t)M);
      stage_vec(hs, s, sm::Q, e->sc.q.data(), (size_t)n);
    } else {  // the raw problem
      const size_t nnzP = (size_t)m.Pp[n], nnzA = (size_t)m.Ap[n];
      memcpy(hs + s.raw[sm::RAW_PP].off, m.Pp, sizeof(int32_t) * ((size_t)n + 1));
      if (nnzP) memcpy(hs + s.raw[sm::RAW_PI].off, m.Pi, sizeof(int32_t) * nnzP);
      if (nnzP) memcpy(hs + s.raw[sm::RAW_PX].off, m.Px, sizeof(double) * nnzP);
      memcpy(hs + s.raw[sm::RAW_AP].off, m.Ap, sizeof(int32_t) * ((size_t)n + 1));
      if (nnzA) memcpy(hs + s.raw[sm::RAW_AI].off, m.Ai, sizeof(int32_t) * nnzA);
      if (nnzA) memcpy(hs + s.raw[sm::RAW_AX].off, m.Ax, sizeof(double) * nnzA);
    }
    stage_vec(hs, s, sm::QRAW, m.q, (size_t)n);
    stage_vec(hs, s, sm::RAW, m.l, (size_t)M);
    memcpy(hs + s.part[sm::RAW].off + sizeof(double) * M, m.u, sizeof(double) * M);
    Dev &d = e->d;
    d.n = n; d.M = M; d.ld = f.ld; d.n_int = 0; d.m_orig = M; d.wh_m = M;
    d.rho = st->rho; d.rho_inv = 1.0 / st->rho; d.sigma = st->sigma; d.alpha = st->alpha; d.eps_abs = st->eps_abs; d.eps_rel = st->eps_rel;
    d.eps_pinf = st->eps_prim_inf; d.eps_dinf = st->eps_dual_inf; d.c = e->sc.c; d.cinv = e->sc.cinv;
    d.pv_ptr = arena_at<int>(dv, s, sm::PV_PTR); d.pv_idx = arena_at<int>(dv, s, sm::PV_IDX);
    d.pv_L = arena_at<double>(dv, s, sm::PV_L); d.pv_At = arena_at<double>(dv, s, sm::PV_AT);
    d.pc_ptr = arena_at<int>(dv, s, sm::PC_PTR); d.pc_idx = arena_at<int>(dv, s, sm::PC_IDX);
    d.pc_L = arena_at<double>(dv, s, sm::PC_L); d.pc_A = arena_at<double>(dv, s, sm::PC_A);
    d.pb_ptr = arena_at<int>(dv, s, sm::PB_PTR); d.pb_idx = arena_at<int>(dv, s, sm::PB_IDX); d.pb_val = arena_at<double>(dv, s, sm::PB_VAL);
    d.pr_ptr = arena_at<int>(dv, s, sm::PR_PTR); d.pr_idx = arena_at<int>(dv, s, sm::PR_IDX); d.pr_val = arena_at<double>(dv, s, sm::PR_VAL);
    d.D = arena_at<double>(dv, s, sm::D_); d.Dinv = arena_at<double>(dv, s, sm::DINV);
    d.E = arena_at<double>(dv, s, sm::E_); d.Einv = arena_at<double>(dv, s, sm::EINV);
    d.q = arena_at<double>(dv, s, sm::Q); d.qraw = arena_at<double>(dv, s, sm::QRAW);
    d.raw_l = arena_at<double>(dv, s, sm::RAW);
    d.raw_u = d.raw_l + M; d.raw_x = d.raw_u + M; d.raw_y = d.raw_x + n;
    d.Linv = arena_at<double>(dv, s, sm::LINV); d.LinvT = arena_at<double>(dv, s, sm::LINVT); d.d2inv = arena_at<double>(dv, s, sm::D2INV);
    d.f_rows = arena_at<double>(dv, s, sm::F_ROWS); d.f_GmT = arena_at<double>(dv, s, sm::F_GMT);
    d.f_Ad = arena_at<double>(dv, s, sm::F_AD); d.f_Atd = arena_at<double>(dv, s, sm::F_ATD); d.f_Pd = arena_at<double>(dv, s, sm::F_PD);
    d.ldf = (M + n + 15) & ~15; d.ldn = (n + 15) & ~15; d.ldm = (M + 15) & ~15;
    d.f_rows2 = d.f_rows;
    d.ldf2 = d.ldf;
    d.ldw = (n + M + 7) & ~7;
    const bool lg = form[(size_t)b] == sm::FORM_LARGE;  // (no W, no Kc: their parts have no bytes)
    d.W = lg ? nullptr : arena_at<double>(dv, s, sm::W_);
    d.Kc = lg ? nullptr : arena_at<double>(dv, s, sm::KC);
    d.l = arena_at<double>(dv, s, sm::L_); d.u = arena_at<double>(dv, s, sm::U_); d.x = arena_at<double>(dv, s, sm::X_);
    d.z = arena_at<double>(dv, s, sm::Z_); d.y = arena_at<double>(dv, s, sm::Y_); d.wh = arena_at<double>(dv, s, sm::WH);
    d.rx = d.wh + M;
    d.cv = arena_at<double>(dv, s, sm::CV); d.ut = arena_at<double>(dv, s, sm::UT); d.xt = arena_at<double>(dv, s, sm::XT);
    d.dx = arena_at<double>(dv, s, sm::DX); d.dy = arena_at<double>(dv, s, sm::DY);
    d.sm = arena_at<double>(dv, s, sm::SM); d.sn = arena_at<double>(dv, s, sm::SN);
    d.xi = arena_at<double>(dv, s, sm::XI); d.xis = arena_at<double>(dv, s, sm::XIS);
    d.root_l = arena_at<double>(dv, s, sm::ROOT_L); d.root_u = arena_at<double>(dv, s, sm::ROOT_U);
    d.digest = 0;
    d.ctrl = arena_at<Ctrl>(dv, s, sm::CTRL);
    d.out_x = arena_at<double>(dv, s, sm::OUT);
    d.out_y = d.out_x + n;
    d.i_idx = arena_at<int>(dv, s, sm::I_IDX);
    SetupModel &t = tab_h[s.entry];
    sm::IO &io = t.io;
    io.n = n; io.M = M; io.ld = d.ld; io.ldf = d.ldf; io.ldn = d.ldn; io.ldm = d.ldm; io.ldw = d.ldw;
    io.rho = d.rho; io.sigma = d.sigma;
    io.pc_ptr = d.pc_ptr; io.pc_idx = d.pc_idx; io.pc_A = d.pc_A;
    io.pb_ptr = d.pb_ptr; io.pb_idx = d.pb_idx; io.pb_val = d.pb_val;
    io.E = d.E; io.raw_l = d.raw_l; io.raw_u = d.raw_u; io.l = d.l; io.u = d.u;
    io.d2inv = arena_at<double>(dv, s, sm::D2INV); io.Linv = arena_at<double>(dv, s, sm::LINV); io.LinvT = arena_at<double>(dv, s, sm::LINVT);
    io.f_rows = arena_at<double>(dv, s, sm::F_ROWS); io.f_GmT = arena_at<double>(dv, s, sm::F_GMT); io.f_Ad = arena_at<double>(dv, s, sm::F_AD);
    io.f_Atd = arena_at<double>(dv, s, sm::F_ATD); io.f_Pd = arena_at<double>(dv, s, sm::F_PD);
    io.W = const_cast<double *>(d.W); io.Kc = const_cast<double *>(d.Kc);
    io.rec = reinterpret_cast<sm::Record *>(dv + s.rec);
    t.ctrl = d.ctrl;
    sm::Auto &au = t.au;
    au.on = st->rho_auto ? 1 : 0;
    au.nv = (int)f.panel_by_var.val.size(); au.nc = (int)f.panel_by_con.val.size();
    au.alpha = d.alpha;
    au.q = d.q; au.pv_At = d.pv_At;
    au.pv_L = arena_at<double>(dv, s, sm::PV_L); au.pc_L = arena_at<double>(dv, s, sm::PC_L);
    if (prepare) {  // entry b of k_prepare_models' table
      pm::IO &pi = reinterpret_cast<pm::IO *>(hs + P.ptab_off)[b];
      pi.n = n; pi.M = M; pi.passes = st->scaling; pi.rho = st->rho;
      pi.Pp = reinterpret_cast<const int *>(dv + s.raw[sm::RAW_PP].off); pi.Pi = reinterpret_cast<const int *>(dv + s.raw[sm::RAW_PI].off);
      pi.Px = reinterpret_cast<const double *>(dv + s.raw[sm::RAW_PX].off);
      pi.Ap = reinterpret_cast<const int *>(dv + s.raw[sm::RAW_AP].off); pi.Ai = reinterpret_cast<const int *>(dv + s.raw[sm::RAW_AI].off);
      pi.Ax = reinterpret_cast<const double *>(dv + s.raw[sm::RAW_AX].off);
      pi.qraw = d.qraw;
      pi.pv_ptr = d.pv_ptr; pi.pc_ptr = d.pc_ptr; pi.pb_ptr = d.pb_ptr; pi.pr_ptr = d.pr_ptr;
      pi.pv_idx = arena_at<int>(dv, s, sm::PV_IDX); pi.pc_idx = arena_at<int>(dv, s, sm::PC_IDX);
      pi.pb_idx = arena_at<int>(dv, s, sm::PB_IDX); pi.pr_idx = arena_at<int>(dv, s, sm::PR_IDX);
      pi.pv_L = arena_at<double>(dv, s, sm::PV_L); pi.pv_At = arena_at<double>(dv, s, sm::PV_AT);
      pi.pc_L = arena_at<double>(dv, s, sm::PC_L); pi.pc_A = arena_at<double>(dv, s, sm::PC_A);
      pi.pb_val = arena_at<double>(dv, s, sm::PB_VAL); pi.pr_val = arena_at<double>(dv, s, sm::PR_VAL);
      pi.D = arena_at<double>(dv, s, sm::D_); pi.Dinv = arena_at<double>(dv, s, sm::DINV);
      pi.E = arena_at<double>(dv, s, sm::E_); pi.Einv = arena_at<double>(dv, s, sm::EINV);
      pi.q = arena_at<double>(dv, s, sm::Q);
      pi.sc = reinterpret_cast<pm::Scalars *>(dv + s.scal.off);
    }
    // the engine joins the group: its pool is the rest of its slice, its stream the group's, its events its own
    e->pool_base = dv + s.part[sm::RESERVE].off;
    e->pool_cap = s.part[sm::RESERVE].bytes;
    e->pool_used = 0;
    RtBundle &r = e->rt;
    r = RtBundle();
    r.device = device;
    {
      std::lock_guard<std::mutex> lk(g_group_mutex);
      grp->refs++;
    }
    e->group = grp;
    r.stream = grp->stream;
    e->stream = r.stream;
    SMCHK(hipEventCreate(&r.ev0));
    SMCHK(hipEventCreate(&r.ev1));
    SMCHK(hipEventCreate(&r.evc0));
    SMCHK(hipEventCreate(&r.evc1));
    SMCHK(hipEventCreateWithFlags(&r.ev_chunk[0], hipEventDisableTiming));
    SMCHK(hipEventCreateWithFlags(&r.ev_chunk[1], hipEventDisableTiming));
    SMCHK(hipEventCreateWithFlags(&r.ev_stage[0], hipEventDisableTiming));
    SMCHK(hipEventCreateWithFlags(&r.ev_stage[1], hipEventDisableTiming));
    r.in_cap = s.in_cap;
    r.out_cap = s.out_cap;
    e->ev0 = r.ev0; e->ev1 = r.ev1; e->evc0 = r.evc0; e->evc1 = r.evc1;
    e->ev_chunk[0] = r.ev_chunk[0]; e->ev_chunk[1] = r.ev_chunk[1];
  }
  tick("host: upload image, table, events");
  // ---- one upload, one launch per form, one download, one synchronisation ----
  if (P.n_small) {
    if (any_auto) SMCHK(lds_limit_once((const void *)k_setup_models_auto, 15));
    else SMCHK(lds_limit_once((const void *)k_setup_models, 14));
  }
  if (P.n_large) {
    if (any_auto_large) SMCHK(lds_limit_once((const void *)k_setup_models_large_auto, 18));
    else SMCHK(lds_limit_once((const void *)k_setup_models_large, 17));
  }
  miosqp_qp_engine *e0 = eng[0];
  SMCHK(hipEventRecord(e0->ev0, grp->stream));
  SMCHK(hipMemcpyAsync(dv, hs, P.up_bytes, hipMemcpyHostToDevice, grp->stream));
  if (prepare)
    hipLaunchKernelGGL(k_prepare_models, dim3((unsigned)B), dim3(pm::THREADS), P.lds_bytes_prepare, grp->stream,
                       reinterpret_cast<const pm::IO *>(dv + P.ptab_off));
  if (P.n_small && any_auto)
    hipLaunchKernelGGL(k_setup_models_auto, dim3((unsigned)P.n_small), dim3(sm::THREADS), P.lds_bytes, grp->stream,
                       reinterpret_cast<const SetupModel *>(dv));
  else if (P.n_small)
    hipLaunchKernelGGL(k_setup_models, dim3((unsigned)P.n_small), dim3(sm::THREADS), P.lds_bytes, grp->stream,
                       reinterpret_cast<const SetupModel *>(dv));
  if (P.n_large && any_auto_large)
    hipLaunchKernelGGL(k_setup_models_large_auto, dim3((unsigned)P.n_large), dim3(sm::THREADS), P.lds_bytes_large, grp->stream,
                       reinterpret_cast<const SetupModel *>(dv) + P.n_small);
  else if (P.n_large)
    hipLaunchKernelGGL(k_setup_models_large, dim3((unsigned)P.n_large), dim3(sm::THREADS), P.lds_bytes_large, grp->stream,
                       reinterpret_cast<const SetupModel *>(dv) + P.n_small);
  SMCHK(hipGetLastError());
  if (prepare)  // (the rows and scalings the device wrote, with the records behind them: one copy)
    SMCHK(hipMemcpyAsync(hs + P.pin_prep, dv + P.prep_off, P.prep_bytes + P.rec_bytes, hipMemcpyDeviceToHost, grp->stream));
  else
    SMCHK(hipMemcpyAsync(hs + P.pin_rec, dv + P.rec_off, P.rec_bytes, hipMemcpyDeviceToHost, grp->stream));
  SMCHK(hipEventRecord(e0->ev1, grp->stream));
  SMCHK(hipStreamSynchronize(grp->stream));
  float ms_dev = 0;
  SMCHK(hipEventElapsedTime(&ms_dev, e0->ev0, e0->ev1));
  tick(prepare ? "upload, k_prepare_models, set-up launches, rows and records back" : P.n_large ? "upload, set-up launches, records back" : any_auto ? "upload, k_setup_models_auto, records back" : "upload, k_setup_models, records back");
  const sm::Record *rec = reinterpret_cast<const sm::Record *>(hs + P.pin_rec);
  for (int b = 0; b < B; b++)
    if (rec[b].bad_pivot) {
      g_err = "KKT factorisation: non-positive pivot in the reduced Hessian (P not PSD?) (model " + std::to_string(b) + ", pivot " +
              std::to_string(rec[b].pivot);
      if (rec[b].bad_pivot == 2) {  // the factor at the rho the launch chose (the per-model two-set-up path fails there too)
        char at[64];
        snprintf(at, sizeof at, ", at the rho chosen at set-up %.17g", rec[b].rho);
        g_err += at;
      }
      g_err += ")";
      return fail(MIOSQP_EFACTOR);
    }
  // ---- prepared on the device: the host's mirrors of the scaled problem and of the rows, from the download (the panel's
  //      values are those at the rho the launch built with; c and cinv go to Dev before any chunk is captured) ----
  if (prepare) {
    for (int b = 0; b < B; b++) {
      miosqp_qp_engine *e = eng[(size_t)b];
      const sm::Slot &s = P.slot[(size_t)b];
      miosqp::Scaled &sc = e->sc;
      miosqp::Factor &f = e->fa;
      const size_t n = (size_t)e->n, M = (size_t)e->M;
      auto back = [&](int part, void *dst, size_t bytes) {
        if (bytes) memcpy(dst, hs + P.pin_prep + (s.part[part].off - P.prep_off), bytes);
      };
      const size_t I = sizeof(int), F = sizeof(double);
      back(sm::PV_IDX, f.panel_by_var.idx.data(), I * f.panel_by_var.idx.size());
      back(sm::PV_L, f.panel_by_var.val.data(), F * f.panel_by_var.val.size());
      back(sm::PV_AT, f.At_val.data(), F * f.At_val.size());
      back(sm::PC_IDX, f.panel_by_con.idx.data(), I * f.panel_by_con.idx.size());
      back(sm::PC_L, f.panel_by_con.val.data(), F * f.panel_by_con.val.size());
      back(sm::PC_A, f.A_val.data(), F * f.A_val.size());
      back(sm::PB_IDX, f.Pbar.idx.data(), I * f.Pbar.idx.size());
      back(sm::PB_VAL, f.Pbar.val.data(), F * f.Pbar.val.size());
      back(sm::PR_IDX, f.Praw.idx.data(), I * f.Praw.idx.size());
      back(sm::PR_VAL, f.Praw.val.data(), F * f.Praw.val.size());
      sc.D.resize(n); sc.Dinv.resize(n); sc.E.resize(M); sc.Einv.resize(M); sc.q.resize(n);
      back(sm::D_, sc.D.data(), F * n);
      back(sm::DINV, sc.Dinv.data(), F * n);
      back(sm::E_, sc.E.data(), F * M);
      back(sm::EINV, sc.Einv.data(), F * M);
      back(sm::Q, sc.q.data(), F * n);
      const pm::Scalars *ps = reinterpret_cast<const pm::Scalars *>(hs + P.pin_prep + (s.scal.off - P.prep_off));
      sc.c = ps->c;
      sc.cinv = ps->cinv;
      e->d.c = sc.c;
      e->d.cinv = sc.cinv;
      // the scaled CSC: a column of P's upper triangle opens its row of Pbar, a column of A is its row by variable
      sc.Px.resize(sc.Pi.size());
      sc.Ax.resize(sc.Ai.size());
      for (size_t j = 0; j < n; j++) {
        const size_t cp = (size_t)(sc.Pp[j + 1] - sc.Pp[j]), ca = (size_t)(sc.Ap[j + 1] - sc.Ap[j]);
        if (cp) memcpy(&sc.Px[(size_t)sc.Pp[j]], &f.Pbar.val[(size_t)f.Pbar.ptr[j]], F * cp);
        if (ca) memcpy(&sc.Ax[(size_t)sc.Ap[j]], &f.At_val[(size_t)f.panel_by_var.ptr[j]], F * ca);
      }
    }
    tick("host: mirrors from the download");
  }
  // ---- rho chosen in the launch: the host's mirror follows (st, Dev, the factor's rho and the panel's values, formed
  //      with the expression the kernel used, which is build_factor(reuse_rows)'s) ----
  for (int b = 0; b < B; b++) {
    if (!ms[b].settings->rho_auto) continue;
    miosqp_qp_engine *e = eng[(size_t)b];
    const double rho = rec[b].rho;
    e->st.rho_auto = 1;
    if (rho == e->st.rho) continue;
    e->st.rho = rho;
    e->d.rho = rho;
    e->d.rho_inv = 1.0 / rho;
    miosqp::Factor &f = e->fa;
    f.rho = rho;
    for (size_t k = 0; k < f.At_val.size(); k++) f.panel_by_var.val[k] = f.At_val[k] == 0.0 ? 0.0 : -rho * f.At_val[k];
    for (size_t k = 0; k < f.A_val.size(); k++) f.panel_by_con.val[k] = f.A_val[k] == 0.0 ? 0.0 : -rho * f.A_val[k];
  }
  // ---- the engines: the fields miosqp_qp_setup sets for resident + fold + W.  (From here on the slab is staging.) ----
  int cus = 0;
  {
    hipDeviceProp_t prop;
    SMCHK(hipGetDeviceProperties(&prop, device));
    cus = prop.multiProcessorCount;
  }
  for (int b = 0; b < B; b++) {
    const miosqp_setup_model &m = ms[b];
    miosqp_qp_engine *e = eng[(size_t)b];
    const sm::Slot &s = P.slot[(size_t)b];
    const miosqp::Factor &f = e->fa;
    Dev &d = e->d;
    const int n = m.n, M = m.M;
    e->rt.h_in = reinterpret_cast<double *>(hs + s.pin_in);
    e->rt.h_out = reinterpret_cast<double *>(hs + s.pin_out);
    e->rt.h_ctrl = reinterpret_cast<Ctrl *>(hs + s.pin_ctrl);
    e->rt.h_ctrl2 = reinterpret_cast<Ctrl *>(hs + s.pin_ctrl2);
    e->h_in = e->rt.h_in; e->h_out = e->rt.h_out; e->h_ctrl = e->rt.h_ctrl; e->h_ctrl2 = e->rt.h_ctrl2;
    e->tpr_pv = pick_tpr((double)f.nnz_panel / n);
    e->tpr_pc = pick_tpr((double)f.nnz_panel / M);
    e->tpr_tail = pick_tpr(0.5 * n);
    e->tpr_pb = pick_tpr((double)f.Pbar.nnz / n);
    e->tpr_pr = pick_tpr((double)f.Praw.nnz / n);
    e->fold = true;
    e->tpr_ff = pick_tpr(M + 0.5 * n);
    e->tpr_fx = pick_tpr(0.5 * n);
    e->tpr_fc = pick_tpr((double)n);
    e->sp_nnzA = f.panel_by_con.idx.size();
    e->sp_nnzP = f.Pbar.idx.size();
    if (form[(size_t)b] == sm::FORM_LARGE) {
      // the fields miosqp_qp_setup sets with coop = 0, resident = 0, fold = 1, pers = 0: the product form on the device, the
      // iterations as captured chunks (d.W and d.Kc are NULL: the graphs hold Dev by value)
      e->coop_cus = cus;
      if (const char *ev = getenv("MIOSQP_COOP_DBG")) d.coop_dbg = atoi(ev);
      tuning_from_env(e);
      e->chunk = e->st.check_termination;
      e->tail_iters = e->st.max_iter % e->chunk;
      int rc = capture_chunk(e, e->chunk, &e->g_full, &e->x_full);
      if (!rc && e->tail_iters > 0) rc = capture_chunk(e, e->tail_iters, &e->g_tail, &e->x_tail);
      if (!rc && m.n_int >= 0) {
        rc = miosqp_qp_set_integer_rows(e, m.n_int, m.i_idx, m.m_orig);
        if (!rc && m.l_root) rc = miosqp_qp_set_root(e, m.l_root, m.u_root, m.eps_int_feas, m.eps_lin);
      }
      if (rc) {
        g_err += " (model " + std::to_string(b) + ")";
        return fail(rc < 0 ? rc : MIOSQP_EARG);
      }
      continue;
    }
    size_t need = resident_lds_doubles(n, M, true) * sizeof(double);
    const bool sp_on = !(getenv("MIOSQP_RES_SP") && atoi(getenv("MIOSQP_RES_SP")) == 0);
    const size_t sp_bytes = res_sp_doubles(e->sp_nnzA, e->sp_nnzP, n, M) * sizeof(double);
    if (sp_on && need + sp_bytes <= 150 * 1024) {
      e->res_sp_off = (int)(need / sizeof(double));
      need += sp_bytes;
    }
    e->resident = true;
    e->res_lds = need;
    e->guard_tol = tol;
    if (tol < 0) {  // switched off (inverse_guard)
      e->guard_resid = -1.0;
      e->guard_tripped = false;
    } else {
      e->guard_resid = rec[b].guard;
      e->guard_tripped = !(rec[b].guard <= tol);
      if (e->guard_tripped)
        fprintf(stderr, "miosqp: explicit KKT inverse residual %.3g above %.3g (ill-conditioned KKT matrix): this engine iterates with "
                        "the factor's sweeps instead\n", rec[b].guard, tol);
    }
    if (e->guard_tripped) {  // as miosqp_qp_setup: the workgroup keeps the product-form sweeps in LDS, if they fit
      d.W = nullptr;
      d.Kc = nullptr;
      e->res_sp_off = -1;
      const size_t need2 = resident_lds_doubles(n, M, false) * sizeof(double);
      if (need2 <= 160 * 1024) e->res_lds = need2;
      else e->resident = false;
    }
    if (e->resident) {
      SMCHK(lds_limit_once((const void *)k_resident, 0));
      resident_lane_groups(e);
    }
    e->coop_cus = cus;
    if (const char *ev = getenv("MIOSQP_COOP_DBG")) d.coop_dbg = atoi(ev);
    tuning_from_env(e);
    e->chunk = e->st.check_termination;
    e->tail_iters = e->st.max_iter % e->chunk;
    if (!e->resident) {  // (a tripped guard on a model whose product form does not fit the LDS: the captured chunks)
      int rc = capture_chunk(e, e->chunk, &e->g_full, &e->x_full);
      if (!rc && e->tail_iters > 0) rc = capture_chunk(e, e->tail_iters, &e->g_tail, &e->x_tail);
      if (rc) return fail(rc);
    }
    if (m.n_int >= 0) {
      int rc = miosqp_qp_set_integer_rows(e, m.n_int, m.i_idx, m.m_orig);
      if (!rc && m.l_root) rc = miosqp_qp_set_root(e, m.l_root, m.u_root, m.eps_int_feas, m.eps_lin);
      if (rc) {
        g_err += " (model " + std::to_string(b) + ")";
        return fail(rc < 0 ? rc : MIOSQP_EARG);
      }
    }
  }
#undef SMCHK
  tick("engines");
  for (int b = 0; b < B; b++) out[b] = eng[(size_t)b];
  const double wall_s = wall() - t_begin;
  stats->models = B;
  stats->launches = (P.n_small ? 1 : 0) + (P.n_large ? 1 : 0) + (prepare ? 1 : 0);
  stats->device_mallocs = (int32_t)(g_made_device_mallocs - made0[0]);  // (with what the engines' own pools took, if anything)
  stats->host_mallocs = (int32_t)(g_made_host_mallocs - made0[1]);
  stats->streams = (int32_t)(g_made_streams - made0[2]);
  stats->reserved = 0;
  stats->arena_bytes = (int64_t)P.total_bytes;
  stats->pinned_bytes = (int64_t)P.pin_bytes;
  stats->lds_bytes = (int64_t)std::max(P.lds_bytes, P.lds_bytes_large);
  stats->device_time = 1e-3 * ms_dev;
  stats->run_time = wall_s;
  if (t_on) fprintf(stderr, "[miosqp setup_models] %-36s %8.3f ms  (%d models)\n", "miosqp_qp_setup_models, all of it", 1e3 * wall_s, (int)B);
  group_unref(grp);  // the call's own reference: the engines hold the rest
  return 0;
}

}  // namespace
