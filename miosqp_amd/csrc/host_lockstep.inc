// part of engine.hip (included there, not compiled alone): B branch-and-bound trees advanced in lock step, driven from the
// host in C++ on device-resident leaves (C ABI miosqp_qp_solve_trees_lockstep, and miosqp_qp_solve_trees_lockstep_rf with
// round and fix between a node's verdict and its children: one more batch per wave over all trees that fire).  The
// wave loop of miosqp_amd/lockstep.py -- per wave one node of every unfinished tree, solved together as the lock-step
// batch with a cost per column -- with the tree logic of lockstep_trees.hpp and the kernels of kernels_lockstep.inc around an unchanged slice_run.  Per wave
// the host sends five integers per column and reads one 64-byte record per column back; no vector crosses PCIe between
// the upload of the roots and the download of the incumbents.
namespace {

struct LockstepStore {
  // per instance: root bounds, raw and scaled costs, incumbents (one allocation, grown when a call brings more instances)
  int inst_cap = 0;
  double *inst_block = nullptr;
  // the slot store shared by all trees (one allocation: lo | hi | x | y, laid out and doubled as search_grow does)
  int cap = 0;
  double *slot_block = nullptr;
  // per column of a wave: the triples (+ child slots) and the incumbent pairs going up, the records coming back
  int col_cap = 0;
  int *d_trip = nullptr, *d_pairs = nullptr;
  LsRec *d_rec = nullptr;
  int *h_trip = nullptr, *h_pairs = nullptr;  // pinned
  LsRec *h_rec = nullptr;                     // pinned
  LsDev dev{};
  std::vector<double> stage;
  miosqp::lockstep::Slots slots;
  std::vector<miosqp::lockstep::Tree> trees;
  void *refill = nullptr;  // RefillCols (host_refill.inc): the per-column arrays of solve_trees_refill
  void *ahead = nullptr;   // AheadCols (host_lockstep_ahead.inc): the mandatory flags and records of solve_trees_lockstep_ahead
  void *sb = nullptr;      // SbStore (host_lockstep_sb.inc): the branching step of solve_trees_lockstep_sb
  // round and fix (solve_trees_lockstep_rf): per candidate column of a heuristic batch the five integers going up, per
  // firing tree its record coming back and, for the winners the host adopts, the tree's number going up
  int rf_inst_cap = 0, rf_col_cap = 0, rf_trip_inst = 0;  // (rf_trip_inst: the trees the column block's second part holds)
  double *rf_block = nullptr;  // [ rf.x | run[0] | run[1] | rec | cand ]
  std::vector<LsRfCand> rf_cand;  // (debug: a batch's candidates on the host, when the caller asked for them)
  int *d_rf_trip = nullptr, *d_rf_adopt = nullptr;
  int *h_rf_trip = nullptr, *h_rf_adopt = nullptr;  // pinned (one block)
  LsRfGroup *h_rf_rec = nullptr;                    // pinned
  LsRfDev rf{};
  hipEvent_t rf_ev0 = nullptr, rf_ev1 = nullptr;    // around a heuristic batch
  std::vector<int> fire;      // the wave's columns whose tree fires
  std::vector<char> branch;   // per column of the wave: its node branches (the verdict, kept from begin to end)
};

void refill_free(void *p);  // (host_refill.inc)
void ahead_free(void *p);   // (host_lockstep_ahead.inc)
void sb_free(void *p);      // (host_lockstep_sb.inc)

// kls_heur_rows in place of kb_heur_rows at the end of slice_run (declared in host.inc; the kernel is used here, see kernels_lockstep.inc)
void launch_ls_heur_rows(miosqp_qp_engine *e, const LsRoots &roots, int ntiles) {
  hipLaunchKernelGGL(kls_heur_rows<0>, dim3((e->d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, e->d, roots);
}

void lockstep_free(void *p) {
  LockstepStore *L = static_cast<LockstepStore *>(p);
  if (!L) return;
  if (L->inst_block) hipFree(L->inst_block);
  if (L->slot_block) hipFree(L->slot_block);
  if (L->d_trip) hipFree(L->d_trip);
  if (L->h_trip) hipHostFree(L->h_trip);
  if (L->h_rec) hipHostFree(L->h_rec);
  if (L->rf_block) hipFree(L->rf_block);
  if (L->d_rf_trip) hipFree(L->d_rf_trip);
  if (L->h_rf_trip) hipHostFree(L->h_rf_trip);
  if (L->h_rf_rec) hipHostFree(L->h_rf_rec);
  if (L->rf_ev0) hipEventDestroy(L->rf_ev0);
  if (L->rf_ev1) hipEventDestroy(L->rf_ev1);
  refill_free(L->refill);
  ahead_free(L->ahead);
  sb_free(L->sb);
  delete L;
}

size_t ls_al(size_t doubles) { return (doubles + 31) & ~(size_t)31; }  // (256-byte boundaries)

int ls_malloc(double **out, size_t doubles, const char *what) {
  if (hipMalloc((void **)out, doubles * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    g_err = std::string("solve_trees_lockstep: no device memory for ") + what + " (" + std::to_string(doubles * sizeof(double)) + " bytes)";
    return MIOSQP_EFULL;
  }
  return 0;
}

// room for B instances and B columns per wave
int lockstep_reserve(miosqp_qp_engine *e, LockstepStore &L, int B) {
  const size_t n = e->n, M = e->M;
  if (B > L.inst_cap) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (L.inst_block) hipFree(L.inst_block);
    L.inst_block = nullptr;
    L.inst_cap = 0;
    const size_t cap = (size_t)B, oM = ls_al(cap * M), on = ls_al(cap * n);
    if (int rc = ls_malloc(&L.inst_block, 2 * oM + 3 * on, "the instances")) return rc;
    double *p = L.inst_block;
    L.dev.root_l = p; p += oM;
    L.dev.root_u = p; p += oM;
    L.dev.qraw = p; p += on;
    L.dev.qs = p; p += on;
    L.dev.inc = p;
    L.inst_cap = B;
  }
  if (B > L.col_cap) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (L.d_trip) hipFree(L.d_trip);
    if (L.h_trip) hipHostFree(L.h_trip);
    if (L.h_rec) hipHostFree(L.h_rec);
    L.d_trip = nullptr; L.h_trip = nullptr; L.h_rec = nullptr;
    L.col_cap = 0;
    const size_t cap = (size_t)B, ints = (LS_TRIP + 3) * cap, ints_al = (ints + 63) & ~(size_t)63;
    // one device allocation: [triples | pairs | records]
    if (hipMalloc((void **)&L.d_trip, ints_al * sizeof(int) + cap * sizeof(LsRec)) != hipSuccess) {
      (void)hipGetLastError();
      L.d_trip = nullptr;
      g_err = "solve_trees_lockstep: no device memory for the wave's columns";
      return MIOSQP_EFULL;
    }
    L.d_pairs = L.d_trip + LS_TRIP * cap;
    L.d_rec = reinterpret_cast<LsRec *>(L.d_trip + ints_al);
    HIPCHK(hipHostMalloc((void **)&L.h_trip, ints * sizeof(int), hipHostMallocDefault));
    L.h_pairs = L.h_trip + LS_TRIP * cap;
    HIPCHK(hipHostMalloc((void **)&L.h_rec, cap * sizeof(LsRec), hipHostMallocDefault));
    L.col_cap = B;
  }
  return 0;
}

// the slot store at `ncap` slots; the first `keep` slots of the old one are copied on the engine's stream (every later
// reader is queued behind the copies) and the old one is released once they are done
int lockstep_slots(miosqp_qp_engine *e, LockstepStore &L, int ncap, int keep) {
  const size_t n = e->n, M = e->M, p = e->d.n_int, c = (size_t)ncap;
  if (c > ((size_t)1 << 29)) {
    g_err = "solve_trees_lockstep: the slot store cannot grow any further";
    return MIOSQP_EFULL;
  }
  const size_t o_hi = ls_al(c * p), o_x = o_hi + ls_al(c * p), o_y = o_x + ls_al(c * n), total = o_y + ls_al(c * M);
  double *blk = nullptr;
  if (int rc = ls_malloc(&blk, total, "the slot store")) return rc;
  double *lo = blk, *hi = blk + o_hi, *x = blk + o_x, *y = blk + o_y;
  if (L.slot_block) {
    if (keep > 0) {
      const size_t k = (size_t)keep;
      HIPCHK(hipMemcpyAsync(lo, L.dev.lo, sizeof(double) * k * p, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(hi, L.dev.hi, sizeof(double) * k * p, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(x, L.dev.x, sizeof(double) * k * n, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(y, L.dev.y, sizeof(double) * k * M, hipMemcpyDeviceToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));  // (growing happens a handful of times per call: the wait does not matter)
    hipFree(L.slot_block);
  }
  L.slot_block = blk;
  L.dev.lo = lo; L.dev.hi = hi; L.dev.x = x; L.dev.y = y;
  L.cap = ncap;
  return 0;
}

// room for the heuristic batches of B trees with K candidates each
int lockstep_rf_reserve(miosqp_qp_engine *e, LockstepStore &L, int B, int K) {
  const size_t n = e->n;
  if (!L.rf_ev0) {
    HIPCHK(hipEventCreate(&L.rf_ev0));
    HIPCHK(hipEventCreate(&L.rf_ev1));
  }
  if (B > L.rf_inst_cap) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (L.rf_block) hipFree(L.rf_block);
    if (L.h_rf_rec) hipHostFree(L.h_rf_rec);
    L.rf_block = nullptr; L.h_rf_rec = nullptr;
    L.rf_inst_cap = 0;
    const size_t cap = (size_t)B, ox = ls_al(cap * n), og = ls_al(cap * sizeof(LsRfGroup) / sizeof(double)),
                 oc = ls_al(cap * RF_MAX_K * sizeof(LsRfCand) / sizeof(double));
    if (int rc = ls_malloc(&L.rf_block, ox + 3 * og + oc, "the heuristic's winners")) return rc;
    L.rf.x = L.rf_block;
    L.rf.run[0] = reinterpret_cast<LsRfGroup *>(L.rf_block + ox);
    L.rf.run[1] = reinterpret_cast<LsRfGroup *>(L.rf_block + ox + og);
    L.rf.rec = reinterpret_cast<LsRfGroup *>(L.rf_block + ox + 2 * og);
    L.rf.cand = reinterpret_cast<LsRfCand *>(L.rf_block + ox + 3 * og);
    HIPCHK(hipHostMalloc((void **)&L.h_rf_rec, cap * sizeof(LsRfGroup), hipHostMallocDefault));
    L.rf_inst_cap = B;
  }
  const size_t cols = (size_t)B * (size_t)K;
  if (cols > (size_t)L.rf_col_cap || L.rf_trip_inst != L.rf_inst_cap) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (L.d_rf_trip) hipFree(L.d_rf_trip);
    if (L.h_rf_trip) hipHostFree(L.h_rf_trip);
    L.d_rf_trip = nullptr; L.h_rf_trip = nullptr;
    L.rf_col_cap = 0;
    // one block each: [five integers per candidate column | the adopted trees], rf_inst_cap of those
    const size_t ints = LS_TRIP * cols + (size_t)L.rf_inst_cap;
    if (hipMalloc((void **)&L.d_rf_trip, ints * sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      L.d_rf_trip = nullptr;
      g_err = "solve_trees_lockstep_rf: no device memory for the heuristic's columns";
      return MIOSQP_EFULL;
    }
    L.d_rf_adopt = L.d_rf_trip + LS_TRIP * cols;
    HIPCHK(hipHostMalloc((void **)&L.h_rf_trip, ints * sizeof(int), hipHostMallocDefault));
    L.h_rf_adopt = L.h_rf_trip + LS_TRIP * cols;
    L.rf_col_cap = (int)cols;
    L.rf_trip_inst = L.rf_inst_cap;
  }
  return 0;
}

// what round and fix asks of lockstep_trees_run (K = 0: the heuristic is off, nothing of it is touched)
struct LsRfArgs {
  int K, max_iter, every;
  miosqp_lockstep_rf_stats *stats;
};

// the body of miosqp_qp_solve_trees_lockstep and, with rf.K > 0, of miosqp_qp_solve_trees_lockstep_rf
int lockstep_trees_run(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u, const double *x0,
                       const double *y0, const double *upper0, const double *x_inc0, int32_t tree_explor_rule,
                       int32_t max_iter_bb, int32_t capacity, double *x_out, miosqp_tree_info *info,
                       miosqp_lockstep_stats *stats, const LsRfArgs &rf) {
  using miosqp::lockstep::Record;
  using miosqp::lockstep::Tree;
  using miosqp::lockstep::Verdict;
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || !stats || max_iter_bb < 1 ||
      tree_explor_rule < 0 || tree_explor_rule > 3 || capacity < 0)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = "solve_trees_lockstep: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending) {
    g_err = "solve_trees_lockstep: streaming chunks are still in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M, m = (size_t)e->d.m_orig, p = (size_t)e->d.n_int;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) {  // (nothing has been queued)
      g_err = "solve_trees_lockstep: l > u in the root of instance " + std::to_string(k / M);
      return MIOSQP_EBOUNDS;
    }
  stats->waves = stats->max_width = stats->grown = 0;
  stats->nodes = stats->iters_slowest = stats->iters_all = 0;
  stats->device_time = stats->run_time = stats->host_time = 0.0;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  if (!e->lockstep) e->lockstep = new LockstepStore();
  LockstepStore &L = *static_cast<LockstepStore *>(e->lockstep);
  if (int rc = lockstep_reserve(e, L, B)) return rc;
  if (rf.K > 0) {
    if (int rc = lockstep_rf_reserve(e, L, B, rf.K)) return rc;
    miosqp_lockstep_rf_stats *rs = rf.stats;
    rs->batches = 0;
    rs->columns = rs->iters_slowest = 0;
    rs->device_time = 0.0;
  }
  {
    // `capacity` is a starting size: a store left by an earlier call is kept when the caller leaves the size to us
    const int want = capacity > 0 ? std::max(capacity, 4) : std::max(64, 4 * B);
    if (!L.slot_block || (capacity > 0 ? L.cap != want : L.cap < want))
      if (int rc = lockstep_slots(e, L, want, 0)) return rc;
    while (L.cap < B) {  // (a starting size below the number of roots)
      if (int rc = lockstep_slots(e, L, 2 * L.cap, 0)) return rc;
      stats->grown++;
    }
  }
  const double t0 = wall();
  struct PqScope {  // every launch helper and the chunk-graph cache look at e->pq; off again on every way out
    miosqp_qp_engine *e;
    explicit PqScope(miosqp_qp_engine *e_) : e(e_) { e->pq = 1; }
    ~PqScope() { e->pq = 0; }
  } scope(e);
  const Dev &d = e->d;
  L.slots.reset(L.cap);
  L.trees.assign((size_t)B, Tree());
  L.fire.clear();  // (a call that ended in an error between begin and end may have left some)
  // ---- the roots: bounds, costs and incumbents per instance; tree b's root is slot b (integer rows of l, u; x0, y0) ----
  {
    const size_t tot = (size_t)B * (2 * M + 2 * n + 2 * p + n + M);
    if (L.stage.size() < tot) L.stage.resize(tot);
    double *h_inc = L.stage.data(), *h_lo = h_inc + (size_t)B * n, *h_hi = h_lo + (size_t)B * p;
    for (int b = 0; b < B; b++) {
      const bool have = x_inc0 != nullptr && upper0[b] < miosqp::lockstep::NO_UPPER;
      if (have) memcpy(h_inc + (size_t)b * n, x_inc0 + (size_t)b * n, sizeof(double) * n);
      else memset(h_inc + (size_t)b * n, 0, sizeof(double) * n);
      memcpy(h_lo + (size_t)b * p, l + (size_t)b * M + m, sizeof(double) * p);
      memcpy(h_hi + (size_t)b * p, u + (size_t)b * M + m, sizeof(double) * p);
      const int s = L.slots.take();  // == b: the free list is fresh
      L.trees[(size_t)b].start(L.slots, s, have ? upper0[b] : miosqp::lockstep::NO_UPPER);
    }
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    // (the sources are the caller's arrays and this call's staging vector: pageable, so the copies are done when they return)
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_l), l, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_u), u, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.qraw), q, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.inc, h_inc, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.lo, h_lo, sizeof(double) * (size_t)B * p, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.hi, h_hi, sizeof(double) * (size_t)B * p, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.x, x0, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.y, y0, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // qbar_b = c D q_b, ONE launch per call: the bits solve_batch_q gives its columns every wave
    hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, d, L.dev.qraw,
                       const_cast<double *>(L.dev.qs), B);
  }
  std::vector<int> live;
  live.reserve((size_t)B);
  int64_t iters_total = 0;
  // ---- the waves ----
  double host_s = 0.0;  // choosing, absorbing, bookkeeping: the wall time between a wave's record and the next wave's launches
  for (;;) {
    double th = wall();
    live.clear();
    for (int b = 0; b < B; b++)
      if (L.trees[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    const int W = (int)live.size();
    while (L.slots.free_count() < 2 * (size_t)W) {  // two child slots per column
      const int keep = L.cap;
      if (int rc = lockstep_slots(e, L, 2 * L.cap, keep)) return rc;
      L.slots.grow(L.cap);
      stats->grown++;
    }
    for (int c = 0; c < W; c++) {
      Tree &T = L.trees[(size_t)live[(size_t)c]];
      const int s = T.pop(L.slots, tree_explor_rule);
      int *tr = L.h_trip + LS_TRIP * c;
      tr[LS_TREE] = live[(size_t)c];
      tr[LS_SLOT] = s;
      tr[LS_WARM] = L.slots.warm_slot(s);
      tr[LS_CHILD0] = L.slots.take();
      tr[LS_CHILD1] = L.slots.take();
    }
    host_s += wall() - th;
    for (int s0 = 0; s0 < W; s0 += e->Bcap) {  // a wave wider than max_batch runs in slices, as solve_batch_q runs it
      const int nb = W - s0 < e->Bcap ? W - s0 : e->Bcap;
      const int ntiles = (nb + 63) / 64;
      if (int rc = slice_begin(e, nb)) return rc;
      if (s0 == 0)  // the wave's one upload (behind slice_begin, as solve_slice queues its own)
        HIPCHK(hipMemcpyAsync(L.d_trip, L.h_trip, sizeof(int) * LS_TRIP * (size_t)W, hipMemcpyHostToDevice, e->stream));
      const int *trip = L.d_trip + LS_TRIP * s0;
      const int big = (int)(n > M ? n : M);
      hipLaunchKernelGGL(kls_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb);
      const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
      if (int rc = slice_run(e, nb, e->st.max_iter, &roots)) return rc;
      hipLaunchKernelGGL(kls_scatter<0>, dim3((int)((n + 63) / 64 + (M + 63) / 64) + 1, ntiles), dim3(256), 0, e->stream, d, L.dev, trip,
                         L.d_rec + s0, nb);
    }
    HIPCHK(hipMemcpyAsync(L.h_rec, L.d_rec, sizeof(LsRec) * (size_t)W, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    // ---- bound_and_branch per tree on its column's record ----
    th = wall();
    const int wave = ++stats->waves;
    int it_max = 0, npairs = 0;
    if (rf.K > 0) L.branch.assign((size_t)W, 0);
    int64_t it_sum = 0;
    for (int c = 0; c < W; c++) {
      const LsRec &g = L.h_rec[c];
      const int *tr = L.h_trip + LS_TRIP * c;
      const int b = tr[LS_TREE];
      Tree &T = L.trees[(size_t)b];
      Record r;
      r.ok = g.status == MIOSQP_QP_SOLVED || g.status == MIOSQP_QP_MAX_ITER_REACHED;
      r.iter = g.iter;
      r.lower = g.lower;
      r.int_inf = g.int_inf;
      r.nextvar = g.nextvar;
      r.heur_feasible = g.hviol <= 0.0;
      r.heur_obj = g.hobj;
      if (stats->node_hviol && T.nodes < stats->node_cap) stats->node_hviol[(size_t)b * stats->node_cap + T.nodes] = g.hviol;
      // (with round and fix: up to the point where the children would enter the list; they enter after the heuristic batch)
      const miosqp::lockstep::Begun bg = T.begin(L.slots, tr[LS_SLOT], r, rf.K > 0 ? rf.every : 0);
      const Verdict v = bg.v;
      if (rf.K == 0) T.end(L.slots, tr[LS_SLOT], tr[LS_CHILD0], tr[LS_CHILD1], v);  // (begin + end: Tree::absorb)
      if (v.branch && g.crossed) {
        g_err = "solve_trees_lockstep: branching produced l > u (instance " + std::to_string(b) + ")";
        return MIOSQP_EBOUNDS;
      }
      if (v.incumbent) {
        int *pr = L.h_pairs + 3 * npairs++;
        pr[0] = b;
        pr[1] = tr[LS_SLOT];
        pr[2] = v.incumbent == 2;
      }
      if (rf.K > 0) {
        L.branch[(size_t)c] = v.branch;
        if (bg.fire) L.fire.push_back(c);
      } else if (!T.can_continue(max_iter_bb)) T.finished_at = wave;
      it_max = g.iter > it_max ? g.iter : it_max;
      it_sum += g.iter;
    }
    host_s += wall() - th;
    if (npairs > 0) {  // (the pairs' pinned block is next written after the next wave's drain: this copy is done by then)
      HIPCHK(hipMemcpyAsync(L.d_pairs, L.h_pairs, sizeof(int) * 3 * (size_t)npairs, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_incumbent<0>, dim3(npairs), dim3(256), 0, e->stream, d, L.dev, L.d_pairs, npairs);
    }
    if (rf.K > 0) {
      // ---- round and fix: the K candidates of every tree that fires, ONE batch; then the children of the whole wave ----
      const int K = rf.K, F = (int)L.fire.size(), C = F * K;
      if (F > 0) {
        th = wall();
        for (int f = 0; f < F; f++) {
          const int *tr = L.h_trip + LS_TRIP * L.fire[(size_t)f];
          for (int k = 0; k < K; k++) {
            int *ct = L.h_rf_trip + LS_TRIP * ((size_t)f * K + k);
            ct[LS_TREE] = tr[LS_TREE];
            ct[LS_SLOT] = ct[LS_WARM] = tr[LS_SLOT];  // the node's own x, y (it is held until its children are decided)
            ct[LS_RF_K] = k;
            ct[LS_RF_GROUP] = f;
          }
        }
        host_s += wall() - th;
        HIPCHK(hipEventRecord(L.rf_ev0, e->stream));
        int slice = 0;
        for (int s0 = 0; s0 < C; s0 += e->Bcap, slice++) {  // sliced as a wave is; a tree's candidates may straddle two slices
          const int nb = C - s0 < e->Bcap ? C - s0 : e->Bcap;
          const int ntiles = (nb + 63) / 64;
          if (int rc = slice_begin(e, nb)) return rc;
          if (s0 == 0)
            HIPCHK(hipMemcpyAsync(L.d_rf_trip, L.h_rf_trip, sizeof(int) * LS_TRIP * (size_t)C, hipMemcpyHostToDevice, e->stream));
          const int *trip = L.d_rf_trip + LS_TRIP * s0;
          const int big = (int)(n > M ? n : M);
          hipLaunchKernelGGL(kls_rf_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb, K);
          const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
          if (int rc = slice_run(e, nb, rf.max_iter, &roots)) return rc;
          hipLaunchKernelGGL(kls_rf_keep<0>, dim3((int)((n + 63) / 64) + 1, ntiles), dim3(256), 0, e->stream, d, L.rf, trip, s0, nb, K, slice);
        }
        HIPCHK(hipMemcpyAsync(L.h_rf_rec, L.rf.rec, sizeof(LsRfGroup) * (size_t)F, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(L.rf_ev1, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        float rf_ms = 0;
        HIPCHK(hipEventElapsedTime(&rf_ms, L.rf_ev0, L.rf_ev1));
        rf.stats->batches++;
        rf.stats->columns += C;
        rf.stats->device_time += 1e-3 * rf_ms;
        miosqp_lockstep_rf_stats *rs = rf.stats;
        if (rs->cand_status || rs->cand_iter || rs->cand_obj || rs->cand_viol) {  // debug: the candidates of every tree's FIRST call
          bool any = false;
          for (int f = 0; f < F && !any; f++) any = L.trees[(size_t)L.h_trip[LS_TRIP * L.fire[(size_t)f] + LS_TREE]].rf_calls == 0;
          if (any) {
            L.rf_cand.resize((size_t)C);
            HIPCHK(hipMemcpy(L.rf_cand.data(), L.rf.cand, sizeof(LsRfCand) * (size_t)C, hipMemcpyDeviceToHost));
            for (int f = 0; f < F; f++) {
              const size_t b = (size_t)L.h_trip[LS_TRIP * L.fire[(size_t)f] + LS_TREE];
              if (L.trees[b].rf_calls != 0) continue;
              for (int k = 0; k < K; k++) {
                const LsRfCand &cd = L.rf_cand[(size_t)f * K + k];
                if (rs->cand_status) rs->cand_status[b * K + k] = cd.status;
                if (rs->cand_iter) rs->cand_iter[b * K + k] = cd.iter;
                if (rs->cand_obj) rs->cand_obj[b * K + k] = cd.obj;
                if (rs->cand_viol) rs->cand_viol[b * K + k] = cd.viol;
              }
            }
          }
        }
      }
      th = wall();
      int nadopt = 0, rf_it_max = 0;
      for (int f = 0; f < F; f++) {  // Workspace.primal_heuristic on the winner: one `< upper` test
        const LsRfGroup &g = L.h_rf_rec[f];
        const int b = L.h_trip[LS_TRIP * L.fire[(size_t)f] + LS_TREE];
        if (L.trees[(size_t)b].heuristic(L.slots, K, g.chosen >= 0, g.obj, g.feasible, g.iters)) L.h_rf_adopt[nadopt++] = b;
        rf_it_max = g.iter_max > rf_it_max ? g.iter_max : rf_it_max;
      }
      rf.stats->iters_slowest += rf_it_max;
      for (int c = 0; c < W; c++) {  // branch_children, in the order of the wave
        const int *tr = L.h_trip + LS_TRIP * c;
        Tree &T = L.trees[(size_t)tr[LS_TREE]];
        T.end(L.slots, tr[LS_SLOT], tr[LS_CHILD0], tr[LS_CHILD1], Verdict{L.branch[(size_t)c] != 0, 0});
        if (!T.can_continue(max_iter_bb)) T.finished_at = wave;
      }
      L.fire.clear();
      host_s += wall() - th;
      if (nadopt > 0) {  // (behind kls_incumbent; the pinned list is next written after the next heuristic batch's drain)
        HIPCHK(hipMemcpyAsync(L.d_rf_adopt, L.h_rf_adopt, sizeof(int) * (size_t)nadopt, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(kls_rf_incumbent<0>, dim3(nadopt), dim3(256), 0, e->stream, d, L.dev, L.rf, L.d_rf_adopt, nadopt);
      }
    }
    stats->nodes += W;
    stats->max_width = W > stats->max_width ? W : stats->max_width;
    stats->iters_slowest += it_max;
    stats->iters_all += it_sum;
    iters_total += it_sum;
    if (wave <= stats->wave_cap) {
      if (stats->wave_width) stats->wave_width[wave - 1] = W;
      if (stats->wave_iter_max) stats->wave_iter_max[wave - 1] = it_max;
      if (stats->wave_iter_mean) stats->wave_iter_mean[wave - 1] = (double)it_sum / W;
    }
  }
  // ---- the incumbents ----
  double *h_inc = L.stage.data();
  HIPCHK(hipMemcpyAsync(h_inc, L.dev.inc, sizeof(double) * (size_t)B * n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  for (int b = 0; b < B; b++) {
    const Tree &T = L.trees[(size_t)b];
    const bool have = x_inc0 != nullptr && upper0[b] < miosqp::lockstep::NO_UPPER;
    info[b].nodes = (int32_t)T.nodes;
    info[b].osqp_iter = (int32_t)T.iters;
    info[b].leaves_left = (int32_t)T.open.size();
    info[b].overflow = 0;
    info[b].max_leaves = (int32_t)T.max_open;
    info[b].found = T.found ? 1 : 0;
    info[b].upper_glob = T.upper;
    info[b].lower_glob = T.lower_glob(L.slots);
    info[b].device_time = 1e-3 * ms / B;
    info[b].run_time = wall_s / B;
    if (T.found || have) memcpy(x_out + (size_t)b * n, h_inc + (size_t)b * n, sizeof(double) * n);
    if (stats->finished_at) stats->finished_at[b] = T.finished_at;
    if (rf.K > 0) {
      miosqp_lockstep_rf_stats *rs = rf.stats;
      if (rs->calls) rs->calls[b] = (int32_t)T.rf_calls;
      if (rs->candidates) rs->candidates[b] = (int32_t)T.rf_candidates;
      if (rs->feasible) rs->feasible[b] = (int32_t)T.rf_feasible;
      if (rs->improved) rs->improved[b] = (int32_t)T.rf_improved;
      if (rs->iters) rs->iters[b] = T.rf_iters;
    }
  }
  stats->device_time = 1e-3 * ms;
  stats->run_time = wall_s;
  stats->host_time = host_s;
  e->loop_ms += ms;
  e->loop_iters += iters_total;
  return 0;
}

}  // namespace

extern "C" {

int miosqp_qp_solve_trees_lockstep(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, double *x_out,
                                   miosqp_tree_info *info, miosqp_lockstep_stats *stats) {
  return lockstep_trees_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info, stats,
                            LsRfArgs{0, 0, 0, nullptr});
}

int miosqp_qp_solve_trees_lockstep_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                      const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                      int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t rf_candidates,
                                      int32_t rf_max_iter, int32_t rf_every, double *x_out, miosqp_tree_info *info,
                                      miosqp_lockstep_stats *stats, miosqp_lockstep_rf_stats *rf_stats) {
  if (!e || !rf_stats) return MIOSQP_EARG;
  if (rf_candidates < 1 || rf_candidates > RF_MAX_K) {
    g_err = "solve_trees_lockstep_rf: rf_candidates must be in 1..32";
    return MIOSQP_EARG;
  }
  if (rf_max_iter <= 0 || (rf_max_iter % e->chunk != 0 && rf_max_iter != e->st.max_iter)) {
    g_err = "solve_trees_lockstep_rf: rf_max_iter must be a positive multiple of check_termination or the engine's max_iter";
    return MIOSQP_EARG;
  }
  if (rf_every < 1) {
    g_err = "solve_trees_lockstep_rf: rf_every must be at least 1";
    return MIOSQP_EARG;
  }
  return lockstep_trees_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info, stats,
                            LsRfArgs{rf_candidates, rf_max_iter, rf_every, rf_stats});
}

}  // extern "C"
