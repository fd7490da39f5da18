// part of engine.hip (included there, not compiled alone): B branch-and-bound trees advanced in lock step, driven from the
// host in C++ on device-resident leaves (C ABI miosqp_qp_solve_trees_lockstep, and miosqp_qp_solve_trees_lockstep_rf with
// round and fix between a node's verdict and its children: one more batch per wave over all trees that fire).  The
// wave loop of miosqp_amd/lockstep.py -- per wave one node of every unfinished tree, solved together as the lock-step
// batch with a cost per column -- with the tree logic of lockstep_trees.hpp and the kernels of kernels_lockstep.inc around an unchanged slice_run.  Per wave
// the host sends five integers per column and reads one 64-byte record per column back; no vector crosses PCIe between
// the upload of the roots and the download of the incumbents.
//
// Who owns what.  This file: the store (LockstepStore, lockstep_reserve, lockstep_slots); the pieces all five tree
// drivers are built from -- LsCall, ls_args_ok / ls_refuse / ls_crossed (checks and refusals), ls_open (store and
// slots), PqScope, ls_upload_roots, ls_room (slot growth), ls_record, ls_wave (a wave's slices), ls_push_incumbents,
// ls_stats_zero / ls_stats_wave, ls_finish (incumbents, events, info[]) --; the wave loop ls_trees_run with the step a
// driver puts between a wave's verdicts and its children (a Step); the plain step (nothing) and the round-and-fix step
// (the heuristic batch) with their two entries.  host_lockstep_sb.inc: the branching step and its entry.
// host_lockstep_ahead.inc and host_refill.inc: a loop of their own (planned waves whose last slice ends early; chunks
// with refilled columns) between the same pieces.
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

// ---- what the five tree drivers share (this file, host_refill.inc, host_lockstep_ahead.inc, host_lockstep_sb.inc) ----

// the arguments every driver takes, and the entry's name as its messages carry it
struct LsCall {
  const char *who;
  miosqp_qp_engine *e;
  int32_t B;
  const double *q, *l, *u, *x0, *y0, *upper0, *x_inc0;
  int32_t tree_explor_rule, max_iter_bb, capacity;
  double *x_out;
  miosqp_tree_info *info;
  bool has_incumbent(int b) const { return x_inc0 != nullptr && upper0[b] < miosqp::lockstep::NO_UPPER; }
};

// the argument check (no message, MIOSQP_EARG); an entry adds its own statistics pointers
bool ls_args_ok(const LsCall &a) {
  return a.e && a.B >= 1 && a.q && a.l && a.u && a.x0 && a.y0 && a.upper0 && a.x_out && a.info && a.max_iter_bb >= 1 &&
         a.tree_explor_rule >= 0 && a.tree_explor_rule <= 3 && a.capacity >= 0;
}

// the refusals behind ENTER, in their order: the engine is not ready, chunks are in flight, `own` (a refusal of the entry's
// own whose place is here, nullptr: none), l > u in a root
int ls_refuse(const LsCall &a, const char *own = nullptr) {
  const miosqp_qp_engine *e = a.e;
  const std::string who = std::string(a.who) + ": ";
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = who + "call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending) {
    g_err = who + "streaming chunks are still in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  if (own) {
    g_err = who + own;
    return MIOSQP_EARG;
  }
  const size_t M = e->M;
  for (size_t k = 0; k < (size_t)a.B * M; k++)
    if (a.l[k] > a.u[k]) {  // (nothing has been queued)
      g_err = who + "l > u in the root of instance " + std::to_string(k / M);
      return MIOSQP_EBOUNDS;
    }
  return 0;
}

// the error exit in the middle of a call: a child of instance b would have l > u
int ls_crossed(const LsCall &a, int b) {
  g_err = std::string(a.who) + ": branching produced l > u (instance " + std::to_string(b) + ")";
  return MIOSQP_EBOUNDS;
}

// the batched engine, the store with room for B instances and `cols` columns per wave, the slot store at its starting
// size (*grown counts the doublings a starting size below the number of roots costs)
int ls_open(const LsCall &a, int cols, LockstepStore **out, int32_t *grown) {
  miosqp_qp_engine *e = a.e;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  if (!e->lockstep) e->lockstep = new LockstepStore();
  LockstepStore &L = *static_cast<LockstepStore *>(e->lockstep);
  *out = &L;
  if (int rc = lockstep_reserve(e, L, cols)) return rc;
  // `capacity` is a starting size: a store left by an earlier call is kept when the caller leaves the size to us
  const int want = a.capacity > 0 ? std::max(a.capacity, 4) : std::max(64, 4 * a.B);
  if (!L.slot_block || (a.capacity > 0 ? L.cap != want : L.cap < want))
    if (int rc = lockstep_slots(e, L, want, 0)) return rc;
  while (L.cap < a.B) {
    if (int rc = lockstep_slots(e, L, 2 * L.cap, 0)) return rc;
    ++*grown;
  }
  return 0;
}

struct PqScope {  // every launch helper and the chunk-graph cache look at e->pq; off again on every way out
  miosqp_qp_engine *e;
  explicit PqScope(miosqp_qp_engine *e_) : e(e_) { e->pq = 1; }
  ~PqScope() { e->pq = 0; }
};

// fresh slots and trees, then the roots: bounds, costs and incumbents per instance; tree b's root is slot b (integer rows
// of l, u; x0, y0).  Records e->ev0 in front of the copies
int ls_upload_roots(const LsCall &a, LockstepStore &L) {
  miosqp_qp_engine *e = a.e;
  const size_t n = e->n, M = e->M, m = (size_t)e->d.m_orig, p = (size_t)e->d.n_int, B = (size_t)a.B;
  L.slots.reset(L.cap);
  L.trees.assign(B, miosqp::lockstep::Tree());
  const size_t tot = B * (2 * M + 2 * n + 2 * p + n + M);
  if (L.stage.size() < tot) L.stage.resize(tot);
  double *h_inc = L.stage.data(), *h_lo = h_inc + B * n, *h_hi = h_lo + B * p;
  for (size_t b = 0; b < B; b++) {
    const bool have = a.has_incumbent((int)b);
    if (have) memcpy(h_inc + b * n, a.x_inc0 + b * n, sizeof(double) * n);
    else memset(h_inc + b * n, 0, sizeof(double) * n);
    memcpy(h_lo + b * p, a.l + b * M + m, sizeof(double) * p);
    memcpy(h_hi + b * p, a.u + b * M + m, sizeof(double) * p);
    const int s = L.slots.take();  // == b: the free list is fresh
    L.trees[b].start(L.slots, s, have ? a.upper0[b] : miosqp::lockstep::NO_UPPER);
  }
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  // (the sources are the caller's arrays and this call's staging vector: pageable, so the copies are done when they return)
  HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_l), a.l, sizeof(double) * B * M, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_u), a.u, sizeof(double) * B * M, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.qraw), a.q, sizeof(double) * B * n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dev.inc, h_inc, sizeof(double) * B * n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dev.lo, h_lo, sizeof(double) * B * p, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dev.hi, h_hi, sizeof(double) * B * p, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dev.x, a.x0, sizeof(double) * B * n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dev.y, a.y0, sizeof(double) * B * M, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  // qbar_b = c D q_b, ONE launch per call: the bits solve_batch_q gives its columns every wave
  hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)((B * n + 255) / 256)), dim3(256), 0, e->stream, e->d, L.dev.qraw,
                     const_cast<double *>(L.dev.qs), a.B);
  return 0;
}

// `need` free slots (two child slots per column about to be sent): the store doubles until they are there.  Returns
// whether it grew -- a driver with per-slot arrays of its own then brings them to L.cap -- and MIOSQP_EFULL through *rc
bool ls_room(miosqp_qp_engine *e, LockstepStore &L, size_t need, int32_t *grown, int *rc) {
  bool grew = false;
  *rc = 0;
  while (L.slots.free_count() < need) {
    const int keep = L.cap;
    if ((*rc = lockstep_slots(e, L, 2 * L.cap, keep)) != 0) return grew;
    L.slots.grow(L.cap);
    ++*grown;
    grew = true;
  }
  return grew;
}

miosqp::lockstep::Record ls_record(const LsRec &g) {
  miosqp::lockstep::Record r;
  r.ok = g.status == MIOSQP_QP_SOLVED || g.status == MIOSQP_QP_MAX_ITER_REACHED;
  r.iter = g.iter;
  r.lower = g.lower;
  r.int_inf = g.int_inf;
  r.nextvar = g.nextvar;
  r.heur_feasible = g.hviol <= 0.0;
  r.heur_obj = g.hobj;
  return r;
}

// one wave of W columns whose five integers stand in L.h_trip: a wave wider than max_batch runs in slices, as
// solve_batch_q runs it; a 64-byte record per column comes back into L.h_rec
int ls_wave(miosqp_qp_engine *e, LockstepStore &L, int W) {
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M;
  const int big = (int)(n > M ? n : M);
  for (int s0 = 0; s0 < W; s0 += e->Bcap) {
    const int nb = W - s0 < e->Bcap ? W - s0 : e->Bcap;
    const int ntiles = (nb + 63) / 64;
    if (int rc = slice_begin(e, nb)) return rc;
    if (s0 == 0)  // the wave's one upload (behind slice_begin, as solve_slice queues its own)
      HIPCHK(hipMemcpyAsync(L.d_trip, L.h_trip, sizeof(int) * LS_TRIP * (size_t)W, hipMemcpyHostToDevice, e->stream));
    const int *trip = L.d_trip + LS_TRIP * s0;
    hipLaunchKernelGGL(kls_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb);
    const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
    if (int rc = slice_run(e, nb, e->st.max_iter, &roots)) return rc;
    hipLaunchKernelGGL(kls_scatter<0>, dim3((int)((n + 63) / 64 + (M + 63) / 64) + 1, ntiles), dim3(256), 0, e->stream, d, L.dev, trip,
                       L.d_rec + s0, nb);
  }
  HIPCHK(hipMemcpyAsync(L.h_rec, L.d_rec, sizeof(LsRec) * (size_t)W, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  return 0;
}

// `npairs` incumbents (tree, slot, rounded) from the pinned h_pairs into the trees' incumbent vectors.  The caller
// writes h_pairs only after the stream has been drained since the last push, so that copy is done by then
int ls_push_incumbents(miosqp_qp_engine *e, const Dev &d, const LsDev &dev, int *d_pairs, const int *h_pairs, int npairs) {
  if (npairs <= 0) return 0;
  HIPCHK(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 3 * (size_t)npairs, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(kls_incumbent<0>, dim3(npairs), dim3(256), 0, e->stream, d, dev, d_pairs, npairs);
  return 0;
}

void ls_stats_zero(miosqp_lockstep_stats *s) {
  s->waves = s->max_width = s->grown = 0;
  s->nodes = s->iters_slowest = s->iters_all = 0;
  s->device_time = s->run_time = s->host_time = 0.0;
}

// wave number `wave` of W columns; it_max / it_sum over the columns the wave waited for, `mean_over` of them
void ls_stats_wave(miosqp_lockstep_stats *s, int wave, int W, int it_max, int64_t it_sum, int mean_over) {
  s->nodes += W;
  s->max_width = W > s->max_width ? W : s->max_width;
  s->iters_slowest += it_max;
  s->iters_all += it_sum;
  if (wave <= s->wave_cap) {
    if (s->wave_width) s->wave_width[wave - 1] = W;
    if (s->wave_iter_max) s->wave_iter_max[wave - 1] = it_max;
    if (s->wave_iter_mean) s->wave_iter_mean[wave - 1] = (double)it_sum / mean_over;
  }
}

// the end of every driver: the incumbents come down, e->ev1 closes the call, info[], x_out and the times are filled
// (Stats: miosqp_lockstep_stats or miosqp_refill_stats).  A driver adds its own counters afterwards
template <class Stats>
int ls_finish(const LsCall &a, LockstepStore &L, double t0, double host_s, Stats *stats) {
  miosqp_qp_engine *e = a.e;
  const size_t n = e->n;
  const int B = a.B;
  double *h_inc = L.stage.data();
  HIPCHK(hipMemcpyAsync(h_inc, L.dev.inc, sizeof(double) * (size_t)B * n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  int64_t iters_total = 0;  // (absorbed nodes only: what info[b].osqp_iter sums to)
  for (int b = 0; b < B; b++) {
    const miosqp::lockstep::Tree &T = L.trees[(size_t)b];
    miosqp_tree_info &o = a.info[b];
    o.nodes = (int32_t)T.nodes;
    o.osqp_iter = (int32_t)T.iters;
    o.leaves_left = (int32_t)T.open.size();
    o.overflow = 0;
    o.max_leaves = (int32_t)T.max_open;
    o.found = T.found ? 1 : 0;
    o.upper_glob = T.upper;
    o.lower_glob = T.lower_glob(L.slots);
    o.device_time = 1e-3 * ms / B;
    o.run_time = wall_s / B;
    if (T.found || a.has_incumbent(b)) memcpy(a.x_out + (size_t)b * n, h_inc + (size_t)b * n, sizeof(double) * n);
    if (stats->finished_at) stats->finished_at[b] = T.finished_at;
    iters_total += T.iters;
  }
  stats->device_time = 1e-3 * ms;
  stats->run_time = wall_s;
  stats->host_time = host_s;
  e->loop_ms += ms;
  e->loop_iters += iters_total;
  return 0;
}

// ---- the wave loop of the plain, the round-and-fix and the strong-branching driver ----

// what a driver puts into ls_trees_run, a Step (a type parameter: the plain driver's per-column path stays inlined):
//   void grown(int cap)
//     the slot store has grown to `cap` slots
//   int verdict(int c, const int *tr, const LsRec &g, const Record &r, Tree &T, int wave, Verdict *v)
//     column c of the wave (tr: its five integers, g: its record, r: the same for the tree logic) at its tree T:
//     Tree::begin -- and Tree::end at once where nothing comes between -- and the verdict
//   int children(int W, int wave, double *host_s)
//     between the verdicts of a wave of W columns (L.branch holds who branches) and the next wave: whatever batch the
//     driver runs, then the children enter the lists (ls_children_enter).  *host_s: the host's own time is added

// branch_children, in the order of the wave
void ls_children_enter(const LsCall &a, LockstepStore &L, int W, int wave) {
  for (int c = 0; c < W; c++) {
    const int *tr = L.h_trip + LS_TRIP * c;
    miosqp::lockstep::Tree &T = L.trees[(size_t)tr[LS_TREE]];
    T.end(L.slots, tr[LS_SLOT], tr[LS_CHILD0], tr[LS_CHILD1], miosqp::lockstep::Verdict{L.branch[(size_t)c] != 0, 0});
    if (!T.can_continue(a.max_iter_bb)) T.finished_at = wave;
  }
}

// from the roots to info[]: per wave one node of every unfinished tree.  The host sends five integers per column and
// reads one 64-byte record per column back
template <class Step>
int ls_trees_run(const LsCall &a, LockstepStore &L, miosqp_lockstep_stats *stats, Step &step) {
  using miosqp::lockstep::Tree;
  using miosqp::lockstep::Verdict;
  miosqp_qp_engine *e = a.e;
  const int B = a.B;
  const double t0 = wall();
  PqScope scope(e);
  if (int rc = ls_upload_roots(a, L)) return rc;
  std::vector<int> live;
  live.reserve((size_t)B);
  double host_s = 0.0;  // choosing, absorbing, bookkeeping: the wall time between a wave's record and the next wave's launches
  for (;;) {
    double th = wall();
    live.clear();
    for (int b = 0; b < B; b++)
      if (L.trees[(size_t)b].can_continue(a.max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    const int W = (int)live.size();
    int rc = 0;
    if (ls_room(e, L, 2 * (size_t)W, &stats->grown, &rc)) step.grown(L.cap);
    if (rc) return rc;
    for (int c = 0; c < W; c++) {
      Tree &T = L.trees[(size_t)live[(size_t)c]];
      const int s = T.pop(L.slots, a.tree_explor_rule);
      int *tr = L.h_trip + LS_TRIP * c;
      tr[LS_TREE] = live[(size_t)c];
      tr[LS_SLOT] = s;
      tr[LS_WARM] = L.slots.warm_slot(s);
      tr[LS_CHILD0] = L.slots.take();
      tr[LS_CHILD1] = L.slots.take();
    }
    host_s += wall() - th;
    if ((rc = ls_wave(e, L, W)) != 0) return rc;
    // ---- bound_and_branch per tree on its column's record ----
    th = wall();
    const int wave = ++stats->waves;
    int it_max = 0, npairs = 0;
    int64_t it_sum = 0;
    L.branch.assign((size_t)W, 0);
    for (int c = 0; c < W; c++) {
      const LsRec &g = L.h_rec[c];
      const int *tr = L.h_trip + LS_TRIP * c;
      const int b = tr[LS_TREE];
      Tree &T = L.trees[(size_t)b];
      if (stats->node_hviol && T.nodes < stats->node_cap) stats->node_hviol[(size_t)b * stats->node_cap + T.nodes] = g.hviol;
      Verdict v{false, 0};
      if ((rc = step.verdict(c, tr, g, ls_record(g), T, wave, &v)) != 0) return rc;
      if (v.incumbent) {
        int *pr = L.h_pairs + 3 * npairs++;
        pr[0] = b;
        pr[1] = tr[LS_SLOT];
        pr[2] = v.incumbent == 2;
      }
      L.branch[(size_t)c] = v.branch;
      it_max = g.iter > it_max ? g.iter : it_max;
      it_sum += g.iter;
    }
    host_s += wall() - th;
    // (the pairs are next written after the next wave's drain)
    if ((rc = ls_push_incumbents(e, e->d, L.dev, L.d_pairs, L.h_pairs, npairs)) != 0) return rc;
    if ((rc = step.children(W, wave, &host_s)) != 0) return rc;
    ls_stats_wave(stats, wave, W, it_max, it_sum, W);
  }
  return ls_finish(a, L, t0, host_s, stats);
}

// ---- the plain driver: nothing between a node's verdict and its children ----
struct LsPlainStep {
  const LsCall &a;
  LockstepStore &L;
  LsPlainStep(const LsCall &a_, LockstepStore &L_) : a(a_), L(L_) {}
  void grown(int) {}
  int verdict(int, const int *tr, const LsRec &g, const miosqp::lockstep::Record &r, miosqp::lockstep::Tree &T, int wave,
              miosqp::lockstep::Verdict *v) {
    *v = T.absorb(L.slots, tr[LS_SLOT], tr[LS_CHILD0], tr[LS_CHILD1], r);
    if (v->branch && g.crossed) return ls_crossed(a, tr[LS_TREE]);
    if (!T.can_continue(a.max_iter_bb)) T.finished_at = wave;
    return 0;
  }
  int children(int, int, double *) { return 0; }
};

// ---- round and fix: one more batch per wave over all trees that fire ----
struct LsRfStep {
  const LsCall &a;
  LockstepStore &L;
  const int K, max_iter, every;
  miosqp_lockstep_rf_stats *rs;
  LsRfStep(const LsCall &a_, LockstepStore &L_, int K_, int max_iter_, int every_, miosqp_lockstep_rf_stats *rs_)
      : a(a_), L(L_), K(K_), max_iter(max_iter_), every(every_), rs(rs_) {}
  void grown(int) {}

  // up to the point where the children would enter the list; they enter after the heuristic batch
  int verdict(int c, const int *tr, const LsRec &g, const miosqp::lockstep::Record &r, miosqp::lockstep::Tree &T, int,
              miosqp::lockstep::Verdict *v) {
    const miosqp::lockstep::Begun bg = T.begin(L.slots, tr[LS_SLOT], r, every);
    *v = bg.v;
    if (v->branch && g.crossed) return ls_crossed(a, tr[LS_TREE]);
    if (bg.fire) L.fire.push_back(c);
    return 0;
  }

  // the K candidates of every tree that fires, ONE batch; then the children of the whole wave
  int children(int W, int wave, double *host_s) {
    miosqp_qp_engine *e = a.e;
    const Dev &d = e->d;
    const size_t n = e->n, M = e->M;
    const int F = (int)L.fire.size(), C = F * K;
    double th;
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
      *host_s += wall() - th;
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
        if (int rc = slice_run(e, nb, max_iter, &roots)) return rc;
        hipLaunchKernelGGL(kls_rf_keep<0>, dim3((int)((n + 63) / 64) + 1, ntiles), dim3(256), 0, e->stream, d, L.rf, trip, s0, nb, K, slice);
      }
      HIPCHK(hipMemcpyAsync(L.h_rf_rec, L.rf.rec, sizeof(LsRfGroup) * (size_t)F, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipEventRecord(L.rf_ev1, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipGetLastError());
      float rf_ms = 0;
      HIPCHK(hipEventElapsedTime(&rf_ms, L.rf_ev0, L.rf_ev1));
      rs->batches++;
      rs->columns += C;
      rs->device_time += 1e-3 * rf_ms;
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
    rs->iters_slowest += rf_it_max;
    ls_children_enter(a, L, W, wave);
    L.fire.clear();
    *host_s += wall() - th;
    if (nadopt > 0) {  // (behind kls_incumbent; the pinned list is next written after the next heuristic batch's drain)
      HIPCHK(hipMemcpyAsync(L.d_rf_adopt, L.h_rf_adopt, sizeof(int) * (size_t)nadopt, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_rf_incumbent<0>, dim3(nadopt), dim3(256), 0, e->stream, d, L.dev, L.rf, L.d_rf_adopt, nadopt);
    }
    return 0;
  }
};

}  // namespace

extern "C" {

int miosqp_qp_solve_trees_lockstep(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, double *x_out,
                                   miosqp_tree_info *info, miosqp_lockstep_stats *stats) {
  const LsCall a{"solve_trees_lockstep", e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info};
  if (!ls_args_ok(a) || !stats) return MIOSQP_EARG;
  ENTER(e);
  if (int rc = ls_refuse(a)) return rc;
  ls_stats_zero(stats);
  LockstepStore *L = nullptr;
  if (int rc = ls_open(a, B, &L, &stats->grown)) return rc;
  LsPlainStep step(a, *L);
  return ls_trees_run(a, *L, stats, step);
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
  // (what the two entries share speaks as the plain entry)
  const LsCall a{"solve_trees_lockstep", e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info};
  if (!ls_args_ok(a) || !stats) return MIOSQP_EARG;
  ENTER(e);
  if (int rc = ls_refuse(a)) return rc;
  ls_stats_zero(stats);
  LockstepStore *Lp = nullptr;
  if (int rc = ls_open(a, B, &Lp, &stats->grown)) return rc;
  LockstepStore &L = *Lp;
  if (int rc = lockstep_rf_reserve(e, L, B, rf_candidates)) return rc;
  rf_stats->batches = 0;
  rf_stats->columns = rf_stats->iters_slowest = 0;
  rf_stats->device_time = 0.0;
  L.fire.clear();  // (a call that ended in an error between begin and end may have left some)
  LsRfStep step(a, L, rf_candidates, rf_max_iter, rf_every, rf_stats);
  if (int rc = ls_trees_run(a, L, stats, step)) return rc;
  for (int b = 0; b < B; b++) {
    const miosqp::lockstep::Tree &T = L.trees[(size_t)b];
    if (rf_stats->calls) rf_stats->calls[b] = (int32_t)T.rf_calls;
    if (rf_stats->candidates) rf_stats->candidates[b] = (int32_t)T.rf_candidates;
    if (rf_stats->feasible) rf_stats->feasible[b] = (int32_t)T.rf_feasible;
    if (rf_stats->improved) rf_stats->improved[b] = (int32_t)T.rf_improved;
    if (rf_stats->iters) rf_stats->iters[b] = T.rf_iters;
  }
  return 0;
}

}  // extern "C"
