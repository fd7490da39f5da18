// part of engine.hip (included there, not compiled alone; the LAST file of the translation unit): B branch-and-bound trees on
// columns that are refilled between chunks (C ABI miosqp_qp_solve_trees_refill).  The trees, slots, roots and costs are the
// lock-step driver's (host_lockstep.inc, lockstep_trees.hpp); the wave is gone: a column holds one node of one tree, and
// at every chunk boundary the columns the test decided are harvested, absorbed by their trees and loaded again with the next
// leaf of a tree that has no node in flight (lockstep_refill.hpp).  Per boundary ONE download (the list of harvested columns
// and their 64-byte records, behind a 64-byte head) and ONE synchronisation, then ONE upload (six integers per filled column
// and the incumbent pairs); no vector crosses PCIe between the roots going up and the incumbents coming down.
namespace {

struct RefillCols {
  int *d_ints = nullptr;   // one device allocation: the per-column arrays | t_fill | t_has | head | list | rec | fills | pairs
  int *h_down = nullptr;   // pinned: head | list | rec
  int *h_up = nullptr;     // pinned: fills | pairs
  int *d_up = nullptr;
  int *c_start = nullptr, *c_harv = nullptr, *t_has = nullptr;
  int Bs = 0;
  RfDev dev{};
  miosqp::lockstep::Refill sched;
  std::vector<miosqp::lockstep::Fill> fills;
};

void refill_free(void *p) {
  RefillCols *R = static_cast<RefillCols *>(p);
  if (!R) return;
  if (R->d_ints) hipFree(R->d_ints);
  if (R->h_down) hipHostFree(R->h_down);
  if (R->h_up) hipHostFree(R->h_up);
  delete R;
}

// the column arrays, once per engine (Bs is fixed from the first batched call on)
int refill_reserve(miosqp_qp_engine *e, RefillCols &R) {
  if (R.Bs) return 0;  // (set last: a call that failed half-way starts over)
  if (R.d_ints) hipFree(R.d_ints);
  if (R.h_down) hipHostFree(R.h_down);
  if (R.h_up) hipHostFree(R.h_up);
  R.d_ints = R.h_down = R.h_up = nullptr;
  const size_t Bs = (size_t)e->d.Bs;
  // ints: c_trip 5 | c_slot | c_tree | c_ident | c_busy | c_fill | c_start | c_harv  (12 Bs) | t_fill 16 | t_has 16 | pad to 64
  //       | head 16 | list Bs | rec 16 Bs | fills 6 Bs | pairs 3 Bs
  const size_t cols = 12 * Bs + 64, down = 16 + Bs + 16 * Bs, up = (RF_FILL + 3) * Bs;
  if (hipMalloc((void **)&R.d_ints, (cols + down + up) * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    R.d_ints = nullptr;
    g_err = "solve_trees_refill: no device memory for the columns";
    return MIOSQP_EFULL;
  }
  HIPCHK(hipMemsetAsync(R.d_ints, 0, (cols + down + up) * sizeof(int), e->stream));
  HIPCHK(hipHostMalloc((void **)&R.h_down, down * sizeof(int), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&R.h_up, up * sizeof(int), hipHostMallocDefault));
  int *p = R.d_ints;
  R.dev.c_trip = p; p += LS_TRIP * Bs;
  R.dev.c_slot = p; p += Bs;
  R.dev.c_tree = p; p += Bs;
  R.dev.c_ident = p; p += Bs;
  R.dev.c_busy = p; p += Bs;
  R.dev.c_fill = p; p += Bs;
  R.c_start = p; p += Bs;
  R.c_harv = p; p += Bs;
  R.dev.t_fill = p; p += 16;
  R.t_has = p; p += 16;
  p += 32;
  R.dev.head = reinterpret_cast<RfHead *>(p); p += 16;
  R.dev.list = p; p += Bs;
  R.dev.rec = reinterpret_cast<LsRec *>(p); p += 16 * Bs;  // (64-byte aligned: every block before it is a multiple of 16 ints)
  R.d_up = p;
  R.Bs = (int)Bs;
  return 0;
}

// the engine's Dev with the streaming test on this driver's column arrays (what the chunk graphs of this mode hold)
Dev refill_dev(const miosqp_qp_engine *e, const RefillCols &R) {
  Dev d = e->d;
  d.stream = 1;
  d.max_iter_s = e->st.max_iter;
  d.c_start = R.c_start;
  d.c_harv = R.c_harv;
  d.t_has = R.t_has;
  return d;
}

// capture_chunk_b with the streaming test: check_termination iterations, the test, the decision per column
int capture_chunk_refill(miosqp_qp_engine *e, const Dev &d, int ntiles) {
  hipGraph_t *g = &e->gr_full[ntiles - 1];
  hipGraphExec_t *x = &e->xr_full[ntiles - 1];
  std::lock_guard<std::mutex> capture_lock(g_capture_mutex);
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  e->in_capture = true;
  if (kbp_here(e, ntiles)) {
    launch_kbp(e, d, ntiles, e->chunk);
  } else {
    hipLaunchKernelGGL(kb_tick, dim3(1), dim3(1), 0, e->stream, d, e->chunk);
    for (int i = 0; i < e->chunk; i++) launch_iteration_b(e, ntiles);
  }
  if (e->fold && e->bd_cfg == 0) {
    const int ncol = ntiles * (64 / BM_COLS);
    hipLaunchKernelGGL(kbm_check_con, dim3(bm_grid((d.M + 15) / 16, ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
    hipLaunchKernelGGL(kbm_check_var, dim3(bm_grid(2 * ((d.n + 15) / 16), ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
  } else {
    hipLaunchKernelGGL(kb_check_con, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
    hipLaunchKernelGGL(kb_check_var, dim3(2 * ((d.n + 3) / 4), ntiles), dim3(256), 0, e->stream, d);
  }
  hipLaunchKernelGGL(kb_check_reduce<true>, dim3(ntiles, KR), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_check_decide, dim3(ntiles), dim3(256), 0, e->stream, d);
  e->in_capture = false;
  HIPCHK(hipStreamEndCapture(e->stream, g));
  HIPCHK(hipGraphInstantiate(x, *g, nullptr, nullptr, 0));
  return 0;
}

}  // namespace

extern "C" {

int miosqp_qp_solve_trees_refill(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                 const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                 int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, double *x_out,
                                 miosqp_tree_info *info, miosqp_refill_stats *stats) {
  using miosqp::lockstep::Fill;
  using miosqp::lockstep::Record;
  using miosqp::lockstep::Tree;
  using miosqp::lockstep::Verdict;
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || !stats || max_iter_bb < 1 ||
      tree_explor_rule < 0 || tree_explor_rule > 3 || capacity < 0)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = "solve_trees_refill: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending) {
    g_err = "solve_trees_refill: streaming chunks are still in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  if (e->st.max_iter % e->chunk != 0) {
    g_err = "solve_trees_refill: a column counts its own chunks: max_iter must be a multiple of check_termination";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M, m = (size_t)e->d.m_orig, p = (size_t)e->d.n_int;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) {  // (nothing has been queued)
      g_err = "solve_trees_refill: l > u in the root of instance " + std::to_string(k / M);
      return MIOSQP_EBOUNDS;
    }
  stats->chunks = stats->columns = stats->grown = 0;
  stats->nodes = stats->iters_all = stats->col_chunks_busy = stats->col_chunks_total = 0;
  stats->device_time = stats->run_time = stats->host_time = stats->chunk_time = 0.0;
  stats->nodes_max_iter = stats->iters_max_iter = 0;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  if (!e->lockstep) e->lockstep = new LockstepStore();
  LockstepStore &L = *static_cast<LockstepStore *>(e->lockstep);
  if (!L.refill) L.refill = new RefillCols();
  RefillCols &R = *static_cast<RefillCols *>(L.refill);
  if (int rc = lockstep_reserve(e, L, B)) return rc;
  if (int rc = refill_reserve(e, R)) return rc;
  {
    // the slot store as miosqp_qp_solve_trees_lockstep sizes it
    const int want = capacity > 0 ? std::max(capacity, 4) : std::max(64, 4 * B);
    if (!L.slot_block || (capacity > 0 ? L.cap != want : L.cap < want))
      if (int rc = lockstep_slots(e, L, want, 0)) return rc;
    while (L.cap < B) {
      if (int rc = lockstep_slots(e, L, 2 * L.cap, 0)) return rc;
      stats->grown++;
    }
  }
  const int C = B < e->Bcap ? B : e->Bcap, ntiles = (C + 63) / 64;
  stats->columns = C;
  e->pool_dirty = true;  // (the columns are ours now: as slice_begin marks them)
  if (int rcj = maybe_rejoin_kbp(e, 8)) return rcj;
  const double t0 = wall();
  struct PqScope {  // every launch helper looks at e->pq; off again on every way out
    miosqp_qp_engine *e;
    explicit PqScope(miosqp_qp_engine *e_) : e(e_) { e->pq = 1; }
    ~PqScope() { e->pq = 0; }
  } scope(e);
  const Dev ds = refill_dev(e, R);
  RfDev rf = R.dev;
  rf.C = C;
  if (!e->xr_full[ntiles - 1])
    if (int rc = capture_chunk_refill(e, ds, ntiles)) return rc;
  L.slots.reset(L.cap);
  L.trees.assign((size_t)B, Tree());
  R.sched.reset(C, B);
  // ---- the roots, exactly as the lock-step driver stores them: tree b's root is slot b ----
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
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_l), l, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.root_u), u, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<double *>(L.dev.qraw), q, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.inc, h_inc, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.lo, h_lo, sizeof(double) * (size_t)B * p, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.hi, h_hi, sizeof(double) * (size_t)B * p, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.x, x0, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dev.y, y0, sizeof(double) * (size_t)B * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, e->d, L.dev.qraw,
                       const_cast<double *>(L.dev.qs), B);
  }
  // ---- the columns: all decided and idle, the working vectors zero (what a wave gives its padding) ----
  const int big = (int)(n > M ? n : M);
  hipLaunchKernelGGL(kb_reset, dim3((ds.Bs + 255) / 256), dim3(256), 0, e->stream, ds, 0);
  hipLaunchKernelGGL(kb_prepare<true>, dim3((big + 3) / 4, ntiles), dim3(256), 0, e->stream, ds, 0);
  hipLaunchKernelGGL(kb_warm_z, dim3((ds.M + 3) / 4, ntiles), dim3(256), 0, e->stream, ds);
  hipLaunchKernelGGL(kls_cols_reset<0>, dim3((ds.Bs + 255) / 256), dim3(256), 0, e->stream, ds, rf);
  int64_t iters_total = 0;
  int epoch = 0, chunk_no = 0;
  double host_s = 0.0, chunk_ms = 0.0;
  int *h_fills = R.h_up, *h_pairs = R.h_up + RF_FILL * (size_t)R.Bs;
  int *d_fills = R.d_up, *d_pairs = R.d_up + RF_FILL * (size_t)R.Bs;
  const RfHead *h_head = reinterpret_cast<const RfHead *>(R.h_down);
  const int *h_list = R.h_down + 16;
  const LsRec *h_rec = reinterpret_cast<const LsRec *>(R.h_down + 16 + R.Bs);
  int npairs = 0;
  for (;;) {
    // ---- fill the free columns (at the first pass: all of them) and send the boundary's one upload ----
    double th = wall();
    const int want = R.sched.fillable(L.trees, max_iter_bb);
    while (L.slots.free_count() < 2 * (size_t)want) {  // two child slots per filled column
      const int keep = L.cap;
      if (int rc = lockstep_slots(e, L, 2 * L.cap, keep)) return rc;
      L.slots.grow(L.cap);
      stats->grown++;
    }
    R.fills.clear();
    const int nfill = R.sched.fill(L.slots, L.trees, tree_explor_rule, max_iter_bb, R.fills);
    for (int k = 0; k < nfill; k++) {
      const Fill &f = R.fills[(size_t)k];
      int *w = h_fills + RF_FILL * k;
      w[0] = f.col; w[1] = f.tree; w[2] = f.slot; w[3] = f.warm; w[4] = f.child0; w[5] = f.child1;
    }
    host_s += wall() - th;
    // (the pinned block was last read by the upload of the boundary before: the drain since then covers it)
    if (npairs > 0) {
      HIPCHK(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 3 * (size_t)npairs, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_incumbent<0>, dim3(npairs), dim3(256), 0, e->stream, ds, L.dev, d_pairs, npairs);
      npairs = 0;
    }
    if (nfill > 0) {
      epoch++;
      HIPCHK(hipMemcpyAsync(d_fills, h_fills, sizeof(int) * RF_FILL * (size_t)nfill, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_refill<0>, dim3((int)((n + 63) / 64 + (M + 63) / 64) + 1, (nfill + 63) / 64), dim3(256), 0, e->stream, ds,
                         L.dev, rf, d_fills, nfill, epoch);
      hipLaunchKernelGGL(kls_refill_z<0>, dim3((ds.M + 3) / 4, ntiles), dim3(256), 0, e->stream, ds, rf, epoch);
    }
    if (R.sched.busy == 0) break;  // nothing in flight and nothing could be filled: every tree is done
    // ---- one chunk, then the boundary: harvest, masked epilogue, scatter + children + records, the one download ----
    const int busy = R.sched.busy;
    HIPCHK(hipEventRecord(e->evc0, e->stream));
    {
      ChipGuard turn(e);  // (the captured chunk may hold a whole-chip launch)
      HIPCHK(hipGraphLaunch(e->xr_full[ntiles - 1], e->stream));
    }
    HIPCHK(hipEventRecord(e->evc1, e->stream));
    {
      Dev df = ds, dh = ds, dq = ds;  // the epilogue kernels find slot / column / tree through c_node
      df.c_node = rf.c_slot;
      df.pl_lo = L.dev.lo;
      df.pl_hi = L.dev.hi;
      dh.c_node = rf.c_ident;
      dq.c_node = rf.c_tree;
      dq.b_qraw = const_cast<double *>(L.dev.qraw);
      const LsRoots roots{L.dev.root_l, L.dev.root_u, rf.c_trip, ds.Bs};
      hipLaunchKernelGGL(kls_harvest<0>, dim3(1), dim3(1024), 0, e->stream, ds, rf);
      hipLaunchKernelGGL(kb_finish, dim3(ntiles), dim3(1024), 0, e->stream, df, 0);
      hipLaunchKernelGGL(kls_heur_rows<1>, dim3((ds.M + 3) / 4, ntiles), dim3(256), 0, e->stream, dh, roots);
      hipLaunchKernelGGL(kb_obj_rows<true>, dim3((ds.n + 3) / 4, ntiles), dim3(256), 0, e->stream, dq);
      hipLaunchKernelGGL(kb_obj_sum, dim3(ntiles), dim3(1024), 0, e->stream, ds);
      hipLaunchKernelGGL(kls_scatter_cols<0>, dim3((int)((n + 63) / 64 + (M + 63) / 64) + 1, ntiles), dim3(256), 0, e->stream, ds, L.dev,
                         rf);
    }
    HIPCHK(hipMemcpyAsync(R.h_down, rf.head, sizeof(int) * (16 + (size_t)R.Bs) + sizeof(LsRec) * (size_t)C, hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    if (h_head->pad) {
      if (h_head->pad != 1) {
        g_err = "batched persistent sweeps: a group barrier timed out, stage " + std::to_string(h_head->pad);
        return MIOSQP_EHIP;
      }
      // the chunk's persistent launch was called off before anything was modified (the test decided nothing, nothing was
      // harvested): this chunk again, as launches.  kbp_leave drops every captured chunk, ours included, and clears pad.
      if (int rc = kbp_leave(e)) return rc;
      if (int rc = capture_chunk_refill(e, ds, ntiles)) return rc;
      continue;  // (nothing to fill: the loop comes straight back to the chunk)
    }
    {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e->evc0, e->evc1));
      chunk_ms += ms;
      e->bloop_ms += ms;
      e->bloop_iters += e->chunk;
      e->bloop_node_iters += (int64_t)e->chunk * busy;
    }
    chunk_no++;
    stats->col_chunks_busy += busy;
    stats->col_chunks_total += C;
    if (stats->chunk_busy && chunk_no <= stats->chunk_cap) stats->chunk_busy[chunk_no - 1] = busy;
    // ---- bound_and_branch per harvested column on its record ----
    th = wall();
    const int count = h_head->count;
    for (int k = 0; k < count; k++) {
      const int c = h_list[k];
      const LsRec &g = h_rec[c];
      Record r;
      r.ok = g.status == MIOSQP_QP_SOLVED || g.status == MIOSQP_QP_MAX_ITER_REACHED;
      r.iter = g.iter;
      r.lower = g.lower;
      r.int_inf = g.int_inf;
      r.nextvar = g.nextvar;
      r.heur_feasible = g.hviol <= 0.0;
      r.heur_obj = g.hobj;
      int b = -1, slot = -1;
      const Verdict v = R.sched.absorb(L.slots, L.trees, c, r, &b, &slot);
      if (v.branch && g.crossed) {
        g_err = "solve_trees_refill: branching produced l > u (instance " + std::to_string(b) + ")";
        return MIOSQP_EBOUNDS;
      }
      if (v.incumbent) {
        int *pr = h_pairs + 3 * npairs++;
        pr[0] = b;
        pr[1] = slot;
        pr[2] = v.incumbent == 2;
      }
      if (!L.trees[(size_t)b].can_continue(max_iter_bb)) L.trees[(size_t)b].finished_at = chunk_no;
      iters_total += g.iter;
      if (g.status == MIOSQP_QP_MAX_ITER_REACHED) {
        stats->nodes_max_iter++;
        stats->iters_max_iter += g.iter;
      }
    }
    stats->nodes += count;
    host_s += wall() - th;
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
  }
  stats->chunks = chunk_no;
  stats->iters_all = iters_total;
  stats->device_time = 1e-3 * ms;
  stats->run_time = wall_s;
  stats->host_time = host_s;
  stats->chunk_time = 1e-3 * chunk_ms;
  e->loop_ms += ms;
  e->loop_iters += iters_total;
  return 0;
}

}  // extern "C"
