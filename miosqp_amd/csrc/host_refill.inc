// part of engine.hip (included there, not compiled alone; behind host_lockstep.inc, whose pieces it uses): B branch-and-bound trees on
// columns that are refilled between chunks (C ABI miosqp_qp_solve_trees_refill).  The trees, slots, roots and costs are the
// lock-step driver's (host_lockstep.inc, lockstep_trees.hpp); the wave is gone: a column holds one node of one tree, and
// at every chunk boundary the columns the test decided are harvested, absorbed by their trees and loaded again with the next
// leaf of a tree that has no node in flight (lockstep_refill.hpp).  Per boundary ONE download (the list of harvested columns
// and their 64-byte records, behind a 64-byte head) and ONE synchronisation, then ONE upload (six integers per filled column
// and the incumbent pairs); no vector crosses PCIe between the roots going up and the incumbents coming down.
//
// This file owns the column arrays, the chunk's capture and the chunk loop with its statistics; checks, store, roots,
// slot growth, the record's conversion, the incumbent push and the end of the call are the pieces of host_lockstep.inc.
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

// the plain driver's call (the pieces of host_lockstep.inc) around a chunk loop instead of a wave loop
int miosqp_qp_solve_trees_refill(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                 const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                 int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, double *x_out,
                                 miosqp_tree_info *info, miosqp_refill_stats *stats) {
  using miosqp::lockstep::Fill;
  using miosqp::lockstep::Verdict;
  const LsCall a{"solve_trees_refill", e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info};
  if (!ls_args_ok(a) || !stats) return MIOSQP_EARG;
  ENTER(e);
  if (int rc = ls_refuse(a, e->st.max_iter % e->chunk != 0
                                ? "a column counts its own chunks: max_iter must be a multiple of check_termination"
                                : nullptr))
    return rc;
  stats->chunks = stats->columns = stats->grown = 0;
  stats->nodes = stats->iters_all = stats->col_chunks_busy = stats->col_chunks_total = 0;
  stats->device_time = stats->run_time = stats->host_time = stats->chunk_time = 0.0;
  stats->nodes_max_iter = stats->iters_max_iter = 0;
  LockstepStore *Lp = nullptr;
  if (int rc = ls_open(a, B, &Lp, &stats->grown)) return rc;
  LockstepStore &L = *Lp;
  if (!L.refill) L.refill = new RefillCols();
  RefillCols &R = *static_cast<RefillCols *>(L.refill);
  if (int rc = refill_reserve(e, R)) return rc;
  const size_t n = e->n, M = e->M;
  const int C = B < e->Bcap ? B : e->Bcap, ntiles = (C + 63) / 64;
  stats->columns = C;
  e->pool_dirty = true;  // (the columns are ours now: as slice_begin marks them)
  if (int rcj = maybe_rejoin_kbp(e, 8)) return rcj;
  const double t0 = wall();
  PqScope scope(e);
  const Dev ds = refill_dev(e, R);
  RfDev rf = R.dev;
  rf.C = C;
  if (!e->xr_full[ntiles - 1])
    if (int rc = capture_chunk_refill(e, ds, ntiles)) return rc;
  R.sched.reset(C, B);
  if (int rc = ls_upload_roots(a, L)) return rc;
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
    int rc = 0;
    ls_room(e, L, 2 * (size_t)want, &stats->grown, &rc);  // two child slots per filled column
    if (rc) return rc;
    R.fills.clear();
    const int nfill = R.sched.fill(L.slots, L.trees, tree_explor_rule, max_iter_bb, R.fills);
    for (int k = 0; k < nfill; k++) {
      const Fill &f = R.fills[(size_t)k];
      int *w = h_fills + RF_FILL * k;
      w[0] = f.col; w[1] = f.tree; w[2] = f.slot; w[3] = f.warm; w[4] = f.child0; w[5] = f.child1;
    }
    host_s += wall() - th;
    // (the pinned block was last read by the upload of the boundary before: the drain since then covers it)
    if ((rc = ls_push_incumbents(e, ds, L.dev, d_pairs, h_pairs, npairs)) != 0) return rc;
    npairs = 0;
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
      if ((rc = kbp_leave(e)) != 0) return rc;
      if ((rc = capture_chunk_refill(e, ds, ntiles)) != 0) return rc;
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
      int b = -1, slot = -1;
      const Verdict v = R.sched.absorb(L.slots, L.trees, c, ls_record(g), &b, &slot);
      if (v.branch && g.crossed) return ls_crossed(a, b);
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
  if (int rc = ls_finish(a, L, t0, host_s, stats)) return rc;
  stats->chunks = chunk_no;
  stats->iters_all = iters_total;
  stats->chunk_time = 1e-3 * chunk_ms;
  return 0;
}

}  // extern "C"
