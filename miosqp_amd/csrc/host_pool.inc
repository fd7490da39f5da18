// part of engine.hip (included there, not compiled alone): host side of the leaf pool / streaming batch (kernels_pool.inc)
namespace {

// one streaming chunk: refill -> check_termination iterations -> test -> harvest
// part: 0 = everything; 1 = what precedes the iterations, 2 = what follows them (the iterations are a persistent
// whole-chip launch that the caller issues between the two, in its turn: pool_launch on a shared chip)
void enqueue_stream_chunk(miosqp_qp_engine *e, int part = 0) {
  // streaming semantics (per-column iteration counts, no "all decided" flag) are a property of THESE launches
  // only: the engine's own Dev keeps stream = 0, so solve_batch on the same engine is unchanged
  Dev d = e->d;
  d.stream = 1;
  const Dev &h = e->dh;  // the harvest tile
  const int ntiles = e->Bcap / 64;
  const int big = e->n > e->M ? e->n : e->M;
  if (part != 2) {
    hipLaunchKernelGGL(kp_assign, dim3(1), dim3(1024), 0, e->stream, d);
    hipLaunchKernelGGL(kp_prepare, dim3((big + 3) / 4), dim3(256), 0, e->stream, d);
    hipLaunchKernelGGL(kp_warm_z, dim3(d.M), dim3(256), 0, e->stream, d);
  }
  if (part == 1) return;
  if (part == 0) {
    if (kbp_here(e, ntiles)) {
      launch_kbp(e, d, ntiles, e->chunk);
    } else {
      hipLaunchKernelGGL(kb_tick, dim3(1), dim3(1), 0, e->stream, d, e->chunk);
      for (int i = 0; i < e->chunk; i++) launch_iteration_b(e, ntiles);
    }
  }
  if (e->fold && e->bd_cfg == 0) {
    const int ncol = ntiles * (64 / BM_COLS);
    hipLaunchKernelGGL(kbm_check_con, dim3(bm_grid((d.M + 15) / 16, ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
    hipLaunchKernelGGL(kbm_check_var, dim3(bm_grid(2 * ((d.n + 15) / 16), ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
  } else {
    hipLaunchKernelGGL(kb_check_con, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
    hipLaunchKernelGGL(kb_check_var, dim3(2 * ((d.n + 3) / 4), ntiles), dim3(256), 0, e->stream, d);
  }
  hipLaunchKernelGGL(kb_check_reduce<false>, dim3(ntiles, KR), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_check_decide, dim3(ntiles), dim3(256), 0, e->stream, d);
  // harvest: the decided columns, gathered into one tile
  hipLaunchKernelGGL(kp_harvest, dim3((big + 3) / 4), dim3(256), 0, e->stream, d, h);
  if (e->fold && e->bd_cfg == 0 && !getenv("MIOSQP_POOL_SPARSE_ROWS"))
    hipLaunchKernelGGL(kh_rows_mfma, dim3(2 * ((d.M + 15) / 16) + 2 * ((d.n + 15) / 16) + 1), dim3(512), 0, e->stream, h);
  else
    hipLaunchKernelGGL(kh_rows_digest, dim3(d.M + d.n + 1), dim3(256), 0, e->stream, h);
  hipLaunchKernelGGL(kh_sums, dim3(32), dim3(256), 0, e->stream, h);
  hipLaunchKernelGGL(kp_commit, dim3((big + 3) / 4), dim3(256), 0, e->stream, d, h);
  hipLaunchKernelGGL(kp_release, dim3(1), dim3(64), 0, e->stream, d);
}

// ... captured once into a graph (one host call per chunk)
int capture_stream_chunk(miosqp_qp_engine *e, int part = 0) {
  hipGraph_t *g = part == 0 ? &e->g_stream : part == 1 ? &e->g_stream_a : &e->g_stream_b;
  hipGraphExec_t *x = part == 0 ? &e->x_stream : part == 1 ? &e->x_stream_a : &e->x_stream_b;
  std::lock_guard<std::mutex> capture_lock(g_capture_mutex);
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  e->in_capture = true;
  enqueue_stream_chunk(e, part);
  e->in_capture = false;
  HIPCHK(hipStreamEndCapture(e->stream, g));
  HIPCHK(hipGraphInstantiate(x, *g, nullptr, nullptr, 0));
  return 0;
}

void drop_stream_graph(miosqp_qp_engine *e) {
  for (hipGraphExec_t *x : {&e->x_stream, &e->x_stream_a, &e->x_stream_b}) {
    if (*x) hipGraphExecDestroy(*x);
    *x = nullptr;
  }
  for (hipGraph_t *g : {&e->g_stream, &e->g_stream_a, &e->g_stream_b}) {
    if (*g) hipGraphDestroy(*g);
    *g = nullptr;
  }
}

// the stream as ONE persistent launch (kernels_bstream.inc): built for this pool, and the persistent sweeps are on (a
// launch that was called off sends the engine to the launches: kbp_leave / maybe_rejoin_kbp)
bool kbs_here(const miosqp_qp_engine *e) { return e->kbs && kbp_here(e, e->Bcap / 64) && e->Bcap <= KBP_G * BM_COLS; }

// `chunks` chunks of the stream in one launch + the one-thread kernel that mirrors the pool's counters (kp_release's part)
void launch_kbs(miosqp_qp_engine *e, int chunks) {
  // (byte copies of the engine's own objects: a struct assignment need not carry the padding, and the block below is
  //  compared bytewise with the one last sent)
  Dev d;
  memcpy(&d, &e->d, sizeof d);
  d.stream = 1;
  if (e->kbs_fault_at > 0 && e->kbs_launches + 1 == e->kbs_fault_at) d.coop_dbg |= 64;  // (fault injection, tests)
  KbsArgs ka;
  memcpy(&ka, &e->kbsa, sizeof ka);
  ka.reg = e->kbpa.reg;
  ka.bar = e->kbpa.bar;
  ka.ncol = (e->Bcap / 64) * (64 / BM_COLS);
  ka.nchunks = chunks;
  ka.iters = e->chunk;
  ka.prof = e->kbs_prof;
  __atomic_store_n(&e->h_pctl[0].pad[0], 0, __ATOMIC_RELEASE);  // (a new launch: the host wants work done)
  {
    // the boundary's copy of the arguments (device memory): sent again only when something in it changed
    KbsBlock now;
    memset(&now, 0, sizeof now);
    memcpy(&now.d, &d, sizeof d);
    memcpy(&now.ka, &ka, sizeof ka);
    if (memcmp(&now, &e->kbs_blk_host, sizeof now) != 0) {
      (void)hipStreamSynchronize(e->stream);
      (void)hipMemcpy(e->kbs_blk, &now, sizeof now, hipMemcpyHostToDevice);
      memcpy(&e->kbs_blk_host, &now, sizeof now);
    }
  }
  {
    ChipGuard turn(e);
    hipLaunchKernelGGL(kbs, dim3(KBP_WGS), dim3(512), KBP_LDS_DOUBLES * sizeof(double), e->stream, d, ka, (const KbsBlock *)e->kbs_blk);
  }
  hipLaunchKernelGGL(kbs_finish, dim3(1), dim3(64), 0, e->stream, d, ka, e->pool_chunk_total + (unsigned long long)chunks);
}

// the launches in flight leave at their next chunk boundary once their groups hold nothing (the host is done with the instance)
void kbs_stop(miosqp_qp_engine *e) {
  if (e->kbs && e->h_pctl) __atomic_store_n(&e->h_pctl[0].pad[0], 1, __ATOMIC_RELEASE);
}

// slot copies while a persistent launch may be running: on a stream of their own (the engine's stream is busy for
// milliseconds; a slot the host may touch is not touched by the launch: its digest has been absorbed / it has not been pushed)
hipStream_t slot_stream(miosqp_qp_engine *e) {
  if (!e->kbs || e->pool_pending == 0) return e->stream;
  if (!e->side && hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess) e->side = nullptr;
  return e->side ? e->side : e->stream;
}

}  // namespace

extern "C" {

int miosqp_qp_pool_create(miosqp_qp_engine *e, int32_t capacity, int32_t columns) {
  if (!e || capacity < 2 || columns < 1) return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest) {
    g_err = "pool_create: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->node_cap) {
    g_err = "pool_create: the pool exists already";
    return MIOSQP_EARG;
  }
  if (e->st.max_iter % e->chunk != 0) {
    g_err = "pool_create: the streaming batch needs max_iter to be a multiple of check_termination";
    return MIOSQP_EARG;
  }
  if (columns > 1024) columns = 1024;
  if (e->Bcap == 0) {
    int rc = alloc_batch(e, columns);
    if (rc) return rc;
  }
  Dev &d = e->d;
  const size_t n = e->n, M = e->M, p = d.n_int > 0 ? d.n_int : 1, cap = capacity;
  const int ring = 8192;
  {
    int rc0 = pool_reserve(e, cap * (n + M + 2 * p + 1) * 8 + (size_t)d.Bs * 64 + (size_t)PT * (10 * n + 5 * M + 600) * 8 + ((size_t)1 << 16));
    if (rc0) return rc0;
  }
#define ALP(field, count)                            \
  do {                                               \
    int rc__ = dalloc(e, &d.field, (size_t)(count)); \
    if (rc__) return rc__;                           \
  } while (0)
  ALP(pl_lo, cap * p); ALP(pl_hi, cap * p); ALP(pl_ws, cap); ALP(sol_x, cap * n); ALP(sol_y, cap * M);
  ALP(c_start, d.Bs); ALP(c_child0, d.Bs); ALP(c_child1, d.Bs);
  ALP(fmap, PT); ALP(hmap, PT); ALP(lt_x, n * PT);
  ALP(pctl, 1);
  // the harvest tile: a Dev of its own (64 columns) on which the epilogue kernels run
  Dev &h = e->dh;
  h = d;
  h.Bs = PT;
  h.stream = 1;
  {
    Dev &d = h;  // the macro writes into `d`
    ALP(b_x, n * PT); ALP(b_dx, n * PT); ALP(b_y, M * PT); ALP(b_dy, M * PT);
    ALP(b_xfin, n * PT); ALP(b_yfin, M * PT); ALP(b_xi, n * PT); ALP(b_xis, (n + 16) * PT); ALP(b_xfs, (n + 16) * PT);
    ALP(b_sm, M * PT); ALP(b_sn, 2 * n * PT); ALP(b_part, (128 + 3 * 128) * PT);
    ALP(c_status, PT); ALP(c_iter, PT); ALP(c_node, PT); ALP(c_child0, PT); ALP(c_child1, PT); ALP(c_done, PT);
    ALP(c_intinf, PT); ALP(c_nextvar, PT); ALP(c_lower, PT); ALP(c_hobj, PT); ALP(c_hviol, PT); ALP(c_pri, PT);
    ALP(c_dua, PT); ALP(c_harv, PT); ALP(t_has, 2);
  }
  // the stream as one persistent launch: partial results of the members, assignment tables, per-group counters, two more
  // right-hand arrays (kernels_bstream.inc)
  e->kbs = false;
  if (e->kbp_capable && d.Bs <= KBP_G * BM_COLS && e->fold && e->bd_cfg == 0 && d.digest &&
      !(getenv("MIOSQP_KBS") && atoi(getenv("MIOSQP_KBS")) == 0)) {
    ALP(b_xfs, n * (size_t)d.Bs);
    {
      int rc = dalloc(e, &e->kbsa.part, (size_t)KBP_G * KBP_MEMBERS * KBS_NQ * 32);
      if (!rc) rc = dalloc(e, &e->kbsa.asg, (size_t)KBP_G * 33 * 4);
      if (!rc) rc = dalloc(e, &e->kbsa.grp, (size_t)KBP_G);
      if (!rc) rc = dalloc(e, &e->kbsa.b_v, M * (size_t)d.Bs);
      if (!rc) rc = dalloc(e, &e->kbs_blk, 1);
      if (rc) return rc;
      memset(&e->kbs_blk_host, 0xff, sizeof e->kbs_blk_host);
    }
    HIPCHK(lds_limit_once((const void *)kbs, 9));
    if (const char *ev = getenv("MIOSQP_KBS_CHUNKS")) e->kbs_chunks = std::max(1, atoi(ev));
    if (const char *ev = getenv("MIOSQP_KBS_FAULT_AT")) e->kbs_fault_at = atoll(ev);
    if (getenv("MIOSQP_KBS_PROF")) {
      int rc = dalloc(e, &e->kbs_prof, (size_t)32 * KBP_WGS);
      if (rc) return rc;
    }
    e->kbs = true;
  }
#undef ALP
  // host-visible control: the ready ring and its tail + incumbent (written by the host), the digest ring and a
  // copy of the counters (written by the device) -- a few KB per chunk over PCIe, no memcpy nodes in the graph
  HIPCHK(hipHostMalloc((void **)&e->h_ready, sizeof(ReadyEntry) * ring, hipHostMallocCoherent));
  HIPCHK(hipHostMalloc((void **)&e->h_dg, sizeof(miosqp_pool_digest) * ring, hipHostMallocCoherent));
  HIPCHK(hipHostMalloc((void **)&e->h_pctl, sizeof(PoolCtl) * 2, hipHostMallocCoherent));
  memset(e->h_ready, 0, sizeof(ReadyEntry) * ring);
  memset(e->h_dg, 0, sizeof(miosqp_pool_digest) * ring);
  memset(e->h_pctl, 0, sizeof(PoolCtl) * 2);
  d.ready = e->h_ready;
  d.dg_ring = e->h_dg;
  d.hctl = e->h_pctl;      // [0]: host -> device (tail, upper), [1]: device -> host (head, fin, active)
  d.ring = ring;
  d.stream = 0;
  d.max_iter_s = e->st.max_iter;
  h.ready = d.ready; h.dg_ring = d.dg_ring; h.hctl = d.hctl; h.ring = ring; h.max_iter_s = d.max_iter_s;
  h.pctl = d.pctl; h.fmap = d.fmap; h.hmap = d.hmap; h.lt_x = d.lt_x;
  h.pl_lo = d.pl_lo; h.pl_hi = d.pl_hi; h.pl_ws = d.pl_ws; h.sol_x = d.sol_x; h.sol_y = d.sol_y;
  e->node_cap = capacity;
  e->pool_seen = 0;
  e->h_pctl[0].upper = 1.7e308;
  hipLaunchKernelGGL(kp_reset, dim3((d.Bs + 255) / 256), dim3(256), 0, e->stream, d);
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int miosqp_qp_pool_reset(miosqp_qp_engine *e) {
  if (!e || !e->node_cap) return MIOSQP_EARG;
  ENTER(e);
  kbs_stop(e);  // (whatever is still queued leaves at its next chunk boundary)
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->side) HIPCHK(hipStreamSynchronize(e->side));
  e->h_pctl[0].pad[0] = 0;
  if (e->kbs) HIPCHK(hipMemsetAsync(e->kbsa.grp, 0, sizeof(KbsGroup) * KBP_G, e->stream));
  e->h_pctl[0].tail = 0;
  e->h_pctl[0].upper = 1.7e308;
  e->pool_seen = 0;
  e->pool_pending = 0;
  e->pool_launched = 0;
  e->pool_chunk_total = 0;
  e->pool_dirty = false;
  memset(e->h_dg, 0, sizeof(miosqp_pool_digest) * (size_t)e->d.ring);  // (no seal of an earlier instance survives)
  hipLaunchKernelGGL(kp_reset, dim3((e->d.Bs + 255) / 256), dim3(256), 0, e->stream, e->d);
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int miosqp_qp_pool_write_node(miosqp_qp_engine *e, int32_t slot, const double *l_int, const double *u_int,
                              const double *x0, const double *y0) {
  if (!e || !e->node_cap || slot < 0 || slot >= e->node_cap || !l_int || !u_int || !x0 || !y0) return MIOSQP_EARG;
  ENTER(e);
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M, p = d.n_int;
  if (host_may_read(l_int) && host_may_read(u_int))  // (a leaf out of another rank's store was checked when it was made)
    for (size_t k = 0; k < p; k++)
      if (l_int[k] > u_int[k]) return MIOSQP_EBOUNDS;
  // (copies on the engine's own stream, then one wait: a blocking copy on the legacy stream may not run while another
  //  engine of the process -- another pool on another host thread -- is capturing its chunk graph; beside a persistent
  //  launch of the stream: on the side stream)
  hipStream_t cs = slot_stream(e);
  if (p) {
    HIPCHK(hipMemcpyAsync(d.pl_lo + slot * p, l_int, sizeof(double) * p, hipMemcpyDefault, cs));
    HIPCHK(hipMemcpyAsync(d.pl_hi + slot * p, u_int, sizeof(double) * p, hipMemcpyDefault, cs));
  }
  HIPCHK(hipMemcpyAsync(d.sol_x + slot * n, x0, sizeof(double) * n, hipMemcpyDefault, cs));
  HIPCHK(hipMemcpyAsync(d.sol_y + slot * M, y0, sizeof(double) * M, hipMemcpyDefault, cs));
  const int self = slot;
  HIPCHK(hipMemcpyAsync(d.pl_ws + slot, &self, sizeof(int), hipMemcpyHostToDevice, cs));
  HIPCHK(hipStreamSynchronize(cs));
  return 0;
}

int miosqp_qp_pool_read_node(miosqp_qp_engine *e, int32_t slot, double *l_int, double *u_int, double *x, double *y) {
  if (!e || !e->node_cap || slot < 0 || slot >= e->node_cap) return MIOSQP_EARG;
  ENTER(e);
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M, p = d.n_int;
  // (stream-ordered behind a chunk in flight, which may be writing the slot; beside a persistent launch of the stream: on
  //  the side stream -- the slot's solution and bounds were stored, system scope, before the digest that named it was sealed)
  hipStream_t cs = slot_stream(e);
  if (l_int && p) HIPCHK(hipMemcpyAsync(l_int, d.pl_lo + slot * p, sizeof(double) * p, hipMemcpyDefault, cs));
  if (u_int && p) HIPCHK(hipMemcpyAsync(u_int, d.pl_hi + slot * p, sizeof(double) * p, hipMemcpyDefault, cs));
  if (x) HIPCHK(hipMemcpyAsync(x, d.sol_x + slot * n, sizeof(double) * n, hipMemcpyDefault, cs));
  if (y) HIPCHK(hipMemcpyAsync(y, d.sol_y + slot * M, sizeof(double) * M, hipMemcpyDefault, cs));
  HIPCHK(hipStreamSynchronize(cs));
  return 0;
}

int miosqp_qp_pool_push(miosqp_qp_engine *e, int32_t count, const int32_t *slot, const int32_t *child0,
                        const int32_t *child1, const double *lower) {
  if (!e || !e->node_cap || count < 0 || (count && (!slot || !child0 || !child1 || !lower))) return MIOSQP_EARG;
  PoolCtl *hc = e->h_pctl;
  const unsigned long long tail = hc[0].tail, head = hc[1].head;  // head: as of the last collected chunk (a lower bound)
  if (tail + (unsigned long long)count - head > (unsigned long long)e->d.ring) {
    g_err = "pool_push: the ready ring is full";
    return MIOSQP_EARG;
  }
  for (int k = 0; k < count; k++) {
    if (slot[k] < 0 || slot[k] >= e->node_cap || child0[k] >= e->node_cap || child1[k] >= e->node_cap) return MIOSQP_EARG;
    ReadyEntry &r = e->h_ready[(tail + k) % (unsigned long long)e->d.ring];
    r.slot = slot[k];
    r.child0 = child0[k];
    r.child1 = child1[k];
    r.pad = 0;
    r.lower = lower[k];
  }
  __atomic_thread_fence(__ATOMIC_RELEASE);  // the entries before the tail that publishes them
  __atomic_store_n(&hc[0].tail, tail + (unsigned long long)count, __ATOMIC_RELEASE);
  return 0;
}

int miosqp_qp_pool_set_upper(miosqp_qp_engine *e, double upper) {
  if (!e || !e->node_cap) return MIOSQP_EARG;
  e->h_pctl[0].upper = upper;
  return 0;
}

int miosqp_qp_pool_launch(miosqp_qp_engine *e, int32_t chunks) {
  if (!e || !e->node_cap || chunks < 1) return MIOSQP_EARG;
  ENTER(e);
  if (e->pool_dirty) {
    g_err = "pool_launch: solve_batch used the columns since the last pool_reset; call miosqp_qp_pool_reset first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending >= POOL_EVENTS) {
    g_err = "pool_launch: too many launches in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  // MIOSQP_POOL_NOGRAPH=1: the chunk's ~70 kernels are launched one by one instead of as a captured graph
  // (rocprofv3 --kernel-trace dies inside hipGraphLaunch after ~230 launches of this graph; eager launches
  // profile fine and cost ~0.3 ms of host time per chunk, hidden behind the chunk in flight)
  static const bool nograph = getenv("MIOSQP_POOL_NOGRAPH") != nullptr;
  if (e->pool_pending == 0) {
    if (int rcj = maybe_rejoin_kbp(e, 64)) return rcj;  // (the drivers drain their launches every 64th round)
  }
  // On a chip this process shares among several engines, the chunk's persistent launch takes its turn among the
  // whole-chip launches (ChipTurn): the chunk is then two captured halves around an eager launch of kbp, so that this
  // pool's refill, test and harvest still run under another pool's sweeps.
  const bool one_launch = kbs_here(e);
  const bool split = !one_launch && !nograph && kbp_here(e, e->Bcap / 64) && chip_shared(e);
  if (one_launch) {
  } else if (split) {
    if (!e->x_stream_a) {
      int rc = capture_stream_chunk(e, 1);
      if (!rc) rc = capture_stream_chunk(e, 2);
      if (rc) return rc;
    }
  } else if (!nograph && !e->x_stream) {
    int rc = capture_stream_chunk(e);
    if (rc) return rc;
  }
  const int slot = (int)(e->pool_launched % POOL_EVENTS);
  if (!e->ev_pool[2 * slot]) {
    HIPCHK(hipEventCreate(&e->ev_pool[2 * slot]));
    HIPCHK(hipEventCreate(&e->ev_pool[2 * slot + 1]));
  }
  // the start event sits in the stream right behind the previous launch: start -> end brackets exactly this
  // launch's execution, also when launches are queued ahead
  HIPCHK(hipEventRecord(e->ev_pool[2 * slot], e->stream));
  if (one_launch) {
    launch_kbs(e, chunks);
    e->kbs_launches++;
    e->kbs_chunks_run += chunks;
  } else {
    e->graph_chunks_run += chunks;
  }
  for (int k = 0; k < chunks && !one_launch; k++) {
    if (nograph) {
      enqueue_stream_chunk(e);
    } else if (split) {
      Dev ds = e->d;
      ds.stream = 1;
      HIPCHK(hipGraphLaunch(e->x_stream_a, e->stream));
      launch_kbp(e, ds, e->Bcap / 64, e->chunk);  // (takes its turn: ChipGuard inside)
      HIPCHK(hipGraphLaunch(e->x_stream_b, e->stream));
    } else {
      // (the captured chunk may hold a whole-chip launch: it takes its turn like solve_slice's chunks do -- an engine
      //  that joined the chip after `split` was decided would otherwise overlap it and send both to the call-off path)
      ChipGuard turn(e);
      HIPCHK(hipGraphLaunch(e->x_stream, e->stream));
    }
  }
  HIPCHK(hipEventRecord(e->ev_pool[2 * slot + 1], e->stream));
  e->pool_chunks[slot] = chunks;
  e->pool_chunk_total += (unsigned long long)chunks;
  e->pool_target[slot] = e->pool_chunk_total;
  e->pool_launched++;
  e->pool_pending++;
  return 0;
}

int miosqp_qp_pool_collect(miosqp_qp_engine *e, int32_t keep_in_flight, miosqp_pool_digest *out, int32_t max_out,
                           int32_t *n_out, int32_t *active, int64_t *ready_left) {
  if (!e || !e->node_cap || (max_out > 0 && !out) || !n_out || keep_in_flight < 0) return MIOSQP_EARG;
  ENTER(e);
  while (e->pool_pending > 0) {  // oldest first
    const int slot = (int)((e->pool_launched - e->pool_pending) % POOL_EVENTS);
    // beyond what the caller wants kept in flight, a launch is retired only when it is over (its last kernel has mirrored its chunk count)
    if (e->pool_pending <= keep_in_flight &&
        __atomic_load_n(&e->h_pctl[1].chunks, __ATOMIC_ACQUIRE) < e->pool_target[slot])
      break;
    hipEvent_t end = e->ev_pool[2 * slot + 1];
    if (e->spin_wait) {
      // the launch's last kernel mirrors the count of completed chunks into host memory: polling that word instead
      // of the event keeps the waiting thread out of the runtime (several pools wait on several host threads)
      const unsigned long long want = e->pool_target[slot];
      unsigned long long spins = 0;
      while (__atomic_load_n(&e->h_pctl[1].chunks, __ATOMIC_ACQUIRE) < want) {
        if ((++spins & 0xfffff) == 0) {
          const hipError_t q = hipEventQuery(end);
          if (q != hipSuccess && q != hipErrorNotReady) HIPCHK(q);
          if (q == hipSuccess) break;  // (the launch is over: the count is as good as it gets)
        }
      }
    }
    HIPCHK(hipEventSynchronize(end));  // (a few microseconds behind the last kernel at most)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev_pool[2 * slot], end));
    e->bloop_ms += ms;
    e->bloop_iters += (int64_t)e->pool_chunks[slot] * e->chunk;
    e->pool_pending--;
  }
  // a full stream synchronisation now and then: event waits alone never give tools that hook the runtime
  // (rocprofv3 --kernel-trace) a point to retire their per-dispatch records; it died after ~16 k graph kernels
  if (e->pool_launched - e->pool_synced >= 64 && e->pool_pending == 0) {
    HIPCHK(hipStreamSynchronize(e->stream));
    e->pool_synced = e->pool_launched;
  }
  const PoolCtl &dc = e->h_pctl[1];
  if (dc.pad[0] && e->kbp) {
    if (dc.pad[0] != 1) {
      g_err = "batched persistent sweeps: a group barrier timed out, stage " + std::to_string(dc.pad[0]);
      return MIOSQP_EHIP;
    }
    // a chunk's persistent launch was called off (nothing iterated, nothing decided): the launches from here on
    int rcl = kbp_leave(e);
    if (rcl) return rcl;
    e->h_pctl[1].pad[0] = 0;
  }
  const unsigned long long fin = __atomic_load_n(&dc.fin, __ATOMIC_ACQUIRE);
  if (fin - e->pool_seen > (unsigned long long)e->d.ring) {
    g_err = "pool_collect: the digest ring overflowed (collect more often)";
    return MIOSQP_EARG;
  }
  int k = 0;
  while (e->pool_seen < fin && k < max_out) {
    const miosqp_pool_digest &src = e->h_dg[e->pool_seen % (unsigned long long)e->d.ring];
    // sealed by its writer (dg_seal): not yet this lap's number -> its stores are still on their way; next collect
    if ((unsigned)__atomic_load_n(&src.reserved, __ATOMIC_ACQUIRE) != (unsigned)(e->pool_seen + 1ull)) break;
    out[k] = src;
    out[k].reserved = 0;
    if (out[k].iter > 0) e->bloop_node_iters += out[k].iter;
    e->pool_seen++;
    k++;
  }
  *n_out = k;
  if (active) *active = dc.active;
  if (ready_left) *ready_left = (int64_t)(e->h_pctl[0].tail - dc.head);
  return 0;
}

}  // extern "C"
