// part of engine.hip (included there, not compiled alone; behind host_lockstep_ahead.inc, the LAST file of the translation
// unit): the lock-step trees of host_lockstep.inc with strong and reliability branching (C ABI
// miosqp_qp_solve_trees_lockstep_sb).  The wave is miosqp_qp_solve_trees_lockstep's -- the same launches, the same record --
// and between a node's verdict (Tree::begin) and the entry of its children (Tree::end) the nodes that branch choose
// their position as Workspace.select_branching does (lockstep_sb.hpp has the logic): their x at the integer positions
// comes down in one block, the 2K children of every node with candidates go out as ONE more batch through the
// unchanged slice_run with the cap sb_max_iter, a 16-byte record per child comes back, and one launch writes the
// children of the chosen positions into the slots the wave reserved (kls_scatter wrote them for the most fractional
// position).  Store, slots, roots, costs, gather, scatter and incumbent kernels are the lock-step driver's.
namespace {

struct SbStore {
  int inst_cap = 0, col_cap = 0, p = 0;
  int *d_ask = nullptr, *h_ask = nullptr;          // [4 inst_cap]: the asking nodes' slots going up, later their quads
  double *d_xint = nullptr, *h_xint = nullptr;     // [inst_cap][2 p]: x at the integer positions | crossing flags
  int *d_col = nullptr, *h_col = nullptr;          // [col_cap][LS_TRIP]: the children's columns
  LsSbChild *d_child = nullptr, *h_child = nullptr;  // [col_cap]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  miosqp::lockstep::SbSlots slots;
  std::vector<miosqp::lockstep::SbTree> trees;
  std::vector<miosqp::lockstep::SbChild> kids;
  struct Ask {
    int col;     // the node's column of the wave
    int first;   // its first child column of the batch (-1: nothing to solve)
    int K;
    int pos;     // the chosen position
  };
  std::vector<Ask> asks;
  std::vector<char> branch;  // per column of the wave: its node branches
};

void sb_release(SbStore *S) {
  if (S->d_ask) hipFree(S->d_ask);
  if (S->h_ask) hipHostFree(S->h_ask);
  if (S->d_xint) hipFree(S->d_xint);
  if (S->h_xint) hipHostFree(S->h_xint);
  if (S->d_col) hipFree(S->d_col);
  if (S->h_col) hipHostFree(S->h_col);
  if (S->d_child) hipFree(S->d_child);
  if (S->h_child) hipHostFree(S->h_child);
  S->d_ask = S->h_ask = S->d_col = S->h_col = nullptr;
  S->d_xint = S->h_xint = nullptr;
  S->d_child = S->h_child = nullptr;
  S->inst_cap = S->col_cap = 0;
}

void sb_free(void *p) {
  SbStore *S = static_cast<SbStore *>(p);
  if (!S) return;
  sb_release(S);
  if (S->ev0) hipEventDestroy(S->ev0);
  if (S->ev1) hipEventDestroy(S->ev1);
  delete S;
}

// room for B asking nodes with 2K children each
int sb_reserve(miosqp_qp_engine *e, SbStore &S, int B, int K) {
  const size_t p = (size_t)e->d.n_int, cols = (size_t)B * 2 * (size_t)K;
  if (!S.ev0) {
    HIPCHK(hipEventCreate(&S.ev0));
    HIPCHK(hipEventCreate(&S.ev1));
  }
  if (B <= S.inst_cap && cols <= (size_t)S.col_cap && (int)p == S.p) return 0;
  HIPCHK(hipStreamSynchronize(e->stream));
  sb_release(&S);
  const size_t cap = (size_t)B;
  bool ok = hipMalloc((void **)&S.d_ask, 4 * cap * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&S.d_xint, cap * 2 * p * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&S.d_col, cols * LS_TRIP * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&S.d_child, cols * sizeof(LsSbChild)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sb_release(&S);
    g_err = "solve_trees_lockstep_sb: no device memory for the children's columns";
    return MIOSQP_EFULL;
  }
  HIPCHK(hipHostMalloc((void **)&S.h_ask, 4 * cap * sizeof(int), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&S.h_xint, cap * 2 * p * sizeof(double), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&S.h_col, cols * LS_TRIP * sizeof(int), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&S.h_child, cols * sizeof(LsSbChild), hipHostMallocDefault));
  S.inst_cap = B;
  S.col_cap = (int)cols;
  S.p = (int)p;
  return 0;
}

// the body of miosqp_qp_solve_trees_lockstep_sb: lockstep_trees_run's wave loop with the branching step
int lockstep_sb_run(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u, const double *x0,
                    const double *y0, const double *upper0, const double *x_inc0, int32_t tree_explor_rule, int32_t max_iter_bb,
                    int32_t capacity, const miosqp::lockstep::SbParams &sp_in, int32_t sb_max_iter, double *x_out,
                    miosqp_tree_info *info, miosqp_lockstep_stats *stats, miosqp_lockstep_sb_stats *ss) {
  using miosqp::lockstep::Record;
  using miosqp::lockstep::SbChild;
  using miosqp::lockstep::SbTree;
  using miosqp::lockstep::Tree;
  using miosqp::lockstep::Verdict;
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = "solve_trees_lockstep_sb: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending) {
    g_err = "solve_trees_lockstep_sb: streaming chunks are still in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M, m = (size_t)e->d.m_orig, p = (size_t)e->d.n_int;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) {  // (nothing has been queued)
      g_err = "solve_trees_lockstep_sb: l > u in the root of instance " + std::to_string(k / M);
      return MIOSQP_EBOUNDS;
    }
  miosqp::lockstep::SbParams sp = sp_in;
  sp.eps_int = e->d.eps_int;
  stats->waves = stats->max_width = stats->grown = 0;
  stats->nodes = stats->iters_slowest = stats->iters_all = 0;
  stats->device_time = stats->run_time = stats->host_time = 0.0;
  ss->batches = 0;
  ss->columns = ss->iters_slowest = 0;
  ss->device_time = 0.0;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  if (!e->lockstep) e->lockstep = new LockstepStore();
  LockstepStore &L = *static_cast<LockstepStore *>(e->lockstep);
  if (int rc = lockstep_reserve(e, L, B)) return rc;
  if (!L.sb) L.sb = new SbStore();
  SbStore &S = *static_cast<SbStore *>(L.sb);
  if (int rc = sb_reserve(e, S, B, sp.K)) return rc;
  {
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
  S.slots.reset(L.cap);
  S.trees.assign((size_t)B, SbTree());
  std::vector<char> called((size_t)B, 0);  // (debug: the tree has had its first call)
  // ---- the roots, as lockstep_trees_run uploads them ----
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
      S.trees[(size_t)b].start((int)p);
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
    hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, d, L.dev.qraw,
                       const_cast<double *>(L.dev.qs), B);
  }
  std::vector<int> live;
  live.reserve((size_t)B);
  int64_t iters_total = 0;
  double host_s = 0.0;
  const int big = (int)(n > M ? n : M);
  // ---- the waves ----
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
      S.slots.grow(L.cap);
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
    for (int s0 = 0; s0 < W; s0 += e->Bcap) {
      const int nb = W - s0 < e->Bcap ? W - s0 : e->Bcap;
      const int ntiles = (nb + 63) / 64;
      if (int rc = slice_begin(e, nb)) return rc;
      if (s0 == 0)
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
    // ---- bound_and_branch per tree on its column's record, up to the children ----
    th = wall();
    const int wave = ++stats->waves;
    int it_max = 0, npairs = 0;
    int64_t it_sum = 0;
    S.branch.assign((size_t)W, 0);
    S.asks.clear();
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
      S.trees[(size_t)b].node_solved(S.slots, tr[LS_SLOT], r.ok, r.lower);
      const Verdict v = T.begin(L.slots, tr[LS_SLOT], r, 0).v;
      if (v.incumbent) {
        int *pr = L.h_pairs + 3 * npairs++;
        pr[0] = b;
        pr[1] = tr[LS_SLOT];
        pr[2] = v.incumbent == 2;
      }
      S.branch[(size_t)c] = v.branch;
      if (v.branch) S.asks.push_back(SbStore::Ask{c, -1, 0, -1});
      it_max = g.iter > it_max ? g.iter : it_max;
      it_sum += g.iter;
    }
    host_s += wall() - th;
    if (npairs > 0) {
      HIPCHK(hipMemcpyAsync(L.d_pairs, L.h_pairs, sizeof(int) * 3 * (size_t)npairs, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_incumbent<0>, dim3(npairs), dim3(256), 0, e->stream, d, L.dev, L.d_pairs, npairs);
    }
    const int A = (int)S.asks.size();
    if (A > 0) {
      // ---- select_branching: the asking nodes' x at the integer positions, ONE download ----
      for (int a = 0; a < A; a++) S.h_ask[a] = L.h_trip[LS_TRIP * S.asks[(size_t)a].col + LS_SLOT];
      HIPCHK(hipEventRecord(S.ev0, e->stream));
      HIPCHK(hipMemcpyAsync(S.d_ask, S.h_ask, sizeof(int) * (size_t)A, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_sb_xint<0>, dim3(A), dim3(256), 0, e->stream, d, L.dev, S.d_ask, A, S.d_xint);
      HIPCHK(hipMemcpyAsync(S.h_xint, S.d_xint, sizeof(double) * (size_t)A * 2 * p, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipGetLastError());
      th = wall();
      int C = 0;
      for (int a = 0; a < A; a++) {
        SbStore::Ask &k = S.asks[(size_t)a];
        const int *tr = L.h_trip + LS_TRIP * k.col;
        const int b = tr[LS_TREE];
        SbTree &ST = S.trees[(size_t)b];
        const double *xa = S.h_xint + (size_t)a * 2 * p, *cross = xa + p;
        const int pos = ST.ask(sp, xa);
        if (pos == -2) {
          g_err = "solve_trees_lockstep_sb: a fractional node without a fractional position (instance " + std::to_string(b) + ")";
          return MIOSQP_EARG;
        }
        if (pos >= 0) {
          k.pos = pos;
          continue;
        }
        k.first = C;
        k.K = (int)ST.cand.size();
        for (int side = 0; side < 2; side++)
          for (int j = 0; j < k.K; j++) {
            const int cp = ST.cand[(size_t)j];
            if (cross[cp] != 0.0) {  // (strong_branch refuses such a child: miosqp_qp_strong_branch, MIOSQP_EBOUNDS)
              g_err = "solve_trees_lockstep_sb: branching produced l > u (instance " + std::to_string(b) + ")";
              return MIOSQP_EBOUNDS;
            }
            int *ct = S.h_col + LS_TRIP * (size_t)C++;
            ct[LS_TREE] = b;
            ct[LS_SLOT] = ct[LS_WARM] = tr[LS_SLOT];  // the node's own x, y (it is held until its children are decided)
            ct[LS_SB_POS] = cp;
            ct[LS_SB_SIDE] = side;
          }
      }
      host_s += wall() - th;
      if (C > 0) {
        // ---- strong_branch: the children of every node with candidates, ONE batch ----
        for (int s0 = 0; s0 < C; s0 += e->Bcap) {  // sliced as a wave is; a node's children may straddle two slices
          const int nb = C - s0 < e->Bcap ? C - s0 : e->Bcap;
          if (int rc = slice_begin(e, nb)) return rc;
          if (s0 == 0) HIPCHK(hipMemcpyAsync(S.d_col, S.h_col, sizeof(int) * LS_TRIP * (size_t)C, hipMemcpyHostToDevice, e->stream));
          const int *trip = S.d_col + LS_TRIP * s0;
          hipLaunchKernelGGL(kls_sb_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb);
          const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
          if (int rc = slice_run(e, nb, sb_max_iter, &roots)) return rc;
          hipLaunchKernelGGL(kls_sb_judge<0>, dim3((nb + 255) / 256), dim3(256), 0, e->stream, d, S.d_child + s0, nb);
        }
        HIPCHK(hipMemcpyAsync(S.h_child, S.d_child, sizeof(LsSbChild) * (size_t)C, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(S.ev1, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        float sb_ms = 0;
        HIPCHK(hipEventElapsedTime(&sb_ms, S.ev0, S.ev1));
        ss->batches++;
        ss->columns += C;
        ss->device_time += 1e-3 * sb_ms;
      }
      th = wall();
      int sb_it_max = 0;
      for (int a = 0; a < A; a++) {
        SbStore::Ask &k = S.asks[(size_t)a];
        const int *tr = L.h_trip + LS_TRIP * k.col;
        const int b = tr[LS_TREE];
        SbTree &ST = S.trees[(size_t)b];
        const double *xa = S.h_xint + (size_t)a * 2 * p, *cross = xa + p;
        const double node_lower = L.h_rec[k.col].lower;
        if (k.first >= 0) {
          // (ask left the tree's frac / cand for this node: a tree has one node per wave)
          S.kids.resize((size_t)(2 * k.K));
          for (int j = 0; j < 2 * k.K; j++) {
            const LsSbChild &cd = S.h_child[k.first + j];
            S.kids[(size_t)j] = SbChild{cd.status == MIOSQP_QP_SOLVED || cd.status == MIOSQP_QP_MAX_ITER_REACHED, cd.iter, cd.lower};
            sb_it_max = cd.iter > sb_it_max ? cd.iter : sb_it_max;
          }
          int best = 0;
          k.pos = ST.decide(sp, xa, node_lower, S.kids.data(), &best);
          if (!called[(size_t)b]) {  // debug: the first call of every tree
            called[(size_t)b] = 1;
            const size_t Km = (size_t)sp.K;
            if (ss->first_k) ss->first_k[b] = k.K;
            if (ss->first_chosen) ss->first_chosen[b] = best;
            for (int j = 0; j < k.K; j++)
              if (ss->first_cand) ss->first_cand[(size_t)b * Km + (size_t)j] = ST.cand[(size_t)j];
            for (int j = 0; j < 2 * k.K; j++) {
              const LsSbChild &cd = S.h_child[k.first + j];
              if (ss->first_status) ss->first_status[(size_t)b * 2 * Km + (size_t)j] = cd.status;
              if (ss->first_iter) ss->first_iter[(size_t)b * 2 * Km + (size_t)j] = cd.iter;
              if (ss->first_lower) ss->first_lower[(size_t)b * 2 * Km + (size_t)j] = cd.lower;
            }
          }
        }
        if (k.pos < 0 || k.pos >= (int)p || cross[k.pos] != 0.0) {  // (Workspace._child refuses l > u)
          g_err = "solve_trees_lockstep_sb: branching produced l > u (instance " + std::to_string(b) + ")";
          return MIOSQP_EBOUNDS;
        }
        ST.branched(sp, S.slots, tr[LS_CHILD0], tr[LS_CHILD1], k.pos, xa, node_lower);
        int *qd = S.h_ask + 4 * a;  // (the slots' upload is done: the download behind it has been waited for)
        qd[0] = tr[LS_SLOT];
        qd[1] = tr[LS_CHILD0];
        qd[2] = tr[LS_CHILD1];
        qd[3] = k.pos;
      }
      ss->iters_slowest += sb_it_max;
      host_s += wall() - th;
      // ---- the children on the chosen positions (the pinned quads are next written after the next wave's drain) ----
      HIPCHK(hipMemcpyAsync(S.d_ask, S.h_ask, sizeof(int) * 4 * (size_t)A, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_sb_children<0>, dim3(A), dim3(256), 0, e->stream, d, L.dev, S.d_ask, A);
    }
    th = wall();
    for (int c = 0; c < W; c++) {  // branch_children, in the order of the wave
      const int *tr = L.h_trip + LS_TRIP * c;
      Tree &T = L.trees[(size_t)tr[LS_TREE]];
      T.end(L.slots, tr[LS_SLOT], tr[LS_CHILD0], tr[LS_CHILD1], Verdict{S.branch[(size_t)c] != 0, 0});
      if (!T.can_continue(max_iter_bb)) T.finished_at = wave;
    }
    host_s += wall() - th;
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
    const SbTree &ST = S.trees[(size_t)b];
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
    if (ss->calls) ss->calls[b] = (int32_t)ST.calls;
    if (ss->children) ss->children[b] = (int32_t)ST.children;
    if (ss->iters) ss->iters[b] = ST.iters;
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

int miosqp_qp_solve_trees_lockstep_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                      const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                      int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t branching_rule,
                                      int32_t sb_candidates, int32_t sb_max_iter, int32_t sb_reliability, double sb_eps,
                                      double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                      miosqp_lockstep_sb_stats *sb_stats) {
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || !stats || !sb_stats || max_iter_bb < 1 ||
      tree_explor_rule < 0 || tree_explor_rule > 3 || capacity < 0)
    return MIOSQP_EARG;
  ENTER(e);
  if (branching_rule != 1 && branching_rule != 2) {
    g_err = "solve_trees_lockstep_sb: branching_rule must be 1 or 2";
    return MIOSQP_EARG;
  }
  if (sb_candidates < 1 || sb_candidates > SB_MAX_K) {
    g_err = "solve_trees_lockstep_sb: sb_candidates must be in 1..32";
    return MIOSQP_EARG;
  }
  if (sb_max_iter <= 0 || sb_max_iter % e->chunk != 0) {
    g_err = "solve_trees_lockstep_sb: sb_max_iter must be a positive multiple of check_termination";
    return MIOSQP_EARG;
  }
  if (sb_reliability < 0) {
    g_err = "solve_trees_lockstep_sb: sb_reliability must not be negative";
    return MIOSQP_EARG;
  }
  if (!(sb_eps > 0.0)) {
    g_err = "solve_trees_lockstep_sb: sb_eps must be positive";
    return MIOSQP_EARG;
  }
  const miosqp::lockstep::SbParams sp{branching_rule, sb_candidates, sb_reliability, sb_eps, 0.0};
  return lockstep_sb_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, sp, sb_max_iter, x_out,
                         info, stats, sb_stats);
}

}  // extern "C"
