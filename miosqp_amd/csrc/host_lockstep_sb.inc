// part of engine.hip (included there, not compiled alone; behind host_lockstep_ahead.inc, the LAST file of the translation
// unit): the lock-step trees of host_lockstep.inc with strong and reliability branching (C ABI
// miosqp_qp_solve_trees_lockstep_sb).  The wave is miosqp_qp_solve_trees_lockstep's -- the same launches, the same record --
// and between a node's verdict (Tree::begin) and the entry of its children (Tree::end) the nodes that branch choose
// their position as Workspace.select_branching does (lockstep_sb.hpp has the logic): their x at the integer positions
// comes down in one block, the 2K children of every node with candidates go out as ONE more batch through the
// unchanged slice_run with the cap sb_max_iter, a 16-byte record per child comes back, and one launch writes the
// children of the chosen positions into the slots the wave reserved (kls_scatter wrote them for the most fractional
// position).  Store, slots, roots, costs, gather, scatter and incumbent kernels are the lock-step driver's.
//
// This file owns the branching step (SbStore, LsSbStep) and the entry with its parameter checks; the call around it --
// checks, store, roots, the wave loop, incumbents, info[] -- is ls_trees_run and the pieces of host_lockstep.inc.
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
  std::vector<Ask> asks;  // the wave's nodes that branch (empty between waves)
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

// the branching step in ls_trees_run (host_lockstep.inc): between the verdicts of a wave and the entry of the children
struct LsSbStep {
  const LsCall &a;
  LockstepStore &L;
  SbStore &S;
  const miosqp::lockstep::SbParams sp;
  const int max_iter;
  miosqp_lockstep_sb_stats *ss;
  std::vector<char> called;  // (debug: the tree has had its first call)
  LsSbStep(const LsCall &a_, LockstepStore &L_, SbStore &S_, const miosqp::lockstep::SbParams &sp_, int max_iter_,
           miosqp_lockstep_sb_stats *ss_)
      : a(a_), L(L_), S(S_), sp(sp_), max_iter(max_iter_), ss(ss_), called((size_t)a_.B, 0) {}

  void grown(int cap) { S.slots.grow(cap); }

  // up to the children: a node that branches asks for its position
  int verdict(int c, const int *tr, const LsRec &, const miosqp::lockstep::Record &r, miosqp::lockstep::Tree &T, int,
              miosqp::lockstep::Verdict *v) {
    S.trees[(size_t)tr[LS_TREE]].node_solved(S.slots, tr[LS_SLOT], r.ok, r.lower);
    *v = T.begin(L.slots, tr[LS_SLOT], r, 0).v;
    if (v->branch) S.asks.push_back(SbStore::Ask{c, -1, 0, -1});
    return 0;
  }

  int children(int W, int wave, double *host_s) {
    using miosqp::lockstep::SbChild;
    using miosqp::lockstep::SbTree;
    miosqp_qp_engine *e = a.e;
    const Dev &d = e->d;
    const size_t n = e->n, M = e->M, p = (size_t)d.n_int;
    const int big = (int)(n > M ? n : M);
    const int A = (int)S.asks.size();
    double th;
    if (A > 0) {
      // ---- select_branching: the asking nodes' x at the integer positions, ONE download ----
      for (int k = 0; k < A; k++) S.h_ask[k] = L.h_trip[LS_TRIP * S.asks[(size_t)k].col + LS_SLOT];
      HIPCHK(hipEventRecord(S.ev0, e->stream));
      HIPCHK(hipMemcpyAsync(S.d_ask, S.h_ask, sizeof(int) * (size_t)A, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_sb_xint<0>, dim3(A), dim3(256), 0, e->stream, d, L.dev, S.d_ask, A, S.d_xint);
      HIPCHK(hipMemcpyAsync(S.h_xint, S.d_xint, sizeof(double) * (size_t)A * 2 * p, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipGetLastError());
      th = wall();
      int C = 0;
      for (int i = 0; i < A; i++) {
        SbStore::Ask &k = S.asks[(size_t)i];
        const int *tr = L.h_trip + LS_TRIP * k.col;
        const int b = tr[LS_TREE];
        SbTree &ST = S.trees[(size_t)b];
        const double *xa = S.h_xint + (size_t)i * 2 * p, *cross = xa + p;
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
            if (cross[cp] != 0.0) return ls_crossed(a, b);  // (strong_branch refuses such a child: miosqp_qp_strong_branch, MIOSQP_EBOUNDS)
            int *ct = S.h_col + LS_TRIP * (size_t)C++;
            ct[LS_TREE] = b;
            ct[LS_SLOT] = ct[LS_WARM] = tr[LS_SLOT];  // the node's own x, y (it is held until its children are decided)
            ct[LS_SB_POS] = cp;
            ct[LS_SB_SIDE] = side;
          }
      }
      *host_s += wall() - th;
      if (C > 0) {
        // ---- strong_branch: the children of every node with candidates, ONE batch ----
        for (int s0 = 0; s0 < C; s0 += e->Bcap) {  // sliced as a wave is; a node's children may straddle two slices
          const int nb = C - s0 < e->Bcap ? C - s0 : e->Bcap;
          if (int rc = slice_begin(e, nb)) return rc;
          if (s0 == 0) HIPCHK(hipMemcpyAsync(S.d_col, S.h_col, sizeof(int) * LS_TRIP * (size_t)C, hipMemcpyHostToDevice, e->stream));
          const int *trip = S.d_col + LS_TRIP * s0;
          hipLaunchKernelGGL(kls_sb_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb);
          const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
          if (int rc = slice_run(e, nb, max_iter, &roots)) return rc;
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
      for (int i = 0; i < A; i++) {
        SbStore::Ask &k = S.asks[(size_t)i];
        const int *tr = L.h_trip + LS_TRIP * k.col;
        const int b = tr[LS_TREE];
        SbTree &ST = S.trees[(size_t)b];
        const double *xa = S.h_xint + (size_t)i * 2 * p, *cross = xa + p;
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
        if (k.pos < 0 || k.pos >= (int)p || cross[k.pos] != 0.0) return ls_crossed(a, b);  // (Workspace._child refuses l > u)
        ST.branched(sp, S.slots, tr[LS_CHILD0], tr[LS_CHILD1], k.pos, xa, node_lower);
        int *qd = S.h_ask + 4 * i;  // (the slots' upload is done: the download behind it has been waited for)
        qd[0] = tr[LS_SLOT];
        qd[1] = tr[LS_CHILD0];
        qd[2] = tr[LS_CHILD1];
        qd[3] = k.pos;
      }
      ss->iters_slowest += sb_it_max;
      *host_s += wall() - th;
      // ---- the children on the chosen positions (the pinned quads are next written after the next wave's drain) ----
      HIPCHK(hipMemcpyAsync(S.d_ask, S.h_ask, sizeof(int) * 4 * (size_t)A, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_sb_children<0>, dim3(A), dim3(256), 0, e->stream, d, L.dev, S.d_ask, A);
      S.asks.clear();
    }
    th = wall();
    ls_children_enter(a, L, W, wave);
    *host_s += wall() - th;
    return 0;
  }
};

}  // namespace

extern "C" {

int miosqp_qp_solve_trees_lockstep_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                      const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                      int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t branching_rule,
                                      int32_t sb_candidates, int32_t sb_max_iter, int32_t sb_reliability, double sb_eps,
                                      double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                      miosqp_lockstep_sb_stats *sb_stats) {
  const LsCall a{"solve_trees_lockstep_sb", e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info};
  if (!ls_args_ok(a) || !stats || !sb_stats) return MIOSQP_EARG;
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
  if (int rc = ls_refuse(a)) return rc;
  const miosqp::lockstep::SbParams sp{branching_rule, sb_candidates, sb_reliability, sb_eps, e->d.eps_int};
  ls_stats_zero(stats);
  sb_stats->batches = 0;
  sb_stats->columns = sb_stats->iters_slowest = 0;
  sb_stats->device_time = 0.0;
  LockstepStore *Lp = nullptr;
  if (int rc = ls_open(a, B, &Lp, &stats->grown)) return rc;
  LockstepStore &L = *Lp;
  if (!L.sb) L.sb = new SbStore();
  SbStore &S = *static_cast<SbStore *>(L.sb);
  if (int rc = sb_reserve(e, S, B, sp.K)) return rc;
  S.slots.reset(L.cap);
  S.trees.assign((size_t)B, miosqp::lockstep::SbTree());
  for (int b = 0; b < B; b++) S.trees[(size_t)b].start(e->d.n_int);
  S.asks.clear();  // (a call that ended in an error between the verdicts and the children may have left some)
  LsSbStep step(a, L, S, sp, sb_max_iter, sb_stats);
  if (int rc = ls_trees_run(a, L, stats, step)) return rc;
  for (int b = 0; b < B; b++) {
    const miosqp::lockstep::SbTree &ST = S.trees[(size_t)b];
    if (sb_stats->calls) sb_stats->calls[b] = (int32_t)ST.calls;
    if (sb_stats->children) sb_stats->children[b] = (int32_t)ST.children;
    if (sb_stats->iters) sb_stats->iters[b] = ST.iters;
  }
  return 0;
}

}  // extern "C"
