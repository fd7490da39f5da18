// part of engine.hip (included there, not compiled alone; behind every file of the translation unit but host_lockstep_sb.inc and its kernels): the lock-step trees of
// host_lockstep.inc with the spare columns of every wave put to use (C ABI miosqp_qp_solve_trees_lockstep_ahead).  A wave
// launches whole tiles of 64 columns; behind the L mandatory columns -- one chosen leaf per live tree, what
// miosqp_qp_solve_trees_lockstep sends -- the rest of the last tile carries other open leaves of the same trees and children
// of nodes already solved ahead (lockstep_ahead.hpp has the tree logic, the order and the argument why results cannot
// change).  The wave ends with its mandatory columns: behind every chunk kls_need counts those still undecided, and an
// ahead column the wave did not wait for comes back UNFINISHED and leaves nothing.  Store, slots, roots, costs, gather
// and incumbent kernels are the lock-step driver's; per wave one upload (five integers and a flag per column), one
// download (a 64-byte record per column), one synchronisation behind the chunk loop's own.
//
// The two kernels below are copies and a short count over vector loads and stores: one launch each, no spin wait, no
// hand-off between workgroups, no whole-chip launch.  They are templates instantiated only here, behind every other
// kernel of the code object (see kernels_lockstep.inc for why).

constexpr int LS_UNFINISHED = -100;  // LsRec.status of a column the wave did not wait for (no QP status uses it)

// the mandatory columns of the slice the test has not decided yet.  One workgroup; nb <= 1024 columns
template <int LS>
__global__ __launch_bounds__(256) void kls_need(Dev d, const int *__restrict__ mand, int *__restrict__ left, int nb) {
  __shared__ int part[4];
  int cnt = 0;
  for (int b = threadIdx.x; b < nb; b += 256) cnt += (d.c_done[b] == 0 && mand[d.c_node[b]] != 0) ? 1 : 0;
  cnt = __popcll(__ballot(cnt & 1)) + 2 * __popcll(__ballot(cnt & 2)) + 4 * __popcll(__ballot(cnt & 4));  // (cnt <= 4)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) *left = part[0] + part[1] + part[2] + part[3];
}

// kls_scatter for a wave that may have ended before its ahead columns: with `mask`, a column whose c_done is 0 is
// UNFINISHED (the mask is c_done: kb_finish has turned its UNSOLVED status into MAX_ITER_REACHED for its own purposes) --
// no x / y store, no children, a record with LS_UNFINISHED and the iterations it had run.  Everything else, and every
// column without `mask`, as kls_scatter does it: the same loads, the same stores, the same bits.  Same grid.
template <int LS>
__global__ __launch_bounds__(256) void kls_scatter_ahead(Dev d, LsDev ls, const int *__restrict__ trip, LsRec *__restrict__ rec, int nb,
                                                         int mask) {
  __shared__ double tile[64][65];
  __shared__ int slot_of[64];
  const int n = d.n, M = d.M, p = d.n_int;
  const int nxt = (n + 63) / 64, nyt = (M + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.y * 64;
  const size_t Bs = (size_t)d.Bs;
  if (threadIdx.x < 64) {
    const int b = b0 + (int)threadIdx.x;
    const bool keep = b < nb && !(mask && d.c_done[b] == 0);
    slot_of[threadIdx.x] = keep ? trip[LS_TRIP * d.c_node[b] + LS_SLOT] : -1;
  }
  if ((int)blockIdx.x < nxt + nyt) {
    const bool isx = (int)blockIdx.x < nxt;
    const int rows = isx ? n : M, r0 = (isx ? (int)blockIdx.x : (int)blockIdx.x - nxt) * 64;
    const double *src = isx ? d.b_xfin : d.b_yfin;
    double *dst = isx ? ls.x : ls.y;
    for (int r = wv; r < 64; r += 4)
      if (r0 + r < rows) tile[r][lane] = src[(size_t)(r0 + r) * Bs + b0 + lane];  // (columns up to Bs exist)
    __syncthreads();
    for (int cc = wv; cc < 64; cc += 4) {
      const int s = slot_of[cc];
      if (s >= 0 && r0 + lane < rows) dst[(size_t)s * rows + r0 + lane] = tile[lane][cc];
    }
    return;
  }
  __syncthreads();
  for (int cc = 0; cc < 64; cc++) {
    const int b = b0 + cc;
    if (b >= nb) break;
    const int node = d.c_node[b];
    if (slot_of[cc] < 0) {  // unfinished
      if (threadIdx.x == 0) {
        LsRec g;
        g.status = LS_UNFINISHED;
        g.iter = d.c_iter[b];
        g.int_inf = g.nextvar = -1;
        g.node = node;
        g.crossed = 0;
        g.pad[0] = g.pad[1] = 0;
        g.lower = g.hviol = g.hobj = g.pad2 = 0.0;
        rec[node] = g;
      }
      continue;
    }
    const int *tr = trip + LS_TRIP * node;
    const size_t s = (size_t)tr[LS_SLOT], c0 = (size_t)tr[LS_CHILD0], c1 = (size_t)tr[LS_CHILD1];
    const int intinf = d.c_intinf[b], nv = d.c_nextvar[b];
    int crossed = 0;
    if (intinf > 0 && nv >= 0) {
      const double xv = d.b_xfin[(size_t)d.i_idx[nv] * Bs + b];
      const double dn = floor(xv), up = ceil(xv);
      for (int k = threadIdx.x; k < p; k += 256) {
        const double lo = ls.lo[s * p + k], hi = ls.hi[s * p + k];
        ls.lo[c0 * p + k] = lo;
        ls.hi[c0 * p + k] = k == nv ? dn : hi;
        ls.lo[c1 * p + k] = k == nv ? up : lo;
        ls.hi[c1 * p + k] = hi;
        if (k == nv) crossed = lo > dn || up > hi;  // one thread sees position nv: it also writes the record
      }
    }
    const bool writer = intinf > 0 && nv >= 0 ? ((int)threadIdx.x == nv % 256) : threadIdx.x == 0;
    if (writer) {
      LsRec g;
      g.status = d.c_status[b];
      g.iter = d.c_iter[b];
      g.int_inf = intinf;
      g.nextvar = nv;
      g.node = node;
      g.crossed = crossed;
      g.pad[0] = g.pad[1] = 0;
      g.lower = d.c_lower[b];
      g.hviol = d.c_hviol[b];
      g.hobj = d.c_hobj[b];
      g.pad2 = 0.0;
      rec[node] = g;
    }
  }
}

namespace {

struct AheadCols {
  int cap = 0;
  int *d_mand = nullptr;  // one device allocation: the flags of a wave's columns | the count of kls_need
  int *h_mand = nullptr;  // pinned: the flags | the count
  miosqp::lockstep::Ahead logic;
  std::vector<miosqp::lockstep::AheadColumn> cols;
  std::vector<miosqp::lockstep::AheadOutcome> out;
  std::vector<int> pair_slot, pair_rounded, touched;  // per tree: the LAST incumbent of the wave; the trees that have one
};

void ahead_free(void *p) {
  AheadCols *A = static_cast<AheadCols *>(p);
  if (!A) return;
  if (A->d_mand) hipFree(A->d_mand);
  if (A->h_mand) hipHostFree(A->h_mand);
  delete A;
}

void launch_ls_need(miosqp_qp_engine *e, const LsNeed &need, int B) {
  hipLaunchKernelGGL(kls_need<0>, dim3(1), dim3(256), 0, e->stream, e->d, need.mand, need.d_left, B);
}

int ahead_reserve(miosqp_qp_engine *e, AheadCols &A, int cols) {
  if (cols <= A.cap) return 0;
  HIPCHK(hipStreamSynchronize(e->stream));
  if (A.d_mand) hipFree(A.d_mand);
  if (A.h_mand) hipHostFree(A.h_mand);
  A.d_mand = A.h_mand = nullptr;
  A.cap = 0;
  if (hipMalloc((void **)&A.d_mand, ((size_t)cols + 1) * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    A.d_mand = nullptr;
    g_err = "solve_trees_lockstep_ahead: no device memory for the wave's flags";
    return MIOSQP_EFULL;
  }
  HIPCHK(hipHostMalloc((void **)&A.h_mand, ((size_t)cols + 1) * sizeof(int), hipHostMallocDefault));
  A.cap = cols;
  return 0;
}

// the body of miosqp_qp_solve_trees_lockstep_ahead: lockstep_trees_run (host_lockstep.inc) without round and fix, the
// wave planned and settled by lockstep_ahead.hpp
int lockstep_ahead_run(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u, const double *x0,
                       const double *y0, const double *upper0, const double *x_inc0, int32_t tree_explor_rule,
                       int32_t max_iter_bb, int32_t capacity, int32_t ahead, double *x_out, miosqp_tree_info *info,
                       miosqp_lockstep_stats *stats, miosqp_lockstep_ahead_stats *as) {
  using miosqp::lockstep::AheadColumn;
  using miosqp::lockstep::AheadEvent;
  using miosqp::lockstep::AheadOutcome;
  using miosqp::lockstep::Tree;
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || !stats || !as || max_iter_bb < 1 ||
      tree_explor_rule < 0 || tree_explor_rule > 3 || capacity < 0)
    return MIOSQP_EARG;
  if (ahead < 1) {
    g_err = "solve_trees_lockstep_ahead: ahead must be at least 1";
    return MIOSQP_EARG;
  }
  ENTER(e);
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = "solve_trees_lockstep_ahead: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->pool_pending) {
    g_err = "solve_trees_lockstep_ahead: streaming chunks are still in flight (pool_collect first)";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M, m = (size_t)e->d.m_orig, p = (size_t)e->d.n_int;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) {  // (nothing has been queued)
      g_err = "solve_trees_lockstep_ahead: l > u in the root of instance " + std::to_string(k / M);
      return MIOSQP_EBOUNDS;
    }
  stats->waves = stats->max_width = stats->grown = 0;
  stats->nodes = stats->iters_slowest = stats->iters_all = 0;
  stats->device_time = stats->run_time = stats->host_time = 0.0;
  as->waves = 0;
  as->columns = as->sent = as->hits = as->discarded = as->called_off = 0;
  as->hit_iters = as->discarded_iters = as->called_off_iters = 0;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  if (!e->lockstep) e->lockstep = new LockstepStore();
  LockstepStore &L = *static_cast<LockstepStore *>(e->lockstep);
  const int Bw = B + 64;  // a wave holds its mandatory columns and less than one tile of ahead columns
  if (int rc = lockstep_reserve(e, L, Bw)) return rc;
  if (!L.ahead) L.ahead = new AheadCols();
  AheadCols &A = *static_cast<AheadCols *>(L.ahead);
  if (int rc = ahead_reserve(e, A, Bw)) return rc;
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
  A.logic.reset(L.cap, B);
  A.pair_slot.assign((size_t)B, -1);
  A.pair_rounded.assign((size_t)B, 0);
  // ---- the roots: bounds, costs and incumbents per instance; tree b's root is slot b (as lockstep_trees_run sends them) ----
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
    hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, d, L.dev.qraw,
                       const_cast<double *>(L.dev.qs), B);
  }
  std::vector<int> live;
  live.reserve((size_t)B);
  int *h_left = A.h_mand + A.cap, *d_left = A.d_mand + A.cap;
  // ---- the waves ----
  double host_s = 0.0;
  for (;;) {
    double th = wall();
    live.clear();
    for (int b = 0; b < B; b++)
      if (L.trees[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    const int W0 = (int)live.size();
    // the mandatory columns are sliced at max_batch as miosqp_qp_solve_trees_lockstep slices them; the last slice launches
    // whole tiles anyway: what they hold beyond its mandatory columns is free (64 ceil(L / 64) - L columns when max_batch
    // is a multiple of 64).  No tile is launched that the mandatory columns alone would not launch.
    const int last0 = ((W0 - 1) / e->Bcap) * e->Bcap, nbl = W0 - last0;
    const int room = std::min(64 * ((nbl + 63) / 64), e->Bcap) - nbl;
    const int free_cols = ahead > 1 ? room : 0;
    while (L.slots.free_count() < 2 * (size_t)(W0 + free_cols)) {  // two child slots per column sent
      const int keep = L.cap;
      if (int rc = lockstep_slots(e, L, 2 * L.cap, keep)) return rc;
      L.slots.grow(L.cap);
      A.logic.grow(L.cap);
      stats->grown++;
    }
    A.logic.plan(L.slots, L.trees, live, tree_explor_rule, ahead, free_cols, A.cols);
    const int W = (int)A.cols.size();
    for (int c = 0; c < W; c++) {
      const AheadColumn &col = A.cols[(size_t)c];
      int *tr = L.h_trip + LS_TRIP * c;
      tr[LS_TREE] = col.tree;
      tr[LS_SLOT] = col.slot;
      tr[LS_WARM] = col.warm;
      tr[LS_CHILD0] = col.c0;
      tr[LS_CHILD1] = col.c1;
      A.h_mand[c] = col.mandatory ? 1 : 0;
    }
    host_s += wall() - th;
    int need_chunks = -1;  // of the slice that carries ahead columns: the chunks it ran
    for (int s0 = 0; s0 < W0; s0 += e->Bcap) {
      const int nb = s0 == last0 ? W - s0 : e->Bcap;
      const int ntiles = (nb + 63) / 64;
      if (int rc = slice_begin(e, nb)) return rc;
      if (s0 == 0) {  // the wave's one upload (behind slice_begin, as solve_slice queues its own)
        HIPCHK(hipMemcpyAsync(L.d_trip, L.h_trip, sizeof(int) * LS_TRIP * (size_t)W, hipMemcpyHostToDevice, e->stream));
        if (W > W0) HIPCHK(hipMemcpyAsync(A.d_mand, A.h_mand, sizeof(int) * (size_t)W, hipMemcpyHostToDevice, e->stream));
      }
      const int *trip = L.d_trip + LS_TRIP * s0;
      const int big = (int)(n > M ? n : M);
      hipLaunchKernelGGL(kls_gather<0>, dim3((big + 255) / 256, nb), dim3(256), 0, e->stream, d, L.dev, trip, nb);
      const LsRoots roots{L.dev.root_l, L.dev.root_u, trip, nb};
      const dim3 sgrid((int)((n + 63) / 64 + (M + 63) / 64) + 1, ntiles);
      if (s0 == last0 && W > W0) {
        LsNeed need{A.d_mand + s0, d_left, h_left, 0, false};
        if (int rc = slice_run(e, nb, e->st.max_iter, &roots, &need)) return rc;
        hipLaunchKernelGGL(kls_scatter_ahead<0>, sgrid, dim3(256), 0, e->stream, d, L.dev, trip, L.d_rec + s0, nb, need.cut ? 1 : 0);
        need_chunks = need.chunks;
      } else {  // a slice of mandatory columns only: the launches of miosqp_qp_solve_trees_lockstep
        if (int rc = slice_run(e, nb, e->st.max_iter, &roots)) return rc;
        hipLaunchKernelGGL(kls_scatter<0>, sgrid, dim3(256), 0, e->stream, d, L.dev, trip, L.d_rec + s0, nb);
      }
    }
    HIPCHK(hipMemcpyAsync(L.h_rec, L.d_rec, sizeof(LsRec) * (size_t)W, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    // ---- the records: stored or absorbed, per tree (lockstep_ahead.hpp) ----
    th = wall();
    const int wave = ++stats->waves;
    int it_max = 0;
    int64_t it_sum = 0;
    A.out.resize((size_t)W);
    for (int c = 0; c < W; c++) {
      const LsRec &g = L.h_rec[c];
      AheadOutcome &o = A.out[(size_t)c];
      o.finished = g.status != LS_UNFINISHED;
      o.crossed = g.crossed != 0;
      o.r.ok = g.status == MIOSQP_QP_SOLVED || g.status == MIOSQP_QP_MAX_ITER_REACHED;
      o.r.iter = g.iter;
      o.r.lower = g.lower;
      o.r.int_inf = g.int_inf;
      o.r.nextvar = g.nextvar;
      o.r.heur_feasible = g.hviol <= 0.0;
      o.r.heur_obj = g.hobj;
      if (c < W0) {
        it_max = g.iter > it_max ? g.iter : it_max;
        it_sum += g.iter;
        if (!o.finished) {  // (kls_need counts every mandatory column: the loop cannot have ended before it was decided)
          g_err = "solve_trees_lockstep_ahead: a mandatory column came back unfinished (instance " + std::to_string(A.cols[(size_t)c].tree) + ")";
          return MIOSQP_EHIP;
        }
      }
    }
    A.touched.clear();
    int bad = -1;
    const bool ok = A.logic.settle(L.slots, L.trees, A.cols, A.out, tree_explor_rule, max_iter_bb, wave, [&](const AheadEvent &ev) {
      if (ev.v.branch && ev.crossed) {
        bad = ev.tree;
        return false;
      }
      if (ev.v.incumbent) {  // several absorbs of a tree may each improve: the blocks of kls_incumbent run in parallel, so only the LAST goes
        if (A.pair_slot[(size_t)ev.tree] < 0) A.touched.push_back(ev.tree);
        A.pair_slot[(size_t)ev.tree] = ev.slot;
        A.pair_rounded[(size_t)ev.tree] = ev.v.incumbent == 2;
      }
      return true;
    });
    if (!ok) {
      for (int b : A.touched) A.pair_slot[(size_t)b] = -1;
      g_err = "solve_trees_lockstep_ahead: branching produced l > u (instance " + std::to_string(bad) + ")";
      return MIOSQP_EBOUNDS;
    }
    int npairs = 0;
    for (int b : A.touched) {
      int *pr = L.h_pairs + 3 * npairs++;
      pr[0] = b;
      pr[1] = A.pair_slot[(size_t)b];
      pr[2] = A.pair_rounded[(size_t)b];
      A.pair_slot[(size_t)b] = -1;
    }
    host_s += wall() - th;
    if (npairs > 0) {  // (a freed slot keeps its x until the next wave's scatter, which is queued behind this launch)
      HIPCHK(hipMemcpyAsync(L.d_pairs, L.h_pairs, sizeof(int) * 3 * (size_t)npairs, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(kls_incumbent<0>, dim3(npairs), dim3(256), 0, e->stream, d, L.dev, L.d_pairs, npairs);
    }
    stats->max_width = W > stats->max_width ? W : stats->max_width;
    stats->iters_slowest += it_max;
    as->columns += W;
    // chunks: what the slowest slice ran -- counted where kls_need ended the loop, ceil(iterations / check_termination)
    // of the slowest column elsewhere (a slice of mandatory columns runs exactly that; the tail at max_iter is one chunk)
    const int chunks_mand = (it_max + e->chunk - 1) / e->chunk;
    const int chunks = need_chunks > chunks_mand ? need_chunks : chunks_mand;
    if (wave <= stats->wave_cap) {
      if (stats->wave_width) stats->wave_width[wave - 1] = W;
      if (stats->wave_iter_max) stats->wave_iter_max[wave - 1] = it_max;
      if (stats->wave_iter_mean) stats->wave_iter_mean[wave - 1] = (double)it_sum / W0;
    }
    if (wave <= as->wave_cap) {
      if (as->wave_width) as->wave_width[wave - 1] = W;
      if (as->wave_iter_mandatory) as->wave_iter_mandatory[wave - 1] = it_max;
      if (as->wave_chunks) as->wave_chunks[wave - 1] = chunks;
    }
  }
  A.logic.finish(L.slots);  // the records nobody reached
  // ---- the incumbents ----
  double *h_inc = L.stage.data();
  HIPCHK(hipMemcpyAsync(h_inc, L.dev.inc, sizeof(double) * (size_t)B * n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  int64_t iters_total = 0;
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
    stats->nodes += T.nodes;
    iters_total += T.iters;
  }
  const miosqp::lockstep::AheadCounts &cn = A.logic.n;
  stats->iters_all = iters_total;  // (absorbed nodes only: what info[b].osqp_iter sums to)
  as->waves = stats->waves;
  as->sent = cn.sent;
  as->hits = cn.hits;
  as->discarded = cn.discarded;
  as->called_off = cn.called_off;
  as->hit_iters = cn.hit_iters;
  as->discarded_iters = cn.discarded_iters;
  as->called_off_iters = cn.called_off_iters;
  as->free_slots = (int32_t)L.slots.free_count();
  as->slot_cap = (int32_t)L.slots.cap;
  stats->device_time = 1e-3 * ms;
  stats->run_time = wall_s;
  stats->host_time = host_s;
  e->loop_ms += ms;
  e->loop_iters += iters_total;
  return 0;
}

}  // namespace

extern "C" {

int miosqp_qp_solve_trees_lockstep_ahead(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                         const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                         int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t ahead,
                                         double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                         miosqp_lockstep_ahead_stats *ahead_stats) {
  return lockstep_ahead_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, ahead, x_out, info,
                            stats, ahead_stats);
}

}  // extern "C"
