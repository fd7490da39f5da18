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
// This file owns the wave loop of this driver -- planning, the last slice with LsNeed and kls_scatter_ahead, settle, the
// choice of the one incumbent per tree that goes up -- and its counters; checks, store, roots, slot growth, the record's
// conversion, the incumbent push, the per-wave statistics and the end of the call are the pieces of host_lockstep.inc.
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

}  // namespace

extern "C" {

// the plain driver's call (the pieces of host_lockstep.inc) around a wave loop of its own: the wave is planned and
// settled by lockstep_ahead.hpp, and its last slice ends with its mandatory columns
int miosqp_qp_solve_trees_lockstep_ahead(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                         const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                         int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t ahead,
                                         double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                         miosqp_lockstep_ahead_stats *as) {
  using miosqp::lockstep::AheadColumn;
  using miosqp::lockstep::AheadEvent;
  using miosqp::lockstep::AheadOutcome;
  using miosqp::lockstep::Tree;
  const LsCall a{"solve_trees_lockstep_ahead", e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, x_out, info};
  if (!ls_args_ok(a) || !stats || !as) return MIOSQP_EARG;
  if (ahead < 1) {
    g_err = "solve_trees_lockstep_ahead: ahead must be at least 1";
    return MIOSQP_EARG;
  }
  ENTER(e);
  if (int rc = ls_refuse(a)) return rc;
  ls_stats_zero(stats);
  as->waves = 0;
  as->columns = as->sent = as->hits = as->discarded = as->called_off = 0;
  as->hit_iters = as->discarded_iters = as->called_off_iters = 0;
  const int Bw = B + 64;  // a wave holds its mandatory columns and less than one tile of ahead columns
  LockstepStore *Lp = nullptr;
  if (int rc = ls_open(a, Bw, &Lp, &stats->grown)) return rc;
  LockstepStore &L = *Lp;
  if (!L.ahead) L.ahead = new AheadCols();
  AheadCols &A = *static_cast<AheadCols *>(L.ahead);
  if (int rc = ahead_reserve(e, A, Bw)) return rc;
  const double t0 = wall();
  PqScope scope(e);
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M;
  if (int rc = ls_upload_roots(a, L)) return rc;
  A.logic.reset(L.cap, B);
  A.pair_slot.assign((size_t)B, -1);
  A.pair_rounded.assign((size_t)B, 0);
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
    int rc = 0;
    if (ls_room(e, L, 2 * (size_t)(W0 + free_cols), &stats->grown, &rc)) A.logic.grow(L.cap);  // two child slots per column sent
    if (rc) return rc;
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
      if ((rc = slice_begin(e, nb)) != 0) return rc;
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
        if ((rc = slice_run(e, nb, e->st.max_iter, &roots, &need)) != 0) return rc;
        hipLaunchKernelGGL(kls_scatter_ahead<0>, sgrid, dim3(256), 0, e->stream, d, L.dev, trip, L.d_rec + s0, nb, need.cut ? 1 : 0);
        need_chunks = need.chunks;
      } else {  // a slice of mandatory columns only: the launches of miosqp_qp_solve_trees_lockstep
        if ((rc = slice_run(e, nb, e->st.max_iter, &roots)) != 0) return rc;
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
      o.r = ls_record(g);
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
      return ls_crossed(a, bad);
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
    // (a freed slot keeps its x until the next wave's scatter, which is queued behind this launch)
    if ((rc = ls_push_incumbents(e, d, L.dev, L.d_pairs, L.h_pairs, npairs)) != 0) return rc;
    ls_stats_wave(stats, wave, W, it_max, it_sum, W0);  // (the iteration figures are the mandatory columns')
    as->columns += W;
    // chunks: what the slowest slice ran -- counted where kls_need ended the loop, ceil(iterations / check_termination)
    // of the slowest column elsewhere (a slice of mandatory columns runs exactly that; the tail at max_iter is one chunk)
    const int chunks_mand = (it_max + e->chunk - 1) / e->chunk;
    const int chunks = need_chunks > chunks_mand ? need_chunks : chunks_mand;
    if (wave <= as->wave_cap) {
      if (as->wave_width) as->wave_width[wave - 1] = W;
      if (as->wave_iter_mandatory) as->wave_iter_mandatory[wave - 1] = it_max;
      if (as->wave_chunks) as->wave_chunks[wave - 1] = chunks;
    }
  }
  A.logic.finish(L.slots);  // the records nobody reached
  if (int rc = ls_finish(a, L, t0, host_s, stats)) return rc;
  // nodes and iterations are the absorbed nodes', not the columns sent: what info[b] sums to
  stats->nodes = stats->iters_all = 0;
  for (int b = 0; b < B; b++) {
    stats->nodes += L.trees[(size_t)b].nodes;
    stats->iters_all += L.trees[(size_t)b].iters;
  }
  const miosqp::lockstep::AheadCounts &cn = A.logic.n;
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
  return 0;
}

}  // extern "C"
