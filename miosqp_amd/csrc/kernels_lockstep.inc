// part of engine.hip (included there, not compiled alone): the device side of B branch-and-bound trees in lock step
// (host_lockstep.inc, C ABI miosqp_qp_solve_trees_lockstep and, with round and fix, miosqp_qp_solve_trees_lockstep_rf).
// The open leaves of ALL trees are slots of one device store (integer-row bounds lo / hi, solution x / y = the children's
// warm start); every tree has its own root bounds, raw and scaled cost and incumbent.  A wave is the unchanged lock-step batch (slice_run) between kls_gather and kls_scatter.
// The kernels here are copies and row sums over vector loads and stores: no spin wait, no hand-off between workgroups,
// no whole-chip launch.
// They are templates (one instantiation each, LS = 0; kls_heur_rows a second one for the refilled columns at the end of this
// file) for the sake of the code object's layout: a template is emitted where it is first used, and every use is in
// host_lockstep.inc and host_refill.inc, the last files of the translation unit -- so these kernels
// sit behind every other kernel and adding them moves none of those (the exchange loops of the cooperative kernels are
// tuned to a fraction of a microsecond per iteration).

// a column of a wave as the host uploads it: the tree, the node's slot, the slot whose solution warm-starts it, and the
// slots reserved for its two children
constexpr int LS_TRIP = 5;
enum { LS_TREE = 0, LS_SLOT = 1, LS_WARM = 2, LS_CHILD0 = 3, LS_CHILD1 = 4 };

struct LsRec {  // what the host reads back per column, in the order of the wave (64 bytes)
  int status, iter, int_inf, nextvar;
  int node, crossed, pad[2];  // crossed: a child's lo > hi (the host refuses it when it branches there)
  double lower, hviol, hobj, pad2;
};

struct LsDev {
  const double *root_l, *root_u;  // [B][M] the instances' root bounds
  const double *qraw, *qs;        // [B][n] raw costs / as k_scale_q_batch leaves them
  double *inc;                    // [B][n] incumbents
  double *lo, *hi, *x, *y;        // the slot store: [cap][n_int], [cap][n], [cap][M]
};

// what slice_run needs to judge the rounded points against the instances' roots instead of the engine's
struct LsRoots {
  const double *root_l, *root_u;
  const int *trip;  // the slice's columns
  int nb;
};

// node c of the slice into d.b_raw (node-major l | u | x0 | y0, as kb_prepare reads it) and its tree's costs into
// b_qraw / b_qs.  grid (row chunks of 256, nb)
template <int LS>
__global__ __launch_bounds__(256) void kls_gather(Dev d, LsDev ls, const int *__restrict__ trip, int nb) {
  const int c = blockIdx.y;
  if (c >= nb) return;
  const size_t n = d.n, M = d.M, m = d.m_orig, p = d.n_int;
  const size_t t = (size_t)trip[LS_TRIP * c + LS_TREE], s = (size_t)trip[LS_TRIP * c + LS_SLOT],
               w = (size_t)trip[LS_TRIP * c + LS_WARM];
  double *rl = d.b_raw + (size_t)c * M, *ru = d.b_raw + (size_t)nb * M + (size_t)c * M;
  double *rx = d.b_raw + 2 * (size_t)nb * M + (size_t)c * n, *ry = d.b_raw + (size_t)nb * (2 * M + n) + (size_t)c * M;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < M) {
    rl[j] = j < m ? ls.root_l[t * M + j] : ls.lo[s * p + (j - m)];
    ru[j] = j < m ? ls.root_u[t * M + j] : ls.hi[s * p + (j - m)];
    ry[j] = ls.y[w * M + j];
  }
  if (j < n) {
    rx[j] = ls.x[w * n + j];
    d.b_qraw[(size_t)c * n + j] = ls.qraw[t * n + j];
    d.b_qs[(size_t)c * n + j] = ls.qs[t * n + j];
  }
}

// kb_heur_rows with the root rows of the tree each column belongs to (through c_node: compaction swaps columns): the same
// product, the same expression -- for a tree whose root is the engine's, the same bits
template <int LS>
__global__ __launch_bounds__(256) void kls_heur_rows(Dev d, LsRoots r) {
  if constexpr (LS == 1) {  // refilled columns (below): only the tiles with a column harvested at this boundary
    if (!d.t_has[blockIdx.y]) return;
  }
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  const double *root_l = d.root_l, *root_u = d.root_u;
  if (b < r.nb) {  // (positions behind the slice's columns are padding that never moved)
    const size_t t = (size_t)r.trip[LS_TRIP * d.c_node[b] + LS_TREE];
    root_l = r.root_l + t * (size_t)d.M;
    root_u = r.root_u + t * (size_t)d.M;
  }
  const double acc = brow_dot(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_xis + b, Bs);
  const double z = d.Einv[row] * acc;
  d.b_sm[row * Bs + b] = fmax(root_l[row] - d.eps_lin - z, z - root_u[row] - d.eps_lin);
}

// After slice_run: the columns' answers into their slots, the children of fractional nodes into the slots the host
// reserved, and the per-column record in wave order.  grid (tiles of 64 rows of x, then of y, then one block for the
// children and records; tiles of 64 columns).  b_xfin / b_yfin are batch-fastest and the store is slot-major: a tile
// goes through LDS so that both the loads (64 consecutive columns of a row) and the stores (64 consecutive entries of a
// slot) are contiguous.
template <int LS>
__global__ __launch_bounds__(256) void kls_scatter(Dev d, LsDev ls, const int *__restrict__ trip, LsRec *__restrict__ rec, int nb) {
  __shared__ double tile[64][65];
  __shared__ int slot_of[64];
  const int n = d.n, M = d.M, p = d.n_int;
  const int nxt = (n + 63) / 64, nyt = (M + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.y * 64;
  const size_t Bs = (size_t)d.Bs;
  if (threadIdx.x < 64) {
    const int b = b0 + (int)threadIdx.x;
    slot_of[threadIdx.x] = b < nb ? trip[LS_TRIP * d.c_node[b] + LS_SLOT] : -1;
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

// the incumbents the host decided in this wave: (tree, slot, rounded?) per pair.  The node's x, with the integer entries
// rounded when the rounding heuristic found it (workspace.py:266-272).  grid (pairs)
template <int LS>
__global__ __launch_bounds__(256) void kls_incumbent(Dev d, LsDev ls, const int *__restrict__ pairs, int npairs) {
  const int k = blockIdx.x;
  if (k >= npairs) return;
  const size_t n = d.n, t = (size_t)pairs[3 * k], s = (size_t)pairs[3 * k + 1];
  const int rounded = pairs[3 * k + 2];
  for (size_t i = threadIdx.x; i < n; i += 256) ls.inc[t * n + i] = ls.x[s * n + i];
  if (!rounded) return;
  __syncthreads();
  for (int j = threadIdx.x; j < d.n_int; j += 256) {
    const size_t i = (size_t)d.i_idx[j];
    ls.inc[t * n + i] = rint(ls.x[s * n + i]);
  }
}

// ------------------------------------------------------------------------------------------
// Round and fix in the lock-step trees (host_lockstep.inc, C ABI miosqp_qp_solve_trees_lockstep_rf): the trees that fire
// in a wave send K candidates each into ONE more batch, F K columns, sliced like a wave.  A candidate column carries a
// wave's five integers with the tree, the node's slot and -- the warm start is the node's own solution -- that slot again;
// the two child entries hold the candidate's number k and the number of its group (the firing tree's place in the
// batch).  Groups are contiguous in candidate order, k ascending, and K need not divide a slice: a group may begin in one
// slice and end in the next.  Like the kernels above: copies and a short scan over vector loads and stores, one launch
// each, no spin wait, no hand-off between workgroups; templates instantiated from host_lockstep.inc only.
enum { LS_RF_K = 3, LS_RF_GROUP = 4 };

struct LsRfGroup {  // what the host reads back per firing tree (32 bytes)
  int chosen;       // the candidate that counts with the lowest c_hobj (ties to the lowest k), -1 when none counts
  int feasible;     // candidates with a status that has an x and c_hviol <= 0
  int iters;        // ADMM iterations of the K candidates
  int iter_max;     // ... and of the slowest one
  double obj;       // the winner's c_hobj
  double pad;
};

struct LsRfCand {  // a candidate as the batch epilogue leaves it, in candidate order (24 bytes)
  int status, iter;
  double obj, viol;  // c_hobj, c_hviol
};

struct LsRfDev {
  double *x;          // [B][n] per tree: the rounded point of its group's running winner
  LsRfCand *cand;     // [B * RF_MAX_K] the batch's candidates, group after group, k ascending
  LsRfGroup *run[2];  // [B] each: a straddling group's record between its two slices, read in [slice & 1], written in [(slice + 1) & 1]
  LsRfGroup *rec;     // [B] the groups' records as the host reads them
};

// candidate c of the slice into d.b_raw (node-major l | u | x0 | y0, as kb_prepare reads it): kls_gather with every integer
// row fixed to the rounding k_rf_candidates gives it (the same expression on the slot's x, lo, hi; Workspace.round_and_fix,
// rf_roundings of bnb.py) and the node's own x, y as the warm start.  grid (row chunks of 256, nb)
template <int LS>
__global__ __launch_bounds__(256) void kls_rf_gather(Dev d, LsDev ls, const int *__restrict__ trip, int nb, int K) {
  const int c = blockIdx.y;
  if (c >= nb) return;
  const size_t n = d.n, M = d.M, m = d.m_orig, p = d.n_int;
  const size_t t = (size_t)trip[LS_TRIP * c + LS_TREE], s = (size_t)trip[LS_TRIP * c + LS_SLOT];
  const int k = trip[LS_TRIP * c + LS_RF_K];
  double *rl = d.b_raw + (size_t)c * M, *ru = d.b_raw + (size_t)nb * M + (size_t)c * M;
  double *rx = d.b_raw + 2 * (size_t)nb * M + (size_t)c * n, *ry = d.b_raw + (size_t)nb * (2 * M + n) + (size_t)c * M;
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < M) {
    double lo, hi;
    if (j < m) {
      lo = ls.root_l[t * M + j];
      hi = ls.root_u[t * M + j];
    } else {
      lo = ls.lo[s * p + (j - m)];
      hi = ls.hi[s * p + (j - m)];
      const double theta = (double)(k + 1) / (double)(K + 1);
      lo = hi = fmin(fmax(floor(ls.x[s * n + (size_t)d.i_idx[j - m]] + theta), lo), hi);
    }
    rl[j] = lo;
    ru[j] = hi;
    ry[j] = ls.y[s * M + j];
  }
  if (j < n) {
    rx[j] = ls.x[s * n + j];
    d.b_qraw[(size_t)c * n + j] = ls.qraw[t * n + j];
    d.b_qs[(size_t)c * n + j] = ls.qs[t * n + j];
  }
}

// The record of the group candidate `v` of the slice belongs to, once this slice is counted: k_rf_pick's scan over the
// group's candidates in the slice, in ascending k, behind what an earlier slice left (a later candidate replaces the
// winner only when strictly lower: ties stay with the lowest k).  col_of: candidate of the slice -> column (c_node
// inverted).  fresh: the winner is a candidate of this slice.
__device__ __forceinline__ LsRfGroup ls_rf_judge(const Dev &d, const LsRfDev &rf, const int *__restrict__ trip, const int *col_of, int v,
                                                 int nb, int K, int slice, bool &fresh) {
  const int k = trip[LS_TRIP * v + LS_RF_K];
  const int first = v - k;  // where the group's candidate 0 is (negative: in the slice before)
  const int v_lo = first > 0 ? first : 0, v_hi = first + K < nb ? first + K : nb;
  LsRfGroup g;
  g.chosen = -1;
  g.feasible = g.iters = g.iter_max = 0;
  g.obj = g.pad = 0.0;
  if (first < 0) g = rf.run[slice & 1][trip[LS_TRIP * v + LS_RF_GROUP]];
  fresh = false;
  for (int w = v_lo; w < v_hi; w++) {
    const int b = col_of[w], st = d.c_status[b], it = d.c_iter[b];
    g.iters += it;
    g.iter_max = it > g.iter_max ? it : g.iter_max;
    if ((st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED) && d.c_hviol[b] <= 0.0) {
      const double o = d.c_hobj[b];
      g.feasible++;
      if (g.chosen < 0 || o < g.obj) {
        g.chosen = w - first;
        g.obj = o;
        fresh = true;
      }
    }
  }
  return g;
}

// After a slice of candidates (s0: the slice's first candidate in the batch): per candidate its status, iterations, c_hobj
// and c_hviol in candidate order (rf.cand), per group with candidates in the slice its record (rf.rec, and rf.run for the slice that
// may finish it), and the rounded point of a winner found in this slice -- its column of b_xi, unscaled, the integer
// entries the fixed values -- into the tree's row of rf.x.  grid (tiles of 64 rows of x, then one block for the records;
// tiles of 64 columns).  b_xi is batch-fastest and rf.x tree-major: a tile goes through LDS as in kls_scatter, so that the
// loads and the stores are both contiguous.  Every block judges the groups of its own columns (a scan of at most K
// candidates per column): nothing is handed from one workgroup to another.
template <int LS>
__global__ __launch_bounds__(256) void kls_rf_keep(Dev d, LsRfDev rf, const int *__restrict__ trip, int s0, int nb, int K, int slice) {
  __shared__ double tile[64][65];
  __shared__ int col_of[1024];  // (a slice has at most 1024 columns)
  __shared__ int tree_of[64];   // the tree whose winner this column of the tile has just become, or -1
  __shared__ int s_any;
  const int n = d.n, nxt = (n + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.y * 64;
  const size_t Bs = (size_t)d.Bs;
  for (int b = threadIdx.x; b < nb; b += 256) col_of[d.c_node[b]] = b;  // (c_node of the slice's columns: a permutation of 0 .. nb-1)
  __syncthreads();
  if (threadIdx.x < 64) {
    const int b = b0 + (int)threadIdx.x;
    int tree = -1;
    if (b < nb) {
      const int v = d.c_node[b], k = trip[LS_TRIP * v + LS_RF_K];
      bool fresh;
      const LsRfGroup g = ls_rf_judge(d, rf, trip, col_of, v, nb, K, slice, fresh);
      if (fresh && g.chosen == k) tree = trip[LS_TRIP * v + LS_TREE];
      if ((int)blockIdx.x == nxt) {
        LsRfCand cd;  // (through c_node: compaction swaps columns)
        cd.status = d.c_status[b];
        cd.iter = d.c_iter[b];
        cd.obj = d.c_hobj[b];
        cd.viol = d.c_hviol[b];
        rf.cand[s0 + v] = cd;
        if (k == 0 || v == 0) {  // the group's first candidate in the slice writes its record
          const int grp = trip[LS_TRIP * v + LS_RF_GROUP];
          rf.run[(slice + 1) & 1][grp] = g;
          rf.rec[grp] = g;
        }
      }
    }
    tree_of[threadIdx.x] = tree;
    const unsigned long long any = __ballot(tree >= 0);
    if (threadIdx.x == 0) s_any = any != 0ull;
  }
  __syncthreads();
  if ((int)blockIdx.x >= nxt || !s_any) return;
  const int r0 = (int)blockIdx.x * 64;
  for (int r = wv; r < 64; r += 4)
    if (r0 + r < n) tile[r][lane] = d.b_xi[(size_t)(r0 + r) * Bs + b0 + lane];  // (columns up to Bs exist)
  __syncthreads();
  for (int cc = wv; cc < 64; cc += 4) {
    const int t = tree_of[cc];
    if (t >= 0 && r0 + lane < n) rf.x[(size_t)t * n + r0 + lane] = tile[lane][cc];
  }
}

// the winners the host adopted in this wave: the tree's row of rf.x becomes its incumbent (Workspace.primal_heuristic:
// self.x = r.x).  Queued behind kls_incumbent: at a node where both heuristics improve, this one is the later.  grid (trees)
template <int LS>
__global__ __launch_bounds__(256) void kls_rf_incumbent(Dev d, LsDev ls, LsRfDev rf, const int *__restrict__ trees, int nt) {
  const int k = blockIdx.x;
  if (k >= nt) return;
  const size_t n = d.n, t = (size_t)trees[k];
  for (size_t i = threadIdx.x; i < n; i += 256) ls.inc[t * n + i] = rf.x[t * n + i];
}

// ------------------------------------------------------------------------------------------
// Refilled columns (host_refill.inc, C ABI miosqp_qp_solve_trees_refill): the same trees on columns that never wait for a
// wave.  The chunk is the streaming one (Dev.stream = 1: a column counts from c_start and reaches max_iter on its own,
// kb_check_decide); at every chunk boundary the columns the test has just decided are harvested IN PLACE -- the masked
// epilogue kb_finish / kls_heur_rows / kb_obj_rows<true> / kb_obj_sum through c_harv and t_has, the expressions of a wave's
// epilogue -- scattered to their slots with their children and records (kls_scatter_cols), and the columns the host hands
// back are loaded from the store (kls_refill + kls_refill_z: the bits kb_prepare<true> and kb_warm_z give a column of a
// wave).  Decided columns are frozen by the iteration kernels (c_done), so a column nobody refills simply waits.
// Like the kernels above: copies and row sums over vector loads and stores, one launch each, no spin wait, no hand-off
// between workgroups; templates instantiated from host_refill.inc only, behind every other kernel of the code object.

struct RfHead {  // first 64 bytes of what the host reads back per boundary
  int count;     // columns harvested at this boundary (their numbers follow in `list`, in column order)
  int pad;       // Ctrl.pad: the chunk's persistent launch was called off (1) or timed out (> 1)
  int iter;      // Ctrl.iter after the chunk
  int res[13];
};

struct RfDev {
  int *c_trip;             // [Bs][LS_TRIP]: what each column holds, as a wave's triples (kls_heur_rows reads the tree there)
  int *c_slot, *c_tree;    // [Bs] the same slot and tree on their own: c_node of kb_finish (pl_lo / pl_hi) and of kb_obj_rows<true> (b_qraw)
  int *c_ident;            // [Bs] b -> b: c_node of kls_heur_rows
  int *c_busy;             // [Bs] 1: the column holds a node that has not been harvested
  int *c_fill, *t_fill;    // [Bs], [16]: the boundary (epoch) at which the column / a column of the tile was last loaded
  RfHead *head;            // | head | list[Bs] | rec[Bs] |, one device block: ONE download per boundary
  int *list;
  LsRec *rec;
  int C;                   // columns in use (the rest of the last tile is padding: decided, never busy)
};

// before the first fill: every column decided and idle (kb_reset, kb_prepare<true> and kb_warm_z with B = 0 have zeroed the
// working vectors, as a wave zeroes its padding)
template <int LS>
__global__ __launch_bounds__(256) void kls_cols_reset(Dev d, RfDev r) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < d.Bs) {
    for (int k = 0; k < LS_TRIP; k++) r.c_trip[LS_TRIP * b + k] = 0;
    r.c_slot[b] = r.c_tree[b] = 0;
    r.c_ident[b] = b;
    r.c_busy[b] = 0;
    r.c_fill[b] = 0;
    d.c_start[b] = 0;
    d.c_harv[b] = 0;
  }
  if (b < 16) {
    r.t_fill[b] = 0;
    d.t_has[b] = 0;
  }
}

// After the chunk's test: the columns decided in this chunk (busy and done), their list in column order, the masks of
// the epilogue.  One workgroup (<= 1024 columns), the ranks as kp_assign takes them.
template <int LS>
__global__ __launch_bounds__(1024) void kls_harvest(Dev d, RfDev r) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  const bool in = t < d.Bs;
  const bool harv = in && t < r.C && r.c_busy[t] != 0 && d.c_done[t] != 0;
  int total;
  const int rank = block_rank(harv, s_wave, &total);
  if (in) d.c_harv[t] = harv ? 1 : 0;
  if (harv) {
    r.list[rank] = t;
    r.c_busy[t] = 0;
  }
  const unsigned long long m = __ballot(harv);
  if ((t & 63) == 0) d.t_has[t >> 6] = m != 0ull;
  if (t == 0) {
    r.head->count = total;
    r.head->pad = d.ctrl->pad;
    r.head->iter = d.ctrl->iter;
  }
}

// kls_scatter for the harvested columns of the tile: answers into their slots, the children of fractional nodes into the
// slots reserved when the column was filled, the record at the column's number.  grid as kls_scatter.
template <int LS>
__global__ __launch_bounds__(256) void kls_scatter_cols(Dev d, LsDev ls, RfDev rf) {
  __shared__ double tile[64][65];
  __shared__ int slot_of[64];
  if (!d.t_has[blockIdx.y]) return;
  const int n = d.n, M = d.M, p = d.n_int;
  const int nxt = (n + 63) / 64, nyt = (M + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.y * 64;
  const size_t Bs = (size_t)d.Bs;
  if (threadIdx.x < 64) {
    const int b = b0 + (int)threadIdx.x;
    slot_of[threadIdx.x] = d.c_harv[b] ? rf.c_slot[b] : -1;
  }
  if ((int)blockIdx.x < nxt + nyt) {
    const bool isx = (int)blockIdx.x < nxt;
    const int rows = isx ? n : M, r0 = (isx ? (int)blockIdx.x : (int)blockIdx.x - nxt) * 64;
    const double *src = isx ? d.b_xfin : d.b_yfin;
    double *dst = isx ? ls.x : ls.y;
    for (int r = wv; r < 64; r += 4)
      if (r0 + r < rows) tile[r][lane] = src[(size_t)(r0 + r) * Bs + b0 + lane];
    __syncthreads();
    for (int cc = wv; cc < 64; cc += 4) {
      const int s = slot_of[cc];
      if (s >= 0 && r0 + lane < rows) dst[(size_t)s * rows + r0 + lane] = tile[lane][cc];
    }
    return;
  }
  __syncthreads();
  for (int cc = 0; cc < 64; cc++) {
    if (slot_of[cc] < 0) continue;
    const int b = b0 + cc;
    const int *tr = rf.c_trip + LS_TRIP * b;
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
      g.node = b;
      g.crossed = crossed;
      g.pad[0] = g.pad[1] = 0;
      g.lower = d.c_lower[b];
      g.hviol = d.c_hviol[b];
      g.hobj = d.c_hobj[b];
      g.pad2 = 0.0;
      rf.rec[b] = g;
    }
  }
}

// The columns the host filled at this boundary: fills[k] = (column, tree, slot, warm-start slot, child slots).  Bounds,
// warm start and cost from the store into the column's scaled working vectors -- per entry the expressions of
// kb_prepare<true> on what kls_gather would have staged --, then the column's bookkeeping.  grid (tiles of 64 rows of the
// n-vectors, then of the M-vectors, then one block for the bookkeeping; tiles of 64 fills).  The store is slot-major and the
// working set batch-fastest: a tile goes through LDS so that the loads (64 consecutive entries of a slot) and the stores
// (the fills' columns of a row: consecutive while the columns are) are both as contiguous as they can be.
constexpr int RF_FILL = 6;
template <int LS>
__global__ __launch_bounds__(256) void kls_refill(Dev d, LsDev ls, RfDev rf, const int *__restrict__ fills, int nfill, int epoch) {
  __shared__ double tile[64][65];
  __shared__ int s_col[64], s_tree[64], s_slot[64], s_warm[64];
  const int n = d.n, M = d.M, m = d.m_orig, p = d.n_int;
  const int nxt = (n + 63) / 64, nyt = (M + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k0 = blockIdx.y * 64;
  const size_t Bs = (size_t)d.Bs;
  if (threadIdx.x < 64) {
    const int k = k0 + (int)threadIdx.x;
    const bool on = k < nfill;
    s_col[threadIdx.x] = on ? fills[RF_FILL * k] : -1;
    s_tree[threadIdx.x] = on ? fills[RF_FILL * k + 1] : 0;
    s_slot[threadIdx.x] = on ? fills[RF_FILL * k + 2] : 0;
    s_warm[threadIdx.x] = on ? fills[RF_FILL * k + 3] : 0;
  }
  __syncthreads();
  const int mycol = s_col[lane];  // the column of fill `lane` (store phase: lane = fill)
  if ((int)blockIdx.x < nxt) {
    const int r0 = (int)blockIdx.x * 64;
    // x0 = the warm-start slot's solution
    for (int e = wv; e < 64; e += 4)
      if (s_col[e] >= 0 && r0 + lane < n) tile[e][lane] = ls.x[(size_t)s_warm[e] * n + r0 + lane];
    __syncthreads();
    double xs[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int j = r0 + wv + 4 * i;
      xs[i] = 0.0;
      if (mycol >= 0 && j < n) {
        xs[i] = d.Dinv[j] * tile[lane][wv + 4 * i];
        d.b_x[(size_t)j * Bs + mycol] = xs[i];
        d.b_dx[(size_t)j * Bs + mycol] = 0.0;
      }
    }
    __syncthreads();
    // the tree's scaled cost
    for (int e = wv; e < 64; e += 4)
      if (s_col[e] >= 0 && r0 + lane < n) tile[e][lane] = ls.qs[(size_t)s_tree[e] * n + r0 + lane];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int j = r0 + wv + 4 * i;
      if (mycol >= 0 && j < n) {
        const double qs = tile[lane][wv + 4 * i];
        d.b_q[(size_t)j * Bs + mycol] = qs;
        d.b_rx[(size_t)j * Bs + mycol] = d.sigma * xs[i] - qs;
      }
    }
    return;
  }
  if ((int)blockIdx.x < nxt + nyt) {
    const int r0 = ((int)blockIdx.x - nxt) * 64;
    const int j_l = r0 + lane;  // load phase: lane = row
    // l: the tree's root on the general rows, the node's on the integer rows
    for (int e = wv; e < 64; e += 4)
      if (s_col[e] >= 0 && j_l < M)
        tile[e][lane] = j_l < m ? ls.root_l[(size_t)s_tree[e] * M + j_l] : ls.lo[(size_t)s_slot[e] * p + (j_l - m)];
    __syncthreads();
    for (int i = 0; i < 16; i++) {
      const int j = r0 + wv + 4 * i;
      if (mycol >= 0 && j < M) d.b_l[(size_t)j * Bs + mycol] = d.E[j] * fmax(tile[lane][wv + 4 * i], -QP_INFTY);
    }
    __syncthreads();
    for (int e = wv; e < 64; e += 4)
      if (s_col[e] >= 0 && j_l < M)
        tile[e][lane] = j_l < m ? ls.root_u[(size_t)s_tree[e] * M + j_l] : ls.hi[(size_t)s_slot[e] * p + (j_l - m)];
    __syncthreads();
    for (int i = 0; i < 16; i++) {
      const int j = r0 + wv + 4 * i;
      if (mycol >= 0 && j < M) d.b_u[(size_t)j * Bs + mycol] = d.E[j] * fmin(tile[lane][wv + 4 * i], QP_INFTY);
    }
    __syncthreads();
    // y0 = the warm-start slot's multipliers
    for (int e = wv; e < 64; e += 4)
      if (s_col[e] >= 0 && j_l < M) tile[e][lane] = ls.y[(size_t)s_warm[e] * M + j_l];
    __syncthreads();
    for (int i = 0; i < 16; i++) {
      const int j = r0 + wv + 4 * i;
      if (mycol >= 0 && j < M) {
        d.b_y[(size_t)j * Bs + mycol] = d.c * d.Einv[j] * tile[lane][wv + 4 * i];
        d.b_dy[(size_t)j * Bs + mycol] = 0.0;
      }
    }
    return;
  }
  // the bookkeeping: one thread per fill
  if (threadIdx.x < 64 && mycol >= 0) {
    const int k = k0 + lane, b = mycol;
    for (int i = 0; i < LS_TRIP; i++) rf.c_trip[LS_TRIP * b + i] = fills[RF_FILL * k + 1 + i];
    rf.c_tree[b] = s_tree[lane];
    rf.c_slot[b] = s_slot[lane];
    rf.c_busy[b] = 1;
    rf.c_fill[b] = epoch;
    rf.t_fill[b >> 6] = epoch;  // (several fills of a tile store the same value)
    d.c_start[b] = d.ctrl->iter;
    d.c_status[b] = MIOSQP_QP_UNSOLVED;
    d.c_iter[b] = 0;
    d.c_pri[b] = d.c_dua[b] = d.c_obj[b] = 0.0;
    d.c_lower[b] = __builtin_nan("");
    d.c_done[b] = 0;
  }
}

// kb_warm_z for the columns loaded at this boundary: the same row product over the tile, stored where the column was
// just filled (the others are iterating or waiting: their z, wh and rx stay)
template <int LS>
__global__ __launch_bounds__(256) void kls_refill_z(Dev d, RfDev rf, int epoch) {
  if (rf.t_fill[blockIdx.y] != epoch) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  const double z = brow_dot(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_x + b, Bs);
  if (rf.c_fill[b] != epoch) return;
  const size_t o = row * Bs + b;
  const double wh = z - d.rho_inv * d.b_y[o];
  d.b_z[o] = z;
  d.b_wh[whrow(d, row) * Bs + b] = wh;
  if (row >= d.wh_m) {  // a bound row taken out of the products: its share of the right-hand side, r~ = rx + t
    const int i = d.i_idx[row - d.m_orig];
    d.b_rx[(size_t)i * Bs + b] += d.a_int[i] * wh;  // kls_refill wrote rx in the launch before; one row per variable
  }
}
