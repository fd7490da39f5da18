// part of engine.hip (included there, not compiled alone): the device side of B branch-and-bound trees in lock step
// (host_lockstep.inc, C ABI miosqp_qp_solve_trees_lockstep).  The open leaves of ALL trees are slots of one device store
// (integer-row bounds lo / hi, solution x / y = the children's warm start); every tree has its own root bounds, raw and
// scaled cost and incumbent.  A wave is the unchanged lock-step batch (slice_run) between kls_gather and kls_scatter.
// The kernels here are copies and row sums over vector loads and stores: no spin wait, no hand-off between workgroups,
// no whole-chip launch.
// They are templates (one instantiation each, LS = 0) for the sake of the code object's layout: a template is emitted where
// it is first used, and every use is in host_lockstep.inc, the last file of the translation unit -- so the four kernels
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
