// part of engine.hip (included there, not compiled alone): strong and reliability branching in the lock-step trees
// (host_lockstep_sb.inc, C ABI miosqp_qp_solve_trees_lockstep_sb).  The nodes that branch in a wave send the 2K children of
// their K candidate positions into ONE more batch, sliced like a wave.  A child column carries a wave's five integers
// with the tree, the node's slot and -- the warm start is the node's own solution -- that slot again; the two child
// entries hold the candidate's position and the side (0: down, u = floor x; 1: up, l = ceil x).  Like the kernels of
// kernels_lockstep.inc: copies over vector loads and stores, one launch each, no spin wait, no hand-off between
// workgroups; templates instantiated from host_lockstep_sb.inc only, behind every other kernel of the code object.
enum { LS_SB_POS = 3, LS_SB_SIDE = 4 };

struct LsSbChild {  // a child as the batch epilogue leaves it, in the order the host uploaded the columns (16 bytes)
  int status, iter;
  double lower;  // c_lower
};

// The x of the asking nodes at the integer positions, and per position whether a child there would cross its bounds
// (Workspace._child refuses l > u): out[a] = x[i_idx[0 .. p-1]] | flags[0 .. p-1] (1.0: floor x < lo or ceil x > hi).
// grid (asking nodes)
template <int LS>
__global__ __launch_bounds__(256) void kls_sb_xint(Dev d, LsDev ls, const int *__restrict__ slots, int na, double *__restrict__ out) {
  const int a = blockIdx.x;
  if (a >= na) return;
  const size_t n = d.n, p = d.n_int, s = (size_t)slots[a];
  double *o = out + (size_t)a * 2 * p;
  for (size_t k = threadIdx.x; k < p; k += 256) {
    const double xv = ls.x[s * n + (size_t)d.i_idx[k]];
    o[k] = xv;
    o[p + k] = (ls.lo[s * p + k] > floor(xv) || ceil(xv) > ls.hi[s * p + k]) ? 1.0 : 0.0;
  }
}

// child c of the slice into d.b_raw (node-major l | u | x0 | y0, as kb_prepare reads it): kls_gather with ONE integer row
// changed as k_sb_children changes it (the same expressions on the slot's x: Workspace.add_left / add_right) and the
// node's own x, y as the warm start.  The store is slot-major and the staging node-major: consecutive threads read and
// write consecutive entries of a row block, no transpose is needed.  grid (row chunks of 256, nb)
template <int LS>
__global__ __launch_bounds__(256) void kls_sb_gather(Dev d, LsDev ls, const int *__restrict__ trip, int nb) {
  const int c = blockIdx.y;
  if (c >= nb) return;
  const size_t n = d.n, M = d.M, m = d.m_orig, p = d.n_int;
  const size_t t = (size_t)trip[LS_TRIP * c + LS_TREE], s = (size_t)trip[LS_TRIP * c + LS_SLOT];
  const size_t pos = (size_t)trip[LS_TRIP * c + LS_SB_POS];
  const int side = trip[LS_TRIP * c + LS_SB_SIDE];
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
      if (j - m == pos) {
        const double v = ls.x[s * n + (size_t)d.i_idx[pos]];
        if (side == 0) hi = floor(v);
        else lo = ceil(v);
      }
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

// After a slice of children: status, iterations and objective per child in upload order (through c_node: compaction
// swaps columns).  rec: the slice's first child.  grid (chunks of 256 columns)
template <int LS>
__global__ __launch_bounds__(256) void kls_sb_judge(Dev d, LsSbChild *__restrict__ rec, int nb) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  LsSbChild g;
  g.status = d.c_status[b];
  g.iter = d.c_iter[b];
  g.lower = d.c_lower[b];
  rec[d.c_node[b]] = g;
}

// The children of the nodes that branch, on the position the host chose: quad = (node slot, child slots c0, c1, position).
// Every row of both children is written -- the node's bounds, and on the chosen row floor x / ceil x -- so the row
// kls_scatter changed for the most fractional position is the node's again.  grid (branching nodes)
template <int LS>
__global__ __launch_bounds__(256) void kls_sb_children(Dev d, LsDev ls, const int *__restrict__ quad, int na) {
  const int a = blockIdx.x;
  if (a >= na) return;
  const size_t n = d.n, p = d.n_int;
  const size_t s = (size_t)quad[4 * a], c0 = (size_t)quad[4 * a + 1], c1 = (size_t)quad[4 * a + 2], nv = (size_t)quad[4 * a + 3];
  const double xv = ls.x[s * n + (size_t)d.i_idx[nv]];
  const double dn = floor(xv), up = ceil(xv);
  for (size_t k = threadIdx.x; k < p; k += 256) {
    const double lo = ls.lo[s * p + k], hi = ls.hi[s * p + k];
    ls.lo[c0 * p + k] = lo;
    ls.hi[c0 * p + k] = k == nv ? dn : hi;
    ls.lo[c1 * p + k] = k == nv ? up : lo;
    ls.hi[c1 * p + k] = hi;
  }
}
