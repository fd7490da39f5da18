// Round and fix (miosqp_qp_round_and_fix): a primal heuristic on the batch path strong branching brought in.  From ONE
// uploaded parent node (l, u, x, y) K candidates are built on the device -- candidate k fixes every integer row to
// min(max(floor(x_i + theta_k), l), u) with theta_k = (k + 1) / (K + 1) --, solved in lock step by slice_run, and judged
// from what the batch epilogue leaves behind: the rounded point's objective (c_hobj) and its worst violation of the
// ROOT's linear constraints (c_hviol).  Only the small RfRec and the winner's x come back to the host.

#define RF_MAX_K 32

// what comes back, per candidate; the winner's rounded x (n doubles) follows the record in the same allocation
struct RfRec {
  double obj[RF_MAX_K];   // objective of the rounded point (NaN without one: infeasible candidate)
  double viol[RF_MAX_K];  // its worst violation of the root bounds, eps_abs slack included: <= 0 is feasible
  int status[RF_MAX_K];
  int iter[RF_MAX_K];
  int chosen;    // the candidate that counts with the lowest objective (ties to the lowest k), -1 when none counts
  int feasible;  // candidates with a status that has an x and viol <= 0
  int col;       // the batch column that holds the winner
  int pad;
};
#define RF_REC_DOUBLES ((sizeof(RfRec) + 7) / 8)

// the candidates straight into the batch's node-major staging, the layout kb_prepare and kb_finish read:
// l[B][M] | u[B][M] | x0[B][n] | y0[B][M] with B = K.  par = l | u | x | y of the parent (3M + n doubles).
// grid (ceil(max(M, n) / 256), K)
__global__ __launch_bounds__(256) void k_rf_candidates(Dev d, const double *par, int K) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const size_t B = (size_t)K, M = d.M, n = d.n;
  const double *pl = par, *pu = pl + M, *px = pu + M, *py = px + n;
  double *rl = d.b_raw, *ru = rl + B * M, *rx = ru + B * M, *ry = rx + B * n;
  if (j < d.M) {
    double lo = pl[j], hi = pu[j];
    if (j >= d.m_orig) {
      const double theta = (double)(b + 1) / (double)(K + 1);
      const double r = fmin(fmax(floor(px[d.i_idx[j - d.m_orig]] + theta), lo), hi);
      lo = hi = r;
    }
    rl[(size_t)b * M + j] = lo;
    ru[(size_t)b * M + j] = hi;
    ry[(size_t)b * M + j] = py[j];
  }
  if (j < d.n) rx[(size_t)b * n + j] = px[j];
}

// after the batch epilogue (kb_obj_sum): per candidate status / iterations / c_hobj / c_hviol from its column (c_node
// maps a column to the candidate it holds after compaction).  A candidate counts when it has an x (SOLVED or
// MAX_ITER_REACHED), its rounded point keeps the root's constraints (viol <= 0) and its objective is below `upper`;
// the argmin of the objective over those, ties to the lowest k.  One wave.
__global__ __launch_bounds__(64) void k_rf_pick(Dev d, RfRec *rec, int K, double upper) {
  __shared__ double ob[RF_MAX_K];
  __shared__ int feas[RF_MAX_K], colof[RF_MAX_K];
  const int t = threadIdx.x;
  if (t < K) {
    const int b = d.c_node[t];
    const int st = d.c_status[t];
    const double o = d.c_hobj[t], v = d.c_hviol[t];
    rec->status[b] = st;
    rec->iter[b] = d.c_iter[t];
    rec->obj[b] = o;
    rec->viol[b] = v;
    ob[b] = o;
    feas[b] = (st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED) && v <= 0.0;
    colof[b] = t;
  }
  __syncthreads();
  if (t == 0) {
    int best = -1, nf = 0;
    for (int k = 0; k < K; k++) {
      if (!feas[k]) continue;
      nf++;
      if (ob[k] < upper && (best < 0 || ob[k] < ob[best])) best = k;
    }
    rec->chosen = best;
    rec->feasible = nf;
    rec->col = best < 0 ? -1 : colof[best];
    rec->pad = 0;
  }
}

// the winner's column of b_xi (unscaled; the integer entries are the fixed values, exact) as n contiguous doubles
// behind the record; nothing is written when no candidate counts
__global__ __launch_bounds__(256) void k_rf_gather(Dev d, const RfRec *rec, double *x_out) {
  const int col = rec->col;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (col < 0 || j >= d.n) return;
  x_out[j] = d.b_xi[(size_t)j * d.Bs + col];
}
