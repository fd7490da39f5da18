// Strong branching (miosqp_qp_strong_branch): the 2K children of one parent node -- candidate k's down child
// (u of its integer row = floor x) and up child (l = ceil x), as Workspace.add_left / add_right build them -- are
// built on the device from ONE uploaded parent, solved by the lock-step batch path (slice_run) with an iteration cap,
// and scored on the device.  Only the small SbRec comes back to the host; the children's iterates stay where they are.

#define SB_MAX_K 32

// what comes back: per child (node order: K down children, then K up children) and per candidate
struct SbRec {
  double lower[2 * SB_MAX_K];  // objective at the clamped x (NaN for an infeasible child)
  double score[SB_MAX_K];
  int status[2 * SB_MAX_K];
  int iter[2 * SB_MAX_K];
  int chosen, pad[3];
};

// the children straight into the batch's node-major staging, the layout kb_prepare and kb_finish read:
// l[B][M] | u[B][M] | x0[B][n] | y0[B][M] with B = 2K.  par = l | u | x | y of the parent (3M + n doubles).
// grid (ceil(max(M, n) / 256), 2K)
__global__ __launch_bounds__(256) void k_sb_children(Dev d, const double *par, const int *cand, int K) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const size_t B = 2 * (size_t)K, M = d.M, n = d.n;
  const double *pl = par, *pu = pl + M, *px = pu + M, *py = px + n;
  double *rl = d.b_raw, *ru = rl + B * M, *rx = ru + B * M, *ry = rx + B * n;
  if (j < d.M) {
    double lo = pl[j], hi = pu[j];
    const int k = b < K ? b : b - K;
    const int c = cand[k];
    if (j == d.m_orig + c) {
      const double v = px[d.i_idx[c]];
      if (b < K) hi = floor(v);
      else lo = ceil(v);
    }
    rl[(size_t)b * M + j] = lo;
    ru[(size_t)b * M + j] = hi;
    ry[(size_t)b * M + j] = py[j];
  }
  if (j < d.n) rx[(size_t)b * n + j] = px[j];
}

// after the batch epilogue (kb_obj_sum): per child status / iterations / lower from its column (c_node maps a column
// to the child it holds after compaction), per candidate score = max(gain_down, eps) * max(gain_up, eps) with
// gain = max(L_child - L_parent, 0), or 1e30 for a child without a lower value (infeasible), and the argmax with ties
// to the lowest candidate.  One wave.
__global__ __launch_bounds__(64) void k_sb_score(Dev d, SbRec *rec, int K, double parent_lower, double eps) {
  __shared__ double lo[2 * SB_MAX_K], sc[SB_MAX_K];
  __shared__ int ok[2 * SB_MAX_K];
  const int t = threadIdx.x;
  if (t < 2 * K) {
    const int b = d.c_node[t];
    const int st = d.c_status[t];
    rec->status[b] = st;
    rec->iter[b] = d.c_iter[t];
    rec->lower[b] = d.c_lower[t];
    lo[b] = d.c_lower[t];
    ok[b] = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
  }
  __syncthreads();
  if (t < K) {
    double gd = ok[t] ? lo[t] - parent_lower : 1e30;
    double gu = ok[K + t] ? lo[K + t] - parent_lower : 1e30;
    gd = gd > 0.0 ? gd : 0.0;
    gu = gu > 0.0 ? gu : 0.0;
    const double s = (gd > eps ? gd : eps) * (gu > eps ? gu : eps);
    sc[t] = s;
    rec->score[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    for (int k = 1; k < K; k++)
      if (sc[k] > sc[best]) best = k;
    rec->chosen = best;
  }
}
