// Derived batches: from ONE uploaded parent node (par = l | u | x | y, 3M + n doubles) B nodes that differ from it in
// a few bounds are built on the device, solved by the lock-step batch path (slice_run) with an iteration cap, and
// judged on the device from what the batch epilogue leaves behind.  Only a small record comes back to the host; the
// nodes' iterates stay where they are.  Two users, each with its own builder and its own judge:
//   strong branching (miosqp_qp_strong_branch): the 2K children of K candidate positions, scored;
//   round and fix (miosqp_qp_round_and_fix): K rounded-and-fixed copies, the best feasible one picked.

// Row j of derived node b (of B) into the batch's node-major staging, the layout kb_prepare and kb_finish read:
// l[B][M] | u[B][M] | x0[B][n] | y0[B][M].  lo, hi: the parent's bounds of row j as the builder edited them (unused
// for j >= M); x and y are the parent's.  Called by every thread of a (ceil(max(M, n) / 256), B) grid.
__device__ __forceinline__ void derived_put(const Dev &d, const double *par, size_t B, int b, int j, double lo,
                                            double hi) {
  const size_t M = d.M, n = d.n;
  const double *px = par + 2 * M, *py = px + n;
  double *rl = d.b_raw, *ru = rl + B * M, *rx = ru + B * M, *ry = rx + B * n;
  if (j < d.M) {
    rl[(size_t)b * M + j] = lo;
    ru[(size_t)b * M + j] = hi;
    ry[(size_t)b * M + j] = py[j];
  }
  if (j < d.n) rx[(size_t)b * n + j] = px[j];
}

// After the batch epilogue (kb_obj_sum): batch column t -> the derived node it holds (c_node, after compaction); the
// node's status and iteration count go into the record's arrays.  has_x: the status comes with an x (SOLVED or
// MAX_ITER_REACHED).
__device__ __forceinline__ int derived_node(const Dev &d, int t, int *status, int *iter, bool &has_x) {
  const int b = d.c_node[t];
  const int st = d.c_status[t];
  status[b] = st;
  iter[b] = d.c_iter[t];
  has_x = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
  return b;
}

// ---- strong branching: candidate k's down child (u of its integer row = floor x) and up child (l = ceil x), as
// Workspace.add_left / add_right build them

#define SB_MAX_K 32

// what comes back: per child (node order: K down children, then K up children) and per candidate
struct SbRec {
  double lower[2 * SB_MAX_K];  // objective at the clamped x (NaN for an infeasible child)
  double score[SB_MAX_K];
  int status[2 * SB_MAX_K];
  int iter[2 * SB_MAX_K];
  int chosen, pad[3];
};

// grid (ceil(max(M, n) / 256), 2K)
__global__ __launch_bounds__(256) void k_sb_children(Dev d, const double *par, const int *cand, int K) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  double lo = 0.0, hi = 0.0;
  if (j < d.M) {
    lo = par[j];
    hi = par[d.M + j];
    const int c = cand[b < K ? b : b - K];
    if (j == d.m_orig + c) {
      const double v = par[2 * (size_t)d.M + d.i_idx[c]];
      if (b < K) hi = floor(v);
      else lo = ceil(v);
    }
  }
  derived_put(d, par, 2 * (size_t)K, b, j, lo, hi);
}

// per child status / iterations / lower from its column, per candidate score = max(gain_down, eps) * max(gain_up, eps)
// with gain = max(L_child - L_parent, 0), or 1e30 for a child without a lower value (infeasible), and the argmax with
// ties to the lowest candidate.  One wave.
__global__ __launch_bounds__(64) void k_sb_score(Dev d, SbRec *rec, int K, double parent_lower, double eps) {
  __shared__ double lo[2 * SB_MAX_K], sc[SB_MAX_K];
  __shared__ int ok[2 * SB_MAX_K];
  const int t = threadIdx.x;
  if (t < 2 * K) {
    bool has_x;
    const int b = derived_node(d, t, rec->status, rec->iter, has_x);
    rec->lower[b] = d.c_lower[t];
    lo[b] = d.c_lower[t];
    ok[b] = has_x;
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

// ---- round and fix: candidate k fixes every integer row to min(max(floor(x_i + theta_k), l), u) with
// theta_k = (k + 1) / (K + 1); judged by the rounded point's objective (c_hobj) and its worst violation of the ROOT's
// linear constraints (c_hviol)

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

// grid (ceil(max(M, n) / 256), K)
__global__ __launch_bounds__(256) void k_rf_candidates(Dev d, const double *par, int K) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  double lo = 0.0, hi = 0.0;
  if (j < d.M) {
    lo = par[j];
    hi = par[d.M + j];
    if (j >= d.m_orig) {
      const double theta = (double)(b + 1) / (double)(K + 1);
      lo = hi = fmin(fmax(floor(par[2 * (size_t)d.M + d.i_idx[j - d.m_orig]] + theta), lo), hi);
    }
  }
  derived_put(d, par, (size_t)K, b, j, lo, hi);
}

// per candidate status / iterations / c_hobj / c_hviol from its column.  A candidate counts when it has an x, its
// rounded point keeps the root's constraints (viol <= 0) and its objective is below `upper`; the argmin of the
// objective over those, ties to the lowest k.  One wave.
__global__ __launch_bounds__(64) void k_rf_pick(Dev d, RfRec *rec, int K, double upper) {
  __shared__ double ob[RF_MAX_K];
  __shared__ int feas[RF_MAX_K], colof[RF_MAX_K];
  const int t = threadIdx.x;
  if (t < K) {
    bool has_x;
    const int b = derived_node(d, t, rec->status, rec->iter, has_x);
    const double o = d.c_hobj[t], v = d.c_hviol[t];
    rec->obj[b] = o;
    rec->viol[b] = v;
    ob[b] = o;
    feas[b] = has_x && v <= 0.0;
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
